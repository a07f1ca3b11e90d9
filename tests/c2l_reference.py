"""numpy restatement of CubedToLatLon for the tests (FV3 fv_grid_utils.F90: c2l_ord4, c2l_ord2; the rotation terms a11 .. a22 of
init_cubed_to_latlon are GridData fields, pace_amd/grid.py).

One rank, storage arrays indexed [i, j, k] with the n_halo-cell halo (Fortran-local index f at storage f + n_halo - 1).  ``u`` / ``v``
must hold valid halo values where the order-4 form reads them (one row / column beyond the sub-domain away from tile edges).
Returns ``ua``, ``va`` on the compute cells, shape (nx, ny, nz)."""
import numpy as np

C1, C2 = 1.125, -0.125


def cubed_to_latlon(u, v, grid, order=4):
    nh, nx, ny, nz = grid.n_halo, grid.nx, grid.ny, grid.nz
    I = slice(nh, nh + nx)
    J = slice(nh, nh + ny)
    dx = grid.dx[:, :, None]
    dy = grid.dy[:, :, None]

    def sh(a, di, dj):
        return a[nh + di : nh + nx + di, nh + dj : nh + ny + dj, :nz]

    # dx / dy weighted two-point form: everywhere for order 2, on the rows / columns next to a tile edge for order 4
    ut = 2.0 * (sh(u, 0, 0) * sh(dx, 0, 0) + sh(u, 0, 1) * sh(dx, 0, 1)) / (sh(dx, 0, 0) + sh(dx, 0, 1))
    vt = 2.0 * (sh(v, 0, 0) * sh(dy, 0, 0) + sh(v, 1, 0) * sh(dy, 1, 0)) / (sh(dy, 0, 0) + sh(dy, 1, 0))
    if order == 4:
        u4 = C2 * (sh(u, 0, -1) + sh(u, 0, 2)) + C1 * (sh(u, 0, 0) + sh(u, 0, 1))
        v4 = C2 * (sh(v, -1, 0) + sh(v, 2, 0)) + C1 * (sh(v, 0, 0) + sh(v, 1, 0))
        inner = np.zeros((nx, ny), dtype=bool)
        inner[(1 if grid.west_edge else 0) : (nx - 1 if grid.east_edge else nx), (1 if grid.south_edge else 0) : (ny - 1 if grid.north_edge else ny)] = True
        ut = np.where(inner[:, :, None], u4, ut)
        vt = np.where(inner[:, :, None], v4, vt)
    elif order != 2:
        raise ValueError(order)
    a11, a12, a21, a22 = (grid.fields[n][I, J, None] for n in ("a11", "a12", "a21", "a22"))
    return a11 * ut + a12 * vt, a21 * ut + a22 * vt
