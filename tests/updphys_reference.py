"""numpy restatement of ApplyPhysicsToDycore (FV3 fv_update_phys: the temperature update and update_dwinds_phys), built from the grid's
corner positions alone -- not from the metric terms pace_amd.grid hands the kernel:

    pt += dt t_dt;   V = u_dt vlon + v_dt vlat at the cell centres (halo cells at their true positions)
    u(i,j) += dt 1/2 (V(i,j-1) + V(i,j)) . e_x(i,j),   v(i,j) += dt 1/2 (V(i-1,j) + V(i,j)) . e_y(i,j)

with, on a face of a tile edge, the averaged vector interpolated along the edge: (1 - w) Vbar_f + w Vbar_f'.  Here the crossing point
x_f of the centres' great circle with the edge is found by bisection (pace_amd.grid takes the intersection of the two planes), and w is
the fraction of the chord x_f -> x_f' at which the face mid-point projects.  ``edge_correction=False`` leaves the plain average on the
tile edges: the negative control of the analytic test.

Arrays are a rank's storage, numpy [i, j(, k)] with the 3-cell halo and the padding row / column / level, as ``Quantity.numpy(r)`` gives them."""
import numpy as np

from pace_amd.grid import _corner_positions

NH = 3


def _unit(v):
    return v / np.sqrt(np.sum(v * v, axis=-1, keepdims=True))


def crossing(c1, c2, pa, pb, iters=80):
    """Where the great circle c1 -> c2 crosses the great circle through pa, pb: bisection on the side of the edge's plane."""
    nrm = np.cross(pa, pb)
    lo, hi = np.zeros(c1.shape[:-1]), np.ones(c1.shape[:-1])
    f_lo = np.sum(c1 * nrm, -1)
    for _ in range(iters):
        mid = 0.5 * (lo + hi)
        f_mid = np.sum(_unit((1.0 - mid)[..., None] * c1 + mid[..., None] * c2) * nrm, -1)
        same = (f_mid > 0) == (f_lo > 0)
        lo, hi = np.where(same, mid, lo), np.where(same, hi, mid)
    t = 0.5 * (lo + hi)
    return _unit((1.0 - t)[..., None] * c1 + t[..., None] * c2)


class Geometry:
    """Centres, unit vectors, face tangents / mid-points and tile-edge weights of one rank, from its corner positions."""

    def __init__(self, part, rank, stretch=None, nh=NH):
        self.part, self.rank, self.nh = part, rank, nh
        self.nx, self.ny, self.n = part.nx, part.ny, part.nx_tile
        self.x0, self.y0 = part.origin(rank)
        P = _corner_positions(part, rank, nh, stretch)
        self.P = P
        A = _unit(P[:-1, :-1] + P[1:, :-1] + P[:-1, 1:] + P[1:, 1:])
        self.A = A
        rxy = np.sqrt(A[..., 0] ** 2 + A[..., 1] ** 2)
        self.lon, self.lat = np.arctan2(A[..., 1], A[..., 0]), np.arctan2(A[..., 2], rxy)
        # east = z x A / |z x A|, north = A x east
        self.vlon = np.stack([-A[..., 1] / rxy, A[..., 0] / rxy, np.zeros_like(rxy)], -1)
        self.vlat = _unit(np.cross(A, self.vlon))
        self.ex = _unit(P[1:, :] - P[:-1, :])  # x-faces (u): [nI-1, nJ, 3]
        self.ey = _unit(P[:, 1:] - P[:, :-1])  # y-faces (v): [nI, nJ-1, 3]
        self.mx = _unit(P[1:, :] + P[:-1, :])
        self.my = _unit(P[:, 1:] + P[:, :-1])
        flags = part.on_tile_edges(rank)
        self.flags = flags
        # tile-edge faces this rank updates: (ii, jj) -> (step along the edge to f', w)
        self.wu, self.wv = {}, {}
        n, nx, ny = self.n, self.nx, self.ny
        for has, jj in ((flags["south"], nh), (flags["north"], nh + ny)):
            if has and n >= 2:
                ii = np.arange(nh - 1, nh + nx + 1)
                g = self.x0 + ii - nh
                ok = (g >= 0) & (g < n)
                x = np.full((len(ii), 3), np.nan)
                x[ok] = crossing(A[ii[ok], jj - 1], A[ii[ok], jj], P[ii[ok], jj], P[ii[ok] + 1, jj])
                for a in range(1, len(ii) - 1):
                    step = 1 if g[a] < n // 2 else -1
                    d = x[a + step] - x[a]
                    self.wu[(int(ii[a]), jj)] = (step, float(np.dot(self.mx[ii[a], jj] - x[a], d) / np.dot(d, d)))
        for has, ii in ((flags["west"], nh), (flags["east"], nh + nx)):
            if has and n >= 2:
                jj = np.arange(nh - 1, nh + ny + 1)
                g = self.y0 + jj - nh
                ok = (g >= 0) & (g < n)
                x = np.full((len(jj), 3), np.nan)
                x[ok] = crossing(A[ii - 1, jj[ok]], A[ii, jj[ok]], P[ii, jj[ok]], P[ii, jj[ok] + 1])
                for a in range(1, len(jj) - 1):
                    step = 1 if g[a] < n // 2 else -1
                    d = x[a + step] - x[a]
                    self.wv[(ii, int(jj[a]))] = (step, float(np.dot(self.my[ii, jj[a]] - x[a], d) / np.dot(d, d)))

    # the faces and cells a rank updates
    @property
    def u_box(self):
        return (slice(self.nh, self.nh + self.nx), slice(self.nh, self.nh + self.ny + 1))

    @property
    def v_box(self):
        return (slice(self.nh, self.nh + self.nx + 1), slice(self.nh, self.nh + self.ny))

    @property
    def c_box(self):
        return (slice(self.nh, self.nh + self.nx), slice(self.nh, self.nh + self.ny))

    def edge_masks(self):
        """Boolean [nI-1, nJ] / [nI, nJ-1] arrays: the updated u / v faces that lie on a tile edge."""
        mu, mv = np.zeros(self.ex.shape[:2], dtype=bool), np.zeros(self.ey.shape[:2], dtype=bool)
        nh, nx, ny = self.nh, self.nx, self.ny
        if self.flags["south"]:
            mu[nh : nh + nx, nh] = True
        if self.flags["north"]:
            mu[nh : nh + nx, nh + ny] = True
        if self.flags["west"]:
            mv[nh, nh : nh + ny] = True
        if self.flags["east"]:
            mv[nh + nx, nh : nh + ny] = True
        return mu, mv


def apply_tendencies(u, v, pt, u_dt, v_dt, t_dt, geo, dt, edge_correction=True):
    """(u, v, pt after the update; mag_u, mag_v, mag_t): the new fields (whole storage, changed on the faces / cells the rank updates only) and,
    on the same faces / cells, the sum of the magnitudes of the terms that were added up -- what a rounding bound scales with."""
    u, v, pt = (np.array(a, dtype=np.float64) for a in (u, v, pt))
    u_dt, v_dt, t_dt = (np.asarray(a, dtype=np.float64) for a in (u_dt, v_dt, t_dt))
    nz = u.shape[2] - 1
    ud, vd = u_dt[:-1, :-1, :nz, None], v_dt[:-1, :-1, :nz, None]
    with np.errstate(invalid="ignore"):
        V = ud * geo.vlon[:, :, None, :] + vd * geo.vlat[:, :, None, :]  # [nI-1, nJ-1, nz, 3]
        M = np.abs(ud) * np.abs(geo.vlon[:, :, None, :]) + np.abs(vd) * np.abs(geo.vlat[:, :, None, :])
        Vu, Mu = np.zeros(geo.ex.shape[:2] + V.shape[2:]), np.zeros(geo.ex.shape[:2] + V.shape[2:])
        Vu[:, 1:-1], Mu[:, 1:-1] = 0.5 * (V[:, :-1] + V[:, 1:]), 0.5 * (M[:, :-1] + M[:, 1:])
        Vv, Mv = np.zeros(geo.ey.shape[:2] + V.shape[2:]), np.zeros(geo.ey.shape[:2] + V.shape[2:])
        Vv[1:-1], Mv[1:-1] = 0.5 * (V[:-1] + V[1:]), 0.5 * (M[:-1] + M[1:])
    Tu, TMu, Tv, TMv = Vu.copy(), Mu.copy(), Vv.copy(), Mv.copy()
    if edge_correction:
        for (ii, jj), (step, w) in geo.wu.items():
            Tu[ii, jj] = (1.0 - w) * Vu[ii, jj] + w * Vu[ii + step, jj]
            TMu[ii, jj] = abs(1.0 - w) * Mu[ii, jj] + abs(w) * Mu[ii + step, jj]
        for (ii, jj), (step, w) in geo.wv.items():
            Tv[ii, jj] = (1.0 - w) * Vv[ii, jj] + w * Vv[ii, jj + step]
            TMv[ii, jj] = abs(1.0 - w) * Mv[ii, jj] + abs(w) * Mv[ii, jj + step]
    ub, vb, cb = geo.u_box, geo.v_box, geo.c_box
    kk = slice(0, nz)
    mag_u = np.abs(u[ub + (kk,)]) + abs(dt) * np.sum(TMu[ub] * np.abs(geo.ex[ub][:, :, None, :]), -1)
    mag_v = np.abs(v[vb + (kk,)]) + abs(dt) * np.sum(TMv[vb] * np.abs(geo.ey[vb][:, :, None, :]), -1)
    mag_t = np.abs(pt[cb + (kk,)]) + abs(dt) * np.abs(t_dt[cb + (kk,)])
    u[ub + (kk,)] += dt * np.sum(Tu[ub] * geo.ex[ub][:, :, None, :], -1)
    v[vb + (kk,)] += dt * np.sum(Tv[vb] * geo.ey[vb][:, :, None, :], -1)
    pt[cb + (kk,)] += dt * t_dt[cb + (kk,)]
    return u, v, pt, mag_u, mag_v, mag_t


def rotation_tendencies(geo, omega):
    """East / north components of omega x r at the cell centres, [nI-1, nJ-1] each (solid-body rotation about the axis ``omega``)."""
    w = np.cross(np.asarray(omega, dtype=np.float64), geo.A)
    return np.sum(w * geo.vlon, -1), np.sum(w * geo.vlat, -1)


def rotation_increments(geo, omega, dt):
    """The exact D-grid increments dt (omega x m_f) . e of the same rotation on the x-faces / y-faces, [nI-1, nJ] / [nI, nJ-1]."""
    om = np.asarray(omega, dtype=np.float64)
    return dt * np.sum(np.cross(om, geo.mx) * geo.ex, -1), dt * np.sum(np.cross(om, geo.my) * geo.ey, -1)
