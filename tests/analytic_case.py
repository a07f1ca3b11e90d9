"""Input builders, exact solutions and checkers of tests/test_analytic_pins.py: the transport, wind and pressure-gradient operators held
against closed-form solutions instead of the oracle, so that an error the oracle and the library share cannot pass.

Ground rule: inputs and expected values come from geometry only -- the corner positions grid.lon / grid.lat (the halo holds the neighbour
tile's true corners), the cell centres lon_agrid / lat_agrid, the sphere radius and closed-form functions of position.  No metric term that
a kernel reads (dx, dy, dxa, sin_sg*, cosa_*, rsin_*, the edge factors, rarea) enters an expected value; area weights the error norms and
nothing else.  The one exception is the Courant number handed to the tracer advection (BellCase), which the operator multiplies back.

The flow is solid-body rotation V(p) = U0 axis x p, U0 = 2 pi a / 12 days, with the stream function psi(p) = -a U0 (p . axis): the area
swept through a face from corner A to corner B in dt is -+ dt (psi(B) - psi(A)), exactly (SIGN_X / SIGN_Y, fixed once by the direction the
flow crosses a face).  Covariant wind components follow from corner positions: the along-edge unit vector is the tangent-projected corner
difference at the face mid-point, the cross-face coordinate direction the tangent-projected central difference of the neighbouring face
mid-points (second order), and on a face that lies on a tile edge the C-grid component is the edge-normal one, V . n.

  pin 1  fxadv        x_area_flux / y_area_flux == dt (psi(B) - psi(A)) on every compute face        (flux_case, flux_errors)
  pin 2  tracer_2d_1l a cosine bell, a Gaussian and a constant carried once round the sphere         (BellCase, oracle_bell)
  pin 3  c_sw, dt2=0  the D-to-C wind conversion against the analytic covariant components           (wind_case, wind_errors)
  pin 4  a2b_ord4     a smooth function from the cell centres to the corners                         (corner_case, corner_errors)
  pin 5a nh_p_grad, p_grad_c  no force on an isentropic atmosphere at rest over terrain                    (resting_state, check_no_force)
  pin 5b remap        layer means linear in pressure stay linear in pressure                         (linear_columns, linear_winds)

and of tests/test_analytic_dynamics.py, on the same rotation with every damping term of d_sw off (DSW_OFF) at a Courant number of 0.1 x 24 / n (dyn_dt):

  pin 6  d_sw         scalars at their departure points, mass fluxes and Courant numbers accumulated     (DswCase.scalar_errors)
  pin 7  d_sw         the wind tendency against -(zeta + f) k x V - grad K by class of faces, and the
                      closed-form kinetic-energy excess of tile-edge corners, 0.5 cot(alpha) Vn Vt       (DswCase.wind_errors, face_classes, edge_ke_excess)
  pin 8  riem_solver3, riem_solver_c   columns held at and relaxed to the hydrostatic thickness of the gas law  (Columns, riem_figures, check_balanced, check_relaxed)
  pin 9  update_dz_d  interface heights at their departure points, no surface velocity over flat ground    (HeightCase)

Edge lengths (pin 7) are great-circle distances of the corners (arc), never dx / dy.

and of tests/test_analytic_damping.py (builders, exact solutions and checkers in tests/damping_case.py, which imports from here):

  pin 10 c_sw         divgd == minus the divergence of rotation + potential flow at the corners                         (damping_case.DivergenceCase)
  pin 11 c_sw, dt2!=0 delpc, ptc, omga at the departure points of the half step; the C-grid wind change against the tendency (damping_case.CswCase)
  pin 12 d_sw         the divergence damping, on against off, against the closed-form damping field                     (damping_case.DivDampCase)
  pin 13 d_sw at rest the del-n chains of delp, pt, q_con, w and the vorticity on a harmonic, per level of the sponge   (damping_case.RestCase)
  pin 14 damping heat d_sw's heat_source == the kinetic energy the one-pass damping takes; del2_cubed on a harmonic; apply_diffusive_heating
                      pointwise against the gas law                                                                     (damping_case.heat_errors, Del2Case, heating_case)
  pin 15 convergence  second order from C24 to C48 wherever the oracle's record shows it: pins 10 and 12 away from the tile edges, pins 13 and 14 at the tile centres

and of tests/test_analytic_steady.py (builders, exact solutions and checkers in tests/steady_case.py, which imports from here):

  pin 16 one acoustic call      isothermal solid-body rotation in gradient-wind balance keeps every prognostic field                     (steady_case.SteadyCase.tendencies)
  pin 17 the call's accumulators  mfxd, mfyd == n_split delp x the exact swept area; cxd, cyd x the upwind area == n_split x the swept area  (steady_case.SteadyCase.accumulator_errors)
  pin 18 step_dynamics          two model steps with remap, tracers, temperature bookends and latlon winds return the closed-form state  (steady_case.StepCase)
  pin 19 rest over terrain      three acoustic calls leave the isothermal atmosphere at rest over a 3 km mountain at rest                (steady_case.SteadyCase.rest_figures)

``python tests/analytic_case.py --record`` (``--record dynamics``: pins 6 - 9 alone, ``--record damping``: pins 10 - 14 alone, ``--record steady``: pins 16 - 19 alone, the other entries kept) measures the numpy oracle's error on the same inputs and writes tests/golden/analytic_pins.json;
the tests hold the library to 1.5 x those figures and to the second-order ratio between C24 and C48 (check_convergence).
"""
import json
import os
import sys

import numpy as np

NH = 3
DAY = 86400.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "analytic_pins.json")
AXIS = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])  # oblique to every tile
SIGN_X, SIGN_Y = -1.0, 1.0  # swept area through an x face (corner j -> j + 1) and a y face (corner i -> i + 1), per dt (psi(B) - psi(A))
RATIO = 3.5  # error(C24) / error(C48) of a second-order scheme is 4
SLACK = 1.5  # library error <= SLACK x the oracle's on the same input
A2B_K = np.array([1.3, -0.7, 2.1])


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _tangent(t, m):
    """t projected on the tangent plane at the unit vector m, normalised"""
    return _unit(t - np.sum(t * m, -1, keepdims=True) * m)


def _grow(a, shape):
    """pad [i, j, 3] to the storage shape by repeating the last row / column (never compared)"""
    while a.shape[0] < shape[0]:
        a = np.concatenate([a, a[-1:]], 0)
    while a.shape[1] < shape[1]:
        a = np.concatenate([a, a[:, -1:]], 1)
    return a


def xyz(lon, lat):
    return np.stack([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)], -1)


class Geometry:
    """Positions (unit vectors, storage shape [i, j, 3]) of one rank: corners P, cell centres C, x-face mid-points mx (corner j -> j + 1),
    y-face mid-points my (corner i -> i + 1), with the along-edge unit vectors tx (on my) and ty (on mx)."""

    def __init__(self, g):
        self.g, self.nx, self.ny = g, g.nx, g.ny
        self.P = xyz(g.lon, g.lat)
        shape = self.P.shape[:2]
        self.C = xyz(g.lon_agrid, g.lat_agrid)
        P = self.P
        self.mx = _grow(_unit(P[:, :-1] + P[:, 1:]), shape)
        self.my = _grow(_unit(P[:-1, :] + P[1:, :]), shape)
        self.ty = _tangent(_grow(P[:, 1:] - P[:, :-1], shape), self.mx)
        self.tx = _tangent(_grow(P[1:, :] - P[:-1, :], shape), self.my)
        self.X = (slice(NH, NH + g.nx + 1), slice(NH, NH + g.ny))  # compute x faces
        self.Y = (slice(NH, NH + g.nx), slice(NH, NH + g.ny + 1))  # compute y faces
        self.cells = (slice(NH, NH + g.nx), slice(NH, NH + g.ny))
        self.corners = (slice(NH, NH + g.nx + 1), slice(NH, NH + g.ny + 1))

    def e1(self):
        """cross-face direction on the x faces: central difference of the neighbouring mid-points; the edge normal on a tile edge"""
        mx, g = self.mx, self.g
        d = np.zeros_like(mx)
        d[1:-1] = mx[2:] - mx[:-2]
        d[0], d[-1] = mx[1] - mx[0], mx[-1] - mx[-2]
        e = _tangent(d, mx)
        for flag, i in ((g.west_edge, NH), (g.east_edge, NH + g.nx)):
            if flag:
                e[i] = np.cross(self.ty[i], mx[i])
        return e

    def e2(self):
        my, g = self.my, self.g
        d = np.zeros_like(my)
        d[:, 1:-1] = my[:, 2:] - my[:, :-2]
        d[:, 0], d[:, -1] = my[:, 1] - my[:, 0], my[:, -1] - my[:, -2]
        e = _tangent(d, my)
        for flag, j in ((g.south_edge, NH), (g.north_edge, NH + g.ny)):
            if flag:
                e[:, j] = np.cross(my[:, j], self.tx[:, j])
        return e


class Flow:
    """Solid-body rotation about ``axis`` on the sphere of radius a, once round in 12 days."""

    def __init__(self, a, axis=AXIS):
        self.a, self.axis = float(a), _unit(np.asarray(axis, dtype=np.float64))
        self.u0 = 2.0 * np.pi * self.a / (12.0 * DAY)
        self.omega = self.u0 / self.a

    def wind(self, p):
        return self.u0 * np.cross(np.broadcast_to(self.axis, p.shape), p)

    def psi(self, p):
        return -self.a * self.u0 * np.sum(p * self.axis, -1)

    def swept(self, G, dt):
        """(x, y) area swept through every face in dt, storage shape [i, j]"""
        s = self.psi(G.P)
        fx, fy = np.zeros_like(s), np.zeros_like(s)
        fx[:, :-1] = SIGN_X * dt * (s[:, 1:] - s[:, :-1])
        fy[:-1, :] = SIGN_Y * dt * (s[1:, :] - s[:-1, :])
        return fx, fy

    def d_grid(self, G):
        """(u, v): the along-edge components at the face mid-points"""
        return np.sum(self.wind(G.my) * G.tx, -1), np.sum(self.wind(G.mx) * G.ty, -1)

    def c_grid(self, G):
        """(uc, vc): the covariant components across the faces (edge-normal on tile-edge faces)"""
        return np.sum(self.wind(G.mx) * G.e1(), -1), np.sum(self.wind(G.my) * G.e2(), -1)

    def rotate_back(self, p, t):
        """Rot(-omega t) p about the axis (Rodrigues)"""
        th = -self.omega * t
        k = np.broadcast_to(self.axis, p.shape)
        return p * np.cos(th) + np.cross(k, p) * np.sin(th) + k * np.sum(k * p, -1, keepdims=True) * (1.0 - np.cos(th))


def levels(a, nz):
    """[i, j] -> [i, j, nz] (the same field on every level)"""
    return np.repeat(np.asarray(a)[:, :, None], nz, 2)


class CheckFailed(AssertionError):
    pass


def require(ok, msg):
    if not ok:
        raise CheckFailed(msg)


def check_bound(label, err, oracle_err, slack=SLACK):
    print(f"{label}: error {err:.4e}, oracle {oracle_err:.4e}")
    require(np.isfinite(err) and err <= slack * oracle_err, f"{label}: error {err:.4e} above {slack} x the oracle's {oracle_err:.4e}")


def check_convergence(label, coarse, fine, ratio=RATIO):
    print(f"{label}: C24 {coarse:.4e} / C48 {fine:.4e} = {coarse / fine:.2f}")
    require(coarse >= ratio * fine, f"{label}: error falls by {coarse / fine:.2f} per doubling, second order needs >= {ratio}")


# ---------------------------------------------------------------------------------------------------------------------------
# pin 1: fxadv
# ---------------------------------------------------------------------------------------------------------------------------
def flux_dt(n, flow):
    """dt at which the largest Courant number is about 0.5: the narrowest cell of the equal-edge gnomonic grid is the corner one, about
    0.71 x the mean width a (pi / 2) / n"""
    return 0.5 * 0.7 * flow.a * (np.pi / 2.0) / n / flow.u0


def flux_case(grids, flow, nz=1):
    """per rank: geometry, analytic uc / vc over the whole storage [i, j, nz]"""
    out = []
    for g in grids:
        G = Geometry(g)
        uc, vc = flow.c_grid(G)
        out.append((G, levels(uc, nz), levels(vc, nz)))
    return out


def flux_errors(case, flow, dt, xfx, yfx):
    """max |got - exact| / max |exact| over the compute faces of every rank: (all faces, tile-edge faces alone)"""
    err = edge = scale = 0.0
    for (G, _, _), fx, fy in zip(case, xfx, yfx):
        ex, ey = flow.swept(G, dt)
        for got, want, F, lines in ((fx, ex, G.X, [(0, G.g.west_edge, 0), (0, G.g.east_edge, -1)]), (fy, ey, G.Y, [(1, G.g.south_edge, 0), (1, G.g.north_edge, -1)])):
            d = np.abs(np.asarray(got)[F] - want[F][..., None])
            require(np.all(np.isfinite(d)), "non-finite area flux")
            err, scale = max(err, float(d.max())), max(scale, float(np.abs(want[F]).max()))
            for ax, flag, idx in lines:
                if flag:
                    edge = max(edge, float(np.take(d, idx, axis=ax).max()))
    return err / scale, edge / scale


def oracle_fluxes(doms, case, dt):
    from fv3_oracle import d_sw as o_dsw

    xs, ys, crs = [], [], []
    for D, (G, uc, vc) in zip(doms, case):
        z = [np.zeros_like(uc) for _ in range(6)]
        o_dsw.fxadv(D, uc.copy(), vc.copy(), *z, dt)
        xs.append(z[2]), ys.append(z[3]), crs.append((z[0], z[1]))
    return xs, ys, crs


def upwind_area(g, sx, sy):
    """the (dxa dy sin_sg, dya dx sin_sg) of the cell upwind of every face, by the sign of sx / sy [i, j(, k)]: the factor between a Courant
    number and an area flux in fxadv and tracer_2d_1l -- metric side, never part of an expected value"""
    def up(a, ax):  # the cell before the face along ax; the first line has none and is never compared
        b = np.roll(a, 1, ax)
        b[(slice(None),) * ax + (0,)] = np.take(a, 0, axis=ax)
        return b

    ax_, ay_ = g.dxa * g.sin_sg3, g.dya * g.sin_sg4
    bx_, by_ = g.dxa * g.sin_sg1, g.dya * g.sin_sg2
    ext = (lambda a: a[:, :, None]) if np.ndim(sx) == 3 else (lambda a: a)
    return (np.where(sx > 0.0, ext(up(ax_, 0) * g.dy), ext(bx_ * g.dy)), np.where(sy > 0.0, ext(up(ay_, 1) * g.dx), ext(by_ * g.dx)))


def courant_consistency(g, crx, cry, xfx, yfx):
    """crx x the upwind (dxa dy sin_sg) against x_area_flux, likewise y, on the compute faces: worst error relative to the largest flux"""
    G = Geometry(g)
    ux, uy = upwind_area(g, np.asarray(crx), np.asarray(cry))
    ex = np.abs(np.asarray(crx) * ux - xfx)[G.X].max() / np.abs(np.asarray(xfx)[G.X]).max()
    ey = np.abs(np.asarray(cry) * uy - yfx)[G.Y].max() / np.abs(np.asarray(yfx)[G.Y]).max()
    return float(max(ex, ey))


# ---------------------------------------------------------------------------------------------------------------------------
# pin 3: the D-to-C wind conversion
# ---------------------------------------------------------------------------------------------------------------------------
def wind_case(grids, flow, nz=1):
    out = []
    for g in grids:
        G = Geometry(g)
        u, v = flow.d_grid(G)
        uc, vc = flow.c_grid(G)
        out.append((G, levels(u, nz), levels(v, nz), uc, vc))
    return out


def wind_errors(case, flow, ucs, vcs):
    """max |got - exact| / U0 over the compute faces: (all, tile-edge faces alone)"""
    err = edge = 0.0
    for (G, _, _, euc, evc), uc, vc in zip(case, ucs, vcs):
        for got, want, F, lines in ((uc, euc, G.X, [(0, G.g.west_edge, 0), (0, G.g.east_edge, -1)]), (vc, evc, G.Y, [(1, G.g.south_edge, 0), (1, G.g.north_edge, -1)])):
            d = np.abs(np.asarray(got)[F] - want[F][..., None])
            require(np.all(np.isfinite(d)), "non-finite C-grid wind")
            err = max(err, float(d.max()))
            for ax, flag, idx in lines:
                if flag:
                    edge = max(edge, float(np.take(d, idx, axis=ax).max()))
    return err / flow.u0, edge / flow.u0


def oracle_winds(doms, case):
    from fv3_oracle import c_sw as o_csw

    ucs, vcs = [], []
    for D, (G, u, v, _, _) in zip(doms, case):
        one, z = np.ones_like(u), lambda: np.zeros_like(u)  # noqa: E731
        uc, vc = z(), z()
        o_csw.c_sw(D, one.copy(), one.copy(), u.copy(), v.copy(), z(), uc, vc, z(), z(), z(), z(), z(), z(), 0.0, nord=0)
        ucs.append(uc), vcs.append(vc)
    return ucs, vcs


# ---------------------------------------------------------------------------------------------------------------------------
# pin 4: a2b_ord4
# ---------------------------------------------------------------------------------------------------------------------------
def smooth(p):
    return np.sin(np.sum(p * A2B_K, -1) + 0.4) + 0.5 * np.cos(2.0 * p[..., 0] - p[..., 2])


def corner_case(grids, nz=1):
    out = []
    for g in grids:
        G = Geometry(g)
        out.append((G, levels(smooth(G.C), nz), smooth(G.P)))
    return out


def corner_classes(G):
    """masks over the compute corners: interior, tile-edge corners, cube corners"""
    g = G.g
    ni, nj = g.nx + 1, g.ny + 1
    on_x, on_y = np.zeros((ni, nj), bool), np.zeros((ni, nj), bool)
    if g.west_edge:
        on_x[0] = True
    if g.east_edge:
        on_x[-1] = True
    if g.south_edge:
        on_y[:, 0] = True
    if g.north_edge:
        on_y[:, -1] = True
    return {"interior": ~(on_x | on_y), "edge": on_x ^ on_y, "corner": on_x & on_y}


def corner_errors(case, outs):
    """max |got - exact| per class of corners (the field is O(1)) and over all of them"""
    err = {"interior": 0.0, "edge": 0.0, "corner": 0.0}
    for (G, _, want), got in zip(case, outs):
        d = np.abs(np.asarray(got)[G.corners] - want[G.corners][..., None])
        require(np.all(np.isfinite(d)), "non-finite corner value")
        for k, m in corner_classes(G).items():
            if m.any():
                err[k] = max(err[k], float(d[m].max()))
    err["all"] = max(err.values())
    return err


def oracle_corners(doms, case):
    from fv3_oracle import a2b_ord4 as o_a2b

    return [o_a2b.a2b_ord4(D, q.copy()) for D, (G, q, _) in zip(doms, case)]


# ---------------------------------------------------------------------------------------------------------------------------
# pin 2: a bell carried once round the sphere
# ---------------------------------------------------------------------------------------------------------------------------
TRACERS = ("bell", "gauss", "one")
BELL_RADIUS, GAUSS_WIDTH = 1.0 / 3.0, 0.18  # great-circle radians: a / 3 and 0.18 a


def bell_centre(part):
    """a cube corner: the south-west corner of tile 0"""
    from pace_amd.grid import tile_point

    return tile_point(0, np.array(0), np.array(0), part.nx_tile)


def bell_flows(centre, a):
    """level 0: an axis perpendicular to the centre, so that the bell rides a great circle that leaves the cube corner obliquely and meets
    cube corners and edges on its way; level 1: the z axis, a square path through four tile edges"""
    return [Flow(a, np.cross(centre, AXIS)), Flow(a, [0.0, 0.0, 1.0])]


def bell_shapes(p, centre):
    r = np.arctan2(np.linalg.norm(np.cross(p, np.broadcast_to(centre, p.shape)), axis=-1), np.sum(p * centre, -1))
    return {"bell": np.where(r < BELL_RADIUS, 0.5 * (1.0 + np.cos(np.pi * r / BELL_RADIUS)), 0.0), "gauss": np.exp(-((r / GAUSS_WIDTH) ** 2)), "one": np.ones_like(r)}


def bell_calls(n, cfl=0.5):
    """calls of one revolution at the Courant number ``cfl`` of the mean cell width a (pi / 2) / n: 192 at C24, 384 at C48 for 0.5"""
    return int(round(4 * n / cfl))


class BellCase:
    """per rank r: q0[r][name] [i, j, 2] the initial tracers, mfx / mfy the exact swept areas x dp1 (dp1 == 1), cx / cy the swept areas
    over the upwind (dxa dy sin_sg) -- the operator multiplies that back, so the flux it transports is the exact one"""

    def __init__(self, part, grids, a, n_calls, turn=1.0):
        self.part, self.grids, self.n_calls, self.turn = part, grids, n_calls, turn
        self.centre = bell_centre(part)
        self.flows = bell_flows(self.centre, a)
        self.period = 2.0 * np.pi / self.flows[0].omega
        self.dt = turn * self.period / n_calls
        self.G = [Geometry(g) for g in grids]
        self.q0, self.mfx, self.mfy, self.cx, self.cy = [], [], [], [], []
        for g, G in zip(grids, self.G):
            sw = [f.swept(G, self.dt) for f in self.flows]
            fx, fy = np.stack([s[0] for s in sw], -1), np.stack([s[1] for s in sw], -1)
            ux, uy = upwind_area(g, fx, fy)
            self.mfx.append(fx), self.mfy.append(fy), self.cx.append(fx / ux), self.cy.append(fy / uy)
            sh = bell_shapes(G.C, self.centre)
            self.q0.append({k: levels(v, 2) for k, v in sh.items()})

    def exact(self, r, name, way=1.0):
        """the solution at the cell centres after the run: q0(Rot(-omega t) p); way = -1 turns it the wrong way (the control)"""
        t = way * self.dt * self.n_calls
        return np.stack([bell_shapes(f.rotate_back(self.G[r].C, t), self.centre)[name] for f in self.flows], -1)

    def errors(self, tracers, way=1.0):
        """{(name, level): (l2, linf)} area-weighted over the cube, plus the side figures: relative tracer-mass change, the constant's
        deviation from 1, min and max per tracer"""
        out, side = {}, {}
        for name in TRACERS:
            num, den, linf, top, mass0, mass1, lo, hi = np.zeros(2), np.zeros(2), np.zeros(2), np.zeros(2), np.zeros(2), np.zeros(2), np.full(2, np.inf), np.full(2, -np.inf)
            for r, (g, G) in enumerate(zip(self.grids, self.G)):
                w = g.area[G.cells][..., None]
                got, want = np.asarray(tracers[r][name], dtype=np.float64)[G.cells][..., :2], self.exact(r, name, way)[G.cells]
                require(np.all(np.isfinite(got)), f"{name}: non-finite")
                num += (w * (got - want) ** 2).sum((0, 1))
                den += (w * want**2).sum((0, 1))
                linf, top = np.maximum(linf, np.abs(got - want).max((0, 1))), np.maximum(top, np.abs(want).max((0, 1)))
                mass0 += (w * self.q0[r][name][G.cells]).sum((0, 1))
                mass1 += (w * got).sum((0, 1))
                lo, hi = np.minimum(lo, got.min((0, 1))), np.maximum(hi, got.max((0, 1)))
            for k in range(2):
                out[(name, k)] = (float(np.sqrt(num[k] / den[k])), float(linf[k] / top[k]))
            side[name] = {"mass": float(np.abs(mass1 / mass0 - 1.0).max()), "min": float(lo.min()), "max": float(hi.max())}
        return out, side


def oracle_bell(doms, bc, hord):
    """the numpy oracle through the run: (tracers per rank, n_split of the last call)"""
    from fv3_oracle import tracer_2d_1l as o_t2
    from fv3_oracle.dyn_core import OracleExchange

    ex = OracleExchange(bc.part, NH)
    tr = [{k: v.copy() for k, v in q.items()} for q in bc.q0]
    ns = None
    for _ in range(bc.n_calls):
        for name in TRACERS:
            ex.scalar([t[name] for t in tr])
        F = [[a.copy() for a in x] for x in (bc.mfx, bc.mfy, bc.cx, bc.cy)]
        dp1 = [np.ones_like(a) for a in bc.cx]
        ns = o_t2.tracer_2d_1l(doms, tr, dp1, *F, hord, halo_update=lambda fs: ex.scalar(fs))
    return tr, ns


# ---------------------------------------------------------------------------------------------------------------------------
# pin 5a: an isentropic atmosphere at rest over terrain feels no pressure-gradient force
# ---------------------------------------------------------------------------------------------------------------------------
P0, THETA, T_CONTROL, PP_BETA, PGF_DT = 1.0e5, 300.0, 250.0, -0.01, 10.0


def terrain(p):
    """surface height [m]: a 3 km Gaussian mountain next to the cube corner the bell starts on, plus a smooth wave, clipped at 0"""
    top = _unit(np.array([0.62, -0.55, -0.56]))  # 0.1 rad from the south-west corner of tile 0
    r = np.arctan2(np.linalg.norm(np.cross(p, np.broadcast_to(top, p.shape)), axis=-1), np.sum(p * top, -1))
    return np.maximum(0.0, 3000.0 * np.exp(-((r / 0.25) ** 2)) + 600.0 * np.sin(3.0 * p[..., 0] + 1.0) * np.cos(2.0 * p[..., 1] - p[..., 2]))


def resting_state(g, c, isentropic=True):
    """[i, j, nz + 1] arrays at the cell centres (halo included) of the hydrostatic atmosphere at rest over ``terrain``: delp, pk3 = pe^kappa,
    gz, pp = beta (gz - gz[top]).  isentropic: gz = A - cp theta pk3 with A = cp theta p0^kappa (theta in the model's unit, 300 K / p0^kappa) --
    linear in pk3, so that every four-point bracket of the operators cancels.  Otherwise the control, gz = phis + R 250 K ln(ps / pe)."""
    kap, cp = c.KAPPA, c.RDGAS / c.KAPPA
    th = THETA / P0**kap
    A = cp * th * P0**kap
    phis = c.GRAV * terrain(xyz(g.lon_agrid, g.lat_agrid))
    ps = ((A - phis) / (cp * th)) ** (1.0 / kap)
    pe = g.ak[None, None, :] + g.bk[None, None, :] * ps[:, :, None]
    pk3 = pe**kap
    gz = A - cp * th * pk3 if isentropic else phis[:, :, None] + c.RDGAS * T_CONTROL * np.log(ps[:, :, None] / pe)
    delp = np.concatenate([np.diff(pe, axis=2), np.diff(pe, axis=2)[:, :, -1:]], 2)
    return {"delp": delp, "pk3": pk3, "gz": gz, "pp": PP_BETA * (gz - gz[:, :, :1])}


def oracle_pgf(D, c, st, u_in=0.0):
    """(u, v) of the oracle's nh_p_grad on a copy of the state"""
    from fv3_oracle import nh as o_nh

    s = {k: v.copy() for k, v in st.items()}
    u, v = np.full_like(s["gz"], u_in), np.full_like(s["gz"], u_in)
    o_nh.nh_p_grad(D, u, v, s["pp"], s["gz"], s["pk3"], s["delp"], PGF_DT, float(D.grid.ptop), c.KAPPA)
    return u, v


def oracle_pgf_c(D, st):
    from fv3_oracle import nh as o_nh

    uc, vc = np.zeros_like(st["gz"]), np.zeros_like(st["gz"])
    o_nh.p_grad_c(D, D.m.rdxc, D.m.rdyc, uc, vc, st["delp"].copy(), st["pk3"].copy(), st["gz"].copy(), PGF_DT)
    return uc, vc


def force(G, u, v, nz):
    """max |u|, |v| on the compute faces (the wind the force left on a state at rest)"""
    return max(float(np.abs(np.asarray(u)[G.Y][..., :nz]).max()), float(np.abs(np.asarray(v)[G.X][..., :nz]).max()))


def check_no_force(label, rest, control, bound=1e-9):
    print(f"{label}: max |du| {rest:.3e} on the isentropic state, {control:.3e} on the control")
    require(np.isfinite(rest) and control > 0.0 and rest <= bound * control, f"{label}: |du| {rest:.3e} on the isentropic state above {bound} x the control's {control:.3e}")


# ---------------------------------------------------------------------------------------------------------------------------
# pin 5b: profiles linear in pressure through the remap
# ---------------------------------------------------------------------------------------------------------------------------
LINEAR = {"q0": (2.0e-3, 1.0e-7), "q1": (5.0, -3.0e-5)}  # tracers: alpha + beta p_mid (positive on 0 .. 1.1e5 Pa)
LINEAR_W, LINEAR_UV = (0.3, -4.0e-6), (-12.0, 2.5e-4)


def _mid(pe):
    return 0.5 * (pe[..., 1:] + pe[..., :-1])


def lagrangian_delp(state_delp, nz, seed=17):
    """the synthetic state's layers made non-uniform: every layer of every column (halo included) stretched by a random 0.7 .. 1.3"""
    rng = np.random.default_rng(seed)
    d = state_delp.copy()
    d[:, :, :nz] *= rng.uniform(0.7, 1.3, d[:, :, :nz].shape)
    return d


def linear_columns(g, delp, nz, profile):
    """(layer means alpha + beta p_mid on the Lagrangian layers [i, j, nz], the same on the Eulerian layers ak + bk ps)"""
    a, b = profile
    pe1 = g.ptop + np.concatenate([np.zeros(delp.shape[:2] + (1,)), np.cumsum(delp[:, :, :nz], 2)], 2)
    pe2 = g.ak[None, None, :] + g.bk[None, None, :] * pe1[:, :, -1:]
    pe2[:, :, 0], pe2[:, :, -1] = g.ptop, pe1[:, :, -1]
    return a + b * _mid(pe1), a + b * _mid(pe2), pe1, pe2


def linear_winds(g, delp, nz, profile):
    """u / v linear in the edge-averaged pressure (u: rows j - 1 and j; v: columns i - 1 and i): (u, u expected, v, v expected), [i, j, nz],
    valid from the second row / column on"""
    a, b = profile
    pe1 = g.ptop + np.concatenate([np.zeros(delp.shape[:2] + (1,)), np.cumsum(delp[:, :, :nz], 2)], 2)
    out = []
    for ax in (1, 0):
        pe0 = 0.5 * (pe1 + np.roll(pe1, 1, ax))
        pe3 = g.ak[None, None, :] + g.bk[None, None, :] * pe0[:, :, -1:]
        pe3[:, :, 0], pe3[:, :, -1] = g.ptop, pe0[:, :, -1]
        out += [a + b * _mid(pe0), a + b * _mid(pe3)]
    return out


def check_linear(label, got, want, profile_range, bound=1e-13):
    err = float(np.abs(np.asarray(got) - want).max())
    print(f"{label}: max error {err:.3e} of a range {profile_range:.3e}")
    require(np.isfinite(err) and err <= bound * profile_range, f"{label}: error {err:.3e} above {bound} x the profile's range {profile_range:.3e}")
    return err


# ---------------------------------------------------------------------------------------------------------------------------
# pins 6 and 7: d_sw on solid-body rotation with every damping term off (tests/test_analytic_dynamics.py)
# ---------------------------------------------------------------------------------------------------------------------------
DYN_NZ = 3
DSW_OFF = dict(nord=0, d2_bg=0.0, d2_bg_k1=0.0, d2_bg_k2=0.0, d4_bg=0.0, dddmp=0.0, d_con=0.0, vtdm4=0.0, ke_bg=0.0, do_vort_damp=False, n_sponge=-1)
D_SW_ORDER = ("delpc", "delp", "pt", "u", "v", "w", "uc", "vc", "ua", "va", "divgd", "mfxd", "mfyd", "cxd", "cyd", "crx", "cry", "xfx", "yfx", "q_con", "zh", "heat_source", "diss_est")
D_SW_INPUTS = ("delp", "pt", "u", "v", "w", "uc", "vc", "mfxd", "mfyd", "cxd", "cyd", "q_con")
SCALARS = ("delp", "pt", "w", "q_con")
K_PT, K_W, K_QC = np.array([-0.9, 1.6, 0.8]), np.array([2.2, 0.6, -1.1]), np.array([0.5, -1.9, 1.4])
Z_AXIS = (0.0, 0.0, 1.0)
SECOND, INTERIOR = 2, 3  # face classes of pin 7 after 0 and 1
CLASS_KEYS = {0: "class0", 1: "class1", SECOND: "second_line", INTERIOR: "class2"}


def dyn_dt(n, flow):
    """Courant number 0.1 at C24 and falling as 1 / n: dt falls as 1 / n^2, so that the error of one call measures the scheme's truncation
    and not the time step's"""
    return 0.1 * (24.0 / n) * 0.7 * flow.a * (np.pi / 2.0) / n / flow.u0


def _wave(p, kvec, phase):
    return np.sin(np.sum(p * kvec, -1) + phase) + 0.5 * np.cos(2.0 * p[..., 1] + p[..., 2] - phase)


# the scalars d_sw transports, as functions of position [..., 3] -> [..., nz]; SCALAR_SCALE is the amplitude the errors are quoted against
SCALAR_SCALE = {"delp": 1000.0, "pt": 20.0, "w": 1.0, "q_con": 0.01}


def scalar_field(name, p, nz=DYN_NZ):
    if name == "delp":
        return levels_last(1000.0 * (2.5 + smooth(p)), nz)
    kvec, base, amp = {"pt": (K_PT, 300.0, 20.0), "w": (K_W, 2.5, 1.0), "q_con": (K_QC, 0.025, 0.01)}[name]
    return np.stack([base + amp * _wave(p, kvec, 0.3 + 0.7 * k) for k in range(nz)], -1)


def levels_last(a, nz):
    return np.repeat(np.asarray(a)[..., None], nz, -1)


def arc(a, b):
    """great-circle angle between unit vectors"""
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=-1), np.sum(a * b, -1))


def face_classes(G):
    """(classes of the u faces [nx, ny + 1], of the v faces [nx + 1, ny]) by the distance in lines from the nearest cube-tile edge: 0 on the edge;
    1 the line next to it in the cross direction (u in cell columns 1 and nx, v in cell rows 1 and ny: faces with one end on the edge); SECOND the line
    after either (u in corner rows 2 and ny, cell columns 2 and nx - 1); INTERIOR two or more lines from every tile edge -- the edges of a sub-domain
    inside a tile included"""
    g = G.g
    cu, cv = np.full((g.nx, g.ny + 1), INTERIOR), np.full((g.nx + 1, g.ny), INTERIOR)
    cross, along = (g.west_edge, g.east_edge), (g.south_edge, g.north_edge)
    for value, first in ((SECOND, 1), (1, 0)):  # the cross direction of u is x, of v (seen transposed) y
        for c, (lo, hi) in ((cu, cross), (cv.T, along)):
            if lo:
                c[first, :] = value
            if hi:
                c[-1 - first, :] = value
    for c, (lo, hi) in ((cu, along), (cv.T, cross)):
        if lo:
            c[:, 1] = np.minimum(c[:, 1], SECOND)
            c[:, 0] = 0
        if hi:
            c[:, -2] = np.minimum(c[:, -2], SECOND)
            c[:, -1] = 0
    return cu, cv


def edge_ke_excess(G, flow):
    """0.5 cot(alpha) Vn Vt on the compute corners [nx + 1, ny + 1] that lie on a cube-tile edge (0 elsewhere and on the cube corners): what d_sw's
    corner kinetic energy holds above 0.5 |V|^2 there.  With t the edge's tangent, n its normal and e the direction of the grid line that crosses the
    edge on the upstream side (all three from corner positions): Vn = V . n, Vt = V . t, cot(alpha) = (e . t) / (e . n)."""
    P, g = G.P, G.g
    ex = np.zeros((g.nx + 1, g.ny + 1))

    def term(p, along_m, along_p, cross_m, cross_p):
        t = _tangent(along_p - along_m, p)
        e_m, e_p = _tangent(p - cross_m, p), _tangent(cross_p - p, p)
        n = _unit(e_p - np.sum(e_p * t, -1, keepdims=True) * t)
        V = flow.wind(p)
        vn, vt = np.sum(V * n, -1), np.sum(V * t, -1)
        e = np.where((vn > 0.0)[..., None], e_m, e_p)
        return 0.5 * np.sum(e * t, -1) / np.sum(e * n, -1) * vn * vt

    J = slice(NH + 1, NH + g.ny)  # without the cube corners
    for flag, i, I in ((g.west_edge, 0, NH), (g.east_edge, -1, NH + g.nx)):
        if flag:
            ex[i, 1:-1] = term(P[I, J], P[I, NH : NH + g.ny - 1], P[I, NH + 2 : NH + g.ny + 1], P[I - 1, J], P[I + 1, J])
    Ii = slice(NH + 1, NH + g.nx)
    for flag, j, Jj in ((g.south_edge, 0, NH), (g.north_edge, -1, NH + g.ny)):
        if flag:
            ex[1:-1, j] = term(P[Ii, Jj], P[NH : NH + g.nx - 1, Jj], P[NH + 2 : NH + g.nx + 1, Jj], P[Ii, Jj - 1], P[Ii, Jj + 1])
    if not (g.west_edge or g.east_edge or g.south_edge or g.north_edge):
        return ex
    # a sub-domain that holds part of an edge: the end corners of that part are ordinary edge corners, not cube corners
    for flag, i, I in ((g.west_edge, 0, NH), (g.east_edge, -1, NH + g.nx)):
        if flag:
            for on_tile_corner, j, Jj in ((g.south_edge, 0, NH), (g.north_edge, -1, NH + g.ny)):
                if not on_tile_corner:
                    ex[i, j] = term(P[I, Jj], P[I, Jj - 1], P[I, Jj + 1], P[I - 1, Jj], P[I + 1, Jj])
    for flag, j, Jj in ((g.south_edge, 0, NH), (g.north_edge, -1, NH + g.ny)):
        if flag:
            for on_tile_corner, i, I in ((g.west_edge, 0, NH), (g.east_edge, -1, NH + g.nx)):
                if not on_tile_corner:
                    ex[i, j] = term(P[I, Jj], P[I - 1, Jj], P[I + 1, Jj], P[I, Jj - 1], P[I, Jj + 1])
    return ex


class DswCase:
    """d_sw on solid-body rotation, per rank r: ins[r] the inputs [i, j, nz] over the whole storage (u, v, uc, vc analytic; delp, pt, w, q_con
    smooth positive functions of position; mfxd, mfyd, cxd, cyd pre-filled with a smooth non-zero field), and the closed-form answers."""

    def __init__(self, n, grids, a, omega_earth, axis=AXIS, nz=DYN_NZ):
        self.n, self.grids, self.nz, self.rot = n, grids, nz, float(omega_earth)
        self.flow = Flow(a, axis)
        self.dt = dyn_dt(n, self.flow)
        self.G = [Geometry(g) for g in grids]
        self.ins = []
        for G in self.G:
            u, v = self.flow.d_grid(G)
            uc, vc = self.flow.c_grid(G)
            sx, sy = self.flow.swept(G, self.dt)
            x = {"u": levels(u, nz), "v": levels(v, nz), "uc": levels(uc, nz), "vc": levels(vc, nz)}
            x.update({k: scalar_field(k, G.C, nz) for k in SCALARS})
            top = 1000.0 * max(np.abs(sx[G.X]).max(), np.abs(sy[G.Y]).max())
            x["mfxd"], x["mfyd"] = levels(top * (2.0 + smooth(G.mx)), nz), levels(top * (2.0 + smooth(G.my)), nz)
            x["cxd"], x["cyd"] = levels(0.05 * (2.0 + smooth(G.mx)), nz), levels(0.05 * (2.0 + smooth(G.my)), nz)
            self.ins.append(x)

    def tendency(self, p):
        """T(p) = -(zeta + f) p x V - grad K of the rotation: zeta = 2 omega s, f = 2 OMEGA p_z, K = U0^2 (1 - s^2) / 2, s = p . axis"""
        fl = self.flow
        s = np.sum(p * fl.axis, -1, keepdims=True)
        return -(2.0 * fl.omega * s + 2.0 * self.rot * p[..., 2:3]) * np.cross(p, fl.wind(p)) + (fl.u0**2 / fl.a) * s * (fl.axis - s * p)

    def scalar_errors(self, outs, way=1.0):
        """max |got - exact| / SCALAR_SCALE over the cells of every rank, per transported scalar; mfx / mfy and cx / cy relative to the largest exact
        value; max |heat_source|, |diss_est|.  way = -1: against the solution turned the wrong way (the control)"""
        fl, dt, nz = self.flow, self.dt, self.nz
        err = dict.fromkeys(SCALARS + ("mfx", "mfy", "cx", "cy", "heat", "diss"), 0.0)
        top = dict.fromkeys(("mfx", "mfy", "cx", "cy"), 0.0)
        for g, G, x, o in zip(self.grids, self.G, self.ins, outs):
            o = {k: np.asarray(v, dtype=np.float64)[:, :, :nz] for k, v in o.items() if v is not None}
            back = fl.rotate_back(G.C[G.cells], way * dt)
            for k in SCALARS:
                require(np.all(np.isfinite(o[k][G.cells])), f"{k}: non-finite")
                err[k] = max(err[k], float(np.abs(o[k][G.cells] - scalar_field(k, back, nz)).max()) / SCALAR_SCALE[k])
            sx, sy = fl.swept(G, dt)
            for k, name, m, s, F in (("mfx", "mfxd", G.mx, sx, G.X), ("mfy", "mfyd", G.my, sy, G.Y)):
                want = scalar_field("delp", fl.rotate_back(m[F], way * 0.5 * dt), nz) * s[F][..., None]
                err[k], top[k] = max(err[k], float(np.abs((o[name] - x[name])[F] - want).max())), max(top[k], float(np.abs(want).max()))
            dcx, dcy = o["cxd"] - x["cxd"], o["cyd"] - x["cyd"]
            ux, uy = upwind_area(g, dcx, dcy)
            for k, d, up, s, F in (("cx", dcx, ux, sx, G.X), ("cy", dcy, uy, sy, G.Y)):
                err[k], top[k] = max(err[k], float(np.abs((d * up)[F] - s[F][..., None]).max())), max(top[k], float(np.abs(s[F]).max()))
            err["heat"] = max(err["heat"], float(np.abs(o["heat_source"][G.cells]).max()))
            err["diss"] = max(err["diss"], float(np.abs(o["diss_est"][G.cells]).max()))
        for k in top:
            err[k] /= top[k]
        return err

    def wind_residuals(self, outs):
        """per rank: (classes, tendency residual, closed-form edge term) of the u faces and of the v faces, with the largest exact tendency.  The
        tendency is (u_out / L - u_in) / dt, L the great-circle length of the face's edge (d_sw returns u dx)."""
        fl, dt, nz = self.flow, self.dt, self.nz
        res, top = [], 0.0
        for G, x, o in zip(self.G, self.ins, outs):
            P = G.P
            Lu, Lv = fl.a * _grow(arc(P[:-1, :], P[1:, :]), P.shape[:2]), fl.a * _grow(arc(P[:, :-1], P[:, 1:]), P.shape[:2])
            ex = edge_ke_excess(G, fl)
            cu, cv = face_classes(G)
            tu = (np.asarray(o["u"], dtype=np.float64)[:, :, :nz][G.Y] / Lu[G.Y][..., None] - x["u"][G.Y]) / dt
            tv = (np.asarray(o["v"], dtype=np.float64)[:, :, :nz][G.X] / Lv[G.X][..., None] - x["v"][G.X]) / dt
            require(np.all(np.isfinite(tu)) and np.all(np.isfinite(tv)), "non-finite wind")
            wu, wv = np.sum(self.tendency(G.my[G.Y]) * G.tx[G.Y], -1), np.sum(self.tendency(G.mx[G.X]) * G.ty[G.X], -1)
            top = max(top, float(np.abs(wu).max()), float(np.abs(wv).max()))
            res.append(((cu, tu - wu[..., None], ((ex[:-1, :] - ex[1:, :]) / Lu[G.Y])[..., None]), (cv, tv - wv[..., None], ((ex[:, :-1] - ex[:, 1:]) / Lv[G.X])[..., None])))
        return res, top

    def wind_errors(self, outs, only=None):
        """max |tendency - exact| / max |exact| per class of faces (face_classes): {"class0", "class1", "second_line", "class2" (two or more lines
        from every tile edge), and "class0_less_edge_term", "class1_less_edge_term": with the closed-form edge term taken off; "class0_inner": class 0 without the faces
        that end on a cube corner, where d_sw's corner kinetic energy is another formula}.  only(rank index, "u" | "v", G) -> mask of the faces to look at (default: all)"""
        res, top = self.wind_residuals(outs)
        err = dict.fromkeys(list(CLASS_KEYS.values()) + ["class0_less_edge_term", "class1_less_edge_term", "class0_inner", "class0_inner_less_edge_term"], 0.0)
        for r, pair in enumerate(res):
            for which, (cls, d, edge) in zip("uv", pair):
                keep = np.ones(cls.shape, bool) if only is None else only(r, which, self.G[r])
                for c, key in CLASS_KEYS.items():
                    m = (cls == c) & keep
                    if m.any():
                        err[key] = max(err[key], float(np.abs(d[m]).max()))
                        if c in (0, 1):
                            err[key + "_less_edge_term"] = max(err[key + "_less_edge_term"], float(np.abs((d - edge)[m]).max()))
                if which == "v":
                    cls, d, edge, keep = cls.T, d.transpose(1, 0, 2), edge.transpose(1, 0, 2), keep.T
                m = ((cls == 0) & keep)[1:-1]  # on the edge, without the two faces that end on a cube corner
                if m.any():
                    err["class0_inner"] = max(err["class0_inner"], float(np.abs(d[1:-1][m]).max()))
                    err["class0_inner_less_edge_term"] = max(err["class0_inner_less_edge_term"], float(np.abs((d - edge)[1:-1][m]).max()))
        return {k: v / top for k, v in err.items()}


def tile0_east(r, which, G):
    """the faces of pin 7's z-axis control: the u faces of the cell column next to the east edge"""
    m = np.zeros((G.nx, G.ny + 1) if which == "u" else (G.nx + 1, G.ny), bool)
    if which == "u" and G.g.east_edge:
        m[-1, :] = True
    return m


def dyn_config(n, layout, nz=DYN_NZ, **kw):
    from pace_amd.config import AcousticDynamicsConfig

    return AcousticDynamicsConfig(**dict(dict(npx=n + 1, npy=n + 1, npz=nz, layout=layout, **DSW_OFF), **kw))


def oracle_d_sw(doms, cfg, dc):
    """the oracle's d_sw on copies of the case's inputs: the outputs per rank"""
    from fv3_oracle import d_sw as o_dsw

    col = o_dsw.get_column_namelist(cfg, dc.nz)
    outs = []
    for D, x in zip(doms, dc.ins):
        w = {k: (x[k].copy() if k in x else np.zeros_like(x["u"])) for k in D_SW_ORDER}
        w["zh"] = None
        o_dsw.d_sw(D, cfg, col, *[w[k] for k in D_SW_ORDER], dc.dt)
        outs.append(w)
    return outs


def dsw_case(shape, grids, c, axis=AXIS):
    return DswCase(SHAPES[shape][0], grids, c.RADIUS, c.OMEGA, axis)


def measure_d_sw(shape, axis=AXIS, ranks=None):
    """the oracle's figures of pins 6 and 7 on one shape"""
    n, layout, rk = SHAPES[shape]
    part, grids, doms, c = make(n, layout, rk if ranks is None else ranks, DYN_NZ)
    dc = dsw_case(shape, grids, c, axis)
    outs = oracle_d_sw(doms, dyn_config(n, layout), dc)
    if ranks is not None:  # the z-axis control of pin 7
        return {"dt": dc.dt, **dc.wind_errors(outs), "tile0_east_class1": dc.wind_errors(outs, tile0_east)["class1"]}
    return {"pin6": {"dt": dc.dt, **dc.scalar_errors(outs)}, "pin7": {"dt": dc.dt, **dc.wind_errors(outs)}}


# ---------------------------------------------------------------------------------------------------------------------------
# pin 9: update_dz_d carries interface heights with the flow
# ---------------------------------------------------------------------------------------------------------------------------
ZS, DZ_LAYER, DZ_WAVE = 100.0, 2000.0, 300.0


def height_field(p, nz=DYN_NZ):
    """[..., nz + 1] interface heights: H_k + 300 m x smooth-like waves above the flat surface ZS"""
    top = [ZS + DZ_LAYER * (nz - k) + DZ_WAVE * _wave(p, K_W, 0.5 * k) / 1.5 for k in range(nz)]
    return np.stack(top + [np.full(p.shape[:-1], ZS)], -1)


class HeightCase:
    """per rank: zh [i, j, nz + 1], zs [i, j, 1], the exact swept areas xfx / yfx and the Courant numbers crx / cry = area over the upwind cell's
    (as BellCase) on nz levels"""

    def __init__(self, n, grids, a, nz=DYN_NZ):
        self.n, self.grids, self.nz = n, grids, nz
        self.flow = Flow(a)
        self.dt = dyn_dt(n, self.flow)
        self.G = [Geometry(g) for g in grids]
        self.ins = []
        for g, G in zip(grids, self.G):
            sx, sy = self.flow.swept(G, self.dt)
            ux, uy = upwind_area(g, sx, sy)
            self.ins.append({"zh": height_field(G.C, nz), "zs": np.full(G.C.shape[:2] + (1,), ZS), "xfx": levels(sx, nz + 1), "yfx": levels(sy, nz + 1),
                             "crx": levels(sx / ux, nz + 1), "cry": levels(sy / uy, nz + 1)})

    def errors(self, zhs, wss, way=1.0):
        """(max |zh - exact| / 300 m over the interfaces above the surface, max |wsd| dt / ZS)"""
        err = ws = 0.0
        for G, zh, w in zip(self.G, zhs, wss):
            got = np.asarray(zh, dtype=np.float64)[G.cells][..., : self.nz + 1]
            require(np.all(np.isfinite(got)), "non-finite height")
            want = height_field(self.flow.rotate_back(G.C[G.cells], way * self.dt), self.nz)
            err = max(err, float(np.abs(got - want)[..., : self.nz].max()) / DZ_WAVE)
            ws = max(ws, float(np.abs(np.asarray(w, dtype=np.float64)[G.cells]).max()) * self.dt / ZS)
        return err, ws


def oracle_heights(doms, grids, cfg, hc):
    from fv3_oracle import d_sw as o_dsw
    from fv3_oracle import nh as o_nh

    col = o_dsw.get_column_namelist(cfg, hc.nz)
    zhs, wss = [], []
    for D, g, x in zip(doms, grids, hc.ins):
        zh, ws = x["zh"].copy(), np.zeros_like(x["zs"])
        o_nh.update_dz_d(D, cfg, col, g.dp_ref, x["zs"], zh, x["crx"].copy(), x["cry"].copy(), x["xfx"].copy(), x["yfx"].copy(), ws, hc.dt)
        zhs.append(zh), wss.append(ws)
    return zhs, wss


def measure_heights(shape):
    n, layout, ranks = SHAPES[shape]
    part, grids, doms, c = make(n, layout, ranks, DYN_NZ)
    hc = HeightCase(n, grids, c.RADIUS)
    err, ws = hc.errors(*oracle_heights(doms, grids, dyn_config(n, layout), hc))
    return {"dt": hc.dt, "zh": err, "ws": ws}


# ---------------------------------------------------------------------------------------------------------------------------
# pin 8: the Riemann solvers relax a column to the closed-form hydrostatic thickness
# ---------------------------------------------------------------------------------------------------------------------------
RIEM_N, RIEM_LEVELS, RIEM_DT, RELAX_DT, RELAX_CALLS, P_SURFACE = 12, (8, 79), 20.0, 200.0, 30, 1.0e5


class Columns:
    """Dry columns at rest over a flat surface, [i, j, nz + 1] arrays (the last level of a layer field repeats): interfaces log-spaced from ptop to
    about 1e5 Pa with every layer's log-thickness jittered by +-3 %, T = 250 + 30 sin(0.4 k), pt = T / pm^kappa, and the thickness the gas law asks
    for, delz_eq = -(delp / g) R pt pm^(kappa - 1), pm = delp / delta ln pe.  spoil: "exponent" builds delz_eq with kappa for kappa - 1, "midpoint"
    with the arithmetic mid-pressure for pm (the controls)."""

    def __init__(self, g, c, nz, spoil=None, seed=5, dtype=np.float64):
        rng = np.random.default_rng(seed)
        shape = np.asarray(g.lon_agrid).shape
        self.nz, self.ptop, self.c, self.dtype = nz, float(g.ptop), c, dtype
        dln = np.log(P_SURFACE / self.ptop) / nz * rng.uniform(0.97, 1.03, shape + (nz,))
        peln = np.log(self.ptop) + np.concatenate([np.zeros(shape + (1,)), np.cumsum(dln, 2)], 2)
        pe = np.exp(peln)
        pe[:, :, 0] = self.ptop
        delp = np.diff(pe, axis=2)
        pm = delp / np.diff(np.log(pe), axis=2)
        T = 250.0 + 30.0 * np.sin(0.4 * np.arange(nz))
        pt = T / pm**c.KAPPA
        pm_built = 0.5 * (pe[:, :, 1:] + pe[:, :, :-1]) if spoil == "midpoint" else pm
        delz = -(delp / c.GRAV) * c.RDGAS * pt * pm_built ** (c.KAPPA if spoil == "exponent" else c.KAPPA - 1.0)
        self.delp, self.pt, self.delz_eq, self.pe = delp, pt, delz, pe
        self.control = delz * rng.uniform(0.97, 1.03, delz.shape)

    def _pad(self, a):
        return np.concatenate([a, a[:, :, -1:]], 2).astype(self.dtype)

    def fields(self, delz):
        """the arguments of riem_solver3 / riem_solver_c for the thickness ``delz``, w = 0"""
        nz, shape = self.nz, delz.shape[:2]
        zh = np.concatenate([-np.cumsum(delz[:, :, ::-1], 2)[:, :, ::-1], np.zeros(shape + (1,))], 2)
        z3, z2 = np.zeros(shape + (nz + 1,), dtype=self.dtype), np.zeros(shape + (1,), dtype=self.dtype)
        return {"cappa": np.full_like(z3, self.c.KAPPA), "q_con": z3.copy(), "delp": self._pad(self.delp), "pt": self._pad(self.pt), "delz": self._pad(delz), "zh": zh.astype(self.dtype),
                "w": z3.copy(), "zs": z2.copy(), "ws": z2.copy(), "pe": z3.copy(), "ppe": z3.copy(), "pk3": z3.copy(), "pk": z3.copy(), "peln": z3.copy()}


def rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    require(np.all(np.isfinite(got)), "non-finite")
    return float(np.abs(got / want - 1.0).max())


def riem_figures(col, cells, solve, which):
    """The figures of pin 8 for one solver.  solve(fields, dt, last_call) runs one call in place on the dict of Columns.fields (riem_solver3: w, delz,
    zh, pe, peln, pk, pk3 out; riem_solver_c: zh holds heights in and the geopotential out, pef in "pe") and returns nothing.
    balanced: one call at RIEM_DT on delz_eq; control: the same call on delz_eq x uniform(0.97, 1.03); relax: RELAX_CALLS calls at RELAX_DT from the
    control, each fed the heights (and for riem_solver3 the w) of the one before."""
    nz, c = col.nz, col.c
    K = cells + (slice(0, nz),)
    K1 = cells + (slice(0, nz + 1),)
    out = {}

    def thickness(f):
        z = np.asarray(f["zh"], dtype=np.float64)
        return (z[:, :, 1:] - z[:, :, :-1])[K]

    def call(f, dt, last):
        """one call; riem_solver_c returns the geopotential, which goes back to heights for the next call and for ``thickness``"""
        solve(f, dt, last)
        if which == "c":
            f["zh"] = (np.asarray(f["zh"], dtype=np.float64) / c.GRAV).astype(col.dtype)

    hydro = col.ptop + np.concatenate([np.zeros(col.delp.shape[:2] + (1,)), np.cumsum(col.delp, 2)], 2)
    for name, dz in (("balanced", col.delz_eq), ("control", col.control)):
        f = col.fields(dz)
        call(f, RIEM_DT, 1)
        out[name + "_delz"] = rel(thickness(f), col.delz_eq[K])
        if which == "3":
            out[name + "_w"] = float(np.abs(np.asarray(f["w"], dtype=np.float64)[K]).max())
            out[name + "_delz_field"] = rel(np.asarray(f["delz"])[K], col.delz_eq[K])
            if name == "balanced":
                out["pe"], out["peln"] = rel(f["pe"][K1], hydro[K1]), rel(f["peln"][K1], np.log(hydro[K1]))
                out["pk"], out["pk3"] = rel(f["pk"][K1], hydro[K1] ** c.KAPPA), rel(f["pk3"][K1], hydro[K1] ** c.KAPPA)
        else:
            out[name + "_pef"] = rel(f["pe"][K1], hydro[K1])
    f = col.fields(col.control)
    for it in range(RELAX_CALLS):
        call(f, RELAX_DT, 0)
        if it == 9:
            out["relax10_delz"] = rel(thickness(f), col.delz_eq[K])
    out["relax_delz"] = rel(thickness(f), col.delz_eq[K])
    if which == "3":
        out["relax_w"] = float(np.abs(np.asarray(f["w"], dtype=np.float64)[K]).max())
    return out


def oracle_riem(D, col, which, p_fac):
    from fv3_oracle import nh as o_nh

    def solve3(f, dt, last):
        o_nh.riem_solver3(D, bool(last), dt, f["cappa"], col.ptop, f["zs"], f["ws"], f["delz"], f["q_con"], f["delp"], f["pt"], f["zh"], f["pe"], f["ppe"], f["pk3"], f["pk"], f["peln"], f["w"], p_fac)

    def solve_c(f, dt, last):
        o_nh.riem_solver_c(D, dt, f["cappa"], col.ptop, f["zs"], f["ws"], f["pt"], f["q_con"], f["delp"], f["zh"], f["pe"], f["w"], p_fac)

    return solve3 if which == "3" else solve_c


def _riem_need(label, fig, bound):
    def need(key, limit):
        lim = limit if bound is None else 4.0 * bound[key]
        require(np.isfinite(fig[key]) and fig[key] <= lim, f"{label}: {key} {fig[key]:.3e} above {lim:.3e}")

    return need


def check_balanced(label, fig, which, bound=None):
    """pin 8 (a) on the figures of riem_figures; ``bound`` (fp32): the oracle's np.float32 figures, held to 4 x each"""
    print(label, {k: f"{v:.2e}" for k, v in fig.items()})
    need = _riem_need(label, fig, bound)
    require(fig["control_delz"] > 5e-3, f"{label}: the control is not out of balance")
    need("balanced_delz", 1e-12)
    if which == "3":
        require(fig["control_w"] > 1.0, f"{label}: the control does not move")
        lim = 1e-9 * fig["control_w"] if bound is None else 4.0 * bound["balanced_w"]
        require(fig["balanced_w"] <= lim, f"{label}: |w| {fig['balanced_w']:.3e} on the balanced column above {lim:.3e}")
        need("balanced_delz_field", 1e-12)
        for k in ("pe", "peln", "pk", "pk3"):
            need(k, 1e-13)
    else:
        require(fig["control_pef"] > 5e-3, f"{label}: the control's pressure is hydrostatic")
        need("balanced_pef", 1e-12)


def check_relaxed(label, fig, which, bound=None):
    """pin 8 (b)"""
    need = _riem_need(label, fig, bound)
    need("relax_delz", 1e-12)
    if which == "3":
        need("relax_w", 1e-10)


def measure_riem(nz, dtype=np.float64, spoil=None):
    part, grids, doms, c = make(RIEM_N, (1, 1), (0,), nz)
    G = Geometry(grids[0])
    col = Columns(grids[0], c, nz, spoil, dtype=dtype)
    p_fac = dyn_config(RIEM_N, (1, 1), nz).p_fac
    return {w: riem_figures(col, G.cells, oracle_riem(doms[0], col, w, p_fac), w) for w in ("3", "c")}


def measure_dynamics():
    """the oracle's figures of pins 6 - 9: {pin: {...}}"""
    out = {"pin6": {}, "pin7": {}, "pin7_z": {}, "pin8": {}, "pin9": {}}
    for shape in SHAPES:
        m = measure_d_sw(shape)
        out["pin6"][shape], out["pin7"][shape] = m["pin6"], m["pin7"]
        out["pin9"][shape] = measure_heights(shape)
        print(shape, m, out["pin9"][shape])
    for shape in ("c24", "c48"):
        out["pin7_z"][shape] = measure_d_sw(shape, Z_AXIS, ranks=(0,))
        print("z axis", shape, out["pin7_z"][shape])
    for nz in RIEM_LEVELS:
        out["pin8"][f"nz{nz}"] = {"fp64": measure_riem(nz), "fp32": measure_riem(nz, np.float32)}
        print("pin8", nz, out["pin8"][f"nz{nz}"])
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the shapes, and the record mode: the numpy oracle's own error on every input, tests/golden/analytic_pins.json
# ---------------------------------------------------------------------------------------------------------------------------
# name: (cells per tile, layout, ranks)
SHAPES = {"c24": (24, (1, 1), tuple(range(6))), "c48": (48, (1, 1), tuple(range(6))), "c48_2x2": (48, (2, 2), (0, 3, 12, 15, 20)), "c65": (65, (1, 1), (0,))}
# name: (cells per tile, layout, hord, Courant number of the mean cell width, revolutions)
BELL_RUNS = {"c24_h6": (24, (1, 1), 6, 0.5, 1.0), "c24_h8": (24, (1, 1), 8, 0.5, 1.0), "c48_h6": (48, (1, 1), 6, 0.5, 1.0), "c48_h8": (48, (1, 1), 8, 0.5, 1.0),
             "c24_2x2_h8": (24, (2, 2), 8, 0.5, 1.0), "c24_cfl13_h8": (24, (1, 1), 8, 1.3, 1.0), "c24_quarter_h8": (24, (1, 1), 8, 0.5, 0.25)}
PGF_NZ = 8


def make(n, layout, ranks, nz):
    """(partitioner, grids, oracle domains) of some ranks"""
    from fv3_oracle.util import Dom
    from pace_amd.constants import get_constants
    from pace_amd.grid import make_grid
    from pace_amd.topology import CubedSpherePartitioner

    c = get_constants()
    part = CubedSpherePartitioner(n, layout)
    grids = [make_grid(part, r, nz=nz) for r in ranks]
    return part, grids, [Dom(g, c) for g in grids], c


def bell_run(name, part, grids, a):
    n, layout, hord, cfl, turn = BELL_RUNS[name]
    return BellCase(part, grids, a, int(round(bell_calls(n, cfl) * turn)), turn)


def bell_record(bc, tracers, n_split, hord):
    err, side = bc.errors(tracers)
    return {"hord": hord, "calls": bc.n_calls, "dt": bc.dt, "n_split": n_split, "axes": [list(f.axis) for f in bc.flows], "centre": list(bc.centre),
            "l2": {t: [err[(t, k)][0] for k in range(2)] for t in TRACERS}, "linf": {t: [err[(t, k)][1] for k in range(2)] for t in TRACERS},
            "min": {t: side[t]["min"] for t in TRACERS}, "max": {t: side[t]["max"] for t in TRACERS}, "mass": {t: side[t]["mass"] for t in TRACERS}}


def measure_single_call_pins(shape):
    """the oracle's errors of pins 1, 3 and 4 on one shape"""
    n, layout, ranks = SHAPES[shape]
    part, grids, doms, c = make(n, layout, ranks, 1)
    flow = Flow(c.RADIUS)
    dt = flux_dt(n, flow)
    fc = flux_case(grids, flow)
    xs, ys, _ = oracle_fluxes(doms, fc, dt)
    e_all, e_edge = flux_errors(fc, flow, dt, xs, ys)
    wc = wind_case(grids, flow)
    w_all, w_edge = wind_errors(wc, flow, *oracle_winds(doms, wc))
    cc = corner_case(grids)
    return {"pin1": {"all": e_all, "edge": e_edge, "dt": dt}, "pin3": {"all": w_all, "edge": w_edge}, "pin4": corner_errors(cc, oracle_corners(doms, cc))}


def pgf_scale(g, c, st):
    """S of the fp32 bound of pin 5a: dt rdx max |gz| max |delta_k pk3| / min (delta_k pk3 of a corner pair) -- the size of one term of the
    operator's bracket, of which the isentropic state leaves only the rounding"""
    G = Geometry(g)
    dk = np.diff(st["pk3"], axis=2)
    return PGF_DT * float(max(g.rdx[G.Y].max(), g.rdy[G.X].max())) * float(np.abs(st["gz"]).max()) * float(dk.max()) / (2.0 * float(dk.min()))


def measure_pgf_k():
    """K of the fp32 bound K eps32 S: 8 x the smallest integer with which the fp64 oracle meets K eps64 S on the isentropic C24 state"""
    part, grids, doms, c = make(24, (1, 1), range(6), PGF_NZ)
    k = 1
    for g, D in zip(grids, doms):
        st = resting_state(g, c)
        f = force(Geometry(g), *oracle_pgf(D, c, st), PGF_NZ)
        k = max(k, int(np.ceil(f / (np.finfo(np.float64).eps * pgf_scale(g, c, st)))))
    return 8 * k


def record(path=GOLDEN):
    out = {"flow": {"axis": list(AXIS), "period_days": 12.0}, "pin1": {}, "pin3": {}, "pin4": {}, "pin2": {}}
    for shape in SHAPES:
        for pin, v in measure_single_call_pins(shape).items():
            out[pin][shape] = v
        print(shape, {p: out[p][shape] for p in ("pin1", "pin3", "pin4")})
    for name, (n, layout, hord, cfl, turn) in BELL_RUNS.items():
        part, grids, doms, c = make(n, layout, range(6 * layout[0] * layout[1]), 2)
        bc = bell_run(name, part, grids, c.RADIUS)
        tr, ns = oracle_bell(doms, bc, hord)
        out["pin2"][name] = bell_record(bc, tr, ns, hord)
        print(name, out["pin2"][name]["l2"], "n_split", ns)
    out["pin5a"] = {"K": measure_pgf_k()}
    print("pin5a", out["pin5a"])
    out.update(measure_dynamics())
    write(out, path)
    return record_damping(path)


def record_dynamics(path=GOLDEN):
    """pins 6 - 9 alone, into the file as it stands (``--record dynamics``)"""
    out = recorded()
    out.update(measure_dynamics())
    return write(out, path)


def record_damping(path=GOLDEN):
    """pins 10, 12 and 13 (tests/damping_case.py) alone, into the file as it stands (``--record damping``)"""
    import damping_case

    out = recorded()
    out.update(damping_case.measure_damping())
    return write(out, path)


def record_steady(path=GOLDEN):
    """pins 16 - 19 (tests/steady_case.py) alone, into the file as it stands (``--record steady``)"""
    import steady_case

    out = recorded()
    out.update(steady_case.measure_steady())
    return write(out, path)


def write(out, path):
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    return out


def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    for p in (os.path.dirname(here), os.path.join(os.path.dirname(here), "oracle"), here):
        if p not in sys.path:
            sys.path.insert(0, p)
    if "--record" in sys.argv:
        record_dynamics() if "dynamics" in sys.argv else record_damping() if "damping" in sys.argv else record_steady() if "steady" in sys.argv else (record(), record_steady())
    else:
        print(__doc__)
