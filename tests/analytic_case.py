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

``python tests/analytic_case.py --record`` measures the numpy oracle's error on the same inputs and writes tests/golden/analytic_pins.json;
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
        record()
    else:
        print(__doc__)
