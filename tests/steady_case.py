"""Builders, exact solutions, checkers, oracle measurement and controls of tests/test_analytic_steady.py: the whole acoustic call and the whole model step
on steady analytic atmospheres (pins 16 - 19), under the ground rule of tests/analytic_case.py -- inputs and expected values come from corner positions, cell
centres, the sphere radius, the hybrid coefficients ak / bk and closed-form functions of position; no metric array that a kernel reads enters either (the upwind
area of pin 17 is pin 6's stated exception).

State A: solid-body rotation V = U0 axis x p (analytic_case.Flow), T = T0 = 300 K, w = 0, phis = 0, q_con = 0, dry cappa, in gradient-wind balance:
  ln ps = ln p0 - (a OMEGA U0 (axis . z) + U0^2 / 2) s^2 / (R T0),  s = p . axis,  p0 = 1e5 Pa
an exact steady solution for the axis z with the project's constants (A-z, Coriolis on) and for analytic_case.AXIS on a planet that does not turn (A-oblique,
OMEGA = 0 in the constants that make the grids, the oracle's domains and the stencil factory).
State B: the same isothermal atmosphere at rest over analytic_case.terrain, ps = p0 exp(-phis / (R T0)).
Both discretely: delp_k = dak + dbk ps, delz_k = -(R T0 / g) d ln pe (exact between two pressures of an isothermal column and the Riemann solvers' own
equilibrium of pin 8), pt = T0 / pkz, pkz = pm^kappa, pm = delp / d ln pe; pe, peln, pk from ps; u, v from Flow.d_grid.
"""
import dataclasses

import numpy as np

import analytic_case as ac

P0, T0 = 1.0e5, 300.0
EPS32 = float(np.finfo(np.float32).eps)
NZ, NZ_FINE = 8, 16
N_SPLIT = 3
STEADY_OFF = dict(ac.DSW_OFF, rf_fast=False)  # every damping term off, as pins 6 and 7, and no Rayleigh damping
STATE_3D = "u v w ua va uc vc delp delz pt pe pk peln pkz q_con omga cappa mfxd mfyd cxd cyd diss_estd".split()
WIND_CLASSES = tuple(ac.CLASS_KEYS.values())
CELL_FIELDS = ("delp", "pt", "delz")
PIN16_FIGURES = WIND_CLASSES + ("core",) + CELL_FIELDS + ("w",)  # core: core_mask, the faces the tile-edge terms have not reached
# name: (cells per tile, layout): the whole cube every time -- the call exchanges halos
CUBES = {"c24": (24, (1, 1)), "c48": (48, (1, 1)), "c48_2x2": (48, (2, 2)), "c65": (65, (1, 1)), "c24_2x2": (24, (2, 2)), "c12": (12, (1, 1))}
AXES = {"z": ac.Z_AXIS, "oblique": tuple(ac.AXIS)}


def constants_for(which):
    """the project's constants for the z axis and for state B; OMEGA = 0 for the oblique axis"""
    from pace_amd.constants import get_constants

    c = get_constants()
    return dataclasses.replace(c, OMEGA=0.0) if which == "oblique" else c


def make_cube(shape, nz, which):
    """(partitioner, grids of every rank, constants)"""
    from pace_amd.grid import make_grid
    from pace_amd.topology import CubedSpherePartitioner

    n, layout = CUBES[shape]
    c = constants_for(which)
    part = CubedSpherePartitioner(n, layout)
    return part, [make_grid(part, r, nz=nz, constants=c) for r in range(part.total_ranks)], c


def config_for(shape, nz, n_split=N_SPLIT, damping=False, **kw):
    from pace_amd.config import AcousticDynamicsConfig

    n, layout = CUBES[shape]
    return AcousticDynamicsConfig(**dict(dict(npx=n + 1, npy=n + 1, npz=nz, layout=layout, n_split=n_split, **({} if damping else STEADY_OFF)), **kw))


# ---------------------------------------------------------------------------------------------------------------------------
# the steady states
# ---------------------------------------------------------------------------------------------------------------------------
def _pad(a):
    return np.concatenate([a, a[:, :, -1:]], 2)


def ln_ps_rotation(p, flow, c, coriolis=True):
    """gradient-wind balance of the rotation under T0; coriolis=False leaves the Coriolis term out (a control)"""
    s = np.sum(p * flow.axis, -1)
    rot = flow.a * c.OMEGA * flow.u0 * flow.axis[2] if coriolis else 0.0
    return np.log(P0) - (rot + 0.5 * flow.u0**2) * s**2 / (c.RDGAS * T0)


def ps_terrain(p, c):
    return P0 * np.exp(-c.GRAV * ac.terrain(p) / (c.RDGAS * T0))


def columns(g, c, ps):
    """the isothermal columns under ps [i, j]: {delp, delz, pt, pkz [i, j, nz]; pe, peln, pk [i, j, nz + 1]}"""
    pe = g.ak[None, None, :] + g.bk[None, None, :] * ps[:, :, None]
    peln = np.log(pe)
    delp, dln = np.diff(pe, axis=2), np.diff(peln, axis=2)
    pkz = (delp / dln) ** c.KAPPA
    return {"delp": delp, "delz": -(c.RDGAS * T0 / c.GRAV) * dln, "pt": T0 / pkz, "pkz": pkz, "pe": pe, "peln": peln, "pk": pe**c.KAPPA}


def steady_state(g, G, c, flow=None, coriolis=True, way=1.0, delz_factor=1.0):
    """(the oracle's / DycoreState's arrays [i, j, nz + 1] of one rank, phis [i, j, 1]).  flow None: state B.  way = -1 turns the wind the other way under the
    same ps, delz_factor stretches every layer (the controls)."""
    nz = g.nz
    shape = G.C.shape[:2] + (nz + 1,)
    st = {k: np.zeros(shape) for k in STATE_3D}
    if flow is None:
        ps, phis = ps_terrain(G.C, c), c.GRAV * ac.terrain(G.C)
    else:
        ps, phis = np.exp(ln_ps_rotation(G.C, flow, c, coriolis)), np.zeros(shape[:2])
        u, v = flow.d_grid(G)
        st["u"], st["v"] = way * ac.levels(u, nz + 1), way * ac.levels(v, nz + 1)
    col = columns(g, c, ps)
    for k in ("delp", "delz", "pt", "pkz"):
        st[k] = _pad(col[k])
    for k in ("pe", "peln", "pk"):
        st[k] = col[k].copy()
    st["delz"] *= delz_factor
    st["cappa"][...] = c.KAPPA
    return st, phis[:, :, None]


class SteadyCase:
    """one cube of state A (which = "z" | "oblique") or B (which = "terrain"): per rank the geometry G[r], the initial state ins[r] and phis[r]"""

    def __init__(self, shape, nz=NZ, which="oblique", **spoil):
        self.shape, self.nz, self.which = shape, nz, which
        self.part, self.grids, self.c = make_cube(shape, nz, which)
        self.n = CUBES[shape][0]
        self.flow = None if which == "terrain" else ac.Flow(self.c.RADIUS, AXES[which])
        self.dt = ac.dyn_dt(self.n, self.flow or ac.Flow(self.c.RADIUS))
        self.G = [ac.Geometry(g) for g in self.grids]
        both = [steady_state(g, G, self.c, self.flow, **spoil) for g, G in zip(self.grids, self.G)]
        self.ins, self.phis = [b[0] for b in both], [b[1] for b in both]

    def copy_ins(self):
        return [{k: v.copy() for k, v in s.items()} for s in self.ins]

    # -------------------------------------------------------------------------------------------------------------------
    def balance_term(self):
        """max |(zeta + f) V| of the rotation, the largest exact term of the wind's balance: zeta = 2 omega s, f = 2 OMEGA p_z, |V| = U0 sqrt(1 - s^2)"""
        fl, top = self.flow, 0.0
        for G in self.G:
            p = G.C[G.cells]
            s = np.sum(p * fl.axis, -1)
            top = max(top, float(np.abs((2.0 * fl.omega * s + 2.0 * self.c.OMEGA * p[..., 2]) * fl.u0 * np.sqrt(np.maximum(0.0, 1.0 - s * s))).max()))
        return top

    def tendencies(self, outs, n_split, n_calls=1):
        """pin 16's figures of the states ``outs`` after n_calls calls of n_split sub-steps: {class: wind tendency / max |(zeta + f) V|}, {delp, pt, delz:
        tendency / (max |x| U0 / a)}, w: / (U0^2 / a)"""
        fl, nz = self.flow, self.nz
        T = n_calls * n_split * self.dt
        fig = dict.fromkeys(PIN16_FIGURES, 0.0)
        top = dict.fromkeys(CELL_FIELDS, 0.0)
        for r, (G, x, o) in enumerate(zip(self.G, self.ins, outs)):
            o = {k: np.asarray(o[k], dtype=np.float64) for k in ("u", "v", "w") + CELL_FIELDS}
            cu, cv = ac.face_classes(G)
            mu, mv = core_mask(self.part, r, G.g)
            for name, F, cls, core in (("u", G.Y, cu, mu), ("v", G.X, cv, mv)):
                d = np.abs(o[name][F][..., :nz] - x[name][F][..., :nz]) / T
                ac.require(np.all(np.isfinite(d)), f"{name}: non-finite")
                if core.any():
                    fig["core"] = max(fig["core"], float(d[core].max()))
                for cl, key in ac.CLASS_KEYS.items():
                    if (cls == cl).any():
                        fig[key] = max(fig[key], float(d[cls == cl].max()))
            for k in CELL_FIELDS:
                d = np.abs(o[k][G.cells][..., :nz] - x[k][G.cells][..., :nz]) / T
                ac.require(np.all(np.isfinite(d)), f"{k}: non-finite")
                fig[k], top[k] = max(fig[k], float(d.max())), max(top[k], float(np.abs(x[k][G.cells][..., :nz]).max()))
            ac.require(np.all(np.isfinite(o["w"][G.cells])), "w: non-finite")
            fig["w"] = max(fig["w"], float(np.abs(o["w"][G.cells][..., :nz]).max()) / T)
        bal = self.balance_term()
        for key in WIND_CLASSES + ("core",):
            fig[key] /= bal
        for k in CELL_FIELDS:
            fig[k] /= top[k] * fl.omega
        fig["w"] /= fl.u0**2 / fl.a
        return fig

    def store_scale(self, n_split):
        """max |x| / (n_split dt) in the unit of each figure of pin 16: what one rounding of the stored field is worth, per eps"""
        top, T = self.field_tops(), n_split * self.dt
        scale = {k: top["wind"] / T / self.balance_term() for k in WIND_CLASSES + ("core",)}
        scale.update({k: 1.0 / T / self.flow.omega for k in CELL_FIELDS})
        scale["w"] = top["w"] / T / (self.flow.u0**2 / self.flow.a)
        return scale

    def field_tops(self):
        """max |x| of every prognostic field over the compute domain (the fp32 addend's scale)"""
        top = {}
        for k, name in (("u", "wind"), ("v", "wind"), ("w", "w")) + tuple((f, f) for f in CELL_FIELDS):
            for G, x in zip(self.G, self.ins):
                top[name] = max(top.get(name, 0.0), float(np.abs(x[k][G.cells]).max()))
        return top

    # -------------------------------------------------------------------------------------------------------------------
    def accumulator_errors(self, outs, n_split):
        """pin 17: max |mfxd - n_split delp(face mid-point) swept| / max |.|, |cxd upwind area - n_split swept| / max |.|, likewise y"""
        fl, nz, c = self.flow, self.nz, self.c
        err, top = dict.fromkeys(("mfx", "mfy", "cx", "cy"), 0.0), dict.fromkeys(("mfx", "mfy", "cx", "cy"), 0.0)
        for g, G, o in zip(self.grids, self.G, outs):
            o = {k: np.asarray(o[k], dtype=np.float64)[:, :, :nz] for k in ("mfxd", "mfyd", "cxd", "cyd")}
            sx, sy = fl.swept(G, self.dt)
            ux, uy = ac.upwind_area(g, o["cxd"], o["cyd"])
            for k, name, cname, m, s, up, F in (("mfx", "mfxd", "cxd", G.mx, sx, ux, G.X), ("mfy", "mfyd", "cyd", G.my, sy, uy, G.Y)):
                ac.require(np.all(np.isfinite(o[name][F])) and np.all(np.isfinite(o[cname][F])), f"{name} / {cname}: non-finite")
                delp = columns(g, c, np.exp(ln_ps_rotation(m[F], fl, c)))["delp"]
                want = n_split * delp * s[F][..., None]
                err[k], top[k] = max(err[k], float(np.abs(o[name][F] - want).max())), max(top[k], float(np.abs(want).max()))
                kc = "c" + k[-1]
                err[kc] = max(err[kc], float(np.abs((o[cname] * up)[F] - n_split * s[F][..., None]).max()))
                top[kc] = max(top[kc], float(n_split * np.abs(s[F]).max()))
        return {k: err[k] / top[k] for k in err}

    def rest_figures(self, outs, n_split, n_calls):
        """pin 19 (state B): max |u|, |v|, |w| over the elapsed time [m/s^2]; delp, pt: max |change| / max |x| (no time scale: the state is at rest)"""
        nz, T = self.nz, n_calls * n_split * self.dt
        fig = dict.fromkeys(("u", "v", "w", "delp", "pt"), 0.0)
        for G, x, o in zip(self.G, self.ins, outs):
            for k, F in (("u", G.Y), ("v", G.X), ("w", G.cells)):
                d = np.abs(np.asarray(o[k], dtype=np.float64)[F][..., :nz])
                ac.require(np.all(np.isfinite(d)), f"{k}: non-finite")
                fig[k] = max(fig[k], float(d.max()) / T)
            for k in ("delp", "pt"):
                a, b = np.asarray(o[k], dtype=np.float64)[G.cells][..., :nz], x[k][G.cells][..., :nz]
                ac.require(np.all(np.isfinite(a)), f"{k}: non-finite")
                fig[k] = max(fig[k], float(np.abs(a - b).max() / np.abs(b).max()))
        return fig


# ---------------------------------------------------------------------------------------------------------------------------
# the oracle's call
# ---------------------------------------------------------------------------------------------------------------------------
def oracle_call(sc, cfg, n_calls=1, states=None, before_call=None):
    """OracleAcousticDynamics on copies of the case's state: the states after n_calls calls of cfg.n_split sub-steps of sc.dt.  before_call(states, dyn, n)
    may spoil them first (the poison derivation)."""
    from fv3_oracle.dyn_core import OracleAcousticDynamics

    st = sc.copy_ins() if states is None else states
    dyn = OracleAcousticDynamics(sc.part, sc.grids, cfg, sc.c, [p.copy() for p in sc.phis])
    for n in range(n_calls):
        if before_call is not None:
            before_call(st, dyn, n)
        dyn(st, cfg.n_split * sc.dt, n_map=n + 1)
    return st


def measure_pin16_17(shape, which, nz=NZ, n_split=N_SPLIT, **spoil):
    sc = SteadyCase(shape, nz, which, **spoil)
    outs = oracle_call(sc, config_for(shape, nz, n_split))
    return sc, outs, {"dt": sc.dt, **sc.tendencies(outs, n_split)}, {"dt": sc.dt, **sc.accumulator_errors(outs, n_split)}


def core_mask(part, r, g):
    """(u faces [nx, ny + 1], v faces [nx + 1, ny]) a quarter of the tile's width or more from every tile edge: what the tile-edge terms of pin 7, carried by the
    sound waves of the sub-steps, have not reached"""
    n = part.nx_tile
    ox, oy = part.origin(r)
    ci, cj = ox + np.arange(g.nx), oy + np.arange(g.ny)  # cell lines
    pi, pj = ox + np.arange(g.nx + 1), oy + np.arange(g.ny + 1)  # corner lines
    cell = lambda i: np.minimum(i, n - 1 - i) >= n // 4  # noqa: E731
    corner = lambda i: np.minimum(i, n - i) >= n // 4  # noqa: E731
    return np.outer(cell(ci), corner(pj)), np.outer(corner(pi), cell(cj))


# ---------------------------------------------------------------------------------------------------------------------------
# the library's call
# ---------------------------------------------------------------------------------------------------------------------------
def library_call(backend, sc, cfg, n_calls=1, dtype=None, before_call=None):
    """fv3_acoustic_step on the case's state, every rank of the cube in one context: the states after n_calls calls.  before_call(state, dyn, n): see the poison"""
    import torch

    from pace_amd._testing import stencil_factory_for
    from pace_amd.dyn_core import AcousticDynamics, DycoreState
    from pace_amd.halo import Layout

    sf = stencil_factory_for(backend)(sc.grids, cfg, sc.c, dtype=dtype or torch.float64)
    st = DycoreState.from_arrays(sf.quantity_factory, [dict(s, phis=p) for s, p in zip(sc.ins, sc.phis)])
    dyn = AcousticDynamics(Layout(sc.part, 1, 0), sc.grids, sf, config=cfg, phis=st.phis, state=st)
    for n in range(n_calls):
        if before_call is not None:
            before_call(st, dyn, n)
        dyn(st, cfg.n_split * sc.dt, n_map=n + 1)
    if backend != "hostemu":
        torch.cuda.synchronize()
    out = st.to_arrays()
    sf.close()
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# pin 18: DynamicalCore.step_dynamics on state A-oblique
# ---------------------------------------------------------------------------------------------------------------------------
K_SPLIT, STEP_N_SPLIT, STEPS, Q0 = 2, 2, 2, 2.0e-3
TRACER_NAMES = ("tracer0", "tracer1", "tracer2")  # the harness's names: a constant, q0 (1 + 0.5 P2(s)), and that times a profile linear in pressure
LINEAR_P = (0.4, 6.0e-6)  # alpha + beta p_mid: 0.4 at the top, 1.0 at 1e5 Pa
STEP_FIGURES = ("pt", "ps", "omga", "w", "delp", "ua", "va", "pkz") + TRACER_NAMES


def tracer_fields(p, col, flow):
    s = np.sum(p * flow.axis, -1)[..., None]
    wave = Q0 * (1.0 + 0.5 * 0.5 * (3.0 * s * s - 1.0)) + 0.0 * col["delp"]
    return {"tracer0": np.full_like(col["delp"], Q0), "tracer1": wave, "tracer2": wave * (LINEAR_P[0] + LINEAR_P[1] * 0.5 * (col["pe"][..., 1:] + col["pe"][..., :-1]))}


class StepCase(SteadyCase):
    """state A-oblique as DynamicalCore.step_dynamics takes it: pt is the temperature T0; three tracers; dt_atmos = k_split n_split dt"""

    def __init__(self, shape, nz=NZ):
        super().__init__(shape, nz, "oblique")
        self.dt_atmos = K_SPLIT * STEP_N_SPLIT * self.dt
        self.cols = [columns(g, self.c, np.exp(ln_ps_rotation(G.C, self.flow, self.c))) for g, G in zip(self.grids, self.G)]
        self.tracers = [{k: _pad(v) for k, v in tracer_fields(G.C, col, self.flow).items()} for G, col in zip(self.G, self.cols)]
        for s in self.ins:
            s["pt"][...] = T0

    def harness_kw(self, damping):
        return dict(nz=self.nz, layout=CUBES[self.shape][1], dt_atmos=self.dt_atmos, k_split=K_SPLIT, n_split=STEP_N_SPLIT, n_tracers=3, hord_tr=8, remap=True, temperature=True,
                    latlon_winds=True, constants=self.c, config_overrides=None if damping else dict(STEADY_OFF))

    def step_errors(self, outs, tracers, ps):
        """every figure of pin 18: max |got - closed form| over the compute cells, relative to the closed form's largest value (omga: to max (delp / |delz|) U0, w and
        the winds: to U0)"""
        fl, nz = self.flow, self.nz
        fig = dict.fromkeys(STEP_FIGURES, 0.0)
        for G, col, x, q0, o, q, p in zip(self.G, self.cols, self.ins, self.tracers, outs, tracers, ps):
            c, K = G.cells, slice(0, nz)
            get = lambda a: np.asarray(a, dtype=np.float64)[c][..., K]  # noqa: E731
            lon, lat = np.asarray(G.g.lon_agrid)[c], np.asarray(G.g.lat_agrid)[c]
            east = np.stack([-np.sin(lon), np.cos(lon), np.zeros_like(lon)], -1)
            north = np.stack([-np.sin(lat) * np.cos(lon), -np.sin(lat) * np.sin(lon), np.cos(lat)], -1)
            V = fl.wind(G.C[c])
            want = {"pt": (np.full_like(col["delp"][c], T0), T0), "delp": (col["delp"][c], np.abs(col["delp"][c]).max()), "pkz": (col["pkz"][c], np.abs(col["pkz"][c]).max()),
                    "w": (0.0, fl.u0), "omga": (0.0, float(np.abs(col["delp"][c] / col["delz"][c]).max()) * fl.u0),
                    "ua": (np.sum(V * east, -1)[..., None], fl.u0), "va": (np.sum(V * north, -1)[..., None], fl.u0)}
            for k, (w_, scale) in want.items():
                got = get(o[k])
                ac.require(np.all(np.isfinite(got)), f"{k}: non-finite")
                fig[k] = max(fig[k], float(np.abs(got - w_).max()) / scale)
            got = np.asarray(p, dtype=np.float64).reshape(G.C.shape[:2])[c]
            ac.require(np.all(np.isfinite(got)), "ps: non-finite")
            fig["ps"] = max(fig["ps"], float(np.abs(got - col["pe"][c][..., nz]).max()) / P0)
            for k in TRACER_NAMES:
                got = get(q[k])
                ac.require(np.all(np.isfinite(got)), f"{k}: non-finite")
                fig[k] = max(fig[k], float(np.abs(got - q0[k][c][..., K]).max() / np.abs(q0[k][c][..., K]).max()))
        return fig


def oracle_step(sc, damping=False, skip_bookend=False):
    """the oracle's step_dynamics between numpy bookends (tests/thermo_reference.py), then the cubed-to-latlon winds (tests/c2l_reference.py): STEPS steps.
    skip_bookend hands T0 in as the loop's pt (a control).  Returns (states, tracers, ps) per rank."""
    import thermo_reference as th
    from c2l_reference import cubed_to_latlon
    from fv3_oracle.dyn_core import OracleAcousticDynamics
    from fv3_oracle.step_dynamics import step_dynamics

    nz = sc.nz
    cfg = config_for(sc.shape, nz, STEP_N_SPLIT, damping, k_split=K_SPLIT, dt_atmos=sc.dt_atmos)
    st, tr = sc.copy_ins(), [{k: v.copy() for k, v in t.items()} for t in sc.tracers]
    dyn = OracleAcousticDynamics(sc.part, sc.grids, cfg, sc.c, [p.copy() for p in sc.phis])
    ps = [None] * len(st)
    for _ in range(STEPS):
        if not skip_bookend:
            for s in st:
                s["pt"], s["pkz"] = th.pt_from_temperature(s["pt"], s["delp"], s["delz"], s["q_con"], s["cappa"])
        step_dynamics(dyn, sc.c, st, tr, sc.dt_atmos, K_SPLIT, hord_tr=8)
        for r, s in enumerate(st):
            s["pt"], _, s["omga"] = th.temperature_from_pt(s["pt"], s["pkz"], s["delp"], s["delz"], s["q_con"], s["cappa"], s["w"])
            ps[r] = s["pe"][:, :, nz].copy()
        dyn.ex.vector([s["u"] for s in st], [s["v"] for s in st], "dgrid")
        for s, g in zip(st, sc.grids):
            ua, va = cubed_to_latlon(s["u"], s["v"], g, order=cfg.c2l_ord)
            s["ua"][ac.NH : ac.NH + g.nx, ac.NH : ac.NH + g.ny, :nz], s["va"][ac.NH : ac.NH + g.nx, ac.NH : ac.NH + g.ny, :nz] = ua, va
    return st, tr, ps


def library_step(backend, sc, damping=False, dtype=None):
    """DycoreHarness(temperature=True): STEPS steps of DynamicalCore.step_dynamics on the case's state.  Returns (states, tracers, ps) per rank."""
    import torch

    from pace_amd._testing import harness_for
    from pace_amd.dyn_core import STATE_NAMES

    h = harness_for(backend)(sc.n, dtype=dtype or torch.float64, **sc.harness_kw(damping))
    R = range(len(sc.grids))
    for r in R:
        for n in STATE_NAMES:
            getattr(h.state, n).set_numpy(sc.ins[r][n], r)
        h.state.phis.set_numpy(sc.phis[r], r)
        for k in TRACER_NAMES:
            h.tracers[k].set_numpy(sc.tracers[r][k], r)
    h.dyn._bind(h.state)  # the surface height the call keeps is the new phis'
    for _ in range(STEPS):
        h.step()
    h.synchronize()
    out = ([{n: getattr(h.state, n).numpy(r) for n in STATE_NAMES} for r in R], [{k: h.tracers[k].numpy(r) for k in TRACER_NAMES} for r in R], [h.dycore.ps.numpy(r) for r in R])
    h.close()
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# pin 19: state B through three calls
# ---------------------------------------------------------------------------------------------------------------------------
REST_CALLS, REST_N_SPLIT = 3, 2


# ---------------------------------------------------------------------------------------------------------------------------
# the poison: the call reads nothing it has not been given
# ---------------------------------------------------------------------------------------------------------------------------
WORKSPACE = ("gz", "zh", "pkc", "pk3", "crx", "cry", "xfx", "yfx", "divgd", "ut", "vt", "delpc", "ptc", "dsw_delpc", "ws3", "wsd")  # every fv3_workspace field but heat_source and zs
CONTENDERS = ("ua", "va", "uc", "vc", "omga", "diss_estd", "mfxd", "mfyd", "cxd", "cyd")
PROGNOSTIC = ("u", "v", "w", "delp", "pt", "delz", "pe", "pk", "peln", "pkz", "mfxd", "mfyd", "cxd", "cyd")
POISON_SHAPE, DERIVE_SHAPE, POISON_CALLS = "c24_2x2", "c12", 2
# The state fields the sequence stores before it reads.  Derivation (derive_poison_list, the oracle alone, tests/test_analytic_steady.py asserts that it still gives
# this list): a contender is on the list if and only if the oracle's two calls on pin 16's A-oblique case (at C12 with three levels and C24's sub-step: the order of stores and reads does
# not depend on the size), n_split = 3, with that field filled with
# NaN before each call, leave every prognostic output free of NaN on the compute cells and bitwise equal to the unpoisoned run.  All ten contenders pass:
# c_sw stores ua, va, uc, vc and omga before p_grad_c, riem_solver_c and d_sw read them; every call zeroes the accumulators and diss_estd first.
POISON_STATE = ("ua", "va", "uc", "vc", "omga", "diss_estd", "mfxd", "mfyd", "cxd", "cyd")


def compute_cells(name, g):
    from helpers import compute_slice

    return compute_slice(name, g.nx, g.ny, g.nz)


def same_prognostics(sc, a, b, names=PROGNOSTIC):
    """None if the prognostic outputs of runs a and b are free of NaN and bitwise equal on the compute cells, otherwise what differs first"""
    for r, g in enumerate(sc.grids):
        for n in names:
            sl = compute_cells(n, g)
            x, y = np.asarray(a[r][n])[sl], np.asarray(b[r][n])[sl]
            if not np.all(np.isfinite(x)):
                return f"{n} rank {r}: non-finite"
            if not np.array_equal(x, y):
                return f"{n} rank {r}: differs by {float(np.abs(x - y).max()):.3e}"
    return None


def derive_poison_list(contenders=CONTENDERS):
    """the oracle-side derivation of POISON_STATE"""
    sc = SteadyCase(DERIVE_SHAPE, ac.DYN_NZ, "oblique")
    sc.dt = ac.dyn_dt(CUBES[POISON_SHAPE][0], sc.flow)  # the sub-step of the library's case (dyn_dt of C12 is beyond the loop's stability)
    cfg = config_for(DERIVE_SHAPE, ac.DYN_NZ, N_SPLIT)
    clean = oracle_call(sc, cfg, POISON_CALLS)
    keep = []
    for name in contenders:
        def spoil(states, dyn, n, name=name):
            for s in states:
                s[name][...] = np.nan

        with np.errstate(all="ignore"):
            if same_prognostics(sc, oracle_call(sc, cfg, POISON_CALLS, before_call=spoil), clean, [p for p in PROGNOSTIC if p != name]) is None:
                keep.append(name)
    return tuple(keep)


def library_poison(state, dyn, n):
    """before_call of library_call: NaN over the whole storage of every workspace field and of every state field on POISON_STATE"""
    cs = dyn.cgrid_shallow_water_lagrangian_dynamics
    work = dict(gz=dyn._gz, zh=dyn._zh, pkc=dyn._pkc, pk3=dyn._pk3, crx=dyn._crx, cry=dyn._cry, xfx=dyn._xfx, yfx=dyn._yfx, divgd=dyn._divgd, ut=dyn._ut, vt=dyn._vt,
                delpc=cs.delpc, ptc=cs.ptc, dsw_delpc=dyn._vt_scratch, ws3=dyn._ws3, wsd=dyn._wsd)
    for k in WORKSPACE:
        work[k].storage.fill_(float("nan"))
    for k in POISON_STATE:
        getattr(state, k).storage.fill_(float("nan"))


# ---------------------------------------------------------------------------------------------------------------------------
# the record: the oracle's figures of pins 16 - 19 (python tests/analytic_case.py --record steady)
# ---------------------------------------------------------------------------------------------------------------------------
PIN16_RUNS = {"c24": ("c24", NZ, N_SPLIT), "c48": ("c48", NZ, N_SPLIT), "c65": ("c65", NZ, N_SPLIT), "c24_n1": ("c24", NZ, 1), "c48_l16": ("c48", NZ_FINE, N_SPLIT)}
REST_RUNS = {"c24": ("c24", NZ), "c48_l16": ("c48", NZ_FINE)}


def measure_rest(run):
    shape, nz = REST_RUNS[run]
    sc = SteadyCase(shape, nz, "terrain")
    outs = oracle_call(sc, config_for(shape, nz, REST_N_SPLIT), REST_CALLS)
    return {"dt": sc.dt, **sc.rest_figures(outs, REST_N_SPLIT, REST_CALLS)}


def measure_step(shape, damping):
    sc = StepCase(shape)
    return {"dt": sc.dt, **sc.step_errors(*oracle_step(sc, damping))}


def ratios(coarse, fine):
    return {k: (coarse[k] / fine[k] if fine[k] > 0.0 else 0.0) for k in coarse if k != "dt"}


def round_off_k(fig, scale):
    """pin 5a's K: 8 x the smallest integer with which the fp64 figure meets K eps64 scale"""
    return 8 * max(1, int(np.ceil(fig / (np.finfo(np.float64).eps * scale))))


def measure_steady(only_c24=False):
    """{pin16, pin17, pin18, pin19}; only_c24: the entries the freshness test re-measures"""
    out = {"pin16": {w: {} for w in AXES}, "pin17": {w: {} for w in AXES}, "pin18": {"off": {}, "default": {}}, "pin19": {}}
    for which in AXES:
        for run, (shape, nz, n_split) in PIN16_RUNS.items():
            if only_c24 and shape != "c24":
                continue
            case, _, p16, p17 = measure_pin16_17(shape, which, nz, n_split)
            out["pin16"][which][run], out["pin17"][which][run] = p16, p17
            if run == "c24" and not only_c24:  # fp32: the figures below 1e3 eps32 max |x| / (n_split dt), and pin 5a's K for each
                scale = case.store_scale(n_split)
                out["pin16"][which]["fp32_K"] = {k: round_off_k(p16[k], scale[k]) for k in PIN16_FIGURES if scale[k] > 0.0 and p16[k] < 1.0e3 * EPS32 * scale[k]}
            print("pin16", which, run, p16, "\npin17", which, run, p17)
        if not only_c24:
            for pin in ("pin16", "pin17"):
                rec = out[pin][which]
                rec["ratio_c24_c48"], rec["ratio_c24_c48_l16"] = ratios(rec["c24"], rec["c48"]), ratios(rec["c24"], rec["c48_l16"])
                print(pin, which, "ratios", rec["ratio_c24_c48"], rec["ratio_c24_c48_l16"])
    for run in REST_RUNS:
        if only_c24 and run != "c24":
            continue
        out["pin19"][run] = measure_rest(run)
        print("pin19", run, out["pin19"][run])
    if only_c24:
        return out
    out["pin19"]["ratio_c24_c48_l16"] = ratios(out["pin19"]["c24"], out["pin19"]["c48_l16"])
    for variant, damping in (("off", False), ("default", True)):
        rec = out["pin18"][variant]
        for shape in ("c24", "c48"):
            rec[shape] = measure_step(shape, damping)
            print("pin18", variant, shape, rec[shape])
        rec["ratio_c24_c48"] = ratios(rec["c24"], rec["c48"])
        print("pin18", variant, "ratios", rec["ratio_c24_c48"])
    return out
