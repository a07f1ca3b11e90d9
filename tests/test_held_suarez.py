"""HeldSuarezForcing (fv3_held_suarez_tend, pace_amd/csrc/fv3_hs.hip): parity with the numpy restatement of the paper (tests/hs_reference.py)
on a JW2006 state plus noise, closed-form pins that need no reference, the relaxation law over n applications, sentinels, fp32 and the
argument refusals."""
import numpy as np
import pytest
import torch

import hs_reference as ref
from pace_amd import lib as _lib
from pace_amd._testing import stencil_factory_for
from pace_amd.config import AcousticDynamicsConfig
from pace_amd.constants import get_constants
from pace_amd.grid import make_grid
from pace_amd.init import baroclinic_state, jw_temperature, jw_zonal_wind
from pace_amd.stencils import HeldSuarezConfig, HeldSuarezForcing
from pace_amd.topology import CubedSpherePartitioner

NH = 3
EPS = {torch.float64: 2.0**-52, torch.float32: 2.0**-23}
CELL = ("x", "y", "z")


def _cube(backend, nx_tile, layout, nz, dtype=torch.float64, **cfg_kw):
    if backend == "hostemu" and dtype == torch.float32:
        from pace_amd import build

        build.build(32, hostemu=True, verbose=False)
    c = get_constants()
    part = CubedSpherePartitioner(nx_tile, layout)
    cfg = AcousticDynamicsConfig(npx=nx_tile + 1, npy=nx_tile + 1, npz=nz, layout=layout, **cfg_kw)
    grids = [make_grid(part, r, nz=nz) for r in range(part.total_ranks)]
    sf = stencil_factory_for(backend)(grids, cfg, c, dtype=dtype)
    return c, part, grids, sf


def _sync(sf):
    if not sf.hostemu:
        torch.cuda.synchronize()


def _jw_inputs(grids, c, seed=5):
    """Per rank: ua, va, T, delp [ni, nj, nz + 1] -- the JW2006 zonal wind, temperature and layer thickness at the cell centres plus
    seeded noise (2 m/s, 2 K, 0.2 % of delp), everywhere in the storage (halo and pad level included: the kernel must not read them, the
    sentinel checks compare them afterwards)."""
    out = []
    g0 = grids[0]
    pe = g0.ak + g0.bk * 1.0e5
    eta = 0.5 * (pe[1:] + pe[:-1]) / 1.0e5
    for r, g in enumerate(grids):
        rng = np.random.default_rng(seed + r)
        s = baroclinic_state(g, c)
        shape = s["delp"].shape
        nz = shape[2] - 1
        lat, lon = g.lat_agrid[:, :, None], g.lon_agrid[:, :, None]
        ua, va, t = np.zeros(shape), np.zeros(shape), np.full(shape, 250.0)
        ua[:, :, :nz] = jw_zonal_wind(lon, lat, eta[None, None, :], c)
        t[:, :, :nz] = jw_temperature(lat, eta[None, None, :], c)
        ua += 2.0 * rng.standard_normal(shape)
        va += 2.0 * rng.standard_normal(shape)
        t += 2.0 * rng.standard_normal(shape)
        delp = s["delp"] * (1.0 + 2.0e-3 * rng.standard_normal(shape))
        out.append(dict(ua=ua, va=va, pt=t, delp=delp))
    return out


def _call(sf, grids, inputs, dt, config=None, fill=7.0, ptop=None):
    """The operator on the cube: (inputs as the device held them before, inputs after, outputs), per rank, float64 numpy.  The outputs start
    as ``fill`` everywhere: what is not written keeps it."""
    qf = sf.quantity_factory
    q = {n: qf.from_array([d[n] for d in inputs], CELL) for n in ("ua", "va", "pt", "delp")}
    ranks = range(len(grids))
    before = [{n: q[n].numpy(r).astype(np.float64) for n in q} for r in ranks]
    out = {n: qf.from_array([np.full_like(inputs[0]["ua"], fill) for _ in ranks], CELL) for n in ("u_dt", "v_dt", "pt_dt")}
    op = HeldSuarezForcing(sf, qf, grids, config=config)
    op(q["ua"], q["va"], q["pt"], q["delp"], out["u_dt"], out["v_dt"], out["pt_dt"], dt, ptop=ptop)
    _sync(sf)
    after = [{n: q[n].numpy(r).astype(np.float64) for n in q} for r in ranks]
    got = [{n: out[n].numpy(r).astype(np.float64) for n in out} for r in ranks]
    return before, after, got


def _box(g):
    return (slice(NH, NH + g.nx), slice(NH, NH + g.ny), slice(0, g.nz))


def _parity(backend, layout, dtype, dt=1800.0, **cfg_kw):
    nz = 8
    c, part, grids, sf = _cube(backend, 12, layout, nz, dtype=dtype, **cfg_kw)
    before, after, got = _call(sf, grids, _jw_inputs(grids, c), dt)
    eps = EPS[dtype]
    worst = {"u_dt": 0.0, "v_dt": 0.0, "pt_dt": 0.0}
    friction_cells = 0
    for r, g in enumerate(grids):
        b = _box(g)
        lat = g.lat_agrid[b[:2]]
        if dtype == torch.float32:
            lat = lat.astype(np.float32).astype(np.float64)
        i = before[r]
        ptop = float(np.float32(g.ptop)) if dtype == torch.float32 else g.ptop
        u_dt, v_dt, t_dt, tm = ref.held_suarez(i["ua"][b], i["va"][b], i["pt"][b], i["delp"][b], lat, ptop, dt)
        bu, bv, bt = ref.error_bound(i["ua"][b], i["va"][b], i["pt"][b], tm, dt, eps, nz)
        for name, want, bound in (("u_dt", u_dt, bu), ("v_dt", v_dt, bv), ("pt_dt", t_dt, bt)):
            a = got[r][name]
            err = np.abs(a[b] - want)
            assert np.all(np.isfinite(a[b]))
            assert np.all(err <= bound), (r, name, float((err - bound).max()))
            with np.errstate(invalid="ignore", divide="ignore"):
                worst[name] = max(worst[name], float(np.nanmax(np.where(bound > 0, err / bound, 0.0))))
            # sentinels: halo cells and the pad level of the outputs keep their fill
            outside = np.ones(a.shape, dtype=bool)
            outside[b] = False
            assert np.all(a[outside] == 7.0), (r, name)
        # ... and every input keeps its bits
        for n in i:
            assert np.array_equal(i[n], after[r][n]), (r, n)
        friction_cells += int(np.count_nonzero(tm["s"] > 0))
        if dtype == torch.float64:  # (the same operations on the same numbers: s is zero in the same cells)
            assert np.all(got[r]["u_dt"][b][tm["s"] == 0] == 0.0) and np.all(got[r]["v_dt"][b][tm["s"] == 0] == 0.0)
    print("max error / bound:", worst)
    assert friction_cells > 0
    return worst


@pytest.mark.parametrize("layout", [(1, 1), (2, 2)])
def test_matches_numpy_restatement(backend, layout):
    """fp64, C12, nz = 8, JW2006 state plus noise.  The bound is hs_reference.error_bound: first-order propagation of one unit round-off per
    arithmetic operation and 1 ulp per log / exp / sin / cos call through the formulas (its docstring has the derivation), evaluated per cell;
    it scales with |T_eq| and |T - T_eq| for the heating and with |ua|, |va| for the friction.  Halo cells and the pad level of the outputs and
    every input are bitwise untouched; u_dt = v_dt = 0 exactly where sigma <= sigma_b."""
    _parity(backend, layout, torch.float64)


def test_fp32_tracks_fp64_restatement(backend):
    """The fp32 build against the fp64 restatement on the fp32-rounded inputs, the same bound with the fp32 epsilon.
    (nord = 0: the fp32 context refuses the C12 del-6 damping tables, which overflow the float range; this operator reads none.)"""
    _parity(backend, (2, 2), torch.float32, nord=0)


def _columns(sf, grids, columns, lat_value, dt, config=None, t=None, ua=None):
    """One rank's storage filled with the same column everywhere and the operator's latitude overridden: returns the column of outputs
    at the first compute cell.  ``columns``: delp[nz]."""
    g = grids[0]
    nz = g.nz
    shape = (g.nx + 2 * NH + 1, g.ny + 2 * NH + 1, nz + 1)

    def fld(col, pad):
        a = np.full(shape, pad, dtype=np.float64)
        a[:, :, :nz] = np.asarray(col, dtype=np.float64)[None, None, :]
        return a

    inputs = [dict(ua=fld(np.full(nz, 10.0) if ua is None else ua, 0.0), va=fld(np.full(nz, -5.0), 0.0), pt=fld(np.full(nz, 250.0) if t is None else t, 250.0),
                   delp=fld(columns, 1.0)) for _ in grids]
    qf = sf.quantity_factory
    q = {n: qf.from_array([d[n] for d in inputs], CELL) for n in inputs[0]}
    out = {n: qf.zeros(CELL) for n in ("u_dt", "v_dt", "pt_dt")}
    op = HeldSuarezForcing(sf, qf, grids, config=config)
    op.lat.storage.fill_(lat_value)
    op(q["ua"], q["va"], q["pt"], q["delp"], out["u_dt"], out["v_dt"], out["pt_dt"], dt, ptop=0.0)
    _sync(sf)
    return {n: out[n].numpy(0)[NH, NH, :nz].astype(np.float64) for n in out}


def test_closed_form_pins(backend):
    """Values that need no reference (fp64, ptop = 0, one column everywhere, the latitude overridden):

    * phi = 0 and a single layer pair chosen so that a layer's p = p0: T_eq = 315 K there, so t_dt = -k_T / (1 + dt k_T) (T - 315) with
      k_T = k_a + (k_s - k_a) s, s = (p0 / ps - 0.7) / 0.3;
    * aloft (p = 50 hPa) the bracket times (p / p0)^kappa is below 200 K: T_eq is the floor, and k_T = k_a (sigma < sigma_b) -- t_dt =
      -k_a / (1 + dt k_a) (T - 200) to a few roundings;
    * at the poles cos^4 = 0 (cos(pi / 2) ~ 6e-17): k_T = k_a at every level, also inside the boundary layer;
    * u_dt = v_dt = 0 exactly at every level with sigma <= sigma_b, and -k_f s / (1 + dt k_f s) ua below;
    * dt -> 0: the explicit form -k (.) of the paper, exactly at dt = 0."""
    nz = 8
    c, part, grids, sf = _cube(backend, 12, (1, 1), nz)
    k_a, k_s, k_f = 1.0 / (40 * 86400.0), 1.0 / (4 * 86400.0), 1.0 / 86400.0
    # interfaces 0, 100, 200, 400, 600, 800, 900, 950, 1050 hPa: layer 7 has p = 1000 hPa = p0, ps = 1050 hPa; layer 0 has p = 50 hPa
    pe = np.array([0.0, 1.0e4, 2.0e4, 4.0e4, 6.0e4, 8.0e4, 9.0e4, 9.5e4, 1.05e5])
    delp = np.diff(pe)
    p = 0.5 * (pe[1:] + pe[:-1])
    sigma = p / pe[-1]
    s = np.maximum(0.0, (sigma - 0.7) / (1.0 - 0.7))
    assert p[7] == 1.0e5 and np.count_nonzero(s) == 3
    dt = 1800.0
    eq = _columns(sf, grids, delp, 0.0, dt)
    k_t = k_a + (k_s - k_a) * s[7]
    want = -k_t / (1.0 + dt * k_t) * (250.0 - 315.0)
    assert abs(eq["pt_dt"][7] - want) <= 8 * 2.0**-52 * abs(want) * (1.0 + 315.0 / 65.0), (eq["pt_dt"][7], want)
    want0 = -k_a / (1.0 + dt * k_a) * (250.0 - 200.0)
    assert (315.0 - 10.0 * np.log(0.05)) * 0.05 ** (2.0 / 7.0) < 200.0  # the floor holds at 50 hPa on the equator
    assert abs(eq["pt_dt"][0] - want0) <= 4 * 2.0**-52 * abs(want0), (eq["pt_dt"][0], want0)
    # friction: zero above sigma_b, the closed form below
    assert np.all(eq["u_dt"][s == 0] == 0.0) and np.all(eq["v_dt"][s == 0] == 0.0)
    for k in np.nonzero(s)[0]:
        kv = k_f * s[k]
        for name, wind in (("u_dt", 10.0), ("v_dt", -5.0)):
            w = -kv / (1.0 + dt * kv) * wind
            assert abs(eq[name][k] - w) <= 16 * 2.0**-52 * abs(w) / (1.0 - 0.7), (k, name, eq[name][k], w)
    # poles: k_T = k_a everywhere; T_eq from the restatement (cos^2 ~ 4e-33 removes the stability term)
    for lat in (0.5 * np.pi, -0.5 * np.pi):
        pole = _columns(sf, grids, delp, lat, dt)
        t_eq = np.maximum(200.0, (315.0 - 60.0) * (p / 1.0e5) ** (2.0 / 7.0))
        w = -k_a / (1.0 + dt * k_a) * (250.0 - t_eq)
        assert np.all(np.abs(pole["pt_dt"] - w) <= 64 * 2.0**-52 * k_a * (t_eq + np.abs(250.0 - t_eq))), (pole["pt_dt"], w)
    # the explicit limit: dt = 0 is -k (.), and a small dt differs from it by the factor 1 / (1 + dt k)
    ex = _columns(sf, grids, delp, 0.3, 0.0)
    small = _columns(sf, grids, delp, 0.3, 1.0e-3)
    tm = ref.terms(delp[None, None, :], np.array([[0.3]]), 0.0)
    for name, k, x in (("u_dt", tm["k_v"][0, 0], np.full(nz, 10.0)), ("pt_dt", tm["k_t"][0, 0], 250.0 - tm["t_eq"][0, 0])):
        assert np.all(np.abs(ex[name] + k * x) <= 64 * 2.0**-52 * k * (np.abs(x) + (tm["t_eq"][0, 0] if name == "pt_dt" else 0.0)))
        assert np.all(np.abs(small[name] - ex[name] / (1.0 + 1.0e-3 * k)) <= 8 * 2.0**-52 * np.abs(ex[name]))


def test_relaxation_law(backend):
    """The dycore off: n applications of T += dt t_dt leave T - T_eq = (1 + dt k_T)^-n (T0 - T_eq) in every cell (T_eq and k_T do not change:
    delp is untouched).  Rounding: each application forms T - T_eq (one rounding of size eps |T|, the cancellation), the product and the sum
    (eps |T| again): 3 eps |T| per step, not amplified (the factor is < 1), plus the kernel's own T_eq and k_T against the restatement's
    (hs_reference.error_bound's d(T_eq), d(k_T), constant over the steps)."""
    nz, n_steps, dt = 8, 5, 6 * 3600.0
    c, part, grids, sf = _cube(backend, 12, (1, 1), nz)
    qf = sf.quantity_factory
    inputs = _jw_inputs(grids, c)
    q = {n: qf.from_array([d[n] for d in inputs], CELL) for n in ("ua", "va", "pt", "delp")}
    out = {n: qf.zeros(CELL) for n in ("u_dt", "v_dt", "pt_dt")}
    op = HeldSuarezForcing(sf, qf, grids)
    t0 = [q["pt"].numpy(r).astype(np.float64) for r in range(6)]
    for _ in range(n_steps):
        op(q["ua"], q["va"], q["pt"], q["delp"], out["u_dt"], out["v_dt"], out["pt_dt"], dt)
        q["pt"].storage.add_(out["pt_dt"].storage, alpha=dt)  # (the pad level and the halo: + dt * 0)
    _sync(sf)
    eps = 2.0**-52
    for r, g in enumerate(grids):
        b = _box(g)
        tm = ref.terms(inputs[r]["delp"][b], g.lat_agrid[b[:2]], g.ptop)
        want = tm["t_eq"] + (1.0 + dt * tm["k_t"]) ** (-n_steps) * (t0[r][b] - tm["t_eq"])
        got = q["pt"].numpy(r)[b]
        _, _, bt = ref.error_bound(np.zeros_like(want), np.zeros_like(want), t0[r][b], tm, dt, eps, nz)
        bound = n_steps * (3 * eps * np.maximum(np.abs(t0[r][b]), tm["t_eq"]) + dt * bt)
        assert np.all(np.abs(got - want) <= bound), float((np.abs(got - want) / bound).max())
        assert float(np.abs(got - t0[r][b]).max()) > 1.0  # (the relaxation moved the temperature by kelvins)


def test_refusals(hostemu):
    c, part, grids, sf = _cube("hostemu", 12, (1, 1), 3)
    qf = sf.quantity_factory
    ua, va, pt, delp, a, b, d = (qf.ones(CELL) for _ in range(7))
    op = HeldSuarezForcing(sf, qf, grids)
    with pytest.raises(_lib.Fv3Error, match="alias"):
        op(ua, va, pt, delp, ua, b, d, 10.0)
    with pytest.raises(_lib.Fv3Error, match="alias"):
        op(ua, va, pt, delp, a, b, pt, 10.0)
    with pytest.raises(_lib.Fv3Error, match="three fields"):
        op(ua, va, pt, delp, a, a, d, 10.0)
    with pytest.raises(_lib.Fv3Error, match="field"):
        op(ua, va, pt, delp, a, b, qf.zeros(("x", "y")), 10.0)
    with pytest.raises(_lib.Fv3Error, match="field"):
        op(ua, va, pt, qf.zeros(("x", "y")), a, b, d, 10.0)
    with pytest.raises(_lib.Fv3Error, match="dt"):
        op(ua, va, pt, delp, a, b, d, -1.0)
    with pytest.raises(ValueError, match="sigma_b"):
        HeldSuarezForcing(sf, qf, grids, config=HeldSuarezConfig(sigma_b=1.0))
    with pytest.raises(ValueError, match="p0"):
        HeldSuarezForcing(sf, qf, grids, config=HeldSuarezConfig(p0=0.0))
    cfg = HeldSuarezConfig()
    assert (cfg.sigma_b, cfg.delta_t_y, cfg.delta_theta_z, cfg.p0, cfg.kappa, cfg.t_min) == (0.7, 60.0, 10.0, 1.0e5, 2.0 / 7.0, 200.0)
    assert (cfg.k_f, cfg.k_a, cfg.k_s) == (1.0 / 86400.0, 1.0 / (40.0 * 86400.0), 1.0 / (4.0 * 86400.0))
