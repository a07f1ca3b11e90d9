"""fv3_sat_adj (pace_amd/csrc/fv3_satadj.hip, fv3_satadj.h) through SaturationAdjustment and the C ABI: the saturation tables against their
closed forms, parity with the numpy restatement (tests/satadj_reference.py) within a tolerance the restatement sets itself, the properties of
the result, untouched cells, the decomposition, the argument checks, the register budget.  Every operator case runs on the host emulation
(CPU suite) and on the HIP library (-m gpu).

The inputs are random cells built to reach every branch of the 17 steps (temperatures of 170 - 310 K, vapour below and above saturation over
water and over ice, every condensate zero, tiny, large or slightly negative) plus the cells of the C12 restart fixture with its liq_wat.
Coverage is a condition of every comparison: _reference asserts it on the restatement's bitmask before it hands anything out."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

import satadj_reference as sref
from pace_amd import constants as pc, lib as _lib
from pace_amd._testing import stencil_factory_for
from pace_amd.config import AcousticDynamicsConfig
from pace_amd.constants import get_constants
from pace_amd.grid import make_grid
from pace_amd.stencils import SatAdjustConfig, SaturationAdjustment, WaterSpecies
from pace_amd.topology import CubedSpherePartitioner
from test_fillz import real  # noqa: F401  (the (backend, dtype) fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "c12_restart_6tiles.npz")
NH = 3
NX = 12
SENTINEL = -777.25
DIMS = ("x", "y", "z")
NP_OF = {torch.float64: np.float64, torch.float32: np.float32}
SPECIES = ("qv", "ql", "qr", "qi", "qs", "qg")
ROLE = dict(qv="qvapor", ql="qliquid", qr="qrain", qi="qice", qs="qsnow", qg="qgraupel")
INPUTS = ("tv",) + SPECIES + ("dp", "delz")
WRITTEN = ("tv",) + SPECIES + ("q_con", "cappa", "pkz")
ALL = INPUTS + ("q_con", "cappa", "pkz")
MDT = 112.5  # a 225 s step with k_split = 2
MIN_CELLS = 20  # every arm of every conditional, in the cells the entry covers
MARGIN = {np.float64: 1.0e-9, np.float32: 1.0e-4}  # cells whose closest comparison is nearer than this may flip a branch: left out
MAX_EXCLUDED = 0.005

# Tolerances, set by the restatement and not by the kernel (measure_tolerances below: the restatement against itself with every exp / log
# result and every table entry nudged by +-1 ulp at random; the largest difference per field over the C12 L8 and L79 inputs and both
# values of last_step, species and q_con scaled by the cell's total water, tv, cappa and pkz by their own value; times 4).
# Measured 2026-10-19 (x86-64 host, numpy 2.2, glibc libm); the raw values are in DESIGN.md.
TOL = {
    np.float64: dict(species=4 * 3.0535e-15, tv=4 * 4.2443e-16, q_con=4 * 1.8344e-15, cappa=4 * 3.9394e-16, pkz=4 * 1.7134e-15),
    np.float32: dict(species=4 * 3.3324e-06, tv=4 * 2.1100e-07, q_con=4 * 1.3771e-06, cappa=4 * 1.0737e-07, pkz=4 * 8.1515e-07),
}
# Properties, measured on the restatement's own output the same way (times 4): total water of a cell (relative to the sum of the absolute
# species), the energy te = cvm T + lv00 qv - li00 q_sol (relative), cloud water left below t_ice - 48 K (kg/kg), the most negative qi (kg/kg)
PROP = {
    np.float64: dict(water=4 * 5.8028e-16, te=4 * 8.3842e-16, cold_ql=4 * 0.0, neg_qi=4 * 0.0),
    np.float32: dict(water=4 * 1.5381e-07, te=4 * 3.1495e-07, cold_ql=4 * 0.0, neg_qi=4 * 0.0),
}
# libm against numpy on the table arguments (largest difference seen 2026-10-19: 30 ulp of the fp64 value), times 2; the fp32
# tables are those values rounded once more: half an ulp of fp32 on top
TABLE_ULP = 2 * 30.0


# ---------------------------------------------------------------------------------------------------------------------------------
# contexts, inputs, the operator, the restatement: each computed once and shared
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _grids(layout, nz):
    part = CubedSpherePartitioner(NX, layout)
    return part, [make_grid(part, r, nz=nz) for r in range(part.total_ranks)]


def _factory(backend, layout, nz, dtype):
    part, grids = _grids(layout, nz)
    # (nord = 0: the fp32 context refuses the C12 del-6 damping tables, which overflow the float range; the adjustment reads none)
    cfg = AcousticDynamicsConfig(npx=NX + 1, npy=NX + 1, npz=nz, layout=layout, nord=0)
    return part, grids, stencil_factory_for(backend)(grids, cfg, get_constants(), dtype=dtype)


def _sync(sf):
    if not sf.hostemu:
        torch.cuda.synchronize()


def _level0(nz):
    """kmp, independently of the library: the first level whose reference mid-pressure exceeds 10 hPa"""
    g = _grids((1, 1), nz)[1][0]
    ph = np.asarray(g.ak, dtype=np.float64) + np.asarray(g.bk, dtype=np.float64) * 1.0e5
    pfull = (ph[1:] - ph[:-1]) / np.log(ph[1:] / ph[:-1])
    return int(np.argmax(pfull > 1.0e3)) if (pfull > 1.0e3).any() else nz


def _saturation(t, den, ice):
    """saturation mixing ratio over water / ice from the closed-form tables in double (the generator's yardstick)"""
    tw, t2 = sref.closed_form_tables()
    tab = t2 if ice else tw
    des = np.append(np.diff(tab), 0.0)
    k = sref.constants(np.float64, MDT)
    return sref.qs2(tab, np.maximum(des, 0.0), t, den, k)[0]


@functools.lru_cache(maxsize=None)
def _inputs(nz, npd):
    """{field: (6, 12, 12, nz)} in npd, read-only.  Random cells by regime; at nz = 79 the lowest 63 levels are the restart fixture's cells
    (T, delp, qv = sphum, ql = liq_wat, the other condensates zero as in the restart).  The last-step property below ("a cell that came in supersaturated above
    t_ice leaves less supersaturated") follows from the step forms only where nothing moves the temperature after the second pass of
    step 8; above t_ice one step does: step 12 melts snow and cools the cell by up to fac_smlt * (T - t_ice), which lowers the saturation
    value again (the restatement itself showed 2 such cells in 519 when large snow was allowed there: 1.7e-3 -> 3.1e-3 kg/kg at 288 K).
    So the random cells that are warmer than 272 K and supersaturated get no more than a trace of snow (the melting branch is still
    covered, by the subsaturated cells), and the random cells' vapour stays 5 % or more away from saturation."""
    rng = np.random.default_rng(2026 + nz)
    cst = get_constants()
    shape = (6, NX, NX, nz)
    t = rng.uniform(170.0, 310.0, shape)
    # a fifth of the cells sits within 3 K of a threshold temperature, where the melting / freezing steps start
    near = rng.random(shape) < 0.2
    t = np.where(near, rng.choice([184.0, 225.16, 233.16, 273.16], shape) + rng.uniform(-3.0, 3.0, shape), t)
    p = np.exp(rng.uniform(np.log(2.0e3), np.log(1.0e5), shape))
    dp = rng.uniform(500.0, 1500.0, shape)
    qv = None
    fixture_levels = 0
    if nz == 79:
        data = np.load(FIXTURE)
        col = lambda key: np.transpose(data[key], (0, 3, 2, 1))  # noqa: E731  (tile, k, j, i) -> (tile, i, j, k)
        fixture_levels = col("T").shape[3]
        lv = slice(nz - fixture_levels, nz)  # (the lowest levels: all of them below kmp)
        t[..., lv] = col("T")
        dp[..., lv] = col("delp")
        pe = np.concatenate([np.full((6, NX, NX, 1), float(data["ak"][0])), float(data["ak"][0]) + np.cumsum(col("delp"), axis=3)], axis=3)
        p[..., lv] = 0.5 * (pe[..., 1:] + pe[..., :-1])
    den = p / (cst.RDGAS * t)
    delz = -dp / (cst.GRAV * den)
    # vapour: 15 % to 160 % of saturation over water (over ice below 250 K for half of the cold cells), capped at 30 g/kg
    rh = np.where(rng.random(shape) < 0.5, rng.uniform(0.15, 0.95, shape), rng.uniform(1.05, 1.6, shape))
    over_ice = (t < 250.0) & (rng.random(shape) < 0.5)
    qsat = np.where(over_ice, _saturation(t, den, True), _saturation(t, den, False))
    qv = np.minimum(rh * qsat, 0.03)
    q = {"qv": qv}
    for f in SPECIES[1:]:
        kind = rng.choice(4, shape, p=[0.3, 0.2, 0.35, 0.15])
        tiny = 10.0 ** rng.uniform(-10.0, -6.5, shape)
        large = 10.0 ** rng.uniform(-5.0, -2.3, shape)
        neg = -(10.0 ** rng.uniform(-9.0, -5.0, shape))
        if f == "qs":  # (see the docstring: no snow to melt where the last-step property is asserted)
            kind = np.where((kind == 2) & (t > 272.0) & (rh > 1.0), 1, kind)
        q[f] = np.select([kind == 0, kind == 1, kind == 2], [0.0, tiny, large], neg)
    if fixture_levels:
        lv = slice(nz - fixture_levels, nz)
        q["qv"][..., lv] = col("sphum")
        q["ql"][..., lv] = col("liq_wat")
        for f in ("qr", "qi", "qs", "qg"):  # (the restart has vapour and cloud water only)
            q[f][..., lv] = 0.0
    q_con = (q["ql"] + q["qr"]) + ((q["qi"] + q["qs"]) + q["qg"])
    tv = t * (1.0 + (cst.RVGAS / cst.RDGAS - 1.0) * q["qv"]) * (1.0 - q_con)
    out = dict(q, tv=tv, dp=dp, delz=delz)
    out = {f: np.ascontiguousarray(out[f].astype(npd)) for f in INPUTS}
    for a in out.values():
        a.setflags(write=False)
    return out


def _scatter(part, glob, r):
    """the (nx, ny, nz) block of rank r out of a (6, 12, 12, nz) array"""
    i0, j0 = part.origin(r)
    return glob[part.tile_index(r), i0 : i0 + part.nx, j0 : j0 + part.ny]


def _padded(cells, fill, npd, kmp):
    n, m, nz = cells.shape
    a = np.full((n + 2 * NH + 1, m + 2 * NH + 1, nz + 1), fill, dtype=npd)
    a[NH : NH + n, NH : NH + m, kmp:nz] = cells[:, :, kmp:]
    return a


def _water(q):
    return WaterSpecies(**{ROLE[s]: q[s] for s in SPECIES})


@functools.lru_cache(maxsize=None)
def _run(backend, dtype, layout, nz, last_step):
    """The operator on _inputs: ({field: (6, 12, 12, nz) after}, {field: [storage arrays after]}, {field: [storage arrays before]}, tables, kmp)"""
    npd = NP_OF[dtype]
    part, grids, sf = _factory(backend, layout, nz, dtype)
    qf = sf.quantity_factory
    op = SaturationAdjustment(sf, qf, grids)
    kmp = op.level0
    glob = _inputs(nz, npd)
    # the sentinel everywhere the entry may not touch: halo, pad level, the levels above kmp (delp / delz: a plain thickness there)
    fill = {f: (1000.0 if f == "dp" else -1000.0 if f == "delz" else SENTINEL) for f in ALL}
    host = {f: [_padded(_scatter(part, glob[f], r) if f in INPUTS else np.full((part.nx, part.ny, nz), SENTINEL, dtype=npd), fill[f], npd, kmp) for r in range(len(grids))] for f in ALL}
    q = {f: qf.from_array(host[f], DIMS) for f in ALL}
    op(_water(q), q["tv"], q["dp"], q["delz"], q["q_con"], q["cappa"], q["pkz"], MDT, last_step=bool(last_step))
    _sync(sf)
    raw = {f: [q[f].numpy(r).copy() for r in range(len(grids))] for f in ALL}
    got = {f: np.full((6, NX, NX, nz), np.nan, dtype=npd) for f in ALL}
    for f in ALL:
        for r in range(len(grids)):
            i0, j0 = part.origin(r)
            got[f][part.tile_index(r), i0 : i0 + part.nx, j0 : j0 + part.ny] = raw[f][r][NH : NH + part.nx, NH : NH + part.ny, :nz]
    return got, raw, host, op.tables().astype(npd), kmp


def _coverage(mask, last_step, what):
    arms = sref.arms(mask, last_step)
    thin = {a: n for a, n in arms.items() if n < MIN_CELLS}
    assert not thin, (what, thin, arms)
    return arms


@functools.lru_cache(maxsize=None)
def _reference(backend, dtype, nz, last_step):
    """The restatement on the covered cells of _inputs with the tables of this backend: (out, mask, margin, keep); asserts the coverage and the excluded share"""
    npd = NP_OF[dtype]
    tables, kmp = _run(backend, dtype, (1, 1), nz, last_step)[3:]
    assert kmp == _level0(nz)
    glob = _inputs(nz, npd)
    k = sref.constants(npd, MDT)
    out, mask, margin = sref.sat_adj(*[glob[f][..., kmp:] for f in INPUTS], tables, k, bool(last_step))
    _coverage(mask, last_step, (npd.__name__, nz, last_step))
    keep = margin >= MARGIN[npd]
    share = 1.0 - keep.mean()
    print(f"sat_adj restatement {npd.__name__} L{nz} last_step={last_step}: {mask.size} cells, {100 * share:.3f} % within {MARGIN[npd]:g} of a branch")
    assert share <= MAX_EXCLUDED, share
    return out, mask, margin, keep


def _total_water(glob, kmp):
    return sum(np.abs(glob[f][..., kmp:].astype(np.float64)) for f in SPECIES)


def _scaled_diffs(a, b, glob, kmp, keep):
    """largest difference per tolerance class between two results on the kept cells"""
    tw = _total_water(glob, kmp)
    d = {}
    sp = [np.abs(a[f].astype(np.float64) - b[f].astype(np.float64)) / tw for f in SPECIES]
    d["species"] = float(max(x[keep].max() for x in sp))
    d["q_con"] = float((np.abs(a["q_con"].astype(np.float64) - b["q_con"].astype(np.float64)) / tw)[keep].max())
    for f in ("tv", "cappa", "pkz"):
        d[f] = float((np.abs(a[f].astype(np.float64) - b[f].astype(np.float64)) / np.abs(b[f].astype(np.float64)))[keep].max())
    return d


def _properties(res, glob, kmp, npd):
    """the property figures of a result ({field: covered cells}) in float64: (water, te, cold_ql, neg_qi, per-cell arrays for the messages)"""
    k = {n: float(v) for n, v in sref.constants(np.float64, MDT).items()}
    f64 = lambda a: a.astype(np.float64)  # noqa: E731
    q0 = {f: f64(glob[f][..., kmp:]) for f in SPECIES}
    q1 = {f: f64(res[f]) for f in SPECIES}
    tw = sum(np.abs(q0[f]) for f in SPECIES)
    water = np.abs(sum(q1[f] for f in SPECIES) - sum(q0[f] for f in SPECIES)) / tw

    def energy(q, tv):
        q_liq, q_sol = q["ql"] + q["qr"], q["qi"] + q["qs"] + q["qg"]
        t = tv / ((1.0 + k["zvir"] * q["qv"]) * (1.0 - (q_liq + q_sol)))
        mc_air = (1.0 - sum(q0[f] for f in SPECIES)) * k["cv_air"]  # (the dry mass fraction the step holds fixed)
        cvm = mc_air + q["qv"] * k["cv_vap"] + q_liq * k["c_liq"] + q_sol * k["c_ice"]
        return cvm * t + k["lv00"] * q["qv"] - k["li00"] * q_sol, t

    te0, t0 = energy(q0, f64(glob["tv"][..., kmp:]))
    te1, t1 = energy(q1, f64(res["tv"]))
    te = np.abs(te1 - te0) / np.abs(te0)
    cold = t1 < k["tice"] - 48.0
    cold_ql = float(np.where(cold, q1["ql"], 0.0).max())
    ok_in = (q0["qi"] + q0["qs"]) >= 0
    neg_qi = float(np.maximum(-np.where(ok_in, q1["qi"], 0.0), 0.0).max())
    return dict(water=float(water.max()), te=float(te.max()), cold_ql=max(cold_ql, 0.0), neg_qi=neg_qi), (t0, t1, q0, q1)


def measure_tolerances(npd, tables_of, seed=7):
    """What TOL and PROP are made of (not a test: call it from a script; DESIGN.md §7, "Saturation adjustment", quotes its output).
    tables_of(nz) -> (4, 2621) float64 tables of the library."""
    rng = np.random.default_rng(seed)

    def nudge(a):
        a = np.asarray(a)
        step = rng.integers(-1, 2, a.shape)
        return np.where(step < 0, np.nextafter(a, npd(-np.inf)), np.where(step > 0, np.nextafter(a, npd(np.inf)), a)).astype(a.dtype)

    worst, props = {}, {}
    for nz in (8, 79):
        kmp = _level0(nz)
        glob = _inputs(nz, npd)
        k = sref.constants(npd, MDT)
        tables = tables_of(nz).astype(npd)
        args = [glob[f][..., kmp:] for f in INPUTS]
        for last_step in (False, True):
            a, _, ma = sref.sat_adj(*args, tables, k, last_step)
            b, _, mb = sref.sat_adj(*args, nudge(tables), k, last_step, exp=lambda x: nudge(np.exp(x)), log=lambda x: nudge(np.log(x)))
            keep = (ma >= MARGIN[npd]) & (mb >= MARGIN[npd])
            for f, v in _scaled_diffs(a, b, glob, kmp, keep).items():
                worst[f] = max(worst.get(f, 0.0), v)
            for f, v in _properties(a, glob, kmp, npd)[0].items():
                props[f] = max(props.get(f, 0.0), v)
    return worst, props


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the tables
# ---------------------------------------------------------------------------------------------------------------------------------
def test_tables_match_the_closed_forms(real):  # noqa: F811
    backend, dtype = real
    npd = NP_OF[dtype]
    tables = _run(backend, dtype, (1, 1), 8, 0)[3]
    assert tables.shape == (4, sref.NTAB) and tables.dtype == npd
    tw, t2 = sref.closed_form_tables()
    t2s = t2.copy()
    t2s[1599] = 0.25 * (t2[1598] + 2.0 * t2[1599] + t2[1600])
    t2s[1600] = 0.25 * (t2[1599] + 2.0 * t2[1600] + t2[1601])
    worst = 0.0
    for got, want in ((tables[0], tw), (tables[1], t2s)):
        ulp = np.spacing(want)
        err = np.abs(got.astype(np.float64) - want) / ulp
        if npd is np.float32:
            err = np.abs(got.astype(np.float64) - want) / np.spacing(want.astype(np.float32)).astype(np.float64)
            bound = 0.5 + TABLE_ULP * float((ulp / np.spacing(want.astype(np.float32))).max())
        else:
            bound = TABLE_ULP
        worst = max(worst, float(err.max()))
        assert err.max() <= bound, (float(err.max()), bound, int(err.argmax()))
    print(f"sat_adj tables {backend} {npd.__name__}: worst {worst:.3f} ulp against the closed forms in numpy double")
    # above the join table2 is tablew, entry for entry
    assert np.array_equal(tables[1][1601:], tables[0][1601:])
    # the two smoothed entries sit between their neighbours' unsmoothed values: the ice branch below, the water branch above
    assert tables[1][1598] < tables[1][1599] < tables[1][1600] < tables[1][1601]
    # the differences are those of the table's own entries, exactly; the last repeats the one before it
    for tab, des in ((tables[0], tables[2]), (tables[1], tables[3])):
        d = tab[1:] - tab[:-1]
        assert d.dtype == npd
        assert np.array_equal(des[:-1], np.where(d > 0, d, npd(0)))
        assert des[-1] == des[-2]
    # the smoothing in the table's own terms: 0.25 * (t[n-1] + 2 t[n] + t[n+1]) of the UNSMOOTHED neighbours, to the rounding of the cast
    if npd is np.float64:
        assert abs(tables[1][1599] - 0.25 * (tables[1][1598] + 2.0 * t2[1599] + t2[1600])) <= 2 * TABLE_ULP * np.spacing(t2[1599])
        assert abs(tables[1][1600] - 0.25 * (t2[1599] + 2.0 * t2[1600] + tables[1][1601])) <= 2 * TABLE_ULP * np.spacing(t2[1600])


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. / 3. parity with the restatement, the properties of the result
# ---------------------------------------------------------------------------------------------------------------------------------
CASES = [((1, 1), 8), ((2, 2), 8), ((1, 1), 79)]
CASE_IDS = ["c12_1x1_l8", "c12_2x2_l8", "c12_1x1_l79"]


@pytest.mark.parametrize("last_step", [0, 1], ids=["mid", "last"])
@pytest.mark.parametrize("layout, nz", CASES, ids=CASE_IDS)
def test_parity_with_the_restatement(real, layout, nz, last_step):  # noqa: F811
    backend, dtype = real
    npd = NP_OF[dtype]
    want, mask, margin, keep = _reference(backend, dtype, nz, last_step)  # (asserts the coverage first)
    got, raw, host, tables, kmp = _run(backend, dtype, layout, nz, last_step)
    assert kmp == _level0(nz) and (kmp > 0) == (nz == 79)
    glob = _inputs(nz, npd)
    res = {f: got[f][..., kmp:] for f in WRITTEN}
    for f in WRITTEN:
        assert np.isfinite(res[f]).all(), f
    d = _scaled_diffs(res, want, glob, kmp, keep)
    print(f"sat_adj {backend} {npd.__name__} {layout} L{nz} last_step={last_step}: " + ", ".join(f"{f} {v:.3e} (bound {TOL[npd][f]:.3e})" for f, v in d.items()))
    for f, v in d.items():
        assert v <= TOL[npd][f], (f, v, TOL[npd][f])


@pytest.mark.parametrize("last_step", [0, 1], ids=["mid", "last"])
@pytest.mark.parametrize("layout, nz", [CASES[0], CASES[2]], ids=[CASE_IDS[0], CASE_IDS[2]])
def test_properties_of_the_result(real, layout, nz, last_step):  # noqa: F811
    backend, dtype = real
    npd = NP_OF[dtype]
    _reference(backend, dtype, nz, last_step)
    got, raw, host, tables, kmp = _run(backend, dtype, layout, nz, last_step)
    glob = _inputs(nz, npd)
    res = {f: got[f][..., kmp:] for f in WRITTEN}
    fig, (t0, t1, q0, q1) = _properties(res, glob, kmp, npd)
    print(f"sat_adj {backend} {npd.__name__} L{nz} last_step={last_step}: " + ", ".join(f"{f} {v:.3e} (bound {PROP[npd][f]:.3e})" for f, v in fig.items()))
    for f, v in fig.items():
        assert v <= PROP[npd][f], (f, v, PROP[npd][f])
    if last_step:
        # the supersaturation over water of every cell that came in supersaturated above t_ice is smaller on the way out
        k = sref.constants(np.float64, MDT)
        t64 = tables.astype(np.float64)
        den = glob["dp"][..., kmp:].astype(np.float64) / (-float(k["grav"]) * glob["delz"][..., kmp:].astype(np.float64))
        s0 = q0["qv"] - sref.qs2(t64[0], t64[2], t0, den, k)[0]
        s1 = q1["qv"] - sref.qs2(t64[0], t64[2], t1, den, k)[0]
        sel = (s0 > 0) & (t0 > float(k["tice"]))
        assert sel.sum() >= MIN_CELLS
        assert (s1[sel] < s0[sel]).all(), (int((s1[sel] >= s0[sel]).sum()), int(sel.sum()))


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. untouched cells, the decomposition
# ---------------------------------------------------------------------------------------------------------------------------------
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


@pytest.mark.parametrize("layout, nz", CASES, ids=CASE_IDS)
def test_cells_outside_the_covered_box_keep_their_bits(real, layout, nz):  # noqa: F811
    backend, dtype = real
    got, raw, host, tables, kmp = _run(backend, dtype, layout, nz, 1)
    part = _grids(layout, nz)[0]
    inside = (slice(NH, NH + part.nx), slice(NH, NH + part.ny), slice(kmp, nz))
    for f in ALL:
        for r in range(len(raw[f])):
            if f in ("dp", "delz"):
                assert np.array_equal(_bits(raw[f][r]), _bits(host[f][r])), (f, r, "only read")
                continue
            outside = np.ones(raw[f][r].shape, dtype=bool)
            outside[inside] = False
            assert np.array_equal(_bits(raw[f][r][outside]), _bits(host[f][r][outside])), (f, r)
            assert not np.array_equal(_bits(raw[f][r][inside]), _bits(host[f][r][inside])), (f, r, "nothing was written")


@pytest.mark.parametrize("last_step", [0, 1], ids=["mid", "last"])
def test_the_result_does_not_depend_on_the_decomposition(real, last_step):  # noqa: F811
    backend, dtype = real
    one = _run(backend, dtype, (1, 1), 8, last_step)[0]
    four = _run(backend, dtype, (2, 2), 8, last_step)[0]
    for f in ALL:
        assert np.array_equal(_bits(one[f]), _bits(four[f])), f


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. argument checks through the C ABI and the Python refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def test_argument_checks(backend):
    nz = 8
    part, grids, sf = _factory(backend, (1, 1), nz, torch.float64)
    qf = sf.quantity_factory
    rng = np.random.default_rng(1)
    mk = lambda: qf.from_array([rng.uniform(1.0e-4, 1.0e-3, (NX + 2 * NH + 1, NX + 2 * NH + 1, nz + 1)) for _ in grids], DIMS)  # noqa: E731
    q = {f: mk() for f in ALL}
    q["dp"].storage.add_(1000.0)
    q["delz"].storage.add_(100.0).neg_()
    q["tv"].storage.add_(280.0)
    flat = qf.zeros(("x", "y"))
    short = _lib.fv3_field()
    C.memmove(C.byref(short), C.byref(q["qv"].field), C.sizeof(_lib.fv3_field))
    short.shape[2] -= 1
    before = {f: q[f].storage.clone() for f in ALL}
    lib, ctx, s = sf.lib, sf.ctx, sf.stream_handle
    latent = _lib.fv3_latent(pc.HLV, pc.HLF, pc.T_ICE)

    def ref(v):
        return None if v is None else (C.pointer(v) if isinstance(v, _lib.fv3_field) else C.pointer(v.field))

    def call(no_ctx=False, no_water=False, no_latent=False, no_params=False, mdt=MDT, last_step=0, **swap):
        par = {n: swap.pop(n, v) for n, v in pc.SAT_ADJ_DEFAULTS.items()}
        f = {k: swap.get(k, q[k]) for k in ALL}
        water = None if no_water else C.byref(_lib.fv3_water(*[ref(f[k]) for k in SPECIES], pc.CV_VAP, pc.C_LIQ, pc.C_ICE))
        params = None if no_params else C.byref(_lib.fv3_sat_params(*[par[n] for n in _lib.SAT_PARAMS]))
        return lib.fv3_sat_adj(None if no_ctx else ctx, water, None if no_latent else C.byref(latent), params, ref(f["tv"]), ref(f["dp"]), ref(f["delz"]), ref(f["q_con"]),
                               ref(f["cappa"]), ref(f["pkz"]), mdt, last_step, s)

    ARG = -1
    assert call(no_ctx=True) == ARG
    cases = [
        ("null water", dict(no_water=True), b"sat_adj: the fv3_water is null"),
        ("null latent", dict(no_latent=True), b"sat_adj: the fv3_latent is null"),
        ("null params", dict(no_params=True), b"sat_adj: the fv3_sat_params is null"),
        ("null tv", dict(tv=None), b"'tv': null"),
        ("null delp", dict(dp=None), b"'delp': null"),
        ("null delz", dict(delz=None), b"'delz': null"),
        ("null q_con", dict(q_con=None), b"'q_con': null"),
        ("null cappa", dict(cappa=None), b"'cappa': null"),
        ("null pkz", dict(pkz=None), b"'pkz': null"),
        ("2-D tv", dict(tv=flat), b"'tv': vertical shape"),
        ("2-D pkz", dict(pkz=flat), b"'pkz': vertical shape"),
        ("mis-shaped qrain", dict(qr=short), b"'qrain': vertical shape"),
        ("2-D qice", dict(qi=flat), b"'qice': vertical shape"),
        ("qliquid and qrain the same", dict(qr=q["ql"]), b"qliquid and qrain are the same field"),
        ("qvapor and qgraupel the same", dict(qg=q["qv"]), b"qvapor and qgraupel are the same field"),
        ("tv is qsnow", dict(tv=q["qs"]), b"tv is the qsnow field"),
        ("pkz is qvapor", dict(pkz=q["qv"]), b"pkz is the qvapor field"),
        ("delp is qice", dict(dp=q["qi"]), b"delp is the qice field"),
        ("q_con and cappa the same", dict(cappa=q["q_con"]), b"q_con and cappa are the same field"),
        ("pkz is delz", dict(pkz=q["delz"]), b"delz and pkz are the same field (delz is only read)"),
        ("tv is delp", dict(tv=q["dp"]), b"tv and delp are the same field"),
        ("mdt = 0", dict(mdt=0.0), b"mdt = 0.000000 is not positive"),
        ("mdt < 0", dict(mdt=-1.0), b"is not positive"),
        ("last_step = 2", dict(last_step=2), b"last_step = 2 (0 or 1)"),
        ("last_step = -1", dict(last_step=-1), b"last_step = -1 (0 or 1)"),
    ] + [(f"null {ROLE[k]}", {k: None}, f"'{ROLE[k]}': null".encode()) for k in SPECIES] \
      + [(f"{n} = 0", {n: 0.0}, f"sat_adj: {n} = 0.000000 is not positive".encode()) for n in _lib.SAT_PARAMS if n.startswith("tau_")] \
      + [("tau_l2v is NaN", dict(tau_l2v=float("nan")), b"tau_l2v = ")]
    for what, kw, word in cases:
        assert call(qv=flat) == ARG and b"'qvapor': vertical shape" in lib.fv3_last_error(ctx)  # (another message in between: the one below is this case's own)
        st = call(**kw)
        msg = lib.fv3_last_error(ctx)
        assert st == ARG, (what, st)
        assert msg and word in msg, (what, msg)
        _sync(sf)
        for f in ALL:
            assert torch.equal(q[f].storage, before[f]), (what, f)
    # the tables do not exist before the context's first adjusting call; the table call checks its own arguments
    op = SaturationAdjustment(sf, qf, grids)
    buf = (C.c_double * (4 * _lib.SAT_NTAB))()
    assert lib.fv3_sat_adj_tables(ctx, buf, 4 * _lib.SAT_NTAB) == ARG and b"first fv3_sat_adj" in lib.fv3_last_error(ctx)
    assert lib.fv3_sat_adj_tables(None, buf, 4 * _lib.SAT_NTAB) == ARG
    assert lib.fv3_sat_adj_level0(ctx, None) == ARG and lib.fv3_sat_adj_level0(None, C.byref(C.c_int())) == ARG
    # the Python refusals: one sentence each
    for kw, word in ((dict(hydrostatic=True), "non-hydrostatic"), (dict(do_qa=True), "do_qa")):
        with pytest.raises(NotImplementedError, match=word) as e:
            SaturationAdjustment(sf, qf, grids, **kw)
        assert str(e.value).count(". ") == 0
    with pytest.raises(_lib.Fv3Error, match="'qrain': null"):
        op(WaterSpecies(q["qv"], qliquid=q["ql"], qice=q["qi"], qsnow=q["qs"], qgraupel=q["qg"]), q["tv"], q["dp"], q["delz"], q["q_con"], q["cappa"], q["pkz"], MDT)
    _sync(sf)
    for f in ALL:
        assert torch.equal(q[f].storage, before[f]), f
    # ... and a call that passes changes what it owns and nothing else; the parameters of the config reach the kernel
    op(_water(q), q["tv"], q["dp"], q["delz"], q["q_con"], q["cappa"], q["pkz"], MDT, last_step=True)
    _sync(sf)
    assert lib.fv3_sat_adj_tables(ctx, buf, 4 * _lib.SAT_NTAB) == 0 and lib.fv3_sat_adj_tables(ctx, buf, 5) == ARG
    assert not torch.equal(q["qv"].storage, before["qv"]) and torch.equal(q["dp"].storage, before["dp"]) and torch.equal(q["delz"].storage, before["delz"])
    assert SatAdjustConfig() == SatAdjustConfig(**pc.SAT_ADJ_DEFAULTS) and [f.name for f in __import__("dataclasses").fields(SatAdjustConfig)] == _lib.SAT_PARAMS
    after = q["qr"].storage.clone()  # (step 3 at these temperatures: ql_mlt decides how much of the melted ice becomes rain)
    for f in WRITTEN:
        q[f].storage.copy_(before[f])
    SaturationAdjustment(sf, qf, grids, SatAdjustConfig(ql_mlt=0.0))(_water(q), q["tv"], q["dp"], q["delz"], q["q_con"], q["cappa"], q["pkz"], MDT, last_step=True)
    _sync(sf)
    assert not torch.equal(q["qr"].storage, after)


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. register budget (read from the code-object metadata of the built library: no GPU needed)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [64, 32])
def test_sat_adj_kernels_stay_inside_the_register_budget(precision):
    """Both kernels: nothing spilled, no scratch, no LDS (the tables are read from global memory).  The stand-alone cell kernel is a
    streaming kernel and wants four waves per SIMD: at most 128 architectural VGPRs.  The adjusting closing kernel of the remap carries the
    column state of the closing kernel (the moist form alone holds 107) through the 17 steps with their exp / log expansions and cannot be
    held to that; what must not happen to it is the cliff below two waves per SIMD, where nothing is left to cover the latency of its
    level-by-level loads: at most 256 architectural VGPRs (the gfx950 limit for two waves; DESIGN.md quotes the count it has)."""
    import shutil

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_budget

    from pace_amd import build

    lib = build.lib_path(precision)
    if not os.path.exists(kernel_budget.READELF):
        pytest.skip(f"{kernel_budget.READELF} not found (no ROCm LLVM tools on this machine)")
    if not os.path.exists(lib):
        if not (os.path.exists(build.HIPCC) or shutil.which(build.HIPCC)):
            pytest.skip("the HIP library is not built and hipcc is not available")
        build.build(precision)
    ks = kernel_budget.kernels(lib)
    if not ks and b"CCOB" in open(lib, "rb").read(1 << 22):
        pytest.skip("compressed offload bundle (--offload-compress): the metadata reader does not unpack it")
    cells = {n: k for n, k in ks.items() if "sat_adj_cells" in n}
    close = {n: k for n, k in ks.items() if "remap_close" in n and "Lb1ELb1E" in n}
    assert len(cells) == 1 and len(close) == 1, (sorted(cells), sorted(n for n in ks if "remap_close" in n))
    for limit, hits in ((128, cells), (256, close)):
        for n, k in hits.items():
            assert k["vgpr"] - k["agpr"] <= limit and k["spill"] == 0 and k["scratch"] == 0 and k["lds"] == 0, (n[:100], k)
