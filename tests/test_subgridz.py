"""fv3_subgrid_z (pace_amd/csrc/fv3_subgridz.hip) through DryConvectiveAdjustment and the C ABI: bitwise parity with the numpy
restatement (tests/subgridz_reference.py) in fp64 and fp32, every place the form changes, hand-computed columns, properties that do
not use the restatement, the footprint, the argument checks, the register budget of the kernels.  Every operator case runs on the
host emulation (CPU suite) and on the HIP library (-m gpu).

Shapes: C12 with 12 x 12 sub-domains, the 6 x 6 blocks of a 2 x 2 layout and the non-square 12 x 6 blocks of a 1 x 2 layout (a 2 x 2
layout of a square tile has no non-square block); nz = 6 unless a case says otherwise."""
import ctypes as C
import functools
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import subgridz_reference as sref
from pace_amd import constants as pc, lib as _lib
from pace_amd._testing import stencil_factory_for
from pace_amd.config import AcousticDynamicsConfig
from pace_amd.constants import get_constants
from pace_amd.grid import make_grid
from pace_amd.stencils import ApplyPhysicsToDycore, DryConvectiveAdjustment, WaterSpecies
from pace_amd.topology import CubedSpherePartitioner
from test_fillz import real  # noqa: F401  (the (backend, dtype) fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NH = 3
SENTINEL = -777.25
DIMS = ("x", "y", "z")
NP_OF = {torch.float64: np.float64, torch.float32: np.float32}
STATE = ("ua", "va", "w", "pt", "delp", "delz", "peln", "pkz")
ROLE = dict(qv="qvapor", ql="qliquid", qr="qrain", qi="qice", qs="qsnow", qg="qgraupel")
# the tracer order of the moist cases: the harness's (vapour, liquid, ice, rain, snow, graupel), then the passive ones
MOIST = dict(qv=0, ql=1, qi=2, qr=3, qs=4, qg=5)
K = get_constants()
KAPPA = K.RDGAS / K.CP_AIR


@functools.lru_cache(maxsize=None)
def _grids(nx_tile, layout, nz):
    part = CubedSpherePartitioner(nx_tile, layout)
    return part, [make_grid(part, r, nz=nz) for r in range(part.total_ranks)]


def _factory(backend, nx_tile, layout, nz, dtype):
    part, grids = _grids(nx_tile, layout, nz)
    # (nord = 0: the fp32 context refuses the C12 del-6 damping tables, which overflow the float range; the operator reads none)
    cfg = AcousticDynamicsConfig(npx=nx_tile + 1, npy=nx_tile + 1, npz=nz, layout=layout, nord=0)
    return part, grids, stencil_factory_for(backend)(grids, cfg, get_constants(), dtype=dtype)


def _sync(sf):
    if not sf.hostemu:
        torch.cuda.synchronize()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _padded(cells, fill, dtype):
    """(nx, ny, nk) cells -> the (nx + 2 NH + 1, ny + 2 NH + 1, nz + 1) storage array (nk = nz, or nz + 1 for peln), `fill` elsewhere"""
    nx, ny, nk = cells.shape
    nz = nk if fill is not None else nk - 1
    a = np.full((nx + 2 * NH + 1, ny + 2 * NH + 1, nz + 1), SENTINEL if fill is None else fill, dtype=dtype)
    a[NH : NH + nx, NH : NH + ny, :nk] = cells
    return a


# ---------------------------------------------------------------------------------------------------------------------------------
# columns built to exercise the operator
# ---------------------------------------------------------------------------------------------------------------------------------
def make_columns(ncol, nz, npd, seed, n_q=0, moist=False, ptop=300.0, scales=(1.0, 8.0, 16.0)):
    """Seeded columns (float64 recipe, cast once): delp of 250 or 1000 Pa times a per-column scale (neighbours differ by a factor of
    4 in about half the pairs; the scales put the mid-level pressures below 200 hPa, between 200 and 400 hPa and above), potential
    temperature rising upwards by 3 - 9 % per level in the stable pairs and falling by 1 - 4 % in the inversions (40 % of the pairs),
    winds of a few m/s with a jump of 40 - 80 m/s in a fifth of the pairs, hydrostatic delz.  Returns ({field: (ncol, nz) array,
    peln: (ncol, nz + 1)}, [tracers])."""
    rng = np.random.default_rng(seed)
    delp = rng.choice([250.0, 1000.0], (ncol, nz)) * rng.choice(scales, (ncol, 1))
    pe = np.concatenate([np.full((ncol, 1), ptop), ptop + np.cumsum(delp, axis=1)], axis=1)
    peln = np.log(pe)
    pm = delp / (peln[:, 1:] - peln[:, :-1])
    pkz = np.exp(KAPPA * np.log(pm))
    theta = np.empty((ncol, nz))  # (in the units of the loop: T = theta * pkz with pkz = p^kappa)
    theta[:, nz - 1] = rng.uniform(220.0, 290.0, ncol) / pkz[:, nz - 1]
    kind = rng.random((ncol, nz))
    for k in range(nz - 2, -1, -1):
        step = np.where(kind[:, k] < 0.4, -rng.uniform(0.01, 0.04, ncol), rng.uniform(0.03, 0.09, ncol))
        theta[:, k] = theta[:, k + 1] * (1.0 + step)
    pt = theta * pkz
    u = rng.normal(0.0, 3.0, (ncol, nz)) + np.cumsum(np.where(rng.random((ncol, nz)) < 0.2, rng.uniform(40.0, 80.0, (ncol, nz)), 0.0), axis=1)
    v = rng.normal(0.0, 3.0, (ncol, nz))
    w = rng.normal(0.0, 0.5, (ncol, nz))
    delz = -(K.RDGAS / K.GRAV) * pt * delp / pm
    f = dict(ua=u, va=v, w=w, pt=pt, delp=delp, delz=delz, peln=peln, pkz=pkz)
    q = []
    if moist:
        q = [rng.uniform(0.0, 4.0e-3, (ncol, nz))] + [rng.uniform(0.0, 2.0e-4, (ncol, nz)) for _ in range(5)]
    q += [rng.uniform(0.0, 1.0, (ncol, nz)) for _ in range(n_q - len(q))]
    return {n: a.astype(npd) for n, a in f.items()}, [a.astype(npd) for a in q]


def run(backend, dtype, nx_tile, layout, nz, cols, water=None, n_sponge=None, fv_sg_adj=600, dt=225.0, ptop=300.0):
    """The operator on `cols` = [(f, q) per sub-domain] (make_columns' form): (after, before, op, (nx, ny)) with after / before
    {field: [storage arrays]} for the state fields, u_dt, v_dt and q0, q1, ..."""
    npd = NP_OF[dtype]
    part, grids, sf = _factory(backend, nx_tile, layout, nz, dtype)
    qf = sf.quantity_factory
    nx, ny = part.nx, part.ny
    assert len(cols) == len(grids)
    n_q = len(cols[0][1])
    host = {}
    for n in STATE:
        fill = None if n == "peln" else (1000.0 if n in ("delp", "pkz") else (-50.0 if n == "delz" else SENTINEL))
        host[n] = [_padded(f[n].reshape(nx, ny, -1), fill, npd) for f, _ in cols]
    for i in range(n_q):
        host[f"q{i}"] = [_padded(q[i].reshape(nx, ny, nz), SENTINEL, npd) for _, q in cols]
    host["u_dt"] = [np.full_like(a, SENTINEL) for a in host["ua"]]
    host["v_dt"] = [np.full_like(a, SENTINEL) for a in host["ua"]]
    dev = {n: qf.from_array(a, DIMS) for n, a in host.items()}
    tracers = {f"q{i}": dev[f"q{i}"] for i in range(n_q)}
    ws = None if water is None else WaterSpecies(**{ROLE[r]: dev[f"q{i}"] for r, i in water.items()})
    op = DryConvectiveAdjustment(sf, qf, grids, n_sponge=nz if n_sponge is None else n_sponge, fv_sg_adj=fv_sg_adj, water_species=ws, tracers=tracers, ptop=ptop)
    op(SimpleNamespace(**{n: dev[n] for n in STATE}), dev["u_dt"], dev["v_dt"], dt)
    _sync(sf)
    after = {n: [dev[n].numpy(r).copy() for r in range(len(grids))] for n in host}
    return after, host, op, (nx, ny)


def check_against_reference(after, host, op, shape, cols, water, nz, dt, tau):
    """Bitwise parity on the compute cells, the footprint everywhere else; returns the restatement's statistics added up."""
    nx, ny = shape
    n_q = len(cols[0][1])
    kb = min(op.kbot, nz)
    cs = (slice(NH, NH + nx), slice(NH, NH + ny), slice(0, nz))
    tot = dict(mixed=0, unmixed=0)
    for r, (f, q) in enumerate(cols):
        want, stats = sref.subgrid_z(f, q, water, kbot=op.kbot, dt=dt, tau=tau, t_min=op.t_min, t_max=op.t_max)
        tot["mixed"] += stats["mixed"]
        tot["unmixed"] += stats["unmixed"]
        pairs = [("pt", want["pt"]), ("w", want["w"]), ("u_dt", want["u_dt"]), ("v_dt", want["v_dt"])] + [(f"q{i}", want["q"][i]) for i in range(n_q)]
        for n, exp in pairs:
            got = after[n][r][cs].reshape(nx * ny, nz)
            bad = _bits(got) != _bits(exp)
            assert not bad.any(), (n, r, np.argwhere(bad)[:5], got[bad][:5], exp[bad][:5])
            # halo cells and the pad level keep what they held; so do the levels below the sponge (the tendencies are zero there)
            outside = np.ones(after[n][r].shape, dtype=bool)
            outside[cs] = False
            assert _same(after[n][r][outside], host[n][r][outside]), (n, r)
            if n in ("u_dt", "v_dt"):
                assert _same(got[:, kb:], np.zeros_like(got[:, kb:])), (n, r)
            else:
                assert _same(got[:, kb:], host[n][r][cs].reshape(nx * ny, nz)[:, kb:]), (n, r)
        for n in ("ua", "va", "delp", "delz", "peln", "pkz"):
            assert _same(after[n][r], host[n][r]), (n, r, "an input was written")
    return tot


SHAPES = [(12, (1, 1)), (12, (2, 2)), (12, (1, 2))]
SHAPE_IDS = ["c12_1x1", "c12_2x2", "c12_1x2"]
TRACERS = [("moist", 8, MOIST), ("dry3", 3, None), ("dry0", 0, None)]
SEED = 7  # (chosen on the host emulation: the branch shares asserted below hold for every shape and tracer set)


def _cols(nx_tile, layout, nz, npd, n_q, moist, seed=SEED, **kw):
    part, grids = _grids(nx_tile, layout, nz)
    return [make_columns(part.nx * part.ny, nz, npd, seed * 1000 + r, n_q=n_q, moist=moist, **kw) for r in range(len(grids))]


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. parity, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what, n_q, water", TRACERS, ids=[t[0] for t in TRACERS])
@pytest.mark.parametrize("nx_tile, layout", SHAPES, ids=SHAPE_IDS)
def test_matches_the_restatement_bitwise(real, nx_tile, layout, what, n_q, water):  # noqa: F811
    backend, dtype = real
    npd, nz = NP_OF[dtype], 6
    cols = _cols(nx_tile, layout, nz, npd, n_q, water is not None)
    after, host, op, shape = run(backend, dtype, nx_tile, layout, nz, cols, water=water)
    tot = check_against_reference(after, host, op, shape, cols, water, nz, 225.0, 600.0)
    n = tot["mixed"] + tot["unmixed"]
    print(f"subgrid_z {backend} {npd.__name__} C{nx_tile} {layout} {what}: {tot['mixed']} of {n} pairs mixed")
    assert 3 * tot["mixed"] >= n and 10 * tot["unmixed"] >= n, tot
    # neighbouring thicknesses really differ by a factor of 4
    f = cols[0][0]
    assert (np.maximum(f["delp"][:, 1:] / f["delp"][:, :-1], f["delp"][:, :-1] / f["delp"][:, 1:]) == 4).mean() > 0.3


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. every place the form changes
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_sponge", [0, 2, 3, 4, 5, 6, 9])
def test_kbot(real, n_sponge):  # noqa: F811
    backend, dtype = real
    npd, nz = NP_OF[dtype], 6
    cols = _cols(12, (1, 1), nz, npd, 8, True)
    after, host, op, shape = run(backend, dtype, 12, (1, 1), nz, cols, water=MOIST, n_sponge=n_sponge)
    assert op.kbot == min(n_sponge, nz)
    tot = check_against_reference(after, host, op, shape, cols, MOIST, nz, 225.0, 600.0)
    if n_sponge < 3:  # nothing happens: zero tendencies, the state bitwise
        assert tot["mixed"] == 0
        for n in ("pt", "w") + tuple(f"q{i}" for i in range(8)):
            assert all(_same(a, b) for a, b in zip(after[n], host[n])), n
        cs = (slice(NH, NH + 12), slice(NH, NH + 12), slice(0, nz))
        assert all(_same(a[cs], np.zeros_like(a[cs])) for a in after["u_dt"] + after["v_dt"])
    else:
        assert tot["mixed"] > 0


def _quiet_column(cols, npd, col, temperatures):
    """`cols` with column `col` of every sub-domain at rest and at the given temperatures (K, per level): isothermal stretches are
    stable (the potential temperature grows upwards with 1 / pkz) and, without wind, far above every ri_ref"""
    for f, _ in cols:
        f["ua"][col], f["va"][col], f["w"][col] = npd(0), npd(0), npd(0)
        f["pt"][col] = np.asarray(temperatures, dtype=npd)
    return cols


@pytest.mark.parametrize("n_sponge", [23, 24])
def test_t_max_switch(real, n_sponge):  # noqa: F811
    """nz = 26: kbot = 23 < min(nz, 24) takes t_max = 315 K, kbot = 24 takes 325 K; column 5 holds a pair whose upper level is at
    320 K in an isothermal column at rest of 250 K: mixed under 315 K only (ri = 0), stable otherwise."""
    backend, dtype = real
    npd, nz = NP_OF[dtype], 26
    cols = _cols(12, (1, 1), nz, npd, 3, False, scales=(1.0,))
    cols = _quiet_column(cols, npd, 5, [250.0] * 9 + [320.0] + [250.0] * 16)
    after, host, op, shape = run(backend, dtype, 12, (1, 1), nz, cols, n_sponge=n_sponge)
    assert op.t_max == (315.0 if n_sponge == 23 else 325.0)
    check_against_reference(after, host, op, shape, cols, None, nz, 225.0, 600.0)
    f, q = cols[0]
    mc = {t: sref.subgrid_z(f, q, None, kbot=n_sponge, dt=225.0, tau=600.0, t_min=165.0, t_max=t)[1]["mc"][0, 5, 10] for t in (315.0, 325.0)}
    assert mc[315.0] > 0 and mc[325.0] == 0, mc  # the switch decides this pair


@pytest.mark.parametrize("ptop", [1.0, 300.0])
def test_t_min_switch(real, ptop):  # noqa: F811
    """ptop below 2 Pa takes t_min = 160 K, else 165 K; column 5 holds a pair whose lower level is at 162 K under 200 K: ri is
    capped at 0.1 (and the pair mixes) under 165 K only; the column is at rest and stable, its lowest level at 163 K."""
    backend, dtype = real
    npd, nz = NP_OF[dtype], 6
    cols = _cols(12, (1, 1), nz, npd, 3, False, ptop=ptop)
    cols = _quiet_column(cols, npd, 5, [200.0] * 4 + [162.0, 163.0])
    after, host, op, shape = run(backend, dtype, 12, (1, 1), nz, cols, ptop=ptop)
    assert op.t_min == (160.0 if ptop < 2.0 else 165.0)
    check_against_reference(after, host, op, shape, cols, None, nz, 225.0, 600.0)
    f, q = cols[0]
    mc = {t: sref.subgrid_z(f, q, None, kbot=nz, dt=225.0, tau=600.0, t_min=t, t_max=325.0)[1]["mc"][0, 5, 4] for t in (160.0, 165.0)}
    assert mc[165.0] > 0 and mc[160.0] == 0, mc


@pytest.mark.parametrize("dt, tau", [(225.0, 600), (600.0, 600), (900.0, 600)], ids=["fra_lt_1", "fra_eq_1", "fra_gt_1"])
def test_relaxation(real, dt, tau):  # noqa: F811
    backend, dtype = real
    npd, nz = NP_OF[dtype], 6
    cols = _cols(12, (1, 1), nz, npd, 8, True)
    after, host, op, shape = run(backend, dtype, 12, (1, 1), nz, cols, water=MOIST, fv_sg_adj=tau, dt=dt)
    tot = check_against_reference(after, host, op, shape, cols, MOIST, nz, dt, float(tau))
    assert tot["mixed"] > 0


def test_ri_ref_regimes(real):  # noqa: F811
    """The mid-level pressure delp / dlog(p) of the pairs' lower levels lies below 200 hPa (ri_ref = 1), between 200 and 400 hPa
    (the ramp) and above 400 hPa (0.25): every regime holds at least a tenth of the pairs of the parity test's columns."""
    backend, dtype = real
    npd, nz = NP_OF[dtype], 6
    cols = _cols(12, (1, 1), nz, npd, 0, False)
    pm = np.concatenate([(f["delp"] / (f["peln"][:, 1:] - f["peln"][:, :-1]))[:, 1:].ravel() for f, _ in cols]).astype(np.float64)
    shares = [(pm < 200.0e2).mean(), ((pm > 200.0e2) & (pm < 400.0e2)).mean(), (pm > 400.0e2).mean()]
    assert min(shares) > 0.1, shares  # (none of the three is a rare case)
    after, host, op, shape = run(backend, dtype, 12, (1, 1), nz, cols)
    check_against_reference(after, host, op, shape, cols, None, nz, 225.0, 600.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. hand-computed columns: dyadic inputs; every step of the three passes written out with one rounded operation per line
# ---------------------------------------------------------------------------------------------------------------------------------
def _hand_column(npd, nz=6):
    """A column that is stable everywhere: potential temperature quadruples from one level to the next one up, no wind"""
    f = dict(ua=np.zeros(nz), va=np.zeros(nz), w=np.zeros(nz), pt=np.full(nz, 256.0), delp=np.full(nz, 2.0), delz=np.full(nz, -64.0),
             peln=np.log(300.0 + 2.0 * np.arange(nz + 1)), pkz=4.0 ** np.arange(-nz + 1, 1.0))
    return {n: a.astype(npd) for n, a in f.items()}, [np.full(nz, 0.5).astype(npd)]


def _hand_pair(npd, f, q, k, t_max, mult):
    """The three passes of the pair (k-1, k) of a dry column in which no other pair mixes, one rounded operation per step; `mult`:
    the factor on ri_ref at this k.  Returns the final (u, v, w, t, q) of the two levels (before the relaxation) and mc per pass."""
    c = sref.constants(npd, False)
    one, zero, half = npd(1), npd(0), npd(0.5)
    m = k - 1
    nz = len(f["pt"])
    gz, gzh = [None] * nz, zero
    for kk in range(nz - 1, -1, -1):
        gz[kk] = gzh - c["g2"] * f["delz"][kk]
        gzh = gzh - c["grav"] * f["delz"][kk]
    X = {n: [f[s][m], f[s][k]] for n, s in (("u", "ua"), ("v", "va"), ("w", "w"), ("t", "pt"))}
    X["q"] = [q[0][m], q[0][k]]
    dpm, dpk = f["delp"][m], f["delp"][k]
    tvol = lambda i, kk: gz[kk] + half * ((X["u"][i] * X["u"][i] + X["v"][i] * X["v"][i]) + X["w"][i] * X["w"][i])  # noqa: E731
    mcs = []
    for n in (1, 2, 3):
        ratio = npd(n) / npd(3)
        te = [c["cv_air"] * X["t"][0] + tvol(0, m), c["cv_air"] * X["t"][1] + tvol(1, k)]
        tv1, tv2 = X["t"][0] * ((one + zero) - zero), X["t"][1] * ((one + zero) - zero)
        pt1, pt2 = tv1 / f["pkz"][m], tv2 / f["pkz"][k]
        du, dv = X["u"][0] - X["u"][1], X["v"][0] - X["v"][1]
        ri = ((gz[m] - gz[k]) * (pt1 - pt2)) / ((half * (pt1 + pt2)) * ((du * du + dv * dv) + npd(1.0e-4)))
        if tv1 > npd(t_max) and tv1 > tv2:
            ri = zero
        pm = dpk / (f["peln"][k + 1] - f["peln"][k])
        assert pm < 200.0e2  # ri_ref = min(1, 0.25 + 0.75 * (400e2 - pm) / 200e2) = 1
        d = npd(400.0e2) - pm
        ri_ref = npd(0.25) + (npd(0.75) * d) / npd(200.0e2)
        ri_ref = npd(mult) * (one if one < ri_ref else ri_ref)
        x = ri / ri_ref
        r = one - (zero if zero > x else x)
        mc = (((ratio * dpm) * dpk) / (dpm + dpk)) * (r * r) if ri < ri_ref else zero
        mcs.append(mc)
        if mc > zero:
            X["te"] = te
            for n_ in ("q", "u", "v", "te", "w"):
                h0 = mc * (X[n_][1] - X[n_][0])
                X[n_] = [X[n_][0] + h0 / dpm, X[n_][1] - h0 / dpk]
            X["t"] = [(X["te"][0] - tvol(0, m)) / c["cv_air"], (X["te"][1] - tvol(1, k)) / c["cv_air"]]
    assert all(type(v) is npd for n_ in ("u", "v", "w", "t", "q") for v in X[n_])
    return X, mcs


@pytest.mark.parametrize("k", [5, 1])
def test_hand_computed_columns(real, k):  # noqa: F811
    """One pair in a column that is stable everywhere else.  k = 5: the upper level at 512 K is above t_max = 325 K and warmer than
    the lower one, so ri = 0 and mc = ratio * 2 * 2 / 4 = ratio in all three passes (the third pass leaves the pair's total energy
    equal).  k = 1: a weak shear puts ri between 1 and 4, so the pair mixes only because ri_ref is 4 there."""
    backend, dtype = real
    npd, nz = NP_OF[dtype], 6
    f, q = _hand_column(npd)
    m = k - 1
    q[0][m], q[0][k] = npd(0.25), npd(0.75)
    f["w"][m], f["w"][k] = npd(0.5), npd(-0.25)
    if k == 5:
        f["pt"][m] = npd(512.0)
        f["ua"][m], f["ua"][k], f["va"][k] = npd(0.125), npd(-0.125), npd(0.0625)
    else:
        f["ua"][m], f["ua"][k] = npd(16.0), npd(-8.0)
    X, mcs = _hand_pair(npd, f, q, k, 325.0, 4 if k == 1 else 1)
    if k == 5:
        assert mcs == [npd(1) / npd(3), npd(2) / npd(3), npd(1)]
    else:
        assert all(mc > 0 for mc in mcs)
        assert _hand_pair(npd, f, q, k, 325.0, 1)[1] == [0, 0, 0]  # without the factor 4 the pair would be stable
    # the expected column: fra = 1 (dt = tau), so the outputs are the mixed values and the tendencies (u0 - ua) / dt
    dt = 512.0
    rdt = npd(1.0 / dt)
    want = dict(pt=f["pt"].copy(), w=f["w"].copy(), q0=q[0].copy(), u_dt=np.zeros(nz, npd), v_dt=np.zeros(nz, npd))
    for i, kk in enumerate((m, k)):
        want["pt"][kk], want["w"][kk], want["q0"][kk] = X["t"][i], X["w"][i], X["q"][i]
        want["u_dt"][kk], want["v_dt"][kk] = rdt * (X["u"][i] - f["ua"][kk]), rdt * (X["v"][i] - f["va"][kk])
    part, grids = _grids(12, (1, 1), nz)
    # the column sits at cell 17 of every sub-domain among copies of the stable column
    base_f, base_q = _hand_column(npd)
    cols = []
    for _ in grids:
        ff = {n: np.tile(a, (144, 1)) for n, a in base_f.items()}
        qq = [np.tile(base_q[0], (144, 1))]
        for n in ff:
            ff[n][17] = f[n]
        qq[0][17] = q[0]
        cols.append((ff, qq))
    after, host, op, (nx, ny) = run(backend, dtype, 12, (1, 1), nz, cols, fv_sg_adj=512, dt=dt)
    cs = (slice(NH, NH + nx), slice(NH, NH + ny), slice(0, nz))
    for r in range(len(grids)):
        for n in ("pt", "w", "q0", "u_dt", "v_dt"):
            got = after[n][r][cs].reshape(144, nz)
            exp = np.zeros((144, nz), npd) if n in ("u_dt", "v_dt") else host[n][r][cs].reshape(144, nz).copy()
            exp[17] = want[n]
            assert _same(got, exp), (n, r, got[17], want[n], np.argwhere(_bits(got) != _bits(exp))[:4])
    assert after["pt"][0][cs].reshape(144, nz)[17, m] != f["pt"][m]


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. pins that do not use the restatement
# ---------------------------------------------------------------------------------------------------------------------------------
def test_stable_column_at_rest_is_untouched(real):  # noqa: F811
    backend, dtype = real
    npd, nz = NP_OF[dtype], 6
    part, grids = _grids(12, (1, 1), nz)
    f, q = _hand_column(npd)
    q = q + [np.linspace(-0.0, 1.0, nz).astype(npd)]  # (a negative zero: `a + (a - a) * fra` would turn it into +0)
    q[1][0] = npd(-0.0)
    cols = [({n: np.tile(a, (144, 1)) for n, a in f.items()}, [np.tile(a, (144, 1)) for a in q]) for _ in grids]
    after, host, op, (nx, ny) = run(backend, dtype, 12, (1, 1), nz, cols)
    cs = (slice(NH, NH + nx), slice(NH, NH + ny), slice(0, nz))
    for r in range(len(grids)):
        for n in ("pt", "w", "q0", "q1"):
            assert _same(after[n][r], host[n][r]), (n, r)
        for n in ("u_dt", "v_dt"):
            assert _same(after[n][r][cs], np.zeros((nx, ny, nz), npd)), (n, r)


def _moist_energy(npd, f, q, pt, w, u, v, kb):
    """float64: (cvm T + gz + ke) of levels 0 .. kb-1 from the given fields"""
    d = lambda a: np.asarray(a, dtype=np.float64)[:, :kb]  # noqa: E731
    c = {n: float(x) for n, x in sref.constants(npd, True).items()}
    sp = {r: d(q[i]) for r, i in MOIST.items()}
    q_liq, q_sol = sp["ql"] + sp["qr"], sp["qi"] + sp["qs"] + sp["qg"]
    cvm = (1.0 - (sp["qv"] + q_liq + q_sol)) * c["cv_air"] + sp["qv"] * c["cv_vap"] + q_liq * c["c_liq"] + q_sol * c["c_ice"]
    dz = d(f["delz"])
    below = np.concatenate([np.cumsum(dz[:, ::-1], axis=1)[:, ::-1][:, 1:], np.zeros((dz.shape[0], 1))], axis=1)
    gz = -c["grav"] * below - c["g2"] * dz
    return cvm * d(pt), gz, 0.5 * (d(u) ** 2 + d(v) ** 2 + d(w) ** 2)


@pytest.mark.parametrize("dt", [600.0, 225.0], ids=["fra_eq_1", "fra_lt_1"])
def test_column_sums_are_conserved(real, dt):  # noqa: F811
    """The mixing exchanges mass-weighted amounts between two levels: sum delp q, sum delp (ua + dt u_dt), sum delp w and (fra >= 1)
    sum delp (cvm T + gz + ke) over the sponge keep their values within 16 kbot eps sum |terms|; the sums are formed in float64."""
    backend, dtype = real
    npd, nz = NP_OF[dtype], 6
    eps = float(np.finfo(npd).eps)
    cols = _cols(12, (1, 1), nz, npd, 8, True)
    after, host, op, (nx, ny) = run(backend, dtype, 12, (1, 1), nz, cols, water=MOIST, dt=dt)
    kb = op.kbot
    cs = (slice(NH, NH + nx), slice(NH, NH + ny), slice(0, nz))
    worst = 0.0
    for r, (f, q) in enumerate(cols):
        g = {n: after[n][r][cs].reshape(nx * ny, nz) for n in after}
        dp = f["delp"].astype(np.float64)[:, :kb]
        d = lambda a: np.asarray(a, dtype=np.float64)[:, :kb]  # noqa: E731

        def conserved(before, now, what):
            nonlocal worst
            s0, s1, scale = (dp * before).sum(axis=1), (dp * now).sum(axis=1), (dp * np.abs(before)).sum(axis=1)
            err = np.abs(s1 - s0) / (eps * scale)
            worst = max(worst, float(err.max()))
            assert (err <= 16 * kb).all(), (what, r, float(err.max()))

        for i in range(8):
            conserved(d(q[i]), d(g[f"q{i}"]), f"q{i}")
        u1, v1 = d(f["ua"]) + dt * d(g["u_dt"]), d(f["va"]) + dt * d(g["v_dt"])
        conserved(d(f["ua"]), u1, "u")
        conserved(d(f["va"]), v1, "v")
        conserved(d(f["w"]), d(g["w"]), "w")
        if dt >= 600.0:
            a = _moist_energy(npd, f, q, f["pt"], f["w"], f["ua"], f["va"], kb)
            b = _moist_energy(npd, f, [g[f"q{i}"] for i in range(8)], g["pt"], g["w"], u1, v1, kb)
            s0, s1 = (dp * sum(a)).sum(axis=1), (dp * sum(b)).sum(axis=1)
            scale = (dp * sum(np.abs(x) for x in a)).sum(axis=1)
            err = np.abs(s1 - s0) / (eps * scale)
            worst = max(worst, float(err.max()))
            assert (err <= 16 * kb).all(), ("energy", r, float(err.max()))
        assert not _same(g["pt"], f["pt"])
    print(f"subgrid_z {backend} {npd.__name__} dt {dt:g}: worst column-sum error {worst:.2f} eps sum|terms| (bound {16 * kb})")


def test_largest_inversion_does_not_grow(real):  # noqa: F811
    """Unstable columns (every pair an inversion of 0.5 - 3 %, no wind): max_k (pt2 - pt1) of the potential temperatures after the
    adjustment is at most what it was.  The mixing drives the total energy cv T + gz of a pair towards equality, which leaves
    T1 - T2 = -g dz / cv where neutral stratification has -g dz / cp: a residual inversion of g dz (1 / cv - 1 / cp) / T that does not
    depend on the one the pair started with: the property is one of layers that are thin against the inversion they carry.  It is
    also one of layers of equal mass.  A pair with inversion D exchanges the share a = mc / delp = ratio / 2 (r = 1 where ri < 0): D
    becomes D (1 - 2a), the inversion d of the pair above becomes d + a D before that pair is mixed in turn, so after a pass the two
    hold at most (2/3 + 1/9), (1/3 + 1/9), 0 and (25/36 + 1/6), (4/9 + 1/3), (1/4 + 1/2) of the larger of D and d in passes 1, 2, 3: below
    1 every time.  With a thin layer next to a thick one the thin one takes nearly the thick one's value and the inversion next to
    it becomes nearly the SUM of the two, so no such bound exists there.  The columns: 250 Pa layers below 500 hPa (40 m deep, residual
    below 0.1 %)."""
    backend, dtype = real
    npd, nz = NP_OF[dtype], 6
    part, grids = _grids(12, (1, 1), nz)
    rng = np.random.default_rng(3)
    cols = []
    for _ in grids:
        f, _q = make_columns(144, nz, npd, 1, ptop=500.0e2, scales=(1.0,))
        f64 = {n: a.astype(np.float64) for n, a in f.items()}
        f64["delp"] = np.full((144, nz), 250.0)
        pe = 500.0e2 + 250.0 * np.arange(nz + 1)
        f64["peln"] = np.tile(np.log(pe), (144, 1))
        pm = f64["delp"] / (f64["peln"][:, 1:] - f64["peln"][:, :-1])
        f64["pkz"] = np.exp(KAPPA * np.log(pm))
        f64["delz"] = -(K.RDGAS / K.GRAV) * 250.0 * f64["delp"] / pm
        theta = 11.5 * np.cumprod(1.0 + rng.uniform(0.005, 0.03, (144, nz)), axis=1)  # grows downwards: unstable everywhere
        f64["pt"] = theta * f64["pkz"]
        f64["ua"], f64["va"], f64["w"] = np.zeros((144, nz)), np.zeros((144, nz)), np.zeros((144, nz))
        cols.append(({n: a.astype(npd) for n, a in f64.items()}, []))
    after, host, op, (nx, ny) = run(backend, dtype, 12, (1, 1), nz, cols, fv_sg_adj=225, dt=225.0)
    cs = (slice(NH, NH + nx), slice(NH, NH + ny), slice(0, nz))
    for r, (f, _q) in enumerate(cols):
        th0 = f["pt"].astype(np.float64) / f["pkz"].astype(np.float64)
        th1 = after["pt"][r][cs].reshape(144, nz).astype(np.float64) / f["pkz"].astype(np.float64)
        inv0, inv1 = (th0[:, 1:] - th0[:, :-1]).max(axis=1), (th1[:, 1:] - th1[:, :-1]).max(axis=1)
        assert (inv0 > 0).all()
        assert (inv1 <= inv0).all(), (r, float((inv1 - inv0).max()))


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. argument checks through the C ABI and the Python refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def test_argument_checks(backend):
    nz = 6
    npd = np.float64
    part, grids, sf = _factory(backend, 12, (1, 1), nz, torch.float64)
    qf = sf.quantity_factory
    cols = _cols(12, (1, 1), nz, npd, 8, True)
    host = {n: [_padded(f[n].reshape(12, 12, -1), None if n == "peln" else 1000.0, npd) for f, _ in cols] for n in STATE}
    for i in range(8):
        host[f"q{i}"] = [_padded(q[i].reshape(12, 12, nz), SENTINEL, npd) for _, q in cols]
    q = {n: qf.from_array(a, DIMS) for n, a in host.items()}
    q["u_dt"], q["v_dt"] = qf.zeros(DIMS), qf.zeros(DIMS)
    work = [qf.zeros(DIMS) for _ in range(13)]
    flat = qf.zeros(("x", "y"))
    short = _lib.fv3_field()
    C.memmove(C.byref(short), C.byref(q["peln"].field), C.sizeof(_lib.fv3_field))
    short.shape[2] -= 1
    everything = dict(q, **{f"work{i}": w for i, w in enumerate(work)})
    before = {n: v.storage.clone() for n, v in everything.items()}
    lib, ctx, s = sf.lib, sf.ctx, sf.stream_handle

    def ref(v):
        return None if v is None else (C.pointer(v) if isinstance(v, _lib.fv3_field) else C.pointer(v.field))

    def call(no_ctx=False, no_params=False, water=True, n_tr=8, tr=None, n_work=13, wk=None, species=None, dt=225.0, tau=600.0, kbot=6, **swap):
        f = {k: swap.get(k, q[k]) for k in STATE + ("u_dt", "v_dt")}
        tr = [q[f"q{i}"] for i in range(n_tr)] if tr is None else tr
        wk = work if wk is None else wk
        sp = dict({r: q[f"q{i}"] for r, i in MOIST.items()}, **(species or {}))
        wstruct = _lib.fv3_water(*[ref(sp[r]) for r in ("qv", "ql", "qr", "qi", "qs", "qg")], pc.CV_VAP, pc.C_LIQ, pc.C_ICE)
        params = _lib.fv3_subgridz_params(dt, tau, 165.0, 325.0, kbot)
        tarr = (_lib.F * max(len(tr), 1))(*[ref(t) for t in tr])
        warr = (_lib.F * max(len(wk), 1))(*[ref(w) for w in wk])
        return lib.fv3_subgrid_z(None if no_ctx else ctx, None if no_params else C.byref(params), C.byref(wstruct) if water else None, n_tr, tarr if tr else None,
                                 *[ref(f[k]) for k in STATE + ("u_dt", "v_dt")], n_work, warr if wk else None, s)

    ARG = -1
    assert call(no_ctx=True) == ARG
    cases = [
        ("null params", dict(no_params=True), b"fv3_subgridz_params is null"),
        ("dt = 0", dict(dt=0.0), b"dt must be finite and > 0"),
        ("dt < 0", dict(dt=-1.0), b"dt must be finite and > 0"),
        ("dt = inf", dict(dt=float("inf")), b"dt must be finite and > 0"),
        ("dt = nan", dict(dt=float("nan")), b"dt must be finite and > 0"),
        ("tau = 0", dict(tau=0.0), b"tau must be > 0"),
        ("tau < 0", dict(tau=-600.0), b"tau must be > 0"),
        ("kbot < 0", dict(kbot=-1), b"kbot = -1 is negative"),
        ("short peln", dict(peln=short), b"'peln': vertical shape"),
        ("too few work fields", dict(n_work=12), b"12 work fields given, 13 needed"),
        ("no work fields", dict(n_work=0, wk=[]), b"0 work fields given, 13 needed"),
        ("null work field", dict(wk=work[:4] + [None] + work[5:]), b"'work 4': null"),
        ("2-D work field", dict(wk=[flat] + work[1:]), b"'work 0': vertical shape"),
        ("null tracer", dict(tr=[q["q0"], None] + [q[f"q{i}"] for i in range(2, 8)]), b"'tracer 1': null"),
        ("a tracer given twice", dict(tr=[q[f"q{i}"] for i in range(7)] + [q["q6"]]), b"tracer 6 and tracer 7 are the same field"),
        ("a species outside the tracers", dict(n_tr=7, tr=[q[f"q{i}"] for i in range(1, 8)]), b"qvapor is not among the tracers"),
        ("null qvapor", dict(species=dict(qv=None)), b"'qvapor': null"),
        ("2-D qsnow", dict(species=dict(qs=flat)), b"'qsnow': vertical shape"),
        ("two roles one field", dict(species=dict(qr=q["q1"])), b"qliquid and qrain are the same field"),
        ("u_dt is v_dt", dict(v_dt=q["u_dt"]), b"u_dt and v_dt are the same field"),
        ("u_dt is ua", dict(u_dt=q["ua"]), b"ua and u_dt are the same field"),
        ("v_dt is a tracer", dict(v_dt=q["q3"]), b"v_dt and tracer 3 are the same field"),
        ("pt is w", dict(pt=q["w"]), b"w and pt are the same field"),
        ("pt is delp", dict(delp=q["pt"]), b"pt and delp are the same field"),
        ("a work field is pkz", dict(wk=work[:2] + [q["pkz"]] + work[3:]), b"pkz and work 2 are the same field"),
        ("a work field twice", dict(wk=work[:12] + [work[0]]), b"work 0 and work 12 are the same field"),
        ("a work field is u_dt", dict(wk=[q["u_dt"]] + work[1:]), b"u_dt and work 0 are the same field"),
        ("a work field is a tracer", dict(wk=work[:5] + [q["q7"]] + work[6:]), b"tracer 7 and work 5 are the same field"),
    ] + [(f"null {n}", {n: None}, f"'{n}': null".encode()) for n in STATE + ("u_dt", "v_dt")] + [
        (f"2-D {n}", {n: flat}, f"'{n}': vertical shape".encode()) for n in STATE + ("u_dt", "v_dt")]
    for what, kw, word in cases:
        assert call(ua=flat) == ARG and b"'ua': vertical shape" in lib.fv3_last_error(ctx)  # (another message in between: the one below is this case's own)
        st = call(**kw)
        msg = lib.fv3_last_error(ctx)
        assert st == ARG, (what, st)
        assert msg and word in msg, (what, msg)
        _sync(sf)
        for n, v in everything.items():
            assert torch.equal(v.storage, before[n]), (what, n)
    # fewer work fields are needed without passive tracers, and dry without tracers
    assert call(n_tr=6, tr=[q[f"q{i}"] for i in range(6)], n_work=7) == ARG and b"7 work fields given, 8 needed" in lib.fv3_last_error(ctx)
    assert call(water=False, n_tr=0, tr=[], n_work=1) == ARG and b"1 work fields given, 2 needed" in lib.fv3_last_error(ctx)
    # the Python refusals, one sentence each
    with pytest.raises(ValueError, match="fv_sg_adj = 0") as e:
        DryConvectiveAdjustment(sf, qf, grids, n_sponge=6, fv_sg_adj=0)
    assert str(e.value).count(". ") == 0
    with pytest.raises(ValueError, match="fv_sg_adj = -600"):
        DryConvectiveAdjustment(sf, qf, grids, n_sponge=6, fv_sg_adj=-600)
    with pytest.raises(NotImplementedError, match="non-hydrostatic") as e:
        DryConvectiveAdjustment(sf, qf, grids, n_sponge=6, fv_sg_adj=600, hydrostatic=True)
    assert str(e.value).count(". ") == 0
    with pytest.raises(NotImplementedError, match="DryConvectiveAdjustment"):
        ApplyPhysicsToDycore(sf, qf, grids, do_sg_conv=True)
    # ... and a call that passes, with kbot clipped to nz, changes pt
    assert call(kbot=9) == 0
    _sync(sf)
    assert not torch.equal(q["pt"].storage, before["pt"]) and torch.equal(q["delp"].storage, before["delp"])


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. register budget (read from the code-object metadata of the built library: no GPU needed)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [64, 32])
def test_subgridz_kernels_stay_inside_the_register_budget(precision):
    """The walk holds two level records and a prefetched third: two waves per SIMD (256 architectural VGPRs) is the ceiling, nothing
    spilled, no scratch, no LDS -- for the moist and the dry main walk and for every group size of the passive kernel."""
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
    main = {n: k for n, k in ks.items() if "subgridz_columns" in n}
    passive = {n: k for n, k in ks.items() if "subgridz_passive" in n}
    assert len(main) == 2 and len(passive) == 4, (sorted(main), sorted(passive))
    for n, k in {**main, **passive}.items():
        assert k["vgpr"] - k["agpr"] <= 256 and k["spill"] == 0 and k["scratch"] == 0 and k["lds"] == 0, (n[:100], k)
