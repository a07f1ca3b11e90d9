"""fv3_neg_adj3 (pace_amd/csrc/fv3_negadj.hip) through AdjustNegativeTracerMixingRatio and the C ABI: hand-computed columns, bitwise
parity with the numpy restatement (tests/negadj_reference.py) on random columns and on the restart fixture in fp64 and fp32, the
properties of the result, the argument checks, the register budget of the kernel.  Every operator case runs on the host emulation
(CPU suite) and on the HIP library (-m gpu)."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

import negadj_reference as nref
from pace_amd import constants as pc, lib as _lib
from pace_amd._testing import stencil_factory_for
from pace_amd.config import AcousticDynamicsConfig
from pace_amd.constants import get_constants
from pace_amd.grid import make_grid
from pace_amd.stencils import AdjustNegativeTracerMixingRatio, WaterSpecies
from pace_amd.topology import CubedSpherePartitioner
from test_fillz import real  # noqa: F401  (the (backend, dtype) fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "c12_restart_6tiles.npz")
NH = 3
SENTINEL = -777.25  # negative: a kernel that touched a halo cell or the pad level would try to fix it
DIMS = ("x", "y", "z")
NP_OF = {torch.float64: np.float64, torch.float32: np.float32}
SPECIES = ("qv", "ql", "qr", "qi", "qs", "qg")  # the restatement's names, in the order of fv3_water
ROLE = dict(qv="qvapor", ql="qliquid", qr="qrain", qi="qice", qs="qsnow", qg="qgraupel")
FIELDS = SPECIES + ("pt", "dp")


@functools.lru_cache(maxsize=None)
def _grids(nx_tile, layout, nz):
    part = CubedSpherePartitioner(nx_tile, layout)
    return part, [make_grid(part, r, nz=nz) for r in range(part.total_ranks)]


def _factory(backend, nx_tile, layout, nz, dtype):
    part, grids = _grids(nx_tile, layout, nz)
    # (nord = 0: the fp32 context refuses the C12 del-6 damping tables, which overflow the float range; neg_adj3 reads none)
    cfg = AcousticDynamicsConfig(npx=nx_tile + 1, npy=nx_tile + 1, npz=nz, layout=layout, nord=0)
    return part, grids, stencil_factory_for(backend)(grids, cfg, get_constants(), dtype=dtype)


def _sync(sf):
    if not sf.hostemu:
        torch.cuda.synchronize()


def _padded(cells, fill, dtype):
    """(n, n, nz) compute cells -> the (n + 2 NH + 1, n + 2 NH + 1, nz + 1) storage array, `fill` everywhere else."""
    n, _, nz = cells.shape
    a = np.full((n + 2 * NH + 1, n + 2 * NH + 1, nz + 1), fill, dtype=dtype)
    a[NH : NH + n, NH : NH + n, :nz] = cells
    return a


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _upload(qf, cells, npd):
    """{field: [compute cells per sub-domain]} -> ({field: Quantity}, {field: [storage arrays]}); dp's halo is a plain thickness"""
    host = {f: [_padded(a, 1000.0 if f == "dp" else SENTINEL, npd) for a in cells[f]] for f in FIELDS}
    return {f: qf.from_array(host[f], DIMS) for f in FIELDS}, host


def _apply(sf, qf, grids, q, positional=True):
    op = AdjustNegativeTracerMixingRatio(sf, qf, grids)
    if positional:  # the reference's argument order: snow before ice
        op(q["qv"], q["ql"], q["qr"], q["qs"], q["qi"], q["qg"], None, q["pt"], q["dp"], None, None)
    else:
        op(pt=q["pt"], delp=q["dp"], water=WaterSpecies(**{ROLE[s]: q[s] for s in SPECIES}))
    _sync(sf)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. hand-computed columns: dyadic species values, exact in both precisions; pt from the formula evaluated for that cell
# ---------------------------------------------------------------------------------------------------------------------------------
CLEAN = dict(qv=0.25, ql=0.25, qr=0.25, qi=0.25, qs=0.25, qg=0.25, pt=280.0, dp=1.0)


def _heat(npd, cell, qg_neg=None, ql_neg=None):
    """pt of a cell after the heating branches: `cell` holds its incoming values, qg_neg / ql_neg the negative graupel / liquid values
    the branches see (None: branch not taken).  One rounded operation per step, in the order of the specification."""
    k = nref.constants(npd)
    v = {f: npd(cell[f]) for f in cell}
    zero, one = npd(0), npd(1)
    s = v["ql"] + v["qr"]
    q_liq = s if s > zero else zero
    s = v["qi"] + v["qs"]
    q_sol = s if s > zero else zero
    cpm = (((one - ((v["qv"] + q_liq) + q_sol)) * k["cv_air"] + v["qv"] * k["cv_vap"]) + q_liq * k["c_liq"]) + q_sol * k["c_ice"]
    lcpk = (k["lv00"] + k["d0_vap"] * v["pt"]) / cpm
    icpk = (k["li00"] + k["dc_ice"] * v["pt"]) / cpm
    pt = v["pt"]
    if qg_neg is not None:
        pt = pt - npd(qg_neg) * icpk
    if ql_neg is not None:
        pt = pt - npd(ql_neg) * lcpk
    assert type(pt) is npd
    return pt


def _hand_cases(nz):
    """[(incoming {field: column}, expected {field: column or callable(npd) -> column})]; fields not named are CLEAN"""
    c = lambda x: [x] * nz  # noqa: E731
    cases = []
    # a single qi < 0 on level 1: paid by the snow of the cell
    cases.append((dict(qi=[0.25, -0.125] + [0.25] * (nz - 2)), dict(qi=[0.25, 0.0] + [0.25] * (nz - 2), qs=[0.25, 0.125] + [0.25] * (nz - 2))))
    # the full cascade qi -> qs -> qg -> qr -> ql -> qv on level 0, both heatings; the vapour stays positive
    cell = dict(qv=0.5, ql=0.03125, qr=0.0625, qi=-0.5, qs=0.25, qg=0.125, pt=280.0)
    inc = {f: [cell[f]] + [CLEAN[f]] * (nz - 1) for f in cell}
    exp = dict(qi=[0.0] + c(0.25)[1:], qs=[0.0] + c(0.25)[1:], qg=[0.0] + c(0.25)[1:], qr=[0.0] + c(0.25)[1:], ql=[0.0] + c(0.25)[1:], qv=[0.46875] + c(0.25)[1:],
               pt=lambda npd, cell=cell: [_heat(npd, cell, qg_neg=-0.125, ql_neg=-0.03125)] + [npd(280.0)] * (nz - 1))
    cases.append((inc, exp))
    # a level whose ql < 0 turns its qv negative, which is then carried down (level 1 -> level 2; dp = 1)
    cell = dict(CLEAN, ql=-0.375)
    cases.append((dict(ql=[0.25, -0.375] + [0.25] * (nz - 2)),
                  dict(ql=[0.25, 0.0] + [0.25] * (nz - 2), qv=[0.25, 0.0, 0.125] + [0.25] * (nz - 3),
                       pt=lambda npd, cell=cell: [npd(280.0), _heat(npd, cell, ql_neg=-0.375)] + [npd(280.0)] * (nz - 2))))
    if nz == 3:
        cases.append((dict(qv=[-1, 1, 1], dp=[2, 1, 4]), dict(qv=[0, 0, 0.75])))
        cases.append((dict(qv=[1, 2, -1]), dict(qv=[1, 1, 0])))  # the bottom borrow
    else:
        cases.append((dict(qv=[-1, 0.5, 2, 1]), dict(qv=[0, 0, 1.5, 1])))
        cases.append((dict(qv=[1, 1, 2, -1]), dict(qv=[1, 1, 1, 0])))
        cases.append((dict(qv=[1, 1, 0.5, -1]), dict(qv=[1, 1, 0, -0.5])))
        cases.append((dict(qv=[1, 1, -1, -1]), dict(qv=[1, 1, 0, -2])))
    return cases


# (sub-domain, i, j) of the columns that hold them: corners, edges and interior cells of different tiles
SPOTS = [(0, 0, 0), (2, 5, 7), (5, 11, 11), (3, 11, 0), (1, 0, 11), (4, 0, 6), (2, 5, 0), (1, 6, 6)]


@pytest.mark.parametrize("nz", [3, 4])
def test_hand_computed_columns(real, nz):  # noqa: F811
    backend, dtype = real
    npd = NP_OF[dtype]
    part, grids, sf = _factory(backend, 12, (1, 1), nz, dtype)
    qf = sf.quantity_factory
    cells = {f: [np.full((12, 12, nz), CLEAN[f], dtype=npd) for _ in grids] for f in FIELDS}
    want = {f: [a.copy() for a in cells[f]] for f in FIELDS}
    cases = _hand_cases(nz)
    assert len(cases) <= len(SPOTS)
    for (r, i, j), (inc, exp) in zip(SPOTS, cases):
        for f, col in inc.items():
            cells[f][r][i, j] = col
            want[f][r][i, j] = col
        for f, col in exp.items():
            want[f][r][i, j] = col(npd) if callable(col) else col
    q, host = _upload(qf, cells, npd)
    _apply(sf, qf, grids, q)
    for f in FIELDS:
        for r in range(len(grids)):
            got, exp = q[f].numpy(r), _padded(want[f][r], 1000.0 if f == "dp" else SENTINEL, npd)
            assert np.array_equal(_bits(got), _bits(exp)), (f, r, np.argwhere(got != exp)[:5], got[got != exp][:5], exp[got != exp][:5])
    # the heating really moved pt in the two columns that take it
    (r, i, j) = SPOTS[1]
    assert q["pt"].numpy(r)[NH + i, NH + j, 0] != 280.0


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. / 3. random columns: bitwise parity with the restatement, the properties of the result
# ---------------------------------------------------------------------------------------------------------------------------------
def _random_cells(n, n_sub, nz, npd, seed=11):
    """Species uniform in [0, 1e-3] (vapour [0, 1e-2]), a cell negative (x -0.3) with probability 0.3 (vapour 0.15), pt in 200 - 300 K,
    dp in 500 - 1500 Pa: (n * n, nz) per sub-domain and field."""
    rng = np.random.default_rng(seed + nz)
    out = {f: [] for f in FIELDS}
    for _ in range(n_sub):
        for f in SPECIES:
            hi, p = (1.0e-2, 0.15) if f == "qv" else (1.0e-3, 0.3)
            a = rng.uniform(0.0, hi, (n * n, nz))
            a = np.where(rng.random((n * n, nz)) < p, a * -0.3, a)
            out[f].append(a.astype(npd))
        out["pt"].append(rng.uniform(200.0, 300.0, (n * n, nz)).astype(npd))
        out["dp"].append(rng.uniform(500.0, 1500.0, (n * n, nz)).astype(npd))
    return out


def _run(backend, dtype, nx_tile, layout, nz, cols, positional=True):
    """The operator on columns `cols` ({field: [(n * n, nz) per sub-domain]}): ({field: [storage arrays after]}, {field: [before]}, n, n_sub)"""
    npd = NP_OF[dtype]
    part, grids, sf = _factory(backend, nx_tile, layout, nz, dtype)
    qf = sf.quantity_factory
    n = part.nx
    q, host = _upload(qf, {f: [a.reshape(n, n, nz) for a in cols[f]] for f in FIELDS}, npd)
    _apply(sf, qf, grids, q, positional)
    return {f: [q[f].numpy(r).copy() for r in range(len(grids))] for f in FIELDS}, host, n, len(grids)


SHAPES = [(12, (1, 1), 3), (12, (1, 1), 4), (12, (1, 1), 5), (12, (1, 1), 8), (24, (2, 2), 7)]
SHAPE_IDS = [f"c{s[0]}_{s[1][0]}x{s[1][1]}_l{s[2]}" for s in SHAPES]


@pytest.mark.parametrize("nx_tile, layout, nz", SHAPES, ids=SHAPE_IDS)
def test_random_columns_match_the_restatement_bitwise(real, nx_tile, layout, nz):  # noqa: F811
    backend, dtype = real
    npd = NP_OF[dtype]
    n_sub = 6 * layout[0] * layout[1]
    cols = _random_cells(nx_tile // layout[0], n_sub, nz, npd)
    got, host, n, n_sub = _run(backend, dtype, nx_tile, layout, nz, cols, positional=(nz % 2 == 1))
    cs = (slice(NH, NH + n), slice(NH, NH + n), slice(0, nz))
    taken = {b: 0 for b in nref.BRANCHES}
    for r in range(n_sub):
        want, counts, _ = nref.neg_adj3(*[cols[f][r] for f in FIELDS])
        for b in nref.BRANCHES:
            taken[b] += counts[b]
        assert np.array_equal(_bits(got["dp"][r]), _bits(host["dp"][r])), "delp was written"
        for f in SPECIES + ("pt",):
            assert want[f].dtype == npd
            g = got[f][r][cs].reshape(n * n, nz)
            # the result is the restatement's, bit for bit (NaN-free inputs: value equality + the sign of zero)
            assert np.array_equal(_bits(g), _bits(want[f])), (f, r, np.argwhere(_bits(g) != _bits(want[f]))[:5], g[g != want[f]][:5], want[f][g != want[f]][:5])
            # halo cells and the pad level keep the sentinel
            outside = np.ones(got[f][r].shape, dtype=bool)
            outside[cs] = False
            assert np.array_equal(_bits(got[f][r][outside]), _bits(host[f][r][outside])), (f, r)
    print(f"neg_adj3 {backend} {npd.__name__} C{nx_tile} {layout} L{nz}: branch members {taken}")
    assert all(v > 0 for v in taken.values()), taken


@pytest.mark.parametrize("nx_tile, layout, nz", SHAPES, ids=SHAPE_IDS)
def test_properties_of_the_result(real, nx_tile, layout, nz):  # noqa: F811
    backend, dtype = real
    npd = NP_OF[dtype]
    eps = float(np.finfo(npd).eps)
    n_sub = 6 * layout[0] * layout[1]
    cols = _random_cells(nx_tile // layout[0], n_sub, nz, npd)
    got, host, n, n_sub = _run(backend, dtype, nx_tile, layout, nz, cols)
    cs = (slice(NH, NH + n), slice(NH, NH + n), slice(0, nz))
    worst = 0.0
    for r in range(n_sub):
        g = {f: got[f][r][cs].reshape(n * n, nz) for f in FIELDS}
        _, _, before = nref.neg_adj3(*[cols[f][r] for f in FIELDS])
        for f in SPECIES[1:]:
            assert (g[f] >= 0).all(), (f, r, float(g[f].min()))
        assert (g["qv"][:, : nz - 2] >= 0).all(), (r, float(g["qv"][:, : nz - 2].min()))
        # level km-2 may be negative only by the rounding of a - (a * da) / da in the bottom step
        assert (before >= 0).all()
        assert (g["qv"][:, nz - 2].astype(np.float64) >= -2.0 * eps * before.astype(np.float64)).all(), (r, float(g["qv"][:, nz - 2].min()))
        # the column's total water, accumulated in float64
        dp = cols["dp"][r].astype(np.float64)
        m0 = sum((cols[f][r].astype(np.float64) * dp).sum(axis=1) for f in SPECIES)
        m1 = sum((g[f].astype(np.float64) * dp).sum(axis=1) for f in SPECIES)
        scale = sum((np.abs(cols[f][r].astype(np.float64)) * dp).sum(axis=1) for f in SPECIES)
        rel = np.abs(m1 - m0) / scale
        worst = max(worst, float(rel.max()) / eps)
        assert (np.abs(m1 - m0) <= (nz + 8) * eps * scale).all(), (r, float(rel.max()) / eps)
    print(f"neg_adj3 {backend} {npd.__name__} C{nx_tile} {layout} L{nz}: worst total-water error {worst:.2f} eps (bound {nz + 8})")
    # a state without any negative value comes back bitwise unchanged
    clean = {f: [np.abs(a) for a in cols[f]] for f in FIELDS}
    got, host, n, n_sub = _run(backend, dtype, nx_tile, layout, nz, clean)
    for f in FIELDS:
        for r in range(n_sub):
            assert np.array_equal(_bits(got[f][r]), _bits(host[f][r])), (f, r)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. real data: the C12 L63 restart fixture, qvapor = sphum, qliquid = liq_wat, the other species zero
# ---------------------------------------------------------------------------------------------------------------------------------
def test_restart_fixture_matches_the_restatement_bitwise(real):  # noqa: F811
    backend, dtype = real
    npd = NP_OF[dtype]
    data = np.load(FIXTURE)
    nz = data["T"].shape[1]
    col = lambda key, t: np.transpose(data[key][t], (2, 1, 0)).reshape(144, nz).astype(npd)  # noqa: E731
    zeros = np.zeros((144, nz), dtype=npd)
    cols = dict(qv=[col("sphum", t) for t in range(6)], ql=[col("liq_wat", t) for t in range(6)], qr=[zeros] * 6, qi=[zeros] * 6, qs=[zeros] * 6, qg=[zeros] * 6,
                pt=[col("T", t) for t in range(6)], dp=[col("delp", t) for t in range(6)])
    n_neg = sum(int((a < 0).sum()) for a in cols["ql"])
    if npd is np.float64:
        assert n_neg == int((data["liq_wat"] < 0).sum()) and n_neg > 0
    got, host, n, n_sub = _run(backend, dtype, 12, (1, 1), nz, cols)
    cs = (slice(NH, NH + n), slice(NH, NH + n), slice(0, nz))
    n_ql = 0
    for r in range(6):
        want, counts, _ = nref.neg_adj3(*[cols[f][r] for f in FIELDS])
        n_ql += counts["ql"]
        for f in SPECIES + ("pt",):
            g = got[f][r][cs].reshape(144, nz)
            assert np.array_equal(_bits(g), _bits(want[f])), (f, r)
        assert (got["ql"][r][cs] >= 0).all()
        assert np.array_equal(_bits(got["dp"][r]), _bits(host["dp"][r]))
    assert n_ql == n_neg, (n_ql, n_neg)
    print(f"neg_adj3 {backend} {npd.__name__} restart fixture: {n_neg} of {6 * 144 * nz} liq_wat cells below zero, all paid from the vapour")


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. argument checks through the C ABI and the Python refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def test_argument_checks(backend):
    nz = 4
    part, grids, sf = _factory(backend, 12, (1, 1), nz, torch.float64)
    qf = sf.quantity_factory
    rng = np.random.default_rng(1)
    mk = lambda: qf.from_array([rng.normal(0.0, 1.0e-3, (12 + 2 * NH + 1, 12 + 2 * NH + 1, nz + 1)) for _ in grids], DIMS)  # noqa: E731
    q = {f: mk() for f in FIELDS}
    q["dp"].storage.abs_().add_(1.0)
    q["pt"].storage.add_(280.0)
    flat = qf.zeros(("x", "y"))
    short = _lib.fv3_field()
    C.memmove(C.byref(short), C.byref(q["qv"].field), C.sizeof(_lib.fv3_field))
    short.shape[2] -= 1
    before = {f: q[f].storage.clone() for f in FIELDS}
    lib, ctx, s = sf.lib, sf.ctx, sf.stream_handle
    latent = _lib.fv3_latent(pc.HLV, pc.HLF, pc.T_ICE)

    def ref(v):
        return None if v is None else (C.pointer(v) if isinstance(v, _lib.fv3_field) else C.pointer(v.field))

    def call(no_ctx=False, no_water=False, no_latent=False, **swap):
        f = {k: swap.get(k, q[k]) for k in FIELDS}
        water = None if no_water else C.byref(_lib.fv3_water(*[ref(f[k]) for k in SPECIES], pc.CV_VAP, pc.C_LIQ, pc.C_ICE))
        return lib.fv3_neg_adj3(None if no_ctx else ctx, water, None if no_latent else C.byref(latent), ref(f["pt"]), ref(f["dp"]), s)

    ARG = -1
    assert call(no_ctx=True) == ARG
    cases = [
        ("null water", dict(no_water=True), b"neg_adj3: the fv3_water is null"),
        ("null latent", dict(no_latent=True), b"neg_adj3: the fv3_latent is null"),
        ("null pt", dict(pt=None), b"'pt': null"),
        ("null delp", dict(dp=None), b"'delp': null"),
        ("2-D pt", dict(pt=flat), b"'pt': vertical shape"),
        ("2-D delp", dict(dp=flat), b"'delp': vertical shape"),
        ("mis-shaped qrain", dict(qr=short), b"'qrain': vertical shape"),
        ("2-D qice", dict(qi=flat), b"'qice': vertical shape"),
        ("qliquid and qrain the same", dict(qr=q["ql"]), b"qliquid and qrain are the same field"),
        ("qvapor and qgraupel the same", dict(qg=q["qv"]), b"qvapor and qgraupel are the same field"),
        ("pt is qsnow", dict(pt=q["qs"]), b"pt is the qsnow field"),
        ("delp is qvapor", dict(dp=q["qv"]), b"delp is the qvapor field"),
        ("pt is delp", dict(pt=q["dp"]), b"pt and delp are the same field"),
    ] + [(f"null {ROLE[k]}", {k: None}, f"'{ROLE[k]}': null".encode()) for k in SPECIES]
    for what, kw, word in cases:
        assert call(qv=flat) == ARG and b"'qvapor': vertical shape" in lib.fv3_last_error(ctx)  # (another message in between: the one below is this case's own)
        st = call(**kw)
        msg = lib.fv3_last_error(ctx)
        assert st == ARG, (what, st)
        assert msg and word in msg, (what, msg)
        _sync(sf)
        for f in FIELDS:
            assert torch.equal(q[f].storage, before[f]), (what, f)
    # the Python refusals
    op = AdjustNegativeTracerMixingRatio(sf, qf, grids)
    with pytest.raises(NotImplementedError, match="qcld must be None") as e:
        op(q["qv"], q["ql"], q["qr"], q["qs"], q["qi"], q["qg"], qf.zeros(DIMS), q["pt"], q["dp"])
    assert str(e.value).count(". ") == 0
    with pytest.raises(NotImplementedError, match="non-hydrostatic") as e:
        AdjustNegativeTracerMixingRatio(sf, qf, grids, hydrostatic=True)
    assert str(e.value).count(". ") == 0
    with pytest.raises(_lib.Fv3Error, match="'qrain': null"):
        op(pt=q["pt"], delp=q["dp"], water=WaterSpecies(q["qv"], qliquid=q["ql"], qice=q["qi"], qsnow=q["qs"], qgraupel=q["qg"]))
    with pytest.raises(_lib.Fv3Error, match="pt is the qsnow field"):
        op(q["qv"], q["ql"], q["qr"], q["qs"], q["qi"], q["qg"], None, q["qs"], q["dp"])
    _sync(sf)
    for f in FIELDS:
        assert torch.equal(q[f].storage, before[f]), f
    # ... and a call that passes changes what the restatement changes (delz and peln are accepted and not read)
    op(q["qv"], q["ql"], q["qr"], q["qs"], q["qi"], q["qg"], None, q["pt"], q["dp"], q["pt"], None)
    _sync(sf)
    assert not torch.equal(q["qi"].storage, before["qi"]) and torch.equal(q["dp"].storage, before["dp"])


def test_dynamical_core_needs_all_six_roles(backend):
    from pace_amd._testing import harness_for
    from pace_amd.fv_dynamics import DynamicalCore

    h = harness_for(backend)(12, nz=5, layout=(1, 1), k_split=1, n_split=1, n_tracers=6, remap=True, temperature=True, moist=True)
    roles = {n: n for n in h.tracers}
    mk = lambda **kw: DynamicalCore(h.layout, h.grids, h.sf, None, None, h.cfg, 225.0, h.state.phis, h.state, tracers=h.tracers, cubed_to_latlon=False, **kw)  # noqa: E731
    with pytest.raises(ValueError, match="all six roles.*qrain"):
        mk(water_species={k: v for k, v in roles.items() if k != "qrain"}, adjust_negative_water=True)
    with pytest.raises(ValueError, match="all six roles"):
        mk(adjust_negative_water=True)
    assert mk(water_species=roles, adjust_negative_water=True).adjust_negative_water is not None
    assert mk(water_species=roles).adjust_negative_water is None and h.dycore.adjust_negative_water is None
    with pytest.raises(ValueError, match="neg_adj=True needs moist=True"):
        harness_for(backend)(12, nz=5, layout=(1, 1), n_tracers=6, remap=True, temperature=True, neg_adj=True)
    h.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. register budget (read from the code-object metadata of the built library: no GPU needed)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [64, 32])
def test_neg_adj_kernel_stays_inside_the_register_budget(precision):
    """A memory-bound column kernel wants four waves per SIMD: at most 128 architectural VGPRs, nothing spilled, no scratch."""
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
    hits = {n: k for n, k in ks.items() if "neg_adj_columns" in n}
    assert len(hits) == 1, sorted(hits)
    for n, k in hits.items():
        assert k["vgpr"] - k["agpr"] <= 128 and k["spill"] == 0 and k["scratch"] == 0 and k["lds"] == 0, (n[:100], k)
