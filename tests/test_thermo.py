"""The thermodynamic bookends of step_dynamics (pace_amd/csrc/fv3_thermo.hip) through TemperatureToPotential /
PotentialToTemperature and the C ABI: parity with the numpy restatement (tests/thermo_reference.py) in fp64 and fp32, both entries,
both recompute_pkz forms, with and without qvapor; round trips; the real restart fixture against pace_amd.init.restart_state;
qvapor = NULL against a field of zeros; what must stay untouched; the argument checks; the register budget of the kernels.  Every
operator case runs on the host emulation (CPU suite) and on the HIP library (-m gpu).

Errors are max-normalised (max |got - want| / max |want|), the convention of tests/helpers.py: assert_close.

fp64 bounds: 1e-12 for pt and pkz, what tests/test_remap.py gives those two fields.  fp32: the device result and the float32
restatement are both compared with the float64 restatement evaluated on the same fp32 inputs; the device error may be at most 4 x
the restatement's own (E_ref): device and numpy exp / log are different implementations, each within a few ulp
(tests/test_device_math.py), and two such pairs are chained.  omga and ps are two roundings and a copy: bitwise."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

import thermo_reference as ref
from pace_amd import lib as _lib
from pace_amd._testing import stencil_factory_for
from pace_amd.config import AcousticDynamicsConfig
from pace_amd.constants import get_constants
from pace_amd.grid import make_grid
from pace_amd.stencils import PotentialToTemperature, TemperatureToPotential
from pace_amd.topology import CubedSpherePartitioner

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NH = 3
SENTINEL = -777.25
DIMS = ("x", "y", "z")
IFACE = ("x", "y", "z_interface")
NP_OF = {torch.float64: np.float64, torch.float32: np.float32}
FIXTURE = os.path.join(ROOT, "tests", "golden", "c12_restart_6tiles.npz")
IN3 = ("delp", "delz", "q_con", "cappa", "qv", "w")


@pytest.fixture(params=[torch.float64, torch.float32], ids=["fp64", "fp32"])
def real(request, backend):
    """(backend, dtype): the fp32 cases need the f32 libraries (host emulation in the CPU suite, the HIP build under -m gpu)."""
    from pace_amd import build

    if request.param == torch.float32:
        if backend == "hostemu":
            build.build(32, hostemu=True, verbose=False)
        else:
            if not os.path.exists(build.lib_path(32)):
                build.build(32)
            _lib.load(32)
    return backend, request.param


@functools.lru_cache(maxsize=None)
def _grids(nx_tile, layout, nz, with_fixture_levels=False):
    part = CubedSpherePartitioner(nx_tile, layout)
    kw = {}
    if with_fixture_levels:
        d = np.load(FIXTURE)
        kw = dict(ak=d["ak"], bk=d["bk"])
    return part, [make_grid(part, r, nz=nz, **kw) for r in range(part.total_ranks)]


def _factory(backend, nx_tile, layout, nz, dtype, with_fixture_levels=False):
    part, grids = _grids(nx_tile, layout, nz, with_fixture_levels)
    # (nord = 0: the fp32 context refuses the C12 del-6 damping tables, which overflow the float range; these entries read none)
    cfg = AcousticDynamicsConfig(npx=nx_tile + 1, npy=nx_tile + 1, npz=nz, layout=layout, nord=0)
    return part, grids, stencil_factory_for(backend)(grids, cfg, get_constants(), dtype=dtype)


def _sync(sf):
    if not sf.hostemu:
        torch.cuda.synchronize()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _err(got, want):
    return float(np.max(np.abs(got.astype(np.float64) - want.astype(np.float64))) / np.max(np.abs(want.astype(np.float64))))


@functools.lru_cache(maxsize=None)
def _random_cells(n, n_sub, nz, npd_name):
    """Per sub-domain, the compute cells (n, n, nz) of physically ranged fields -- the value ranges of the restart fixture
    (tests/golden/c12_restart_6tiles.npz): T 182 .. 308 K, specific humidity up to 0.018, q_con up to 6e-4, delp 73 .. 3700 Pa, the
    full pressure between 50 Pa and 1020 hPa (which makes delz = rrg delp T_v / p negative), cappa = kappa (1 - 0.2 q_con), w of a
    few cm/s; pe (n, n, nz + 1) = ptop + the running sum of delp.  Computed once per shape and dtype, shared, never modified."""
    npd = np.dtype(npd_name).type
    c = get_constants()
    rng = np.random.default_rng(20261018 + n + 7 * nz)
    out = []
    for _ in range(n_sub):
        shp = (n, n, nz)
        T = rng.uniform(182.0, 308.0, shp)
        qv = rng.uniform(1.0e-7, 0.018, shp) * (rng.random(shp) < 0.8)  # (a fifth exact zeros)
        q_con = rng.uniform(0.0, 6.0e-4, shp) * (rng.random(shp) < 0.5)
        delp = rng.uniform(73.0, 3700.0, shp)
        p = np.exp(rng.uniform(np.log(50.0), np.log(1.02e5), shp))
        delz = c.RDG * delp * T * (1.0 + c.ZVIR * qv) * (1.0 - q_con) / p
        cappa = c.KAPPA * (1.0 - 0.2 * q_con)
        w = rng.normal(0.0, 0.05, shp)
        pe = np.concatenate([np.full((n, n, 1), 300.0), 300.0 + np.cumsum(delp, axis=2)], axis=2)
        d = dict(T=T, qv=qv, q_con=q_con, delp=delp, delz=delz, cappa=cappa, w=w, pe=pe)
        d = {k: np.ascontiguousarray(v.astype(npd)) for k, v in d.items()}
        for v in d.values():
            v.setflags(write=False)
        assert (d["delz"] < 0).all()
        out.append(d)
    return out


def _padded(cells, fill, npd, iface=False):
    """compute cells (n, n, nk) -> the (n + 2 NH + 1, n + 2 NH + 1, nz + 1) storage array, `fill` everywhere else (an interface
    field has no pad level: nk = nz + 1)."""
    n, _, nk = cells.shape
    a = np.full((n + 2 * NH + 1, n + 2 * NH + 1, nk + (0 if iface else 1)), fill, dtype=npd)
    a[NH : NH + n, NH : NH + n, :nk] = cells
    return a


class Fields:
    """Device quantities of one case: the inputs from the shared cells (the sentinel outside the compute box and on the pad level),
    pt / pkz from the given cells, omga and ps filled with the sentinel."""

    def __init__(self, sf, cells, pt, pkz, npd):
        qf = sf.quantity_factory
        self.sf, self.npd, self.n, self.nz = sf, npd, pt[0].shape[0], pt[0].shape[2]
        self.host = {k: [_padded(c[k], SENTINEL, npd) for c in cells] for k in IN3}
        self.host["pe"] = [_padded(c["pe"], SENTINEL, npd, iface=True) for c in cells]
        self.host["pt"] = [_padded(a, SENTINEL, npd) for a in pt]
        self.host["pkz"] = [_padded(a, SENTINEL, npd) for a in pkz]
        self.host["omga"] = [np.full_like(a, SENTINEL) for a in self.host["pt"]]
        self.host["ps"] = [np.full(a.shape[:2], SENTINEL, dtype=npd) for a in self.host["pt"]]
        self.q = {k: qf.from_array(v, ("x", "y") if k == "ps" else (IFACE if k == "pe" else DIMS)) for k, v in self.host.items()}

    def cells(self, name, r):
        n, nz = self.n, self.nz
        a = self.q[name].numpy(r)
        return a[NH : NH + n, NH : NH + n] if name == "ps" else a[NH : NH + n, NH : NH + n, :nz]

    def check_untouched(self, written):
        """The inputs are unchanged everywhere; the written fields keep the sentinel outside the compute box and on the pad level;
        a possible output that was not given to the call is unchanged everywhere.  Bitwise."""
        _sync(self.sf)
        n, nz = self.n, self.nz
        for name, host in self.host.items():
            for r, h in enumerate(host):
                got = self.q[name].numpy(r)
                if name not in written:
                    assert np.array_equal(_bits(got), _bits(h)), f"{name} (not an output of this call) was written"
                    continue
                outside = np.ones(h.shape, dtype=bool)
                if name == "ps":
                    outside[NH : NH + n, NH : NH + n] = False
                else:
                    outside[NH : NH + n, NH : NH + n, :nz] = False
                assert np.array_equal(_bits(got[outside]), _bits(h[outside])), f"{name}: a halo cell or the pad level was written"
                host[r] = got  # (what a later call on these fields must leave alone)


def _fwd(F, qv):
    q = F.q
    TemperatureToPotential(F.sf)(q["pt"], q["pkz"], q["delp"], q["delz"], q["q_con"], q["cappa"], q["qv"] if qv else None)
    F.check_untouched({"pt", "pkz"})


def _bwd(F, qv, recompute, omga=True, ps=True):
    q = F.q
    PotentialToTemperature(F.sf)(q["pt"], q["pkz"], q["delp"], q["delz"], q["q_con"], q["cappa"], q["w"], q["pe"], qvapor=q["qv"] if qv else None,
                                 omga=q["omga"] if omga else None, ps=q["ps"] if ps else None, recompute_pkz=recompute)
    F.check_untouched({"pt"} | ({"pkz"} if recompute else set()) | ({"omga"} if omga else set()) | ({"ps"} if ps else set()))


def _as64(c):
    return {k: v.astype(np.float64) for k, v in c.items()}


def _bound(name, got, want_own, want64, npd, worst):
    """fp64: the restatement in the array's dtype within 1e-12.  fp32: at most 4 x the restatement's own error against float64."""
    if npd == np.float64:
        e = _err(got, want_own)
        worst[name] = max(worst.get(name, (0.0, 0.0))[0], e), 0.0
        assert e <= 1.0e-12, (name, e)
    else:
        e, e_ref = _err(got, want64), _err(want_own, want64)
        w = worst.get(name, (0.0, 0.0))
        worst[name] = max(w[0], e), max(w[1], e_ref)
        assert e <= 4.0 * e_ref, (name, e, e_ref)


SHAPES = [(12, (1, 1), 3), (12, (1, 1), 4), (12, (1, 1), 5), (12, (1, 1), 7), (24, (2, 2), 4), (96, (1, 1), 3)]
SHAPE_IDS = [f"c{s[0]}_{s[1][0]}x{s[1][1]}_l{s[2]}" for s in SHAPES]


# ---------------------------------------------------------------------------------------------------------------------------------
# parity with the restatement: both entries, both recompute_pkz forms, with and without qvapor, fp64 and fp32
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qv", [True, False], ids=["qvapor", "dry"])
@pytest.mark.parametrize("nx_tile, layout, nz", SHAPES, ids=SHAPE_IDS)
def test_both_entries_match_the_restatement(real, nx_tile, layout, nz, qv):
    backend, dtype = real
    npd = NP_OF[dtype]
    part, grids, sf = _factory(backend, nx_tile, layout, nz, dtype)
    n, n_sub = part.nx, len(grids)
    cells = _random_cells(n, n_sub, nz, npd.__name__)
    worst = {}
    # the restatement in the array's dtype and in float64 on the same inputs
    own, r64 = [], []
    for c in cells:
        o, c64 = {}, _as64(c)
        d = {}
        for tag, cc, out in (("own", c, o), ("r64", c64, d)):
            out["pt"], out["pkz"] = ref.pt_from_temperature(cc["T"], cc["delp"], cc["delz"], cc["q_con"], cc["cappa"], cc["qv"] if qv else None)
        # the closing entry is fed the array-dtype loop form in both evaluations: the same inputs for the device and both restatements
        for cc, out in ((c, o), (c64, d)):
            pt_in, pkz_in = o["pt"].astype(cc["T"].dtype), o["pkz"].astype(cc["T"].dtype)
            out["T0"], _, out["omga"] = ref.temperature_from_pt(pt_in, pkz_in, cc["delp"], cc["delz"], cc["q_con"], cc["cappa"], cc["w"], cc["qv"] if qv else None, False)
            out["T1"], out["pkz1"], _ = ref.temperature_from_pt(pt_in, pkz_in, cc["delp"], cc["delz"], cc["q_con"], cc["cappa"], cc["w"], cc["qv"] if qv else None, True)
        assert all(v.dtype == npd for v in o.values())
        own.append(o)
        r64.append(d)
    # ---- fv3_pt_from_temperature
    F = Fields(sf, cells, [c["T"] for c in cells], [np.full_like(c["T"], SENTINEL) for c in cells], npd)
    _fwd(F, qv)
    for r in range(n_sub):
        _bound("fwd pt", F.cells("pt", r), own[r]["pt"], r64[r]["pt"], npd, worst)
        _bound("fwd pkz", F.cells("pkz", r), own[r]["pkz"], r64[r]["pkz"], npd, worst)
    # ---- fv3_temperature_from_pt, recompute_pkz = 0: tv = pt * pkz
    F = Fields(sf, cells, [o["pt"] for o in own], [o["pkz"] for o in own], npd)
    _bwd(F, qv, False)
    for r in range(n_sub):
        _bound("bwd T (pkz given)", F.cells("pt", r), own[r]["T0"], r64[r]["T0"], npd, worst)
        assert np.array_equal(_bits(F.cells("omga", r)), _bits(own[r]["omga"]))
        assert np.array_equal(_bits(F.cells("ps", r)), _bits(cells[r]["pe"][:, :, nz]))
    # ---- recompute_pkz = 1: pkz comes in as the sentinel and is rebuilt
    F = Fields(sf, cells, [o["pt"] for o in own], [np.full_like(o["pkz"], SENTINEL) for o in own], npd)
    _bwd(F, qv, True)
    for r in range(n_sub):
        _bound("bwd T (pkz rebuilt)", F.cells("pt", r), own[r]["T1"], r64[r]["T1"], npd, worst)
        _bound("bwd pkz (rebuilt)", F.cells("pkz", r), own[r]["pkz1"], r64[r]["pkz1"], npd, worst)
        assert np.array_equal(_bits(F.cells("omga", r)), _bits(own[r]["omga"]))
        assert np.array_equal(_bits(F.cells("ps", r)), _bits(cells[r]["pe"][:, :, nz]))
    print(f"thermo {backend} {npd.__name__} C{nx_tile} {layout} L{nz} qv={qv}: (error, E_ref) " + ", ".join(f"{k} ({v[0]:.2e}, {v[1]:.2e})" for k, v in worst.items()))


def test_the_closing_entry_without_omga_and_ps(backend):
    """omga = NULL and ps = NULL: neither is written, pt is what the full call gives."""
    nz = 5
    part, grids, sf = _factory(backend, 12, (1, 1), nz, torch.float64)
    cells = _random_cells(12, len(grids), nz, "float64")
    loop = [ref.pt_from_temperature(c["T"], c["delp"], c["delz"], c["q_con"], c["cappa"], c["qv"]) for c in cells]
    for recompute in (False, True):
        A = Fields(sf, cells, [l[0] for l in loop], [l[1] for l in loop], np.float64)
        B = Fields(sf, cells, [l[0] for l in loop], [l[1] for l in loop], np.float64)
        _bwd(A, True, recompute)
        _bwd(B, True, recompute, omga=False, ps=False)
        for r in range(len(grids)):
            assert np.array_equal(_bits(A.q["pt"].numpy(r)), _bits(B.q["pt"].numpy(r)))
            assert np.array_equal(_bits(A.q["pkz"].numpy(r)), _bits(B.q["pkz"].numpy(r)))


# ---------------------------------------------------------------------------------------------------------------------------------
# round trip: PotentialToTemperature(TemperatureToPotential(T)) against T
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("recompute", [False, True], ids=["pkz_given", "pkz_rebuilt"])
@pytest.mark.parametrize("nx_tile, layout, nz", [SHAPES[2], SHAPES[4]], ids=[SHAPE_IDS[2], SHAPE_IDS[4]])
def test_round_trip_returns_the_temperature(real, nx_tile, layout, nz, recompute):
    backend, dtype = real
    npd = NP_OF[dtype]
    part, grids, sf = _factory(backend, nx_tile, layout, nz, dtype)
    cells = _random_cells(part.nx, len(grids), nz, npd.__name__)
    F = Fields(sf, cells, [c["T"] for c in cells], [np.full_like(c["T"], SENTINEL) for c in cells], npd)
    _fwd(F, True)
    _bwd(F, True, recompute)
    e = max(_err(F.cells("pt", r), c["T"]) for r, c in enumerate(cells))
    # the restatement's own round trip in the same dtype
    e_ref = 0.0
    for c in cells:
        pt, pkz = ref.pt_from_temperature(c["T"], c["delp"], c["delz"], c["q_con"], c["cappa"], c["qv"])
        T, _, _ = ref.temperature_from_pt(pt, pkz, c["delp"], c["delz"], c["q_con"], c["cappa"], c["w"], c["qv"], recompute)
        e_ref = max(e_ref, _err(T, c["T"]))
    print(f"thermo round trip {backend} {npd.__name__} C{nx_tile} L{nz} recompute={recompute}: error {e:.2e}, the restatement's own {e_ref:.2e}")
    if npd == np.float64:
        assert e <= 1.0e-12, e
    else:
        assert e <= 4.0 * e_ref, (e, e_ref)


# ---------------------------------------------------------------------------------------------------------------------------------
# real data: the restart fixture, against the host conversion of pace_amd.init.restart_state
# ---------------------------------------------------------------------------------------------------------------------------------
def test_real_restart_data_against_restart_state(backend):
    from pace_amd.init import restart_state

    data = np.load(FIXTURE)
    nz = data["T"].shape[1]
    part, grids, sf = _factory(backend, 12, (1, 1), nz, torch.float64, with_fixture_levels=True)
    c = get_constants()
    cells, want = [], []
    for r, g in enumerate(grids):
        tile = part.tile_index(r)
        f = lambda k: np.ascontiguousarray(np.transpose(np.asarray(data[k][tile], dtype=np.float64), (2, 1, 0)))  # noqa: E731
        q_con = f("liq_wat")
        pe = np.concatenate([np.full((12, 12, 1), float(g.ak[0])), float(g.ak[0]) + np.cumsum(f("delp"), axis=2)], axis=2)
        cells.append(dict(T=f("T"), qv=f("sphum"), q_con=q_con, cappa=c.KAPPA * (1.0 - 0.2 * q_con), delp=f("delp"), delz=f("DZ"), w=f("W"), pe=pe))
        s = restart_state(g, data, tile, part.origin(r), c)
        want.append({k: s[k][NH : NH + 12, NH : NH + 12, :nz] for k in ("pt", "pkz")})
    # T -> the loop's form: what restart_state computes on the host
    F = Fields(sf, cells, [c_["T"] for c_ in cells], [np.full_like(c_["T"], SENTINEL) for c_ in cells], np.float64)
    _fwd(F, True)
    e = {k: max(_err(F.cells(k, r), want[r][k]) for r in range(len(grids))) for k in ("pt", "pkz")}
    # restart_state's output + the sphum field -> the fixture's T, in both forms
    et = {}
    for recompute in (False, True):
        F = Fields(sf, cells, [w_["pt"] for w_ in want], [w_["pkz"] for w_ in want], np.float64)
        _bwd(F, True, recompute)
        et[recompute] = max(_err(F.cells("pt", r), cells[r]["T"]) for r in range(len(grids)))
        assert float(min(F.cells("pt", r).min() for r in range(len(grids)))) > 100.0  # a temperature again (the loop's form is 9 .. 76 here)
    print(f"thermo real data {backend}: pt {e['pt']:.2e}, pkz {e['pkz']:.2e} against restart_state; T back {et[False]:.2e} (pkz given), {et[True]:.2e} (pkz rebuilt)")
    assert max(w_["pt"].max() for w_ in want) < 100.0
    assert e["pt"] <= 1.0e-12 and e["pkz"] <= 1.0e-12, e
    assert et[False] <= 1.0e-12 and et[True] <= 1.0e-12, et


# ---------------------------------------------------------------------------------------------------------------------------------
# qvapor = NULL is a qvapor field of zeros, bitwise
# ---------------------------------------------------------------------------------------------------------------------------------
def test_null_qvapor_equals_a_field_of_zeros_bitwise(real):
    backend, dtype = real
    npd = NP_OF[dtype]
    nz = 5
    part, grids, sf = _factory(backend, 12, (1, 1), nz, dtype)
    cells = _random_cells(12, len(grids), nz, npd.__name__)
    zero = [dict(c, qv=np.zeros_like(c["qv"])) for c in cells]
    mk = lambda cs: Fields(sf, cs, [c["T"] for c in cs], [np.full_like(c["T"], SENTINEL) for c in cs], npd)  # noqa: E731
    A, B = mk(zero), mk(cells)
    _fwd(A, True)
    _fwd(B, False)
    loop = [(A.cells("pt", r).copy(), A.cells("pkz", r).copy()) for r in range(len(grids))]
    for r in range(len(grids)):
        for k in ("pt", "pkz"):
            assert np.array_equal(_bits(A.q[k].numpy(r)), _bits(B.q[k].numpy(r))), k
    for recompute in (False, True):
        A = Fields(sf, zero, [l[0] for l in loop], [l[1] for l in loop], npd)
        B = Fields(sf, cells, [l[0] for l in loop], [l[1] for l in loop], npd)
        _bwd(A, True, recompute)
        _bwd(B, False, recompute)
        for r in range(len(grids)):
            for k in ("pt", "pkz", "omga", "ps"):
                assert np.array_equal(_bits(A.q[k].numpy(r)), _bits(B.q[k].numpy(r))), (k, recompute)


# ---------------------------------------------------------------------------------------------------------------------------------
# argument checks through the C ABI
# ---------------------------------------------------------------------------------------------------------------------------------
def test_argument_checks(backend):
    nz = 4
    part, grids, sf = _factory(backend, 12, (1, 1), nz, torch.float64)
    qf = sf.quantity_factory
    cells = _random_cells(12, len(grids), nz, "float64")
    F = Fields(sf, cells, [c["T"] for c in cells], [c["T"] * 0.0 + 3.0 for c in cells], np.float64)
    q = F.q
    flat = qf.zeros(("x", "y"))
    ps_on_pe = _lib.fv3_field()
    C.memmove(C.byref(ps_on_pe), C.byref(flat.field), C.sizeof(_lib.fv3_field))
    ps_on_pe.ptr = q["pe"].field.ptr  # a field of the 2-D layout at pe's address
    before = {k: v.storage.clone() for k, v in q.items()}
    lib, ctx, s = sf.lib, sf.ctx, sf.stream_handle
    fwd_names = ("pt", "pkz", "delp", "delz", "q_con", "cappa", "qv")
    bwd_names = ("pt", "pkz", "delp", "delz", "q_con", "cappa", "qv", "w", "omga", "pe", "ps")

    def call(entry, ctx_=ctx, recompute=0, **swap):
        names = fwd_names if entry == "fwd" else bwd_names
        args = []
        for nme in names:
            v = swap.get(nme, q[nme])
            args.append(None if v is None else (C.byref(v) if isinstance(v, _lib.fv3_field) else v.fref))
        if entry == "fwd":
            return lib.fv3_pt_from_temperature(ctx_, *args, s)
        return lib.fv3_temperature_from_pt(ctx_, *args, recompute, s)

    ARG = -1
    cases = [
        ("fwd: 2-D pt", "fwd", dict(pt=flat), b"'pt_': vertical shape"),
        ("fwd: 2-D cappa", "fwd", dict(cappa=flat), b"'cappa_': vertical shape"),
        ("fwd: null delz", "fwd", dict(delz=None), b"'delz_': null"),
        ("fwd: 2-D qvapor", "fwd", dict(qv=flat), b"'qvapor_': vertical shape"),
        ("fwd: pt is pkz", "fwd", dict(pkz=q["pt"]), b"pt and pkz are the same field"),
        ("fwd: pt is delp", "fwd", dict(pt=q["delp"]), b"pt is the delp field"),
        ("fwd: pkz is cappa", "fwd", dict(pkz=q["cappa"]), b"pkz is the cappa field"),
        ("fwd: pt is qvapor", "fwd", dict(qv=q["pt"]), b"pt is the qvapor field"),
        ("bwd: 2-D pkz", "bwd", dict(pkz=flat), b"'pkz_': vertical shape"),
        ("bwd: 3-D ps", "bwd", dict(ps=q["omga"]), b"'ps_': expected a 2-D field"),
        ("bwd: 2-D omga", "bwd", dict(omga=flat), b"'omga_': vertical shape"),
        ("bwd: 2-D pe", "bwd", dict(pe=flat), b"'pe_': vertical shape"),
        ("bwd: pt is pkz", "bwd", dict(pkz=q["pt"]), b"pt and pkz are the same field"),
        ("bwd: omga is pt", "bwd", dict(omga=q["pt"]), b"pt and omga are the same field"),
        ("bwd: omga is pkz", "bwd", dict(omga=q["pkz"]), b"pkz and omga are the same field"),
        ("bwd: omga is w", "bwd", dict(omga=q["w"]), b"omga is the w field"),
        ("bwd: omga is delp", "bwd", dict(omga=q["delp"]), b"is the delp field"),
        ("bwd: pt is delz", "bwd", dict(pt=q["delz"]), b"is the delz field"),
        ("bwd: pkz is q_con", "bwd", dict(pkz=q["q_con"]), b"is the q_con field"),
        ("bwd: pt is pe", "bwd", dict(pt=q["pe"]), b"is the pe field"),
        ("bwd: pkz is qvapor", "bwd", dict(qv=q["pkz"]), b"is the qvapor field"),
        ("bwd: ps at pe's address", "bwd", dict(ps=ps_on_pe), b"ps is the pe field"),
        ("bwd: recompute_pkz = 2", "bwd2", {}, b"recompute_pkz = 2"),
    ]
    for what, entry, swap, word in cases:
        assert call("fwd", q_con=None) == ARG and b"'q_con_': null" in lib.fv3_last_error(ctx)  # (another message in between: the one below is this case's own)
        st = call("bwd", recompute=2) if entry == "bwd2" else call(entry, **swap)
        msg = lib.fv3_last_error(ctx)
        assert st == ARG, (what, st)
        assert msg and word in msg, (what, msg)
        _sync(sf)
        for k, b in before.items():
            assert torch.equal(q[k].storage, b), (what, k)
    # a null context: a status and a message, without a context to hold it
    assert call("fwd", ctx_=None) == ARG and b"context is null" in lib.fv3_last_error(None)
    assert call("bwd", ctx_=None) == ARG and b"context is null" in lib.fv3_last_error(None)
    # ... and the operators raise what the entries report
    with pytest.raises(_lib.Fv3Error, match="same field"):
        TemperatureToPotential(sf)(q["pt"], q["pt"], q["delp"], q["delz"], q["q_con"], q["cappa"])
    with pytest.raises(_lib.Fv3Error, match="is the w field"):
        PotentialToTemperature(sf)(q["pt"], q["pkz"], q["delp"], q["delz"], q["q_con"], q["cappa"], q["w"], q["pe"], omga=q["w"])
    _sync(sf)
    for k, b in before.items():
        assert torch.equal(q[k].storage, b), k


# ---------------------------------------------------------------------------------------------------------------------------------
# register budget (read from the code-object metadata of the built library: no GPU needed)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [64, 32])
def test_thermo_kernels_stay_inside_the_register_budget(precision):
    """Streaming cell kernels want at least four waves per SIMD: every instantiation (qvapor present / absent in the preamble; x
    recompute_pkz x omga present / absent in the closing entry; the ps row copy) has at most 128 architectural VGPRs, nothing
    spilled, no scratch, no LDS."""
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
    fwd = {n: k for n, k in ks.items() if "thermo_fwd" in n}
    bwd = {n: k for n, k in ks.items() if "thermo_bwd" in n}
    ps = {n: k for n, k in ks.items() if "fv3_temperature_from_pt" in n}
    assert len(fwd) == 2 and len(bwd) == 8 and len(ps) == 1, (sorted(fwd), sorted(bwd), sorted(ps))
    for a in "01":
        assert sum(f"thermo_fwdILb{a}E" in n for n in fwd) == 1
        for b in "01":
            for c in "01":
                assert sum(f"thermo_bwdILb{a}ELb{b}ELb{c}E" in n for n in bwd) == 1
    for n, k in {**fwd, **bwd, **ps}.items():
        assert k["vgpr"] - k["agpr"] <= 128 and k["spill"] == 0 and k["scratch"] == 0 and k["lds"] == 0, (n[:120], k)
