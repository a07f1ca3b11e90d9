"""moist_cv for six water species (pace_amd/csrc/fv3_moist.hip) through MoistCV / TemperatureToPotential(water=...) and the C ABI:
bitwise parity of q_con, cappa and cvm with the numpy restatement (tests/moist_reference.py) in fp64 and fp32, a NULL species against
a field of zeros, cvm = NULL, what must stay untouched; the fused preamble against fv3_moist_cv + fv3_pt_from_temperature (bitwise)
and against the restatement (the bounds of tests/test_thermo.py); the argument checks; the register budget of the kernels.  Every
operator case runs on the host emulation (CPU suite) and on the HIP library (-m gpu), on the shapes of tests/test_thermo.py.

The species are drawn in the ranges of the restart fixture (specific humidity up to 0.018, condensate up to 6e-4 per species), with
exact zeros and a few slightly negative condensate values (what a remap leaves before fillz); a random subset of the five optional
species is NULL."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

import moist_reference as mref
import test_thermo as tt
import thermo_reference as tref
from pace_amd import lib as _lib
from pace_amd.stencils import MoistCV, TemperatureToPotential, WaterSpecies
from test_thermo import real  # noqa: F401  (the (backend, dtype) fixture)

ROOT = tt.ROOT
NH, SENTINEL, DIMS, NP_OF = tt.NH, tt.SENTINEL, tt.DIMS, tt.NP_OF
_bits, _sync = tt._bits, tt._sync
OPTIONAL = mref.ROLES[1:]


@functools.lru_cache(maxsize=None)
def _species(n, n_sub, nz, npd_name):
    """Per sub-domain the compute cells (n, n, nz) of the six species, and the optional roles that are given as NULL for this shape
    (a random subset, fixed by the shape).  Computed once per shape and dtype, shared, never modified."""
    npd = np.dtype(npd_name).type
    rng = np.random.default_rng(20261019 + n + 11 * nz)
    out = []
    for _ in range(n_sub):
        shp = (n, n, nz)
        d = {"qvapor": rng.uniform(1.0e-7, 0.018, shp) * (rng.random(shp) < 0.8)}
        for role in OPTIONAL:
            q = rng.uniform(0.0, 6.0e-4, shp) * (rng.random(shp) < 0.5)  # (half exact zeros)
            neg = rng.random(shp) < 0.02
            q[neg] = -rng.uniform(1.0e-12, 1.0e-7, int(neg.sum()))  # slightly negative layer means
            d[role] = q
        d = {k: np.ascontiguousarray(v.astype(npd)) for k, v in d.items()}
        for v in d.values():
            v.setflags(write=False)
        assert any((d[r] == 0).any() for r in OPTIONAL) and any((d[r] < 0).any() for r in OPTIONAL)
        out.append(d)
    null = tuple(r for r in OPTIONAL if rng.random() < 0.4)
    return out, null


class Water:
    """Device quantities of one case: the species (the sentinel outside the compute box and on the pad level; a role in `null` is not
    given, a role in `zeros` is a field of zeros), and the named outputs filled with the sentinel."""

    def __init__(self, sf, species, npd, null=(), zeros=(), outputs=("q_con", "cappa", "cvm"), extra=None):
        qf = sf.quantity_factory
        self.sf, self.npd = sf, npd
        self.n, _, self.nz = species[0]["qvapor"].shape
        self.host = {}
        for role in mref.ROLES:
            if role in null:
                continue
            self.host[role] = [tt._padded(np.zeros_like(s[role]) if role in zeros else s[role], 0.0 if role in zeros else SENTINEL, npd) for s in species]
        for k, cells in (extra or {}).items():
            self.host[k] = [tt._padded(a, SENTINEL, npd) for a in cells]
        shape = tt._padded(species[0]["qvapor"], SENTINEL, npd).shape
        for k in outputs:
            self.host[k] = [np.full(shape, SENTINEL, dtype=npd) for _ in species]
        self.q = {k: qf.from_array(v, DIMS) for k, v in self.host.items()}
        self.water = WaterSpecies(**{r: self.q[r] for r in mref.ROLES if r in self.q})

    def cells(self, name, r):
        return self.q[name].numpy(r)[NH : NH + self.n, NH : NH + self.n, : self.nz]

    def check_untouched(self, written):
        """Inputs and outputs that were not given are unchanged everywhere; the written fields keep the sentinel outside the compute
        box and on the pad level.  Bitwise."""
        _sync(self.sf)
        n, nz = self.n, self.nz
        for name, host in self.host.items():
            for r, h in enumerate(host):
                got = self.q[name].numpy(r)
                if name not in written:
                    assert np.array_equal(_bits(got), _bits(h)), f"{name} (not an output of this call) was written"
                    continue
                outside = np.ones(h.shape, dtype=bool)
                outside[NH : NH + n, NH : NH + n, :nz] = False
                assert np.array_equal(_bits(got[outside]), _bits(h[outside])), f"{name}: a halo cell or the pad level was written"
                inside = got[NH : NH + n, NH : NH + n, :nz]
                assert not (inside == npd_sentinel(self.npd)).any(), f"{name}: a compute cell was not written"


def npd_sentinel(npd):
    return npd(SENTINEL)


def _reference(species, null):
    return [mref.moist_cv(**{r: (None if r in null else s[r]) for r in mref.ROLES}) for s in species]


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. fv3_moist_cv against the restatement: bitwise, both precisions, both builds
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx_tile, layout, nz", tt.SHAPES, ids=tt.SHAPE_IDS)
def test_moist_cv_matches_the_restatement_bitwise(real, nx_tile, layout, nz):  # noqa: F811
    backend, dtype = real
    npd = NP_OF[dtype]
    part, grids, sf = tt._factory(backend, nx_tile, layout, nz, dtype)
    species, null = _species(part.nx, len(grids), nz, npd.__name__)
    for nulls in (null, (), OPTIONAL):  # the shape's random subset, all six species, qvapor alone
        want = _reference(species, nulls)
        W = Water(sf, species, npd, null=nulls)
        MoistCV(sf)(W.water, W.q["q_con"], W.q["cappa"], W.q["cvm"])
        W.check_untouched({"q_con", "cappa", "cvm"})
        for r in range(len(grids)):
            for k, w in zip(("q_con", "cappa", "cvm"), want[r]):
                assert w.dtype == npd and np.array_equal(_bits(W.cells(k, r)), _bits(w)), (k, r, nulls)
        # cvm = NULL writes nothing extra, q_con and cappa are the same
        V = Water(sf, species, npd, null=nulls)
        MoistCV(sf)(V.water, V.q["q_con"], V.q["cappa"])
        V.check_untouched({"q_con", "cappa"})
        for r in range(len(grids)):
            for k in ("q_con", "cappa"):
                assert np.array_equal(_bits(V.q[k].numpy(r)), _bits(W.q[k].numpy(r))), (k, r)
    c = want[0][1]
    print(f"moist_cv {backend} {npd.__name__} C{nx_tile} {layout} L{nz}: NULL {null or 'none'}; cappa {c.min():.6f} .. {c.max():.6f} (qvapor alone)")


def test_a_null_species_is_a_field_of_zeros_bitwise(real):  # noqa: F811
    backend, dtype = real
    npd = NP_OF[dtype]
    nz = 5
    part, grids, sf = tt._factory(backend, 12, (1, 1), nz, dtype)
    species, _ = _species(12, len(grids), nz, npd.__name__)
    for roles in (("qrain",), ("qliquid", "qrain"), ("qice", "qsnow", "qgraupel"), OPTIONAL):
        A = Water(sf, species, npd, null=roles)
        B = Water(sf, species, npd, zeros=roles)
        MoistCV(sf)(A.water, A.q["q_con"], A.q["cappa"], A.q["cvm"])
        MoistCV(sf)(B.water, B.q["q_con"], B.q["cappa"], B.q["cvm"])
        _sync(sf)
        for r in range(len(grids)):
            for k in ("q_con", "cappa", "cvm"):
                assert np.array_equal(_bits(A.q[k].numpy(r)), _bits(B.q[k].numpy(r))), (k, roles)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the fused preamble against fv3_moist_cv + fv3_pt_from_temperature (bitwise) and against the restatement
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx_tile, layout, nz", tt.SHAPES, ids=tt.SHAPE_IDS)
def test_fused_preamble_is_moist_cv_then_the_dry_preamble(real, nx_tile, layout, nz):  # noqa: F811
    backend, dtype = real
    npd = NP_OF[dtype]
    part, grids, sf = tt._factory(backend, nx_tile, layout, nz, dtype)
    n_sub = len(grids)
    species, null = _species(part.nx, n_sub, nz, npd.__name__)
    cells = tt._random_cells(part.nx, n_sub, nz, npd.__name__)
    extra = lambda: {"delp": [c["delp"] for c in cells], "delz": [c["delz"] for c in cells]}  # noqa: E731

    def fields():
        W = Water(sf, species, npd, null=null, outputs=("q_con", "cappa", "pkz"), extra=extra())
        W.host["pt"] = [tt._padded(c["T"], SENTINEL, npd) for c in cells]
        W.q["pt"] = sf.quantity_factory.from_array(W.host["pt"], DIMS)
        return W

    A, B = fields(), fields()
    q = A.q
    TemperatureToPotential(sf)(q["pt"], q["pkz"], q["delp"], q["delz"], q["q_con"], q["cappa"], water=A.water)
    A.check_untouched({"pt", "pkz", "q_con", "cappa"})
    q = B.q
    MoistCV(sf)(B.water, q["q_con"], q["cappa"])
    TemperatureToPotential(sf)(q["pt"], q["pkz"], q["delp"], q["delz"], q["q_con"], q["cappa"], q["qvapor"])
    B.check_untouched({"pt", "pkz", "q_con", "cappa"})
    worst = {}
    for r in range(n_sub):
        for k in ("pt", "pkz", "q_con", "cappa"):
            assert np.array_equal(_bits(A.q[k].numpy(r)), _bits(B.q[k].numpy(r))), (k, r)
        # the restatement in the array's dtype and in float64 on the same inputs
        sp = {k: (None if k in null else species[r][k]) for k in mref.ROLES}
        c = cells[r]
        q_con, cappa, _ = mref.moist_cv(**sp)
        own = tref.pt_from_temperature(c["T"], c["delp"], c["delz"], q_con, cappa, sp["qvapor"])
        q64, c64, _ = mref.moist_cv(**{k: (None if v is None else v.astype(np.float64)) for k, v in sp.items()})
        r64 = tref.pt_from_temperature(*(c[k].astype(np.float64) for k in ("T", "delp", "delz")), q64, c64, sp["qvapor"].astype(np.float64))
        assert np.array_equal(_bits(A.cells("q_con", r)), _bits(q_con)) and np.array_equal(_bits(A.cells("cappa", r)), _bits(cappa))
        tt._bound("moist fwd pt", A.cells("pt", r), own[0], r64[0], npd, worst)
        tt._bound("moist fwd pkz", A.cells("pkz", r), own[1], r64[1], npd, worst)
    print(f"moist preamble {backend} {npd.__name__} C{nx_tile} {layout} L{nz}: (error, E_ref) " + ", ".join(f"{k} ({v[0]:.2e}, {v[1]:.2e})" for k, v in worst.items()))


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. argument checks through the C ABI (fv3_moist_cv, fv3_pt_from_temperature_moist; fv3_remap_moist: tests/test_moist_step.py)
# ---------------------------------------------------------------------------------------------------------------------------------
def test_argument_checks(backend):
    nz = 4
    part, grids, sf = tt._factory(backend, 12, (1, 1), nz, torch.float64)
    qf = sf.quantity_factory
    species, _ = _species(12, len(grids), nz, "float64")
    cells = tt._random_cells(12, len(grids), nz, "float64")
    W = Water(sf, species, np.float64, outputs=("q_con", "cappa", "cvm", "pkz"), extra={"delp": [c["delp"] for c in cells], "delz": [c["delz"] for c in cells], "pt": [c["T"] for c in cells]})
    q = W.q
    flat = qf.zeros(("x", "y"))
    other = qf.zeros(DIMS)
    short = _lib.fv3_field()
    C.memmove(C.byref(short), C.byref(other.field), C.sizeof(_lib.fv3_field))
    short.shape[2] -= 1  # a 3-D field of another vertical extent
    before = {k: v.storage.clone() for k, v in q.items()}
    lib, ctx, s = sf.lib, sf.ctx, sf.stream_handle
    ARG = -1

    def ref(v):
        return None if v is None else (C.pointer(v) if isinstance(v, _lib.fv3_field) else C.pointer(v.field))

    def water(**swap):
        sp = {r: swap.get(r, q[r]) for r in mref.ROLES}
        return C.byref(_lib.fv3_water(*[ref(sp[r]) for r in mref.ROLES], 1384.5, 4185.5, 1972.0))

    def cv(ctx_=ctx, no_water=False, **swap):
        o = {k: swap.get(k, q[k]) for k in ("q_con", "cappa", "cvm")}
        return lib.fv3_moist_cv(ctx_, None if no_water else water(**swap), *[ref(o[k]) for k in ("q_con", "cappa", "cvm")], s)

    def fwd(ctx_=ctx, no_water=False, **swap):
        o = {k: swap.get(k, q[k]) for k in ("pt", "pkz", "delp", "delz", "q_con", "cappa")}
        return lib.fv3_pt_from_temperature_moist(ctx_, *[ref(o[k]) for k in ("pt", "pkz", "delp", "delz", "q_con", "cappa")], None if no_water else water(**swap), s)

    cases = [
        ("cv: null water", cv, dict(no_water=True), b"moist_cv: the fv3_water is null"),
        ("cv: null qvapor", cv, dict(qvapor=None), b"'qvapor': null"),
        ("cv: 2-D qrain", cv, dict(qrain=flat), b"'qrain': vertical shape"),
        ("cv: mis-shaped qsnow", cv, dict(qsnow=short), b"'qsnow': vertical shape"),
        ("cv: 2-D qvapor", cv, dict(qvapor=flat), b"'qvapor': vertical shape"),
        ("cv: 2-D cappa", cv, dict(cappa=flat), b"'cappa_': vertical shape"),
        ("cv: null q_con", cv, dict(q_con=None), b"'q_con_': null"),
        ("cv: 2-D cvm", cv, dict(cvm=flat), b"'cvm_': vertical shape"),
        ("cv: q_con is cappa", cv, dict(cappa=q["q_con"]), b"q_con and cappa are the same field"),
        ("cv: cvm is q_con", cv, dict(cvm=q["q_con"]), b"q_con and cvm are the same field"),
        ("cv: cvm is cappa", cv, dict(cvm=q["cappa"]), b"cappa and cvm are the same field"),
        ("cv: q_con is qliquid", cv, dict(q_con=q["qliquid"]), b"q_con is the qliquid field"),
        ("cv: cappa is qvapor", cv, dict(cappa=q["qvapor"]), b"cappa is the qvapor field"),
        ("cv: cvm is qgraupel", cv, dict(cvm=q["qgraupel"]), b"cvm is the qgraupel field"),
        ("fwd: null water", fwd, dict(no_water=True), b"pt_from_temperature_moist: the fv3_water is null"),
        ("fwd: null qvapor", fwd, dict(qvapor=None), b"'qvapor': null"),
        ("fwd: 2-D qice", fwd, dict(qice=flat), b"'qice': vertical shape"),
        ("fwd: mis-shaped qliquid", fwd, dict(qliquid=short), b"'qliquid': vertical shape"),
        ("fwd: 2-D pt", fwd, dict(pt=flat), b"'pt_': vertical shape"),
        ("fwd: null delz", fwd, dict(delz=None), b"'delz_': null"),
        ("fwd: pt is pkz", fwd, dict(pkz=q["pt"]), b"pt and pkz are the same field"),
        ("fwd: q_con is cappa", fwd, dict(cappa=q["q_con"]), b"q_con and cappa are the same field"),
        ("fwd: pkz is q_con", fwd, dict(q_con=q["pkz"]), b"pkz and q_con are the same field"),
        ("fwd: pt is delp", fwd, dict(pt=q["delp"]), b"pt is the delp field"),
        ("fwd: cappa is delz", fwd, dict(cappa=q["delz"]), b"cappa is the delz field"),
        ("fwd: q_con is qrain", fwd, dict(q_con=q["qrain"]), b"q_con is the qrain field"),
        ("fwd: pt is qvapor", fwd, dict(pt=q["qvapor"]), b"pt is the qvapor field"),
    ]
    for what, entry, swap, word in cases:
        assert cv(q_con=flat) == ARG and b"'q_con_': vertical shape" in lib.fv3_last_error(ctx)  # (another message in between: the one below is this case's own)
        st = entry(**swap)
        msg = lib.fv3_last_error(ctx)
        assert st == ARG, (what, st)
        assert msg and word in msg, (what, msg)
        _sync(sf)
        for k, b in before.items():
            assert torch.equal(q[k].storage, b), (what, k)
    assert cv(ctx_=None) == ARG and b"context is null" in lib.fv3_last_error(None)
    assert fwd(ctx_=None) == ARG and b"context is null" in lib.fv3_last_error(None)
    # ... and the operators raise what the entries report
    with pytest.raises(_lib.Fv3Error, match="same field"):
        MoistCV(sf)(W.water, q["q_con"], q["q_con"])
    with pytest.raises(_lib.Fv3Error, match="is the qsnow field"):
        TemperatureToPotential(sf)(q["pt"], q["pkz"], q["delp"], q["delz"], q["qsnow"], q["cappa"], water=W.water)
    with pytest.raises(ValueError, match="qvapor is required"):
        WaterSpecies(None, qliquid=q["qliquid"])
    _sync(sf)
    for k, b in before.items():
        assert torch.equal(q[k].storage, b), k


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. register budget (read from the code-object metadata of the built library: no GPU needed)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [64, 32])
def test_moist_cell_kernels_stay_inside_the_register_budget(precision):
    """Streaming cell kernels want at least four waves per SIMD: both instantiations of the moist_cv kernel (cvm present / absent),
    the fused preamble and the thickness kernel of the moist fill have at most 128 architectural VGPRs, nothing spilled, no scratch, no LDS."""
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
    cv = {n: k for n, k in ks.items() if "moist_cv_cells" in n}
    pre = {n: k for n, k in ks.items() if "moist_preamble_cells" in n}
    # ... and the cell kernel of the moist remap that turns delp into the Eulerian thickness before the filling (the second launch3<4>
    # lambda of remap_all; the first is the T_v kernel of both remaps)
    dp2 = {n: k for n, k in ks.items() if "remap_all" in n and "fv3_k3ILi4E" in n and "EUliiiiE0_" in n}
    assert len(cv) == 2 and len(pre) == 1 and len(dp2) == 1, (sorted(cv), sorted(pre), sorted(dp2))
    for a in "01":
        assert sum(f"moist_cv_cellsILb{a}E" in n for n in cv) == 1
    for n, k in {**cv, **pre, **dp2}.items():
        print(f"f{precision} {n[:70]}: {k}")
        assert k["vgpr"] - k["agpr"] <= 128 and k["spill"] == 0 and k["scratch"] == 0 and k["lds"] == 0, (n[:120], k)
