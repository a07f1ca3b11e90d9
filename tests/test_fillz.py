"""fv3_fillz (pace_amd/csrc/fv3_fillz.hip) through FillNegativeTracerValues and the C ABI: hand-computed columns, bitwise parity with
the numpy restatement (tests/fillz_reference.py) on random columns in fp64 and fp32, the argument checks, the register budget of
the kernels.  Every case runs on the host emulation (CPU suite) and on the HIP library (-m gpu).

(fv3_fillz answers nz < 2 with FV3_ERR_UNSUPPORTED, but a context needs nz >= 3 to be created, so that status cannot be reached
through the ABI and has no case here.)"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

from fillz_reference import BRANCHES, fillz as ref_fillz
from pace_amd import lib as _lib
from pace_amd._testing import stencil_factory_for
from pace_amd.config import AcousticDynamicsConfig
from pace_amd.constants import get_constants
from pace_amd.grid import make_grid
from pace_amd.stencils import FillNegativeTracerValues
from pace_amd.topology import CubedSpherePartitioner

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NH = 3
SENTINEL = -777.25  # negative: a kernel that touched a halo cell or the pad level would try to fill it
DIMS = ("x", "y", "z")
NP_OF = {torch.float64: np.float64, torch.float32: np.float32}


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
def _grids(nx_tile, layout, nz):
    part = CubedSpherePartitioner(nx_tile, layout)
    return part, [make_grid(part, r, nz=nz) for r in range(part.total_ranks)]


def _factory(backend, nx_tile, layout, nz, dtype):
    part, grids = _grids(nx_tile, layout, nz)
    # (nord = 0: the fp32 context refuses the C12 del-6 damping tables, which overflow the float range; fillz reads none)
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
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


# ---------------------------------------------------------------------------------------------------------------------------------
# hand-computed columns: exact in both precisions, independent of either implementation
# ---------------------------------------------------------------------------------------------------------------------------------
HAND = {
    3: [  # (q, dp, expected)
        ([-1, 3, 0], [1, 1, 1], [0, 2, 0]),
        ([2, -1, 3], [1, 1, 1], [1, 0, 3]),
        ([-1, 1, 1], [2, 1, 4], [0, 0, 0.75]),
    ],
    4: [
        ([1, -3, 1, 4], [1, 1, 1, 1], [0, 0, 0, 3]),    # both borrows, then fac = 0.75
        ([1, 2, 0, -1], [1, 1, 1, 1], [1, 2, 0, -1]),   # the bottom layer is left alone
        ([1, 2, 3, -1], [1, 1, 1, 1], [1, 2, 2, 0]),
        ([0, -2, 1, 0], [1, 1, 1, 1], [0, -1, 0, 0]),   # sum0 <= 0: no non-local fix
    ],
}
# (sub-domain, i, j) of the columns that hold them: corners, edges and interior cells of different tiles
SPOTS = [(0, 0, 0), (2, 5, 7), (5, 11, 11), (3, 11, 0)]


@pytest.mark.parametrize("nz", [3, 4])
def test_hand_computed_columns(real, nz):
    backend, dtype = real
    npd = NP_OF[dtype]
    part, grids, sf = _factory(backend, 12, (1, 1), nz, dtype)
    qf = sf.quantity_factory
    q_cells = [np.full((12, 12, nz), 1.5, dtype=npd) for _ in grids]
    dp_cells = [np.ones((12, 12, nz), dtype=npd) for _ in grids]
    want = [a.copy() for a in q_cells]
    for (r, i, j), (q, dp, exp) in zip(SPOTS, HAND[nz]):
        q_cells[r][i, j] = q
        dp_cells[r][i, j] = dp
        want[r][i, j] = exp
    tr = {"q": qf.from_array([_padded(a, SENTINEL, npd) for a in q_cells], DIMS)}
    dp = qf.from_array([_padded(a, 1.0, npd) for a in dp_cells], DIMS)
    FillNegativeTracerValues(sf, qf, grids)(dp, tr)
    _sync(sf)
    for r in range(len(grids)):
        got = tr["q"].numpy(r)
        assert np.all(got == _padded(want[r], SENTINEL, npd)), (r, got[NH : NH + 12, NH : NH + 12, :nz][want[r] != got[NH : NH + 12, NH : NH + 12, :nz]])


# ---------------------------------------------------------------------------------------------------------------------------------
# random columns: bitwise parity with the restatement, the properties of the algorithm
# ---------------------------------------------------------------------------------------------------------------------------------
def _random_inputs(n, n_sub, nz, n_tracers, npd):
    """dp and the tracers' compute cells per sub-domain: dp uniform in (50, 2000), q = N(0.3, 1) with 30 % exact zeros, the first
    quarter of the columns made non-negative.  Tracer 0 and dp share the generator of seed 5, tracer t has seed 5 + t."""
    ncol = n * n
    rngs = [np.random.default_rng(5 + t) for t in range(n_tracers)]
    dps, qs = [], [[] for _ in range(n_tracers)]
    for _ in range(n_sub):
        dps.append(rngs[0].uniform(50.0, 2000.0, (ncol, nz)).astype(npd))
        for t, rng in enumerate(rngs):
            q = (rng.normal(0.3, 1.0, (ncol, nz)) * (rng.random((ncol, nz)) < 0.7)).astype(npd)
            q[: ncol // 4] = np.abs(q[: ncol // 4])
            qs[t].append(q)
    return dps, qs


SHAPES = [(12, (1, 1), 3), (12, (1, 1), 5), (12, (1, 1), 8), (12, (1, 1), 79), (12, (2, 2), 8), (96, (1, 1), 5)]


@pytest.mark.parametrize("n_tracers", [2, 5])
@pytest.mark.parametrize("nx_tile, layout, nz", SHAPES, ids=[f"c{s[0]}_{s[1][0]}x{s[1][1]}_l{s[2]}" for s in SHAPES])
def test_random_columns_match_the_restatement_bitwise(real, nx_tile, layout, nz, n_tracers):
    backend, dtype = real
    npd = NP_OF[dtype]
    part, grids, sf = _factory(backend, nx_tile, layout, nz, dtype)
    qf = sf.quantity_factory
    n, n_sub = part.nx, len(grids)
    ncol = n * n
    dps, qs = _random_inputs(n, n_sub, nz, n_tracers, npd)
    dp_host = [_padded(d.reshape(n, n, nz), 1000.0, npd) for d in dps]
    q_host = [[_padded(q.reshape(n, n, nz), SENTINEL, npd) for q in qs[t]] for t in range(n_tracers)]
    dp = qf.from_array(dp_host, DIMS)
    tr = {f"q{t}": qf.from_array(q_host[t], DIMS) for t in range(n_tracers)}
    FillNegativeTracerValues(sf, qf, grids)(dp, tr)
    _sync(sf)
    eps = float(np.finfo(npd).eps)
    taken = {b: 0 for b in BRANCHES}
    cs = (slice(NH, NH + n), slice(NH, NH + n), slice(0, nz))
    worst_mass = 0.0
    for r in range(n_sub):
        assert np.array_equal(_bits(dp.numpy(r)), _bits(dp_host[r])), "dp was written"
        for t in range(n_tracers):
            want, br = ref_fillz(qs[t][r], dps[r])
            assert want.dtype == npd
            got_full = tr[f"q{t}"].numpy(r)
            got = got_full[cs].reshape(ncol, nz)
            # the result is the restatement's, bit for bit (NaN-free inputs: value equality + the sign of zero)
            assert np.array_equal(_bits(got), _bits(want)), (r, t, np.argwhere(_bits(got) != _bits(want))[:5], got[got != want][:5], want[got != want][:5])
            # halo cells and the pad level keep the sentinel
            outside = np.ones(got_full.shape, dtype=bool)
            outside[cs] = False
            assert np.array_equal(_bits(got_full[outside]), _bits(q_host[t][r][outside]))
            # the all-positive quarter is not modified
            assert np.array_equal(_bits(got[: ncol // 4]), _bits(qs[t][r][: ncol // 4]))
            assert not br["zfix"][: ncol // 4].any() and not br["top"][: ncol // 4].any()
            # column mass
            m0 = (qs[t][r].astype(np.float64) * dps[r].astype(np.float64)).sum(axis=1)
            m1 = (got.astype(np.float64) * dps[r].astype(np.float64)).sum(axis=1)
            scale = np.abs(qs[t][r].astype(np.float64) * dps[r].astype(np.float64)).sum(axis=1)
            rel = np.abs(m1 - m0) / np.where(scale > 0, scale, 1.0)
            worst_mass = max(worst_mass, float(rel.max()) / eps)
            assert np.all(np.abs(m1 - m0) <= 8.0 * eps * scale), (r, t, float(rel.max()) / eps)
            # the non-local fix leaves nothing negative below the top level
            assert not (got[br["nonlocal"], 1:] < 0).any()
            for b in BRANCHES:
                taken[b] += int(br[b].sum())
    print(f"fillz {backend} {npd.__name__} C{nx_tile} {layout} L{nz} x{n_tracers}: branch members {taken}, worst mass error {worst_mass:.2f} eps")
    assert all(v > 0 for v in taken.values()), taken


# ---------------------------------------------------------------------------------------------------------------------------------
# argument checks through the C ABI
# ---------------------------------------------------------------------------------------------------------------------------------
def test_argument_checks(backend):
    nz = 4
    part, grids, sf = _factory(backend, 12, (1, 1), nz, torch.float64)
    qf = sf.quantity_factory
    rng = np.random.default_rng(1)
    mk = lambda: qf.from_array([rng.normal(0.0, 1.0, (12 + 2 * NH + 1, 12 + 2 * NH + 1, nz + 1)) for _ in grids], DIMS)  # noqa: E731
    q0, q1, dp = mk(), mk(), mk()
    dp.storage.abs_().add_(1.0)
    flat = qf.zeros(("x", "y"))
    other = torch.zeros((6, nz + 2, 12 + 2 * NH + 1, 12 + 2 * NH + 1), dtype=torch.float64, device=q0.storage.device)
    from pace_amd.quantity import Quantity

    odd = Quantity(other, DIMS)
    before = [x.storage.clone() for x in (q0, q1, dp)]
    fn, ctx, s = sf.lib.fv3_fillz, sf.ctx, sf.stream_handle

    def arr(*qs):
        return (_lib.F * max(len(qs), 1))(*[C.pointer(q.field) for q in qs])

    ARG, UNSUPPORTED = -1, -3
    cases = [
        ("negative n_tracers", (-1, arr(q0), dp.fref), ARG, b"n_tracers"),
        ("null list", (1, None, dp.fref), ARG, b"null"),
        ("null dp", (1, arr(q0), None), ARG, b"null"),
        ("2-D dp", (1, arr(q0), flat.fref), ARG, b"dp"),
        ("a tracer that fails the layout check", (2, arr(q0, odd), dp.fref), ARG, b"tracer"),
        ("a 2-D tracer", (1, arr(flat), dp.fref), ARG, b"tracer"),
        ("dp among the tracers", (2, arr(q0, dp), dp.fref), ARG, b"dp"),
        ("the same tracer twice", (3, arr(q0, q1, q0), dp.fref), ARG, b"same field"),
    ]
    assert UNSUPPORTED == -3  # (the status of nz < 2: see the module docstring)
    for what, (n, lst, d), status, word in cases:
        sf.lib.fv3_fillz(ctx, 0, arr(), dp.fref, s)  # (a passing call in between: the message below is this case's own)
        st = fn(ctx, n, lst, d, s)
        msg = sf.lib.fv3_last_error(ctx)
        assert st == status, (what, st)
        assert msg and word in msg, (what, msg)
        _sync(sf)
        for x, b in zip((q0, q1, dp), before):
            assert torch.equal(x.storage, b), what
    # no tracers: fine, nothing happens
    assert fn(ctx, 0, None, dp.fref, s) == 0
    assert fn(ctx, 0, arr(), dp.fref, s) == 0
    _sync(sf)
    for x, b in zip((q0, q1, dp), before):
        assert torch.equal(x.storage, b)
    # ... and the operator raises what the entry reports
    with pytest.raises(_lib.Fv3Error, match="same field"):
        FillNegativeTracerValues(sf, qf, grids)(dp, {"a": q0, "b": q0})


# ---------------------------------------------------------------------------------------------------------------------------------
# register budget (read from the code-object metadata of the built library: no GPU needed)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [64, 32])
def test_fillz_kernels_stay_inside_the_register_budget(precision):
    """A memory-bound column kernel wants four waves per SIMD: every instantiation (1 .. 4 tracers per thread) has at most 128
    architectural VGPRs, nothing spilled, no scratch."""
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
    hits = {n: k for n, k in ks.items() if "fillz_group" in n}
    assert len(hits) == 4, sorted(hits)
    for g in range(1, 5):
        assert sum(f"fillz_groupILi{g}E" in n for n in hits) == 1, (g, sorted(hits))
    for n, k in hits.items():
        assert k["vgpr"] - k["agpr"] <= 128 and k["spill"] == 0 and k["scratch"] == 0, (n[:100], k)
