"""The halo layer -- pace_amd/topology.py's maps, pace_amd/halo.py's plans and message layout, the gather kernels of csrc/fv3_ctx.hip and the halo
plans of csrc/fv3_halo.hip -- against a reference built from positions on the sphere (tests/halo_reference.py), point by point.  A correct halo update
is a signed copy, so EVERY value comparison below is exact equality and every test asserts how many points it compared.

  1  the reference itself: it imports none of the library's frame algebra, and its interface sync is a bit-exact no-op on the D-grid winds the Fortran
     model wrote (tests/golden/c12_restart_6tiles.npz: 144 faces x 63 levels) -- and stops being one with the along-edge order reversed or a sign flipped
  2  build_halo_map / build_interface_sync_map == the reference, as dictionaries (destination component, i, j) -> (source tile, source component,
     tile-global i, tile-global j, sign); the entry count against the closed form; five controls, each of which must make the same comparer fail
  3  HaloExchanger updates of coded fields (tests/halo_exchange_case.py) on the host emulation and on the MI355X, fp64 and fp32: kinds, depths, layouts,
     level counts around the gather kernels' 8-level thread tile, 2-D fields, updates of more gathers than one batched launch takes, FV3_GATHER_BATCH=0 in a
     fresh process, and the ordering of the communication stream against the compute stream
  4  the plan ABI alone (fv3_gather_*, fv3_halo_plan_*, fv3_ctx_set_xfer) with hand-made plans against a numpy restatement
  6  more sub-domains in one process than a context holds: a ValueError that says so

(5, the message path between processes, is in tests/test_distributed.py and tests/test_gpu_invariants.py.)

Nothing here has a tolerance.  The counts are closed forms: per rank and component the depth-d frame (ex + 2 d)(ey + 2 d) - ex ey of the component's
extent, minus d^2 for every corner of the rank that is a cube corner; nx + ny for the sync.  An exchange needs a context, and a context takes
sub-domains of 6 x 6 cells or more, so C12 layouts 3x3 and 4x4 are compared as maps only.

Measured: every test passed on its first run on the host emulation and on the MI355X, fp64 and fp32; the GPU cases of this file take 14 s together
(100 tests; the FV3_GATHER_BATCH=0 child 3.7 s, the two C48 L32 stream cases 0.3 s each, every other case below 0.25 s).
"""
import ast
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import halo_exchange_case as hc
import halo_reference as hr
from pace_amd.topology import STAGGER, CubedSpherePartitioner, build_halo_map, build_interface_sync_map

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "c12_restart_6tiles.npz")
NH = 3
LIB_STAGGER = {
    "cell": [STAGGER["cell"]],
    "corner": [STAGGER["corner"]],
    "dgrid": [STAGGER["dgrid_u"], STAGGER["dgrid_v"]],
    "cgrid": [STAGGER["cgrid_u"], STAGGER["cgrid_v"]],
}


def _build32(request, param):
    from pace_amd import build, lib

    if param == "hostemu":
        build.build(32, hostemu=True, verbose=False)
    else:
        request.getfixturevalue("gpu_backend")
        if not os.path.exists(build.lib_path(32)):
            build.build(32)
        lib.load(32)
    return param


@pytest.fixture(params=["hostemu", pytest.param("hip:gfx950", marks=pytest.mark.gpu)])
def backend32(request):
    """The fp32 library: its host emulation (CPU suite) or the HIP build (-m gpu)."""
    return _build32(request, request.param)


@pytest.fixture(params=["hostemu", pytest.param("hip:gfx950", marks=pytest.mark.gpu)])
def backend_both(request):
    """Both precisions of one backend (for the tests that take the precision as a parameter, or run both in one child process)."""
    request.getfixturevalue("hostemu" if request.param == "hostemu" else "gpu_backend")
    return _build32(request, request.param)


# ---------------------------------------------------------------------------------------------------------------------------
# 1  the reference
# ---------------------------------------------------------------------------------------------------------------------------
FORBIDDEN = ("edge_transform", "EdgeTransform", "_locate", "build_halo_map", "build_interface_sync_map", "GatherMap")


def test_reference_imports_none_of_the_library_frame_algebra():
    tree = ast.parse(open(os.path.join(ROOT, "tests", "halo_reference.py")).read())
    imported = []
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            imported += [(a.name, None) for a in node.names]
        elif isinstance(node, ast.ImportFrom):
            imported += [(node.module, a.name) for a in node.names]
    assert sorted(imported) == [("numpy", None), ("pace_amd.grid", "tile_point")], imported
    names = {n.id for n in ast.walk(tree) if isinstance(n, ast.Name)} | {n.attr for n in ast.walk(tree) if isinstance(n, ast.Attribute)}
    assert not names & set(FORBIDDEN), names & set(FORBIDDEN)


def test_reference_sync_is_a_bit_exact_no_op_on_the_fortran_winds():
    data = np.load(GOLDEN)
    n, nz = 12, 63
    G = [[np.transpose(data["u"][t], (2, 1, 0)).astype(np.float64) for t in range(6)], [np.transpose(data["v"][t], (2, 1, 0)).astype(np.float64) for t in range(6)]]
    assert G[0][0].shape == (n, n + 1, nz) and G[1][0].shape == (n + 1, n, nz)
    st = hr.scatter(n, (1, 1), "sync_dgrid", G, np.nan)
    cu, cv = (slice(NH, NH + n), slice(NH, NH + n + 1)), (slice(NH, NH + n + 1), slice(NH, NH + n))

    def changed(sources=None):
        new, written = hr.apply_update(n, (1, 1), "sync_dgrid", 0, G, st, sources=sources)
        assert written == 144  # 6 tiles x (12 faces of the north row + 12 of the east column) = the 12 shared edges
        return sum(int((new[t][0][cu] != st[t][0][cu]).sum() + (new[t][1][cv] != st[t][1][cv]).sum()) for t in range(6))

    assert changed() == 0
    assert np.std(G[0][0][:, n, :]) > 1.0  # (the winds there are not trivially equal)
    own = {t: hr.halo_sources(n, (1, 1), t, "sync_dgrid", 0) for t in range(6)}
    assert sum(len(v) for v in own.values()) == 144 and all(s is not None and s[0] != t for t, v in own.items() for s in v.values())
    # mutation (a): the along-edge order of the sources reversed on every edge
    rev = {}
    for t, src in own.items():
        rev[t] = {}
        for comp in (0, 1):
            keys = sorted(k for k in src if k[0] == comp)
            rev[t].update({k: src[k2] for k, k2 in zip(keys, reversed(keys))})
    assert changed(rev) > 0.8 * 144 * nz
    # mutation (b): ONE sign flipped -- the 63 levels of that face change (where the wind is not zero)
    key = (0, NH + 4, NH + n)
    t2, c2, gi, gj, sg = own[2][key]
    flip = {t: dict(v) for t, v in own.items()}
    flip[2][key] = (t2, c2, gi, gj, -sg)
    nonzero = int((G[c2][t2][gi, gj, :] != 0).sum())
    assert nonzero > 60 and changed(flip) == nonzero


# ---------------------------------------------------------------------------------------------------------------------------
# 2  the library's maps against the reference
# ---------------------------------------------------------------------------------------------------------------------------
def library_map(part, rank, kind, depth):
    ni = part.nx + 2 * NH + 1
    if kind == "sync_dgrid":
        return build_interface_sync_map(part, rank, LIB_STAGGER["dgrid"], NH, ni)
    return build_halo_map(part, rank, LIB_STAGGER[kind], depth, NH, ni)


def as_dict(part, m):
    """GatherMap -> {(dst component, i, j): (source tile, source component, tile-global i, tile-global j, sign)}: the source as a point of its TILE, which
    removes the freedom of which rank owns a shared interface.  The rank arithmetic is restated here."""
    lx, ly = part.layout
    nx, ny = part.nx_tile // lx, part.nx_tile // ly
    ni = nx + 2 * NH + 1
    out = {}
    for e in range(len(m.dst_flat)):
        sr = int(m.src_rank[e])
        tile, sub = sr // (lx * ly), sr % (lx * ly)
        sx, sy = sub % lx, sub // lx
        si, sj = int(m.src_flat[e]) % ni, int(m.src_flat[e]) // ni
        key = (int(m.dst_comp[e]), int(m.dst_flat[e]) % ni, int(m.dst_flat[e]) // ni)
        assert key not in out, f"destination {key} written twice"
        out[key] = (tile, int(m.src_comp[e]), sx * nx + si - NH, sy * ny + sj - NH, int(m.sign[e]))
    return out


def compare_maps(lib, n, layout, rank, kind, depth):
    """The comparer: raises AssertionError unless the library's map is the reference's.  Returns the number of entries compared."""
    every = hc.sources(n, layout, rank, kind, depth)
    assert len(every) == hr.frame_count(n, layout, rank, kind, depth)  # no point of the halo frame is left out of the comparison
    ref = {k: v for k, v in every.items() if v is not None}
    # closed form: per component (ex + 2 d)(ey + 2 d) - ex ey, minus d^2 per corner of the rank that is a cube corner; the sync: nx + ny
    R = hr.Rank(n, layout, rank)
    if kind == "sync_dgrid":
        count = R.nx + R.ny
    else:
        count = sum((ex + 2 * depth) * (ey + 2 * depth) - ex * ey - R.tile_corners() * depth**2 for ex, ey in (R.extent(s) for s in hr.KINDS[kind]))
    assert len(ref) == count == hr.expected_count(n, layout, rank, kind, depth), (len(ref), count)
    assert set(lib) == set(ref), f"key sets differ: {sorted(set(lib) ^ set(ref))[:5]}"
    bad = [(k, lib[k], ref[k]) for k in ref if lib[k] != ref[k]]
    assert not bad, f"{len(bad)} entries differ, first (key, library, reference): {bad[0]}"
    return len(ref)


KIND_DEPTHS = [(k, d) for k in ("cell", "corner", "dgrid", "cgrid") for d in (1, 2, 3)] + [("sync_dgrid", 0)]


@pytest.mark.parametrize("n, layout", [(12, (1, 1)), (12, (2, 2)), (12, (3, 3)), (12, (1, 2)), (12, (2, 1)), (12, (4, 4)), (24, (2, 2)), (24, (3, 2)), (24, (4, 3))])
def test_library_maps_are_the_reference_maps(n, layout):
    part = CubedSpherePartitioner(n, layout)
    compared = 0
    for rank in range(part.total_ranks):
        for kind, depth in KIND_DEPTHS:
            compared += compare_maps(as_dict(part, library_map(part, rank, kind, depth)), n, layout, rank, kind, depth)
    lx, ly = layout
    nx, ny = n // lx, n // ly
    # the whole cube in closed form: frames of every rank minus the 24 d x d blocks beyond the 8 cube corners (3 tiles each), per component
    want = 0
    for kind, depth in KIND_DEPTHS:
        if kind == "sync_dgrid":
            want += 6 * lx * ly * (nx + ny)
            continue
        for ox, oy in hr.KINDS[kind]:
            ex, ey = nx + (ox == 0), ny + (oy == 0)
            want += 6 * lx * ly * ((ex + 2 * depth) * (ey + 2 * depth) - ex * ey) - 24 * depth**2
    assert compared == want, (compared, want)


def _mutations(part, rank, m):
    """the controls: (name, mutated copy of the library's map), where the map has what the control needs"""
    import copy

    lx, ly = part.layout
    own_tile = rank // (lx * ly)
    tiles = m.src_rank // (lx * ly)
    out = []
    across = np.nonzero(tiles != own_tile)[0]
    if len(across):  # the along-edge order reversed on one tile edge (the entries of one neighbouring tile, one destination component)
        sel = across[(tiles[across] == tiles[across[0]]) & (m.dst_comp[across] == m.dst_comp[across[0]])]
        x = copy.deepcopy(m)
        x.src_flat[sel], x.src_rank[sel] = m.src_flat[sel][::-1].copy(), m.src_rank[sel][::-1].copy()
        out.append(("reversed", x))
    x = copy.deepcopy(m)
    x.sign[len(m.sign) // 2] *= -1
    out.append(("sign", x))
    swapped = np.nonzero(m.src_comp != m.dst_comp)[0]
    if len(swapped):  # the components exchanged on one rotated edge
        sel = swapped[m.src_rank[swapped] == m.src_rank[swapped[0]]]
        x = copy.deepcopy(m)
        x.src_comp[sel] = 1 - m.src_comp[sel]
        out.append(("components", x))
    inside = np.nonzero((tiles == own_tile) & (m.src_rank != rank))[0]
    if len(inside):  # every source shifted by one cell on one sub-domain edge
        sel = inside[m.src_rank[inside] == m.src_rank[inside[0]]]
        x = copy.deepcopy(m)
        x.src_flat[sel] = m.src_flat[sel] + 1
        out.append(("shifted", x))
    x = copy.deepcopy(m)
    for f in ("dst_comp", "dst_flat", "src_rank", "src_comp", "src_flat", "sign"):
        setattr(x, f, np.delete(getattr(m, f), len(m.sign) // 3))
    out.append(("dropped", x))
    return out


def test_every_control_makes_the_map_comparer_fail():
    """C12 layout 2x2, rank 2 (north-west sub-domain of tile 0: two tile edges, both rotated, and two sub-domain edges)"""
    n, layout, rank = 12, (2, 2), 2
    part = CubedSpherePartitioner(n, layout)
    seen = {}
    for kind, depth in KIND_DEPTHS:
        m = library_map(part, rank, kind, depth)
        compare_maps(as_dict(part, m), n, layout, rank, kind, depth)
        for name, mutated in _mutations(part, rank, m):
            with pytest.raises(AssertionError):
                compare_maps(as_dict(part, mutated), n, layout, rank, kind, depth)
            seen.setdefault(name, set()).add(kind)
    every = {k for k, _ in KIND_DEPTHS}
    assert seen["reversed"] == every and seen["sign"] == every and seen["dropped"] == every
    assert seen["components"] == {"dgrid", "cgrid", "sync_dgrid"}  # (a scalar has no second component)
    assert seen["shifted"] == every


# ---------------------------------------------------------------------------------------------------------------------------
# 3  the exchanger
# ---------------------------------------------------------------------------------------------------------------------------
CASES = hc.case_list()


def _expected_points(case):
    n, layout, nz, kind, depth, groups, two_d = case
    return groups * sum(hr.expected_count(n, layout, r, kind, depth) for r in range(hr.total_ranks(layout)))


@pytest.mark.parametrize("case", CASES, ids=[hc.case_id(c) for c in CASES])
def test_update_matches_the_reference(backend, case):
    assert hc.run_case(backend, torch.float64, case) == _expected_points(case)


@pytest.mark.parametrize("case", CASES, ids=[hc.case_id(c) for c in CASES])
def test_update_matches_the_reference_fp32(backend32, case):
    assert hc.run_case(backend32, torch.float32, case) == _expected_points(case)


def test_case_list_covers_what_it_claims():
    levels = {c[2] + 1 for c in CASES if not c[6]}
    assert {7, 8, 9, 16, 17} <= levels and any(c[6] for c in CASES)
    assert {c[5] for c in CASES if c[3] == "cell"} >= {1, 13} and any(c[3] == "dgrid" and c[5] == 4 for c in CASES)
    assert {(c[3], c[4]) for c in CASES if c[1] == (1, 2)} >= {(k, d) for k in ("cell", "corner", "dgrid", "cgrid") for d in (3, 1)} | {("sync_dgrid", 0)}


def test_an_updater_refuses_to_mix_2d_and_3d_quantities(backend):
    from pace_amd.halo import HaloExchanger

    sf, part, lay = hc.factory(backend, torch.float64, 12, (1, 1), 7)
    qf = sf.quantity_factory
    with pytest.raises(ValueError, match="2-D and 3-D"):
        HaloExchanger.shared(sf, lay).updater("cell", [(qf.zeros(("x", "y", "z")),), (qf.zeros(("x", "y")),)])


def test_one_launch_per_gather_in_a_fresh_process(backend_both):
    """FV3_GATHER_BATCH=0 is read once per process: the whole case list, both precisions, in ONE child."""
    backend, precisions = backend_both, "64,32"
    env = dict(os.environ, FV3_GATHER_BATCH="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "halo_exchange_case.py"), "--backend", backend, "--precisions", precisions],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    assert f"checked {2 * sum(_expected_points(c) for c in CASES)} halo points" in r.stdout, r.stdout[-1000:]


def _stream_case(backend, monkeypatch, between):
    from pace_amd.halo import HaloExchanger

    monkeypatch.setenv("FV3_HALO_STREAM", "1")  # the exchange on the context's communication stream, even in one process
    n, layout, nz = 48, (1, 1), 32
    sf, part, lay = hc.factory(backend, torch.float64, n, layout, nz, fresh=True)
    ex = HaloExchanger.shared(sf, lay)
    if backend != "hostemu":
        assert ex.comm_stream is not None and sf.lib.fv3_ctx_get_comm_stream(sf.ctx)
    vec = hc.Coded(sf, lay, n, layout, "dgrid", 3, 1, first_field=0)
    sca = hc.Coded(sf, lay, n, layout, "cell", 3, 2, first_field=1)
    ups, fills = [], []
    for cd in (vec, sca):
        groups = cd.quantities(fill=False)
        ups.append(ex.updater(cd.kind, groups, n_halo=3))
        fills.append([[torch.from_numpy(cd.host_tensor(g, c)).to(sf.device) for c in range(cd.ncomp)] for g in range(len(groups))])
    qf = sf.quantity_factory
    other_src, other_dst = qf.empty(("x", "y", "z")), qf.zeros(("x", "y", "z"))
    other_src.storage.copy_(torch.arange(other_src.storage.numel(), dtype=torch.float64).reshape(other_src.storage.shape))
    hc.sync_device(sf)
    clones = []
    for cd, up, fill in zip((vec, sca), ups, fills):
        # the fill of the source fields is enqueued on the compute stream immediately before start(), the clone immediately after wait(): nothing
        # but the exchanger's own events orders the communication stream against them
        for gp, fg in zip(cd.q, fill):
            for q, f in zip(gp, fg):
                q.storage.copy_(f, non_blocking=True)
        up.start()
        if between:
            sf.call("copy", other_src.fref, other_dst.fref)  # an unrelated kernel on the compute stream while the exchange is in flight
        up.wait()
        clones.append([[q.storage.clone() for q in gp] for gp in cd.q])
    hc.sync_device(sf)
    checked = sum(cd.check(storages=cl) for cd, cl in zip((vec, sca), clones))
    # C48, one rank per tile: u 48 x 49, v 49 x 48, three cell fields... per tile, frames of depth 3 minus four 3 x 3 blocks
    frame = lambda ex_, ey_: (ex_ + 6) * (ey_ + 6) - ex_ * ey_ - 4 * 9  # noqa: E731
    assert checked == 6 * (frame(48, 49) + frame(49, 48) + 2 * frame(48, 48))
    if between:
        assert torch.equal(other_dst.storage, other_src.storage)


def test_exchange_on_the_communication_stream_is_ordered_against_the_compute_stream(backend, monkeypatch):
    _stream_case(backend, monkeypatch, between=False)


def test_compute_stream_work_between_start_and_wait(backend, monkeypatch):
    _stream_case(backend, monkeypatch, between=True)


# ---------------------------------------------------------------------------------------------------------------------------
# 4  the plan ABI alone
# ---------------------------------------------------------------------------------------------------------------------------
SENT = hc.SENTINEL


def _dev(sf, a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64)).to(sf.dtype).to(sf.device)


def _host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _gather_plan(sf, d, s, g):
    d, s, g = np.ascontiguousarray(d, dtype=np.int64), np.ascontiguousarray(s, dtype=np.int64), np.ascontiguousarray(g, dtype=np.int8)
    h = C.c_void_p()
    st = sf.lib.fv3_gather_plan_create(sf.ctx, C.byref(h), len(d), d.ctypes.data_as(C.POINTER(C.c_int64)), s.ctypes.data_as(C.POINTER(C.c_int64)),
                                       g.ctypes.data_as(C.POINTER(C.c_int8)))
    assert st == 0 and h.value
    return h


def _random_gather(rng, n, p_dst, p_src):
    """n unique destination offsets in random order, sources with repeats, signs of both kinds"""
    d = rng.permutation(p_dst)[:n]
    s = rng.integers(0, p_src, n)
    g = rng.choice(np.array([-1, 1]), n)
    g[0] = -1
    if n > 1:
        g[-1] = 1
    return d, s, g


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
def test_gather_run_is_a_signed_indexed_copy(backend_both, dtype):
    """dst[d[e] + k dks] = sign[e] src[s[e] + k sks], everything else untouched: element counts around the 256-thread workgroup and level counts around
    the 8-level thread tile, dks != sks."""
    sf, _, _ = hc.factory(backend_both, dtype, 12, (1, 1), 7)
    rng = np.random.default_rng(11)
    moved = 0
    for n in (1, 255, 256, 257, 1000):
        for nk in (1, 7, 8, 9, 17):
            pd, ps = n + 37, n + 11
            d, s, g = _random_gather(rng, n, pd, ps)
            src = rng.integers(1, 2**20, ps * nk).astype(np.float64)
            dst0 = np.full(pd * nk, SENT)
            tsrc, tdst = _dev(sf, src), _dev(sf, dst0)
            h = _gather_plan(sf, d, s, g)
            assert sf.lib.fv3_gather_run(sf.ctx, h, _ptr(tdst), pd, _ptr(tsrc), ps, nk, sf.stream_handle) == 0
            hc.sync_device(sf)
            want = dst0.copy()
            for k in range(nk):
                want[d + k * pd] = g * src[s + k * ps]
            got = _host(tdst)
            assert np.array_equal(got, want), (n, nk, np.argwhere(got != want)[:3].tolist())
            assert np.array_equal(_host(tsrc), src)
            assert int((want != SENT).sum()) == n * nk
            moved += n * nk
            # nk = 0: FV3_OK and nothing written
            tdst2 = _dev(sf, dst0)
            assert sf.lib.fv3_gather_run(sf.ctx, h, _ptr(tdst2), pd, _ptr(tsrc), ps, 0, sf.stream_handle) == 0
            hc.sync_device(sf)
            assert np.array_equal(_host(tdst2), dst0)
            assert sf.lib.fv3_gather_plan_destroy(h) == 0
    assert moved == (1 + 255 + 256 + 257 + 1000) * (1 + 7 + 8 + 9 + 17)
    # n = 0: FV3_OK and nothing written
    h = C.c_void_p()
    z, z8 = np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int8)
    assert sf.lib.fv3_gather_plan_create(sf.ctx, C.byref(h), 0, z.ctypes.data_as(C.POINTER(C.c_int64)), z.ctypes.data_as(C.POINTER(C.c_int64)),
                                         z8.ctypes.data_as(C.POINTER(C.c_int8))) == 0
    tdst, tsrc = _dev(sf, np.full(64, SENT)), _dev(sf, np.arange(64.0))
    assert sf.lib.fv3_gather_run(sf.ctx, h, _ptr(tdst), 8, _ptr(tsrc), 8, 8, sf.stream_handle) == 0
    hc.sync_device(sf)
    assert np.array_equal(_host(tdst), np.full(64, SENT))
    assert sf.lib.fv3_gather_plan_destroy(h) == 0


class _PeerCase:
    """One halo plan with one emulated peer: per group a LOCAL copy, two PACKs and two UNPACKs; the message is [group][k][entry]."""

    P, NK, NG, CNT = 300, 9, 2, 40

    def __init__(self, sf, seed=5):
        from pace_amd import lib as L

        self.sf, self.L = sf, L
        rng = np.random.default_rng(seed)
        P, nk, ng, cnt = self.P, self.NK, self.NG, self.CNT
        self.F = [rng.integers(1, 2**20, P * nk).astype(np.float64) for _ in range(ng)]
        self.H0 = [np.full(P * nk, SENT) for _ in range(ng)]
        slots = rng.permutation(cnt)  # message slots, split between the two pack (and the two unpack) plans in interleaved order
        dsts = rng.permutation(P)  # unique destination offsets: the first 60 for the local copy, then 25 + 15 for the unpacks
        sg = lambda m: rng.choice(np.array([-1, 1]), m)  # noqa: E731
        self.local = (dsts[:60], rng.integers(0, P, 60), sg(60))
        self.pack = [(slots[:25], rng.integers(0, P, 25), sg(25)), (slots[25:], rng.integers(0, P, 15), sg(15))]
        uslots = rng.permutation(cnt)
        self.unpack = [(dsts[60:85], uslots[:25], sg(25)), (dsts[85:100], uslots[25:], sg(15))]
        self.elems = ng * nk * cnt
        # numpy restatement
        self.msg = np.zeros(self.elems)
        self.want = [h.copy() for h in self.H0]
        for g in range(ng):
            for d, s, sign in self.pack:
                for k in range(nk):
                    self.msg[g * cnt * nk + k * cnt + d] = sign * self.F[g][s + k * P]
        for g in range(ng):
            d, s, sign = self.local
            for k in range(nk):
                self.want[g][d + k * P] = sign * self.F[g][s + k * P]
            for d, s, sign in self.unpack:
                for k in range(nk):
                    self.want[g][d + k * P] = sign * self.msg[g * cnt * nk + k * cnt + s]
        self.written = ng * nk * (60 + 25 + 15)
        self.tF = [_dev(sf, f) for f in self.F]
        self.tH = [_dev(sf, h) for h in self.H0]
        self.plans = {"local": _gather_plan(sf, *self.local), "pack": [_gather_plan(sf, *p) for p in self.pack], "unpack": [_gather_plan(sf, *p) for p in self.unpack]}
        self.ident = _gather_plan(sf, np.arange(self.elems), np.arange(self.elems), np.ones(self.elems))

    def ops(self, peer=0, null_plan=False):
        L, P, nk, cnt = self.L, self.P, self.NK, self.CNT
        ops = []
        for g in range(self.NG):
            F, H = self.tF[g].data_ptr(), self.tH[g].data_ptr()
            ops.append(L.fv3_halo_op(None if null_plan else self.plans["local"].value, H, F, P, P, 0, 0, -1, L.HALO_LOCAL, nk, 0))
            for h in self.plans["pack"]:
                ops.append(L.fv3_halo_op(h.value, None, F, 0, P, g * cnt * nk, cnt, peer, L.HALO_PACK, nk, 0))
            for h in self.plans["unpack"]:
                ops.append(L.fv3_halo_op(h.value, H, None, P, 0, g * cnt * nk, cnt, peer, L.HALO_UNPACK, nk, 0))
        return ops

    def create(self, send=None, recv=None, **kw):
        L = self.L
        ops = self.ops(**kw)
        ops_a = (L.fv3_halo_op * len(ops))(*ops)
        peers_a = (L.fv3_halo_peer * 1)(L.fv3_halo_peer(1, 0, self.elems, self.elems, send.data_ptr() if send is not None else None,
                                                         recv.data_ptr() if recv is not None else None))
        h = C.c_void_p()
        st = self.sf.lib.fv3_halo_plan_create(self.sf.ctx, C.byref(h), len(ops), ops_a, 1, peers_a)
        return st, h

    def buffers(self, h):
        out = []
        for recv in (0, 1):
            p, n = C.c_void_p(), C.c_int64()
            assert self.sf.lib.fv3_halo_plan_buffer(h, 0, recv, C.byref(p), C.byref(n)) == 0
            assert p.value and n.value == self.elems
            out.append(p)
        return out

    def transport(self, h, calls, fail=False):
        """a host transport that moves the send buffer into the receive buffer (with the library's own gather, on the same stream)"""
        sf = self.sf
        send, recv = self.buffers(h)

        def xfer(_user, plan, phase):
            calls.append((int(plan), int(phase)))
            if fail:
                return 1
            if phase == 0:
                return sf.lib.fv3_gather_run(sf.ctx, self.ident, recv, 0, send, 0, 1, sf.stream_handle)
            return 0

        cb = self.L.fv3_xfer_fn(xfer)
        assert sf.lib.fv3_ctx_set_xfer(sf.ctx, cb, None) == 0
        return cb

    def fields(self):
        hc.sync_device(self.sf)
        return [_host(t) for t in self.tH]


def _fresh(backend, dtype):
    sf, _, _ = hc.factory(backend, dtype, 12, (1, 1), 7, fresh=True)
    if not sf.hostemu:
        assert sf.lib.fv3_ctx_set_comm_stream(sf.ctx, 0) == 0
    return sf


@pytest.mark.parametrize("own_buffers", [False, True], ids=["plan-buffers", "caller-buffers"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
def test_halo_plan_with_one_emulated_peer(backend_both, dtype, own_buffers):
    sf = _fresh(backend_both, dtype)
    pc = _PeerCase(sf)
    send = recv = None
    if own_buffers:
        send, recv = _dev(sf, np.full(pc.elems, SENT)), _dev(sf, np.full(pc.elems, SENT))
    st, h = pc.create(send, recv)
    assert st == 0, sf.lib.fv3_last_error(sf.ctx)
    if own_buffers:
        s, r = pc.buffers(h)
        assert s.value == send.data_ptr() and r.value == recv.data_ptr()
    calls = []
    cb = pc.transport(h, calls)  # noqa: F841  (kept alive)
    # wait() without start(): FV3_OK, nothing written, the transport not called
    assert sf.lib.fv3_halo_plan_wait(sf.ctx, h, sf.stream_handle) == 0
    assert all(np.array_equal(a, b) for a, b in zip(pc.fields(), pc.H0)) and calls == []
    assert sf.lib.fv3_halo_plan_start(sf.ctx, h, sf.stream_handle) == 0
    # start() twice without wait()
    assert sf.lib.fv3_halo_plan_start(sf.ctx, h, sf.stream_handle) != 0
    assert b"start() called twice without wait()" in sf.lib.fv3_last_error(sf.ctx)
    assert sf.lib.fv3_halo_plan_wait(sf.ctx, h, sf.stream_handle) == 0
    assert calls == [(h.value, 0), (h.value, 1)]
    got = pc.fields()
    for g in range(pc.NG):
        assert np.array_equal(got[g], pc.want[g]), (g, np.argwhere(got[g] != pc.want[g])[:3].tolist())
        assert np.array_equal(_host(pc.tF[g]), pc.F[g])
    assert sum(int((w != SENT).sum()) for w in pc.want) == pc.written
    if own_buffers:  # the message itself: [group][k][entry]
        assert np.array_equal(_host(send), pc.msg) and np.array_equal(_host(recv), pc.msg)
    assert sf.lib.fv3_halo_plan_destroy(h) == 0
    sf.lib.fv3_ctx_set_xfer(sf.ctx, pc.L.fv3_xfer_fn(), None)


def test_halo_plan_protocol_and_argument_errors(backend):
    sf = _fresh(backend, torch.float64)
    pc = _PeerCase(sf)
    # refused by fv3_halo_plan_create: a peer index out of range, a null gather plan
    for kw in (dict(peer=1), dict(peer=-1), dict(null_plan=True)):
        st, h = pc.create(**kw)
        assert st != 0 and not h.value
        assert b"bad operation" in sf.lib.fv3_last_error(sf.ctx)
    st, h = pc.create()
    assert st == 0
    # fv3_ctx_set_halo_plans: more plans than the sequencer has updates is refused, as is a count without a list; none is fine
    many = (C.c_void_p * 1000)(*([h.value] * 1000))
    assert sf.lib.fv3_ctx_set_halo_plans(sf.ctx, many, 1000) != 0 and sf.lib.fv3_ctx_set_halo_plans(sf.ctx, None, 1) != 0
    assert sf.lib.fv3_ctx_set_halo_plans(sf.ctx, None, 0) == 0
    # messages, but no transport on this context
    assert sf.lib.fv3_halo_plan_start(sf.ctx, h, sf.stream_handle) != 0
    assert b"no transport" in sf.lib.fv3_last_error(sf.ctx)
    assert sf.lib.fv3_halo_plan_wait(sf.ctx, h, sf.stream_handle) == 0  # (never started)
    # a transport that reports an error
    calls = []
    cb = pc.transport(h, calls, fail=True)  # noqa: F841
    assert sf.lib.fv3_halo_plan_start(sf.ctx, h, sf.stream_handle) != 0
    assert b"host transport reported an error (start)" in sf.lib.fv3_last_error(sf.ctx)
    assert calls == [(h.value, 0)]
    assert sf.lib.fv3_halo_plan_wait(sf.ctx, h, sf.stream_handle) == 0 and calls == [(h.value, 0)]
    hc.sync_device(sf)
    # nothing was unpacked: the fields hold at most the LOCAL copies (which follow the transport, so not even those)
    assert all(np.array_equal(a, b) for a, b in zip(pc.fields(), pc.H0))
    assert sf.lib.fv3_halo_plan_destroy(h) == 0
    sf.lib.fv3_ctx_set_xfer(sf.ctx, pc.L.fv3_xfer_fn(), None)


def test_an_exception_in_the_transport_callback_is_raised_again_by_the_updater(backend):
    """The callback must not let an exception cross the C frame: it returns 1, start() fails, and HaloUpdater raises the callback's exception."""
    from pace_amd.halo import HaloExchanger

    sf, part, lay = hc.factory(backend, torch.float64, 12, (1, 1), 7, world=2, proc=0, fresh=True)
    lay.loopback = True  # one process playing 1 of 2 alone: the library's plans over a host transport that loops the messages back
    ex = HaloExchanger(sf, lay)
    assert ex.transport == "loopback"
    up = ex.updater("cell", [(sf.quantity_factory.zeros(("x", "y", "z")),)])
    up.update()
    ex._by_plan.clear()  # the callback's look-up of its updater now raises KeyError inside the C call
    with pytest.raises(KeyError):
        up.start()
    assert b"host transport reported an error (start)" in sf.lib.fv3_last_error(sf.ctx)


# ---------------------------------------------------------------------------------------------------------------------------
# 6  more sub-domains than a context holds
# ---------------------------------------------------------------------------------------------------------------------------
def test_more_sub_domains_than_a_context_holds_is_a_value_error(hostemu):
    with pytest.raises(ValueError, match=r"54 sub-domains.*FV3_MAX_SUB = 32.*more processes"):
        hc.factory("hostemu", torch.float64, 12, (3, 3), 7, world=1, proc=0, fresh=True)
