"""Tracer advection (fv3_tracer_2d_1l) and the vertical remap (fv3_remap) against the oracle on the inputs a real run gives them,
and on the edge cases their limiters exist for -- where the smooth, strictly positive tracers of test_tracer_advection.py /
test_remap.py never go:

* the Fortran model's C12 L63 restart (tests/golden/c12_restart_6tiles.npz): specific humidity from 1e-7 to 1.8e-2, cloud water
  that is exactly 0 in half the cells and -5e-20 in a fifth, temperatures down to 182 K (below the remap's 184 K floor of T_v);
* fronts, a blob on exact zeros, a field spanning 1e-12 .. 1e-7 and 2-dx spikes through tile edges and cube corners, on
  130-cell sub-domains (several march strips; forced short march segments), a non-square layout and 8 levels;
* hand-built Lagrangian columns: target layers covering 3 or more source layers next to source layers 1e-3 as thick as their
  neighbours, tracer layers with zero / negative means, a cold T_v minimum, winds that change sign, 12 and 79 levels;
* the fp32 build of both operators against the fp64 oracle.

Every case also asserts, through the oracle's opt-in branch counters (fv3_oracle.ppm / fv3_oracle.remap), that the limiter
branches it exists for were taken."""
import copy
import os

import numpy as np
import pytest
import torch

from helpers import Case, oracle_cube
from pace_amd.constants import get_constants
from pace_amd._testing import stencil_factory_for
from pace_amd.halo import Layout
from pace_amd.stencils import FiniteVolumeTransport, LagrangianToEulerian, TracerAdvection

from fv3_oracle import ppm as o_ppm
from fv3_oracle import remap as o_remap
from fv3_oracle import tracer_2d_1l as o_t2
from fv3_oracle.dyn_core import OracleAcousticDynamics
from test_restart_six_tiles import GOLDEN, _restart_cube

NH = 3

# fp32 build against the fp64 oracle, field-scale relative (each tracer against its own maximum).  Every bound is 2 x the worst
# error measured over the cases of this file on the host emulation and on the MI355X (tracer advection: the same to the digits
# shown on both).
# Tracer advection, per hord (tracers / dp1, mfxd, mfyd, cxd):
#   hord 8: 4.5e-7 on the synthetic fields, 3.0e-6 on the real-state front / 1.6e-7 -- pert_ppm's flattening at the tile edges
#   (bl br < 0 or not) is the one switch of the monotone scheme that a front can sit on.
#   hord 6: 1.5e-3, hord 5: 4.4e-3 (2.5e-6 and 3.2e-4 on the real moisture) -- the smt5 switch of the unlimited schemes is not
#   continuous: next to a 0 / 1 front or a spike a cell whose |bl - br| and 3 |bl + br| (hord 6) or bl br and 0 (hord 5) agree to
#   fp32 round-off takes the other branch than in fp64, and its flux moves by O(the jump).  Smooth fields stay at round-off.
# Remap (host emulation / MI355X where they differ: the device's fp32 log / exp and its fused multiply-adds):
#   real state: delp 4.3e-6 (an Eulerian layer is the difference of two fp32 interface pressures ~1e5 Pa), tracers 1.0e-5,
#   u 1.4e-6, v 1.1e-6, pkz 3.7e-7 / 9.8e-7, pk 3.8e-7 / 7.3e-7, pt 2.4e-7 / 3.1e-7, peln 5.4e-8 / 1.6e-7, the rest <= 3.2e-7.
#   hand-built columns: source layers 1e-3 as thick as their neighbours (~1 Pa at ~1e5 Pa) are held by fp32 interface pressures
#   to ~6e-3 Pa and by fp32 log-pressures to ~1e-6, so their thickness is known to a few per cent, and the edge-value system
#   (thickness ratios of 1e3 in its coefficients) carries that into the neighbouring parabolas: pt (remapped in log p)
#   1.2e-2 / 4.0e-2, pkz 4.1e-3 / 2.6e-2, delz 3.6e-2, tracers 3.2e-4, u / v 1.7e-5, w 1.6e-5, delp 7.2e-6, peln 5.1e-8 / 1.6e-7,
#   pe / pk / ps <= 7e-7.
TOL32_TRACER = {8: 6e-6, 6: 3e-3, 5: 9e-3, "fluxes": 3.2e-7}
TOL32_REMAP = {
    "real": {"delp": 9e-6, "pt": 6.2e-7, "delz": 6.4e-7, "w": 3.4e-7, "pe": 2.6e-7, "peln": 3.2e-7, "pk": 1.5e-6, "pkz": 2e-6, "u": 2.8e-6, "v": 2.2e-6,
             "tracer": 2e-5, "ps": 7.6e-8},
    "hand": {"delp": 1.5e-5, "pt": 8e-2, "delz": 7.2e-2, "w": 3.2e-5, "pe": 2.6e-7, "peln": 3.2e-7, "pk": 1.4e-6, "pkz": 5.2e-2, "u": 3.4e-5, "v": 2.8e-5,
             "tracer": 6.4e-4, "ps": 7.6e-8},
}


@pytest.fixture(params=["hostemu", pytest.param("hip:gfx950", marks=pytest.mark.gpu)])
def backend32(request):
    """The fp32 library: its host emulation (CPU suite) or the HIP build (-m gpu)."""
    from pace_amd import build, lib

    if request.param == "hostemu":
        build.build(32, hostemu=True, verbose=False)
    else:
        request.getfixturevalue("gpu_backend")
        if not os.path.exists(build.lib_path(32)):
            build.build(32)
        lib.load(32)
    return request.param


@pytest.fixture(scope="module")
def data():
    return np.load(GOLDEN)


@pytest.fixture
def ppm_counts():
    o_ppm.enable_counters(True)
    yield o_ppm
    o_ppm.enable_counters(False)


@pytest.fixture
def remap_counts():
    o_remap.enable_counters(True)
    o_remap.reset_counters()
    yield o_remap
    o_remap.enable_counters(False)


def _sync(backend):
    if backend != "hostemu":
        torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------
_REAL = {}


def _real_lagrangian(data, layout):
    """The six restart tiles after one oracle acoustic call (2 sub-steps of 60 s): (c, part, cfg, grids, odyn, dp1 before the
    call, state after it, wsd of the last sub-step).  Cached per layout; callers get copies."""
    if layout not in _REAL:
        c, part, cfg, grids, states, phis = _restart_cube(data, layout)
        odyn = OracleAcousticDynamics(part, grids, cfg, c, phis)
        ost = [{k: v.copy() for k, v in s.items()} for s in states]
        dp1 = [s["delp"].copy() for s in ost]
        odyn(ost, 60.0, 1)
        wsd = [t["wsd"].copy() for t in odyn.tmp]
        _REAL[layout] = (c, part, cfg, grids, odyn, dp1, ost, wsd)
    c, part, cfg, grids, odyn, dp1, ost, wsd = _REAL[layout]
    cp = lambda L: [a.copy() for a in L]  # noqa: E731
    return c, part, cfg, grids, odyn, cp(dp1), [{k: v.copy() for k, v in s.items()} for s in ost], cp(wsd)


def _restart_cells(data, name, part, r, nz):
    """[i, j, k] compute cells of rank r from the restart's [tile][k, y, x]"""
    ox, oy = part.origin(r)
    return np.transpose(np.asarray(data[name][part.tile_index(r)], dtype=np.float64), (2, 1, 0))[ox : ox + part.nx, oy : oy + part.ny, :nz]


def _with_halo(a, nz):
    """compute cells -> (nx + 2 nh + 1, ny + 2 nh + 1, nz) with edge-replicated halos (the halo update replaces them)"""
    return np.ascontiguousarray(np.pad(a[:, :, :nz], ((NH, NH + 1), (NH, NH + 1), (0, 0)), mode="edge"))


def _front(g, nz):
    """a 0 / 1 front on the sphere (a wavy line of latitude, tilted with height): it crosses tile edges at arbitrary angles"""
    lon, lat = g.fields["lon_agrid"], g.fields["lat_agrid"]
    k = np.arange(nz)[None, None, :]
    return np.where(lat[:, :, None] > 0.35 * np.sin(2.0 * lon[:, :, None] + 0.05 * k) - 0.2, 1.0, 0.0)


def _real_tracers(data, part, grids, odyn, nz):
    tr = []
    for r, g in enumerate(grids):
        tr.append({"sphum": _with_halo(_restart_cells(data, "sphum", part, r, nz), nz), "liq_wat": _with_halo(_restart_cells(data, "liq_wat", part, r, nz), nz),
                   "front": np.ascontiguousarray(_front(g, nz))})
    for name in tr[0]:
        odyn.ex.scalar([t[name] for t in tr])
    return tr


def _synthetic_tracers(part, odyn, nz):
    """Per rank, in tile-index space (so every tile carries the same pattern and each front meets the tile edges, the corners included):
    front_diag: 0 / 1 across the diagonal i = j, through the SW and NE cube corners; blob: a cos^2 bump on exact zeros;
    front_we: 0 / 1 across a line of constant j (meets the W and E edges); tiny: 1e-12 .. 1e-7; front_sn: 0 / 1 across a line
    of constant i (meets the S and N edges); spikes: 2-dx spikes on a background; one: a constant (the unpaired slot).  Paired
    as (front_diag, blob), (front_we, tiny), (front_sn, spikes): the two slots of a Q4_TRC wave differ."""
    n = part.nx_tile
    tr = []
    for r in range(part.total_ranks):
        ox, oy = part.origin(r)
        i = (np.arange(part.nx + 2 * NH + 1) - NH + ox + 0.5)[:, None, None]
        j = (np.arange(part.ny + 2 * NH + 1) - NH + oy + 0.5)[None, :, None]
        k = np.arange(nz)[None, None, :]
        shp = (part.nx + 2 * NH + 1, part.ny + 2 * NH + 1, nz)
        rho = np.sqrt(((i - 0.3 * n) / (0.18 * n)) ** 2 + ((j - 0.62 * n) / (0.22 * n)) ** 2 + 0.0 * k)
        d = {
            "front_diag": np.broadcast_to(np.where(i > j + 0.3 * (k - nz / 2), 1.0, 0.0), shp),
            "blob": np.broadcast_to(np.where(rho < 1.0, np.cos(0.5 * np.pi * np.minimum(rho, 1.0)) ** 2, 0.0) * (1.0 + 0.1 * k), shp),
            "front_we": np.broadcast_to(np.where(j < 0.41 * n + k, 0.8, 0.05), shp),
            "tiny": np.broadcast_to(10.0 ** (-12.0 + 5.0 * (0.5 + 0.5 * np.sin(2 * np.pi * i / n) * np.cos(2 * np.pi * (j + k) / n))), shp),
            "front_sn": np.broadcast_to(np.where(i < 0.57 * n - k, 0.0, 2.0), shp),
            "spikes": np.broadcast_to(1.0 + np.where((np.floor(i) % 2 == 0) & (np.abs(j - 0.5 * n) < 0.3 * n), 3.0, 0.0) + 0.01 * k, shp),
            "one": np.full(shp, 0.75),
        }
        tr.append({kk: np.array(v, dtype=np.float64) for kk, v in d.items()})  # (writable copies)
    for name in tr[0]:
        odyn.ex.scalar([t[name] for t in tr])
    return tr


def _fluxes(odyn, dp1, ost, nz, want_split):
    """the advection's inputs from an acoustic call: dp1 = the air mass before it, the accumulated mass fluxes / Courant numbers
    after it; the Courant numbers scaled (as test_tracer_advection._inputs does) so that the operator needs ``want_split`` sub-cycles"""
    V = lambda a: a[:, :, :nz].copy()  # noqa: E731
    base = max(max(np.abs(V(s["cxd"])[D.sl(1, D.nx, 1, D.ny)]).max(), np.abs(V(s["cyd"])[D.sl(1, D.nx, 1, D.ny)]).max()) for D, s in zip(odyn.doms, ost))
    scale = 1.0 if want_split == 1 else (want_split - 0.6) / base
    F = dict(dp1=[V(a) for a in dp1], mfx=[V(s["mfxd"]) for s in ost], mfy=[V(s["mfyd"]) for s in ost], cx=[V(s["cxd"]) * scale for s in ost],
             cy=[V(s["cyd"]) * scale for s in ost])
    odyn.ex.scalar(F["dp1"])
    return F


def _synthetic_lagrangian(n, layout, nz, dt=150.0):
    part, cfg, grids, ost, phis, odyn = oracle_cube(n, layout, nz, dict(n_split=2))
    dp1 = [s["delp"].copy() for s in ost]
    odyn(ost, dt, 1)
    return part, cfg, grids, odyn, dp1, ost


# ---------------------------------------------------------------------------------------------------------------------------
# tracer advection
# ---------------------------------------------------------------------------------------------------------------------------
def _advect(backend, part, cfg, grids, odyn, tr, F, hord, dtype=torch.float64):
    """library and oracle from the same inputs; returns (n_split, device tracers, device inputs); tr / F hold the oracle's results"""
    sf = stencil_factory_for(backend)(grids, cfg, get_constants(), dtype=dtype)
    qf = sf.quantity_factory
    pad = lambda a: np.concatenate([a, a[:, :, -1:]], axis=2)  # noqa: E731
    Q = {k: qf.from_array([pad(a) for a in v], ("x", "y", "z")) for k, v in F.items()}
    T = {name: qf.from_array([pad(t_[name]) for t_ in tr], ("x", "y", "z")) for name in tr[0]}
    op = TracerAdvection(sf, qf, FiniteVolumeTransport(sf, qf, grids, hord=hord), grids, Layout(part, 1, 0), T)
    op(T, Q["dp1"], Q["mfx"], Q["mfy"], Q["cx"], Q["cy"])
    _sync(backend)
    o_ppm.reset_counters()
    ns = o_t2.tracer_2d_1l(odyn.doms, tr, F["dp1"], F["mfx"], F["mfy"], F["cx"], F["cy"], hord, halo_update=lambda fs: odyn.ex.scalar(fs))
    return op.n_split, ns, T, Q


def _tracer_errors(odyn, tr, F, T, Q, nz):
    """worst field-scale relative error per tracer (each against its own maximum) and of dp1 / mfxd / cxd, over the ranks"""
    worst = {}
    for r, D in enumerate(odyn.doms):
        C = D.sl(1, D.nx, 1, D.ny)
        pairs = [(name, T[name].numpy(r)[:, :, :nz][C], tr[r][name][C]) for name in tr[0]]
        pairs += [("dp1", Q["dp1"].numpy(r)[:, :, :nz][C], F["dp1"][r][C]),
                  ("mfxd", Q["mfx"].numpy(r)[:, :, :nz][D.sl(1, D.nx + 1, 1, D.ny)], F["mfx"][r][D.sl(1, D.nx + 1, 1, D.ny)]),
                  ("mfyd", Q["mfy"].numpy(r)[:, :, :nz][D.sl(1, D.nx, 1, D.ny + 1)], F["mfy"][r][D.sl(1, D.nx, 1, D.ny + 1)]),
                  ("cxd", Q["cx"].numpy(r)[:, :, :nz][D.sl(1, D.nx + 1, D.jsd, D.jed)], F["cx"][r][D.sl(1, D.nx + 1, D.jsd, D.jed)])]
        for name, got, want in pairs:
            got = got.astype(np.float64)
            assert np.all(np.isfinite(got)), f"{name} rank {r}: non-finite"
            assert np.all(np.isfinite(want)), f"{name} rank {r}: the oracle is not finite"
            sc = np.abs(want).max()
            worst[name] = max(worst.get(name, 0.0), float(np.abs(got - want).max() / sc) if sc > 0 else float(np.abs(got).max()))
    return worst


FP64_TRACER_TOL = {"dp1": 1e-14, "mfxd": 1e-14, "mfyd": 1e-14, "cxd": 1e-14}


def _assert_fp64(worst):
    bad = {k: v for k, v in worst.items() if v > FP64_TRACER_TOL.get(k, 1e-13)}
    assert not bad, f"field-scale relative errors above tolerance: {bad} (all: {worst})"


def _assert_ppm_branches(hord, pert_both=False):
    n = o_ppm.counters()
    if hord == 8:
        need = ["ppm8_dm_clamped", "ppm8_edge_clamped", "ppm8_bl_clamped", "ppm8_br_clamped", "pert_ppm_flat"] + (["pert_ppm_lo", "pert_ppm_hi"] if pert_both else [])
    else:
        need = [f"smt5_true_hord{hord}", f"smt5_false_hord{hord}"]
    missing = [k for k in need if n[k] == 0]
    assert not missing, f"hord {hord}: branches never taken: {missing} ({n})"


@pytest.mark.parametrize("layout", [(1, 1), (2, 2)])
@pytest.mark.parametrize("want_split", [1, 3])
@pytest.mark.parametrize("hord", [5, 6, 8])
def test_tracer_advection_of_the_real_moisture_matches_the_oracle(backend, data, ppm_counts, hord, want_split, layout):
    """sphum, liq_wat and a 0 / 1 front (3 tracers: one pair + the unpaired slot) on the six restart tiles, advected with the
    fluxes of one acoustic call of the real state; (2, 2) puts the halo update between the sub-cycles inside tile edges."""
    nz = 63
    c, part, cfg, grids, odyn, dp1, ost, _ = _real_lagrangian(data, layout)
    tr = _real_tracers(data, part, grids, odyn, nz)
    F = _fluxes(odyn, dp1, ost, nz, want_split)
    got_split, ns, T, Q = _advect(backend, part, cfg, grids, odyn, tr, F, hord)
    assert got_split == ns == want_split
    _assert_fp64(_tracer_errors(odyn, tr, F, T, Q, nz))
    _assert_ppm_branches(hord)


# the synthetic shapes: (tile size, layout, levels, FV3_SEG, sub-cycles)
SHAPES = {
    "130": (130, (1, 1), 4, None, 2),            # 130-cell sub-domains: several march strips per row
    "130_seg32": (130, (1, 1), 4, "32", 1),      # ... with 32-row march segments: one wave runs several segments
    "nonsquare": (24, (2, 1), 4, None, 3),       # 12 x 24 sub-domains
    "nz8": (24, (1, 1), 8, None, 2),
}
_SYN = {}


def _synthetic_case(shape):
    n, layout, nz, seg, want_split = SHAPES[shape]
    key = (n, layout, nz)
    if key not in _SYN:
        _SYN[key] = _synthetic_lagrangian(n, layout, nz)
    part, cfg, grids, odyn, dp1, ost = _SYN[key]
    tr = _synthetic_tracers(part, odyn, nz)
    F = _fluxes(odyn, [a.copy() for a in dp1], ost, nz, want_split)
    return part, cfg, grids, odyn, tr, F, nz, seg, want_split


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("hord", [5, 6, 8])
def test_tracer_advection_of_fronts_zeros_and_spikes_matches_the_oracle(backend, ppm_counts, monkeypatch, shape, hord):
    part, cfg, grids, odyn, tr, F, nz, seg, want_split = _synthetic_case(shape)
    if seg:
        monkeypatch.setenv("FV3_SEG", seg)
    got_split, ns, T, Q = _advect(backend, part, cfg, grids, odyn, tr, F, hord)
    assert got_split == ns == want_split
    _assert_fp64(_tracer_errors(odyn, tr, F, T, Q, nz))
    _assert_ppm_branches(hord, pert_both=True)
    # the constant stays constant, the blob on exact zeros does not go negative (hord 8 is monotone)
    for r, D in enumerate(odyn.doms):
        C = D.sl(1, D.nx, 1, D.ny)
        assert np.abs(T["one"].numpy(r)[:, :, :nz][C] - 0.75).max() < 1e-14
        if hord == 8:
            assert T["blob"].numpy(r)[:, :, :nz][C].min() >= 0.0


@pytest.mark.parametrize("case", ["real", "130", "nonsquare"])
@pytest.mark.parametrize("hord", [5, 6, 8])
def test_fp32_tracer_advection_tracks_the_fp64_oracle(backend32, data, case, hord):
    """the fp32 library on the inputs above, against the fp64 oracle: finite, a constant kept to fp32 round-off, field-scale bounds TOL32_TRACER"""
    if case == "real":
        nz = 63
        c, part, cfg, grids, odyn, dp1, ost, _ = _real_lagrangian(data, (2, 2))
        tr = _real_tracers(data, part, grids, odyn, nz)
        for t_ in tr:
            t_["one"] = np.full_like(t_["sphum"], 0.75)
        F = _fluxes(odyn, dp1, ost, nz, 3)
    else:
        part, cfg, grids, odyn, tr, F, nz, _, _ = _synthetic_case(case)
    cfg = copy.copy(cfg)
    cfg.nord = 1  # (the fp32 context refuses the default del-6 damping tables at these resolutions; the advection reads none)
    got_split, ns, T, Q = _advect(backend32, part, cfg, grids, odyn, tr, F, hord, dtype=torch.float32)
    assert got_split == ns
    worst = _tracer_errors(odyn, tr, F, T, Q, nz)
    print(f"fp32 tracer advection, {case}, hord {hord}:", {k: f"{v:.1e}" for k, v in worst.items()})
    for r, D in enumerate(odyn.doms):
        C = D.sl(1, D.nx, 1, D.ny)
        assert np.abs(T["one"].numpy(r)[:, :, :nz][C].astype(np.float64) - 0.75).max() < 4 * 0.75 * np.finfo(np.float32).eps
    for k, v in worst.items():
        assert v < TOL32_TRACER["fluxes" if k in ("dp1", "mfxd", "mfyd", "cxd") else hord], (k, v, worst)


# ---------------------------------------------------------------------------------------------------------------------------
# vertical remap
# ---------------------------------------------------------------------------------------------------------------------------
REMAP_TOL = {"delp": 1e-13, "pt": 1e-12, "delz": 1e-12, "w": 1e-11, "pe": 1e-14, "peln": 1e-14, "pk": 1e-13, "pkz": 1e-12, "u": 1e-12, "v": 1e-12, "tracer": 1e-12, "ps": 1e-14}
NAMES = ("pt", "delp", "delz", "peln", "pe", "pk", "pkz", "u", "v", "w", "cappa")


def _remap(backend, grids, cfg, ost, wsd, tr, doms, dtype=torch.float64):
    """library and oracle on the same Lagrangian state (ost / tr are remapped in place by the oracle); returns the library's
    quantities, tracers, ps and the oracle's ps, plus the column masses before the remap"""
    c = get_constants()
    sf = stencil_factory_for(backend)(grids, cfg, c, dtype=dtype)
    qf = sf.quantity_factory
    Q = {k: qf.from_array([s[k] for s in ost], ("x", "y", "z")) for k in NAMES}
    T = {f"q{t}": qf.from_array([tr[r][t] for r in range(len(ost))], ("x", "y", "z")) for t in range(len(tr[0]))}
    ps = qf.zeros(("x", "y"))
    W = qf.from_array([np.asarray(w_).reshape(w_.shape[0], w_.shape[1]) for w_ in wsd], ("x", "y"))
    m0 = []
    for r, D in enumerate(doms):
        C = D.sl(1, D.nx, 1, D.ny)
        dp = ost[r]["delp"][C][:, :, : D.grid.nz]
        m0.append((dp.sum(axis=2), [(tr[r][t][C][:, :, : D.grid.nz] * dp).sum(axis=2) for t in range(len(tr[r]))]))
    LagrangianToEulerian(sf, qf, grids)(T, *[Q[k] for k in NAMES], ps, W)
    _sync(backend)
    o_ps = [o_remap.lagrangian_to_eulerian(D, c, ost[r], wsd[r], tr[r]) for r, D in enumerate(doms)]
    return Q, T, ps, o_ps, m0


def _remap_errors(Q, T, ps, o_ps, ost, tr, doms):
    worst = {}

    def put(k, got, want):
        got = got.astype(np.float64)
        assert np.all(np.isfinite(got)), f"{k}: non-finite"
        sc = np.abs(want).max()
        worst[k] = max(worst.get(k, 0.0), float(np.abs(got - want).max() / sc) if sc > 0 else float(np.abs(got).max()))

    for r, D in enumerate(doms):
        nz = D.grid.nz
        C = D.sl(1, D.nx, 1, D.ny)
        for k in ("delp", "pt", "delz", "w", "pe", "peln", "pk", "pkz"):
            kk = nz + 1 if k in ("pe", "peln", "pk") else nz
            put(k, Q[k].numpy(r)[C][:, :, :kk], ost[r][k][C][:, :, :kk])
        put("u", Q["u"].numpy(r)[D.sl(1, D.nx, 1, D.ny + 1)][:, :, :nz], ost[r]["u"][D.sl(1, D.nx, 1, D.ny + 1)][:, :, :nz])
        put("v", Q["v"].numpy(r)[D.sl(1, D.nx + 1, 1, D.ny)][:, :, :nz], ost[r]["v"][D.sl(1, D.nx + 1, 1, D.ny)][:, :, :nz])
        for t in range(len(tr[r])):
            put(f"tracer{t}", T[f"q{t}"].numpy(r)[C][:, :, :nz], tr[r][t][C][:, :, :nz])
        put("ps", ps.numpy(r)[C], o_ps[r][C])
    return worst


def _remap_properties(Q, T, tr, m0, doms, grids, rtol, positive=()):
    """column air mass and tracer mass conserved, levels back on ak + bk ps, positive-definite tracers >= 0 where the oracle's are"""
    for r, D in enumerate(doms):
        nz = D.grid.nz
        C = D.sl(1, D.nx, 1, D.ny)
        dp = Q["delp"].numpy(r)[C][:, :, :nz].astype(np.float64)
        mass0, tm0 = m0[r]
        assert np.abs(dp.sum(axis=2) - mass0).max() <= rtol * mass0.max()
        for t in range(len(tr[r])):
            q = T[f"q{t}"].numpy(r)[C][:, :, :nz].astype(np.float64)
            tm1 = (q * dp).sum(axis=2)
            assert np.abs(tm1 - tm0[t]).max() <= rtol * max(np.abs(tm0[t]).max(), np.abs(tr[r][t][C][:, :, :nz] * dp).sum(axis=2).max()), f"tracer {t} mass, rank {r}"
            if t in positive:
                want = tr[r][t][C][:, :, :nz]
                assert q[want >= 0.0].min(initial=0.0) >= 0.0, f"tracer {t}: negative where the oracle is >= 0"
        pe = Q["pe"].numpy(r)[C][:, :, : nz + 1].astype(np.float64)
        g = grids[r]
        want = g.ak[None, None, :] + g.bk[None, None, :] * pe[:, :, -1:]
        assert np.abs(pe[:, :, 1:-1] - want[:, :, 1:-1]).max() <= rtol * pe.max()


def _real_remap_inputs(data, layout):
    nz = 63
    c, part, cfg, grids, odyn, _, ost, wsd = _real_lagrangian(data, layout)
    rng = np.random.default_rng(11)
    wsd = [w_ + 1e-3 * (rng.random(w_.shape) - 0.5) for w_ in wsd]
    assert max(np.abs(w_).max() for w_ in wsd) > 1e-4
    tr = []
    for r, g in enumerate(grids):
        front = np.zeros_like(ost[r]["delp"])
        front[:, :, :nz] = _front(g, nz) * 1e-3
        q = []
        for name in ("sphum", "liq_wat"):
            a = np.zeros_like(ost[r]["delp"])
            a[:, :, :nz] = _with_halo(_restart_cells(data, name, part, r, nz), nz)
            q.append(a)
        tr.append(q + [np.ascontiguousarray(front)])
    return cfg, grids, odyn.doms, ost, wsd, tr


def _tv(s, rrg):
    """the T_v the remap integrates (pt is T_v / pkz of the full pressure)"""
    pt, cp = s["pt"], s["cappa"]
    with np.errstate(all="ignore"):
        return pt * np.exp(cp / (1.0 - cp) * np.log(rrg * s["delp"] / s["delz"] * pt))


@pytest.mark.parametrize("layout", [(1, 1), (2, 2)])
def test_remap_of_the_real_state_matches_the_oracle(backend, data, remap_counts, layout):
    """the restart's T (T_v below the 184 K floor), sphum / liq_wat (zeros, -5e-20) and a 0 / 1 front, after one acoustic call of the
    real state with its terrain; wsd nonzero"""
    cfg, grids, doms, ost, wsd, tr = _real_remap_inputs(data, layout)
    rrg = -get_constants().RDGAS / get_constants().GRAV
    tv = min(float(_tv(s, rrg)[D.sl(1, D.nx, 1, D.ny)][:, :, :63].min()) for s, D in zip(ost, doms))
    assert tv < 184.0, tv  # the remapped temperature T_v reaches below the floor of its flattening
    for s in ost:
        s["pkz"][...] = 1.0
    Q, T, ps, o_ps, m0 = _remap(backend, grids, cfg, ost, wsd, tr, doms)
    worst = _remap_errors(Q, T, ps, o_ps, ost, tr, doms)
    bad = {k: v for k, v in worst.items() if v > REMAP_TOL["tracer" if k.startswith("tracer") else k]}
    assert not bad, f"field-scale relative errors above tolerance: {bad} (all: {worst})"
    _remap_properties(Q, T, tr, m0, doms, grids, 1e-12, positive=(0, 2))
    n = o_remap.counters()
    for k in ("iv0_nonpos", "iv12_flat", "iv12_a6da_lo", "iv12_a6da_hi", "constrain_iv0", "flat_2dz", "flat_qmin"):
        assert n[k] > 0, f"the real state did not reach {k}: {n}"


def _hand_built_columns(nz, seed=3):
    """One rank of C12 with every column (halos included) a hand-built Lagrangian column: pe(0) = ptop, pe(km) = ps,
    pe = ptop + running sum of delp, peln = log pe, pk = pe^kappa; source layers 1e-3 as thick as their neighbours every few
    levels (so target layers cover 3 or more of them); T_v with a V-shaped 181 K minimum in the interior (below the 184 K floor
    of the remap's flattening; monotone either side, so only the floor flattens it); delz hydrostatic for that T_v; u / v changing sign with height and
    across the columns; tracers: a linear ramp through an exactly-zero layer (zero mean between a negative and a positive
    neighbour), a humidity-like profile, cloud-water-like layers of 0 / -5e-20 / 1e-4, a sharp front, a constant."""
    c = get_constants()
    case = Case(12, (1, 1), (0,), nz=nz)
    g = case.grids[0]
    ni, nj = case.shape[:2]
    rng = np.random.default_rng(seed)
    st = {k: np.zeros((ni, nj, nz + 1)) for k in NAMES}
    tr = [np.zeros((ni, nj, nz + 1)) for _ in range(5)]
    wsd = np.zeros((ni, nj, 1))
    k = np.arange(nz)
    for i in range(ni):
        for j in range(nj):
            ps = 1.0e5 + 3000.0 * np.sin(0.7 * i + 0.3 * j)
            dpe = np.diff(g.ak + g.bk * ps)
            wgt = 1.0 + 0.35 * np.sin(1.3 * k + 0.9 * i - 0.4 * j) + 0.1 * rng.random(nz)
            thin = (k % 5 == (i + 2 * j) % 5) & (k > 0) & (k < nz - 1)
            wgt = np.where(thin, 1e-3, wgt)
            dp = dpe * wgt
            dp *= (ps - g.ptop) / dp.sum()
            pe = np.concatenate([[g.ptop], g.ptop + np.cumsum(dp)])
            pe[-1] = ps
            dp = np.diff(pe)
            pm = 0.5 * (pe[1:] + pe[:-1])
            kmin = 2 + (i + j) % (nz - 4)
            tv = 181.0 + 20.0 * np.sqrt(np.abs(k - kmin)) + 0.5 * np.sin(0.3 * i + 0.2 * j)  # (monotone either side of kmin)
            cp = c.KAPPA * (1.0 - 0.02 * np.sin(k + i))
            st["delp"][i, j, :nz] = dp
            st["pe"][i, j, :] = pe
            st["peln"][i, j, :] = np.log(pe)
            st["pk"][i, j, :] = pe ** c.KAPPA
            st["delz"][i, j, :nz] = -c.RDGAS / c.GRAV * dp * tv / pm
            st["cappa"][i, j, :nz] = cp
            st["pt"][i, j, :nz] = tv / pm ** cp
            st["pkz"][i, j, :nz] = 1.0
            st["u"][i, j, :nz] = 25.0 * np.sin(0.5 * k + 0.4 * i - 0.2 * j) + 3.0
            st["v"][i, j, :nz] = -18.0 * np.cos(0.45 * k - 0.3 * i + 0.5 * j)
            st["w"][i, j, :nz] = 0.3 * np.sin(0.8 * k + i) + 0.05 * rng.random(nz)
            wsd[i, j, 0] = 0.02 * np.cos(i - j)
            k0 = 2 + (2 * i + j) % (nz - 4)
            tr[0][i, j, :nz] = 2e-5 * (k - k0)                                   # ... -2e-5, 0, +2e-5 ...: a zero mean inside a ramp
            tr[1][i, j, :nz] = 1.8e-2 * np.exp(-8.0 * (1.0 - pm / ps)) + 1e-7      # sphum-like
            tr[2][i, j, :nz] = np.where((k + i + j) % 4 == 0, 1e-4 * (1 + rng.random(nz)), np.where((k + i) % 3 == 0, -5e-20, 0.0))
            tr[3][i, j, :nz] = np.where(k > (i + j) % nz, 1e-3, 0.0)
            tr[4][i, j, :nz] = 0.75
    return case, st, tr, wsd


@pytest.mark.parametrize("nz", [12, 79])
def test_remap_of_hand_built_columns_matches_the_oracle(backend, remap_counts, nz):
    """thin source layers, a cold T_v minimum, zero / negative tracer means, sign-changing winds: every limiter branch the remap has"""
    case, st, tr, wsd = _hand_built_columns(nz)
    Q, T, ps, o_ps, m0 = _remap(backend, case.grids, case.cfg, [st], [wsd], [tr], case.doms)
    worst = _remap_errors(Q, T, ps, o_ps, [st], [tr], case.doms)
    bad = {k: v for k, v in worst.items() if v > REMAP_TOL["tracer" if k.startswith("tracer") else k]}
    assert not bad, f"field-scale relative errors above tolerance: {bad} (all: {worst})"
    _remap_properties(Q, T, [tr], m0, case.doms, case.grids, 1e-12, positive=(1, 3, 4))
    C = case.doms[0].sl(1, 12, 1, 12)
    assert np.abs(T["q4"].numpy(0)[C][:, :, :nz] - 0.75).max() < 1e-14
    n = o_remap.counters()
    missing = [k for k in ("iv0_nonpos", "iv12_flat", "iv12_a6da_lo", "iv12_a6da_hi", "constrain_iv0", "top_ivm1", "bot_ivm1", "flat_2dz", "flat_qmin", "span3")
               if n[k] == 0]
    assert not missing, f"branches never taken: {missing} ({n})"


@pytest.mark.parametrize("case", ["real", "hand12", "hand79"])
def test_fp32_remap_tracks_the_fp64_oracle(backend32, data, case):
    """the fp32 library against the fp64 oracle: finite, positive-definite tracers >= 0, a constant kept to fp32 round-off,
    field-scale bounds TOL32_REMAP"""
    if case == "real":
        cfg, grids, doms, ost, wsd, tr = _real_remap_inputs(data, (2, 2))
        for r in range(len(ost)):
            ost[r]["pkz"][...] = 1.0
            tr[r].append(np.full_like(tr[r][0], 0.75))
        positive, one = (0, 1, 2), 3
    else:
        c_, st, trh, w_ = _hand_built_columns(int(case[4:]))
        cfg, grids, doms, ost, wsd, tr = c_.cfg, c_.grids, c_.doms, [st], [w_], [trh]
        positive, one = (0, 1, 2, 3), 4
    cfg = copy.copy(cfg)
    cfg.nord = 1
    inputs = [[a.copy() for a in t_] for t_ in tr]
    Q, T, ps, o_ps, m0 = _remap(backend32, grids, cfg, ost, wsd, tr, doms, dtype=torch.float32)
    worst = _remap_errors(Q, T, ps, o_ps, ost, tr, doms)
    print(f"fp32 remap, {case}:", {k: f"{v:.1e}" for k, v in worst.items()})
    for r, D in enumerate(doms):
        C = D.sl(1, D.nx, 1, D.ny)
        nz = D.grid.nz
        for t in positive:
            # >= 0 where the oracle is; a tracer that enters with negative layer means (cloud water's -5e-20) is held to that floor
            q = T[f"q{t}"].numpy(r)[C][:, :, :nz]
            floor = min(0.0, float(inputs[r][t][C][:, :, :nz].min()))
            assert q[tr[r][t][C][:, :, :nz] >= 0.0].min(initial=0.0) >= floor, f"tracer {t}: negative where the oracle is >= 0"
        assert np.abs(T[f"q{one}"].numpy(r)[C][:, :, :nz].astype(np.float64) - 0.75).max() < 4 * 0.75 * np.finfo(np.float32).eps
    for k, v in worst.items():
        assert v < TOL32_REMAP["real" if case == "real" else "hand"]["tracer" if k.startswith("tracer") else k], (k, v, worst)
