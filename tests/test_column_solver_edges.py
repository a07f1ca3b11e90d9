"""The non-hydrostatic column chain (riem_solver_c, riem_solver3, the closing height scans of update_dz_c / update_dz_d, pk3_halo,
edge_pe, ray_fast, apply_diffusive_heating) alone through the C ABI against the oracle, where test_operator_parity.py's smooth C12 L8 /
L10 states never go:

* the p_fac pressure floor of SIM1 taken in part of every column (layer thickness stretched by blocks, p_fac = 0.5);
* level counts of every residue mod 8, with partial and full last register groups, on both sides of every switch between the
  kernel forms (gam in registers / in the scratch field, wave kernels / column kernels), in fp64 and in fp32;
* the forced forms (FV3_RIEM_MODE=columns / wave, FV3_RIEM_REGS=0), each in a child process, against the oracle element by element;
* the dz_min scan where it acts, both upwind signs of update_dz_c, the three limits of the diffusive heating on both sides and in
  both signs, the Rayleigh layer's level classes;
* the Fortran model's C12 L63 restart with its terrain and moisture (one recorded oracle call, every operator replayed alone);
* the fp32 build against the fp64 oracle.

The synthetic cases (level sweep, forced forms, fp32 sweep, height scans, heating, Rayleigh layer) assert through the oracle's opt-in
branch counters (fv3_oracle.nh), per oracle call, that the branch they exist for was taken; the real-state replays assert none.  Every
comparison is element by element on the operator's whole output region, field-scale relative (max |a - b| / max |b| per rank).

fp64 bounds: the per-field tolerances of test_operator_parity.py (TOL below) hold in every case; no case needed a bound derived from
the oracle's own round-off.  Worst errors measured over the module (host emulation / MI355X where they differ): riem_solver3 w 2.4e-12 /
4.3e-11 (smooth state, L11: w there is a small remainder of cancelling terms), delz 3.1e-13 / 3.6e-13 and zh 3.9e-14 (floor state, L80),
ppe 2.7e-11 (real state), pk3 / pk 9.3e-16, peln 1.5e-16, pe 0; riem_solver_c gz 8.7e-15 / 9.2e-15, pef 2.9e-14 (floor state, L127); the
height updates, the heating, ray_fast, nh_p_grad and edge_pe 0.  The round-off of the fp64 oracle itself on the floor state (against its
np.longdouble solve, test_fp64_oracle_round_off_on_the_floor_state) is w 2.5e-13, delz 2.0e-13, zh 2.6e-14, ppe 1.2e-13 at the worst of
L8 / L79 / L81: of the size of the library's errors there.

fp32 bounds (TOL32): per field 2 x the worst error against the fp64 oracle over this module's cases, measured on the host emulation and
on the MI355X (host emulation / MI355X where they differ; the device's fp32 log / exp and fused multiply-adds account for factors up to
3.1, no field exceeds the host emulation by more):
  smooth: update_dz_c: gz 3.3e-7, ws3 0; riem_solver_c: gz 1.1e-6 / 1.6e-6, pef 1.7e-6 / 1.8e-6; update_dz_d: zh 3.7e-7, wsd 0;
    riem_solver3: w 6.9e-3 / 1.3e-2, delz 2.4e-6 / 6.0e-6, zh 1.1e-6 / 2.7e-6, ppe 1.1e-2 / 1.9e-2, pk3 4.7e-7 / 8.1e-7, pe 5.8e-7,
    pk 4.7e-7 / 8.1e-7, peln 9.3e-8 / 1.9e-7; pk3_halo: pk3 4.6e-7 / 8.2e-7; pe_halo: pe 5.4e-7; apply_diffusive_heating: pt 9.7e-8
  floor: riem_solver_c: gz 5.7e-6 / 6.0e-6, pef 5.0e-5 / 5.7e-5; riem_solver3: w 1.7e-4 / 3.3e-4, delz 1.7e-4 / 2.0e-4, zh 1.6e-5 /
    1.5e-5, ppe 8.2e-5 / 1.7e-4, pk3 4.7e-7 / 8.1e-7, pe 5.8e-7, pk 4.7e-7 / 8.1e-7, peln 9.3e-8 / 1.9e-7; pk3_halo: pk3 4.6e-7 /
    8.2e-7; pe_halo: pe 5.4e-7; apply_diffusive_heating: pt 9.7e-8
  real: update_dz_c: gz 2.8e-7, ws3 5.4e-3; riem_solver_c: gz 3.4e-7 / 6.1e-7, pef 5.1e-7 / 7.3e-7; update_dz_d: zh 3.4e-7, wsd
    6.0e-3; riem_solver3: w 4.5e-4 / 9.8e-4, delz 1.0e-6 / 2.3e-6, zh 3.7e-7 / 5.7e-7, ppe 3.9e-3 / 1.2e-2, pk3 4.3e-7 / 7.6e-7, pe
    4.5e-7, pk 4.3e-7 / 7.6e-7, peln 7.4e-8 / 1.7e-7; pk3_halo: pk3 4.2e-7 / 7.2e-7; pe_halo: pe 2.9e-7; apply_diffusive_heating: pt
    5.4e-8
  w and ppe (and ws3 / wsd on the real terrain) are remainders of cancelling terms -- w of the smooth state out of accelerations that
  nearly balance, ppe ~1e2 Pa out of pressures ~1e5 Pa, ws3 = (zs - gz) / dt out of heights ~1e3 m -- so fp32 holds them to 1e-3 ..
  1e-2 of their own scale.  ws3 / wsd of the synthetic state are exactly 0 on both sides (flat terrain: zs and the bottom height are equal).
"""
import copy
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import Case, compare_cubes, oracle_cube, run_device_cube
from pace_amd.constants import get_constants

import fv3_oracle.nh as o_nh
from fv3_oracle.dyn_core import OracleAcousticDynamics
from fv3_oracle.util import Dom
from test_operator_parity import Dev, Recorder, recorded
from test_restart_six_tiles import GOLDEN, _restart_cube

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANK = 2

CELLS = lambda D: D.sl(1, D.nx, 1, D.ny)  # noqa: E731
RING1 = lambda D: D.sl(0, D.nx + 1, 0, D.ny + 1)  # noqa: E731
RING2 = lambda D: D.sl(-1, D.nx + 2, -1, D.ny + 2)  # noqa: E731
U = lambda D: D.sl(1, D.nx, 1, D.ny + 1)  # noqa: E731
V = lambda D: D.sl(1, D.nx + 1, 1, D.ny)  # noqa: E731

# oracle function -> (C entry, arguments, outputs); pe_halo is the library's edge_pe.  An argument is ("f", i) = field from oracle argument i (counted after
# the Dom), ("s", i) = scalar, ("b", i) = flag; an output is (name, oracle argument, region, first level, levels: "nz" / "nz+1" / "2d").
F, S = (lambda i: ("f", i)), (lambda i: ("s", i))
PLANS = {
    "update_dz_c": ("update_dz_c", [F(1), F(2), F(3), F(4), F(5), S(6)], [("gz", 4, RING1, 0, "nz+1"), ("ws3", 5, RING1, 0, "2d")]),
    "riem_solver_c": ("riem_solver_c", [S(0), F(1), S(2), F(3), F(4), F(5), F(6), F(7), F(8), F(9), F(10)], [("gz", 8, RING1, 0, "nz+1"), ("pef", 9, RING1, 0, "nz+1")]),
    "update_dz_d": ("update_dz_d", [F(3), F(4), F(5), F(6), F(7), F(8), F(9), S(10)], [("zh", 4, CELLS, 0, "nz+1"), ("wsd", 9, CELLS, 0, "2d")]),
    "riem_solver3": ("riem_solver3", [("b", 0), S(1), F(2), S(3)] + [F(i) for i in range(4, 17)],
                     [("w", 16, CELLS, 0, "nz"), ("delz", 6, CELLS, 0, "nz"), ("zh", 10, CELLS, 0, "nz+1"), ("ppe", 12, CELLS, 0, "nz+1"), ("pk3", 13, CELLS, 0, "nz+1"),
                      ("pe", 11, CELLS, 0, "nz+1"), ("pk", 14, CELLS, 0, "nz+1"), ("peln", 15, CELLS, 0, "nz+1")]),
    "pk3_halo": ("pk3_halo", [F(0), F(1), S(2), S(3)], [("pk3", 0, RING2, 1, "nz+1")]),
    "pe_halo": ("edge_pe", [F(0), F(1), S(2)], [("pe", 0, RING1, 0, "nz+1")]),
    "nh_p_grad": ("nh_p_grad", [F(0), F(1), F(2), F(3), F(4), F(5), S(6), S(7), S(8)], [("u", 0, U, 0, "nz"), ("v", 1, V, 0, "nz")]),
    "apply_diffusive_heating": ("apply_diffusive_heating", [F(0), F(1), F(2), F(3), F(4), S(5)], [("pt", 4, CELLS, 0, "nz")]),
    "ray_fast": ("ray_fast", [F(1), F(2), F(3), S(6), S(7)], [("u", 1, U, 0, "nz"), ("v", 2, V, 0, "nz"), ("w", 3, CELLS, 0, "nz")]),
    # (tests/test_height_pgf_operator_edges.py; ("i", n) = integer argument)
    "p_grad_c": ("p_grad_c", [F(2), F(3), F(4), F(5), F(6), S(7)], [("uc", 2, V, 0, "nz"), ("vc", 3, U, 0, "nz")]),
    "del2_cubed": ("del2_cubed", [F(0), S(1), ("i", 2)], [("heat_source", 0, CELLS, 0, "nz")]),
}
# the tolerances of test_operator_parity.py (test_update_dz_c, test_riem_solver_c, test_update_dz_d, test_riem_solver3_on_recorded_inputs,
# test_pk3_halo_and_edge_pe, test_nh_p_grad, test_ray_fast, test_del2_cubed_and_diffusive_heating)
TOL = {
    "update_dz_c": {"gz": 1e-13, "ws3": 1e-11},
    "riem_solver_c": {"gz": 1e-12, "pef": 1e-12},
    "update_dz_d": {"zh": 1e-13, "wsd": 1e-10},
    "riem_solver3": {"w": 1e-10, "delz": 1e-12, "zh": 1e-13, "ppe": 1e-9, "pk3": 1e-13, "pe": 1e-14, "pk": 1e-13, "peln": 1e-14},
    "pk3_halo": {"pk3": 1e-13},
    "pe_halo": {"pe": 1e-14},
    "nh_p_grad": {"u": 1e-12, "v": 1e-12},
    "apply_diffusive_heating": {"pt": 1e-14},
    "ray_fast": {"u": 1e-13, "v": 1e-13, "w": 1e-13},
    "p_grad_c": {"uc": 1e-13, "vc": 1e-13},
    "del2_cubed": {"heat_source": 1e-12},
}
# fp32 build against the fp64 oracle: 2 x the worst measured error (module docstring), per state and operator
TOL32 = {
    "smooth": {
        "update_dz_c": {"gz": 6.6e-7, "ws3": 0},
        "riem_solver_c": {"gz": 3.2e-6, "pef": 3.6e-6},
        "update_dz_d": {"zh": 7.4e-7, "wsd": 0},
        "riem_solver3": {"w": 2.6e-2, "delz": 1.2e-5, "zh": 5.4e-6, "ppe": 3.8e-2, "pk3": 1.6e-6, "pe": 1.2e-6, "pk": 1.6e-6, "peln": 3.8e-7},
        "pk3_halo": {"pk3": 1.6e-6},
        "pe_halo": {"pe": 1.1e-6},
        "apply_diffusive_heating": {"pt": 1.9e-7},
    },
    "floor": {
        "riem_solver_c": {"gz": 1.2e-5, "pef": 1.1e-4},
        "riem_solver3": {"w": 6.6e-4, "delz": 4.0e-4, "zh": 3.2e-5, "ppe": 3.4e-4, "pk3": 1.6e-6, "pe": 1.2e-6, "pk": 1.6e-6, "peln": 3.8e-7},
        "pk3_halo": {"pk3": 1.6e-6},
        "pe_halo": {"pe": 1.1e-6},
        "apply_diffusive_heating": {"pt": 1.9e-7},
    },
    "real": {
        "update_dz_c": {"gz": 5.6e-7, "ws3": 1.1e-2},
        "riem_solver_c": {"gz": 1.2e-6, "pef": 1.5e-6},
        "update_dz_d": {"zh": 6.8e-7, "wsd": 1.2e-2},
        "riem_solver3": {"w": 2.0e-3, "delz": 4.6e-6, "zh": 1.1e-6, "ppe": 2.4e-2, "pk3": 1.5e-6, "pe": 9.0e-7, "pk": 1.5e-6, "peln": 3.4e-7},
        "pk3_halo": {"pk3": 1.4e-6},
        "pe_halo": {"pe": 5.8e-7},
        "apply_diffusive_heating": {"pt": 1.1e-7},
    },
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


@pytest.fixture
def counts():
    o_nh.enable_counters(True)
    yield o_nh
    o_nh.enable_counters(False)


@pytest.fixture(scope="module")
def data():
    return np.load(GOLDEN)


# ---------------------------------------------------------------------------------------------------------------------------
# one operator alone: oracle call record, library replay, element-wise errors
# ---------------------------------------------------------------------------------------------------------------------------
def ocall(name, D, *args):
    """the oracle's operator on copies of ``args``: a call record like the Recorder's, plus the branch counts of this call alone"""
    cp = lambda a: a.copy() if isinstance(a, np.ndarray) else a  # noqa: E731
    work = [cp(a) for a in args]
    before = o_nh.counters()
    getattr(o_nh, name)(D, *work)
    after = o_nh.counters()
    return dict(ins=[cp(a) for a in args], outs=work, D=D, counts={k: after[k] - before[k] for k in after})


def assert_floor_counts(calls, kind):
    """each SIM1 call of the case on its own: the floor state takes the p_fac floor in part of its levels, the smooth state in none"""
    solves = [key for key in calls if key.startswith("riem_solver")]
    assert solves
    for key in solves:
        n = calls[key]["counts"]
        if kind == "floor":
            assert n["sim1_floor"] > 0 and n["sim1_free"] > 0, (key, n)
        else:
            assert n["sim1_floor"] == 0 and n["sim1_free"] > 0, (key, n)


def device(backend, grids, cfg, constants=None, dtype=torch.float64):
    """test_operator_parity.Dev with the constants / precision of the case"""
    return Dev(backend, grids, cfg, constants=constants, dtype=dtype)


def replay(dv, name, cl):
    """the library's operator alone on the inputs of the call records ``cl`` (one per rank): {oracle argument: [array per rank]}"""
    entry, args, outs = PLANS[name]
    qs, call_args = {}, []
    for kind, i in args:
        if kind == "f":
            qs[i] = dv.q([c["ins"][i] for c in cl])
            call_args.append(qs[i].fref)
        else:
            v = cl[0]["ins"][i]
            call_args.append(int(bool(v)) if kind == "b" else int(v) if kind == "i" else float(v))
    dv.sf.call(entry, *call_args)
    if dv.sf.backend != "hostemu":
        torch.cuda.synchronize()
    return {i: [qs[i].numpy(r).astype(np.float64) for r in range(len(cl))] for _, i, *_ in outs}


def errors(name, got, cl, nz):
    """worst field-scale relative error per output over the ranks, every element of the operator's output region; finite everywhere"""
    worst = {}
    for fname, i, region, k0, lev in PLANS[name][2]:
        for r, c in enumerate(cl):
            D = c["D"]
            g, w = got[i][r].copy(), np.asarray(c["outs"][i], dtype=np.float64).copy()
            if lev == "2d":
                g, w = g.reshape(g.shape[0], g.shape[1]), w.reshape(w.shape[0], w.shape[1])
            if region is RING1:
                # the cube-corner halo cell of a cell-centred field belongs to no neighbour: never read, not compared
                for (ci, cj), has in (((0, 0), D.sw), ((D.nx + 1, 0), D.se), ((D.nx + 1, D.ny + 1), D.ne), ((0, D.ny + 1), D.nw)):
                    if has:
                        g[D.sl(ci, ci, cj, cj)] = 0.0
                        w[D.sl(ci, ci, cj, cj)] = 0.0
            g, w = g[region(D)], w[region(D)]
            if lev != "2d":
                k1 = nz if lev == "nz" else nz + 1
                g, w = g[:, :, k0:k1], w[:, :, k0:k1]
            assert np.all(np.isfinite(w)), f"{name} {fname} rank {r}: the oracle is not finite"
            assert np.all(np.isfinite(g)), f"{name} {fname} rank {r}: non-finite"
            sc = np.abs(w).max()
            e = float(np.abs(g - w).max())
            worst[fname] = max(worst.get(fname, 0.0), e / sc if sc > 0 else e)
    return worst


def check(name, got, cl, nz, tol=None, label=""):
    worst = errors(name, got, cl, nz)
    print(f"{label} {name}:", {k: f"{v:.1e}" for k, v in worst.items()})
    tol = tol or TOL[name]
    bad = {k: v for k, v in worst.items() if not v <= tol[k]}
    assert not bad, f"{label} {name}: field-scale relative errors above tolerance: {bad} (all: {worst}; bounds: {tol})"
    return worst


# ---------------------------------------------------------------------------------------------------------------------------
# the synthetic column case: one C12 rank, smooth or with the layer thickness stretched by blocks
# ---------------------------------------------------------------------------------------------------------------------------
KINDS = {"smooth": (1.0, 0.05), "floor": (3.0, 0.5)}  # (stretch, p_fac)
DT = 18.75


def stretch_factor(nz, stretch):
    k = np.arange(nz)
    return np.where((k // max(1, min(8, nz // 3))) % 2 == 1, stretch, 1.0)


def column_case(nz, kind, backend, dtype=torch.float64):
    stretch, p_fac = KINDS[kind]
    kw = dict(p_fac=p_fac)
    if dtype == torch.float32:
        kw["nord"] = 1  # (the fp32 context refuses the default del-6 damping tables at this resolution; no operator here reads them)
    cs = Case(12, (1, 1), (RANK,), nz=nz, backend=backend, cfg_kw=kw, dtype=dtype)
    x = {k: v.copy() for k, v in cs.states[0].items()}
    x["delz"][:, :, :nz] *= stretch_factor(nz, stretch)[None, None, :]
    return cs, x


def column_calls(cs, x, ops=("riem_solver_c", "riem_solver3_0", "riem_solver3_1", "pk3_halo", "pe_halo")):
    """the oracle's call records of the column operators on the case's inputs"""
    c, D, nz, g = cs.c, cs.doms[0], cs.nz, cs.grids[0]
    ni, nj = x["u"].shape[:2]
    zs = x["phis"] * c.RGRAV
    zh = np.zeros_like(x["u"])
    zh[:, :, nz] = zs[:, :, 0]
    for k in range(nz - 1, -1, -1):
        zh[:, :, k] = zh[:, :, k + 1] - x["delz"][:, :, k]
    z = lambda: np.zeros_like(zh)  # noqa: E731
    calls = {}
    if "riem_solver_c" in ops:
        # on the compute domain + 1 ring; the surface vertical velocity varies over the columns and changes sign
        i, j = np.arange(ni)[:, None, None], np.arange(nj)[None, :, None]
        ws = 0.05 * np.sin(0.9 * i + 0.4 * j) + 0.01 * np.cos(0.3 * i - 1.1 * j)
        assert ws[RING1(D)].min() < -0.02 and ws[RING1(D)].max() > 0.02
        calls["riem_solver_c"] = ocall("riem_solver_c", D, 0.5 * DT, x["cappa"], g.ptop, x["phis"], ws, x["pt"], x["q_con"], x["delp"], zh, z(), x["w"], cs.cfg.p_fac)
    for last in (0, 1):
        if f"riem_solver3_{last}" in ops:
            calls[f"riem_solver3_{last}"] = ocall("riem_solver3", D, bool(last), DT, x["cappa"], g.ptop, zs, np.full_like(zs, 0.01), x["delz"], x["q_con"], x["delp"], x["pt"], zh,
                                                  x["pe"], z(), z(), x["pk"], x["peln"], x["w"], cs.cfg.p_fac)
    if "pk3_halo" in ops:
        pk3 = calls["riem_solver3_1"]["outs"][13] if "riem_solver3_1" in calls else z()
        calls["pk3_halo"] = ocall("pk3_halo", D, pk3, x["delp"], g.ptop, c.KAPPA)
    if "pe_halo" in ops:
        calls["pe_halo"] = ocall("pe_halo", D, x["pe"], x["delp"], g.ptop)
    return calls


def op_of(key):
    return key[:-2] if key.startswith("riem_solver3_") else key


def library_outputs(case, backend):
    """The library's outputs of one named case (``riem:<kind>:<nz>``) on one backend, as {"<call>/<oracle argument>": array}: what
    tests/column_case.py writes for the parent test (the kernel forms are chosen once per process)."""
    what, kind, nz = case.split(":")
    assert what == "riem"
    cs, x = column_case(int(nz), kind, backend)
    calls = column_calls(cs, x, ops=("riem_solver_c", "riem_solver3_1"))
    dv = device(backend, cs.grids, cs.cfg)
    out = {}
    for key, cl in calls.items():
        for i, arrs in replay(dv, op_of(key), [cl]).items():
            out[f"{case}/{key}/{i}"] = arrs[0]
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# 2. level-count sweep, fp64
# ---------------------------------------------------------------------------------------------------------------------------
LEVELS = [3, 4, 5, 6, 7, 9, 11, 13, 77, 78, 79, 80, 81, 127, 128, 129]


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("nz", LEVELS)
def test_column_solvers_at_every_level_count_match_the_oracle(backend, counts, nz, kind):
    """riem_solver_c (compute domain + 1 ring, sign-changing ws), riem_solver3 (last_call 0 and 1), pk3_halo and edge_pe alone, at
    level counts of every residue mod 8 and on both sides of the fp64 switches (gam in registers below 80 levels; riem_solver3 as
    wave kernels up to 80, riem_solver_c up to 128), on the smooth state and with the p_fac floor taken in part of the levels."""
    cs, x = column_case(nz, kind, backend)
    calls = column_calls(cs, x)
    assert_floor_counts(calls, kind)
    dv = device(backend, cs.grids, cs.cfg)
    for key, cl in calls.items():
        check(op_of(key), replay(dv, op_of(key), [cl]), [cl], nz, label=f"L{nz} {kind} {key}")


@pytest.mark.parametrize("nz", [8, 79, 81])
def test_fp64_oracle_round_off_on_the_floor_state(hostemu, nz):
    """The reference's own error: riem_solver3 of the fp64 oracle against the same oracle run in np.longdouble (every work array of
    sim1_solver takes the dtype of its inputs).  A correct library carries a round-off of the same size, so a tolerance in use must at
    least cover the oracle's: the fp64 oracle stays inside every tolerance of TOL against its long-double self.  (Measured, at the
    worst of the three level counts: w 2.5e-13 and ppe 1.2e-13 at L81, delz 2.0e-13 and zh 2.6e-14 -- a quarter of its 1e-13 -- at L79; a
    case that exceeded TOL would get 4 x its own figure as its bound.)"""
    cs, x = column_case(nz, "floor", "hostemu")
    cl = column_calls(cs, x, ops=("riem_solver3_1",))["riem_solver3_1"]
    L = lambda a: a.astype(np.longdouble) if isinstance(a, np.ndarray) else a  # noqa: E731
    work = [L(a) for a in cl["ins"]]
    o_nh.riem_solver3(cs.doms[0], *work)
    assert all(work[i].dtype == np.longdouble for _, i, *_ in PLANS["riem_solver3"][2])
    assert np.finfo(np.longdouble).eps < 1e-18  # (an extended type: where long double is double this measures nothing)
    ref = dict(cl, outs=[np.asarray(a, dtype=np.float64) if isinstance(a, np.ndarray) else a for a in work])
    got = {i: [cl["outs"][i]] for _, i, *_ in PLANS["riem_solver3"][2]}
    check("riem_solver3", got, [ref], nz, label=f"fp64 oracle against long double, L{nz}")


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the forced kernel forms against the oracle, each in a child process
# ---------------------------------------------------------------------------------------------------------------------------
FORMS = {"FV3_RIEM_MODE=columns": (8, 79, 80), "FV3_RIEM_MODE=wave": (8, 79, 80, 127), "FV3_RIEM_REGS=0": (8, 79, 80)}
_CHILD = {}
_CHILD_FAILED = {}


def _child(tmp_path, backend, setting, levels):
    """one child process of tests/column_case.py under its own timeout.  A failed child fails the test and is not started again; after
    it no further child is started on that backend either (whatever it was -- a fault, a time limit -- nothing more goes to the device
    from here): the tests that still want one fail with the first failure's message."""
    key = (backend, setting)
    if backend in _CHILD_FAILED:
        pytest.fail(f"no further child process on {backend}: {_CHILD_FAILED[backend]}")
    if key not in _CHILD:
        out = str(tmp_path / f"{setting.replace('=', '_') or 'default'}.npz")
        env = {k: v for k, v in os.environ.items() if not k.startswith("FV3_RIEM_")}
        if setting:
            name, val = setting.split("=")
            env[name] = val
        cases = ",".join(f"riem:floor:{nz}" for nz in levels)
        try:
            subprocess.run([sys.executable, os.path.join(ROOT, "tests", "column_case.py"), "--cases", cases, "--backend", backend, "--out", out], check=True, env=env, timeout=300)
            with np.load(out) as f:
                _CHILD[key] = {k: f[k] for k in f.files}
        except Exception as e:
            _CHILD_FAILED[backend] = f"the child with {setting or 'the default forms'} failed: {e!r}"
            raise
    return _CHILD[key]


@pytest.mark.parametrize("setting", list(FORMS))
def test_forced_kernel_forms_match_the_oracle_and_the_default_form(backend, counts, tmp_path, setting):
    """FV3_RIEM_MODE=columns (thread-per-column kernels), FV3_RIEM_MODE=wave (the wave kernels where the default leaves them: riem_solver3
    at L127) and FV3_RIEM_REGS=0 (gam through the scratch field) on the floor state: each form against the oracle at the tolerances of
    the level sweep, and against the default form element by element at 1e-11 (test_alternative_kernel_forms_agree's bound)."""
    levels = FORMS[setting]
    forced = _child(tmp_path, backend, setting, levels)
    default = _child(tmp_path, backend, "", (8, 79, 80, 127))
    for nz in levels:
        case = f"riem:floor:{nz}"
        cs, x = column_case(nz, "floor", backend)
        calls = column_calls(cs, x, ops=("riem_solver_c", "riem_solver3_1"))
        assert_floor_counts(calls, "floor")
        for key, cl in calls.items():
            pick = lambda src: {i: [src[f"{case}/{key}/{i}"]] for _, i, *_ in PLANS[op_of(key)][2]}  # noqa: E731
            check(op_of(key), pick(forced), [cl], nz, label=f"{setting} L{nz}")
            ref = dict(cl, outs={i: a[0] for i, a in pick(default).items()})
            check(op_of(key), pick(forced), [ref], nz, tol=dict.fromkeys(TOL[op_of(key)], 1e-11), label=f"{setting} against the default form, L{nz}")


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the height scan where it acts
# ---------------------------------------------------------------------------------------------------------------------------
DZ_MIN_CASES = {8: 700.0, 79: 40.0}  # L79: the layers of the lowest levels are 29 .. 40 m thick


def _with_dz_min(cl, dz_min):
    """the recorded call records on Doms whose constants carry ``dz_min``; outs recomputed by the oracle"""
    cst = dataclasses.replace(get_constants(), DZ_MIN=dz_min)
    return cst, [dict(c, D=Dom(c["D"].grid, cst)) for c in cl]


@pytest.mark.parametrize("layout, nz", [((1, 1), 8), ((2, 2), 8), ((1, 1), 79), ((2, 2), 79)])
def test_height_scans_where_dz_min_acts_match_the_oracle(backend, counts, layout, nz):
    """update_dz_c and update_dz_d alone with dz_min of the order of the layer thickness (L8: 700 m against layers from 625 m; L79: 40 m,
    which only the lowest layers fall short of): heights the scan raised and heights it left both occur; update_dz_c takes both upwind
    branches in x and in y."""
    part, cfg, grids, calls, _ = recorded(layout, nz=nz)
    for name in ("update_dz_c", "update_dz_d"):
        cst, cl = _with_dz_min(calls[name], DZ_MIN_CASES[nz])
        counts.reset_counters()
        cl = [ocall(name, c["D"], *c["ins"]) for c in cl]
        n = counts.counters()
        short = "dzc" if name == "update_dz_c" else "dzd"
        assert n[f"{short}_limited"] > 0 and n[f"{short}_free"] > 0, n
        if nz == 79:
            assert n[f"{short}_limited"] < 0.2 * n[f"{short}_free"], n
        if name == "update_dz_c":
            assert all(n[f"dzc_upwind_{s}_{d}"] > 0 for s in ("pos", "neg") for d in "xy"), n
        dv = device(backend, grids, cfg, constants=cst)
        check(name, replay(dv, name, cl), cl, nz, label=f"dz_min {DZ_MIN_CASES[nz]} {layout}")


def test_full_acoustic_call_with_the_height_scan_acting_matches_the_oracle(backend, counts):
    """Two sub-steps at L8 with dz_min = 700 m: inside the sequencer update_dz_d leaves its scan to riem_solver3's pre-sweep, so this
    puts the pre-sweep form in front of the oracle with the limit acting (test_full_acoustic_call's tolerances)."""
    from test_parity import STATE, TOL as TOL_CALL

    nz = 8
    cst = dataclasses.replace(get_constants(), DZ_MIN=700.0)
    part, cfg, grids, ost, phis, _ = oracle_cube(12, (1, 1), nz, dict(n_split=2))
    init = [{k: v.copy() for k, v in s.items()} for s in ost]
    odyn = OracleAcousticDynamics(part, grids, cfg, cst, phis)
    counts.reset_counters()
    odyn(ost, 225.0, 1)
    n = counts.counters()
    assert n["dzd_limited"] > 0 and n["dzd_free"] > 0 and n["dzc_limited"] > 0, n
    got, *_ = run_device_cube(backend, part, cfg, grids, init, phis, 225.0, constants=cst)
    compare_cubes(got, ost, part, nz, STATE, TOL_CALL)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. heating limiter and Rayleigh layer
# ---------------------------------------------------------------------------------------------------------------------------
def heating_call(cs, x, f=0.01):
    """a heat source whose |dtmp| = |heat| / (cv delp) is 0.5 x and 2 x the limit of its level (0.1 f at level 0, 0.5 f at level 1, f below),
    in both signs, in a pattern that puts all four in every level"""
    nz, c = cs.nz, cs.c
    ni, nj = x["u"].shape[:2]
    i, j, k = np.arange(ni)[:, None, None], np.arange(nj)[None, :, None], np.arange(nz)[None, None, :]
    lim = np.full(nz, f)
    lim[0] *= 0.1
    lim[1] *= 0.5
    ratio = np.array([0.5, -0.5, 2.0, -2.0])[(i + 2 * j + k) % 4] * (1.0 + 0.1 * np.sin(0.7 * i + 0.3 * j + k))
    hs = np.zeros_like(x["u"])
    hs[:, :, :nz] = ratio * lim[None, None, :] * c.CV_AIR * x["delp"][:, :, :nz]
    return ocall("apply_diffusive_heating", cs.doms[0], x["delp"], x["delz"], x["cappa"], hs, x["pt"], f)


@pytest.mark.parametrize("nz", [3, 8, 79])
def test_diffusive_heating_on_both_sides_of_its_limits_matches_the_oracle(backend, counts, nz):
    cs, x = column_case(nz, "smooth", backend)
    counts.reset_counters()
    cl = heating_call(cs, x)
    n = counts.counters()
    assert n["heat_limited"] > 0 and n["heat_free"] > 0, n
    C = CELLS(cs.doms[0])
    d = (cl["outs"][4] - cl["ins"][4])[C][:, :, :nz]
    for k in range(nz):  # every level: warmed and cooled, cut and not cut
        a = np.abs(d[:, :, k])
        assert d[:, :, k].min() < 0.0 < d[:, :, k].max() and a.max() > 1.5 * a.min(), k
    check("apply_diffusive_heating", replay(device(backend, cs.grids, cs.cfg), "apply_diffusive_heating", [cl]), [cl], nz, label=f"L{nz}")


@pytest.mark.parametrize("case", ["L3_none", "L79", "L79_margin", "L79_nudged_only"])
def test_ray_fast_level_classes_match_the_oracle(backend, counts, case):
    """L3: no level under rf_cutoff (+ the nudging margin): the operator returns at once, u / v / w unchanged.  L79: the reference's level
    set (7 damped levels; no level falls into the 100 Pa margin above rf_cutoff).  L79_margin: rf_cutoff just under the pressure of level
    7, so that this level is not damped but receives the momentum fix.  L79_nudged_only: rf_cutoff just under the pressure of the top
    level: a level is nudged, none damped -- the momentum taken out is zero, so nothing may change."""
    from pace_amd.grid import make_grid

    nz = 3 if case == "L3_none" else 79
    kw = {}
    if case in ("L79_margin", "L79_nudged_only"):
        k = 7 if case == "L79_margin" else 0
        g0 = make_grid(Case(12, (1, 1), (RANK,), nz=3).part, RANK, nz=nz)
        margin = min(100.0, 10.0 * g0.ptop)
        kw["rf_cutoff"] = float(g0.pfull[k] - 0.5 * min(margin, g0.pfull[k + 1] - g0.pfull[k]))
    cs = Case(12, (1, 1), (RANK,), nz=nz, backend=backend, cfg_kw=kw)
    x, g = cs.states[0], cs.grids[0]
    counts.reset_counters()
    cl = ocall("ray_fast", cs.doms[0], cs.cfg, x["u"], x["v"], x["w"], g.dp_ref, g.pfull, DT, g.ptop)
    n = counts.counters()
    changed = max(np.abs(cl["outs"][i] - cl["ins"][i]).max() for i in (1, 2, 3))
    if case == "L3_none":
        assert n["ray_damped"] == 0 and n["ray_nudged_only"] == 0 and n["ray_none"] == 3 and changed == 0.0, n
    elif case == "L79":
        assert n["ray_damped"] > 0 and n["ray_nudged_only"] == 0 and n["ray_none"] > 0 and changed > 0.0, n
    elif case == "L79_margin":
        assert n["ray_damped"] == 7 and n["ray_nudged_only"] == 1 and n["ray_none"] > 0 and changed > 0.0, n
    else:
        assert n["ray_damped"] == 0 and n["ray_nudged_only"] > 0 and n["ray_none"] > 0 and changed == 0.0, n
    check("ray_fast", replay(device(backend, cs.grids, cs.cfg), "ray_fast", [cl]), [cl], nz, label=case)


# ---------------------------------------------------------------------------------------------------------------------------
# 6. the real state: one recorded oracle call of the six restart tiles, every column operator replayed alone
# ---------------------------------------------------------------------------------------------------------------------------
REAL_OPS = ("update_dz_c", "riem_solver_c", "update_dz_d", "riem_solver3", "pk3_halo", "pe_halo", "nh_p_grad")
_REAL = {}


def real_calls(data, layout):
    if layout not in _REAL:
        c, part, cfg, grids, states, phis = _restart_cube(data, layout)
        odyn = OracleAcousticDynamics(part, grids, cfg, c, phis)
        ost = [{k: v.copy() for k, v in s.items()} for s in states]
        with Recorder() as rec:
            odyn(ost, 60.0, 1)
        _REAL[layout] = (part, cfg, grids, rec.calls)
    return _REAL[layout]


@pytest.mark.parametrize("layout", [(1, 1), (2, 2)])
def test_column_operators_on_the_real_state_match_the_oracle(backend, data, layout):
    """63 levels, terrain, real moisture in q_con / cappa; both sub-steps of the call (the second is riem_solver3's last_call)"""
    part, cfg, grids, calls = real_calls(data, layout)
    nr = part.total_ranks
    dv = device(backend, grids, cfg)
    for name in REAL_OPS:
        assert len(calls[name]) == (nr if name == "pe_halo" else 2 * nr)  # (the halo of pe: once per call, after the last sub-step)
        for it in range(len(calls[name]) // nr):
            cl = calls[name][it * nr : (it + 1) * nr]
            check(name, replay(dv, name, cl), cl, 63, label=f"real {layout} sub-step {it}")


# ---------------------------------------------------------------------------------------------------------------------------
# 7. fp32 against the fp64 oracle
# ---------------------------------------------------------------------------------------------------------------------------
LEVELS32 = [8, 79, 127, 128, 129, 160, 161, 256, 257]


def _tol32(kind, op):
    return TOL32[kind][op]


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("nz", LEVELS32)
def test_fp32_column_solvers_track_the_fp64_oracle(backend32, counts, nz, kind):
    """the fp32 build on both sides of its switches (gam in registers below 128 levels; riem_solver3 as wave kernels up to 160,
    riem_solver_c up to 256; 256 / 257 levels: riem_solver_c alone): finite, field-scale bounds TOL32"""
    cs, x = column_case(nz, kind, backend32, dtype=torch.float32)
    deep = nz >= 256
    calls = column_calls(cs, x, ops=("riem_solver_c",) if deep else ("riem_solver_c", "riem_solver3_0", "riem_solver3_1", "pk3_halo", "pe_halo"))
    assert_floor_counts(calls, kind)
    if not deep:
        calls["apply_diffusive_heating"] = heating_call(cs, x)
    dv = device(backend32, cs.grids, cs.cfg, dtype=torch.float32)
    for key, cl in calls.items():
        check(op_of(key), replay(dv, op_of(key), [cl]), [cl], nz, tol=_tol32(kind, op_of(key)), label=f"fp32 L{nz} {kind} {key}")


@pytest.mark.parametrize("nz", [8, 79, 127, 128, 129, 160, 161])
def test_fp32_height_updates_track_the_fp64_oracle(backend32, nz):
    """update_dz_c / update_dz_d in fp32 on the recorded inputs of one synthetic C12 call per level count"""
    part, cfg, grids, calls, _ = recorded((1, 1), nz=nz)
    cfg = copy.copy(cfg)
    cfg.nord = 1
    for name in ("update_dz_c", "update_dz_d"):
        cl = calls[name]
        if name == "update_dz_d":  # (the oracle with the damping order of the fp32 context)
            import fv3_oracle.d_sw as o_dsw

            cl = [ocall(name, c["D"], cfg, o_dsw.get_column_namelist(cfg, nz), *c["ins"][2:]) for c in cl]
        dv = device(backend32, grids, cfg, dtype=torch.float32)
        check(name, replay(dv, name, cl), cl, nz, tol=_tol32("smooth", name), label=f"fp32 L{nz}")


def test_fp32_column_operators_on_the_real_state_track_the_fp64_oracle(backend32, data):
    part, cfg, grids, calls = real_calls(data, (1, 1))
    cfg = copy.copy(cfg)
    cfg.nord = 1
    nr = part.total_ranks
    dv = device(backend32, grids, cfg, dtype=torch.float32)
    import fv3_oracle.d_sw as o_dsw

    for name in ("update_dz_c", "riem_solver_c", "update_dz_d", "riem_solver3", "pk3_halo", "pe_halo", "apply_diffusive_heating"):
        cl = calls[name][-nr:]  # (the last sub-step: riem_solver3's last_call)
        if name == "update_dz_d":  # (the oracle with the damping order of the fp32 context)
            cl = [ocall(name, c["D"], cfg, o_dsw.get_column_namelist(cfg, 63), *c["ins"][2:]) for c in cl]
        check(name, replay(dv, name, cl), cl, 63, tol=_tol32("real", name), label="fp32 real")
