"""The horizontal shallow-water operators -- c_sw, d_sw (fxadv, the four scalar transports, xtp_u / ytp_v, the corner kinetic energy, the
divergence damping), fv_tp_2d and a2b_ord4 -- alone through the C ABI against the oracle, where the smooth C12 states of test_parity.py /
test_operator_parity.py never go (input families: tests/horizontal_case.py):

* Courant numbers up to 0.85 in both signs (strong; the suite's own are ~1e-3): the cfl-dependent half of every PPM flux at its working weight;
* 2-dx winds and a divergence input spread over the cap of the damping coefficient da_min_c max(d2_bg, min(0.20, dddmp x)) (rough): capped,
  free and floored corners in the same launch, in each of the library's four copies of the formula;
* a rectangle of exactly zero wind and constant scalars over a cube corner (still): every switch on its equality side;
* 0 / 1 fronts in pt, q_con and w (front); the Fortran model's C12 L63 restart (real), c_sw and d_sw replayed alone on one recorded call;
* every configuration switch d_sw reads -- hord 5 everywhere and one transport at a time, nord 0 - 2, the vorticity damping, the damping heat,
  the background coefficients -- on multi-strip sub-domains;
* the fp32 build of every operator against the fp64 oracle, with a bound per operator, input family and field.

Every comparison is element by element on the operator's whole output region (only the never-read cube-corner halo cell of c_sw's cell-centred
outputs is left out, as in test_parity.test_c_sw), field-scale relative per rank (max |a - b| / max |b|).  Before it, the oracle's outputs are
asserted finite and the new air mass positive.  Every case asserts from the oracle's opt-in branch counters (fv3_oracle.d_sw / c_sw / ppm),
per rank, that the switches it exists for were taken: the less-taken side of a switch covers 1 % of the counted points, a tile-edge switch
4 points of either sign on every tile edge the rank has.

Shapes (SHAPES; a marching wave owns a strip of up to 58 columns and a segment of 64 rows, FV3_SEG forces shorter segments per launch):
  c12        12 x 12, ranks 0, 3      nx < 16: the generic per-point stage B of c_sw; one partial strip
  c12_2x2    6 x 6, ranks 0 5 10 15   nx < 8: d_sw's staged wind stage (the a2b-epilogue copy of the damping coefficient on every level with a
                                      chain), asserted through its FV3_DEBUG_FD line; one rank with each of the four cube corners
  c24_2x2    12 x 12, FV3_SEG=8       one strip, two segments; the fused wind stage (fv3_wind.hip) on levels 3..5 and its frame launch on the corner
                                      rows next to the tile edges; also with FV3_DSW_WINDSTAGE=staged, FV3_DSW_DELN=arrays, FV3_DSW_MARCH=old (FV3_DEBUG_FD
                                      lines asserted); with 3 levels (sponge only: the array form of every chain) and with 9
  c72_3x3    24 x 24, FV3_SEG=8       ranks 0, 1, 4: two, one and no tile edge; three segments
  c65        65 x 65, ranks 0, 4      two strips, the second 7 columns wide; a one-row last segment
  c140_2x2   70 x 70, FV3_SEG=32      two strips, three segments (32 + 32 + 6), one cube corner per rank
  c48_3x1    16 x 48                  a non-square sub-domain, ranks with three and with two tile edges
6 levels: levels 0..2 are the sponge layers (nord 0 form of the damping, del-n chains as arrays below fd_k0), 3..5 run the chains inside the
marches.  hord 5 takes the run-time-order launches (dsw_scalars_t<..., Q4_INTERIOR / Q4_EDGE>), not the pair march of fv3_tp4x.hip.

fp64 bounds: the project's own (d_sw 1e-13, heat_source 1e-12: test_operator_parity.test_d_sw_on_recorded_inputs; divgd 1e-11: test_parity.test_d_sw;
c_sw 1e-12; fxadv / fv_tp_2d / a2b_ord4 1e-13) hold in every case; none needed a bound derived from the oracle's round-off.  Worst errors over
the module: host emulation 0 in every field of every case (the same expressions in the same order); MI355X not measured yet.  The fp64 oracle's own round-off
on the rough C65 input (against its np.longdouble run, test_fp64_oracle_round_off_on_the_rough_inputs): heat_source 5.1e-16, mfxd / mfyd
5.0e-16, delp / pt / w / q_con 4.2e-16 .. 4.7e-16, u / v 3.2e-16, the Courant numbers and area fluxes 2.8e-16 .. 3.1e-16.

fp32 bounds (TOL32): per operator, family and field 2 x the worst error against the fp64 oracle over C24 2 x 2 (nord 2: the fp32 context refuses
the del-8 coefficients on C48 and coarser) and C65 (real: C12, nord 1), measured on the host emulation (the MI355X figures are still to be added; the bounds below hold 2 x the
host emulation's).  rough and front have rows of their own: a switch that flips in fp32 moves a flux by the size of the jump (front: pt 8.6e-4,
q_con 8.4e-3 of the field).  u / v and the heat source under strong winds, and the mass fluxes of the smooth state (Courant numbers ~1e-3: the
flux is a small remainder), are held to 1e-5 .. 1e-4 of their own scale.
Measured (host emulation):
  a2b_ord4 smooth: qout 2.2e-07
  c_sw real: delpc 6.6e-08, divgd 1.3e-06, omga 1.3e-07, ptc 1.8e-07, ua 1.5e-07, uc 2.4e-07, ut 2.2e-07, vc 2.1e-07, vt 2.7e-07
  c_sw smooth: delpc 7.9e-08, divgd 1.9e-05, omga 1.4e-07, ptc 2.0e-07, ua 2.5e-07, uc 3.4e-07, ut 3.6e-07, vc 3.6e-07, vt 3.7e-07
  c_sw strong: delpc 1.2e-07, divgd 3.1e-07, omga 1.4e-07, ptc 2.1e-07, ua 1.6e-07, uc 2.6e-07, ut 2.9e-07, vc 2.0e-07, vt 2.7e-07
  d_sw front: crx 1.9e-07, cry 2.0e-07, cxd 1.9e-07, cyd 2.0e-07, delp 6.1e-06, divgd 4.1e-08, heat_source 6.7e-05, mfxd 1.5e-05, mfyd 1.3e-05, pt 8.6e-04, q_con 8.4e-03, u 2.1e-04, v 1.7e-04, w 1.9e-06, xfx 2.5e-07, yfx 2.6e-07
  d_sw real: crx 1.5e-07, cry 1.8e-07, cxd 1.1e-07, cyd 9.4e-08, delp 6.5e-08, divgd 4.8e-08, heat_source 5.9e-07, mfxd 1.9e-06, mfyd 6.4e-06, pt 2.0e-07, q_con 1.1e-07, u 1.7e-07, v 1.6e-07, w 1.4e-07, xfx 1.7e-07, yfx 1.6e-07
  d_sw rough: crx 1.9e-07, cry 2.0e-07, cxd 1.9e-07, cyd 2.0e-07, delp 6.1e-06, divgd 3.1e-08, heat_source 1.0e-06, mfxd 1.5e-05, mfyd 1.3e-05, pt 1.0e-05, q_con 2.3e-07, u 1.5e-07, v 1.6e-07, w 5.2e-07, xfx 2.5e-07, yfx 2.6e-07
  d_sw smooth: crx 1.8e-07, cry 1.8e-07, cxd 1.8e-07, cyd 1.8e-07, delp 2.7e-07, divgd 4.1e-08, heat_source 9.4e-06, mfxd 7.1e-05, mfyd 3.3e-05, pt 4.5e-07, q_con 1.6e-07, u 1.2e-06, v 4.3e-06, w 1.6e-07, xfx 2.1e-07, yfx 2.6e-07
  d_sw strong: crx 1.9e-07, cry 2.0e-07, cxd 1.9e-07, cyd 2.0e-07, delp 6.1e-06, divgd 4.1e-08, heat_source 6.7e-05, mfxd 1.5e-05, mfyd 1.3e-05, pt 1.0e-05, q_con 2.3e-07, u 2.1e-04, v 1.7e-04, w 5.2e-07, xfx 2.5e-07, yfx 2.6e-07
  fv_tp_2d_hord5 front: fx 5.4e-06, fy 6.6e-06
  fv_tp_2d_hord5 smooth: fx 5.0e-04, fy 4.5e-04
  fv_tp_2d_hord5 strong: fx 6.2e-06, fy 7.9e-06
  fv_tp_2d_hord6 front: fx 1.3e-04, fy 2.0e-04
  fv_tp_2d_hord6 smooth: fx 5.0e-04, fy 4.5e-04
  fv_tp_2d_hord6 strong: fx 2.0e-05, fy 2.0e-05
  fxadv smooth: crx 1.8e-07, cry 1.8e-07, ut 1.2e-07, vt 1.3e-07, xfx 2.1e-07, yfx 2.6e-07
  fxadv strong: crx 1.9e-07, cry 2.0e-07, ut 1.4e-07, vt 1.6e-07, xfx 2.5e-07, yfx 2.6e-07
"""
import os

import numpy as np
import pytest
import torch

import horizontal_case as hc
from helpers import Case

from fv3_oracle import a2b_ord4 as o_a2b
from fv3_oracle import c_sw as o_csw
from fv3_oracle import d_sw as o_dsw
from fv3_oracle import fvtp2d as o_tp
from fv3_oracle import ppm as o_ppm

CELLS = lambda D: D.sl(1, D.nx, 1, D.ny)  # noqa: E731
U = lambda D: D.sl(1, D.nx, 1, D.ny + 1)  # noqa: E731
V = lambda D: D.sl(1, D.nx + 1, 1, D.ny)  # noqa: E731
XF = lambda D: D.sl(1, D.nx + 1, D.jsd, D.jed)  # noqa: E731
YF = lambda D: D.sl(D.isd, D.ied, 1, D.ny + 1)  # noqa: E731
CORNERS = lambda D: D.sl(1, D.nx + 1, 1, D.ny + 1)  # noqa: E731
# d_sw's outputs and the region each is defined on (test_operator_parity.test_d_sw_on_recorded_inputs; divgd: test_parity.test_d_sw)
DSW_OUT = {"delp": CELLS, "pt": CELLS, "w": CELLS, "q_con": CELLS, "u": U, "v": V, "heat_source": CELLS, "mfxd": V, "mfyd": U, "cxd": XF, "cyd": YF, "crx": XF, "cry": YF,
           "xfx": XF, "yfx": YF, "divgd": CORNERS}
TOL_DSW = {"default": 1e-13, "heat_source": 1e-12, "divgd": 1e-11}
TOL_CSW = {"default": 1e-12}
TOL_TP = {"default": 1e-13}

TOL32 = {
    "a2b_ord4": {
        "smooth": {"qout": 4.4e-07},
    },
    "c_sw": {
        "real": {"delpc": 1.4e-07, "divgd": 2.6e-06, "omga": 2.6e-07, "ptc": 3.6e-07, "ua": 3e-07, "uc": 4.8e-07, "ut": 4.4e-07, "vc": 4.2e-07, "vt": 5.4e-07},
        "smooth": {"delpc": 1.6e-07, "divgd": 3.8e-05, "omga": 2.8e-07, "ptc": 4e-07, "ua": 5e-07, "uc": 6.8e-07, "ut": 7.2e-07, "vc": 7.2e-07, "vt": 7.4e-07},
        "strong": {"delpc": 2.4e-07, "divgd": 6.2e-07, "omga": 2.8e-07, "ptc": 4.2e-07, "ua": 3.2e-07, "uc": 5.2e-07, "ut": 5.8e-07, "vc": 4e-07, "vt": 5.4e-07},
    },
    "d_sw": {
        "front": {"crx": 3.8e-07, "cry": 4e-07, "cxd": 3.8e-07, "cyd": 4e-07, "delp": 1.3e-05, "divgd": 8.2e-08, "heat_source": 0.00014, "mfxd": 3e-05, "mfyd": 2.6e-05, "pt": 0.0018, "q_con": 0.017, "u": 0.00042, "v": 0.00034, "w": 3.8e-06, "xfx": 5e-07, "yfx": 5.2e-07},
        "real": {"crx": 3e-07, "cry": 3.6e-07, "cxd": 2.2e-07, "cyd": 1.9e-07, "delp": 1.3e-07, "divgd": 9.6e-08, "heat_source": 1.2e-06, "mfxd": 3.8e-06, "mfyd": 1.3e-05, "pt": 4e-07, "q_con": 2.2e-07, "u": 3.4e-07, "v": 3.2e-07, "w": 2.8e-07, "xfx": 3.4e-07, "yfx": 3.2e-07},
        "rough": {"crx": 3.8e-07, "cry": 4e-07, "cxd": 3.8e-07, "cyd": 4e-07, "delp": 1.3e-05, "divgd": 6.2e-08, "heat_source": 2e-06, "mfxd": 3e-05, "mfyd": 2.6e-05, "pt": 2e-05, "q_con": 4.6e-07, "u": 3e-07, "v": 3.2e-07, "w": 1.1e-06, "xfx": 5e-07, "yfx": 5.2e-07},
        "smooth": {"crx": 3.6e-07, "cry": 3.6e-07, "cxd": 3.6e-07, "cyd": 3.6e-07, "delp": 5.4e-07, "divgd": 8.2e-08, "heat_source": 1.9e-05, "mfxd": 0.00015, "mfyd": 6.6e-05, "pt": 9e-07, "q_con": 3.2e-07, "u": 2.4e-06, "v": 8.6e-06, "w": 3.2e-07, "xfx": 4.2e-07, "yfx": 5.2e-07},
        "strong": {"crx": 3.8e-07, "cry": 4e-07, "cxd": 3.8e-07, "cyd": 4e-07, "delp": 1.3e-05, "divgd": 8.2e-08, "heat_source": 0.00014, "mfxd": 3e-05, "mfyd": 2.6e-05, "pt": 2e-05, "q_con": 4.6e-07, "u": 0.00042, "v": 0.00034, "w": 1.1e-06, "xfx": 5e-07, "yfx": 5.2e-07},
    },
    "fv_tp_2d_hord5": {
        "front": {"fx": 1.1e-05, "fy": 1.4e-05},
        "smooth": {"fx": 0.001, "fy": 0.0009},
        "strong": {"fx": 1.3e-05, "fy": 1.6e-05},
    },
    "fv_tp_2d_hord6": {
        "front": {"fx": 0.00026, "fy": 0.0004},
        "smooth": {"fx": 0.001, "fy": 0.0009},
        "strong": {"fx": 4e-05, "fy": 4e-05},
    },
    "fxadv": {
        "smooth": {"crx": 3.6e-07, "cry": 3.6e-07, "ut": 2.4e-07, "vt": 2.6e-07, "xfx": 4.2e-07, "yfx": 5.2e-07},
        "strong": {"crx": 3.8e-07, "cry": 4e-07, "ut": 2.8e-07, "vt": 3.2e-07, "xfx": 5e-07, "yfx": 5.2e-07},
    },
}


@pytest.fixture(params=["hostemu", pytest.param("hip:gfx950", marks=pytest.mark.gpu)])
def backend(request):
    request.getfixturevalue("hostemu" if request.param == "hostemu" else "gpu_backend")
    return request.param


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
    for m in (o_dsw, o_csw, o_ppm):
        m.enable_counters(True)
    yield
    for m in (o_dsw, o_csw, o_ppm):
        m.enable_counters(False)


@pytest.fixture(scope="module")
def data():
    from test_restart_six_tiles import GOLDEN

    return np.load(GOLDEN)


# ---------------------------------------------------------------------------------------------------------------------------
# one operator alone: the library through the C ABI, the oracle per rank with the branch counts of that rank, element-wise errors
# ---------------------------------------------------------------------------------------------------------------------------
def _pad(a):
    return np.concatenate([a, a[:, :, -1:]], axis=2)


def _sync(backend):
    if backend != "hostemu":
        torch.cuda.synchronize()


def _reset():
    for m in (o_dsw, o_csw, o_ppm):
        m.reset_counters()


def _counted():
    n = dict(o_dsw.counters())
    n.update(o_csw.counters())
    n.update(o_ppm.counters())
    return n


def errors(pairs, worst=None):
    """pairs: (field, rank, library values, oracle values) on the operator's whole output region -> worst field-scale relative error
    per field (max |a - b| / max |b| per rank); both sides finite everywhere"""
    worst = {} if worst is None else worst
    for name, r, got, want in pairs:
        got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
        assert np.all(np.isfinite(want)), f"{name} rank {r}: the oracle is not finite"
        assert np.all(np.isfinite(got)), f"{name} rank {r}: non-finite"
        sc = np.abs(want).max()
        e = float(np.abs(got - want).max())
        worst[name] = max(worst.get(name, 0.0), e / sc if sc > 0 else e)
    return worst


def check(label, worst, tol):
    print(f"{label}:", {k: f"{v:.1e}" for k, v in worst.items()})
    bad = {k: v for k, v in worst.items() if not v <= tol.get(k, tol.get("default"))}
    assert not bad, f"{label}: field-scale relative errors above tolerance: {bad} (all: {worst}; bounds: {tol})"
    return worst


def oracle_d_sw(cs, ins, dt, dtype=np.float64):
    """the oracle's d_sw per rank on copies of ``ins``: ([outputs per rank], [branch counts per rank]); finite, new delp positive"""
    col = o_dsw.get_column_namelist(cs.cfg, cs.nz)
    wants, counts = [], []
    for r, (D, x) in enumerate(zip(cs.doms, ins)):
        w = {k: np.array(v, dtype=dtype) for k, v in x.items() if k in hc.D_SW_IN}
        for n in ("delpc", "crx", "cry", "xfx", "yfx", "heat_source", "diss_est"):
            w[n] = np.zeros_like(w["u"])
        w["zh"] = None
        _reset()
        o_dsw.d_sw(D, cs.cfg, col, *[w[n] for n in hc.D_SW_ARGS], dt)
        counts.append(_counted())
        for n, R in DSW_OUT.items():
            assert np.all(np.isfinite(w[n][R(D)])), f"oracle {n} rank {r}: non-finite"
        assert w["delp"][CELLS(D)].min() > 0.0, f"oracle delp rank {r}: not positive"
        wants.append(w)
    return wants, counts


def library_d_sw(cs, ins, dt, backend):
    nz = cs.nz
    Q = {n: cs.q([_pad(x[n]) for x in ins]) if n in hc.D_SW_IN else cs.q() for n in hc.D_SW_ARGS}
    cs.sf.call("d_sw", *[Q[n].fref for n in hc.D_SW_ARGS], dt)
    _sync(backend)
    return [{n: Q[n].numpy(r)[:, :, :nz] for n in DSW_OUT} for r in range(len(ins))]


def run_d_sw(cs, ins, dt, backend):
    wants, counts = oracle_d_sw(cs, ins, dt)
    gots = library_d_sw(cs, ins, dt, backend)
    worst = errors((n, r, gots[r][n][R(D)], wants[r][n][R(D)]) for r, D in enumerate(cs.doms) for n, R in DSW_OUT.items())
    return worst, counts, wants


def _ring1_pair(D, name, got, want):
    """c_sw's cell-centred outputs on the compute domain + 1 ring, without the never-read cube-corner halo cell (test_parity.test_c_sw)"""
    got, want = got.copy(), want.copy()
    for (ci, cj), has in (((0, 0), D.sw), ((-1, 0), D.se), ((-1, -1), D.ne), ((0, -1), D.nw)):
        if has:
            got[ci, cj] = want[ci, cj] = 0.0
    return got, want


def run_c_sw(cs, ins, dt2, backend):
    """c_sw alone: outputs and regions of test_parity.test_c_sw"""
    nz = cs.nz
    Q = {n: cs.q([x[n] for x in ins]) for n in hc.C_SW_IN}
    ut, vt, divgd, delpc, ptc = (cs.q() for _ in range(5))
    cs.sf.call("c_sw", *[Q[n].fref for n in hc.C_SW_IN[:9]], ut.fref, vt.fref, divgd.fref, Q["omga"].fref, delpc.fref, ptc.fref, dt2)
    _sync(backend)
    pairs, counts = [], []
    for r, (D, x) in enumerate(zip(cs.doms, ins)):
        s = {k: v[:, :, :nz].copy() for k, v in x.items()}
        o_ut, o_vt, o_div = (np.zeros_like(s["u"]) for _ in range(3))
        _reset()
        e_delpc, e_ptc = o_csw.c_sw(D, *[s[n] for n in hc.C_SW_IN[:9]], o_ut, o_vt, o_div, s["omga"], dt2, nord=cs.cfg.nord)
        counts.append(_counted())
        C1 = D.sl(0, D.nx + 1, 0, D.ny + 1)
        assert e_delpc[C1].min() > 0.0, f"oracle delpc rank {r}: not positive"
        for name, q, want, R in (("delpc", delpc, e_delpc, C1), ("ptc", ptc, e_ptc, C1), ("omga", Q["omga"], s["omga"], C1), ("divgd", divgd, o_div, CORNERS(D)),
                                 ("uc", Q["uc"], s["uc"], V(D)), ("vc", Q["vc"], s["vc"], U(D)), ("ut", ut, o_ut, D.sl(0, D.nx + 2, 0, D.ny + 1)),
                                 ("vt", vt, o_vt, D.sl(0, D.nx + 1, 0, D.ny + 2)), ("ua", Q["ua"], s["ua"], C1)):
            if name == "divgd" and cs.cfg.nord == 0:
                continue  # (c_sw forms the corner divergence for the damping chains only)
            got, wnt = q.numpy(r)[:, :, :nz][R], want[R]
            if name in ("delpc", "ptc", "omga"):
                got, wnt = _ring1_pair(D, name, got, wnt)
            pairs.append((name, r, got, wnt))
    return errors(pairs), counts


# ---------------------------------------------------------------------------------------------------------------------------
# what the counters must show
# ---------------------------------------------------------------------------------------------------------------------------
def total(counts):
    return {k: sum(n[k] for n in counts) for k in counts[0]}


def two_sided(n, names, what, share=0.01):
    """every side of a switch covers at least ``share`` of the counted points"""
    tot = sum(n[k] for k in names)
    assert tot > 0, f"{what}: never evaluated"
    low = {k: n[k] for k in names if n[k] < share * tot or n[k] == 0}
    assert not low, f"{what}: sides below {share:.0%} of {tot} points: {low}"


def edges_two_sided(cs, counts, prefixes):
    """tile-edge switches: on every tile edge a rank has, at least 4 points of either sign.  prefixes: {edge letter: counter prefix}"""
    for D, n in zip(cs.doms, counts):
        for e, has in (("w", D.west), ("e", D.east), ("s", D.south), ("n", D.north)):
            for p in prefixes.get(e, ()) if has else ():
                assert n[p + "_pos"] >= 4 and n[p + "_neg"] >= 4, f"rank {D.grid.rank if hasattr(D.grid, 'rank') else '?'}: {p}: {n[p + '_pos']} / {n[p + '_neg']}"


FXADV_EDGES = {"w": ("fxadv_ut_w",), "e": ("fxadv_ut_e",), "s": ("fxadv_vt_s",), "n": ("fxadv_vt_n",)}
DIV0_EDGES = {"w": ("div0_vort_w",), "e": ("div0_vort_e",), "s": ("div0_ptc_s",), "n": ("div0_ptc_n",)}
CSW_EDGES = {"w": ("uc_w", "ke_w"), "e": ("uc_e", "ke_e"), "s": ("vc_s", "vort_s"), "n": ("vc_n", "vort_n")}


def assert_strong(cs, ins, dt, counts, lo=0.5, hi=0.9):
    top, both = hc.max_courant(cs, ins, dt)
    assert lo <= top <= hi and both, f"max Courant number {top:.3f}, both signs: {both}"
    n = total(counts)
    two_sided(n, ("cfl_pos", "cfl_nonpos"), "sign of the Courant number")
    assert n["cfl_gt_half"] >= 0.01 * (n["cfl_pos"] + n["cfl_nonpos"]), f"|c| > 0.5 at {n['cfl_gt_half']} of {n['cfl_pos'] + n['cfl_nonpos']} fluxes"
    edges_two_sided(cs, counts, FXADV_EDGES)


def assert_hord(cs, n):
    for h in sorted({cs.cfg.hord_dp, cs.cfg.hord_tm, cs.cfg.hord_vt, cs.cfg.hord_mt}):
        two_sided(n, (f"smt5_true_hord{h}", f"smt5_false_hord{h}"), f"smt5 of hord {h}")


# ---------------------------------------------------------------------------------------------------------------------------
# 1. d_sw alone, fp64
# ---------------------------------------------------------------------------------------------------------------------------
DT = 60.0
CORNER_RANKS = (0, 5, 10, 15)  # 2 x 2 layout: tile 0 SW, tile 1 SE (rank 5), tile 2 NE (rank 10), tile 3 NW (rank 15) cube corners
# name: (cells per tile, layout, ranks, FV3_SEG, levels)
SHAPES = {
    "c12": (12, (1, 1), (0, 3), None, 6),
    "c12_2x2": (12, (2, 2), CORNER_RANKS, None, 6),
    "c24_2x2": (24, (2, 2), CORNER_RANKS, "8", 6),
    "c24_2x2_L3": (24, (2, 2), (0, 10), "8", 3),
    "c24_2x2_L9": (24, (2, 2), (5, 15), "8", 9),
    "c72_3x3": (72, (3, 3), (0, 1, 4), "8", 6),
    "c65": (65, (1, 1), (0, 4), None, 6),
    "c140_2x2": (140, (2, 2), CORNER_RANKS, "32", 6),
    "c48_3x1": (48, (3, 1), (0, 1, 2), None, 6),
}


def case(shape, backend, monkeypatch, cfg_kw=None, dtype=torch.float64):
    n, layout, ranks, seg, nz = SHAPES[shape]
    if seg:
        monkeypatch.setenv("FV3_SEG", seg)
    return Case(n, layout, ranks, nz=nz, backend=backend, cfg_kw=dict(n_split=1, **(cfg_kw or {})), dtype=dtype)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_d_sw_on_strong_winds_matches_the_oracle(backend, counts, monkeypatch, shape):
    """Courant numbers up to 0.8 in both signs, every shape: the cfl-dependent half of every PPM flux at its working weight"""
    cs = case(shape, backend, monkeypatch)
    ins = hc.strong(cs, DT)
    worst, n, _ = run_d_sw(cs, ins, DT, backend)
    assert_strong(cs, ins, DT, n)
    assert_hord(cs, total(n))
    check(f"d_sw strong {shape}", worst, TOL_DSW)


def assert_damping(n, form, sides):
    """the coefficient da_min_c max(d2_bg, min(0.20, x)) of one form: each of ``sides`` covers 1 % of the form's corners, the others none"""
    names = [f"damp{form}_{s}" for s in ("capped", "floored", "free")]
    tot = sum(n[k] for k in names)
    assert tot > 0, f"damping form {form}: never evaluated"
    for s in ("capped", "floored", "free"):
        if s in sides:
            assert n[f"damp{form}_{s}"] >= 0.01 * tot, f"damping form {form}: {s} at {n[f'damp{form}_{s}']} of {tot} corners ({ {k: n[k] for k in names} })"


# (shape, environment): the nx < 8 ranks of C12 2 x 2 and FV3_DSW_WINDSTAGE=staged send every level with a chain to the staged copy of the coefficient
# (a2b epilogue); the others run the fused march (fv3_wind.hip) with the frame launch on the three corner rows / columns next to a tile edge
ROUGH = [("c12", {}), ("c12_2x2", {}), ("c24_2x2", {}), ("c24_2x2", {"FV3_DSW_WINDSTAGE": "staged"}), ("c24_2x2", {"FV3_DSW_DELN": "arrays"}), ("c24_2x2", {"FV3_DSW_MARCH": "old"}),
         ("c65", {}), ("c140_2x2", {})]
DEBUG_LINE = {"": ("fd_k0 = 3 of 6", "fused wind stage on levels 3..5 of 6", "pair march, role"), "FV3_DSW_WINDSTAGE": ("fused wind stage on levels 6..5 of 6",),
              "FV3_DSW_DELN": ("fd_k0 = 6 of 6",), "FV3_DSW_MARCH": ()}


@pytest.mark.parametrize("shape, env", ROUGH, ids=lambda v: v if isinstance(v, str) else ",".join(f"{k}={x}" for k, x in v.items()) or "default")
def test_d_sw_on_rough_winds_takes_every_side_of_the_damping_coefficient(backend, counts, monkeypatch, capfd, shape, env):
    """2-dx winds and a divergence input spread over the cap: the higher-order coefficient capped, free and floored (d2_bg = 0.05) in
    the same launch, in its staged, frame and fused copies; the forms behind per-call switches, asserted through the FV3_DEBUG_FD lines"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("FV3_DEBUG_FD", "1")
    cs = case(shape, backend, monkeypatch, dict(d2_bg=0.05))
    ins = hc.rough(cs, DT)
    capfd.readouterr()
    worst, n, _ = run_d_sw(cs, ins, DT, backend)
    err = capfd.readouterr().err
    if shape == "c24_2x2":
        for line in DEBUG_LINE[next(iter(env), "")]:
            assert line in err, (line, err)
        if "FV3_DSW_MARCH" in env:
            assert "pair march, role" not in err, err
    if shape == "c12_2x2":
        assert "fused wind stage on levels 6..5 of 6" in err, err  # (nx < 8: staged)
    assert_damping(total(n), "n", ("capped", "floored", "free"))
    edges_two_sided(cs, n, FXADV_EDGES)
    check(f"d_sw rough {shape} {env}", worst, TOL_DSW)


@pytest.mark.parametrize("shape", ["c12_2x2", "c65"])
def test_d_sw_on_a_still_rectangle_matches_the_oracle(backend, counts, monkeypatch, shape):
    """exactly zero wind and constant scalars over the SW cube corner: c == 0, bl == br == 0 -- every switch on its equality side"""
    cs = case(shape, backend, monkeypatch)
    ins = hc.still(cs)
    worst, n, wants = run_d_sw(cs, ins, DT, backend)
    D, w, box = cs.doms[0], wants[0], hc.still_box(cs.doms[0])
    assert D.sw
    inner = (slice(hc.NH, box[0].stop - 1), slice(hc.NH, box[1].stop - 1))  # faces with still cells on both sides
    assert inner[0].stop > inner[0].start
    assert np.all(w["crx"][inner] == 0.0) and np.all(w["cry"][inner] == 0.0), "the Courant numbers of the still rectangle are not exactly zero"
    assert n[0]["cfl_nonpos"] > 0
    far = (slice(hc.NH, box[0].stop - 4), slice(hc.NH, box[1].stop - 4))  # cells whose PPM stencils stay inside the rectangle
    if far[0].stop > far[0].start:
        assert np.all(w["pt"][far] == 300.0) and np.all(w["delp"][far] == 1000.0), "the still scalars moved"
    check(f"d_sw still {shape}", worst, TOL_DSW)


@pytest.mark.parametrize("shape", ["c24_2x2", "c65"])
def test_d_sw_on_fronts_matches_the_oracle(backend, counts, monkeypatch, shape):
    """0 / 1 fronts in pt, q_con and w under Courant numbers up to 0.85: the smt5 switch of the scalar transports on both sides"""
    cs = case(shape, backend, monkeypatch)
    ins = hc.front(cs, DT)
    worst, n, _ = run_d_sw(cs, ins, DT, backend)
    assert_strong(cs, ins, DT, n)
    assert_hord(cs, total(n))
    check(f"d_sw front {shape}", worst, TOL_DSW)


_REAL = {}


def real_calls(data):
    """one recorded oracle call (two sub-steps of 60 s) on the six restart tiles: c_sw's and d_sw's call records"""
    if not _REAL:
        from test_column_solver_edges import real_calls as rc

        part, cfg, grids, calls = rc(data, (1, 1))
        _REAL.update(part=part, cfg=cfg, grids=grids, calls=calls)
    return _REAL


def _real_case(data, backend, dtype=torch.float64, cfg_kw=None):
    import copy

    from test_operator_parity import Dev

    R = real_calls(data)
    cfg = copy.copy(R["cfg"])
    for k, v in (cfg_kw or {}).items():
        setattr(cfg, k, v)
    return R, cfg, Dev(backend, R["grids"], cfg, dtype=dtype)


def run_real_d_sw(data, backend, dtype=torch.float64, cfg_kw=None):
    R, cfg, dv = _real_case(data, backend, dtype, cfg_kw)
    nr, nz = R["part"].total_ranks, 63
    cl = R["calls"]["d_sw"][-nr:]  # (the last sub-step: the accumulators hold the first one's fluxes)
    names = list(hc.D_SW_ARGS)
    Q = {n: dv.q([c["ins"][2 + i] for c in cl]) for i, n in enumerate(names)}
    dt = float(cl[0]["ins"][2 + len(names)])
    dv.sf.call("d_sw", *[Q[n].fref for n in names], dt)
    _sync(backend)
    col = o_dsw.get_column_namelist(cfg, nz)
    pairs = []
    for r, c in enumerate(cl):
        D = c["D"]
        w = [a.copy() if isinstance(a, np.ndarray) else a for a in c["ins"][2 : 2 + len(names)]]
        o_dsw.d_sw(D, cfg, col, *w, dt)
        want = dict(zip(names, w))
        assert want["delp"][CELLS(D)][:, :, :nz].min() > 0.0
        pairs += [(n, r, Q[n].numpy(r)[Rg(D)][:, :, :nz], want[n][Rg(D)][:, :, :nz]) for n, Rg in DSW_OUT.items()]
    return errors(pairs)


def run_real_c_sw(data, backend, dtype=torch.float64, cfg_kw=None):
    R, cfg, dv = _real_case(data, backend, dtype, cfg_kw)
    nr, nz = R["part"].total_ranks, 63
    cl = R["calls"]["c_sw"][-nr:]
    # c_sw(D, delp, pt, u, v, w, uc, vc, ua, va, ut, vt, divgd, omga, dt2, nord)
    names = ["delp", "pt", "u", "v", "w", "uc", "vc", "ua", "va", "ut", "vt", "divgd", "omga"]
    Q = {n: dv.q([c["ins"][i] for c in cl]) for i, n in enumerate(names)}
    delpc, ptc = dv.q([np.zeros_like(c["ins"][0]) for c in cl]), dv.q([np.zeros_like(c["ins"][0]) for c in cl])
    dt2 = float(cl[0]["ins"][13])
    dv.sf.call("c_sw", *[Q[n].fref for n in names], delpc.fref, ptc.fref, dt2)
    _sync(backend)
    pairs = []
    for r, c in enumerate(cl):
        D = c["D"]
        w = dict(zip(names, [a.copy() for a in c["ins"][:13]]))
        e_delpc, e_ptc = o_csw.c_sw(D, *[w[n] for n in names], dt2, nord=cfg.nord)
        C1 = D.sl(0, D.nx + 1, 0, D.ny + 1)
        assert e_delpc[C1].min() > 0.0
        for name, q, want, Rg in (("delpc", delpc, e_delpc, C1), ("ptc", ptc, e_ptc, C1), ("omga", Q["omga"], w["omga"], C1), ("divgd", Q["divgd"], w["divgd"], CORNERS(D)),
                                  ("uc", Q["uc"], w["uc"], V(D)), ("vc", Q["vc"], w["vc"], U(D)), ("ut", Q["ut"], w["ut"], D.sl(0, D.nx + 2, 0, D.ny + 1)),
                                  ("vt", Q["vt"], w["vt"], D.sl(0, D.nx + 1, 0, D.ny + 2)), ("ua", Q["ua"], w["ua"], C1)):
            got, wnt = q.numpy(r)[Rg][:, :, :nz], want[Rg][:, :, :nz]
            if name in ("delpc", "ptc", "omga"):
                got, wnt = _ring1_pair(D, name, got, wnt)
            pairs.append((name, r, got, wnt))
    return errors(pairs)


def test_d_sw_and_c_sw_on_the_real_state_match_the_oracle(backend, data):
    """the Fortran model's C12 L63 restart: terrain, moisture and winds of a real run, c_sw and d_sw replayed alone"""
    check("c_sw real", run_real_c_sw(data, backend), TOL_CSW)
    check("d_sw real", run_real_d_sw(data, backend), TOL_DSW)


# ---- the configuration matrix on the multi-strip shapes
H5 = dict(hord_dp=5, hord_tm=5, hord_vt=5, hord_mt=5)
CONFIGS = [{}, H5, dict(hord_dp=5), dict(hord_tm=5), dict(hord_vt=5), dict(hord_mt=5), dict(nord=0), dict(nord=1), dict(nord=2), dict(do_vort_damp=False), dict(vtdm4=0.0),
           dict(d_con=0.0), dict(d2_bg=0.05), dict(d4_bg=0.0), dict(dddmp=0.0), dict(ke_bg=1e-4), dict(n_sponge=0)]


@pytest.mark.parametrize("shape", ["c65", "c140_2x2"])
@pytest.mark.parametrize("kw", CONFIGS, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()) or "default")
def test_d_sw_config_matrix_on_multi_strip_shapes_matches_the_oracle(backend, counts, monkeypatch, shape, kw):
    """every configuration switch d_sw reads, on two strips (C65: the second partial, a one-row last segment; C140 2 x 2: 70 cells, 32-row
    segments, one cube corner per rank) under rough winds at Courant numbers up to 0.85.  nord = 0 gets the stronger checkerboard its
    coefficient needs to pass the cap at 1 % of the corners."""
    cs = case(shape, backend, monkeypatch, kw)
    ins = hc.rough(cs, DT, amp_top=0.6 if kw.get("nord") == 0 else 0.15, cfl=0.85)
    worst, counts_, _ = run_d_sw(cs, ins, DT, backend)
    n = total(counts_)
    assert_strong(cs, ins, DT, counts_)
    assert_hord(cs, n)
    if kw.get("nord") == 0:
        assert n["dampn_capped"] + n["dampn_free"] + n["dampn_floored"] == 0
        assert_damping(n, "0", ("capped", "floored", "free"))
        edges_two_sided(cs, counts_, DIV0_EDGES)
    elif kw.get("dddmp") == 0.0:
        assert n["dampn_capped"] == 0 and n["dampn_free"] == 0 and n["dampn_floored"] > 0
    else:
        assert_damping(n, "n", ("capped", "free", "floored") if "d2_bg" in kw else ("capped", "free"))
    off = kw.get("do_vort_damp") is False or kw.get("vtdm4") == 0.0  # (vtdm4 = 0 alone leaves the two lowest sponge levels their own damp_vt)
    assert (n["damp_vt_off"] > 0) == off and (n["damp_vt_on"] == 0) == (kw.get("do_vort_damp") is False), n
    assert n["damp_w_on"] > 0
    assert (n["d_con_on"] == 0) == (kw.get("d_con") == 0.0) and n["d_con_off"] > 0, n
    check(f"d_sw {shape} {kw}", worst, TOL_DSW)


def test_fp64_oracle_round_off_on_the_rough_inputs(hostemu, monkeypatch):
    """The reference's own error where the outputs are remainders of cancelling terms (u / v, the heat source under the 2-dx winds): d_sw of
    the fp64 oracle against the same oracle run in np.longdouble on the same arrays.  A correct library carries a round-off of the same
    size, so a bound in use must at least cover the oracle's: the fp64 oracle stays inside TOL_DSW against its long-double self (measured
    values: module docstring; a field that exceeded its bound would get 4 x its own figure)."""
    assert np.finfo(np.longdouble).eps < 1e-18  # (an extended type: where long double is double this measures nothing)
    cs = case("c65", "hostemu", monkeypatch, dict(d2_bg=0.05))
    ins = hc.rough(cs, DT, cfl=0.85)
    w64, _ = oracle_d_sw(cs, ins, DT)
    w80, _ = oracle_d_sw(cs, ins, DT, dtype=np.longdouble)
    assert all(w80[0][n].dtype == np.longdouble for n in DSW_OUT)
    worst = errors((n, r, w64[r][n][R(D)], w80[r][n][R(D)]) for r, D in enumerate(cs.doms) for n, R in DSW_OUT.items())
    check("fp64 oracle against long double, d_sw rough c65", worst, TOL_DSW)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. c_sw alone, fp64: the sizes of test_parity.test_c_sw and C65
# ---------------------------------------------------------------------------------------------------------------------------
DT2 = 30.0
CSW_SHAPES = {"c12": (12, (1, 1), (0, 3), None, 4), "c12_2x2": (12, (2, 2), CORNER_RANKS, None, 4), "c24": (24, (1, 1), (0, 4), None, 4), "c48_2x2": (48, (2, 2), CORNER_RANKS, "8", 4),
              "c72": (72, (1, 1), (2,), "16", 4), "c65": (65, (1, 1), (0, 4), None, 4)}
SHAPES.update({"csw_" + k: v for k, v in CSW_SHAPES.items()})


def assert_c_sw_switches(cs, counts_):
    n = total(counts_)
    for f in ("flux_x", "flux_y", "fyv", "fxv"):
        two_sided(n, (f + "_pos", f + "_neg"), f"c_sw {f}")
    edges_two_sided(cs, counts_, CSW_EDGES)


@pytest.mark.parametrize("nord", [0, 3])
@pytest.mark.parametrize("shape", list(CSW_SHAPES))
def test_c_sw_on_strong_winds_matches_the_oracle(backend, counts, monkeypatch, shape, nord):
    """D-grid winds at dt2 |u| / dx up to 0.2 in both signs on every tile edge: both upwind sides of the mass / heat / w fluxes, of the
    vorticity fluxes and of every tile-edge formula, with and without the corner divergence (nord 0)"""
    cs = case("csw_" + shape, backend, monkeypatch, dict(nord=nord))
    worst, n = run_c_sw(cs, hc.strong_c(cs, DT2), DT2, backend)
    assert_c_sw_switches(cs, n)
    check(f"c_sw strong {shape} nord {nord}", worst, TOL_CSW)


@pytest.mark.parametrize("shape", ["c12_2x2", "c65"])
def test_c_sw_on_a_still_rectangle_matches_the_oracle(backend, counts, monkeypatch, shape):
    """zero winds over the SW cube corner: every upwind choice of the rectangle on its equality side (wind > 0 is false)"""
    cs = case("csw_" + shape, backend, monkeypatch)
    ins = hc.still_c(cs)
    worst, n = run_c_sw(cs, ins, DT2, backend)
    assert cs.doms[0].sw and n[0]["uc_w_neg"] >= 4 and n[0]["vc_s_neg"] >= 4 and n[0]["ke_w_neg"] >= 4 and n[0]["vort_s_neg"] >= 4, n[0]
    check(f"c_sw still {shape}", worst, TOL_CSW)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. fxadv, fv_tp_2d, a2b_ord4 alone, fp64
# ---------------------------------------------------------------------------------------------------------------------------
FXADV_OUT = {"crx": XF, "xfx": XF, "ut": XF, "cry": YF, "yfx": YF, "vt": YF}


def run_fxadv(cs, ins, dt, backend):
    Q = {k: cs.q([_pad(x[k]) for x in ins]) for k in ("uc", "vc")}
    out = {k: cs.q() for k in ("crx", "cry", "xfx", "yfx", "ut", "vt")}
    cs.sf.call("fxadv", Q["uc"].fref, Q["vc"].fref, *[out[k].fref for k in ("crx", "cry", "xfx", "yfx", "ut", "vt")], dt)
    _sync(backend)
    pairs, counts_, wants = [], [], []
    for r, (D, x) in enumerate(zip(cs.doms, ins)):
        w = {k: np.zeros_like(x["uc"]) for k in out}
        _reset()
        w["ra_x"], w["ra_y"] = o_dsw.fxadv(D, x["uc"].copy(), x["vc"].copy(), *[w[k] for k in ("crx", "cry", "xfx", "yfx", "ut", "vt")], dt)
        counts_.append(_counted())
        wants.append(w)
        pairs += [(k, r, out[k].numpy(r)[:, :, : cs.nz][R(D)], w[k][R(D)]) for k, R in FXADV_OUT.items()]
    return errors(pairs), counts_, wants


TP_SHAPES = ["c12_2x2", "c24_2x2", "c65", "c48_3x1"]


@pytest.mark.parametrize("shape", TP_SHAPES)
def test_fxadv_on_strong_winds_matches_the_oracle(backend, counts, monkeypatch, shape):
    cs = case(shape, backend, monkeypatch)
    ins = hc.strong(cs, DT)
    worst, n, _ = run_fxadv(cs, ins, DT, backend)
    edges_two_sided(cs, n, FXADV_EDGES)
    top, both = hc.max_courant(cs, ins, DT)
    assert 0.5 <= top <= 0.9 and both
    check(f"fxadv strong {shape}", worst, TOL_TP)


def _tp_field(cs, ins, family):
    if family == "front":
        from test_tracer_remap_edges import _front

        return [x["pt"] * (1.0 + 0.15 * _front(g, cs.nz)) for g, x in zip(cs.grids, ins)]  # (the front alone is constant nearly everywhere: smt5 true below 1 %)
    return [x["pt"].copy() for x in ins]


def run_fv_tp_2d(cs, ins, q, F, hord, backend):
    """plain, damped, mass-flux weighted + damped (the three forms of test_parity.test_fxadv_and_fv_tp_2d) on the fluxes ``F`` of the oracle's
    fxadv: worst errors of fx / fy over the forms, and the branch counts summed over forms and ranks"""
    nz = cs.nz
    mass = [x["delp"] for x in ins]
    dev = {k: cs.q([_pad(f[k]) for f in F]) for k in ("crx", "cry", "xfx", "yfx")}
    Qm = cs.q([_pad(a) for a in mass])
    mfx, mfy = cs.q([_pad(f["xfx"] * 1.1) for f in F]), cs.q([_pad(f["yfx"] * 0.9) for f in F])
    worst, tot = {}, None
    for variant in range(3):
        Qq, fx, fy = cs.q([_pad(a) for a in q]), cs.q(), cs.q()
        extra = [(None, None, None, hord, -1, 0.0), (None, None, None, hord, 2, 0.06), (mfx.fref, mfy.fref, Qm.fref, hord, 2, 0.06)][variant]
        cs.sf.call("fv_tp_2d", Qq.fref, *[dev[k].fref for k in ("crx", "cry", "xfx", "yfx")], fx.fref, fy.fref, *extra)
        _sync(backend)
        for r, (D, f) in enumerate(zip(cs.doms, F)):
            kw = [dict(), dict(nord=2, damp_c=0.06), dict(mfx=f["xfx"] * 1.1, mfy=f["yfx"] * 0.9, mass=mass[r], nord=2, damp_c=0.06)][variant]
            _reset()
            efx, efy = o_tp.fv_tp_2d(D, q[r].copy(), f["crx"], f["cry"], f["xfx"], f["yfx"], f["ra_x"], f["ra_y"], hord, **kw)
            tot = _counted() if tot is None else {k: v + tot[k] for k, v in _counted().items()}
            errors([("fx", r, fx.numpy(r)[:, :, :nz][V(D)], efx[V(D)]), ("fy", r, fy.numpy(r)[:, :, :nz][U(D)], efy[U(D)])], worst)
    return worst, tot


@pytest.mark.parametrize("hord", [5, 6])
@pytest.mark.parametrize("family", ["strong", "front"])
@pytest.mark.parametrize("shape", TP_SHAPES)
def test_fv_tp_2d_on_strong_winds_and_fronts_matches_the_oracle(backend, counts, monkeypatch, shape, family, hord):
    """the three forms, order 5 and 6, on the smooth pt and on pt with the 0 / 1 front as a 15 % jump: smt5 on both sides, Courant numbers of
    both signs and above 0.5"""
    cs = case(shape, backend, monkeypatch)
    ins = hc.strong(cs, DT)
    _, _, F = run_fxadv(cs, ins, DT, backend)
    worst, tot = run_fv_tp_2d(cs, ins, _tp_field(cs, ins, family), F, hord, backend)
    two_sided(tot, (f"smt5_true_hord{hord}", f"smt5_false_hord{hord}"), f"smt5 of hord {hord}")
    two_sided(tot, ("cfl_pos", "cfl_nonpos"), "sign of the Courant number")
    assert tot["cfl_gt_half"] >= 0.01 * (tot["cfl_pos"] + tot["cfl_nonpos"])
    check(f"fv_tp_2d {family} {shape} hord {hord}", worst, TOL_TP)


def _a2b_input(cs):
    """the smooth pt plus a 2-dx checkerboard of 1 % of it"""
    out = []
    for r, s in enumerate(cs.states):
        i, j, _ = hc._index(cs, r)
        a = s["pt"][:, :, : cs.nz]
        out.append(a * (1.0 + 0.01 * np.where((i + j) % 2 == 0, 1.0, -1.0)))
    return out


@pytest.mark.parametrize("shape", ["c12_2x2", "c24_2x2", "c65", "c140_2x2", "c48_3x1"])
def test_a2b_ord4_on_a_checkerboard_matches_the_oracle(backend, monkeypatch, shape):
    cs = case(shape, backend, monkeypatch)
    qin = _a2b_input(cs)
    Q, O = cs.q([_pad(a) for a in qin]), cs.q()
    cs.sf.call("a2b_ord4", Q.fref, O.fref, 0, cs.nz, 0)
    _sync(backend)
    worst = errors(("qout", r, O.numpy(r)[:, :, : cs.nz][CORNERS(D)], o_a2b.a2b_ord4(D, qin[r].copy())[CORNERS(D)]) for r, D in enumerate(cs.doms))
    check(f"a2b_ord4 {shape}", worst, TOL_TP)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the fp32 build against the fp64 oracle
# ---------------------------------------------------------------------------------------------------------------------------
def tol32(op, family):
    return TOL32[op][family]


# the fp32 context refuses damping coefficients (damp da_min)^(nord + 1) beyond its range: the default del-8 chain on C48 and coarser
FP32_SHAPES = {"c24_2x2": dict(nord=2), "c65": {}}
D_SW_FAMILIES = {"smooth": lambda cs: hc.smooth(cs), "strong": lambda cs: hc.strong(cs, DT), "rough": lambda cs: hc.rough(cs, DT, cfl=0.85), "front": lambda cs: hc.front(cs, DT)}


@pytest.mark.parametrize("family", list(D_SW_FAMILIES))
@pytest.mark.parametrize("shape", list(FP32_SHAPES))
def test_fp32_d_sw_tracks_the_fp64_oracle(backend32, monkeypatch, shape, family):
    cs = case(shape, backend32, monkeypatch, dict(d2_bg=0.05, **FP32_SHAPES[shape]), dtype=torch.float32)
    worst, _, _ = run_d_sw(cs, D_SW_FAMILIES[family](cs), DT, backend32)
    check(f"fp32 d_sw {family} {shape}", worst, tol32("d_sw", family))


@pytest.mark.parametrize("family", ["smooth", "strong"])
@pytest.mark.parametrize("shape", list(FP32_SHAPES))
def test_fp32_c_sw_tracks_the_fp64_oracle(backend32, monkeypatch, shape, family):
    cs = case(shape, backend32, monkeypatch, FP32_SHAPES[shape], dtype=torch.float32)
    worst, _ = run_c_sw(cs, hc.smooth_c(cs) if family == "smooth" else hc.strong_c(cs, DT2), DT2, backend32)
    check(f"fp32 c_sw {family} {shape}", worst, tol32("c_sw", family))


@pytest.mark.parametrize("family", ["smooth", "strong", "front"])
@pytest.mark.parametrize("shape", list(FP32_SHAPES))
def test_fp32_fxadv_fv_tp_2d_and_a2b_ord4_track_the_fp64_oracle(backend32, monkeypatch, shape, family):
    """smooth: the winds of the smooth state and its pt; strong: strong winds, the smooth pt; front: strong winds, pt with the 15 % jump --
    the smt5 switch of a cell next to the jump can flip in fp32, which moves its flux by the size of the jump: a row of its own"""
    cs = case(shape, backend32, monkeypatch, FP32_SHAPES[shape], dtype=torch.float32)
    ins = hc.smooth(cs) if family == "smooth" else hc.strong(cs, DT)
    worst, _, F = run_fxadv(cs, ins, DT, backend32)
    if family != "front":
        check(f"fp32 fxadv {family} {shape}", worst, tol32("fxadv", family))
    for hord in (5, 6):
        worst, _ = run_fv_tp_2d(cs, ins, _tp_field(cs, ins, family), F, hord, backend32)
        check(f"fp32 fv_tp_2d hord {hord} {family} {shape}", worst, tol32(f"fv_tp_2d_hord{hord}", family))
    if family == "smooth":
        qin = _a2b_input(cs)
        Q, O = cs.q([_pad(a) for a in qin]), cs.q()
        cs.sf.call("a2b_ord4", Q.fref, O.fref, 0, cs.nz, 0)
        _sync(backend32)
        worst = errors(("qout", r, O.numpy(r)[:, :, : cs.nz][CORNERS(D)], o_a2b.a2b_ord4(D, qin[r].copy())[CORNERS(D)]) for r, D in enumerate(cs.doms))
        check(f"fp32 a2b_ord4 {shape}", worst, tol32("a2b_ord4", "smooth"))


def test_fp32_d_sw_and_c_sw_on_the_real_state_track_the_fp64_oracle(backend32, data):
    """(nord = 1: the damping order the fp32 context accepts at C12, as in test_column_solver_edges)"""
    check("fp32 c_sw real", run_real_c_sw(data, backend32, torch.float32, dict(nord=1)), tol32("c_sw", "real"))
    check("fp32 d_sw real", run_real_d_sw(data, backend32, torch.float32, dict(nord=1)), tol32("d_sw", "real"))
