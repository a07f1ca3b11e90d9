"""The height advection (update_dz_c, update_dz_d with edge_profile, the single-tracer transport marches and the del-n chain of the interface heights), the
pressure-gradient operators (nh_p_grad fused and staged, p_grad_c), del2_cubed and the glue kernels set_gz / compute_geopotential alone through the C ABI
against the oracle, where the smooth C12 calls of test_operator_parity.py never go (input families: tests/height_pgf_case.py):

* Courant numbers and area fluxes of the oracle's fxadv on strong winds (up to 0.85, both signs on every tile edge) under heights with a 2-dx checkerboard of
  5 % of the layer thickness, on every shape of test_horizontal_operator_edges.SHAPES: strip seams (i = 58 / 59), segment seams, partial strips, every cube
  corner, a non-square rank; the same with a 300 m front in every interface (the smt5 switch of hord_tm 6 and 5) and with a rectangle of exactly zero wind and
  level interfaces over a cube corner (every switch on its equality side; the heights there come out bitwise unchanged);
* every configuration switch update_dz_d reads (hord_tm, nord 0 - 2, vtdm4, do_vort_damp, n_sponge, d2_bg_k2) with FV3_ALT=dz_damp_scaled, with 3, 6 and 9 levels;
* the forms behind per-call switches (FV3_DZ_DELN=arrays, FV3_TP2D_MARCH=old, FV3_NH_PGF=staged) and, each in a child process of
  tests/height_pgf_forms_case.py, the forms chosen once per process (FV3_EDGE_PROFILE_GENERIC / _REG / _LDS, FV3_EP_ONE_LAUNCH=0, FV3_TP2D_MODE=staged,
  FV3_DEL6_MODE=staged, FV3_TP2D_FA=0), against the oracle and against the default form;
* every branch of edge_profile_columns: 3, 8, 9, 79, 80, 127, 128 (the 64 KB limit of the run-time wave form) and 129 levels (the generic form);
* nh_p_grad and p_grad_c on air masses with a 50 % front, heights with a random 2-dx checkerboard of up to 300 m and a pressure perturbation of up to 200 Pa;
* del2_cubed alone with nmax 1, 2, 3 on a random checkerboard, on nx < 10 and on multi-strip ranks with each of the four cube corners and with none;
* set_gz and compute_geopotential against their numpy restatement, bitwise, cells outside their boxes untouched;
* the fp32 build of the operators against the fp64 oracle.

Every comparison is element by element on the operator's whole output region (PLANS of test_column_solver_edges.py), field-scale relative per rank
(max |a - b| / max |b|).  Before the library runs, every case asserts per rank from the oracle alone: outputs finite; new heights decreasing by more than dz_min in
every layer (the closing scan, which has its own tests, acts nowhere); update_dz_c takes each upwind side in at least 20 % of its faces in x and in y; in update_dz_d
the less-taken side of the sign of the Courant number and of the smt5 switch covers 1 % of the counted points, |c| > 0.5 occurs in 1 %, fxadv's tile-edge switches
take 4 points of either sign on every tile edge of the rank; the interfaces with and without the del-n damping (fv3_oracle.nh counters dzd_damped /
dzd_undamped) are those the configuration asks for; pgf_rough: the smallest corner delp and corner pk3 difference are 0.05 x their largest; heat_rough: the
amplitude kept after nmax = 1, 2, 3 passes decreases with nmax and is below 0.7 after one.

fp64 bounds: the project's own (update_dz_c gz 1e-13, ws3 1e-11; update_dz_d zh 1e-13, wsd 1e-10; nh_p_grad 1e-12; p_grad_c 1e-13; del2_cubed 1e-12; the glue 0).
Worst errors over the module, per operator and family, host emulation / MI355X: 0 / 0 in every field of every case -- update_dz_d (zh, wsd) and update_dz_c (gz, ws3)
on strong, front and still, update_dz_d over the configuration matrix, every switch and every level count; nh_p_grad (u, v; fused and staged) and p_grad_c (uc, vc) on
pgf_rough; del2_cubed on heat_rough; the glue.  The marches evaluate the oracle's expressions in the oracle's order and both builds contract no multiply-add, so the
strip, segment and shuffle structure of the device kernels changes no bit.  No bound had to come from the long-double run.  The fp64 oracle's own round-off on the
C65 inputs (against its np.longdouble run, test_fp64_oracle_round_off_on_the_new_families): update_dz_d zh 7.7e-16, wsd 4.4e-15; update_dz_c gz 5.8e-16, ws3 5.1e-15;
nh_p_grad u 8.7e-15, v 8.9e-15; p_grad_c uc / vc 1.4e-16; del2_cubed 7.8e-16.
The del-n damping of the heights in its default form (the raw damp_vt as coefficient) stays below the bounds whatever it computes -- a cube-corner patch flux left
out of it changes zh by less than 1e-13 of its scale; the configuration matrix runs it under FV3_ALT=dz_damp_scaled, where the same omission fails 16 cases.
update_dz_c's one-kernel zh -> gz form (fv3_update_dz_c_from) has no entry of its own in the C ABI: it meets the oracle through the sequencer's tests only.
fp32 bounds: per operator, family and field 4 x max(E32, eps32), E32 = the numpy oracle run in np.float32 (inputs, the Dom's metric arrays and dp_ref cast)
against the fp64 oracle, worst over FP32_SHAPES; computed in the test.
E32 (worst of C24 2 x 2 with nord 2 and C65): heights_strong: update_dz_d zh 5.1e-7, wsd 2.5e-6; update_dz_c gz 3.1e-7, ws3 3.5e-6; pgf_rough: nh_p_grad u / v 2.3e-5;
p_grad_c uc 9.3e-8, vc 7.6e-8 (below eps32 = 1.2e-7, which then sets the bound); heat_rough: del2_cubed 5.9e-7.
The library's errors, host emulation and MI355X alike to the two digits printed (C24 2 x 2 / C65): update_dz_d zh 4.4e-7 / 4.9e-7, wsd 2.8e-6 / 2.1e-6; update_dz_c gz
3.1e-7 / 3.3e-7, ws3 3.2e-6 / 2.5e-6; nh_p_grad u 2.3e-5 / 4.4e-6, v 2.3e-5 / 4.7e-6; p_grad_c uc 9.3e-8 / 7.5e-8, vc 7.6e-8; del2_cubed 5.9e-7: no case above 1.1 x E32, none
needed more than 4 x.  The rounding of the inputs to fp32 dominates both sides (nh_p_grad: differences of geopotentials ~1e5 m2/s2 that carry a 300 m checkerboard;
ws3 / wsd: (zs - z) / dt out of heights ~1e3 m).
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import height_pgf_case as hp
import horizontal_case as hc
import test_column_solver_edges as cse
import test_horizontal_operator_edges as hoe
from helpers import Case
from test_operator_parity import Dev

from fv3_oracle import a2b_ord4 as o_a2b
from fv3_oracle import d_sw as o_dsw
from fv3_oracle import nh as o_nh
from fv3_oracle import ppm as o_ppm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 60.0
TOL = {k: cse.TOL[k] for k in ("update_dz_c", "update_dz_d", "nh_p_grad", "p_grad_c", "del2_cubed")}
HEIGHT_SHAPES = ["c12", "c12_2x2", "c24_2x2", "c72_3x3", "c65", "c140_2x2", "c48_3x1"]
PGF_SHAPES = ["c12_2x2", "c24_2x2", "c65", "c140_2x2", "c48_3x1"]
HILL = lambda nz: 400.0 if nz < 79 else 40.0  # noqa: E731  (height_pgf_case.heights_strong)
SEAM = 59  # the first column of the second strip (a marching wave owns up to 58 columns)


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
    for m in (o_dsw, o_nh, o_ppm):
        m.enable_counters(True)
    yield
    for m in (o_dsw, o_nh, o_ppm):
        m.enable_counters(False)


# ---------------------------------------------------------------------------------------------------------------------------
# one operator alone: oracle call records (test_column_solver_edges.ocall), library replay on the case's own context, element-wise errors
# ---------------------------------------------------------------------------------------------------------------------------
def case(shape, backend, setenv, cfg_kw=None, dtype=torch.float64, nz=None):
    """a shape of test_horizontal_operator_edges.SHAPES (FV3_SEG as the shape asks, 0 = automatic), optionally with another level count"""
    n, layout, ranks, seg, nz0 = hoe.SHAPES[shape]
    setenv("FV3_SEG", seg or "0")
    return Case(n, layout, ranks, nz=nz or nz0, backend=backend, cfg_kw=dict(n_split=1, **(cfg_kw or {})), dtype=dtype)


class CaseDev(Dev):
    """test_operator_parity.Dev on the context a Case already holds"""

    def __init__(self, cs):
        self.sf, self.qf, self.nz = cs.sf, cs.qf, cs.nz


def ocall(name, D, *args):
    """test_column_solver_edges.ocall, with the PPM branch counts of this call beside the operator's own"""
    o_ppm.reset_counters()
    cl = cse.ocall(name, D, *args)
    cl["ppm"] = o_ppm.counters()
    return cl


def dz_d_args(cs, ins, dt=DT):
    col = o_dsw.get_column_namelist(cs.cfg, cs.nz)
    return [(D, cs.cfg, col, g.dp_ref, x["zs"], x["zh"], x["crx"], x["cry"], x["xfx"], x["yfx"], x["ws"], dt) for D, g, x in zip(cs.doms, cs.grids, ins)]


def dz_c_args(cs, ins, dt2=DT / 2):
    return [(D, g.dp_ref, x["zs"], x["ut_c"], x["vt_c"], x["zh"], x["ws"], dt2) for D, g, x in zip(cs.doms, cs.grids, ins)]


def nh_p_grad_args(cs, ins, dt=DT):
    return [(D, x["u"], x["v"], x["pp"], x["gz"], x["pk3"], x["delp"], dt, g.ptop, cs.c.KAPPA) for D, g, x in zip(cs.doms, cs.grids, ins)]


def p_grad_c_args(cs, ins, dt2=DT / 2):
    return [(D, D.m.rdxc, D.m.rdyc, x["uc"], x["vc"], x["delp"], x["pk3"], x["gz"], dt2) for D, x in zip(cs.doms, ins)]


def del2_args(cs, qs, cd, nmax):
    return [(D, q, cd, nmax) for D, q in zip(cs.doms, qs)]


def ocalls(name, args):
    return [ocall(name, *a) for a in args]


def library(name, cs, cls):
    return cse.replay(CaseDev(cs), name, cls)


def run(name, cs, cls, label, tol=None):
    """the library on the inputs of the call records against their outputs: worst errors, checked; also the library's outputs"""
    got = library(name, cs, cls)
    return hoe.check(f"{label} {name}", cse.errors(name, got, cls, cs.nz), tol or TOL[name]), got


# ---------------------------------------------------------------------------------------------------------------------------
# what the oracle must show before the library runs
# ---------------------------------------------------------------------------------------------------------------------------
def assert_layers(name, cls, idx, region):
    """finite new heights that decrease by more than dz_min in every layer: the closing scan acted nowhere"""
    for r, c in enumerate(cls):
        D, z = c["D"], c["outs"][idx]
        d = z[:, :, :-1] - z[:, :, 1:]
        if region is cse.RING1:  # (the never-read cube-corner halo cell)
            for (ci, cj), has in (((0, 0), D.sw), ((D.nx + 1, 0), D.se), ((D.nx + 1, D.ny + 1), D.ne), ((0, D.ny + 1), D.nw)):
                if has:
                    d[D.sl(ci, ci, cj, cj)] = np.inf
        assert np.all(np.isfinite(z[region(D)])), f"oracle {name} rank {r}: non-finite heights"
        assert d[region(D)].min() > D.c.DZ_MIN, f"oracle {name} rank {r}: thinnest layer {d[region(D)].min()} m"


def assert_dz_d(cs, cls, fcounts, strong=True):
    assert_layers("update_dz_d", cls, 4, cse.CELLS)
    on = np.append(cls[0]["ins"][1]["damp_vt"], cls[0]["ins"][1]["damp_vt"][-1]) > 1.0e-5
    for r, c in enumerate(cls):
        n, p = c["counts"], c["ppm"]
        assert n["dzd_limited"] == 0 and n["dzd_free"] > 0, (r, n)
        assert (n["dzd_damped"], n["dzd_undamped"]) == (int(on.sum()), int((~on).sum())), (r, n)
        if strong:
            hoe.two_sided(p, ("cfl_pos", "cfl_nonpos"), f"rank {r}: sign of the Courant number")
            assert p["cfl_gt_half"] >= 0.01 * (p["cfl_pos"] + p["cfl_nonpos"]), (r, p)
            h = cs.cfg.hord_tm
            hoe.two_sided(p, (f"smt5_true_hord{h}", f"smt5_false_hord{h}"), f"rank {r}: smt5 of hord {h}")
    if strong:
        hoe.edges_two_sided(cs, fcounts, hoe.FXADV_EDGES)
    return on


def assert_dz_c(cs, cls, share=0.2):
    assert_layers("update_dz_c", cls, 4, cse.RING1)
    for r, c in enumerate(cls):
        n = c["counts"]
        for d in "xy":
            pos, neg = n[f"dzc_upwind_pos_{d}"], n[f"dzc_upwind_neg_{d}"]
            assert min(pos, neg) >= share * (pos + neg), f"rank {r}: update_dz_c upwind sides in {d}: {pos} / {neg}"


def both_height_updates(cs, ins, fcounts, label):
    cls = ocalls("update_dz_d", dz_d_args(cs, ins))
    assert_dz_d(cs, cls, fcounts)
    run("update_dz_d", cs, cls, label)
    cls = ocalls("update_dz_c", dz_c_args(cs, ins))
    assert_dz_c(cs, cls)
    run("update_dz_c", cs, cls, label)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. update_dz_d and update_dz_c, fp64
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", HEIGHT_SHAPES)
def test_height_updates_on_strong_winds_match_the_oracle(backend, counts, monkeypatch, shape):
    """Courant numbers up to 0.85 in both signs under heights with a 2-dx checkerboard, every shape: strip and segment seams, every cube corner"""
    cs = case(shape, backend, monkeypatch.setenv)
    ins, fc = hp.heights_strong(cs, DT)
    both_height_updates(cs, ins, fc, f"strong {shape}")


@pytest.mark.parametrize("shape", ["c24_2x2", "c65"])
def test_height_updates_on_a_front_match_the_oracle(backend, counts, monkeypatch, shape):
    """a 300 m jump in every interface height under the strong winds: the smt5 switch of hord_tm 6 and 5 next to a discontinuity"""
    for hord in (6, 5):
        cs = case(shape, backend, monkeypatch.setenv, dict(hord_tm=hord))
        ins, fc = hp.heights_front(cs, DT)
        both_height_updates(cs, ins, fc, f"front {shape} hord_tm {hord}")


@pytest.mark.parametrize("shape", ["c12_2x2", "c65"])
def test_height_updates_on_a_still_rectangle_leave_its_heights_bitwise_unchanged(backend, counts, monkeypatch, shape):
    """exactly zero Courant numbers / area fluxes / winds, flat terrain and level interfaces (heights that are powers of two) over the SW cube corner: c == 0, bl == br == 0, a zero del-n flux -- every
    switch on its equality side; the heights of the cells whose stencils stay inside the rectangle come out as they went in, in the oracle and in the library"""
    cs = case(shape, backend, monkeypatch.setenv)
    ins, _ = hp.heights_still(cs, DT)
    D, box = cs.doms[0], hc.still_box(cs.doms[0])
    assert D.sw
    inner = (slice(hc.NH, box[0].stop - 1), slice(hc.NH, box[1].stop - 1))  # faces with still cells on both sides
    far = (slice(hc.NH, box[0].stop - 4), slice(hc.NH, box[1].stop - 4))  # cells whose PPM / del-n stencils stay inside the rectangle
    for n in ("crx", "cry", "xfx", "yfx", "ut_c", "vt_c"):
        assert inner[0].stop > inner[0].start and np.all(ins[0][n][inner] == 0.0), n
    for name, args, check_counts in (("update_dz_d", dz_d_args(cs, ins), lambda cls: assert_dz_d(cs, cls, None, strong=False)),
                                     ("update_dz_c", dz_c_args(cs, ins), lambda cls: assert_layers("update_dz_c", cls, 4, cse.RING1))):
        cls = ocalls(name, args)
        check_counts(cls)
        if name == "update_dz_d":
            assert cls[0]["ppm"]["cfl_nonpos"] > 0
        _, got = run(name, cs, cls, f"still {shape}")
        if far[0].stop > far[0].start:
            zin = cls[0]["ins"][4]  # (zh of update_dz_d, gz of update_dz_c)
            assert np.array_equal(cls[0]["outs"][4][far], zin[far]), f"{name}: the oracle moved the still heights"
            assert np.array_equal(got[4][0][far], zin[far]), f"{name}: the library moved the still heights"
        else:
            assert shape == "c12_2x2"  # (6 x 6 cells: no cell is four cells away from the moving air)


# ---- the configuration matrix on the multi-strip shapes
CONFIGS = [{}, dict(hord_tm=5), dict(nord=0), dict(nord=1), dict(nord=2), dict(vtdm4=0.0), dict(do_vort_damp=False), dict(n_sponge=0), dict(d2_bg_k2=0.0)]
MATRIX = [(kw, 6) for kw in CONFIGS] + [({}, 3), ({}, 9), (dict(vtdm4=0.0), 9)]


@pytest.mark.parametrize("shape", ["c65", "c140_2x2"])
@pytest.mark.parametrize("kw, nz", MATRIX, ids=lambda v: f"L{v}" if isinstance(v, int) else ",".join(f"{k}={x}" for k, x in v.items()) or "default")
def test_update_dz_d_config_matrix_on_multi_strip_shapes_matches_the_oracle(backend, counts, monkeypatch, shape, kw, nz):
    """every configuration switch update_dz_d reads, on two strips, under FV3_ALT=dz_damp_scaled (the damping of the heights at the weight of d_sw's vorticity
    damping, in the oracle and in the library): 3 levels = sponge interfaces only (every chain as arrays), 9 levels; vtdm4 = 0 leaves the damping to the two sponge
    interfaces (damped and undamped interfaces in one call), do_vort_damp = False to none"""
    monkeypatch.setenv("FV3_ALT", "dz_damp_scaled")
    cs = case(shape, backend, monkeypatch.setenv, kw, nz=nz)
    ins, fc = hp.heights_strong(cs, DT)
    cls = ocalls("update_dz_d", dz_d_args(cs, ins))
    on = assert_dz_d(cs, cls, fc)
    if kw.get("vtdm4") == 0.0:
        assert on.any() and not on.all()
    else:
        assert on.all() == (kw.get("do_vort_damp") is not False) and on.any() == on.all()
    run("update_dz_d", cs, cls, f"{shape} L{nz} {kw}")


# ---- the forms behind per-call switches
LIVE = {"FV3_DZ_DELN=arrays": "update_dz_d", "FV3_TP2D_MARCH=old": "update_dz_d", "FV3_NH_PGF=staged": "nh_p_grad"}


@pytest.mark.parametrize("shape", ["c24_2x2", "c140_2x2"])
@pytest.mark.parametrize("setting", list(LIVE))
def test_forms_behind_per_call_switches_match_the_oracle(backend, counts, monkeypatch, capfd, shape, setting):
    """the del-n chain of every interface as one staged launch, the older single-tracer march, nh_p_grad as four a2b_ord4 launches + the level-walking update: each
    against the oracle at the bounds of the default form"""
    monkeypatch.setenv(*setting.split("="))
    monkeypatch.setenv("FV3_DEBUG_FD", "1")
    cs = case(shape, backend, monkeypatch.setenv)
    if LIVE[setting] == "update_dz_d":
        ins, fc = hp.heights_strong(cs, DT)
        cls = ocalls("update_dz_d", dz_d_args(cs, ins))
        assert_dz_d(cs, cls, fc)
        capfd.readouterr()
        run("update_dz_d", cs, cls, f"{setting} {shape}")
        assert "[update_dz_d] closing scan: own kernel" in capfd.readouterr().err  # (the only line update_dz_d reports; nh_p_grad reports none)
    else:
        cls = pgf_calls(cs, "nh_p_grad")
        run("nh_p_grad", cs, cls, f"{setting} {shape}")


# ---- every branch of edge_profile_columns
@pytest.mark.parametrize("nz", [3, 8, 9, 79, 80, 127, 128, 129])
def test_update_dz_d_at_every_level_count_of_edge_profile_matches_the_oracle(backend, counts, monkeypatch, nz):
    """C12, one rank: edge_profile as wave<79>, wave<127>, the run-time wave form up to its 64 KB of LDS (fp64: 128 levels) and the generic form beyond"""
    monkeypatch.setenv("FV3_SEG", "0")
    cs = Case(12, (1, 1), (0,), nz=nz, backend=backend, cfg_kw=dict(n_split=1))
    ins, fc = hp.heights_strong(cs, DT, hill=HILL(nz))
    cls = ocalls("update_dz_d", dz_d_args(cs, ins))
    assert_dz_d(cs, cls, fc)
    run("update_dz_d", cs, cls, f"L{nz}")


# ---- the forms chosen once per process, each in a child process
ONCE = ["FV3_EDGE_PROFILE_GENERIC=1", "FV3_EDGE_PROFILE_REG=1", "FV3_EDGE_PROFILE_LDS=1", "FV3_EP_ONE_LAUNCH=0", "FV3_TP2D_MODE=staged", "FV3_DEL6_MODE=staged", "FV3_TP2D_FA=0"]
FORM_CASES = ("c24_2x2:8", "c12:79")
_CHILD, _CHILD_FAILED, _FORM_ORACLE = {}, {}, {}


def forms_case(name, backend, setenv):
    """a named case of the forms test (``<shape>:<levels>``): the Case and update_dz_d's arguments per rank"""
    shape, nz = name.split(":")
    cs = case(shape, backend, setenv, nz=int(nz))
    ins, fc = hp.heights_strong(cs, DT, hill=HILL(cs.nz))
    return cs, dz_d_args(cs, ins), fc


def library_outputs(name, backend):
    """the library's update_dz_d outputs of one named case, as {"<case>/<oracle argument>/<rank>": array}: what tests/height_pgf_forms_case.py writes"""
    cs, args, _ = forms_case(name, backend, os.environ.__setitem__)
    got = library("update_dz_d", cs, [dict(ins=list(a[1:]), D=a[0]) for a in args])
    return {f"{name}/{i}/{r}": a for i, arrs in got.items() for r, a in enumerate(arrs)}


def _child(tmp_path, backend, setting):
    """one child process of tests/height_pgf_forms_case.py under its own timeout, as test_column_solver_edges._child: a failed child fails the test and is not
    started again, and after it no further child is started on that backend"""
    key = (backend, setting)
    if backend in _CHILD_FAILED:
        pytest.fail(f"no further child process on {backend}: {_CHILD_FAILED[backend]}")
    if key not in _CHILD:
        out = str(tmp_path / f"{setting.replace('=', '_') or 'default'}.npz")
        names = [s.split("=")[0] for s in ONCE]
        env = {k: v for k, v in os.environ.items() if k not in names}
        if setting:
            name, val = setting.split("=")
            env[name] = val
        try:
            subprocess.run([sys.executable, os.path.join(ROOT, "tests", "height_pgf_forms_case.py"), "--cases", ",".join(FORM_CASES), "--backend", backend, "--out", out],
                           check=True, env=env, timeout=300)
            with np.load(out) as f:
                _CHILD[key] = {k: f[k] for k in f.files}
        except Exception as e:
            _CHILD_FAILED[backend] = f"the child with {setting or 'the default forms'} failed: {e!r}"
            raise
    return _CHILD[key]


@pytest.mark.parametrize("setting", ONCE)
def test_forms_chosen_once_per_process_match_the_oracle_and_the_default_form(backend, counts, tmp_path, monkeypatch, setting):
    """edge_profile's generic, register-resident and run-time-level wave forms and its four-launch form, fv_tp_2d and the del-n fluxes as one launch per stage,
    the general form of the marches with the chain inside: update_dz_d under each, on C24 2 x 2 L8 (two segments) and C12 L79, against the oracle at the bounds
    of the default form and against the default form's child element by element at 1e-11"""
    forced = _child(tmp_path, backend, setting)
    default = _child(tmp_path, backend, "")
    for name in FORM_CASES:
        if name not in _FORM_ORACLE:
            cs, args, fc = forms_case(name, backend, monkeypatch.setenv)
            cls = ocalls("update_dz_d", args)
            assert_dz_d(cs, cls, fc)
            _FORM_ORACLE[name] = (cs.nz, cls)
        nz, cls = _FORM_ORACLE[name]
        outs = [i for _, i, *_ in cse.PLANS["update_dz_d"][2]]
        pick = lambda src: {i: [src[f"{name}/{i}/{r}"] for r in range(len(cls))] for i in outs}  # noqa: E731
        hoe.check(f"{setting} {name}", cse.errors("update_dz_d", pick(forced), cls, nz), TOL["update_dz_d"])
        ref = [dict(c, outs={i: pick(default)[i][r] for i in outs}) for r, c in enumerate(cls)]
        hoe.check(f"{setting} against the default form, {name}", cse.errors("update_dz_d", pick(forced), ref, nz), dict(default=1e-11))


# ---------------------------------------------------------------------------------------------------------------------------
# 2. nh_p_grad and p_grad_c on rough inputs
# ---------------------------------------------------------------------------------------------------------------------------
def assert_pgf_rough(cs, ins, floor=0.05):
    """the weights of the two gradients are far from zero and far from uniform: corner delp and corner pk3 differences, smallest against largest"""
    for r, (D, g, x) in enumerate(zip(cs.doms, cs.grids, ins)):
        C = hoe.CORNERS(D)
        wk1 = o_a2b.a2b_ord4(D, x["delp"].copy())[C]
        pk3 = x["pk3"].copy()
        pk3[C + (slice(0, 1),)] = g.ptop**cs.c.KAPPA
        low = pk3[:, :, 1:].copy()
        o_a2b.a2b_ord4(D, low, replace=True)
        wk = np.diff(np.concatenate([pk3[:, :, :1], low], axis=2)[C], axis=2)
        for name, a in (("corner delp", wk1), ("corner pk3 difference", wk)):
            assert a.min() >= floor * a.max() and a.max() > 1.5 * a.min(), f"rank {r}: {name} {a.min()} .. {a.max()}"


def pgf_calls(cs, name):
    ins = hp.pgf_rough(cs)
    assert_pgf_rough(cs, ins)
    return ocalls(name, nh_p_grad_args(cs, ins) if name == "nh_p_grad" else p_grad_c_args(cs, ins))


@pytest.mark.parametrize("form", ["default", "staged"])
@pytest.mark.parametrize("shape", PGF_SHAPES)
def test_nh_p_grad_on_rough_inputs_matches_the_oracle(backend, monkeypatch, shape, form):
    """u / v on their own staggered regions: the fused march (60-corner strips, a2b_point at the tile edges) and the staged form"""
    if form == "staged":
        monkeypatch.setenv("FV3_NH_PGF", "staged")
    cs = case(shape, backend, monkeypatch.setenv)
    cls = pgf_calls(cs, "nh_p_grad")
    assert all(np.abs(c["outs"][i] - c["ins"][i]).max() > 1.0 for c in cls for i in (0, 1))  # (the gradients move the winds by metres per second)
    run("nh_p_grad", cs, cls, f"pgf_rough {shape} {form}")


@pytest.mark.parametrize("shape", PGF_SHAPES)
def test_p_grad_c_on_rough_inputs_matches_the_oracle(backend, monkeypatch, shape):
    """uc / vc on their own staggered regions, pkc = pk3 and delpc = delp of pgf_rough"""
    cs = case(shape, backend, monkeypatch.setenv)
    cls = pgf_calls(cs, "p_grad_c")
    assert all(np.abs(c["outs"][i] - c["ins"][i]).max() > 0.0 for c in cls for i in (2, 3))
    run("p_grad_c", cs, cls, f"pgf_rough {shape}")


# ---------------------------------------------------------------------------------------------------------------------------
# 3. del2_cubed alone
# ---------------------------------------------------------------------------------------------------------------------------
def heat_calls(cs, nmaxes=(1, 2, 3)):
    """the oracle's del2_cubed on heat_rough with each nmax; the amplitude a pass keeps (rms over the compute domain, per rank) falls with nmax"""
    qs, cd = hp.heat_rough(cs)
    calls = {n: ocalls("del2_cubed", del2_args(cs, qs, cd, n)) for n in (1, 2, 3)}
    for r, D in enumerate(cs.doms):
        rms = lambda a: float(np.sqrt(np.mean(a[cse.CELLS(D)] ** 2)))  # noqa: E731
        kept = [rms(calls[n][r]["outs"][0]) / rms(qs[r]) for n in (1, 2, 3)]
        print(f"heat_rough rank {r}: amplitude kept after 1, 2, 3 passes", [f"{k:.2f}" for k in kept])
        assert kept[0] < 0.7 and kept[2] < kept[1] < kept[0], (r, kept)
    return {n: calls[n] for n in nmaxes}


@pytest.mark.parametrize("shape", PGF_SHAPES + ["c72_3x3"])
def test_del2_cubed_on_a_rough_heat_source_matches_the_oracle(backend, monkeypatch, shape):
    """nmax 1, 2, 3 (the halo rings a pass updates shrink with the passes left; the cube-corner means and corner copies of every pass): nx < 10 (C12 2 x 2),
    multi-strip ranks, each of the four cube corners (the 2 x 2 layouts) and a rank with none (C72 3 x 3 rank 4)"""
    cs = case(shape, backend, monkeypatch.setenv)
    if len(cs.doms) == 4:
        assert sorted((D.sw, D.se, D.ne, D.nw) for D in cs.doms) == sorted(tuple(i == j for j in range(4)) for i in range(4))  # (one rank per cube corner)
    if shape == "c72_3x3":
        assert not any(f for D in cs.doms[2:] for f in (D.west, D.east, D.south, D.north))
    for nmax, cls in heat_calls(cs).items():
        run("del2_cubed", cs, cls, f"heat_rough {shape} nmax {nmax}")


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the glue kernels
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["c12_2x2", "c65"])
def test_set_gz_and_compute_geopotential_match_their_restatement_bitwise(backend, monkeypatch, shape):
    """As fv3_ctx.hip writes them.  set_gz(zs, delz, gz): on the compute domain (1..nx, 1..ny) gz[nz] = zs and, from the ground up, gz[k] = gz[k + 1] - delz[k]
    (one running difference per column).  compute_geopotential(zh, gz): gz = zh * grav on the compute domain + 2 rings (-1..nx + 2, -1..ny + 2), every interface
    0..nz.  Neither touches a cell outside its box: the output starts as a sentinel."""
    cs = case(shape, backend, monkeypatch.setenv)
    dv, nz, sentinel = CaseDev(cs), cs.nz, -7.0
    zs = [hp.terrain(cs, r) + np.zeros(cs.shape[:2] + (1,)) for r in range(len(cs.doms))]
    delz = [s["delz"] for s in cs.states]
    zh = [hp.rough_heights(cs, r, zs[r]) for r in range(len(cs.doms))]
    blank = [np.full(cs.shape, sentinel) for _ in cs.doms]
    gz, gp = dv.q(blank), dv.q(blank)
    cs.sf.call("set_gz", dv.q(zs).fref, dv.q(delz).fref, gz.fref)
    cs.sf.call("compute_geopotential", dv.q(zh).fref, gp.fref)
    if backend != "hostemu":
        torch.cuda.synchronize()
    for r, D in enumerate(cs.doms):
        want = blank[r].copy()
        C = cse.CELLS(D)
        z = zs[r][C][:, :, 0].copy()
        want[C + (nz,)] = z
        for k in range(nz - 1, -1, -1):
            z = z - delz[r][C + (k,)]
            want[C + (k,)] = z
        assert np.array_equal(gz.numpy(r), want), f"set_gz rank {r}: {np.abs(gz.numpy(r) - want).max()}"
        want = blank[r].copy()
        want[cse.RING2(D)] = zh[r][cse.RING2(D)] * cs.c.GRAV
        assert np.array_equal(gp.numpy(r), want), f"compute_geopotential rank {r}: {np.abs(gp.numpy(r) - want).max()}"


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the comparer itself, and the reference's own round-off
# ---------------------------------------------------------------------------------------------------------------------------
def test_comparer_notices_one_element_at_the_strip_seam_and_in_a_corner_patch(backend, counts, monkeypatch):
    """control: the library's own zh of the C65 strong case passes; the same array with one element of the strip seam's first column (i = 59) scaled by 1 + 1e-10
    fails, and so does del2_cubed's output with the SW cube corner's cell scaled"""
    cs = case("c65", backend, monkeypatch.setenv)
    ins, _ = hp.heights_strong(cs, DT)
    cls = ocalls("update_dz_d", dz_d_args(cs, ins))
    _, got = run("update_dz_d", cs, cls, "control c65")
    o = cs.doms[0].o
    assert got[4][0][SEAM + o, 30 + o, 0] >= 0.9 * np.abs(cls[0]["outs"][4]).max()
    got[4][0][SEAM + o, 30 + o, 0] *= 1.0 + 1.0e-10
    with pytest.raises(AssertionError, match="zh"):
        hoe.check("control c65, seam element scaled", cse.errors("update_dz_d", got, cls, cs.nz), TOL["update_dz_d"])
    cls = heat_calls(cs, nmaxes=(3,))[3]
    _, got = run("del2_cubed", cs, cls, "control c65")
    assert cs.doms[0].sw
    k = int(np.argmax(np.abs(got[0][0][1 + o, 1 + o, : cs.nz])))
    assert abs(got[0][0][1 + o, 1 + o, k]) >= 0.1 * np.abs(cls[0]["outs"][0]).max()
    got[0][0][1 + o, 1 + o, k] *= 1.0 + 1.0e-10
    with pytest.raises(AssertionError, match="heat_source"):
        hoe.check("control c65, corner cell scaled", cse.errors("del2_cubed", got, cls, cs.nz), TOL["del2_cubed"])


def oracle_as(name, args, dtype):
    """the oracle's operator with every floating-point input, the Dom's metric arrays and dp_ref in ``dtype``: call records whose outputs have that dtype"""
    cls = []
    for a in args:
        work = hp.as_dtype(a[1:], dtype)
        D = hp.dom_as(a[0], dtype)
        getattr(o_nh, name)(D, *work)
        plan = cse.PLANS[name][2]
        assert all(work[i].dtype == dtype for _, i, *_ in plan), (name, [work[i].dtype for _, i, *_ in plan])
        cls.append(dict(D=a[0], outs=work))
    return cls


def self_error(name, args, cls64, dtype, nz):
    """the oracle in ``dtype`` against the fp64 oracle: errors as the library's are measured.  np.longdouble: the fp64 oracle's own round-off (the
    long-double outputs are the reference); np.float32: E32 (the fp64 outputs are the reference)"""
    other = oracle_as(name, args, dtype)
    outs = [i for _, i, *_ in cse.PLANS[name][2]]
    if dtype == np.longdouble:
        return cse.errors(name, {i: [c["outs"][i] for c in cls64] for i in outs}, other, nz)
    return cse.errors(name, {i: [np.asarray(c["outs"][i], dtype=np.float64) for c in other] for i in outs}, cls64, nz)


def test_fp64_oracle_round_off_on_the_new_families(hostemu, monkeypatch):
    """The reference's own error: the fp64 oracle against the same oracle run in np.longdouble on the C65 inputs of every family (its work arrays take the dtype
    of their inputs; the outputs' dtype is asserted).  A correct library carries a round-off of the same size, so a bound in use must at least cover the
    oracle's: the fp64 oracle stays inside every fp64 bound of this module against its long-double self (measured: module docstring; a case that exceeded its
    bound would get 4 x its own figure)."""
    assert np.finfo(np.longdouble).eps < 1e-18  # (an extended type: where long double is double this measures nothing)
    cs = case("c65", "hostemu", monkeypatch.setenv)
    ins, _ = hp.heights_strong(cs, DT)
    pgf = hp.pgf_rough(cs)
    qs, cd = hp.heat_rough(cs)
    for name, args in (("update_dz_d", dz_d_args(cs, ins)), ("update_dz_c", dz_c_args(cs, ins)), ("nh_p_grad", nh_p_grad_args(cs, pgf)), ("p_grad_c", p_grad_c_args(cs, pgf)),
                       ("del2_cubed", del2_args(cs, qs, cd, 3))):
        hoe.check(f"fp64 oracle against long double, c65 {name}", self_error(name, args, ocalls(name, args), np.longdouble, cs.nz), TOL[name])


# ---------------------------------------------------------------------------------------------------------------------------
# 6. the fp32 build against the fp64 oracle
# ---------------------------------------------------------------------------------------------------------------------------
# the fp32 context refuses damping coefficients (damp da_min)^(nord + 1) beyond its range: the default del-8 chain on C48 and coarser
FP32_SHAPES = {"c24_2x2": dict(nord=2), "c65": {}}
EPS32 = float(np.finfo(np.float32).eps)
FAMILIES32 = ("heights_strong", "pgf_rough", "heat_rough")


def family_ops(cs, family):
    """[(operator, its arguments per rank)] of one family"""
    if family == "heights_strong":
        ins, _ = hp.heights_strong(cs, DT)
        return [("update_dz_d", dz_d_args(cs, ins)), ("update_dz_c", dz_c_args(cs, ins))]
    if family == "pgf_rough":
        ins = hp.pgf_rough(cs)
        return [("nh_p_grad", nh_p_grad_args(cs, ins)), ("p_grad_c", p_grad_c_args(cs, ins))]
    qs, cd = hp.heat_rough(cs)
    return [("del2_cubed", del2_args(cs, qs, cd, 3))]


_FP32 = {}


def fp32_cases(family, backend32, setenv):
    """{shape: (Case, [(operator, fp64 call records)])} and {operator: {field: E32}} (worst over the shapes) of one family, built once per backend"""
    key = (family, backend32)
    if key not in _FP32:
        cases, e32 = {}, {}
        for shape, kw in FP32_SHAPES.items():
            cs = case(shape, backend32, setenv, kw, dtype=torch.float32)
            ops = []
            for name, args in family_ops(cs, family):
                cls = ocalls(name, args)
                for f, e in self_error(name, args, cls, np.float32, cs.nz).items():
                    e32.setdefault(name, {})[f] = max(e32.get(name, {}).get(f, 0.0), e)
                ops.append((name, cls))
            cases[shape] = (cs, ops)
        print(f"E32 {family}:", {n: {f: f"{e:.1e}" for f, e in d.items()} for n, d in e32.items()})
        _FP32[key] = (cases, e32)
    return _FP32[key]


@pytest.mark.parametrize("family", FAMILIES32)
@pytest.mark.parametrize("shape", list(FP32_SHAPES))
def test_fp32_operators_track_the_fp64_oracle(backend32, monkeypatch, shape, family):
    """bound per operator, family and field: 4 x max(E32, eps32) -- the factor covers what separates numpy's fp32 from the device's (contracted multiply-adds,
    the order of a few sums; test_column_solver_edges measured up to 3.1 between the host emulation and the device)"""
    cases, e32 = fp32_cases(family, backend32, monkeypatch.setenv)
    cs, ops = cases[shape]
    monkeypatch.setenv("FV3_SEG", hoe.SHAPES[shape][3] or "0")
    for name, cls in ops:
        run(name, cs, cls, f"fp32 {family} {shape}", tol={f: 4.0 * max(e, EPS32) for f, e in e32[name].items()})
