"""Read and write footprints of the acoustic operators and of the whole acoustic call.

Every parity test hands the library and the oracle the same arrays, finite everywhere, so a kernel that reads one cell too many (a level
too deep, a halo ring too far, a cube-corner block INTEGRATION.md calls "redirected") or writes one (into a halo cell, the pad level nz,
past the end of the allocation) passes them.  Here the library is compared with ITSELF, bit for bit, and the oracle decides which cells
may hold NaN (tests/footprint_case.py: region names, tables, engine).  The module contains no tolerance.

1. One operator alone, three calls in one context on guarded fields (clean, poisoned, clean again), after two oracle runs per rank
   (clean / the whole table poisoned at once) have shown that the oracle does not need any cell of the table:
     * the poisoned call equals the clean one, and is finite, on every region the parity tests compare (DSW_OUT, FXADV_OUT, c_sw's list
       without the cube-corner cell, test_operator_parity._cmp's regions);
     * the third call equals the first over the whole storage (no state kept between calls);
     * the first call changes no bit outside the allowed write set; the guard bands of all three calls are intact.
   Shapes: c12_2x2 (6 x 6, one cube corner per rank, staged forms), c24_2x2 + FV3_SEG=8 (12 x 12: fused wind stage, marches, two segments),
   c72_3x3 + FV3_SEG=8 ranks 0 1 4 (two, one, no tile edge), c48_3x1 (16 x 48); column operators c12_2x2 and c48_3x1 on the recorded
   oracle sequence (8 levels), ray_fast and update_dz_d on the whole C12 cube at 79 levels.  The fp32 build (nord 2) on c24_2x2.  The kernel-form
   switches on c24_2x2, except: c_sw's (its interior forms exist from 16 x 16 on: c48_3x1, c72_3x3), FV3_EDGE_PROFILE_* also at 79 levels (where
   _LDS acts), FV3_DZ_SCAN=separate in the whole call (the stand-alone entry always scans itself).  Every form case asserts from the FV3_DEBUG_FD
   lines that the form it names ran and the default one did not (DEFAULT_FORMS: the default cases take the forms their shapes are chosen for).
2. The whole acoustic call (AcousticDynamics.__call__, native sequencer, all ranks in one context, two calls): NaN in everything outside
   helpers.compute_slice of every state field and in all of every workspace field except zs, before each call; the compute cells of every
   state field equal the clean run bit for bit.  C12 2 x 2 (nz 8, n_split 2) under the sequencer's switches, C24 2 x 2 with FV3_SEG=8, fp32 on C24.

Per operator: ``unread`` = the validated poison table (footprint_case.TABLES, found with ``python tests/footprint_case.py --discover`` over the
shapes above, asserted again by the two oracle runs of every case; ``pad``, level nz, is added to every cell-level 3-D input; an argument
without an input is ``all``), ``writes`` = the allowed write set (the region the parity test compares; levels 0 .. nz - 1, interfaces 0 .. nz).
  d_sw          unread  delp pt u v w uc vc divgd q_con: corner_blocks; ua va: depth>=2, corner_blocks; mfxd mfyd: depth>=1 (the whole halo);
                        heat_source: depth>=1; cxd: diagonal, W / E halo; cyd: diagonal, S / N halo; delpc crx cry xfx yfx zh diss_est: all
                writes  delp pt w q_con heat_source: cells; u mfyd: u faces; v mfxd: v faces; cxd crx xfx: x faces of every row; cyd cry yfx: y faces
                        of every column; divgd: corners.  Exceptions: delpc any cell (include/fv3_mi355x.h, fv3_d_sw: the work array of the divergence
                        damping); uc / vc any cell ("the reference's d_sw uses uc/vc as work arrays ... unchanged except in the
                        12 x 12 windows at cube corners")
  c_sw          unread  delp pt w: depth>=3, corner_blocks; u: S / N halo depth>=3; v: W / E halo depth>=3; uc vc ua va omga ut vt divgd delpc ptc: all
                writes  delpc ptc omga ua: cells + 1 ring; divgd: corners; uc: v faces; vc: u faces; ut: i 0..nx+2, j 0..ny+1; vt: i 0..nx+1, j 0..ny+2.
                        Exception: uc vc ua va also wherever the oracle's d2a2c_vect stores them (header, fv3_c_sw)
  fxadv         unread  uc vc: corner_blocks; the six outputs: all
                writes  crx xfx ut: x faces of every row; cry yfx vt: y faces of every column.  Exception: ut / vt also wherever the oracle stores
                        them (beside the faces, except on the rows / columns along a tile edge; header, fv3_fxadv)
  fv_tp_2d      unread  q: corner_blocks; crx xfx: diagonal, W / E halo; cry yfx: diagonal, S / N halo; mfx mfy: depth>=1; mass: depth>=2, diagonal; fx fy: all
  (hord 5, 6; plain and mass-weighted + damped)     writes  fx: v faces; fy: u faces
  a2b_ord4      unread  qin: depth>=3, corner_blocks; qout: all                          writes  qout: corners
  update_dz_c   unread  zs ut vt: depth>=2, corner_blocks; gz: depth>=3, corner_blocks; ws: all          writes  gz ws: cells + 1 ring
  riem_solver_c unread  cappa phis ws ptc q_con delpc gz w3: depth>=2, corner_blocks; pef: all              writes  gz pef: cells + 1 ring
  p_grad_c      unread  uc vc: depth>=1; delpc pkc gz: depth>=2, diagonal                                 writes  uc: v faces; vc: u faces
  update_dz_d   unread  zs: depth>=1; zh: corner_blocks; crx xfx: diagonal, W / E halo; cry yfx: diagonal, S / N halo; ws: all     writes  zh ws: cells
  riem_solver3  unread  cappa zs ws delz q_con delp pt zh w: depth>=1; pe ppe pk3 pk peln: all              writes  w delz zh ppe pk3 pe pk peln: cells
  pk3_halo      unread  pk3: depth>=1; delp: depth>=3                                                     writes  pk3: cells + 2 rings
  edge_pe       unread  pe: depth>=1; delp: depth>=2, corner_blocks                                       writes  pe: cells + 1 ring
  nh_p_grad     unread  u v: depth>=1; pp gz pk3 delp: depth>=3, corner_blocks                            writes  u: u faces; v: v faces; pp, gz, pk3
                        bit for bit over the whole storage ("the three inputs come back unchanged")
  ray_fast      unread  u v w: depth>=1                                                                   writes  u: u faces; v: v faces; w: cells
  del2_cubed    unread  q: corner_blocks                  writes  q: cells.  Exception: also the rings the oracle's earlier iterations store
  apply_diffusive_heating   unread  delp delz cappa heat_source pt: depth>=1                              writes  pt: cells
An output on "cells + 1 ring" may be stored on the whole rectangle: its cube-corner halo cell is not compared by the parity tests (it has no
neighbour) and holds no defined value (header, "Footprints").

Where each statement was observed: the tables on the fp64 oracle; every assertion of the module on the
host emulation AND on an MI355X (gfx950), fp64 and fp32, default forms and every switch listed in LIVE, ONCE and SEQ: all cases pass on both.

FINDINGS (all of them on the host emulation already; the MI355X build behaves the same)
  * No operator, form or precision reads a cell of its table, keeps state between calls, stores into a pad level or past either end of a field.
  * d_sw's write set is exactly the compared regions plus the three work arrays, in every form.
  * The oracle does NOT keep to the compared regions itself, as the cross-check was expected to show: whole-array numpy stores uc / vc / ua / va
    (c_sw), ut / vt (fxadv), q (del2_cubed) and d_sw's / nh_p_grad's work arrays on wider ranges (footprint_case.ORACLE_WORK).  The library
    follows the reference there, so the allowed set of c_sw's winds, fxadv's ut / vt and del2_cubed's q is widened by the oracle's own stores --
    by nothing the library does -- and the cross-check holds for every other field.
  * fxadv, fixed: the stand-alone entry stored ut on i = 0, nx + 2, nx + 3 and vt on j = 0, ny + 2, ny + 3 of the two rows / columns along a
    tile edge too (6 columns per tile edge, the frame kernel's whole range), where the oracle leaves them untouched.  Nothing read them.  The
    frame kernel of fv3_fxadv now stores the faces only there (fv3_dsw.hip; inside d_sw, where ut / vt are scratch, nothing changed); the
    compared regions keep their bits.
  * Ring-1 outputs (gz, ws3, pef, pe, omga, delpc, ptc) are stored on the cube-corner halo cell as well; stated in the header and INTEGRATION.md.
  * Undocumented precondition of the acoustic call: phis is read on ONE halo ring (riem_solver_c) and no halo update fills it -- with NaN there
    every state field comes out NaN.  Now stated in the header and INTEGRATION.md; part 2 plants NaN in phis from the second ring outwards.
  * FV3_DEBUG_FD now also reports the form of c_sw, fv_tp_2d, the Riemann solvers and edge_profile, so that a form case can show it ran.
"""
import os
import subprocess
import sys

import pytest
import torch

import footprint_case as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLUMN_OPS = ("update_dz_c", "riem_solver_c", "p_grad_c", "update_dz_d", "riem_solver3", "pk3_halo", "edge_pe", "nh_p_grad", "del2_cubed", "apply_diffusive_heating")
CASES = [(op, s) for op in fc.HORIZONTAL for s in fc.H_SHAPES] + [(op, s) for op in COLUMN_OPS for s in fc.COLUMN_SHAPES] + [("ray_fast", "c12_L79"), ("update_dz_d", "c12_L79")]
ALL_OPS = fc.HORIZONTAL + COLUMN_OPS


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


_DEVICE_FAILED = {}


def _run(backend, fn, *args, **kw):
    """a failed assertion is a finding and the next case runs; anything else on the device (an error of the runtime, a failed launch) ends
    the module's device work: the cases that follow fail with the first error's message and start nothing"""
    if backend in _DEVICE_FAILED:
        pytest.fail(f"no further case on {backend}: {_DEVICE_FAILED[backend]}")
    try:
        return fn(*args, **kw)
    except AssertionError:
        raise
    except Exception as e:
        if backend != "hostemu":
            _DEVICE_FAILED[backend] = repr(e)
        raise


# ---------------------------------------------------------------------------------------------------------------------------
# 0. the tables hold at least what the oracle was found not to read
# ---------------------------------------------------------------------------------------------------------------------------
def _covers(table, name, spec):
    have = table.get(name, ())
    return spec in have or fc._implied(spec, have)


def test_the_poison_tables_hold_the_minimum():
    import horizontal_case as hc

    d = fc.TABLES["d_sw"]
    for n in hc.D_SW_IN:
        assert _covers(d, n, "corner_blocks"), n
    for n, spec in (("mfxd", "depth>=1"), ("mfyd", "depth>=1"), ("ua", "depth>=2"), ("va", "depth>=2"), ("cxd", "diagonal"), ("cyd", "diagonal")):
        assert _covers(d, n, spec), (n, spec)
    c = fc.TABLES["c_sw"]
    for n in ("delp", "pt", "w"):
        assert _covers(c, n, "depth>=3"), n
    for n in ("uc", "vc", "ua", "va", "omga"):
        assert "all" in c[n], n  # (ut, vt, divgd, delpc, ptc have no input at all: Setup marks them ``all``)
    for op in ("riem_solver3", "ray_fast", "apply_diffusive_heating"):  # horizontally pointwise: everything outside the output region of each input
        for n in fc.REC_OPS[op][1]:
            assert _covers(fc.TABLES[op], n, "depth>=1"), (op, n)


def test_every_cell_level_input_gets_the_pad_level(hostemu):
    for op, shape in (("d_sw", "c12_2x2"), ("c_sw", "c12_2x2"), ("riem_solver3", "c12_2x2"), ("nh_p_grad", "c12_2x2")):
        with fc.env(FV3_SEG=fc.seg_of(shape)):
            S = fc.make(op, shape, "hostemu")
        for n in S.names:
            if S.kind[n] == "L":
                assert "pad" in S.table[n] or "all" in S.table[n], (op, n)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. one operator alone
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op, shape", CASES, ids=[f"{o}-{s}" for o, s in CASES])
def test_operator_reads_and_writes_only_what_it_may(backend, op, shape):
    _run(backend, fc.run_case, op, shape, backend)


def test_the_engine_notices_a_poisoned_cell_that_is_read_and_a_write_outside_the_set(backend):
    """the checks have teeth: with depth>=1 of d_sw's ua (the ring the damping reads) added to the table the oracle side fails, and so does
    the library's poisoned call when the oracle side is skipped; with u taken out of the allowed set its store is reported"""
    with fc.env(FV3_SEG=fc.seg_of("c12_2x2")):
        S = fc.make("d_sw", "c12_2x2", backend)
        S.table["ua"] = ("depth>=1", "pad")
        msgs = []
        fc.check_oracle(S, msgs)
        assert any("depend on the poison table" in m for m in msgs), msgs
        msgs = []
        _run(backend, fc.check_library, S, backend, msgs)
        assert any("a cell of the poison table is read" in m for m in msgs), msgs
        S = fc.make("d_sw", "c12_2x2", backend)
        fc.check_oracle(S, [])
        S.out = {k: v for k, v in S.out.items() if k != "u"}
        msgs = []
        _run(backend, fc.check_library, S, backend, msgs)
        assert msgs and all(m.startswith("u rank") and "written outside the allowed set" in m for m in msgs), msgs


def test_guard_bands_notice_a_store_past_either_end(hostemu):
    S = fc.make("a2b_ord4", "c12_2x2", "hostemu")
    g = fc.Guarded(S.sf, False)
    assert g.guards_intact()
    g.buf[fc.GUARD - 1] = 0.0
    assert not g.guards_intact()
    g = fc.Guarded(S.sf, True)
    g.buf[fc.GUARD + g.n] = 0.0
    assert not g.guards_intact()
    assert fc.GUARD % 64 == 0


# What FV3_DEBUG_FD reports when a form is taken (the d_sw lines: test_horizontal_operator_edges.DEBUG_LINE)
CSW_FORM = {"march": "[c_sw] interior as one march", "two_row": "[c_sw] two-row stage-B kernel on the interior", "generic": "[c_sw] generic per-point stage kernels everywhere"}
EP_FORM = {"wave79": "edge_profile: wave form, 79 levels", "wave": "edge_profile: wave form, level count at run time", "reg": "edge_profile: register-resident column form",
           "generic": "edge_profile: generic thread-per-column form"}
# switches read at every call, set in this process: (switch, value, operator, shape, lines that must appear, lines that must not).  c_sw's interior
# forms exist on sub-domains of 16 x 16 and more only (c48_3x1: 16 x 48, c72_3x3: 24 x 24); below that every point takes the generic kernels.
LIVE = [("FV3_DSW_WINDSTAGE", "staged", "d_sw", "c24_2x2", None, ()), ("FV3_DSW_DELN", "arrays", "d_sw", "c24_2x2", None, ()), ("FV3_DSW_MARCH", "old", "d_sw", "c24_2x2", None, ("pair march, role",)),
        ("FV3_CSW_MARCH", "0", "c_sw", "c48_3x1", (CSW_FORM["two_row"],), (CSW_FORM["march"],)), ("FV3_CSW_MARCH", "0", "c_sw", "c72_3x3", (CSW_FORM["two_row"],), (CSW_FORM["march"],)),
        ("FV3_CSW_B_GENERIC", "1", "c_sw", "c48_3x1", (CSW_FORM["generic"],), (CSW_FORM["march"],)), ("FV3_CSW_B_GENERIC", "1", "c_sw", "c72_3x3", (CSW_FORM["generic"],), (CSW_FORM["march"],))]


@pytest.mark.parametrize("name, value, op, shape, want, never", LIVE, ids=[f"{c[0]}={c[1]}-{c[2]}-{c[3]}" for c in LIVE])
def test_operator_forms_behind_per_call_switches(backend, monkeypatch, capfd, name, value, op, shape, want, never):
    import test_horizontal_operator_edges as the

    monkeypatch.setenv(name, value)
    monkeypatch.setenv("FV3_DEBUG_FD", "1")
    capfd.readouterr()
    _run(backend, fc.run_case, op, shape, backend)
    err = capfd.readouterr().err
    for line in the.DEBUG_LINE[name] if want is None else want:  # the form the switch asks for was taken
        assert line in err, (line, err[-2000:])
    for line in never:
        assert line not in err, (line, err[-2000:])


DEFAULT_FORMS = [("d_sw", "c24_2x2", None), ("d_sw", "c12_2x2", ("fused wind stage on levels 6..5 of 6",)), ("c_sw", "c48_3x1", (CSW_FORM["march"],)), ("c_sw", "c72_3x3", (CSW_FORM["march"],)),
                 ("c_sw", "c24_2x2", (CSW_FORM["generic"],)), ("update_dz_d", "c24_2x2", (EP_FORM["wave"], "[fv_tp_2d] marching form", "closing scan: own kernel")), ("update_dz_d", "c12_L79", (EP_FORM["wave79"],)),
                 ("fv_tp_2d_hord6", "c24_2x2", ("[fv_tp_2d] marching form",)), ("riem_solver_c", "c24_2x2", ("[riem_solver_c] wave form",)), ("riem_solver3", "c24_2x2", ("[riem_solver3] wave form",))]


@pytest.mark.parametrize("op, shape, want", DEFAULT_FORMS, ids=[f"{o}-{s}" for o, s, _ in DEFAULT_FORMS])
def test_default_cases_take_the_forms_their_shapes_are_chosen_for(backend, monkeypatch, capfd, op, shape, want):
    """c24_2x2: d_sw's fused wind stage and pair marches on levels 3..5; c12_2x2 (nx < 8): its staged forms; c_sw's march from 16 x 16 on;
    update_dz_d's edge_profile instantiation for 79 levels and its run-time form; the wave forms of the Riemann solvers"""
    import test_horizontal_operator_edges as the

    monkeypatch.setenv("FV3_DEBUG_FD", "1")
    capfd.readouterr()
    _run(backend, fc.run_case, op, shape, backend)
    err = capfd.readouterr().err
    for line in the.DEBUG_LINE[""] if want is None else want:
        assert line in err, (line, err[-2000:])


# switches read once per process: one child process per setting -- (operators, shapes, lines that must appear, lines that must not).
# FV3_EDGE_PROFILE_LDS only matters at 79 / 127 levels, where it replaces the instantiation for that level count by the run-time form.
TP = ("fv_tp_2d_hord5", "fv_tp_2d_hord6", "fv_tp_2d_hord5_plain", "fv_tp_2d_hord6_plain", "update_dz_d", "d_sw")
ONCE = {"FV3_TP2D_MODE=staged": (TP, "c24_2x2", ("[fv_tp_2d] staged form",), ("[fv_tp_2d] marching form",)),
        "FV3_RIEM_MODE=columns": (("riem_solver_c", "riem_solver3"), "c24_2x2", ("[riem_solver_c] column form", "[riem_solver3] column form"), ("wave form",)),
        "FV3_EDGE_PROFILE_LDS=1": (("update_dz_d",), "c12_L79", (EP_FORM["wave"],), (EP_FORM["wave79"],)),
        "FV3_EDGE_PROFILE_REG=1": (("update_dz_d",), "c24_2x2,c12_L79", (EP_FORM["reg"],), ("edge_profile: wave form",)),
        "FV3_EDGE_PROFILE_GENERIC=1": (("update_dz_d",), "c24_2x2,c12_L79", (EP_FORM["generic"],), ("edge_profile: wave form", EP_FORM["reg"]))}
_CHILD_FAILED = {}


def _child(backend, setting, ops, shapes, want, never):
    """tests/footprint_case.py --run in a process of its own, under a time limit.  After a child has failed on a backend no further child
    is started there (whatever it was, nothing more goes to the device from here): the tests that still want one fail with its message."""
    if backend in _CHILD_FAILED or backend in _DEVICE_FAILED:
        pytest.fail(f"no further child process on {backend}: {_CHILD_FAILED.get(backend) or _DEVICE_FAILED[backend]}")
    env = {k: v for k, v in os.environ.items() if not k.startswith(("FV3_TP2D_", "FV3_RIEM_", "FV3_EDGE_PROFILE_"))}
    name, val = setting.split("=")
    env[name] = val
    env["FV3_DEBUG_FD"] = "1"
    cmd = [sys.executable, os.path.join(ROOT, "tests", "footprint_case.py"), "--run", ",".join(ops), shapes, "--backend", backend]
    try:
        p = subprocess.run(cmd, env=env, timeout=300, capture_output=True, text=True)
    except Exception as e:
        _CHILD_FAILED[backend] = f"the child with {setting} failed: {e!r}"
        raise
    if p.returncode != 0:
        if p.returncode != 1:  # (1: an assertion of the case; anything else: the process itself died)
            _CHILD_FAILED[backend] = f"the child with {setting} ended with status {p.returncode}"
        pytest.fail(f"{setting}: status {p.returncode}\n{p.stdout[-4000:]}\n{p.stderr[-4000:]}")
    for shape in shapes.split(","):
        for op in ops:
            assert f"footprint case {op} {shape} on {backend}: passed" in p.stdout, p.stdout
    for line in want:  # the form the switch asks for was taken, the default one was not
        assert line in p.stderr, (line, p.stderr[-2000:])
    for line in never:
        assert line not in p.stderr, (line, p.stderr[-2000:])


@pytest.mark.parametrize("setting", list(ONCE))
def test_operator_forms_behind_per_process_switches(backend, setting):
    _child(backend, setting, *ONCE[setting])


@pytest.mark.parametrize("op", ALL_OPS)
def test_fp32_operator_reads_and_writes_only_what_it_may(backend32, op):
    """the fp32 build (nord 2, as test_horizontal_operator_edges.FP32_SHAPES): the fp64 oracle validates the table, the fp32 library is
    compared with itself"""
    _run(backend32, fc.run_case, op, "c24_2x2", backend32, torch.float32, dict(nord=2))


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the whole acoustic call
# ---------------------------------------------------------------------------------------------------------------------------
def _plant(st, dyn, part, nz, planted):
    """NaN in everything outside the compute slice of every state field and in all of every workspace field except zs"""
    from helpers import compute_slice
    from pace_amd.dyn_core import STATE_NAMES

    for n in STATE_NAMES + ["phis"]:
        q = getattr(st, n)
        sl = compute_slice(n, part.nx, part.ny, nz)
        two_d = q.is_2d
        a = q.storage.permute(0, 2, 1) if two_d else q.storage.permute(0, 3, 2, 1)
        m = torch.ones(a.shape[1:], dtype=torch.bool, device=a.device)
        if n == "phis":  # read on the compute domain + 1 ring (riem_solver_c's zs of the C-grid heights): the caller's halo, a precondition of the call
            sl = tuple(slice(x.start - 1, x.stop + 1) for x in sl[:2])
        m[sl[:2] if two_d else sl] = False
        a[:, m] = float("nan")
        planted[n] = planted.get(n, 0) + int(m.sum()) * a.shape[0]
        assert bool(torch.isnan(q.storage).any())
    cs = dyn.cgrid_shallow_water_lagrangian_dynamics
    for w in (dyn._gz, dyn._zh, dyn._pkc, dyn._pk3, dyn._crx, dyn._cry, dyn._xfx, dyn._yfx, dyn._divgd, dyn._ut, dyn._vt, dyn._vt_scratch, dyn._heat_source, dyn._ws3, dyn._wsd,
              cs.delpc, cs.ptc):
        w.storage.fill_(float("nan"))


def _whole_call(backend, n, nz, poisoned, dtype=torch.float64, cfg_kw=None, halo_plans=True):
    from helpers import oracle_cube
    from pace_amd._testing import stencil_factory_for
    from pace_amd.constants import get_constants
    from pace_amd.dyn_core import AcousticDynamics, DycoreState
    from pace_amd.halo import Layout

    part, cfg, grids, ost, phis, _ = oracle_cube(n, (2, 2), nz, dict(n_split=2, **(cfg_kw or {})))
    sf = stencil_factory_for(backend)(grids, cfg, get_constants(), dtype=dtype)
    st = DycoreState.from_arrays(sf.quantity_factory, [dict(s, phis=p) for s, p in zip(ost, phis)])
    dyn = AcousticDynamics(Layout(part, 1, 0), grids, sf, config=cfg, phis=st.phis, state=st)
    assert dyn.native
    if not halo_plans:
        dyn.halo.native = False
    planted = {}
    for n_map in (1, 2):
        if poisoned:
            _plant(st, dyn, part, nz, planted)
        dyn(st, 225.0, n_map=n_map)
    if backend != "hostemu":
        torch.cuda.synchronize()
    return st.to_arrays(), planted, part


def _assert_whole_call(backend, n, nz, dtype=torch.float64, cfg_kw=None, halo_plans=True):
    import numpy as np

    from helpers import compute_slice

    clean, _, part = _run(backend, _whole_call, backend, n, nz, False, dtype, cfg_kw, halo_plans)
    dirty, planted, _ = _run(backend, _whole_call, backend, n, nz, True, dtype, cfg_kw, halo_plans)
    bad = []
    for r in range(part.total_ranks):
        for name in clean[r]:
            sl = compute_slice(name, part.nx, part.ny, nz)
            a, b = clean[r][name], dirty[r][name]
            a, b = (a[sl[:2]], b[sl[:2]]) if a.ndim == 2 else (a[sl], b[sl])
            assert planted[name] > 0, name
            if not (np.all(np.isfinite(a)) and fc.same(a, b)):
                bad.append(f"{name} rank {r}: {int((fc.bits(a) != fc.bits(b)).sum())} compute cells differ, {int((~np.isfinite(b)).sum())} not finite")
    assert not bad, "the acoustic call reads cells outside the compute domain that it has not filled itself:\n  " + "\n  ".join(bad[:40])


SEQ = ["", "FV3_DZ_SCAN=separate", "FV3_PINGPONG=0", "FV3_ACC_DEFER=0", "FV3_ACC_STORE=0", "FV3_DEL2_FUSED=0", "FV3_GZ_FIRST=copy", "FV3_AUX_STREAM=0", "FV3_FRAME_FIRST=1", "FV3_SEQ_DELZ=every", "FV3_SEQ_UAVA=every"]


@pytest.mark.parametrize("setting", SEQ, ids=[s or "default" for s in SEQ])
def test_acoustic_call_needs_nothing_outside_the_compute_domain(backend, monkeypatch, capfd, setting):
    """C12 2 x 2, 8 levels, n_split 2, two calls, under each switch of the sequencer (all read per call or per context).  update_dz_d's
    closing scan is riem_solver3's pre-sweep inside the sequencer only: FV3_DZ_SCAN=separate is exercised here, and asserted to act"""
    if setting:
        monkeypatch.setenv(*setting.split("="))
    monkeypatch.setenv("FV3_DEBUG_FD", "1")
    capfd.readouterr()
    _assert_whole_call(backend, 12, 8)
    err = capfd.readouterr().err
    own, deferred = "closing scan: own kernel" in err, "closing scan: left to riem_solver3's pre-sweep" in err
    assert (own, deferred) == ((True, False) if setting == "FV3_DZ_SCAN=separate" else (False, True)), err[-2000:]


def test_acoustic_call_with_a_halo_callback_needs_nothing_outside_the_compute_domain(backend):
    """the halo updates through the callback (form (b) of the integration guide) instead of registered plans: the call runs in place"""
    _assert_whole_call(backend, 12, 8, halo_plans=False)


def test_acoustic_call_on_two_segments_needs_nothing_outside_the_compute_domain(backend, monkeypatch):
    monkeypatch.setenv("FV3_SEG", "8")
    _assert_whole_call(backend, 24, 8)


def test_fp32_acoustic_call_needs_nothing_outside_the_compute_domain(backend32, monkeypatch):
    monkeypatch.setenv("FV3_SEG", "8")
    _assert_whole_call(backend32, 24, 8, torch.float32, dict(nord=2))
