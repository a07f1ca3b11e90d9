"""The plans of the column height chain, pinned: every line that update_dz_d, riem_solver_c, riem_solver3 and the fv_tp_2d they call report under FV3_DEBUG_FD
(the ``[update_dz_d]``, ``[riem_solver_c]``, ``[riem_solver3]`` and ``[fv_tp_2d]`` lines: forms, level ranges -- hence where the del-n chain moves into the
march -- and who runs the closing scan), in the order they come, for

  dzd    update_dz_d alone on C24 2 x 2 L8 (12 x 12 sub-domains, two segments) and C12 L79, default and under each per-call switch
  riem   riem_solver_c and riem_solver3 (last_call 0 and 1) alone on C12 at 8, 79 and 81 levels
  child  the forms chosen once per process, each in a child process of the existing case scripts (tests/column_case.py, tests/height_pgf_forms_case.py)
  step   one fv3_acoustic_step of two sub-steps on the whole C24 2 x 2 L8 cube: default, FV3_DZ_SCAN=separate, FV3_FRAME_FIRST=1

tests/golden/column_plan_lines.json holds the expected lines, one section per backend (the host emulation has no auxiliary stream and no frame-first
transport).  They were recorded from the commit BEFORE the plans existed (the decisions then still spread over fv3_nh.hip), by
tools/record_column_plan_lines.py, which is not part of the suite, so the file says what the operators did, not what this code prints."""
import contextlib
import json
import os
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "column_plan_lines.json")
TAGS = ("[update_dz_d]", "[riem_solver_c]", "[riem_solver3]", "[fv_tp_2d]")

DZD_CASES = ("c24_2x2:8", "c12:79")
DZD_LIVE = ("", "FV3_DZ_DELN=arrays", "FV3_TP2D_MARCH=old", "FV3_DZ_SCAN=separate")
RIEM_LEVELS = (8, 79, 81)
RIEM_ONCE = ("FV3_RIEM_MODE=columns", "FV3_RIEM_MODE=wave", "FV3_RIEM_REGS=0")  # (test_column_solver_edges.FORMS)
RIEM_CHILD_CASES = "riem:floor:8,riem:floor:79,riem:floor:127"
DZD_ONCE = ("FV3_EDGE_PROFILE_GENERIC=1", "FV3_EDGE_PROFILE_REG=1", "FV3_EDGE_PROFILE_LDS=1", "FV3_EP_ONE_LAUNCH=0", "FV3_TP2D_MODE=staged", "FV3_DEL6_MODE=staged",
            "FV3_TP2D_FA=0")  # (test_height_pgf_operator_edges.ONCE)
STEP_VARIANTS = ("", "FV3_DZ_SCAN=separate", "FV3_FRAME_FIRST=1")
CHILDREN = [("column_case", s) for s in RIEM_ONCE] + [("height_pgf_forms_case", s) for s in DZD_ONCE]


def key(group, what, setting):
    return f"{group}|{what}|{setting or '-'}"


KEYS = ([key("dzd", c, s) for c in DZD_CASES for s in DZD_LIVE] + [key("riem", f"L{nz}", "") for nz in RIEM_LEVELS] + [key("child", script, s) for script, s in CHILDREN]
        + [key("step", "c24_2x2", s) for s in STEP_VARIANTS])


def report(err):
    return [ln for ln in err.splitlines() if ln.startswith(TAGS)]


@contextlib.contextmanager
def environment(setting):
    """FV3_DEBUG_FD and one ``NAME=value`` setting in os.environ (the per-call switches are read there at every call), put back afterwards"""
    new = {"FV3_DEBUG_FD": "1"}
    if setting:
        name, val = setting.split("=")
        new[name] = val
    old = {k: os.environ.get(k) for k in list(new) + ["FV3_SEG"]}
    os.environ.update(new)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@contextlib.contextmanager
def stderr_of_the_library():
    """what the C library writes to file descriptor 2 inside the block, as ``.text`` afterwards"""

    class Out:
        text = ""

    out = Out()
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as f:
        os.dup2(f.fileno(), 2)
        try:
            yield out
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            f.seek(0)
            out.text = f.read().decode()


def _sync(backend):
    if backend != "hostemu":
        import torch

        torch.cuda.synchronize()


def lines_dzd(backend, name, setting):
    import test_height_pgf_operator_edges as hpe

    with environment(setting):
        cs, args, _ = hpe.forms_case(name, backend, os.environ.__setitem__)
        with stderr_of_the_library() as out:
            hpe.library("update_dz_d", cs, [dict(ins=list(a[1:]), D=a[0]) for a in args])
            _sync(backend)
    return report(out.text)


def lines_riem(backend, nz):
    import test_column_solver_edges as cse

    with environment(""):
        cs, x = cse.column_case(nz, "floor", backend)
        calls = cse.column_calls(cs, x, ops=("riem_solver_c", "riem_solver3_0", "riem_solver3_1"))
        dv = cse.device(backend, cs.grids, cs.cfg)
        with stderr_of_the_library() as out:
            for k, cl in calls.items():
                cse.replay(dv, cse.op_of(k), [cl])
            _sync(backend)
    return report(out.text)


def lines_child(backend, script, setting, tmp):
    """one child process of an existing case script with the forms of ``setting``, under its own time limit; its stderr"""
    once = [s.split("=")[0] for s in RIEM_ONCE + DZD_ONCE]
    env = {k: v for k, v in os.environ.items() if k not in once}
    env["FV3_DEBUG_FD"] = "1"
    name, val = setting.split("=")
    env[name] = val
    cases = RIEM_CHILD_CASES if script == "column_case" else ",".join(DZD_CASES)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", script + ".py"), "--cases", cases, "--backend", backend, "--out", os.path.join(str(tmp), "out.npz")],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (script, setting, r.returncode, r.stderr[-2000:])
    return report(r.stderr)


_CUBE = {}


def lines_step(backend, setting):
    from helpers import oracle_cube, run_device_cube

    if not _CUBE:
        part, cfg, grids, ost, phis, _ = oracle_cube(24, (2, 2), 8, dict(n_split=2))
        _CUBE["c24_2x2"] = (part, cfg, grids, ost, phis)
    part, cfg, grids, ost, phis = _CUBE["c24_2x2"]
    with environment(setting):
        os.environ["FV3_SEG"] = "8"  # (the shape c24_2x2 of test_horizontal_operator_edges.SHAPES)
        init = [{k: v.copy() for k, v in s.items()} for s in ost]
        with stderr_of_the_library() as out:
            run_device_cube(backend, part, cfg, grids, init, phis, 225.0)
    return report(out.text)


def collect(backend, tmp, keys=KEYS):
    """{key: lines} of the named cases on one backend: what tools/record_column_plan_lines.py writes into the golden file"""
    got = {}
    for k in keys:
        group, what, setting = k.split("|")
        setting = "" if setting == "-" else setting
        got[k] = (lines_dzd(backend, what, setting) if group == "dzd" else lines_riem(backend, int(what[1:])) if group == "riem"
                  else lines_child(backend, what, setting, tmp) if group == "child" else lines_step(backend, setting))
    return got


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))


def test_the_golden_file_holds_exactly_the_cases_of_this_module(golden):
    """so that the case tests below, each asserting its own key, visit every key of both sections"""
    assert sorted(golden) == ["hip:gfx950", "hostemu"]
    for section in golden.values():
        assert sorted(section) == sorted(KEYS)
        assert all(lines and all(ln.startswith(TAGS) for ln in lines) for lines in section.values())


_CHILD_FAILED = {}


@pytest.mark.parametrize("k", KEYS)
def test_plan_lines_match_the_recorded_ones(backend, golden, tmp_path, k):
    if k.startswith("child|"):  # (as test_column_solver_edges._child: after a failed child no further one is started on that backend)
        if backend in _CHILD_FAILED:
            pytest.fail(f"no further child process on {backend}: {_CHILD_FAILED[backend]}")
        try:
            got = collect(backend, tmp_path, [k])[k]
        except Exception as e:
            _CHILD_FAILED[backend] = f"the child of {k} failed: {e!r}"
            raise
    else:
        got = collect(backend, tmp_path, [k])[k]
    assert got == golden[backend][k], (k, got, golden[backend][k])
