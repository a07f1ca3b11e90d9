"""The kernel-form switches (pace_amd/csrc/fv3_switch.h): one table, the only reader of the environment in the library.

CPU only.  The table is checked against the sources, INTEGRATION.md §2 and the toggles of the A/B test; its parsing and
its read-once / per-call policies are checked on stand-alone programs that include nothing but the header, each run as
a fresh child process."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pace_amd", "csrc")
HEADER = os.path.join(CSRC, "fv3_switch.h")
ROW = re.compile(r'^\s*X\((\w+), "(FV3_\w+)", (ONCE|LIVE), (\w+), "([^"]*)", (-?\d+), "(.*)"\)\s*\\?\s*$')
KINDS = {"present", "off_if_0", "on_if_1", "tri", "word", "integer", "names"}


def _rows():
    """[(identifier, environment name, policy, kind, [words], integer default, description)] in table order."""
    lines = open(HEADER).read().splitlines()
    rows = [ROW.match(ln) for ln in lines if re.match(r"\s*X\(\w+, \"", ln)]
    assert rows and all(rows), "every X(...) row of the table is one line of the documented shape"
    return [(m[1], m[2], m[3], m[4], m[5].split("|") if m[5] else [], int(m[6]), m[7]) for m in rows]


ROWS = _rows()
BY_NAME = {r[1]: r for r in ROWS}


def test_only_the_switch_header_reads_the_environment():
    readers = sorted(f for f in os.listdir(CSRC) if os.path.isfile(os.path.join(CSRC, f)) and not f.endswith(".so") and "getenv" in open(os.path.join(CSRC, f), errors="replace").read())
    assert readers == ["fv3_switch.h"]


def test_table_rows_are_unique_and_well_formed():
    assert len({r[0] for r in ROWS}) == len(ROWS) and len(BY_NAME) == len(ROWS)
    for ident, name, _policy, kind, words, _dflt, what in ROWS:
        assert name == "FV3_" + ident and kind in KINDS and what
        assert bool(words) == (kind == "word"), name
        assert "default" in what, f"{name}: the description names the default form"


def _doc_rows():
    """{name: policy} of the switch table of INTEGRATION.md §2, and the names in their order."""
    lines = open(os.path.join(ROOT, "INTEGRATION.md")).read().splitlines()
    start = [i for i, ln in enumerate(lines) if re.match(r"\|\s*switch\s*\|\s*values\s*\|\s*default\s*\|\s*read\s*\|", ln)]
    assert len(start) == 1
    out = []
    for ln in lines[start[0] + 2 :]:
        if not ln.startswith("|"):
            break
        cells = [c.strip() for c in ln.strip().strip("|").split("|")]
        assert len(cells) == 5 and re.fullmatch(r"`FV3_\w+`", cells[0]) and cells[3] in ("once", "per call"), ln
        out.append((cells[0].strip("`"), "ONCE" if cells[3] == "once" else "LIVE"))
    return out


def test_integration_md_lists_the_same_rows_in_the_same_order():
    assert _doc_rows() == [(r[1], r[2]) for r in ROWS]


def test_every_toggle_of_the_ab_test_names_a_row():
    text = open(os.path.join(ROOT, "tests", "test_gpu_invariants.py")).read()
    m = re.search(r'"toggle",\s*\[([^\]]*)\],?\s*\)\s*def test_alternative_kernel_forms_agree', text)
    toggles = re.findall(r'"(FV3_\w+)=([^"]*)"', m[1])
    assert len(toggles) >= 41
    for name, val in toggles:
        assert name in BY_NAME, name
        if BY_NAME[name][3] == "word":
            assert val in BY_NAME[name][4], (name, val)


def test_switches_the_parity_tests_flip_in_one_process_are_read_per_call():
    live = "SEG ALT DEBUG_FD CSW_MARCH CSW_B_GENERIC PINGPONG ACC_DEFER ACC_STORE GZ_FIRST SEQ_DELZ SEQ_UAVA FRAME_FIRST NH_PGF DZ_SCAN DZ_DELN DEL2_FUSED DEL2_HEAT".split()
    text = open(os.path.join(ROOT, "tests", "test_parity.py")).read()
    live += [n[4:] for n in re.findall(r'setenv\("(FV3_DSW_\w+)"', text)]
    for ident in live:
        assert BY_NAME["FV3_" + ident][2] == "LIVE", ident
    # the three that were read once at one site and per call at another are read once everywhere
    for ident in ("KE_STAGED", "TP2D_MODE", "DEL6_MODE"):
        assert BY_NAME["FV3_" + ident][2] == "ONCE", ident


def _compile(tmp, name, body):
    src = tmp / (name + ".cpp")
    src.write_text('#include "fv3_switch.h"\n#include <cstdio>\nint main() {\n' + body + "  return 0;\n}\n")
    exe = tmp / name
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    return str(exe)


def _run(exe, env):
    base = {k: v for k, v in os.environ.items() if not k.startswith("FV3_")}
    return subprocess.run([exe], env=dict(base, **env), check=True, capture_output=True, text=True, timeout=60).stdout


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """Program that prints fv3_sw() of every row, fv3_sw_is() of every listed word and two fv3_alt() names."""
    body = ""
    for ident, name, _p, _k, words, _d, _w in ROWS:
        body += f'  printf("{name} %d\\n", fv3_sw(FV3SW_{ident}));\n'
        for w in words + ["nosuchword"] if words else []:
            body += f'  printf("{name}={w} %d\\n", (int)fv3_sw_is(FV3SW_{ident}, "{w}"));\n'
    body += '  printf("alt %d%d\\n", (int)fv3_alt("dz_damp_scaled"), (int)fv3_alt("heat_dt_full"));\n'
    return _compile(tmp_path_factory.mktemp("sw"), "dump", body)


def _dump(exe, env):
    return dict(ln.rsplit(" ", 1) for ln in _run(exe, env).splitlines())


def _expected(kind, words, dflt, v):
    """fv3_sw() by the rules of the kinds; v is None: unset."""
    if kind in ("present", "names"):
        return int(v is not None)
    if kind == "off_if_0":
        return int(not (v is not None and v[:1] == "0"))
    if kind == "on_if_1":
        return int(v is not None and v[:1] == "1")
    if kind == "tri":
        return -1 if v is None else 0 if v[:1] == "0" else 1 if v[:1] == "1" else 2
    if kind == "word":
        return words.index(v) + 1 if v in words else 0
    m = re.match(r"\s*[-+]?\d+", v or "")  # integer: atoi
    return dflt if v is None else int(m[0]) if m else 0


ALL_WORDS = sorted({w for r in ROWS for w in r[4]})


@pytest.mark.parametrize("value", [None, "", "0", "1", "junk", "-3", "96"] + [w for w in ALL_WORDS if w != "0"])
def test_every_row_parses_by_the_rule_of_its_kind(dump, value):
    got = _dump(dump, {} if value is None else {r[1]: value for r in ROWS})
    for _ident, name, _p, kind, words, dflt, _w in ROWS:
        want = _expected(kind, words, dflt, value)
        assert int(got[name]) == want, (name, kind, value)
        for w in words:
            assert int(got[f"{name}={w}"]) == int(value == w), (name, w, value)
        if words:
            assert got[f"{name}=nosuchword"] == "0"


def test_the_idioms_of_the_old_call_sites(dump):
    """The figures the operators relied on, spelled out (not derived from the table)."""
    unset, empty, zero, one, junk = (_dump(dump, {} if v is None else {r[1]: v for r in ROWS}) for v in (None, "", "0", "1", "junk"))
    # present: set at all
    assert (unset["FV3_KE_STAGED"], empty["FV3_KE_STAGED"], zero["FV3_KE_STAGED"], one["FV3_KE_STAGED"]) == ("0", "1", "1", "1")
    assert (unset["FV3_CSW_B_GENERIC"], zero["FV3_CSW_B_GENERIC"]) == ("0", "1")
    # off_if_0: on by default, and for anything that does not start with 0
    assert (unset["FV3_PINGPONG"], empty["FV3_PINGPONG"], zero["FV3_PINGPONG"], one["FV3_PINGPONG"], junk["FV3_PINGPONG"]) == ("1", "1", "0", "1", "1")
    # on_if_1: off by default, and for anything that does not start with 1
    assert (unset["FV3_CSW_DEFER"], empty["FV3_CSW_DEFER"], zero["FV3_CSW_DEFER"], one["FV3_CSW_DEFER"], junk["FV3_CSW_DEFER"]) == ("0", "0", "0", "1", "0")
    # word: anything else is the default form
    assert (unset["FV3_TP2D_MODE=staged"], junk["FV3_TP2D_MODE=staged"], junk["FV3_TP2D_MODE"]) == ("0", "0", "0")
    assert _dump(dump, {"FV3_TP2D_MODE": "staged"})["FV3_TP2D_MODE=staged"] == "1"
    assert (zero["FV3_CSW_MARCH=0"], zero["FV3_CSW_MARCH=abc"], one["FV3_CSW_MARCH=0"]) == ("1", "0", "0")
    # integer
    assert (unset["FV3_Q4_KB"], zero["FV3_Q4_KB"], unset["FV3_KE_KB"], unset["FV3_CSW_WIN_KC"]) == ("16", "0", "16", "2")
    assert int(unset["FV3_SEG"]) <= 0 and int(_dump(dump, {"FV3_SEG": "-3"})["FV3_SEG"]) <= 0 and _dump(dump, {"FV3_SEG": "96"})["FV3_SEG"] == "96"  # <= 0: automatic
    # FV3_HORD_CONST: unset / 0 / 1 are three states (fv3_tp2d.hip, fv3_wind.hip ask "is it 0", fv3_tp4.hip "is it 1"); junk is neither 0 nor 1
    assert len({unset["FV3_HORD_CONST"], zero["FV3_HORD_CONST"], one["FV3_HORD_CONST"]}) == 3
    assert (zero["FV3_HORD_CONST"], one["FV3_HORD_CONST"]) == ("0", "1") and junk["FV3_HORD_CONST"] not in ("0", "1")
    # FV3_FRAME_FIRST: unset leaves the choice to the sequencer, 1 forces the form on, any other value off
    assert unset["FV3_FRAME_FIRST"] == "-1" and one["FV3_FRAME_FIRST"] == "1" and int(zero["FV3_FRAME_FIRST"]) >= 0 and int(junk["FV3_FRAME_FIRST"]) >= 0 and junk["FV3_FRAME_FIRST"] != "1"
    # FV3_ALT: whole names of a comma-separated list
    assert unset["alt"] == "00"
    assert _dump(dump, {"FV3_ALT": "heat_dt_full"})["alt"] == "01"
    assert _dump(dump, {"FV3_ALT": "heat_zero_first_call, dz_damp_scaled,heat_dt_full"})["alt"] == "11"
    assert _dump(dump, {"FV3_ALT": "dz_damp_scaled_not,xheat_dt_full"})["alt"] == "00"


def test_once_rows_keep_their_first_answer_and_live_rows_follow(tmp_path):
    once = next(r for r in ROWS if r[1] == "FV3_Q4_KB")
    live = next(r for r in ROWS if r[1] == "FV3_SEG")
    assert once[2] == "ONCE" and live[2] == "LIVE"
    q = '  printf("%d %d\\n", fv3_sw(FV3SW_Q4_KB), fv3_sw(FV3SW_SEG));\n'
    body = q + '  setenv("FV3_Q4_KB", "8", 1);\n  setenv("FV3_SEG", "32", 1);\n' + q + '  unsetenv("FV3_Q4_KB");\n  unsetenv("FV3_SEG");\n' + q
    exe = _compile(tmp_path, "cache", body)
    assert _run(exe, {}).split() == ["16", "0", "16", "32", "16", "0"]
    assert _run(exe, {"FV3_Q4_KB": "4", "FV3_SEG": "96"}).split() == ["4", "96", "4", "32", "4", "0"]
