"""d_sw's plan, pinned: which forms and level ranges one fv3_d_sw call chooses (its FV3_DEBUG_FD report: the ``[d_sw]`` lines of dsw_plan and of the marches it
dispatches to) for every configuration of the matrix and every per-call switch, on two small shapes:

  c12_2x2   6 x 6 sub-domains: every level goes through the staged wind kernels
  c24_2x2   12 x 12, FV3_SEG=8, 6 levels: sponge layers 0..2 staged, the fused wind stage on 3..5

tests/golden/d_sw_plan_lines.json holds the expected lines, one section per backend (the host emulation has no auxiliary stream: nothing forks there).  They
were recorded from the commit BEFORE the plan existed (the decisions then still interleaved with the launches), by a script outside the suite, so the file
says what the operator did, not what this code prints."""
import json
import os

import numpy as np
import pytest

import horizontal_case as hc
from test_horizontal_operator_edges import CONFIGS, case

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "d_sw_plan_lines.json")))
SWITCHES = [("FV3_DSW_SCALARS", "separate"), ("FV3_DSW_SCALARS", "quad"), ("FV3_DSW_DELN", "arrays"), ("FV3_DSW_MARCH", "old"), ("FV3_DSW_MARCH", "coupled"),
            ("FV3_DSW_VORT_DELN", "arrays"), ("FV3_DSW_WINDSTAGE", "staged"), ("FV3_DSW_SPONGE_WIND", "serial"), ("FV3_DSW_HEAT", "separate"), ("FV3_DSW_SIDE", "copy"),
            ("FV3_DSW_VORT_IN_KE", "1")]
CASES = [(kw, {}) for kw in CONFIGS] + [({}, {k: v}) for k, v in SWITCHES]


def _key(shape, kw, env):
    return f"{shape}|{','.join(f'{k}={v}' for k, v in kw.items()) or 'default'}|{','.join(f'{k}={v}' for k, v in env.items()) or '-'}"


@pytest.mark.parametrize("shape", ["c12_2x2", "c24_2x2"])
def test_d_sw_plan_lines_match_the_recorded_ones(backend, monkeypatch, capfd, shape):
    """one d_sw call per configuration and per switch; no case is left out (every key of the shape in the golden section is visited)"""
    want = GOLDEN[backend]
    monkeypatch.setenv("FV3_DEBUG_FD", "1")
    seen = set()
    for kw, env in CASES:
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            cs = case(shape, backend, mp, kw)
            ins = hc.smooth(cs)
            Q = {n: cs.q([np.concatenate([x[n], x[n][:, :, -1:]], axis=2) for x in ins]) if n in hc.D_SW_IN else cs.q() for n in hc.D_SW_ARGS}
            capfd.readouterr()
            cs.sf.call("d_sw", *[Q[n].fref for n in hc.D_SW_ARGS], 60.0)
            if backend != "hostemu":
                import torch

                torch.cuda.synchronize()
            got = [line for line in capfd.readouterr().err.splitlines() if line.startswith("[d_sw]")]
        key = _key(shape, kw, env)
        assert got == want[key], (key, got, want[key])
        seen.add(key)
    assert seen == {k for k in want if k.startswith(shape + "|")} and len(seen) == len(CONFIGS) + len(SWITCHES)
