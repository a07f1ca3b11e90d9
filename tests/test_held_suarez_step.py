"""The step with the Held-Suarez forcing: ``DycoreHarness(held_suarez=True)`` is ``DynamicalCore.step_dynamics`` followed by HeldSuarezForcing and
ApplyPhysicsToDycore called by hand, bit for bit; it does not depend on the decomposition; without the switch nothing changes; the driver's
flag, refusal and json key; the tool."""
import importlib.util
import json
import os

import numpy as np
import pytest

from pace_amd import driver
from pace_amd._testing import harness_for
from pace_amd.dyn_core import STATE_NAMES
from pace_amd.stencils import ApplyPhysicsToDycore, HeldSuarezConfig, HeldSuarezForcing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, NZ, STEPS = 12, 8, 2
CASE = dict(nz=NZ, layout=(1, 1), dt_atmos=225.0, k_split=2, n_split=2, n_tracers=2, hord_tr=8, remap=True, temperature=True, latlon_winds=True, init="baroclinic")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _compute(q, r):
    return q.sub(r).view[...].detach().cpu().numpy()


def _snapshot(h):
    out = {n: [_compute(getattr(h.state, n), r) for r in range(len(h.grids))] for n in STATE_NAMES}
    for n, q in h.tracers.items():
        out[n] = [_compute(q, r) for r in range(len(h.grids))]
    out["ps"] = [_compute(h.dycore.ps, r) for r in range(len(h.grids))]
    return out


def _assert_same(a, b, what):
    assert set(a) == set(b)
    for n in a:
        for r, (x, y) in enumerate(zip(a[n], b[n])):
            assert x.shape == y.shape and np.array_equal(_bits(x), _bits(y)), (what, n, r, float(np.abs(x - y).max()))


def test_harness_step_is_step_dynamics_plus_the_two_operators(backend):
    """Two steps at C12, nz = 8.  The timer sees the clocks "HeldSuarez" and "ApplyPhysics" once per step; the forced run differs from the
    unforced one (the JW2006 temperature is not the Held-Suarez equilibrium)."""
    from pace_amd.timer import Timer

    A = harness_for(backend)(N, held_suarez=True, **CASE)
    B = harness_for(backend)(N, **CASE)
    C = harness_for(backend)(N, **CASE)
    qf = B.sf.quantity_factory
    forcing = HeldSuarezForcing(B.sf, qf, B.grids)
    apply = ApplyPhysicsToDycore(B.sf, qf, B.grids, comm=B.layout)
    cell = ("x", "y", "z")
    u_dt, v_dt, t_dt = qf.zeros(cell), qf.zeros(cell), qf.zeros(cell)
    timer = Timer()
    for _ in range(STEPS):
        A.step(timer)
        s = B.state
        B.dycore.step_dynamics(s)
        forcing(s.ua, s.va, s.pt, s.delp, u_dt, v_dt, t_dt, B.cfg.dt_atmos)
        apply(s, u_dt, v_dt, t_dt, B.cfg.dt_atmos)
        C.step()
    for h in (A, B, C):
        h.synchronize()
    assert timer.hits["HeldSuarez"] == STEPS and timer.hits["ApplyPhysics"] == STEPS and timer.hits["DynCore"] == STEPS * CASE["k_split"]
    a, b, c = _snapshot(A), _snapshot(B), _snapshot(C)
    _assert_same(a, b, "harness against the operators by hand")
    for n in ("u", "v", "pt"):
        assert any(not np.array_equal(x, y) for x, y in zip(a[n], c[n])), n
    assert all(np.isfinite(x).all() for n in a for x in a[n])
    for h in (A, B, C):
        h.close()


def test_without_the_switch_nothing_changes(backend):
    """held_suarez=False is bitwise a harness built without the argument, and builds neither operator nor buffer."""
    A = harness_for(backend)(N, held_suarez=False, **CASE)
    B = harness_for(backend)(N, **CASE)
    for _ in range(STEPS):
        A.step()
        B.step()
    A.synchronize(), B.synchronize()
    _assert_same(_snapshot(A), _snapshot(B), "held_suarez=False against no argument")
    assert A.held_suarez is None and A.apply_physics is None and not hasattr(A, "u_dt")
    D = harness_for(backend)(N, **{**CASE, "temperature": False, "n_tracers": 0})
    assert D.held_suarez is None
    for h in (A, B, D):
        h.close()


# the C-grid winds are workspace of the acoustic sub-step, not model state (tests/test_step_dynamics.py compares every other field too)
C_GRID_WORKSPACE = ("uc", "vc")


def test_the_forced_step_does_not_depend_on_the_decomposition(backend):
    """1 x 1 against 2 x 2 (6 x 6 sub-domains), two forced steps: every state field, the tracers and ps, bit for bit."""
    runs = {}
    for layout in ((1, 1), (2, 2)):
        h = harness_for(backend)(N, held_suarez=True, **{**CASE, "layout": layout})
        for _ in range(STEPS):
            h.step()
        h.synchronize()
        runs[layout] = (h, _snapshot(h))
    h1, one = runs[(1, 1)]
    h4, four = runs[(2, 2)]
    for r in range(len(h4.grids)):
        tile, (ox, oy) = h4.part.tile_index(r), h4.part.origin(r)
        for name, subs in four.items():
            if name in C_GRID_WORKSPACE:
                continue
            a = subs[r]
            want = one[name][tile][ox : ox + a.shape[0], oy : oy + a.shape[1]]
            assert np.array_equal(_bits(a), _bits(want)), (name, r, float(np.abs(a - want).max()))
    h1.close()
    h4.close()


def test_harness_refusals_and_config(hostemu):
    mk = harness_for(hostemu)
    for drop in ("temperature", "latlon_winds"):
        with pytest.raises(ValueError, match="held_suarez=True needs temperature=True, remap=True and latlon_winds=True"):
            mk(N, held_suarez=True, **{**CASE, drop: False})
    with pytest.raises(ValueError, match="held_suarez=True needs"):
        mk(N, held_suarez=True, **{**CASE, "remap": False, "temperature": False})
    h = mk(N, held_suarez=True, held_suarez_config=HeldSuarezConfig(t_min=210.0), **CASE)
    assert h.held_suarez.config.t_min == 210.0 and h.held_suarez.params.t_min == 210.0
    h.close()


YAML = """
dycore_only: true
disable_step_physics: true
performance_config:
  experiment_name: c12_held_suarez
nx_tile: 12
nz: 79
dt_atmos: 225
minutes: 15
layout: [1, 1]
dycore_config:
  a_imp: 1.0
  beta: 0.
  d4_bg: 0.15
  hord_dp: 6
  hord_tr: 8
  k_split: 1
  n_split: 2
  nord: 3
  n_sponge: 48
"""


def test_driver_held_suarez_refusal(tmp_path):
    p = tmp_path / "c.yaml"
    p.write_text(YAML)
    for flags in (["--temperature", "--remap"], ["--remap", "--latlon-winds"], []):
        with pytest.raises(SystemExit) as e:
            driver.main([str(p), "--held-suarez", "--tracers", "2"] + flags)
        msg = str(e.value)
        assert "--held-suarez needs --temperature --remap --latlon-winds" in msg and msg.count(". ") == 0  # one sentence


@pytest.mark.gpu
def test_driver_held_suarez_run(tmp_path, gpu_backend, capsys):
    p, out = tmp_path / "c.yaml", tmp_path / "perf.json"
    p.write_text(YAML)
    common = [str(p), "--steps", "2", "--tracers", "2", "--remap", "--temperature", "--latlon-winds", "--out", str(out)]
    assert driver.main(common + ["--held-suarez"]) == 0
    assert '"forcing": "held_suarez"' in capsys.readouterr().out
    d = json.load(open(out))
    assert d["setup"]["forcing"] == "held_suarez" and d["setup"]["finite"]
    assert {"HeldSuarez", "ApplyPhysics", "CubedToLatLon", "mainloop"} <= set(d["times"])
    assert driver.main(common) == 0
    assert '"forcing": "none"' in capsys.readouterr().out
    d = json.load(open(out))
    assert d["setup"]["forcing"] == "none" and "HeldSuarez" not in d["times"]


def test_tool_two_steps_end_finite(backend):
    spec = importlib.util.spec_from_file_location("held_suarez_tool", os.path.join(ROOT, "tools", "held_suarez.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    lines = []
    res = tool.run(12, steps=2, nz=NZ, every_h=1.0, make_harness=harness_for(backend), say=lines.append)
    assert res["steps"] == 2 and len(res["records"]) == 2 and all(r["finite"] for r in res["records"])
    last = res["records"][-1]
    assert 990.0 < last["ps_min_hPa"] <= last["ps_max_hPa"] < 1010.0
    t = np.array(last["t"])
    assert np.all(np.isfinite(t)) and np.all(np.abs(t - 300.0) < 5.0)  # two hours of forcing move the temperature by less than a kelvin
    assert np.all(np.abs(np.array(last["ua"])) < 5.0)
    assert any("hPa  ua" in s for s in lines)
