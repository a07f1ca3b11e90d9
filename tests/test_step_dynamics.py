"""DynamicalCore.step_dynamics (pace_amd/fv_dynamics.py) through DycoreHarness(temperature=True) and the driver's --temperature: pt
is a temperature in K before and after a step, omga = delp / delz * w and ps are diagnosed, and the step in between is the merged
body of DycoreHarness.step and nothing else.  The step cases run on the host emulation (CPU suite) and on the HIP library (-m gpu)."""
import json
import os

import numpy as np
import pytest
import torch

import zarr_v2_read as zr
from pace_amd import driver, restart
from pace_amd._testing import harness_for
from pace_amd.dyn_core import STATE_NAMES
from pace_amd.stencils import PotentialToTemperature, TemperatureToPotential

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "c12_restart_6tiles.npz")
NH = 3
N, NZ = 12, 8
CASE = dict(nz=NZ, layout=(1, 1), dt_atmos=225.0, k_split=2, n_split=2, n_tracers=2, hord_tr=8, remap=True)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _compute(q, r):
    """the compute domain of sub-domain r (the staggered / interface end included where the quantity has one), host copy"""
    return q.sub(r).view[...].detach().cpu().numpy()


def _snapshot(h, ps):
    out = {n: [_compute(getattr(h.state, n), r) for r in range(len(h.grids))] for n in STATE_NAMES}
    for n, q in h.tracers.items():
        out[n] = [_compute(q, r) for r in range(len(h.grids))]
    out["ps"] = [_compute(ps, r) for r in range(len(h.grids))]
    return out


def _assert_same(a, b, what):
    assert set(a) == set(b)
    for n in a:
        for r, (x, y) in enumerate(zip(a[n], b[n])):
            assert x.shape == y.shape and np.array_equal(_bits(x), _bits(y)), (what, n, r, float(np.abs(x - y).max()))


# ---------------------------------------------------------------------------------------------------------------------------------
# sequencing: step_dynamics = the bookends around the merged body, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", [False, True], ids=["nofill", "fill"])
def test_step_dynamics_is_the_bookends_around_the_harness_step_bitwise(backend, fill):
    A = harness_for(backend)(N, temperature=True, fill=fill, **CASE)
    B = harness_for(backend)(N, fill=fill, **CASE)
    assert A.dycore is not None and B.dycore is None and A.dycore.fill is fill and A.dycore.ps is A.ps
    s = B.state
    to_pt, to_t = TemperatureToPotential(B.sf), PotentialToTemperature(B.sf)
    to_t(s.pt, s.pkz, s.delp, s.delz, s.q_con, s.cappa, s.w, s.pe, recompute_pkz=True)
    for step in range(2):
        A.step()
        to_pt(s.pt, s.pkz, s.delp, s.delz, s.q_con, s.cappa)
        B.step()
        to_t(s.pt, s.pkz, s.delp, s.delz, s.q_con, s.cappa, s.w, s.pe, omga=s.omga, ps=B.ps, recompute_pkz=False)
        A.synchronize()
        B.synchronize()
        _assert_same(_snapshot(A, A.dycore.ps), _snapshot(B, B.ps), f"step {step}")
    t = _compute(A.state.pt, 0)[..., :NZ]
    assert np.isfinite(t).all() and 100.0 < t.min() and t.max() < 380.0
    A.close()
    B.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# meaning: on the real restart state pt is the fixture's temperature, omga and ps are what their names say
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", [False, True], ids=["nofill", "fill"])
def test_pt_is_a_temperature_and_omga_ps_are_diagnosed(backend, fill):
    data = np.load(FIXTURE)
    nz = data["T"].shape[1]
    kw = dict(nz=nz, layout=(1, 1), dt_atmos=450.0, k_split=1, n_split=3, init="restart", init_data=data, ak=data["ak"], bk=data["bk"], n_tracers=1, hord_tr=8,
              remap=True, fill=fill)
    h = harness_for(backend)(N, temperature=True, vapor="tracer0", **kw)
    cs = (slice(NH, NH + N), slice(NH, NH + N), slice(0, nz))
    worst = 0.0
    for r in range(6):
        want = np.transpose(data["T"][h.part.tile_index(r)], (2, 1, 0))
        assert np.array_equal(h.tracers["tracer0"].numpy(r)[cs], np.transpose(data["sphum"][h.part.tile_index(r)], (2, 1, 0)))
        worst = max(worst, float(np.abs(h.state.pt.numpy(r)[cs] - want).max() / np.abs(want).max()))
    print(f"step_dynamics {backend}: pt of the restart state against the fixture's T: {worst:.2e}")
    assert worst <= 1.0e-12
    h.step()
    h.synchronize()
    s = h.sanity()  # the reference SafetyChecker's bounds [REF driver/pace/driver/driver.py:557-560]
    assert all(ok for _, _, ok in s.values())
    assert 100.0 <= s["pt"][0] and s["pt"][1] <= 380.0, s["pt"]
    assert -1.0 <= s["delp"][0] and s["delp"][1] <= 4000.0, s["delp"]
    assert -200.0 <= s["u"][0] and s["u"][1] <= 200.0 and -200.0 <= s["v"][0] and s["v"][1] <= 200.0
    st = h.state
    for r in range(6):
        delp, delz, w = (getattr(st, n).numpy(r)[cs] for n in ("delp", "delz", "w"))
        assert np.array_equal(_bits(st.omga.numpy(r)[cs]), _bits(delp / delz * w))
        assert np.array_equal(_bits(h.dycore.ps.numpy(r)[cs[:2]]), _bits(st.pe.numpy(r)[cs[0], cs[1], nz]))
        assert np.abs(st.omga.numpy(r)[cs]).max() > 0.0
    h.close()
    # the same run in the default mode: pt is the loop's form, far below any temperature -- the defect the temperature mode removes
    d = harness_for(backend)(N, **kw)
    d.step()
    d.synchronize()
    assert d.sanity()["pt"][1] < 100.0
    d.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# the halos of pt and pkz are not model data
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", [False, True], ids=["nofill", "fill"])
def test_pt_and_pkz_halos_are_not_model_data(backend, fill):
    runs = []
    for spoil in (False, True):
        h = harness_for(backend)(N, temperature=True, fill=fill, **CASE)
        if spoil:
            for q in (h.state.pt, h.state.pkz):
                keep = q.storage[:, :, NH : NH + N, NH : NH + N].clone()
                q.storage.fill_(1.0e30)
                q.storage[:, :, NH : NH + N, NH : NH + N] = keep
        h.step()
        h.synchronize()
        runs.append(_snapshot(h, h.dycore.ps))
        h.close()
    _assert_same(runs[0], runs[1], "halo")


# ---------------------------------------------------------------------------------------------------------------------------------
# decomposition: one sub-domain per tile against four (host emulation)
# ---------------------------------------------------------------------------------------------------------------------------------
# uc / vc are not compared: the C-grid winds are workspace of the acoustic loop -- every sub-step rebuilds them from u, v before it
# reads them, nothing carries them from one step to the next -- and what the last sub-step leaves in them differs between the two
# decompositions by ~1e-27 m/s where the wind itself is ~1e-28 m/s (rounding noise of a cancellation next to a sub-domain boundary).
# The default harness without temperature=True shows the same difference in the same two fields and in no other: it is not a
# property of the step this file tests.  Every other state field, the tracers and ps are compared.
C_GRID_WORKSPACE = ("uc", "vc")


@pytest.mark.parametrize("fill", [False, True], ids=["nofill", "fill"])
def test_the_step_does_not_depend_on_the_decomposition(hostemu, fill):
    n = 24
    runs = {}
    for layout in ((1, 1), (2, 2)):
        h = harness_for(hostemu)(n, temperature=True, fill=fill, init="baroclinic", **{**CASE, "layout": layout})
        h.step()
        runs[layout] = (h, _snapshot(h, h.dycore.ps))
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
    assert 100.0 < min(x.min() for x in one["pt"]) and max(x.max() for x in one["pt"]) < 380.0
    h1.close()
    h4.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# nothing is allocated at call time
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", [False, True], ids=["nofill", "fill"])
def test_step_dynamics_allocates_nothing(backend, fill):
    h = harness_for(backend)(N, temperature=True, fill=fill, **CASE)
    h.dycore.step_dynamics(h.state)
    h.synchronize()
    on_gpu = not h.sf.hostemu
    scratch = h.sf.lib.fv3_ctx_scratch_bytes(h.sf.ctx)
    mem = torch.cuda.memory_allocated() if on_gpu else 0
    h.dycore.step_dynamics(h.state)
    h.synchronize()
    assert h.sf.lib.fv3_ctx_scratch_bytes(h.sf.ctx) == scratch and scratch > 0
    if on_gpu:
        assert torch.cuda.memory_allocated() == mem
    h.close()


def test_temperature_without_remap_is_refused(backend):
    with pytest.raises(ValueError, match="temperature=True needs remap=True"):
        harness_for(backend)(N, temperature=True, **{**CASE, "remap": False})


def test_dynamical_core_constructor_and_timers(hostemu):
    """The reference's call [REF driver/pace/driver/driver.py:494-504], a timedelta timestep, no tracers, the reference's timer names."""
    from datetime import timedelta

    from pace_amd.fv_dynamics import DynamicalCore
    from pace_amd.timer import Timer

    h = harness_for(hostemu)(N, **{**CASE, "n_tracers": 0})
    core = DynamicalCore(comm=h.layout, grid_data=h.grids, stencil_factory=h.sf, quantity_factory=h.sf.quantity_factory, damping_coefficients=None, config=h.cfg,
                         timestep=timedelta(seconds=225), phis=h.state.phis, state=h.state)
    assert core.timestep == 225.0 and core.tracers == {} and core.dp1 is None and core.cubed_to_latlon is not None and core.ps.is_2d
    s = h.state
    PotentialToTemperature(h.sf)(s.pt, s.pkz, s.delp, s.delz, s.q_con, s.cappa, s.w, s.pe, recompute_pkz=True)
    timer = Timer()
    core.step_dynamics(s, timer)
    assert timer.hits == {"DynCore": 2, "Remapping": 2, "CubedToLatLon": 1}
    t = _compute(s.pt, 0)[..., :NZ]
    assert np.isfinite(t).all() and 100.0 < t.min() and t.max() < 380.0
    with pytest.raises(ValueError, match="vapor"):
        DynamicalCore(h.layout, h.grids, h.sf, None, None, h.cfg, 225.0, h.state.phis, h.state, vapor="qvapor")
    h.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# restart files: the pt_form attribute
# ---------------------------------------------------------------------------------------------------------------------------------
def test_restart_files_say_what_pt_holds(hostemu, tmp_path):
    h = harness_for(hostemu)(N, temperature=True, **CASE)
    ranks = h.layout.local_ranks
    plain = restart.save_state(h.state, ranks, str(tmp_path / "plain"), extra=h.tracers)
    again = restart.save_state(h.state, ranks, str(tmp_path / "again"), extra=h.tracers, pt_form=None)
    marked = restart.save_state(h.state, ranks, str(tmp_path / "marked"), extra=h.tracers, pt_form=restart.PT_TEMPERATURE)
    from scipy.io import netcdf_file

    for p, a, m in zip(plain, again, marked):
        assert open(p, "rb").read() == open(a, "rb").read()  # without the argument: the bytes of a file written before it existed
        with netcdf_file(p, "r", mmap=False) as f:
            assert list(f._attributes) == ["history", "rank"]
        with netcdf_file(m, "r", mmap=False) as f:
            assert list(f._attributes) == ["history", "rank", "pt_form"] and f.pt_form == b"temperature"
            assert np.array_equal(np.array(f.variables["pt"][:]), h.state.pt.numpy(f.rank))
    assert restart.pt_form(str(tmp_path / "plain"), 0) is None and restart.pt_form(str(tmp_path / "marked"), 5) == "temperature"
    restart.check_pt_form(ranks, str(tmp_path / "plain"), temperature=False)
    restart.check_pt_form(ranks, str(tmp_path / "marked"), temperature=True)
    with pytest.raises(ValueError, match="has no pt_form") as e:
        restart.check_pt_form(ranks, str(tmp_path / "plain"), temperature=True)
    assert str(e.value).count(". ") == 0 and str(e.value).endswith(".")  # one sentence
    with pytest.raises(ValueError, match='has pt_form = "temperature"') as e:
        restart.check_pt_form(ranks, str(tmp_path / "marked"), temperature=False)
    assert str(e.value).count(". ") == 0 and str(e.value).endswith(".")
    h.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# driver
# ---------------------------------------------------------------------------------------------------------------------------------
YAML = """
dycore_only: true
disable_step_physics: true
initialization:
  type: analytic
  config:
    case: baroclinic
performance_config:
  experiment_name: c12_temperature
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
BLOCK = """
output_frequency: 1
diagnostics_config:
  path: {path}
  output_format: zarr
  names: [pt, omga, ps, delp, delz, w, qvapor]
"""


def test_driver_temperature_needs_remap(tmp_path):
    p = tmp_path / "c.yaml"
    p.write_text(YAML)
    with pytest.raises(SystemExit) as e:
        driver.main([str(p), "--temperature", "--tracers", "2"])
    assert "--temperature needs --remap" in str(e.value)


@pytest.mark.gpu
def test_driver_temperature_run_stores_pt_omga_ps(tmp_path, gpu_backend, capsys):
    p, out, store = tmp_path / "c.yaml", tmp_path / "perf.json", tmp_path / "store"
    p.write_text(YAML + BLOCK.format(path=store))
    assert driver.main([str(p), "--steps", "2", "--tracers", "2", "--remap", "--temperature", "--out", str(out)]) == 0
    said = capsys.readouterr().out
    assert '"pt": "temperature"' in said and "does not hold qvapor -- dropped" in said  # ps is stored, not dropped
    d = json.load(open(out))
    assert d["setup"]["pt"] == "temperature" and d["setup"]["finite"] and set(d["times"]) == {"mainloop", "DynCore", "TracerAdvection", "Remapping"}
    store = str(store)
    assert {"pt", "omga", "ps", "delp"} <= set(zr.names(store)) and "qvapor" not in zr.names(store)
    pt, omga, ps = zr.read(store, "pt"), zr.read(store, "omga"), zr.read(store, "ps")
    assert pt.shape == (2, 6, 79, 12, 12) and ps.shape == (2, 6, 12, 12)
    assert 100.0 <= pt.min() and pt.max() <= 380.0
    assert 9.0e4 < ps.min() and ps.max() < 1.1e5
    assert np.array_equal(_bits(omga), _bits(zr.read(store, "delp") / zr.read(store, "delz") * zr.read(store, "w"))) and np.abs(omga).max() > 0.0
    # the default mode says so too, and keeps dropping ps
    sub = tmp_path / "default"
    sub.mkdir()
    p2, out2 = sub / "c.yaml", sub / "perf.json"
    p2.write_text(YAML + BLOCK.format(path=sub / "store"))
    assert driver.main([str(p2), "--steps", "1", "--tracers", "2", "--remap", "--out", str(out2)]) == 0
    assert '"pt": "loop"' in capsys.readouterr().out
    assert json.load(open(out2))["setup"]["pt"] == "loop" and "ps" not in zr.names(str(sub / "store"))
    assert zr.read(str(sub / "store"), "pt").max() < 100.0


@pytest.mark.gpu
def test_driver_restart_modes_do_not_mix(tmp_path, gpu_backend, capsys):
    p = tmp_path / "c.yaml"
    p.write_text(YAML)
    common = [str(p), "--steps", "1", "--tracers", "2", "--remap", "--out", str(tmp_path / "perf.json")]
    t_dir, l_dir = str(tmp_path / "restart_t"), str(tmp_path / "restart_loop")
    assert driver.main(common + ["--temperature", "--save-restart", t_dir]) == 0
    assert driver.main(common + ["--save-restart", l_dir]) == 0
    assert restart.pt_form(t_dir, 0) == "temperature" and restart.pt_form(l_dir, 0) is None
    # temperature -> temperature continues, from the temperature the file holds
    assert driver.main(common + ["--temperature", "--restart", t_dir, "--save-restart", str(tmp_path / "restart_t2")]) == 0
    assert "state loaded from" in capsys.readouterr().out
    from scipy.io import netcdf_file

    with netcdf_file(os.path.join(str(tmp_path / "restart_t2"), "restart_dycore_state_0.nc"), "r", mmap=False) as f:
        t = np.array(f.variables["pt"][:])[NH : NH + 12, NH : NH + 12, :79]
    assert 100.0 <= t.min() and t.max() <= 380.0
    # ... and the two refusals, one sentence each
    with pytest.raises(SystemExit) as e:
        driver.main(common + ["--restart", t_dir])
    assert 'has pt_form = "temperature"' in str(e.value) and "without --temperature" in str(e.value)
    with pytest.raises(SystemExit) as e:
        driver.main(common + ["--temperature", "--restart", l_dir])
    assert "has no pt_form" in str(e.value) and "--temperature run restarts only from files written by one" in str(e.value)
