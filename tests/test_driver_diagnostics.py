"""The driver's ``diagnostics_config`` block: parsing and name filtering on CPU; on the GPU a short run of ``driver.main`` that writes a
Zarr store, and the two-process store of tests/diag_case.py."""
import json
import os

import numpy as np
import pytest

import zarr_v2_read as zr
from pace_amd import driver
from test_driver import YAML

BLOCK = """
output_initial_state: true
output_frequency: 2
diagnostics_config:
  path: {path}
  output_format: zarr
  names: [u, v, ua, va, pt, delp, qvapor, qliquid, ps]
  derived_names: [column_integrated_tracer1, column_integrated_qrain]
  z_select:
    - level: 65
      names: [pt, qvapor]
    - level: 3
      names: [qice]
"""


def test_load_config_returns_the_diagnostics_fields(tmp_path):
    p = tmp_path / "c.yaml"
    p.write_text(YAML + BLOCK.format(path="output"))
    run, _, _ = driver.load_config(str(p))
    assert run["output_initial_state"] is True and run["output_frequency"] == 2 and run["start_time"] is None
    d = run["diagnostics_config"]
    assert d["path"] == "output" and d["output_format"] == "zarr" and d["names"][:2] == ["u", "v"] and d["z_select"][0] == {"level": 65, "names": ["pt", "qvapor"]}
    p.write_text(YAML.replace("    case: baroclinic", "    case: baroclinic\n    start_time: 2016-08-01 00:00:00"))
    run, _, _ = driver.load_config(str(p))  # no block: the defaults of the reference's DriverConfig
    assert run["diagnostics_config"] is None and run["output_initial_state"] is False and run["output_frequency"] == 1
    from pace_amd.monitor import as_datetime

    assert as_datetime(run["start_time"]).isoformat() == "2016-08-01T00:00:00" and as_datetime(None).isoformat() == "2000-01-01T00:00:00"


def test_filtering_drops_what_this_build_does_not_hold(tmp_path):
    import yaml

    from pace_amd.diagnostics import DiagnosticsConfig
    from pace_amd.dyn_core import STATE_NAMES

    block = yaml.safe_load(BLOCK.format(path=str(tmp_path)))["diagnostics_config"]
    kept, dropped = driver.filter_diagnostics(block, STATE_NAMES + ["phis", "tracer0", "tracer1"])
    assert kept["names"] == ["u", "v", "ua", "va", "pt", "delp"]
    assert kept["derived_names"] == ["column_integrated_tracer1"]
    assert kept["z_select"] == [{"level": 65, "names": ["pt"]}]
    assert dropped == ["qvapor", "qliquid", "ps", "column_integrated_qrain", "qvapor", "qice"]
    assert block["names"][-1] == "ps"  # (the caller's block is not modified)
    c = DiagnosticsConfig.from_dict(kept)
    assert c.path == str(tmp_path) and c.z_select[0].level == 65


def _main(tmp_path, yaml_text, *extra):
    p = tmp_path / "c.yaml"
    p.write_text(yaml_text)
    out = tmp_path / "perf.json"
    assert driver.main([str(p), "--steps", "2", "--tracers", "2", "--remap", "--latlon-winds", "--out", str(out)] + list(extra)) == 0
    return json.load(open(out))


@pytest.mark.gpu
def test_driver_writes_a_zarr_store(tmp_path, gpu_backend, capsys):
    store = tmp_path / "store"
    with_block = _main(tmp_path, YAML + BLOCK.format(path=store).replace("output_frequency: 2", "output_frequency: 1"))
    said = capsys.readouterr().out
    assert "does not hold qvapor, qliquid, ps, column_integrated_qrain, qvapor, qice" in said
    store = str(store)
    assert zr.names(store) == sorted("u v ua va pt delp column_integrated_tracer1 pt_z65 time lat lon lat_agrid lon_agrid".split())
    assert np.array_equal(zr.read(store, "time"), [0.0, 225.0, 450.0])  # the initial state and two steps
    ua, u = zr.read(store, "ua"), zr.read(store, "u")
    assert ua.shape == (3, 6, 79, 12, 12) and u.shape == (3, 6, 79, 13, 12)
    assert np.isfinite(ua[2]).all() and np.abs(ua[2]).max() > 1.0
    assert not np.array_equal(ua[2], u[2][:, :, :12])  # CubedToLatLon ran before the store: eastward winds, not the D-grid component
    assert np.array_equal(zr.read(store, "pt_z65"), zr.read(store, "pt")[:, :, 65])
    ci = zr.read(store, "column_integrated_tracer1")
    assert ci.shape == (3, 6, 12, 12) and np.isfinite(ci).all() and (ci > 0).all()
    # without the block: the same timer json, and no directory
    sub = tmp_path / "plain"
    sub.mkdir()
    plain = _main(sub, YAML)
    assert set(plain) == set(with_block) and set(plain["times"]) == set(with_block["times"]) and set(plain["setup"]) == set(with_block["setup"])
    assert sorted(os.listdir(sub)) == ["c.yaml", "perf.json"]


@pytest.mark.gpu
def test_driver_flags_override_the_block(tmp_path, gpu_backend):
    """--diagnostics-path overrides the block's path (and output_frequency 2 over 2 steps stores the initial state and step 2);
    --no-diagnostics ignores the block."""
    _main(tmp_path, YAML + BLOCK.format(path=tmp_path / "never"), "--diagnostics-path", str(tmp_path / "there"))
    assert not (tmp_path / "never").exists() and np.array_equal(zr.read(str(tmp_path / "there"), "time"), [0.0, 450.0])
    off = tmp_path / "off"
    off.mkdir()
    _main(off, YAML + BLOCK.format(path=off / "never"), "--no-diagnostics")
    assert sorted(os.listdir(off)) == ["c.yaml", "perf.json"]


@pytest.mark.gpu
def test_two_process_store_is_byte_identical_on_the_gpu(tmp_path, gpu_backend):
    """The content of the host-emulation test (tests/test_diagnostics_output.py) on hip:gfx950: two gloo processes that share device 0
    (three processes with the GPU open, this one included)."""
    from diag_case import HARNESS, NX, assert_two_process_store_is_byte_identical, config, run
    from pace_amd.harness import DycoreHarness

    h = DycoreHarness(NX, **HARNESS)
    run(h, [config(tmp_path / "zarr1", "zarr").diagnostics_factory(h)], 2, output_initial_state=True)
    h.close()
    assert_two_process_store_is_byte_identical(gpu_backend, str(tmp_path / "zarr1"), tmp_path)
