"""DiagnosticsConfig / ZSelect / MonitorDiagnostics construction (CPU): the checks of the reference's
tests/main/driver/test_diagnostics_config.py restated for this build, plus the ones this build adds (strict names, level range)."""
import os
import warnings

import pytest

from pace_amd.diagnostics import DiagnosticsConfig, MonitorDiagnostics, NullDiagnostics, ZSelect, diagnostics_factory


@pytest.fixture(scope="module")
def harness(hostemu):
    from pace_amd._testing import hostemu_harness

    return hostemu_harness(12, nz=4, layout=(1, 1), n_tracers=1)


def test_returns_null_diagnostics_if_no_path_given(harness):
    config = DiagnosticsConfig(path=None, names=[], derived_names=[])
    assert isinstance(config.diagnostics_factory(harness), NullDiagnostics)
    assert isinstance(diagnostics_factory(harness), NullDiagnostics)
    assert isinstance(DiagnosticsConfig.from_dict(None).diagnostics_factory(harness), NullDiagnostics)


@pytest.mark.parametrize("output_format", ["zarr", "netcdf"])
def test_returns_monitor_diagnostics_if_path_given(harness, tmp_path, output_format):
    config = DiagnosticsConfig(path=str(tmp_path / "out"), output_format=output_format, names=["u"], derived_names=[])
    d = config.diagnostics_factory(harness)
    assert isinstance(d, MonitorDiagnostics) and d.variables == ["u"]
    assert os.path.isdir(tmp_path / "out")


def test_raises_if_names_given_but_no_path():
    with pytest.raises(ValueError, match="path must be given"):
        DiagnosticsConfig(path=None, names=["foo"], derived_names=[])


def test_raises_if_derived_names_given_but_no_path():
    with pytest.raises(ValueError, match="path must be given"):
        DiagnosticsConfig(path=None, names=[], derived_names=["foo"])


def test_raises_on_another_output_format(tmp_path):
    with pytest.raises(ValueError, match="'zarr' or 'netcdf'"):
        DiagnosticsConfig(path=str(tmp_path), output_format="hdf5")


def test_from_dict_takes_the_yaml_block(tmp_path):
    c = DiagnosticsConfig.from_dict({"path": str(tmp_path), "output_format": "netcdf", "time_chunk_size": 3, "names": ["u", "pt"], "derived_names": ["column_integrated_tracer0"],
                                     "z_select": [{"level": 2, "names": ["pt"]}]})
    assert c.output_format == "netcdf" and c.time_chunk_size == 3 and c.names == ["u", "pt"]
    assert c.z_select == [ZSelect(level=2, names=["pt"])]
    with pytest.raises(ValueError, match="unknown keys"):
        DiagnosticsConfig.from_dict({"path": str(tmp_path), "nmaes": ["u"]})


def test_zselect_raises_on_a_2d_field(harness, tmp_path):
    config = DiagnosticsConfig(path=str(tmp_path), names=[], z_select=[ZSelect(level=0, names=["phis"])])
    with pytest.raises(AssertionError):
        config.diagnostics_factory(harness)


def test_zselect_raises_when_the_third_dim_is_not_z(harness, tmp_path):
    from pace_amd.monitor import ZarrMonitor
    from pace_amd.quantity import Quantity

    odd = Quantity(harness.state.pt.storage, ("z", "x", "y"), "K")
    with pytest.raises(ValueError, match="dimension \\(x, y, z\\)"):
        MonitorDiagnostics(ZarrMonitor(str(tmp_path), harness.layout), [], [], [ZSelect(level=0, names=["odd"])], state=harness.state, tracers={"odd": odd},
                           stencil_factory=harness.sf)
    with pytest.raises(ValueError, match="dimension \\(x, y, z\\)"):  # an interface field: its third dim is z_interface
        DiagnosticsConfig(path=str(tmp_path), z_select=[ZSelect(level=0, names=["pe"])]).diagnostics_factory(harness)


@pytest.mark.parametrize("level", [-1, 4, 5])
def test_zselect_raises_on_a_level_outside_the_field(harness, tmp_path, level):
    """(deviation from the reference, whose raw slice would return the pad level for level == nz)"""
    config = DiagnosticsConfig(path=str(tmp_path), z_select=[ZSelect(level=level, names=["pt"])])
    with pytest.raises(ValueError, match="outside \\[0, 4\\)"):
        config.diagnostics_factory(harness)


def test_unknown_name_lists_the_known_ones(harness, tmp_path):
    config = DiagnosticsConfig(path=str(tmp_path), names=["u", "qvapor"])
    with pytest.raises(ValueError, match="qvapor") as e:
        config.diagnostics_factory(harness)
    for known in ("delp", "phis", "tracer0"):
        assert known in str(e.value)
    with pytest.raises(ValueError, match="qrain"):
        DiagnosticsConfig(path=str(tmp_path), derived_names=["column_integrated_qrain"]).diagnostics_factory(harness)


def test_unknown_derived_name_warns_and_writes_nothing(harness, tmp_path):
    config = DiagnosticsConfig(path=str(tmp_path / "z"), names=["phis"], derived_names=["total_precipitation"])
    with pytest.warns(UserWarning, match="total_precipitation is not a supported diagnostic variable"):
        d = config.diagnostics_factory(harness)
    assert d.variables == ["phis"]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        d.store(0.0)
        d.cleanup()
    assert sorted(n for n in os.listdir(tmp_path / "z") if not n.startswith(".")) == ["phis", "time"]


def test_buffers_are_allocated_once_for_the_largest_variable(harness, tmp_path):
    config = DiagnosticsConfig(path=str(tmp_path), names=["phis", "v", "pe"], derived_names=["column_integrated_tracer0"], z_select=[ZSelect(level=1, names=["pt"])])
    d = config.diagnostics_factory(harness)
    assert d.variables == ["phis", "v", "pe", "column_integrated_tracer0", "pt_z1"]
    assert d._dev.numel() == d._host.numel() == 6 * 5 * 12 * 12  # pe: nz + 1 levels (v has 6 * 4 * 12 * 13: smaller)
    dev, host = d._dev.data_ptr(), d._host.data_ptr()
    d.store(0.0)
    d.store(1.0)
    assert (d._dev.data_ptr(), d._host.data_ptr()) == (dev, host)
