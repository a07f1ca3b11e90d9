"""The vertical filling of negative tracer values inside the step (DycoreHarness(..., remap=True, fill=True): fv3_fillz right after
fv3_remap) and in the driver (``dycore_config.fill`` / ``--fill``).  The step cases run on the host emulation (CPU suite) and on the
HIP library (-m gpu)."""
import functools
import json

import numpy as np
import pytest

from fillz_reference import fillz as ref_fillz
from pace_amd import driver
from pace_amd._testing import harness_for

NH = 3
N = 12
STATE = "delp pt u v w delz pe peln pk pkz".split()


def _two_blocks(nz):
    """tracer0 of the step case, compute cells (i, j, k), all 0-based: the indicator A (1 <= i <= 6, 2 <= j <= 9) on the even levels,
    B (4 <= i <= 10, 1 <= j <= 7) on the odd ones, each times 1 + 0.1 k, exact zero elsewhere.  The blocks overlap, so the undershoots the unlimited
    scheme leaves around one level's block sit in columns that hold mass on the neighbouring level."""
    i, j = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    A = ((i >= 1) & (i <= 6) & (j >= 2) & (j <= 9)).astype(np.float64)
    B = ((i >= 4) & (i <= 10) & (j >= 1) & (j <= 7)).astype(np.float64)
    q = np.zeros((N + 2 * NH + 1, N + 2 * NH + 1, nz + 1))
    for k in range(nz):
        q[NH : NH + N, NH : NH + N, k] = (A if k % 2 == 0 else B) * (1.0 + 0.1 * k)
    return q


@functools.lru_cache(maxsize=None)
def _undershoot_pair(backend):
    """One step of the C12 L6 case with hord_tr = 5, filling off and on: host copies of the tracer and the state."""
    nz = 6
    out = {}
    for fill in (False, True):
        h = harness_for(backend)(N, nz=nz, layout=(1, 1), dt_atmos=450.0, k_split=1, n_split=3, n_tracers=1, hord_tr=5, remap=True, fill=fill)
        for r in range(len(h.grids)):
            h.tracers["tracer0"].set_numpy(_two_blocks(nz), r)
        h.step()
        h.synchronize()
        out[fill] = {n: [getattr(h.state, n).numpy(r) for r in range(6)] for n in STATE}
        out[fill]["tracer0"] = [h.tracers["tracer0"].numpy(r) for r in range(6)]
        h.close()
    return out


def test_step_with_fill_is_the_restatement_on_the_unfilled_step(backend):
    """fill=True changes the tracer -- to what the numpy restatement makes of the fill=False tracer and delp, bit for bit -- and
    nothing else.  Measured on the host emulation with fill=False: 1271 negative cells after the step, 321 columns flagged (zfix),
    142 of them with the non-local fix; the restatement changes 1231 values."""
    nz = 6
    run = _undershoot_pair(backend)
    cs = (slice(NH, NH + N), slice(NH, NH + N), slice(0, nz))
    n_neg = n_zfix = n_nl = n_changed = 0
    for r in range(6):
        q0 = run[False]["tracer0"][r]
        want_cells, br = ref_fillz(q0[cs].reshape(N * N, nz), run[False]["delp"][r][cs].reshape(N * N, nz))
        want = q0.copy()
        want[cs] = want_cells.reshape(N, N, nz)
        assert np.array_equal(run[True]["tracer0"][r].view(np.uint64), want.view(np.uint64)), (r, np.abs(run[True]["tracer0"][r] - want).max())
        n_neg += int((q0[cs] < 0).sum())
        n_zfix += int(br["zfix"].sum())
        n_nl += int(br["nonlocal"].sum())
        n_changed += int((want != q0).sum())
        for n in STATE:
            assert np.array_equal(run[True][n][r].view(np.uint64), run[False][n][r].view(np.uint64)), (n, r)
    print(f"fillz step {backend}: {n_neg} negative cells without filling, {n_zfix} flagged columns, {n_nl} non-local fixes, {n_changed} values changed")
    # (guards of the test, not of the kernel: the input must reach the code)
    assert n_zfix >= 1 and n_nl >= 1 and n_changed >= 1


def test_fill_is_the_identity_on_positive_tracers(backend):
    """Two steps of k_split = 2 with the harness's own positive tracers and the monotone scheme: nothing is negative, so tracers and
    state are bitwise equal with the filling on and off -- the existing configurations cannot have changed."""
    runs = {}
    for fill in (False, True):
        h = harness_for(backend)(N, nz=6, layout=(1, 1), dt_atmos=450.0, k_split=2, n_split=3, n_tracers=2, hord_tr=8, remap=True, fill=fill)
        assert (h.cfg.fill, h.remap.fill, h.remap._fillz is not None) == (fill, fill, fill)
        for _ in range(2):
            h.step()
        h.synchronize()
        runs[fill] = {n: [getattr(h.state, n).numpy(r) for r in range(6)] for n in STATE}
        for t in ("tracer0", "tracer1"):
            runs[fill][t] = [h.tracers[t].numpy(r) for r in range(6)]
        h.close()
    cs = (slice(NH, NH + N), slice(NH, NH + N), slice(0, 6))
    for n in STATE + ["tracer0", "tracer1"]:
        for r in range(6):
            assert np.array_equal(runs[True][n][r].view(np.uint64), runs[False][n][r].view(np.uint64)), (n, r)
    assert all((runs[False][t][r][cs] > 0).all() for t in ("tracer0", "tracer1") for r in range(6))


def test_fill_without_remap_is_refused(backend):
    with pytest.raises(ValueError, match="remap"):
        harness_for(backend)(N, nz=6, layout=(1, 1), dt_atmos=450.0, k_split=1, n_split=3, n_tracers=1, remap=False, fill=True)


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
  experiment_name: c12_fill
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


def test_driver_reads_fill_from_the_yaml_and_the_option(tmp_path):
    with_key, without = tmp_path / "fill.yaml", tmp_path / "nofill.yaml"
    with_key.write_text(YAML + "  fill: true\n")
    without.write_text(YAML)
    _, dy, ignored = driver.load_config(str(with_key))
    assert dy["fill"] is True and "fill" not in ignored
    _, dy0, _ = driver.load_config(str(without))
    assert "fill" not in dy0
    # the yaml decides when --tracers N --remap are both given ...
    assert driver.resolve_fill("yaml", dy, 2, True) is True
    assert driver.resolve_fill("yaml", dy0, 2, True) is False  # (absent: FV3's namelist default)
    # ... --fill overrides it ...
    assert driver.resolve_fill("off", dy, 2, True) is False
    assert driver.resolve_fill("on", dy0, 2, True) is True
    # ... and without the remap or without tracers there is nothing to fill
    for opt in ("yaml", "on"):
        assert driver.resolve_fill(opt, dy, 2, False) is False
        assert driver.resolve_fill(opt, dy, 0, True) is False
    with pytest.raises(ValueError):
        driver.resolve_fill("maybe", dy, 2, True)
    with pytest.raises(SystemExit):
        driver.main([str(with_key), "--fill", "maybe"])
    from pace_amd.config import AcousticDynamicsConfig

    assert AcousticDynamicsConfig().fill is False and AcousticDynamicsConfig.from_dict({"fill": True}).fill is True


@pytest.mark.gpu
def test_driver_run_with_fill_says_so(tmp_path, capsys):
    p = tmp_path / "fill.yaml"
    p.write_text(YAML + "  fill: true\n")
    out = tmp_path / "perf.json"
    assert driver.main([str(p), "--steps", "2", "--tracers", "2", "--remap", "--out", str(out)]) == 0
    d = json.load(open(out))
    assert d["setup"]["fill"] is True and d["setup"]["remap"] and d["setup"]["tracers"] == 2 and d["setup"]["finite"]
    assert '"fill": true' in capsys.readouterr().out
