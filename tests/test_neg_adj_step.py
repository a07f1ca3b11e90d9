"""neg_adj3 inside the step: DycoreHarness(neg_adj=True) / DynamicalCore(adjust_negative_water=True) against the same step with the
operator called by hand, the decomposition, and the driver's --neg-adj.  The step cases run on the host emulation (CPU suite) and on
the HIP library (-m gpu)."""
import json
import os

import numpy as np
import pytest

import test_moist_step as tm
from pace_amd import driver
from pace_amd._testing import harness_for
from pace_amd.harness import WATER_NAMES
from pace_amd.stencils import AdjustNegativeTracerMixingRatio

N, NZ = 12, 8
CASE = dict(nz=NZ, layout=(1, 1), dt_atmos=225.0, k_split=2, n_split=2, n_tracers=7, hord_tr=8, remap=True, temperature=True, moist=True, latlon_winds=True)
_bits, _snapshot, _assert_same = tm._bits, tm._snapshot, tm._assert_same


def _plant(h, seed=3):
    """negative values in one cell in forty of every water species, and one column in forty negative from top to bottom -- which the
    vertical filling cannot mend, the species having nothing to give there (the same cells in every harness built alike)"""
    rng = np.random.default_rng(seed)
    for role in WATER_NAMES:
        q = h.tracers[role]
        for r in range(len(h.grids)):
            a = q.numpy(r).copy()
            m = (rng.random(a.shape) < 0.025) | (rng.random(a.shape[:2]) < 0.025)[:, :, None]
            a[m] = -np.abs(a[m]) * 0.3 - 1.0e-9
            q.set_numpy(a, r)


def _negatives(h):
    return sum(int((tm._compute(h.tracers[role], r)[..., : h.cfg.npz] < 0).sum()) for role in WATER_NAMES for r in range(len(h.grids)))


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. sequencing: the step with neg_adj is the step without it followed by the operator, bit for bit (CubedToLatLon, which runs after
#    the operator inside the step and before it here, reads neither pt nor the species)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("init", ["synthetic", "restart"])
@pytest.mark.parametrize("fill", [False, True], ids=["nofill", "fill"])
def test_step_with_neg_adj_is_the_step_followed_by_the_operator_bitwise(backend, fill, init):
    kw, nz = dict(CASE, fill=fill), NZ
    if init == "restart":  # (all 63 levels with the file's own ak / bk: the state is not a balanced one on fewer)
        data = np.load(tm.FIXTURE)
        nz = data["T"].shape[1]
        kw.update(nz=nz, init="restart", init_data=data, ak=data["ak"], bk=data["bk"])
    A = harness_for(backend)(N, neg_adj=True, **kw)
    B = harness_for(backend)(N, **kw)
    assert A.neg_adj and A.dycore.adjust_negative_water is not None and B.dycore.adjust_negative_water is None
    if init == "synthetic":
        _plant(A)
        _plant(B)
    op = AdjustNegativeTracerMixingRatio(B.sf)
    tr = B.tracers
    worked = 0
    for step in range(2):
        A.step()
        B.step()
        B.synchronize()
        worked += _negatives(B)
        op(tr["qvapor"], tr["qliquid"], tr["qrain"], tr["qsnow"], tr["qice"], tr["qgraupel"], None, B.state.pt, B.state.delp, B.state.delz, B.state.peln)
        A.synchronize()
        B.synchronize()
        snap = _snapshot(A, A.dycore.ps)
        _assert_same(snap, _snapshot(B, B.ps), f"step {step}")
        for role in WATER_NAMES[1:]:
            assert all((x[..., :nz] >= 0).all() for x in snap[role]), role
        t = np.concatenate([x[..., :nz].ravel() for x in snap["pt"]])
        assert np.isfinite(t).all() and 100.0 < t.min() and t.max() < 380.0
    assert worked > 0  # the operator had negative values to fix
    A.close()
    B.close()


def test_the_neg_adj_clock_is_timed(backend):
    from pace_amd.timer import Timer

    h = harness_for(backend)(N, neg_adj=True, **CASE)
    timer = Timer()
    h.step(timer)
    h.synchronize()
    assert timer.hits["NegAdj3"] == 1 and timer.hits["CubedToLatLon"] == 1
    h.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. decomposition: one sub-domain per tile against four
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_step_with_neg_adj_does_not_depend_on_the_decomposition(backend):
    n, nz = 24, 7
    runs = {}
    for layout in ((1, 1), (2, 2)):
        h = harness_for(backend)(n, neg_adj=True, fill=True, init="baroclinic", **{**CASE, "nz": nz, "layout": layout, "n_tracers": 6})
        # the moist baroclinic wave has vapour only: every condensate species is a share of it minus a constant (the same arithmetic in
        # every cell), negative where the air is dry
        for share, role in zip((0.02, 0.004, 0.01, 0.003, 0.002), tm.CONDENSATE):
            h.tracers[role].storage.copy_(h.tracers["qvapor"].storage * share - 4.0e-3 * share)
        h.synchronize()
        assert _negatives(h) > 0
        h.step()
        h.synchronize()
        runs[layout] = (h, _snapshot(h, h.dycore.ps))
    h1, one = runs[(1, 1)]
    h4, four = runs[(2, 2)]
    for r in range(len(h4.grids)):
        tile, (ox, oy) = h4.part.tile_index(r), h4.part.origin(r)
        for name in ("pt",) + tuple(WATER_NAMES):
            a = four[name][r]
            want = one[name][tile][ox : ox + a.shape[0], oy : oy + a.shape[1]]
            assert np.array_equal(_bits(a), _bits(want)), (name, r, float(np.abs(a - want).max()))
    for role in tm.CONDENSATE:
        assert all((x[..., :nz] >= 0).all() for x in one[role]), role
    assert 100.0 < min(x[..., :nz].min() for x in one["pt"]) and max(x[..., :nz].max() for x in one["pt"]) < 380.0
    h1.close()
    h4.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. driver
# ---------------------------------------------------------------------------------------------------------------------------------
def test_driver_neg_adj_without_moist_is_refused_in_one_sentence(tmp_path):
    for extra in ([], ["--temperature", "--remap"]):
        with pytest.raises(SystemExit) as e:
            driver.main([tm._yaml(tmp_path), "--neg-adj"] + extra)
        msg = str(e.value)
        assert "--neg-adj needs --moist" in msg and msg.count(". ") == 0, msg


@pytest.mark.gpu
def test_driver_neg_adj_run(tmp_path, gpu_backend, capsys):
    out = tmp_path / "perf.json"
    p = tm._yaml(tmp_path)
    common = [p, "--steps", "2", "--out", str(out), "--moist", "--temperature", "--remap", "--fill", "on"]
    assert driver.main(common + ["--neg-adj"]) == 0
    said = capsys.readouterr().out
    assert '"neg_adj": true' in said
    d = json.load(open(out))
    assert d["setup"]["neg_adj"] is True and d["setup"]["finite"] and d["setup"]["thermodynamics"] == "moist_cv"
    assert "neg_adj3 is left out" not in d["setup"]["note"] and "NegAdj3" in d["times"]
    assert driver.main(common) == 0
    said = capsys.readouterr().out
    assert '"neg_adj": false' in said
    d = json.load(open(out))
    assert d["setup"]["neg_adj"] is False and d["setup"]["finite"] and "neg_adj3 is left out" in d["setup"]["note"] and "NegAdj3" not in d["times"]
