"""Reference savepoint FVDynamics-Out ua / va: the eastward / northward winds CubedToLatLon leaves at the end of fv_dynamics
[REF tests/savepoint/thresholds/fv_dynamics.yaml; thresholds in tests/golden/reference_thresholds_fv_dynamics.json].

Consumer of the files tools/gen_golden.py records where pyFV3 imports (all six ranks, ``mpirun -n 6``): FVDynamics-In -> one step of the
harness with ``latlon_winds`` -> ua, va against FVDynamics-Out with the reference's own thresholds.  None exists in this tree, so the
test skips like the other savepoint consumers."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(__file__))
import savepoint_checkers as sc  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "golden_c12")


def check_latlon_winds(path, backend, nx=12):
    from pace_amd._testing import harness_for
    from pace_amd.dyn_core import STATE_NAMES

    ranks = sc.ranks_present(path, "FVDynamics-In")
    inp = [sc.load(path, "FVDynamics-In", r) for r in ranks]
    out = [sc.load(path, "FVDynamics-Out", r) for r in ranks]
    nz = inp[0]["u"].shape[2] - 1
    m = sc.meta(path).get("config", {})
    tnames = sorted(k for k in inp[0] if k.startswith("tracer_"))
    over = {k: m[k] for k in ("hord_dp", "hord_mt", "hord_tm", "hord_vt", "nord", "d4_bg", "d2_bg", "d2_bg_k1", "d2_bg_k2", "d_con", "dddmp", "vtdm4", "ke_bg", "p_fac", "rf_fast",
                              "rf_cutoff", "tau", "delt_max", "do_vort_damp", "n_sponge", "c2l_ord") if k in m}
    h = harness_for(backend)(nx, nz=nz, layout=(1, 1), dt_atmos=float(m.get("dt_atmos", 225.0)), k_split=int(m.get("k_split", 1)), n_split=int(m.get("n_split", 1)),
                             config_overrides=over, n_tracers=len(tnames), hord_tr=int(m.get("hord_tr", 8)), remap=True, latlon_winds=True)
    nzp = nz + 1
    for i in ranks:
        for n in STATE_NAMES + ["phis"]:
            getattr(h.state, n).set_numpy(sc._pad3(inp[i].get(n, inp[i].get("state_" + n)), nzp), i)
        for t, n in enumerate(tnames):
            h.tracers[f"tracer{t}"].set_numpy(sc._pad3(inp[i][n], nzp), i)
    h.step()
    h.synchronize()
    errs = {}
    sl = sc._sl(nx, nx, nz, sc.CELL)
    for i in ranks:
        for var in ("ua", "va"):
            errs[var] = max(errs.get(var, 0.0), sc.excess("FVDynamics-Out", var, getattr(h.state, var).numpy(i)[sl], sc._pad3(out[i][var], nzp)[sl]))
    return errs


def test_latlon_winds_against_reference_savepoints(hostemu):
    if sc.ranks_present(GOLDEN, "FVDynamics-In") != list(range(6)):
        pytest.skip("reference parity unpinned: tests/golden/golden_c12/FVDynamics-In_call0_rank*.npz is absent for all six ranks (generate it with "
                    "tools/gen_golden.py where pyFV3 imports, mpirun -n 6)")
    errs = check_latlon_winds(GOLDEN, "hostemu")
    bad = {k: v for k, v in errs.items() if not v <= 1.0}
    assert not bad, f"ua / va leave the reference's thresholds (excess factors): {errs}"

