"""The saturation adjustment inside the step: fv3_remap_moist_sat (pace_amd/csrc/fv3_remap.hip) against fv3_remap_moist followed by fv3_sat_adj,
DynamicalCore(saturation_adjustment=True) / DycoreHarness(sat_adj=True) against the same operators called by hand, the decomposition, the
neutrality of the default and moist paths and the driver's --sat-adj.  The operator and step cases run on the host emulation (CPU suite) and
on the HIP library (-m gpu).  The remap inputs are those of tests/test_moist_step.py (BeforeRemap: genuinely Lagrangian levels with planted
negative condensate), which the adjustment meets below and above saturation."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

import zarr_v2_read as zr
from pace_amd import driver
from pace_amd._testing import harness_for
from pace_amd.fv_dynamics import DynamicalCore
from pace_amd.harness import WATER_NAMES
from pace_amd.stencils import LagrangianToEulerian, SatAdjustConfig, SaturationAdjustment
from test_moist_step import CASE, CONDENSATE, N, NZ, BeforeRemap, _assert_same, _bits, _snapshot
from test_thermo import real  # noqa: F401  (the (backend, dtype) fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MDT = 112.5
OWNED = ("pt", "pkz", "q_con", "cappa") + tuple(WATER_NAMES)  # what the adjustment may change of a moist remap's result


def _remap_three_ways(B, fill, last_step):
    """(fused, by hand, the plain moist remap) on the saved inputs of B"""
    h = B.h
    s, d = h.state, h.dycore
    op = SaturationAdjustment(h.sf)
    kmp, nz = op.level0, B.nz
    args = (d.tracers, s.pt, s.delp, s.delz, s.peln, s.pe, s.pk, s.pkz, s.u, s.v, s.w, s.cappa, d.ps, d.acoustic_dynamics._wsd)
    B.restore()
    LagrangianToEulerian(h.sf, fill=fill)(*args, q_con=s.q_con, water=d.water, sat_adjust=op, mdt=MDT, last_step=last_step)
    h.synchronize()
    fused = _snapshot(h, d.ps)
    B.restore()
    LagrangianToEulerian(h.sf, fill=fill)(*args, q_con=s.q_con, water=d.water)
    h.synchronize()
    moist = _snapshot(h, d.ps)
    tv = h.sf.quantity_factory.zeros(("x", "y", "z"))
    tv.storage.copy_(s.pt.storage * s.pkz.storage)
    op(d.water, tv, s.delp, s.delz, s.q_con, s.cappa, s.pkz, MDT, last_step=last_step)
    s.pt.storage[:, kmp:nz] = tv.storage[:, kmp:nz] / s.pkz.storage[:, kmp:nz]  # (storage is [sub-domain, k, j, i]; above kmp pt stays the remap's)
    h.synchronize()
    return fused, _snapshot(h, d.ps), moist, kmp


@pytest.mark.parametrize("last_step", [False, True], ids=["mid", "last"])
@pytest.mark.parametrize("nz, fill", [(8, False), (8, True), (79, True)], ids=["l8_nofill", "l8_fill", "l79_fill"])
def test_fused_remap_is_the_moist_remap_followed_by_the_adjustment(real, nz, fill, last_step):  # noqa: F811
    backend, dtype = real
    B = BeforeRemap(backend, 12, (1, 1), nz, dtype=dtype)
    fused, by_hand, moist, kmp = _remap_three_ways(B, fill, last_step)
    assert (kmp > 0) == (nz == 79)
    _assert_same(fused, by_hand, f"fused against by hand, L{nz} fill={fill} last_step={last_step}")
    # everything the adjustment does not own is the moist remap's, bit for bit; what it owns has moved
    _assert_same(fused, moist, "fused against the moist remap", skip=OWNED)
    assert "tracer6" in fused and "u" in fused and "ps" in fused
    for n in OWNED:
        same = all(np.array_equal(_bits(a[..., :kmp]), _bits(b[..., :kmp])) for a, b in zip(fused[n], moist[n]))
        assert same, (n, "changed above kmp")
    moved = [n for n in OWNED if any(not np.array_equal(_bits(a), _bits(b)) for a, b in zip(fused[n], moist[n]))]
    assert {"pt", "pkz", "cappa", "qvapor"} <= set(moved), moved
    for n in OWNED:
        assert all(np.isfinite(a[..., :nz]).all() for a in fused[n]), n
    B.h.close()


def _supersaturate(h):
    """the moist baroclinic wave has vapour only, below saturation: three times the vapour and a share of it in every condensate species"""
    h.tracers["qvapor"].storage.mul_(3.0)
    for share, role in zip((0.02, 0.004, 0.01, 0.003, 0.002), CONDENSATE):
        h.tracers[role].storage.copy_(h.tracers["qvapor"].storage * share)


def test_step_dynamics_is_its_operators_called_by_hand(backend):
    kw = dict(init="baroclinic", fill=True, **{**CASE, "n_tracers": 6})
    assert kw["k_split"] == 2
    A = harness_for(backend)(N, moist=True, sat_adj=True, **kw)
    Bh = harness_for(backend)(N, moist=True, **kw)
    assert A.dycore.saturation_adjustment is not None and Bh.dycore.saturation_adjustment is None
    for h in (A, Bh):
        _supersaturate(h)
    A.step()
    A.synchronize()
    s, d = Bh.state, Bh.dycore
    op = SaturationAdjustment(Bh.sf)
    d.temperature_to_potential(s.pt, s.pkz, s.delp, s.delz, s.q_con, s.cappa, d.qvapor, water=d.water)
    for k, last in enumerate((False, True)):  # the first remap of the step is not the last one, the second is
        d.dp1.storage.copy_(s.delp.storage)
        d.acoustic_dynamics(s, 225.0 / 2, n_map=k + 1)
        d._tracer_halo.update()
        d.tracer_advection(d.tracers, d.dp1, s.mfxd, s.mfyd, s.cxd, s.cyd)
        d.remap(d.tracers, s.pt, s.delp, s.delz, s.peln, s.pe, s.pk, s.pkz, s.u, s.v, s.w, s.cappa, d.ps, d.acoustic_dynamics._wsd, q_con=s.q_con, water=d.water,
                sat_adjust=op, mdt=225.0 / 2, last_step=last)
    d.potential_to_temperature(s.pt, s.pkz, s.delp, s.delz, s.q_con, s.cappa, s.w, s.pe, qvapor=d.qvapor, omga=s.omga, ps=d.ps, recompute_pkz=False)
    Bh.synchronize()
    a, b = _snapshot(A, A.dycore.ps), _snapshot(Bh, d.ps)
    _assert_same(a, b, "step_dynamics against its operators")
    # the adjustment had work: cloud water where there was a fixed share of the vapour before, a finite temperature
    assert max(float(x[..., :NZ].max()) for x in a["qliquid"]) > 1.0e-4
    t = np.concatenate([x[..., :NZ].ravel() for x in a["pt"]])
    assert np.isfinite(t).all() and 100.0 < t.min() and t.max() < 400.0
    # the other order of the two flags is another result: last_step reaches the kernel
    C_ = harness_for(backend)(N, moist=True, **kw)
    _supersaturate(C_)
    s, d = C_.state, C_.dycore
    d.temperature_to_potential(s.pt, s.pkz, s.delp, s.delz, s.q_con, s.cappa, d.qvapor, water=d.water)
    d.dp1.storage.copy_(s.delp.storage)
    d.acoustic_dynamics(s, 225.0 / 2, n_map=1)
    d._tracer_halo.update()
    d.tracer_advection(d.tracers, d.dp1, s.mfxd, s.mfyd, s.cxd, s.cyd)
    saved = {n: q.storage.clone() for n, q in d.tracers.items()}
    for n, q in (("pt", s.pt), ("delp", s.delp), ("delz", s.delz), ("pe", s.pe), ("peln", s.peln), ("pk", s.pk), ("pkz", s.pkz), ("u", s.u), ("v", s.v), ("w", s.w), ("cappa", s.cappa)):
        saved[n] = q.storage.clone()
    out = []
    for last in (False, True):
        for n, q in list(d.tracers.items()) + [("pt", s.pt), ("delp", s.delp), ("delz", s.delz), ("pe", s.pe), ("peln", s.peln), ("pk", s.pk), ("pkz", s.pkz), ("u", s.u), ("v", s.v), ("w", s.w), ("cappa", s.cappa)]:
            q.storage.copy_(saved[n])
        d.remap(d.tracers, s.pt, s.delp, s.delz, s.peln, s.pe, s.pk, s.pkz, s.u, s.v, s.w, s.cappa, d.ps, d.acoustic_dynamics._wsd, q_con=s.q_con, water=d.water, sat_adjust=op, mdt=225.0 / 2,
                last_step=last)
        C_.synchronize()
        out.append(d.tracers["qvapor"].storage.clone())
    assert not torch.equal(out[0], out[1])
    for h in (A, Bh, C_):
        h.close()


def test_dynamical_core_needs_all_six_roles_for_the_adjustment(backend):
    h = harness_for(backend)(12, nz=5, layout=(1, 1), k_split=1, n_split=1, n_tracers=6, remap=True, temperature=True, moist=True)
    roles = {n: n for n in h.tracers}
    mk = lambda **kw: DynamicalCore(h.layout, h.grids, h.sf, None, None, h.cfg, 225.0, h.state.phis, h.state, tracers=h.tracers, cubed_to_latlon=False, **kw)  # noqa: E731
    with pytest.raises(ValueError, match="saturation_adjustment=True needs water_species with all six roles.*qsnow"):
        mk(water_species={k: v for k, v in roles.items() if k != "qsnow"}, saturation_adjustment=True)
    with pytest.raises(ValueError, match="all six roles"):
        mk(saturation_adjustment=True)
    core = mk(water_species=roles, saturation_adjustment=True, sat_adjust_config=SatAdjustConfig(tau_v2l=90.0))
    assert core.saturation_adjustment.config.tau_v2l == 90.0 and core.saturation_adjustment.params.tau_v2l == 90.0 and core.saturation_adjustment.params.tau_l2v == 300.0
    assert mk(water_species=roles).saturation_adjustment is None and h.dycore.saturation_adjustment is None
    with pytest.raises(ValueError, match="sat_adj=True needs moist=True"):
        harness_for(backend)(12, nz=5, layout=(1, 1), n_tracers=6, remap=True, temperature=True, sat_adj=True)
    rm = LagrangianToEulerian(h.sf)
    s, d = h.state, h.dycore
    args = (d.tracers, s.pt, s.delp, s.delz, s.peln, s.pe, s.pk, s.pkz, s.u, s.v, s.w, s.cappa, d.ps, d.acoustic_dynamics._wsd)
    with pytest.raises(ValueError, match="sat_adjust needs water"):
        rm(*args, sat_adjust=core.saturation_adjustment, mdt=MDT)
    with pytest.raises(ValueError, match="sat_adjust needs mdt"):
        rm(*args, q_con=s.q_con, water=d.water, sat_adjust=core.saturation_adjustment)
    with pytest.raises(TypeError):
        rm(*args, s.q_con, d.water, core.saturation_adjustment)  # (keyword-only)
    h.close()


def test_the_adjusting_step_does_not_depend_on_the_decomposition(backend):
    n = 24
    runs = {}
    for layout in ((1, 1), (2, 2)):
        h = harness_for(backend)(n, moist=True, sat_adj=True, fill=True, init="baroclinic", **{**CASE, "layout": layout, "n_tracers": 6})
        _supersaturate(h)
        h.step()
        h.synchronize()
        runs[layout] = (h, _snapshot(h, h.dycore.ps))
    h1, one = runs[(1, 1)]
    h4, four = runs[(2, 2)]
    for r in range(len(h4.grids)):
        tile, (ox, oy) = h4.part.tile_index(r), h4.part.origin(r)
        for name in OWNED:
            a = four[name][r]
            want = one[name][tile][ox : ox + a.shape[0], oy : oy + a.shape[1]]
            assert np.array_equal(_bits(a), _bits(want)), (name, r, float(np.abs(a - want).max()))
    assert max(float(x[..., :NZ].max()) for x in one["qliquid"]) > 1.0e-4
    h1.close()
    h4.close()


# the default or the moist step in a process of its own, where no adjusting object has ever existed
FRESH_PROCESS = """
import sys
import numpy as np
from pace_amd._testing import harness_for
from pace_amd.dyn_core import STATE_NAMES
backend, path, n, kw = sys.argv[1], sys.argv[2], int(sys.argv[3]), eval(sys.argv[4])
h = harness_for(backend)(n, **kw)
h.step()
h.synchronize()
fields = {k: getattr(h.state, k) for k in STATE_NAMES}
fields.update(h.tracers)
fields["ps"] = h.dycore.ps
np.savez(path, **{f"{k}:{r}": q.sub(r).view[...].detach().cpu().numpy() for k, q in fields.items() for r in range(len(h.grids))})
h.close()
"""


def test_default_and_moist_paths_are_bitwise_what_they_were_after_an_adjusting_object_was_built(backend, tmp_path):
    base = dict(fill=True, **{**CASE, "n_tracers": 6})
    modes = dict(default=dict(vapor="tracer0", **base), moist=dict(moist=True, **base))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT] + [p for p in os.environ.get("PYTHONPATH", "").split(os.pathsep) if p]))
    fresh = {}
    for mode, kw in modes.items():
        path = str(tmp_path / f"{mode}.npz")
        subprocess.run([sys.executable, "-c", FRESH_PROCESS, backend, path, str(N), repr(kw)], check=True, env=env, cwd=ROOT)
        fresh[mode] = np.load(path)

    def run(kw):
        h = harness_for(backend)(N, **kw)
        assert h.dycore.saturation_adjustment is None
        h.step()
        h.synchronize()
        out = _snapshot(h, h.dycore.ps)
        h.close()
        return out

    m = harness_for(backend)(N, moist=True, sat_adj=True, **base)
    m.step()
    m.synchronize()
    m.close()
    for mode, kw in modes.items():
        got = run(kw)
        want = {k: [fresh[mode][f"{k}:{r}"] for r in range(len(v))] for k, v in got.items()}
        _assert_same(want, got, f"{mode} path against a process without an adjusting object")


# ---------------------------------------------------------------------------------------------------------------------------------
# driver
# ---------------------------------------------------------------------------------------------------------------------------------
def _yaml(tmp_path, name="c.yaml", store=None, source="c48_moist_sat_adj.yaml", **dycore):
    """an example yaml cut to C12 with two sub-steps, with a diagnostics block that lists the six species where asked"""
    y = yaml.safe_load(open(os.path.join(ROOT, "examples", source)))
    y.update(nx_tile=12, seconds=450)
    y["dycore_config"].update(n_split=2, **dycore)
    y["performance_config"] = {"experiment_name": "c12_sat_adj"}
    if store is not None:
        y["output_frequency"] = 1
        y["diagnostics_config"] = {"path": str(store), "output_format": "zarr", "names": ["pt", "delp", "q_con", "cappa"] + list(WATER_NAMES)}
    p = tmp_path / name
    p.write_text(yaml.safe_dump(y))
    return str(p)


def test_the_example_is_the_dycore_only_example_plus_the_adjustment_keys():
    a = yaml.safe_load(open(os.path.join(ROOT, "examples", "c48_dycore_only.yaml")))
    b = yaml.safe_load(open(os.path.join(ROOT, "examples", "c48_moist_sat_adj.yaml")))
    extra = {k: v for k, v in b["dycore_config"].items() if k not in a["dycore_config"]}
    assert {k: v for k, v in b.items() if k != "dycore_config"} == {k: v for k, v in a.items() if k != "dycore_config"}
    assert {k: b["dycore_config"][k] for k in a["dycore_config"]} == a["dycore_config"]
    assert extra.pop("do_sat_adj") is True and extra and set(extra) <= set(driver.SAT_ADJ_KEYS)
    run, dy, ignored = driver.load_config(os.path.join(ROOT, "examples", "c48_moist_sat_adj.yaml"))
    assert sorted(ignored) == sorted(["nwat", "do_sat_adj"] + list(extra))  # (the list the driver prints without --moist)
    assert driver.resolve_sat_adj("yaml", run["sat_adj"], True) and not driver.resolve_sat_adj("yaml", run["sat_adj"], False)
    assert not driver.resolve_sat_adj("off", run["sat_adj"], True) and driver.resolve_sat_adj("on", {}, True) and not driver.resolve_sat_adj("yaml", {}, True)


def test_driver_sat_adj_refusals_are_one_sentence(tmp_path):
    for argv, word in (([_yaml(tmp_path), "--sat-adj", "on", "--remap"], "--sat-adj on needs --moist"),
                       ([_yaml(tmp_path), "--sat-adj", "on", "--tracers", "6", "--remap", "--temperature"], "--sat-adj on needs --moist")):
        with pytest.raises(SystemExit) as e:
            driver.main(argv)
        msg = str(e.value)
        assert word in msg and msg.count(". ") == 0, msg
    with pytest.raises(SystemExit):
        driver.main([_yaml(tmp_path), "--sat-adj", "maybe"])


@pytest.mark.gpu
def test_driver_sat_adj_run_and_restart_round_trip(tmp_path, gpu_backend, capsys, monkeypatch):
    import pace_amd.init as pinit

    plain = pinit.baroclinic_humidity
    monkeypatch.setattr(pinit, "baroclinic_humidity", lambda lat, delp, peln: 3.0 * plain(lat, delp, peln))  # supersaturated in the lower troposphere
    store, out = tmp_path / "store", tmp_path / "perf.json"
    p = _yaml(tmp_path, store=store, do_sat_adj=False)  # (the key says off: --sat-adj on overrides it)
    common = ["--moist", "--temperature", "--remap", "--fill", "on"]
    r1 = str(tmp_path / "restart_1")
    assert driver.main([p, "--steps", "1", "--out", str(out), "--save-restart", r1, "--sat-adj", "on"] + common) == 0
    said = capsys.readouterr().out
    assert '"sat_adj": true (--sat-adj on)' in said and "keys not read" not in said
    d = json.load(open(out))
    assert d["setup"]["sat_adj"] is True and d["setup"]["finite"] and d["setup"]["thermodynamics"] == "moist_cv"
    assert "no saturation adjustment" not in d["times_note"] and "fv_sat_adj inside every remap" in d["times_note"] and "the saturation adjustment (" not in d["setup"]["note"]
    assert set(d["times"]) == {"mainloop", "DynCore", "TracerAdvection", "Remapping"}  # (the adjustment's time stays under "Remapping")
    ql, t = zr.read(str(store), "qliquid")[-1], zr.read(str(store), "pt")[-1]
    assert ql.max() > 0 and np.isfinite(t).all() and 100.0 < t.min() and t.max() < 400.0
    # the yaml's own key, two steps in one run against one step, a restart, one more step: the same files, bit for bit
    p2 = _yaml(tmp_path, "nodiag.yaml")
    two, again = str(tmp_path / "restart_2"), str(tmp_path / "restart_1_1")
    assert driver.main([p2, "--steps", "2", "--out", str(out), "--save-restart", two] + common) == 0
    said = capsys.readouterr().out
    assert '"sat_adj": true' in said and "(--sat-adj" not in said and "keys not read" not in said
    first = str(tmp_path / "restart_y1")
    assert driver.main([p2, "--steps", "1", "--out", str(out), "--save-restart", first] + common) == 0
    assert driver.main([p2, "--steps", "1", "--out", str(out), "--restart", first, "--save-restart", again] + common) == 0
    from scipy.io import netcdf_file

    def same_files(a_dir, b_dir, expect_equal=True):
        equal = True
        for rank in range(6):
            with netcdf_file(os.path.join(a_dir, f"restart_dycore_state_{rank}.nc"), "r", mmap=False) as a, netcdf_file(os.path.join(b_dir, f"restart_dycore_state_{rank}.nc"), "r", mmap=False) as b:
                assert set(WATER_NAMES) <= set(a.variables) and set(a.variables) == set(b.variables)
                for name in a.variables:
                    x, y = np.array(a.variables[name][:]), np.array(b.variables[name][:])
                    if x.dtype.kind != "f":
                        continue
                    if expect_equal:
                        assert np.array_equal(x, y, equal_nan=True), (rank, name)
                    equal = equal and np.array_equal(x, y, equal_nan=True)
        return equal

    same_files(two, again)
    # --sat-adj off reproduces the moist run (the dycore-only example, which has no do_sat_adj) bit for bit, and says so
    off, moist = str(tmp_path / "restart_off"), str(tmp_path / "restart_moist")
    assert driver.main([p2, "--steps", "1", "--out", str(out), "--save-restart", off, "--sat-adj", "off"] + common) == 0
    said = capsys.readouterr().out
    assert '"sat_adj": false (--sat-adj off)' in said
    d = json.load(open(out))
    assert d["setup"]["sat_adj"] is False and "no saturation adjustment" in d["times_note"]
    assert driver.main([_yaml(tmp_path, "moist.yaml", source="c48_dycore_only.yaml"), "--steps", "1", "--out", str(out), "--save-restart", moist] + common) == 0
    same_files(off, moist)
    assert not same_files(first, moist, expect_equal=False)  # (the adjusting run is another run)
    # without --moist the keys stay on the list of keys nobody read
    assert driver.main([p2, "--steps", "1", "--tracers", "2", "--remap", "--temperature", "--out", str(out)]) == 0
    said = capsys.readouterr().out
    assert '"sat_adj": false' in said and "keys not read by the acoustic path: do_sat_adj, nwat, qi_lim" in said
