"""The stretched cubed sphere (Schmidt transform of the corner positions): geometry against closed forms that do not go through the
implementation's lat / lon algebra, the global area minima, the halo metric against the neighbour's interior, the config / ABI flag
and the driver's ``grid_config`` block.  CPU only (the kernels on this grid: tests/test_stretched_parity.py)."""
import json
import os

import numpy as np
import pytest
import torch

import halo_reference as hr
import stretched_case as sc
from pace_amd import driver, restart
from pace_amd._testing import hostemu_factory, hostemu_harness
from pace_amd.config import AcousticDynamicsConfig
from pace_amd.constants import get_constants
from pace_amd.grid import _GRID_2D, SchmidtTransform, _corner_positions, damping_coefficients, global_area_minima, great_circle_dist, make_grid
from pace_amd.topology import CubedSpherePartitioner

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLE = os.path.join(ROOT, "examples", "c48_stretched.yaml")
NH = 3


# ---------------------------------------------------------------------------------------------------------------------------
# 1. opt-in: no stretch, or a factor of 1, is today's grid bit for bit
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [12, 24])
@pytest.mark.parametrize("layout", [(1, 1), (2, 2)])
def test_factor_one_is_the_uniform_grid_bitwise(n, layout):
    part = CubedSpherePartitioner(n, layout)
    for r in range(part.total_ranks):
        base = make_grid(part, r, nz=4)
        for stretch in (None, SchmidtTransform(), SchmidtTransform(1.0, 172.5, 17.5)):
            g = make_grid(part, r, nz=4, stretch=stretch)
            assert g.stretch is None
            for name in _GRID_2D:
                assert np.array_equal(g.fields[name], base.fields[name]), name
            for name in ("edge_w", "edge_e", "edge_s", "edge_n", "corner_extrap"):
                assert np.array_equal(getattr(g, name), getattr(base, name)), name
            assert g.da_min == base.da_min and g.da_min_c == base.da_min_c
    c = get_constants()
    assert global_area_minima(n, c, stretch=SchmidtTransform()) == global_area_minima(n, c)
    d = damping_coefficients(base, stretch=SchmidtTransform())
    assert d.da_min == base.da_min and d.da_min_c == base.da_min_c
    with pytest.raises(ValueError, match="stretch"):
        damping_coefficients(base, stretch=sc.STRETCH)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. closed form: c tan(theta' / 2) = tan(theta / 2), theta from the south pole before, theta' from the target after
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stretch", [sc.STRETCH, sc.STRETCH_B], ids=["c3_172.5_17.5", "c1.5_10_-40"])
def test_every_corner_obeys_the_schmidt_relation(stretch):
    """Distances are angles between unit vectors (atan2 of cross and dot product); nothing here forms a latitude or a longitude of a
    grid point.  The relation has no relative scale at its two fixed points -- the south pole (tan = 0: the centre corner of tile 5
    at even N) and its antipode (tan = infinity: the centre corner of tile 2) -- so it is checked as c tan(theta' / 2) = tan(theta / 2)
    on the southern hemisphere and as cot(theta' / 2) = c cot(theta / 2) on the northern one, each to 1e-12 of its value with an
    absolute floor of 1e-12 (rad / 2) for the fixed point itself."""
    n, c = 12, stretch.stretch_factor
    part = CubedSpherePartitioner(n, (1, 1))
    south, target = np.array([0.0, 0.0, -1.0]), sc.target_vector(stretch)
    for tile in range(6):
        for nh in (0, NH):  # the tile's own corners; with the edge halos and the cube-corner fill blocks
            before = _corner_positions(part, tile, nh)
            after = _corner_positions(part, tile, nh, stretch)
            th = great_circle_dist(before, south)
            th2 = great_circle_dist(after, target)
            lo = th <= 0.5 * np.pi
            a, b = c * np.tan(0.5 * th2[lo]), np.tan(0.5 * th[lo])
            assert np.all(np.abs(a - b) <= 1e-12 * b + 1e-12), (tile, nh, np.abs(a - b).max())
            a, b = 1.0 / np.tan(0.5 * th2[~lo]), c / np.tan(0.5 * th[~lo])
            assert np.all(np.abs(a - b) <= 1e-12 * b + 1e-12), (tile, nh, np.abs(a - b).max())
    # the four corners around the centre of tile 5 average to the target (and at even N the centre corner is the target)
    P = _corner_positions(part, sc.REFINED_TILE, 0, stretch)
    m = n // 2
    mean = P[m - 1, m - 1] + P[m + 1, m - 1] + P[m + 1, m + 1] + P[m - 1, m + 1]
    assert great_circle_dist(mean / np.linalg.norm(mean), target) <= 1e-12
    assert great_circle_dist(P[m, m], target) <= 1e-12
    # refinement by c at the centre of tile 5: the centre cell's edge against the uniform grid's
    P0 = _corner_positions(part, sc.REFINED_TILE, 0)
    ratio = great_circle_dist(P0[m, m], P0[m + 1, m]) / great_circle_dist(P[m, m], P[m + 1, m])
    assert abs(ratio / c - 1.0) < 0.02, ratio


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the cells and the dual cells tile the sphere
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stretch", [sc.STRETCH, sc.STRETCH_B], ids=["c3", "c1.5"])
def test_areas_of_the_six_tiles_tile_the_sphere(stretch):
    c = get_constants()
    n = sc.N
    part, gs = sc.grids((1, 1), stretch=stretch)
    sphere = 4 * np.pi * c.RADIUS**2
    assert abs(sum(g.area[NH : NH + n, NH : NH + n].sum() for g in gs) / sphere - 1) < 1e-12
    w = np.ones((n + 1, n + 1))  # a tile-edge corner belongs to two tiles, a cube corner to three
    w[0, :] = w[-1, :] = w[:, 0] = w[:, -1] = 0.5
    w[0, 0] = w[0, -1] = w[-1, 0] = w[-1, -1] = 1 / 3
    assert abs(sum((g.area_c[NH : NH + n + 1, NH : NH + n + 1] * w).sum() for g in gs) / sphere - 1) < 1e-12
    assert len({round(float(g.area[NH : NH + n, NH : NH + n].sum()), 3) for g in gs}) > 2  # (the tiles are not congruent)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. decomposition independence
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [(2, 2), (3, 3)])
def test_metric_terms_do_not_depend_on_the_decomposition(layout):
    """every metric field of every rank against the matching window of the 1 x 1 tile, compute domain (cells, with the north / east
    line for the staggered ones), as tests/test_grid.py does on the uniform grid"""
    _, whole = sc.grids((1, 1))
    part, gs = sc.grids(layout)
    m = part.nx
    for r, g in enumerate(gs):
        g1 = whole[part.tile_index(r)]
        x0, y0 = part.origin(r)
        for name in _GRID_2D:
            a = g.fields[name][NH : NH + m + 1, NH : NH + m + 1]
            b = g1.fields[name][NH + x0 : NH + x0 + m + 1, NH + y0 : NH + y0 + m + 1]
            if name in ("a11", "a12", "a21", "a22", "lon_agrid", "lat_agrid", "f0", "area", "rarea", "dxa", "dya", "rdxa", "rdya", "cosa_s", "rsin2", "sin_sg5") or name[:6] in ("sin_sg", "cos_sg"):
                a, b = a[:m, :m], b[:m, :m]  # cell-centred
            elif name in ("dx", "rdx", "dyc", "rdyc", "cosa_v", "sina_v", "rsin_v", "divg_u", "del6_u"):
                a, b = a[:m, :], b[:m, :]  # y interfaces
            elif name in ("dy", "rdy", "dxc", "rdxc", "cosa_u", "sina_u", "rsin_u", "divg_v", "del6_v"):
                a, b = a[:, :m], b[:, :m]  # x interfaces
            scale = np.abs(b).max()
            assert np.allclose(a, b, rtol=1e-12, atol=1e-13 * scale), (name, r, np.abs(a - b).max() / scale)
        assert g.da_min == g1.da_min and g.da_min_c == g1.da_min_c


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the global minima
# ---------------------------------------------------------------------------------------------------------------------------
def test_area_minima_are_global_and_the_same_on_every_rank():
    n = sc.N
    c = get_constants()
    uniform = global_area_minima(n, c)
    seen = set()
    brute = {}
    for layout in ((1, 1), (2, 2), (3, 3)):
        part, gs = sc.grids(layout)
        m = part.nx
        brute[layout] = (min(float(g.area[NH : NH + m, NH : NH + m].min()) for g in gs), min(float(g.area_c[NH : NH + m + 1, NH : NH + m + 1].min()) for g in gs))
        seen |= {(g.da_min, g.da_min_c) for g in gs}
    assert len(seen) == 1
    da_min, da_min_c = seen.pop()
    for layout, (a, ac) in brute.items():
        assert np.isclose(da_min, a, rtol=1e-12, atol=0) and np.isclose(da_min_c, ac, rtol=1e-12, atol=0), layout
    assert (da_min, da_min_c) == global_area_minima(n, c, stretch=sc.STRETCH)
    # refined by 3 at the target: the smallest cell is several times smaller than the uniform grid's corner cell
    assert da_min < 0.5 * uniform[0] and da_min_c < 0.5 * uniform[1]
    # and it sits on the refined tile, not where the uniform grid has it
    _, gs = sc.grids((1, 1))
    assert min(range(6), key=lambda t: gs[t].area[NH : NH + n, NH : NH + n].min()) == sc.REFINED_TILE


# ---------------------------------------------------------------------------------------------------------------------------
# 6. the halo metric is the neighbour's interior
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [(1, 1), (2, 2)])
def test_halo_metric_is_the_neighbours_interior(layout):
    """dx (on the y interfaces: the D-grid's u points), dy (x interfaces: v points) and area (cells) in every rank's edge halo against
    the whole tiles' interior values at the source points tests/halo_reference.py derives from positions on the (unstretched) sphere;
    across a rotated edge the source of a dx is a dy."""
    n = sc.N
    _, whole = sc.grids((1, 1))
    part, gs = sc.grids(layout)
    G = {"dgrid": [[g.dx[NH : NH + n, NH : NH + n + 1] for g in whole], [g.dy[NH : NH + n + 1, NH : NH + n] for g in whole]],
         "cell": [[g.area[NH : NH + n, NH : NH + n] for g in whole]]}
    swapped = checked = 0
    for r, g in enumerate(gs):
        for kind, fields in (("dgrid", (g.dx, g.dy)), ("cell", (g.area,))):
            for (comp, i, j), src in hr.halo_sources(n, layout, r, kind, NH).items():
                if src is None:
                    continue
                t, c2, gi, gj, _sign = src
                want = G[kind][c2][t][gi, gj]
                assert abs(fields[comp][i, j] / want - 1.0) <= 1e-11, (r, kind, comp, i, j)
                swapped += int(c2 != comp)
                checked += 1
    assert swapped > 0 and checked > swapped
    # the check can fail: on this grid dx and dy of a halo point differ by far more than the tolerance
    g = gs[0]
    assert np.abs(g.dx[:NH, NH : NH + part.ny] / g.dy[:NH, NH : NH + part.ny] - 1.0).max() > 1e-3


# ---------------------------------------------------------------------------------------------------------------------------
# 7. config and ABI
# ---------------------------------------------------------------------------------------------------------------------------
def test_validate_accepts_stretched_and_refuses_nested():
    assert AcousticDynamicsConfig(stretched_grid=True).validate().stretched_grid
    with pytest.raises(NotImplementedError, match="nested"):
        AcousticDynamicsConfig(nested=True).validate()
    with pytest.raises(NotImplementedError, match="nested"):
        AcousticDynamicsConfig(nested=True, stretched_grid=True).validate()


def test_fp32_context_takes_the_stretched_damping_form(hostemu):
    """C12, nord = 3, fp32: the congruent form (da_min_c d4_bg)^4 leaves the float range and its context is refused (tests/test_abi.py);
    the stretched form da_min d4_bg^4 is a number of ordinary size and the context is created."""
    from pace_amd import build, lib

    build.build(32, hostemu=True, verbose=False)
    _, gs = sc.grids((1, 1), nz=4)
    g = gs[0]
    fmax = float(np.finfo(np.float32).max)
    assert (g.da_min_c * 0.15) ** 4 > fmax
    assert 1.0 < g.da_min * 0.15**4 < 1e-20 * fmax
    with pytest.raises(lib.Fv3Error, match="overflows"):
        hostemu_factory(list(gs), sc.config((1, 1), nz=4, nord=3, d4_bg=0.15), dtype=torch.float32)
    sf = hostemu_factory(list(gs), sc.config((1, 1), nz=4, nord=3, d4_bg=0.15, stretched_grid=True), dtype=torch.float32)
    assert sf.ctx and sf.config.stretched_grid
    sf.close()


def test_operators_check_their_stretched_grid_keyword(hostemu):
    from pace_amd.dyn_core import AcousticDynamics
    from pace_amd.halo import Layout
    from pace_amd.stencils import DGridShallowWaterLagrangianDynamics

    part, gs = sc.grids((1, 1), nz=4)
    for flag in (False, True):
        cfg = sc.config((1, 1), nz=4, stretched_grid=flag)
        sf = hostemu_factory(list(gs), cfg)
        DGridShallowWaterLagrangianDynamics(sf, stretched_grid=flag)
        DGridShallowWaterLagrangianDynamics(sf)
        AcousticDynamics(Layout(part, 1, 0), list(gs), sf, stretched_grid=flag)
        with pytest.raises(ValueError, match="stretched_grid"):
            DGridShallowWaterLagrangianDynamics(sf, stretched_grid=not flag)
        with pytest.raises(ValueError, match="stretched_grid"):
            AcousticDynamics(Layout(part, 1, 0), list(gs), sf, stretched_grid=not flag)
        sf.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 8. driver, harness, restart
# ---------------------------------------------------------------------------------------------------------------------------
UNIFORM_YAML = """
dycore_only: true
disable_step_physics: true
initialization:
  type: analytic
  config:
    case: baroclinic
nx_tile: 12
nz: 8
dt_atmos: 225
seconds: 450
layout: [1, 1]
dycore_config:
  k_split: 1
  n_split: 2
"""
GRID_BLOCK = """
grid_config:
  type: generated
  config:
    stretch_factor: 3.0
    lon_target: 172.5
    lat_target: 17.5
    ks: 0
"""
WANT = {"stretch_factor": 3.0, "lon_target": 172.5, "lat_target": 17.5}


class _Stop(Exception):
    pass


def test_example_yaml_reaches_the_harness(monkeypatch, hostemu):
    run, dy, _ = driver.load_config(EXAMPLE)
    assert run["grid"] == WANT and run["nx_tile"] == 48 and driver.grid_entry(run["grid"]) == WANT
    seen = {}

    def stub(*a, **kw):
        seen.update(kw)
        raise _Stop

    with monkeypatch.context() as mp:
        mp.setattr("pace_amd.harness.DycoreHarness", stub)
        with pytest.raises(_Stop):
            driver.main([EXAMPLE, "--steps", "1"])
    assert {k: seen[k] for k in WANT} == WANT
    # the same keywords on a small harness: stretched grids and the flag
    h = hostemu_harness(12, nz=4, **driver.harness_grid_kwargs(run["grid"]))
    assert h.cfg.stretched_grid and h.stretch == sc.STRETCH and all(g.stretch == sc.STRETCH for g in h.grids)
    assert h.grids[0].da_min == sc.grids((1, 1))[1][0].da_min
    h.close()
    h = hostemu_harness(12, nz=4)
    assert not h.cfg.stretched_grid and h.stretch is None and h.grids[0].stretch is None
    h.close()


def test_yaml_without_grid_config_is_uniform_and_other_grids_are_refused(tmp_path, monkeypatch):
    p = tmp_path / "u.yaml"
    p.write_text(UNIFORM_YAML)
    run, _, _ = driver.load_config(str(p))
    assert driver.grid_entry(run["grid"]) == "uniform" and driver.harness_grid_kwargs(run["grid"]) == {}
    seen = {}

    def stub(*a, **kw):
        seen.update(kw)
        raise _Stop

    monkeypatch.setattr("pace_amd.harness.DycoreHarness", stub)
    with pytest.raises(_Stop):
        driver.main([str(p), "--steps", "1"])
    assert not any(k in seen for k in WANT)
    p.write_text(UNIFORM_YAML + GRID_BLOCK)
    assert driver.grid_entry(driver.load_config(str(p))[0]["grid"]) == WANT
    p.write_text(UNIFORM_YAML + GRID_BLOCK + "    grid_type: 4\n")
    with pytest.raises(ValueError, match="grid_type"):
        driver.load_config(str(p))
    with pytest.raises(SystemExit, match="grid_type"):
        driver.main([str(p)])
    p.write_text(UNIFORM_YAML + "grid_config:\n  type: external\n  config:\n    grid_file_path: x\n")
    with pytest.raises(ValueError, match="external"):
        driver.load_config(str(p))


def test_restart_files_carry_the_grid_and_do_not_mix(tmp_path, hostemu):
    hs = hostemu_harness(12, nz=4, stretch_factor=3.0, lon_target=172.5, lat_target=17.5)
    hu = hostemu_harness(12, nz=4)
    ds, du = str(tmp_path / "s"), str(tmp_path / "u")
    restart.save_state(hs.state, hs.layout.local_ranks, ds, stretch=hs.stretch)
    restart.save_state(hu.state, hu.layout.local_ranks, du, stretch=hu.stretch)
    ref = str(tmp_path / "ref")
    restart.save_state(hu.state, hu.layout.local_ranks, ref)
    for r in hu.layout.local_ranks:  # files of uniform runs stay byte for byte what they are
        assert open(os.path.join(du, f"restart_dycore_state_{r}.nc"), "rb").read() == open(os.path.join(ref, f"restart_dycore_state_{r}.nc"), "rb").read()
    assert restart.grid_of(ds, 0) == sc.STRETCH.key and restart.grid_of(du, 0) is None
    restart.check_grid(hs.layout.local_ranks, ds, hs.stretch)
    restart.check_grid(hu.layout.local_ranks, du, None)
    with pytest.raises(ValueError, match="stretched by 3"):
        restart.check_grid(hu.layout.local_ranks, ds, hu.stretch)
    with pytest.raises(ValueError, match="uniform grid"):
        restart.check_grid(hs.layout.local_ranks, du, hs.stretch)
    with pytest.raises(ValueError, match="stretched by 3"):
        restart.check_grid(hs.layout.local_ranks, ds, sc.STRETCH_B)
    hs.close(), hu.close()


@pytest.mark.gpu
def test_driver_runs_stretched_and_its_restart_is_refused_by_a_uniform_run(tmp_path, gpu_backend):
    ps, pu = tmp_path / "s.yaml", tmp_path / "u.yaml"
    ps.write_text(UNIFORM_YAML + GRID_BLOCK)
    pu.write_text(UNIFORM_YAML)
    out, rs, ru = tmp_path / "s.json", str(tmp_path / "rs"), str(tmp_path / "ru")
    assert driver.main([str(ps), "--steps", "2", "--out", str(out), "--save-restart", rs]) == 0
    d = json.load(open(out))
    assert d["setup"]["grid"] == WANT and d["setup"]["finite"]
    assert driver.main([str(pu), "--steps", "1", "--out", str(out), "--save-restart", ru]) == 0
    assert json.load(open(out))["setup"]["grid"] == "uniform"
    with pytest.raises(SystemExit, match="--restart: .*stretched by 3"):
        driver.main([str(pu), "--steps", "1", "--out", str(out), "--restart", rs])
    with pytest.raises(SystemExit, match="--restart: .*uniform grid"):
        driver.main([str(ps), "--steps", "1", "--out", str(out), "--restart", ru])
    assert driver.main([str(ps), "--steps", "1", "--out", str(out), "--restart", rs]) == 0
