"""Every operator of the path against the oracle on the stretched grid (C12, nz 8, stretch 3 about (172.5, 17.5)): the first grid
without symmetries -- the six tiles differ and no tile is symmetric in itself -- so a kernel that read dx for a transposed dy or a
west-edge coefficient on the east cannot pass by accident.  Every case runs on the host emulation (CPU suite) and on the HIP library
(``-m gpu``).

The whole-cube cases and the operator cases are the uniform-grid tests themselves (tests/test_parity.py, test_operator_parity.py,
test_tracer_advection.py, test_remap.py, test_cubed_to_latlon.py, test_diag_kernels.py): their case builders are made to build
stretched grids (tests/stretched_case.py: ``stretched``) and their comparisons run unchanged, tolerances included.  The operator cases
run on all six tiles of the 1 x 1 layout (tile 5, refined, and tile 2, coarsened, among them) and on all 24 sub-domains of the 2 x 2
layout (every one of which holds a cube corner).

Analytic pins (tests/analytic_case.py).  The uniform-grid bounds do not carry over -- the coarse side of this grid is three times
coarser -- so each pin's bound is the oracle's own error on the same stretched grid, times two (the spread the existing pins allow
between the fp64 kernel and the oracle on reordered sums).  Measured on the host emulation (library / oracle): see DESIGN.md §8g.
"""
import numpy as np
import pytest
import torch

import analytic_case as ac
import helpers
import stretched_case as sc
import test_analytic_pins as pins
import test_cubed_to_latlon as t_c2l
import test_diag_kernels as t_diag
import test_operator_parity as t_op
import test_parity as t_par
import test_remap as t_remap
import test_tracer_advection as t_tr
from helpers import compare_cubes, run_device_cube
from pace_amd._testing import harness_for

N, NZ = sc.N, sc.NZ
DT = 225.0
LAYOUTS = [(1, 1), (2, 2)]


def _copy(states):
    return [{k: v.copy() for k, v in s.items()} for s in states]


# ---------------------------------------------------------------------------------------------------------------------------
# 1. whole cube, geometry only (stretched_grid off on both sides)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_full_acoustic_call_on_the_stretched_grid(backend, layout):
    part, cfg, grids, ost, phis, odyn = sc.oracle_cube(layout, NZ, dict(n_split=2))
    assert all(g.stretch == sc.STRETCH for g in grids) and not cfg.stretched_grid
    init = _copy(ost)
    odyn(ost, DT, 1)
    got, *_ = run_device_cube(backend, part, cfg, grids, init, phis, DT)
    worst = compare_cubes(got, ost, part, NZ, t_par.STATE, t_par.TOL)
    print("stretched full call", layout, {k: f"{v:.1e}" for k, v in worst.items()})


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the flag: dd8 = da_min d4_bg^(nord + 1)
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_flag_selects_the_stretched_divergence_damping(backend):
    """The oracle's only use of d4_bg is dd8 = (da_min_c d4_bg)^(nord + 1), so the library with the flag and d4_bg = b must equal the
    oracle with d4_bg' = (da_min b^(nord + 1))^(1 / (nord + 1)) / da_min_c."""
    b, nord = 0.15, 3
    g0 = sc.grids((1, 1))[1][0]
    b_eq = sc.equivalent_d4_bg(g0, b, nord)
    assert np.isclose((g0.da_min_c * b_eq) ** (nord + 1), g0.da_min * b ** (nord + 1), rtol=1e-13)
    part, ocfg, grids, ost, phis, odyn = sc.oracle_cube((1, 1), NZ, dict(n_split=2, nord=nord, d4_bg=b_eq))
    init = _copy(ost)
    cfg_on = sc.config((1, 1), NZ, n_split=2, nord=nord, d4_bg=b, stretched_grid=True)
    cfg_off = sc.config((1, 1), NZ, n_split=2, nord=nord, d4_bg=b)
    # first, on the CPU: the flag moves u / v by at least 100 x the comparison's tolerance -- otherwise the case shows nothing
    on, *_ = run_device_cube("hostemu", part, cfg_on, grids, init, phis, DT)
    off, *_ = run_device_cube("hostemu", part, cfg_off, grids, init, phis, DT)
    moved = 0.0
    for name in ("u", "v"):
        for r in range(part.total_ranks):
            sl = helpers.compute_slice(name, part.nx, part.ny, NZ)
            moved = max(moved, float(np.abs(on[r][name][sl] - off[r][name][sl]).max() / np.abs(off[r][name][sl]).max()))
    print(f"the flag moves u / v by {moved:.2e} of the field scale")
    assert moved >= 100.0 * max(t_par.TOL["u"], t_par.TOL["v"])
    odyn(ost, DT, 1)
    got = on if backend == "hostemu" else run_device_cube(backend, part, cfg_on, grids, init, phis, DT)[0]
    compare_cubes(got, ost, part, NZ, t_par.STATE, t_par.TOL)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. operators alone against the oracle
# ---------------------------------------------------------------------------------------------------------------------------
_RECORDED = {}


def _recorded(layout, nz=NZ):
    """tests/test_operator_parity.py: ``recorded`` on the stretched cube (its own cache is keyed without the grid, so it is not used)"""
    key = (tuple(layout), nz)
    if key not in _RECORDED:
        part, cfg, grids, ost, phis, odyn = sc.oracle_cube(layout, nz, dict(n_split=1))
        with t_op.Recorder() as rec:
            odyn(ost, DT, 1)
        _RECORDED[key] = (part, cfg, grids, rec.calls, odyn)
    return _RECORDED[key]


OPERATOR_CASES = ["test_update_dz_c", "test_riem_solver_c", "test_p_grad_c", "test_d_sw_on_recorded_inputs", "test_update_dz_d", "test_riem_solver3_on_recorded_inputs",
                  "test_pk3_halo_and_edge_pe", "test_nh_p_grad", "test_del2_cubed_and_diffusive_heating"]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", OPERATOR_CASES)
def test_operator_alone_on_recorded_inputs(backend, monkeypatch, case, layout):
    monkeypatch.setattr(t_op, "recorded", _recorded)
    assert all(g.stretch == sc.STRETCH for g in _recorded(layout)[2])
    getattr(t_op, case)(backend, layout)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_c_sw_alone_on_recorded_inputs(backend, layout):
    """c_sw(D, delp, pt, u, v, w, uc, vc, ua, va, ut, vt, divgd, omga, dt2) on the inputs the oracle's sequence hands to it: the C-grid
    winds, the A-grid winds, the contravariant winds, the divergence, and delpc / ptc / the advected w (the oracle returns the three)."""
    part, cfg, grids, calls, _ = _recorded(layout)
    cl = calls["c_sw"]
    dv = t_op.Dev(backend, grids, cfg)
    names = ("delp", "pt", "u", "v", "w", "uc", "vc", "ua", "va", "ut", "vt", "divgd", "omga")
    Q = {n: dv.q([c["ins"][i] for c in cl]) for i, n in enumerate(names)}
    delpc, ptc = dv.q([np.zeros_like(c["ins"][0]) for c in cl]), dv.q([np.zeros_like(c["ins"][0]) for c in cl])
    dt2 = float(cl[0]["ins"][13])
    # fv3_c_sw(delp, pt, u, v, w, uc, vc, ua, va, ut, vt, divgd, omga, delpc, ptc, dt2)
    dv.sf.call("c_sw", *[Q[n].fref for n in names], delpc.fref, ptc.fref, dt2)
    nz = dv.nz
    # regions and tolerance of tests/test_parity.py: test_c_sw
    for r, c in enumerate(cl):
        D = c["D"]
        C1 = D.sl(0, D.nx + 1, 0, D.ny + 1)
        outs = c["outs"]
        checks = [("delpc", delpc, c["ret"][0], C1), ("ptc", ptc, c["ret"][1], C1), ("omga", Q["omga"], outs[12], C1), ("divgd", Q["divgd"], outs[11], D.sl(1, D.nx + 1, 1, D.ny + 1)),
                  ("uc", Q["uc"], outs[5], D.sl(1, D.nx + 1, 1, D.ny)), ("vc", Q["vc"], outs[6], D.sl(1, D.nx, 1, D.ny + 1)),
                  ("ut", Q["ut"], outs[9], D.sl(0, D.nx + 2, 0, D.ny + 1)), ("vt", Q["vt"], outs[10], D.sl(0, D.nx + 1, 0, D.ny + 2)),
                  ("ua", Q["ua"], outs[7], C1), ("va", Q["va"], outs[8], C1)]
        for name, q, want, R in checks:
            got, wnt = q.numpy(r)[:, :, :nz][R].copy(), np.asarray(want)[:, :, :nz][R].copy()
            if name in ("delpc", "ptc", "omga"):  # the (never used) cube-corner halo cell of cell-centred outputs is excluded
                for (ci, cj), has in (((0, 0), D.sw), ((-1, 0), D.se), ((-1, -1), D.ne), ((0, -1), D.nw)):
                    if has:
                        got[ci, cj] = wnt[ci, cj] = 0.0
            helpers.assert_close(f"{name} rank {r}", got, wnt, 1e-12, 1e-12)


@pytest.mark.parametrize("n, layout, ranks", [(12, (1, 1), (sc.REFINED_TILE, sc.COARSE_TILE)), (12, (2, 2), (20, 21, 22, 23, 8, 11))])
def test_c_sw_fxadv_a2b_on_synthetic_inputs(backend, monkeypatch, n, layout, ranks):
    """tests/test_parity.py's c_sw, fxadv + fv_tp_2d and a2b_ord4 cases, on tiles 5 and 2 / on the four sub-domains of tile 5 and two of tile 2"""
    with sc.stretched():
        t_par.test_c_sw(backend, n, layout, ranks, None, monkeypatch)
        t_par.test_fxadv_and_fv_tp_2d(backend, n, layout, ranks)
        t_par.test_a2b_ord4(backend, n, layout, ranks)


@pytest.mark.parametrize("layout, want_split", [((1, 1), 1), ((2, 2), 2)])
def test_tracer_advection_on_the_stretched_grid(backend, layout, want_split):
    with sc.stretched():
        t_tr.test_tracer_advection_matches_the_oracle(backend, N, layout, want_split, 2, 8)


def test_remap_on_the_stretched_grid(backend):
    """(the remap is column work: one case)"""
    with sc.stretched():
        t_remap.test_remap_matches_the_oracle(backend, N, (2, 2), 1, 12)


@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_cubed_to_latlon_on_the_stretched_grid(backend, layout, order):
    """against tests/c2l_reference.py, which reads a11 .. a22 of the stretched grid: the rotation to east / north at every cell centre
    of a grid whose tiles are turned against the meridians in six different ways"""
    with sc.stretched(t_c2l):
        t_c2l.test_matches_numpy_restatement(backend, N, layout, order)


def test_column_integral_on_the_stretched_grid(backend, monkeypatch):
    """fv3_diag_column_integral forms RGRAV sum_k q delp per column; it applies no area weight itself (the caller of a global mean
    does), so the stretched grid enters through the context it runs in only."""
    monkeypatch.setattr(t_diag, "_case", t_diag._case.__wrapped__)  # (its cache is keyed without the grid)
    with sc.stretched():
        t_diag.test_column_integral(backend, 64, (N, (1, 2), 5, (10, 11, 4)))


# ---------------------------------------------------------------------------------------------------------------------------
# 4. analytic pins: the library's error against the oracle's on the same stretched grid
# ---------------------------------------------------------------------------------------------------------------------------
PIN_FACTOR = 2.0
PIN_NZ = 3


def _pin_case(backend, layout, cfg_kw=None, nz=PIN_NZ):
    part = sc.grids(layout)[0]
    with sc.stretched():
        return helpers.Case(N, layout, tuple(range(part.total_ranks)), nz=nz, backend=backend, cfg_kw=cfg_kw)


def _require(label, lib, oracle):
    print(f"{label}: library {lib:.4e}, oracle {oracle:.4e}")
    assert np.isfinite(lib) and lib <= PIN_FACTOR * oracle, f"{label}: library error {lib:.4e} above {PIN_FACTOR} x the oracle's {oracle:.4e}"


@pytest.mark.parametrize("layout", LAYOUTS)
def test_pin_solid_body_rotation_through_fxadv(backend, layout):
    cs = _pin_case(backend, layout)
    flow = ac.Flow(cs.c.RADIUS)
    dt = ac.flux_dt(3 * N, flow)  # Courant number about 0.5 on the refined side
    fc = ac.flux_case(cs.grids, flow, cs.nz)
    uc, vc = cs.q([pins._pad(x[1]) for x in fc]), cs.q([pins._pad(x[2]) for x in fc])
    out = {k: cs.q() for k in ("crx", "cry", "xfx", "yfx", "ut", "vt")}
    cs.sf.call("fxadv", uc.fref, vc.fref, *[out[k].fref for k in ("crx", "cry", "xfx", "yfx", "ut", "vt")], dt)
    pins._sync(backend)
    R = range(len(cs.grids))
    lib = ac.flux_errors(fc, flow, dt, [out["xfx"].numpy(r)[:, :, : cs.nz] for r in R], [out["yfx"].numpy(r)[:, :, : cs.nz] for r in R])
    xs, ys, _ = ac.oracle_fluxes(cs.doms, fc, dt)
    ora = ac.flux_errors(fc, flow, dt, xs, ys)
    _require(f"fxadv {layout} all faces", lib[0], ora[0])
    _require(f"fxadv {layout} tile-edge faces", lib[1], ora[1])


@pytest.mark.parametrize("layout", LAYOUTS)
def test_pin_d_to_c_winds_of_c_sw(backend, layout):
    cs = _pin_case(backend, layout, cfg_kw=dict(nord=0))
    flow = ac.Flow(cs.c.RADIUS)
    wc = ac.wind_case(cs.grids, flow, cs.nz)
    DIMS3 = helpers.DIMS3
    Q = {"delp": cs.qf.ones(DIMS3), "pt": cs.qf.ones(DIMS3), "u": cs.q([pins._pad(x[1]) for x in wc]), "v": cs.q([pins._pad(x[2]) for x in wc])}
    Q.update({k: cs.q() for k in ("w", "uc", "vc", "ua", "va", "ut", "vt", "divgd", "omga", "delpc", "ptc")})
    cs.sf.call("c_sw", *[Q[k].fref for k in ("delp", "pt", "u", "v", "w", "uc", "vc", "ua", "va", "ut", "vt", "divgd", "omga", "delpc", "ptc")], 0.0)
    pins._sync(backend)
    R = range(len(cs.grids))
    lib = ac.wind_errors(wc, flow, [Q["uc"].numpy(r)[:, :, : cs.nz] for r in R], [Q["vc"].numpy(r)[:, :, : cs.nz] for r in R])
    ora = ac.wind_errors(wc, flow, *ac.oracle_winds(cs.doms, wc))
    _require(f"d2a2c {layout} all faces", lib[0], ora[0])
    _require(f"d2a2c {layout} tile-edge faces", lib[1], ora[1])


@pytest.mark.parametrize("layout", LAYOUTS)
def test_pin_a2b_ord4(backend, layout):
    cs = _pin_case(backend, layout)
    cc = ac.corner_case(cs.grids, cs.nz)
    Q, O = cs.q([pins._pad(x[1]) for x in cc]), cs.q()
    cs.sf.call("a2b_ord4", Q.fref, O.fref, 0, cs.nz, 0)
    pins._sync(backend)
    lib = ac.corner_errors(cc, [O.numpy(r)[:, :, : cs.nz] for r in range(len(cs.grids))])
    ora = ac.corner_errors(cc, ac.oracle_corners(cs.doms, cc))
    for k in ("interior", "edge", "corner", "all"):
        _require(f"a2b_ord4 {layout} {k}", lib[k], ora[k])


@pytest.mark.parametrize("which", ["d", "c"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_pin_atmosphere_at_rest(backend, layout, which):
    """nh_p_grad ("d") / p_grad_c ("c") on the isentropic atmosphere at rest over the 3 km mountain: the wind the force leaves
    against the oracle's, the largest over the cube each; and, as on the uniform grid, within 1e-9 of the control state's."""
    cs = _pin_case(backend, layout, nz=ac.PGF_NZ)
    rest, sts = pins.library_pgf(cs, backend, True, which)
    control, _ = pins.library_pgf(cs, backend, False, which)
    lib = ora = 0.0
    for r, (g, D) in enumerate(zip(cs.grids, cs.doms)):
        G = ac.Geometry(g)
        if which == "d":
            o = ac.force(G, *ac.oracle_pgf(D, cs.c, sts[r]), cs.nz)
        else:
            ouc, ovc = ac.oracle_pgf_c(D, sts[r])
            o = ac.force(G, ovc, ouc, cs.nz)
        lib, ora = max(lib, rest[r]), max(ora, o)
    # (the control over the whole cube: the mountain lies on the coarse side, and the sub-domains of the refined side see flat ground)
    ac.check_no_force(f"{which} {layout}", lib, max(control))
    _require(f"atmosphere at rest, {'nh_p_grad' if which == 'd' else 'p_grad_c'} {layout}", lib, ora)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. step_dynamics: 1 x 1 against 2 x 2
# ---------------------------------------------------------------------------------------------------------------------------
STEP = dict(nz=NZ, dt_atmos=DT, k_split=2, n_split=2, n_tracers=2, hord_tr=8, remap=True, temperature=True, init="baroclinic")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def test_step_dynamics_does_not_depend_on_the_decomposition(backend):
    """tests/test_step_dynamics.py's case on the stretched grid (harness keywords: stretched grids and the flag): every state field but
    the uc / vc workspace, the tracers and ps, bit for bit"""
    from test_step_dynamics import C_GRID_WORKSPACE, _snapshot

    runs = {}
    for layout in LAYOUTS:
        h = harness_for(backend)(N, layout=layout, **sc.STRETCH.as_dict(), **STEP)
        assert h.cfg.stretched_grid
        h.step()
        h.synchronize()
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
            assert np.all(np.isfinite(a))
            assert np.array_equal(_bits(a), _bits(want)), (name, r, float(np.abs(a - want).max()))
    assert 100.0 < min(x.min() for x in one["pt"]) and max(x.max() for x in one["pt"]) < 380.0
    h1.close()
    h4.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 6. one fp32 case of (1)
# ---------------------------------------------------------------------------------------------------------------------------
FP32_TOL = {"delp": 2e-5, "pt": 2e-5, "u": 2e-4, "v": 2e-4}  # tests/test_gpu_invariants.py: test_fp32_build_tracks_fp64


def test_fp32_full_acoustic_call_on_the_stretched_grid(backend):
    """The fp32 library against the fp64 oracle, the stated fp32 tolerance of the uniform grid (field-relative: 2e-5 for delp / pt, 2e-4
    for u / v).  nord = 1: with the flag off the default del-8 table (da_min_c d4_bg)^4 leaves the float range on C12 and the context
    refuses it (tests/test_stretched_grid.py)."""
    from pace_amd import build

    if backend == "hostemu":
        build.build(32, hostemu=True, verbose=False)
    part, cfg, grids, ost, phis, odyn = sc.oracle_cube((1, 1), NZ, dict(n_split=2, nord=1), noise=0.0)
    init = _copy(ost)
    odyn(ost, DT, 1)
    got, *_ = run_device_cube(backend, part, cfg, grids, init, phis, DT, dtype=torch.float32)
    worst = compare_cubes(got, ost, part, NZ, tuple(FP32_TOL), {**FP32_TOL, "default": 0.0})
    print("stretched fp32 full call", {k: f"{v:.1e}" for k, v in worst.items()})
