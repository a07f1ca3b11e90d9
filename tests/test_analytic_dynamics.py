"""d_sw, update_dz_d and the Riemann solvers against closed-form solutions (builders, exact solutions and checkers: tests/analytic_case.py), continuing
tests/test_analytic_pins.py under the same ground rule: inputs and expected values come from corner positions, cell centres, the sphere radius and
closed-form functions of position; no metric term a kernel reads enters an expected value (edge lengths are great-circle distances of the corners; the
Courant number times the upwind area is the stated exception).  Nothing below needs the oracle at run time.

The flow is solid-body rotation about the oblique axis, every damping term of d_sw off (nord 0, d2_bg = d2_bg_k1 = d2_bg_k2 = d4_bg = dddmp = d_con = vtdm4 =
ke_bg = 0, do_vort_damp False) and n_sponge = -1, which the context accepts: all three levels are compared.  dt = 0.1 (24 / n) 0.7 a (pi / 2) / n / U0,
Courant number 0.1 at C24 and falling as 1 / n, so that one call's error measures the scheme and not the time step.

  6   d_sw          delp, pt, w, q_con == their initial function at the departure point of the cell centre; mfx / mfy += delp at the half-step departure
                    point of the face mid-point x the exact swept area; cx / cy += swept area over the upwind cell's; heat_source = diss_est = 0
  7   d_sw          (u_out / L - u_in) / dt == the projection of -(zeta + f) k x V - grad K on the face's edge, by class of faces (below)
  8   riem_solver3, riem_solver_c   a dry column at delz_eq = -(delp / g) R pt pm^(kappa - 1), pm = delp / delta ln pe, stays there (a); a column 3 % off it
                    relaxes to it in 30 calls (b).  riem_solver_c returns no w: every call of its relaxation starts from w = 0
  9   update_dz_d   interface heights == their initial function at the departure point; wsd = 0 to round-off over a flat surface

Thresholds; nothing is fitted to the library.  Pins 6, 7, 9: error <= 1.5 x the numpy oracle's on the same input (tests/golden/analytic_pins.json, ``python
tests/analytic_case.py --record``), error(C24) / error(C48) >= 3.5, C65 no worse than C48, C48 on 2 x 2 ranks within the whole tile's bounds.  The oracle's own
ratio of pin 9 is 6.3, so 3.5 holds there too.  heat_source and diss_est exactly 0; wsd <= 64 eps zs / dt (a constant through the transport: a few roundings of
zs = 100 m, over dt).  Pin 8 fp64: |w| <= 1e-9 x the control's, delz 1e-12, pe / peln / pk / pk3 1e-13, pef 1e-12, after the relaxation delz 1e-12 and |w| <=
1e-10.  fp32: pin 6 at C24 within the fp64 bounds (truncation > 1e3 eps32); pin 8 within 4 x the oracle's own residual in np.float32.

Pin 7, the classes of D-grid faces by their distance in lines from the nearest cube-tile edge (sub-domain edges inside a tile count as interior):
  class 0      on the edge.  Away from the cube corners the error is 1.5e-2 of the largest tendency at C24, 1.4e-2 at C48, 1.6e-2 at C65: it does not converge.
  class 1      the line next to the edge in the cross direction (u in cell columns 1 and nx, v in rows 1 and ny).  0.13 at C24, 0.28 at C48, 0.43 at C65: it grows as 1 / dx.
  second line  one line further in, in either direction.  The median error falls fourfold per doubling, isolated faces stay at 5e-3 .. 9e-3 (unexplained).
  class 2+     two or more lines from every tile edge.  1.6e-3 at C24, 4.1e-4 at C48 (ratio 3.89), 2.3e-4 at C65: second order.
What the split showed: the 1.6e-2 that a first measurement found on "the edge and the second line together", not converging, is class 0 itself, not the second line.  Both class 0 and class 1 are the tile-edge
kinetic-energy term of DESIGN.md section 2 (uncertain restatement 12): d_sw's corner kinetic energy on a tile edge holds 0.5 cot(alpha) Vn Vt above 0.5 |V|^2,
class 1 sees its difference across one cell (excess / L, growing as 1 / dx), class 0 its difference along the edge (a derivative, constant).  With the closed-form
term (edge_ke_excess, from corner geometry) taken off, class 0 away from the cube corners is left with 2.2e-3 (C24), 5.7e-4 (C48), 3.5e-4 (C65): ratio 3.9, asserted
as >= 1.8, which pins the term.  Class 1 is left with 6.0e-3 (C24), 8.7e-3 (C48) over the cube -- typical faces 5e-4 and 2.8e-4, below a factor 1.8, and the same
isolated faces as the second line -- so the remainder of class 1 is held by its recorded figure only.
The z-axis control: a flow about the z axis crosses tile 0's east edge at right angles (Vt = 0); there the class 1 faces show 4.9e-4 (C24) and 3.0e-4 (C48), inside
the class 2+ bound of the oblique flow, while the same faces under the oblique flow miss it by two orders: the term is what the derivation says.

Controls (CPU, oracle only), each asserting that the same checker raises CheckFailed: pins 6 and 9 against the solution turned the wrong way, pin 7 without the
Coriolis term in the expected tendency and class 1 held to the class 2+ bound under the oblique flow, pin 8 (b) against delz_eq built with the exponent kappa and
with the arithmetic mid-pressure.

Measured, host emulation and MI355X alike (fp64): every figure of pins 6, 7 and 9 equals the oracle's recorded one to the five digits printed (delp 3.4971e-04 /
5.1364e-05, ratio 6.81; pt 7.77, w 7.36, q_con 6.47, mfx 3.60, cx 3.75; pin 7 per class as listed above; zh 3.6444e-04 / 5.7780e-05, 6.31, C65 1.1201e-05; wsd 5.7e-16 ..
7.1e-16 zs / dt); pin 8 balanced |w| 3.9e-13 (nz 8) and 9.6e-13 (nz 79) against controls of 8.5 and 5.3 m/s, delz 2.0e-15 .. 2.1e-14, pe / peln exact, pk / pk3 4.4e-16, pef
1.6e-15 .. 2.0e-15; relaxed delz 1.6e-15 (nz 8) and 8.1e-15 (nz 79) with |w| 2.5e-13 (5.1e-10 and 7.1e-11 after ten calls), riem_solver_c 2.2e-15 and 2.1e-14.
fp32: pin 6 within 0.05 % of the fp64 figures on both backends; pin 8, oracle in np.float32 / host emulation / MI355X: relaxed delz of riem_solver3 1.5e-6 / 1.5e-6 / 1.8e-6
(nz 8) and 1.1e-5 / 1.1e-5 / 1.9e-5 (nz 79), balanced |w| 2.0e-4 / 2.1e-4 / 3.2e-4 and 2.5e-4 / 2.6e-4 / 4.3e-4, pef 6.3e-7 / 5.4e-7 / 9.6e-7 and 3.4e-7 / 3.5e-7 / 7.6e-7: the
device is within 2.3 x the oracle where 4 x is allowed.  No pin failed on its first run on either backend.
"""
import numpy as np
import pytest
import torch

import analytic_case as ac
from helpers import DIMS3, Case
from test_analytic_pins import _pad, _sync, backend32, memo  # noqa: F401  (backend32 is a fixture)

REC = ac.recorded()
EPS = float(np.finfo(np.float64).eps)
PIN6_FIELDS = ac.SCALARS + ("mfx", "mfy", "cx", "cy")
PIN7_HELD = ("class0", "class1", "second_line", "class2", "class0_less_edge_term", "class1_less_edge_term", "class0_inner", "class0_inner_less_edge_term")
WHOLE = {"c48_2x2": "c48"}  # the 2 x 2 ranks are held to the whole tile's figures


def _rec(pin, shape):
    return REC[pin][WHOLE.get(shape, shape)]


# ---------------------------------------------------------------------------------------------------------------------------
# pins 6 and 7: one d_sw call per backend and shape
# ---------------------------------------------------------------------------------------------------------------------------
def library_d_sw(backend, shape, axis=ac.AXIS, ranks=None, dtype=torch.float64):
    n, layout, rk = ac.SHAPES[shape]
    cs = Case(n, layout, rk if ranks is None else ranks, nz=ac.DYN_NZ, backend=backend, cfg_kw=ac.DSW_OFF, dtype=dtype)
    dc = ac.dsw_case(shape, cs.grids, cs.c, axis)
    Q = {k: cs.q([_pad(x[k]) for x in dc.ins]) if k in ac.D_SW_INPUTS else cs.q() for k in ac.D_SW_ORDER}
    cs.sf.call("d_sw", *[Q[k].fref for k in ac.D_SW_ORDER], dc.dt)
    _sync(backend)
    keep = ac.SCALARS + ("u", "v", "mfxd", "mfyd", "cxd", "cyd", "heat_source", "diss_est")
    return dc, [{k: Q[k].numpy(r) for k in keep} for r in range(len(cs.grids))]


def d_sw(backend, shape):
    def run():
        dc, outs = library_d_sw(backend, shape)
        assert abs(dc.dt - REC["pin6"][shape]["dt"]) <= 1e-12 * dc.dt
        return {"pin6": dc.scalar_errors(outs), "pin7": dc.wind_errors(outs)}

    return memo(("d_sw", backend, shape), run)


def check_scalars(label, e, rec):
    for k in PIN6_FIELDS:
        ac.check_bound(f"{label} {k}", e[k], rec[k])
    ac.require(e["heat"] == 0.0 and e["diss"] == 0.0, f"{label}: heat_source {e['heat']:.3e}, diss_est {e['diss']:.3e} with every damping term off")


@pytest.mark.parametrize("shape", list(ac.SHAPES))
def test_d_sw_carries_scalars_and_accumulates_fluxes(backend, shape):
    """pin 6: C24 and C48 on all six tiles, five of C48's 2 x 2 ranks, C65 (strip seam at i = 59)"""
    check_scalars(f"d_sw {shape}", d_sw(backend, shape)["pin6"], _rec("pin6", shape))


def test_d_sw_scalars_converge_at_second_order(backend):
    e24, e48, e65 = (d_sw(backend, s)["pin6"] for s in ("c24", "c48", "c65"))
    for k in PIN6_FIELDS:
        ac.check_convergence(f"d_sw {k}", e24[k], e48[k])
        ac.require(e65[k] <= e48[k], f"d_sw {k}: C65's error {e65[k]:.3e} above C48's {e48[k]:.3e}")


def test_fp32_d_sw_carries_scalars_and_accumulates_fluxes(backend32):
    """C24 in fp32: the bounds of fp64"""
    dc, outs = library_d_sw(backend32, "c24", dtype=torch.float32)
    check_scalars("fp32 d_sw c24", dc.scalar_errors(outs), REC["pin6"]["c24"])


@pytest.mark.parametrize("shape", list(ac.SHAPES))
def test_d_sw_wind_tendency_by_class_of_faces(backend, shape):
    """pin 7.  Class 2+ is the second-order scheme; classes 0 and 1 carry the tile-edge kinetic-energy term (module docstring: class 0 is the 1.5e-2 that does
    not converge, class 1 grows as 1 / dx, the second line converges but for isolated faces) and are held to the oracle's recorded figures, as are what
    is left of them once the closed-form term is taken off."""
    e, rec = d_sw(backend, shape)["pin7"], _rec("pin7", shape)
    for k in PIN7_HELD:
        ac.check_bound(f"d_sw tendency {shape} {k}", e[k], rec[k])


def test_d_sw_wind_tendency_converges_away_from_tile_edges(backend):
    """class 2+ at second order; class 0 away from the cube corners, less the closed-form edge term, by >= 1.8 per doubling (measured 3.9), which pins the
    term.  What is left of class 1 does not fall by 1.8 (6.0e-3 at C24, 8.7e-3 at C48: isolated faces) and is held by its recorded figure alone."""
    e24, e48, e65 = (d_sw(backend, s)["pin7"] for s in ("c24", "c48", "c65"))
    ac.check_convergence("d_sw tendency class 2+", e24["class2"], e48["class2"])
    ac.require(e65["class2"] <= e48["class2"], "d_sw tendency class 2+: C65's error above C48's")
    ac.check_convergence("d_sw tendency class 0 less the edge term", e24["class0_inner_less_edge_term"], e48["class0_inner_less_edge_term"], ratio=1.8)


def z_axis_error(outs_of):
    """tile 0 alone under the flow about the z axis: the class 1 faces next to its east edge"""
    return {shape: (lambda dc, outs: dc.wind_errors(outs, ac.tile0_east)["class1"])(*outs_of(shape)) for shape in ("c24", "c48")}


def check_z_axis(label, err):
    for shape, e in err.items():
        ac.check_bound(f"{label} {shape}, class 1 at tile 0's east edge against class 2+", e, REC["pin7"][shape]["class2"])


def test_d_sw_edge_term_vanishes_where_the_flow_crosses_the_edge_at_right_angles(backend):
    """the flow about the z axis crosses tile 0's east edge with Vt = 0: class 1 there meets the class 2+ bound of the oblique flow (4.9e-4 and 3.0e-4
    against 1.5 x 1.6e-3 and 1.5 x 4.1e-4)"""
    check_z_axis("z axis", z_axis_error(lambda shape: library_d_sw(backend, shape, ac.Z_AXIS, ranks=(0,))))


# ---------------------------------------------------------------------------------------------------------------------------
# pin 9: update_dz_d
# ---------------------------------------------------------------------------------------------------------------------------
def library_heights(backend, shape):
    n, layout, ranks = ac.SHAPES[shape]
    cs = Case(n, layout, ranks, nz=ac.DYN_NZ, backend=backend, cfg_kw=ac.DSW_OFF)
    hc = ac.HeightCase(n, cs.grids, cs.c.RADIUS)
    Q = {k: cs.q([x[k] for x in hc.ins]) for k in ("zh", "crx", "cry", "xfx", "yfx")}
    zs, ws = cs.q([x["zs"] for x in hc.ins], ("x", "y")), cs.qf.zeros(("x", "y"))
    cs.sf.call("update_dz_d", zs.fref, *[Q[k].fref for k in ("zh", "crx", "cry", "xfx", "yfx")], ws.fref, hc.dt)
    _sync(backend)
    R = range(len(cs.grids))
    return hc, [Q["zh"].numpy(r) for r in R], [ws.numpy(r) for r in R]


def heights(backend, shape):
    return memo(("pin9", backend, shape), lambda: (lambda hc, zh, ws: hc.errors(zh, ws))(*library_heights(backend, shape)))


def check_heights(label, err, ws, rec):
    ac.check_bound(f"{label} zh", err, rec["zh"])
    print(f"{label}: |wsd| dt / zs {ws:.2e}")
    ac.require(ws <= 64.0 * EPS, f"{label}: wsd {ws:.3e} zs / dt over a flat surface, above 64 eps")


@pytest.mark.parametrize("shape", list(ac.SHAPES))
def test_update_dz_d_carries_interface_heights_with_the_flow(backend, shape):
    check_heights(f"update_dz_d {shape}", *heights(backend, shape), _rec("pin9", shape))


def test_update_dz_d_converges_at_second_order(backend):
    ac.check_convergence("update_dz_d zh", heights(backend, "c24")[0], heights(backend, "c48")[0])
    ac.require(heights(backend, "c65")[0] <= heights(backend, "c48")[0], "update_dz_d: C65's error above C48's")


# ---------------------------------------------------------------------------------------------------------------------------
# pin 8: the Riemann solvers
# ---------------------------------------------------------------------------------------------------------------------------
RIEM3_ARGS = ("zs", "ws", "delz", "q_con", "delp", "pt", "zh", "pe", "ppe", "pk3", "pk", "peln", "w")
RIEMC_ARGS = ("zs", "ws", "pt", "q_con", "delp", "zh", "pe", "w")


def library_riem(cs, backend, col, which):
    def solve(f, dt, last):
        Q = {k: cs.q([v], ("x", "y") if k in ("zs", "ws") else DIMS3) for k, v in f.items()}
        if which == "3":
            cs.sf.call("riem_solver3", int(last), float(dt), Q["cappa"].fref, col.ptop, *[Q[k].fref for k in RIEM3_ARGS])
            back = ("w", "delz", "zh", "pe", "peln", "pk", "pk3")
        else:
            cs.sf.call("riem_solver_c", float(dt), Q["cappa"].fref, col.ptop, *[Q[k].fref for k in RIEMC_ARGS])
            back = ("zh", "pe")
        _sync(backend)
        for k in back:
            f[k] = Q[k].numpy(0).copy()

    return solve


def riem(backend, nz, which, dtype=torch.float64):
    cfg_kw = dict(nord=1) if dtype == torch.float32 else None  # (the default damping order overflows fp32 on a grid this coarse; the solvers do not read it)
    cs = Case(ac.RIEM_N, (1, 1), (0,), nz=nz, backend=backend, cfg_kw=cfg_kw, dtype=dtype)
    col = ac.Columns(cs.grids[0], cs.c, nz, dtype=np.float32 if dtype == torch.float32 else np.float64)
    return ac.riem_figures(col, ac.Geometry(cs.grids[0]).cells, library_riem(cs, backend, col, which), which)


@pytest.mark.parametrize("which", ["3", "c"])
@pytest.mark.parametrize("nz", ac.RIEM_LEVELS)
def test_riemann_solvers_hold_and_find_the_hydrostatic_thickness(backend, nz, which):
    """pin 8, C12 with 8 and 79 levels: (a) one call at dt 20 s leaves the balanced column alone and moves the control; (b) 30 calls at dt 200 s bring the
    control to delz_eq = -(delp / g) R pt pm^(kappa - 1)"""
    fig = riem(backend, nz, which)
    ac.check_balanced(f"riem_solver{which} nz {nz}", fig, which)
    ac.check_relaxed(f"riem_solver{which} nz {nz}", fig, which)


@pytest.mark.parametrize("which", ["3", "c"])
@pytest.mark.parametrize("nz", ac.RIEM_LEVELS)
def test_fp32_riemann_solvers_hold_and_find_the_hydrostatic_thickness(backend32, nz, which):
    """every figure within 4 x the numpy oracle's own in np.float32 (the fp32 log / exp of numpy and of the device differ by a few ulp per level)"""
    fig, bound = riem(backend32, nz, which, torch.float32), REC["pin8"][f"nz{nz}"]["fp32"][which]
    ac.check_balanced(f"fp32 riem_solver{which} nz {nz}", fig, which, bound)
    ac.check_relaxed(f"fp32 riem_solver{which} nz {nz}", fig, which, bound)


# ---------------------------------------------------------------------------------------------------------------------------
# the controls: every checker has teeth (CPU, oracle only)
# ---------------------------------------------------------------------------------------------------------------------------
def _oracle_d_sw(shape, axis=ac.AXIS, ranks=None):
    n, layout, rk = ac.SHAPES[shape]
    part, grids, doms, c = ac.make(n, layout, rk if ranks is None else ranks, ac.DYN_NZ)
    dc = ac.dsw_case(shape, grids, c, axis)
    return dc, ac.oracle_d_sw(doms, ac.dyn_config(n, layout), dc)


def test_control_pin6_solution_turned_the_wrong_way_fails():
    dc, outs = _oracle_d_sw("c24")
    check_scalars("oracle d_sw c24", dc.scalar_errors(outs), REC["pin6"]["c24"])
    with pytest.raises(ac.CheckFailed):
        check_scalars("oracle d_sw c24 (wrong way)", dc.scalar_errors(outs, way=-1.0), REC["pin6"]["c24"])


def test_control_pin7_tendency_without_coriolis_fails():
    dc, outs = _oracle_d_sw("c24")
    ac.check_bound("oracle d_sw tendency c24 class 2+", dc.wind_errors(outs)["class2"], REC["pin7"]["c24"]["class2"])
    dc.rot = 0.0
    with pytest.raises(ac.CheckFailed):
        ac.check_bound("oracle d_sw tendency c24 class 2+ (no Coriolis term)", dc.wind_errors(outs)["class2"], REC["pin7"]["c24"]["class2"])


def test_control_pin7_oblique_flow_misses_the_right_angle_bound():
    """the z-axis control passes on the oracle and raises under the oblique flow, on the same faces"""
    check_z_axis("oracle, z axis", z_axis_error(lambda shape: _oracle_d_sw(shape, ac.Z_AXIS, ranks=(0,))))
    with pytest.raises(ac.CheckFailed):
        check_z_axis("oracle, oblique axis", z_axis_error(lambda shape: _oracle_d_sw(shape, ranks=(0,))))


@pytest.mark.parametrize("spoil", ["exponent", "midpoint"])
def test_control_pin8_wrong_equilibrium_fails(spoil):
    """delz_eq built with the exponent kappa for kappa - 1, or with the arithmetic mid-pressure for pm: the relaxation does not end there"""
    good, bad = ac.measure_riem(8), ac.measure_riem(8, spoil=spoil)
    for which in ("3", "c"):
        ac.check_balanced(f"oracle riem_solver{which}", good[which], which)
        ac.check_relaxed(f"oracle riem_solver{which}", good[which], which)
        with pytest.raises(ac.CheckFailed):
            ac.check_relaxed(f"oracle riem_solver{which} ({spoil})", bad[which], which)


def test_control_pin9_solution_turned_the_wrong_way_fails():
    n, layout, ranks = ac.SHAPES["c24"]
    part, grids, doms, c = ac.make(n, layout, ranks, ac.DYN_NZ)
    hc = ac.HeightCase(n, grids, c.RADIUS)
    zhs, wss = ac.oracle_heights(doms, grids, ac.dyn_config(n, layout), hc)
    check_heights("oracle update_dz_d c24", *hc.errors(zhs, wss), REC["pin9"]["c24"])
    with pytest.raises(ac.CheckFailed):
        check_heights("oracle update_dz_d c24 (wrong way)", *hc.errors(zhs, wss, way=-1.0), REC["pin9"]["c24"])
