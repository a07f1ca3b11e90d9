"""The corner divergence of c_sw and the damping operators of d_sw against closed-form solutions (builders, exact solutions and checkers:
tests/damping_case.py), continuing tests/test_analytic_pins.py and tests/test_analytic_dynamics.py under the same ground rule: inputs and expected values come
from corner positions, cell centres, the sphere radius and closed-form functions of position; no metric array a kernel reads enters an expected value (edge
lengths are great-circle distances of the corners; area weights the l2 norm of pin 13 and nothing else).  The stated exception: da_min and da_min_c enter the
expected coefficients as configuration, and are held here once to the smallest spherical-excess area of the cells and of the dual cells
(test_area_minima_are_the_smallest_spherical_excess_areas).  Nothing below needs the oracle at run time.

Fields: solid-body rotation about AXIS (analytic_case.Flow), a potential flow V = grad chi, chi = a c P_l(p . b) about the oblique pole b (div V = -l (l + 1)
chi / a^2, no vorticity), l = 3 and l = 1; scalars d0 (1 + eps P_3(p . b)); for pin 13 a rotational wind with the stream function a c P_3(p . b).

  10  c_sw, divgd   == -div(V_rot + V_div) at the corners, by class of corners; the rotation alone gives 0.  FV3's divg_d is MINUS the divergence (uf(i-1) -
                    uf(i) + vf(j-1) - vf(j)), and so is the library's and the oracle's: d_sw's ke += damp divg_d then damps.
  11  c_sw, dt2 != 0  two calls on the rotation with smooth delp, pt, w, at dt2 = half of dyn_dt and at 0: delpc, ptc, omga == the fields at the departure
                    points of the half step (Flow.rotate_back); (uc, vc)(dt2) - (uc, vc)(0) == dt2 x the projection of -(zeta + f) k x V - grad K (zeta, f
                    and K in closed form, as pin 7) on Geometry.e1 / e2, by face_classes.  The transport is first-order upwind, but at a Courant number
                    falling as 1 / n its error falls fourfold per doubling (oracle: 3.7 .. 4.0); the wind tendency is first order (oracle: 2.0 on every class).
  12  d_sw          two calls on identical inputs, the damping under test against DSW_OFF; the damping enters ke linearly, so u dx (on) - u dx (off) ==
                    F(A) - F(B) over the face from corner A to corner B, F = [da_min_c d2 + (da_min_c d4_bg)^(n + 1) lam^n] divg_d (every pass of FV3's chain is
                    MINUS the Laplacian, so no (-1)^n is left), lam = l (l + 1) / a^2; with dddmp = 0.5 (nord 2) F += da_min_c dddmp dt sqrt(divg_d^2 + zeta^2)
                    divg_d, zeta = 2 omega (p . axis), in the free branch.  divgd is handed in as the exact -div V.  d_sw returns u dx and v dy (fv3_d_sw's
                    contract, as the reference operator; dyn_core divides afterwards), so the increment is compared per unit length, over arc(A, B) a.
  13  d_sw at rest  uc = vc = 0 (no transport), default configuration on five levels: one call takes the share (damp area lam)^(n + 1) off the harmonic part of
                    delp, pt, q_con (area = da_min, fv_tp_2d's deln_flux) and w (da_min_c, d_sw's own del6_vt_flux), and changes the rotational wind by minus
                    that share (da_min_c) of itself; the (order, coefficient) pair of every field and level is written out by hand (damping_case.SPONGE_TABLE),
                    with n_sponge = -1 as a second case.  The l2 norm of every harmonic does not grow.

What the pins found (restatements 13 and 14), none of it a difference between library and oracle:
  * FV3's del-n operator is not the Laplacian on this grid.  Its fluxes are sina dy / dx times the difference along the grid line (divg_u, del6_v), without the
    cross-derivative terms a non-orthogonal grid needs, so a harmonic is not its eigenfunction: the oracle's one pass over P_3 gives 0.93 .. 1.05 lam P_3 along a
    tile's centre line, 0.67 .. 1.96 a quarter tile off it, the same at C24 and C48 (it does not converge).  The closed forms of pins 12 (nord >= 1) and 13 hold
    only where the grid lines cross at right angles and the cells are square, at the tile's centre.  The missing term grows as the square of the distance
    from it, so class "centre" reaches two cells from the centre at every resolution and one pass converges there: the scalars 2.4e-2 (C24), 1.0e-2 (C48),
    5.6e-3 (C65), the vorticity 8.7e-3, 2.1e-3, 6.9e-4, del2_cubed 1.9e-2, 9.5e-3, 5.6e-3, the damping heat 1.3e-2, 3.2e-3, 1.3e-3.  The chains do not: 8e-2
    (nord 1), 0.37 (nord 2) and 1.0 (nord 3) for the divergence, 0.51 .. 0.29 for the del-6 of the scalars (the error of a pass is not smooth, and the next
    passes differentiate it).  That still tells the
    exponent n from n + 1 (a factor 1e9 or more), da_min from da_min_c (27 %), the mass-weighted flux with and without its 1/2 and the sponge table from the
    table one level down on the one-pass levels; it does not check the higher orders to better than their order of magnitude, and a bound "<= 1.5 x the
    oracle's error" of 0.5 or 1.0 passes a library that damps nothing.  So the amount damped ("largest" of pin 12, on the centre faces; "size" of pins 13 and 14, on the
    interior class: the largest change got over the largest exact one, 0.31 .. 1.9) is held to the oracle's both ways, within 1.5 x -- parity, not closed form.  Every other class is held to the oracle's recorded figure, which says
    that library and oracle agree there and nothing more.
  * divergence_corner is O(1) wrong on the tile-edge line: 9.1e-2 of the largest divergence at C24, 9.6e-2 at C48, 7.1e-2 at C65 (l = 1: 0.23, 0.24, 0.23), zero
    at the middle of an edge and growing towards its ends, the same for the rotation alone (3.7e-2).  The winds in the halo are not the cause (they equal the
    exchanged ones to 1e-13), nor are d2a2c_vect's ua / va: with the analytic contravariant winds handed to the oracle's divergence_corner the edge line stays at
    9.8e-2 (C24) and 9.9e-2 (C48) and the cube corners unchanged (the tile-edge flux of divergence_corner reads no ua / va).  The cause is dxc / dyc across the edge: the straight arc between
    two centres, while the dual cell's side bends there and rarea_c is the bent cell's; with the bent length (up to 14 % more) in the oracle's metric the edge line
    falls to 8.7e-3 (C24) and 4.8e-3 (C48).  Whether FV3's dxc is the straight arc is not known here, so nothing was changed (restatement 14).  The
    nord-0 damping increment on the faces that touch the edge (classes 0 and 1) is this error over dx: 0.76 / 0.90 at C24, 1.4 / 1.8 at C48.
  * one line of corners, three from a tile edge, is first order (3.4e-3, 1.9e-3): there d2a2c_vect goes from two-point to four-point averages (with the
    analytic ua / va the line is second order, 1.7e-3 and 4.0e-4).

Thresholds; nothing is fitted to the library.  Every figure <= 1.5 x the numpy oracle's on the same input (tests/golden/analytic_pins.json, ``python
tests/analytic_case.py --record damping``); C48 on 2 x 2 ranks is held to its own record (its ranks see other faces than the whole tile).  Round-off bounds: the
rotation's divergence at a cube corner <= 64 eps max|V| / sqrt(da_min_c) (six products of |V| dyc, summed and divided by the dual area); the rotation's
increment under nord 2 (divgd = 0 handed in) <= 8 x eps max |u dx| / L, the round-off of the difference.  Pin 15: second order (ratio >= 3.5 from C24 to C48) is
asserted where the oracle's record shows it: pin 10 "interior", pin 12 nord 0 and the Smagorinsky case on "class2" and "second_line" (nord 0) -- not on
any edge class and not on "centre" of the higher orders, which do not converge (above).  Every on/off difference has its closed-form signal >= 1e4 x eps |u dx| /
L (asserted): 2.6e12 (nord 0) .. 2.4e5 (nord 3) at C24; nord 3 has 9e2 at C48 and runs at C24 only.
fp32 (backend32): pin 11 at C24 within the fp64 bounds (truncation 2e-3 / 2e-2 against eps32 x 4 and eps32 / (dt2 (zeta + f)) = 2e-6); pin 10 at C24; the error of the interior is truncation (1.9e-3 >> eps32 |V| / dx / max|D| = 1e-5 x 12), the bounds of fp64 with eps32 x 64 x
max|V| / sqrt(da_min_c) added.

stretched_grid (pin 12, nord 1, the C12 grid of tests/stretched_case.py): FV3's da_min d4_bg^(nord + 1) is not a power of an area; with d4_bg = 0.15 its increment
is 0.28 x the round-off of the on/off difference, so the form is tested at d4_bg = 0.15 da_min_c / sqrt(da_min) = 2.8e4 (the closed form is linear in dd8).
On this grid (C12, one chain pass, cells three times finer on one tile than opposite) the record is O(1) on every class, "centre" 0.79 and "class2" 1.0: the
closed-form coefficient da_min d4_bg^(n + 1) is not checked to better than the factor 1.5 of the both-ways "largest" figure, which is parity with the oracle at
the equivalent d4_bg.  It tells the stretched form from the congruent one (1e10) and nothing finer.
l = 1 (pin 12): the nord-0 run is repeated on the potential flow of degree 1 at C24 ("nord0_l1": class 2+ 3.9e-3, centre 1.8e-3).

  14  the damping heat  (a) d_sw at rest with every damping one pass (nord 0, so nord_v = nord_w = 0; n_sponge -1), d_con = 1, ke_bg = 0, no divergence damping, and
                    vtdm4 set so that one call takes the share s = 0.2 off the wind and off w: heat_source == delp [(s - s^2 / 2) |V|^2 + s w' (w - s w' / 2)],
                    the kinetic energy -(V . dV + |dV|^2 / 2) - dw (w + dw / 2) taken by dV = -s V, dw = -s w' (w' = 40 P_3(p_z), the harmonic part of w, as
                    large as the wind and +-1 x 40 at the centres of the polar tiles); the controls without |dV|^2 / 2 and without dw^2 / 2 miss by 6.5e-2 and
                    6.2e-2 against 1.3e-2.  Under the default sponge (second case, the same fields) the column's d_con
                    is off on levels 0 - 2: the wind heat is 0 there although the wind is damped, the heat of w is still added under the global d_con, and
                    heat_source == s_k w' (w - s_k w' / 2) with the one-pass shares of SPONGE_TABLE, without the delp weight (FV3's d_sw weighs by delp inside
                    the block the level's d_con guards; library and oracle do the same): "centre" 1.1e-2 (C24), 2.9e-3 (C48), ratio 3.8.  The regular levels 3 - 4
                    are of order 2 (restatement 13) and are recorded.  (b) fv3_del2_cubed, nmax
                    1 - 3, cd = 0.2 da_min: the harmonic part times (1 - cd lam)^nmax.  (c) apply_diffusive_heating is pointwise: pt += sign(dT) min(lim_k, |dT|) /
                    pkz, dT = heat / (cv delp), pkz = (rdg delp pt / delz)^(cappa / (1 - cappa)), to round-off (4 eps |pt| + 32 eps |dpt|), fp32 likewise.  This
                    is the staged operator.  The fused form (fv3_del2_heat_fused, FV3_DEL2_HEAT) has no entry in the C ABI; it runs inside fv3_acoustic_step
                    only, where tests/test_parity.py holds it bitwise to the staged operators pinned here.
fp32, pin 13 (C24, the default sponge over nord = 1, which the fp32 context accepts): the one-pass levels on "centre" within the fp64 bound plus 8 eps32 x the
field over the largest exact change, "size" both ways with the same allowance; the order-1 levels change the fields by less than eps32 and must be finite.  Both kinds run: "mass" for the del-2 of delp, "fields" for the rest.

Controls (CPU, oracle only), each asserting that the same checker raises CheckFailed: pin 10 against +div V; pin 11 against the fields turned the wrong way
and without the Coriolis term; pin 12 with the exponent n for n + 1 (nord 1, 2,
3), with da_min for da_min_c (nord 0, Smagorinsky), with a (-1)^n put in (nord 1, 3); pin 13 with the exponent n, with the mass-weighted flux taken without its
1/2, with the sponge table one level down (on the one-pass levels); pin 14 with the heat without |dV|^2 / 2 and without dw^2 / 2, with the wind heat left on at the sponge levels and the heat of w weighted by delp there, del2_cubed with a pass too few, the heating without
its limit.
The same mistakes put into a scratch copy of the kernel sources (host-emulation build) fail the matching pins at C24: dd8 with the exponent nord -> pin 12
nord 1, 2, 3 and the Smagorinsky case (nord 3 by "largest" alone); d6_w with the exponent nord_w -> pin 13 "fields" (w); the sponge's damp_vt = d2 for 0.5 d2 ->
pin 13 "mass" and "fields"; the heat of w without dw / 2 (every form) -> pin 14 "centre" (4.9e-2 against 1.3e-2); d_con kept on at the sponge levels of the context's table -> pin 14 under the default sponge, and no other pin; fC taken out of c_sw -> pin 11; da_min for da_min_c in the context -> pin 12 at every order, pin 13 w and vort; the
mass-weighted deln flux without its 1/2 (every form of fv_tp_2d) -> pin 13 pt and q_con at every level.

Measured, host emulation and MI355X alike (fp64): every figure of pins 10 - 14 equals the oracle's recorded one to the five digits printed (pin 10 interior
1.9120e-03 / 4.8095e-04 / 2.1789e-04 at C24 / C48 / C65, ratio 3.98; pin 11 delpc 2.8e-3 / 7.6e-4, class 2+ 3.0e-2 / 1.5e-2; pin 12 nord 0 class 2+ 2.7e-3 / 6.9e-4,
Smagorinsky 2.4e-4 / 6.2e-5; pin 13 and 14 "centre" as listed above, ratios 4.09 (vorticity), 2.38 (scalars), 4.01 (heat)), the rotation's cube-corner divergence
2.3e-14 (C24) .. 1.2e-13 (C65) of bounds 1.7e-13 .. 4.6e-13 (fp32: 3.9e-7 of 9.1e-5), the rotation's nord-2 increment exactly 0 against a round-off of 6.6e-9 of the
potential flow's, apply_diffusive_heating exact in fp64 and 0.23 of its bound in fp32; fp32 pin 13 "centre" 2.3e-2 .. 2.5e-2 (scalars) and 8.7e-3 (vorticity)
against the fp64 oracle's 2.4e-2 and 8.7e-3.  The damping heat under the default sponge: "centre" 1.0891e-02 / 2.8981e-03 on levels 0 - 2, as the oracle's.  The 58 GPU cases take 11 s together.
"""
import numpy as np
import pytest
import torch

import analytic_case as ac
import damping_case as dm
from helpers import DIMS3, Case
from test_analytic_pins import _pad, _sync, backend32, memo  # noqa: F401  (backend32 is a fixture)

REC = ac.recorded()
EPS = float(np.finfo(np.float64).eps)
EPS32 = float(np.finfo(np.float32).eps)
C_SW_ORDER = ("delp", "pt", "u", "v", "w", "uc", "vc", "ua", "va", "ut", "vt", "divgd", "omga", "delpc", "ptc")
HELD10 = ("interior", "third_line", "edge", "corner")


def check_all(label, e, rec, keys):
    for k in keys:
        ac.check_bound(f"{label} {k}", e[k], rec[k])


# ---------------------------------------------------------------------------------------------------------------------------
# the configuration scalars of the expected coefficients
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["c24", "c48_2x2"])
def test_area_minima_are_the_smallest_spherical_excess_areas(shape):
    """da_min / da_min_c of the grid against the spherical excess of the cells / dual cells from corner and centre positions, over all ranks of the cube"""
    n, layout, _ = ac.SHAPES[shape]
    part, grids, doms, c = ac.make(n, layout, range(6 * layout[0] * layout[1]), 1)
    amin, cmin = dm.area_minima(grids, c.RADIUS)
    for g in grids:
        assert abs(g.da_min - amin) <= 1e-11 * amin and abs(g.da_min_c - cmin) <= 1e-11 * cmin, (g.da_min, amin, g.da_min_c, cmin)
    assert 1.2 < amin / cmin < 1.5  # (the two differ by enough for the pins to tell them apart)


# ---------------------------------------------------------------------------------------------------------------------------
# pin 10: the corner divergence of c_sw
# ---------------------------------------------------------------------------------------------------------------------------
def library_c_sw(backend, cs, ins, dt2=0.0):
    Q = {k: (cs.q([_pad(x[k]) for x in ins]) if k in ins[0] else cs.qf.ones(DIMS3) if k in ("delp", "pt") else cs.q()) for k in C_SW_ORDER}
    cs.sf.call("c_sw", *[Q[k].fref for k in C_SW_ORDER], float(dt2))
    _sync(backend)
    return [{k: Q[k].numpy(r) for k in ("divgd", "uc", "vc", "delpc", "ptc", "omga")} for r in range(len(cs.grids))]


def library_divergence(backend, shape, dtype=torch.float64):
    n, layout, ranks = ac.SHAPES[shape]
    cs = Case(n, layout, ranks, nz=ac.DYN_NZ, backend=backend, cfg_kw=dict(nord=1), dtype=dtype)
    out = {}
    for key, kw in (("l3", dict(l=3)), ("l1", dict(l=1)), ("rotation", dict(rotation_only=True))):
        dc = dm.DivergenceCase(cs.grids, cs.c.RADIUS, **kw)
        out[key] = dc.errors([o["divgd"] for o in library_c_sw(backend, cs, dc.ins)])
    g = cs.grids[0]
    out["round_off"] = dc.top_wind / np.sqrt(g.da_min_c) / dc.top_div  # max|V| / sqrt(da_min_c) in the unit of the errors
    return out


def divergence(backend, shape):
    return memo(("pin10", backend, shape), lambda: library_divergence(backend, shape))


def check_divergence(label, e, rec, extra=0.0):
    for key in ("l3", "l1"):
        for k in HELD10:
            ac.check_bound(f"{label} {key} {k}", max(e[key][k] - extra, 0.0), rec[key][k])
    for k in ("interior", "third_line", "edge"):
        ac.check_bound(f"{label} rotation {k}", max(e["rotation"][k] - extra, 0.0), rec["rotation"][k])
    bound = 64.0 * EPS * e["round_off"] + extra
    print(f"{label} rotation, cube corners: {e['rotation']['corner']:.3e}, bound {bound:.3e}")
    ac.require(e["rotation"]["corner"] <= bound, f"{label}: the rotation's divergence at a cube corner {e['rotation']['corner']:.3e} above {bound:.3e}")


@pytest.mark.parametrize("shape", list(ac.SHAPES))
def test_corner_divergence_of_a_potential_flow(backend, shape):
    """pin 10: divgd of c_sw == -div V at every compute corner, l = 3 and l = 1 on top of the rotation, and the rotation alone"""
    check_divergence(f"divgd {shape}", divergence(backend, shape), REC["pin10"][shape])


def test_corner_divergence_converges_at_second_order_in_the_interior(backend):
    """pin 15 for pin 10.  The tile-edge line and the cube corners do not converge and the third line is first order (module docstring): held by their records"""
    e24, e48, e65 = (divergence(backend, s) for s in ("c24", "c48", "c65"))
    for key in ("l3", "l1", "rotation"):
        ac.check_convergence(f"divgd {key} interior", e24[key]["interior"], e48[key]["interior"])
        ac.require(e65[key]["interior"] <= e48[key]["interior"], f"divgd {key}: C65's error above C48's")


def test_fp32_corner_divergence_of_a_potential_flow(backend32):
    """C24 in fp32: the bounds of fp64 plus 64 eps32 max|V| / sqrt(da_min_c)"""
    e = library_divergence(backend32, "c24", dtype=torch.float32)
    check_divergence("fp32 divgd c24", e, REC["pin10"]["c24"], extra=64.0 * EPS32 * e["round_off"])


# ---------------------------------------------------------------------------------------------------------------------------
# pin 11: the half step of c_sw
# ---------------------------------------------------------------------------------------------------------------------------
HELD11 = tuple(dm.CSW_SCALARS) + tuple(dm.FACE_KEYS.values())


def library_half_step(backend, shape, dtype=torch.float64):
    n, layout, ranks = ac.SHAPES[shape]
    cs = Case(n, layout, ranks, nz=ac.DYN_NZ, backend=backend, cfg_kw=dict(nord=1), dtype=dtype)
    cc = dm.CswCase(n, cs.grids, cs.c.RADIUS, cs.c.OMEGA)
    assert abs(cc.dt2 - REC["pin11"][shape]["dt2"]) <= 1e-12 * cc.dt2
    return cc.errors(library_c_sw(backend, cs, cc.ins, cc.dt2), library_c_sw(backend, cs, cc.ins, 0.0))


def half_step(backend, shape):
    return memo(("pin11", backend, shape), lambda: library_half_step(backend, shape))


@pytest.mark.parametrize("shape", list(ac.SHAPES))
def test_c_sw_half_step_on_the_rotation(backend, shape):
    """pin 11: two c_sw calls, at dt2 (half the Courant number of dyn_dt) and at 0"""
    check_all(f"c_sw half step {shape}", half_step(backend, shape), REC["pin11"][shape], HELD11)


def test_c_sw_half_step_converges(backend):
    """the scalars at second order in this setting (first-order upwind at a Courant number that falls as 1 / n: error ~ c h^2; the oracle's ratios 3.7 .. 4.0),
    the wind tendency at first order (the upwind corner vorticity and the one-sided kinetic energy; the oracle's ratio 2.0 on every class): asserted as >= 1.8"""
    e24, e48, e65 = (half_step(backend, s) for s in ("c24", "c48", "c65"))
    for k in dm.CSW_SCALARS:
        ac.check_convergence(f"c_sw {k}", e24[k], e48[k])
    for k in dm.FACE_KEYS.values():
        ac.check_convergence(f"c_sw tendency {k}", e24[k], e48[k], ratio=1.8)
    for k in HELD11:
        ac.require(e65[k] <= e48[k], f"c_sw {k}: C65's error above C48's")


def test_fp32_c_sw_half_step_on_the_rotation(backend32):
    """C24 in fp32: the bounds of fp64 (truncation 2e-3 of the scalars and 2e-2 of the tendency against eps32 x 4 and eps32 / (dt2 (zeta + f)) = 2e-6)"""
    check_all("fp32 c_sw half step c24", library_half_step(backend32, "c24", dtype=torch.float32), REC["pin11"]["c24"], HELD11)


# ---------------------------------------------------------------------------------------------------------------------------
# pins 12 and 13: d_sw
# ---------------------------------------------------------------------------------------------------------------------------
def library_d_sw(backend, shape, cfg_kw, ins, dt, nz, dtype=torch.float64, cs=None):
    """one d_sw call on the case's inputs; ``cs``: a ready Case (the stretched grid), else the shape's"""
    if cs is None:
        n, layout, ranks = ac.SHAPES[shape]
        cs = Case(n, layout, ranks, nz=nz, backend=backend, cfg_kw=cfg_kw, dtype=dtype)
    Q = {k: cs.q([_pad(x[k]) for x in ins]) if k in ins[0] else cs.q() for k in ac.D_SW_ORDER}
    cs.sf.call("d_sw", *[Q[k].fref for k in ac.D_SW_ORDER], float(dt))
    _sync(backend)
    return [{k: Q[k].numpy(r) for k in ac.SCALARS + ("u", "v", "heat_source")} for r in range(len(cs.grids))]


def library_divdamp(backend, shape, run, rotation_only=False):
    """(the figures, the scale they are quoted in when the rotation runs alone)"""
    n, layout, ranks = ac.SHAPES[shape]
    part, grids, _, c = ac.make(n, layout, ranks, ac.DYN_NZ)
    dc = dm.DivDampCase(n, grids, c.RADIUS, c.OMEGA, l=dm.DIVDAMP_L.get(run, 3), rotation_only=rotation_only)
    on = library_d_sw(backend, shape, dm.damp_config(run), dc.ins, dc.dt, ac.DYN_NZ)
    off = library_d_sw(backend, shape, ac.DSW_OFF, dc.ins, dc.dt, ac.DYN_NZ)
    scale = dm.rotation_scale(n, grids, c, run) if rotation_only else None
    return dc.errors(on, off, dm.damp_config(run), scale=scale), scale


def check_size(label, got, rec):
    """how much was damped, held to the oracle's both ways: where the closed form cannot tell a damping that is too weak from the scheme's own deviation (the
    chains of order >= 1, module docstring), a figure "<= 1.5 x the oracle's error" alone would pass a library that damps nothing"""
    print(f"{label}: {got:.4e}, oracle {rec:.4e}")
    ac.require(rec / ac.SLACK <= got <= ac.SLACK * rec, f"{label}: {got:.4e} is not within {ac.SLACK} x the oracle's {rec:.4e} either way")


def check_divdamp(label, e, rec):
    print(f"{label}: signal {e['signal']:.2e} x the round-off of the difference")
    ac.require(e["signal"] >= 1e4, f"{label}: the closed-form signal is only {e['signal']:.2e} x eps |u dx| / L")
    check_all(label, e, rec, dm.HELD12)
    check_size(f"{label} largest increment", e["largest"], rec["largest"])


@pytest.mark.parametrize("shape, run", [(s, r) for s, runs in dm.DIVDAMP_SHAPES.items() for r in runs])
def test_divergence_damping_increment(backend, shape, run):
    """pin 12: nord 0 with d2_bg, nord 1 .. 3 with d4_bg, nord 2 with dddmp = 0.5 in the free branch.  "class2" and "second_line" are the closed form for nord 0
    and the Smagorinsky case, "centre" for the chains (module docstring)"""
    e = memo(("pin12", backend, shape, run), lambda: library_divdamp(backend, shape, run)[0])
    check_divdamp(f"divergence damping {shape} {run}", e, REC["pin12"][shape][run])


def test_divergence_damping_leaves_the_rotation_alone(backend):
    """nord 2: divgd = 0 is handed in and the chain returns 0 -- the increment is 0 to the round-off of the difference.  nord 0 forms its own divergence
    from the winds: its truncation error, held to the record (in the unit of the same run's largest increment on V_rot + V_div)"""
    e, scale = library_divdamp(backend, "c24", "nord2", rotation_only=True)
    worst = max(e[k] for k in dm.HELD12)
    print(f"rotation, nord 2: largest increment {worst:.3e} of the potential flow's, round-off of the difference {e['noise'] / scale:.3e}")
    ac.require(worst * scale <= 8.0 * e["noise"], f"the rotation's increment {worst:.3e} under nord 2 is above the round-off of the difference")
    check_all("rotation, nord 0", library_divdamp(backend, "c24", "nord0", rotation_only=True)[0], REC["pin12_rotation"]["c24"]["nord0"], dm.HELD12)


def test_divergence_damping_on_the_stretched_grid(backend):
    """stretched_grid: dd8 = da_min d4_bg^(nord + 1), nord 1 on the C12 grid of tests/stretched_case.py, at the d4_bg that makes the form visible
    (damping_case.stretched_config).  The oracle's record was made with the congruent form at the equivalent d4_bg"""
    import stretched_case as sc

    grids, _, c = dm.stretched_grids()
    kw = dm.stretched_config(grids[0])
    dc = dm.DivDampCase(dm.STRETCHED_N, grids, c.RADIUS, c.OMEGA)
    with sc.stretched():
        on, off = (library_d_sw(backend, None, None, dc.ins, dc.dt, ac.DYN_NZ, cs=Case(dm.STRETCHED_N, (1, 1), range(6), nz=ac.DYN_NZ, backend=backend, cfg_kw=k)) for k in (kw, ac.DSW_OFF))
    check_divdamp("divergence damping, stretched C12 nord 1", dc.errors(on, off, kw), REC["pin12_stretched"]["c12_stretched"][dm.STRETCHED_RUN])


def test_control_pin12_congruent_form_on_the_stretched_grid_fails():
    grids, doms, c = dm.stretched_grids()
    kw = dm.stretched_config(grids[0])
    dc = dm.DivDampCase(dm.STRETCHED_N, grids, c.RADIUS, c.OMEGA)
    import stretched_case as sc

    d4 = sc.equivalent_d4_bg(grids[0], kw["d4_bg"], kw["nord"])
    on, off = dm.oracle_d_sw_pair(doms, ac.dyn_config(dm.STRETCHED_N, (1, 1), nord=kw["nord"], d4_bg=d4), ac.dyn_config(dm.STRETCHED_N, (1, 1)), dc)
    rec = REC["pin12_stretched"]["c12_stretched"][dm.STRETCHED_RUN]
    check_divdamp("oracle, stretched C12 nord 1", dc.errors(on, off, kw), rec)
    with pytest.raises(ac.CheckFailed):
        check_size("oracle, stretched C12 nord 1 (congruent form) largest increment", dc.errors(on, off, dict(kw, stretched_grid=False))["largest"], rec["largest"])


def test_divergence_damping_converges_at_second_order_where_it_is_closed_form(backend):
    """pin 15 for pin 12: nord 0 away from the tile edges and the Smagorinsky case two or more lines from them (its second line carries the chain's edge error)"""
    get = lambda shape, run: memo(("pin12", backend, shape, run), lambda: library_divdamp(backend, shape, run)[0])  # noqa: E731
    for run, keys in (("nord0", ("class2", "second_line")), ("smag", ("class2",))):
        for k in keys:
            ac.check_convergence(f"divergence damping {run} {k}", get("c24", run)[k], get("c48", run)[k])
            ac.require(get("c65", run)[k] <= get("c48", run)[k], f"divergence damping {run} {k}: C65's error above C48's")


def library_rest(backend, shape, kind, dtype=torch.float64, **kw):
    n, layout, ranks = ac.SHAPES[shape]
    part, grids, _, c = ac.make(n, layout, ranks, dm.DAMP_NZ)
    rc = dm.RestCase(grids, c.RADIUS, kind)
    cfg_kw = {**dm._DEFAULTS, **dm.REST_CONFIG, **kw}
    outs = library_d_sw(backend, shape, cfg_kw, rc.ins, rc.dt, dm.DAMP_NZ, dtype=dtype)
    return rc.errors(outs, dm.table_for(kw))


def check_rest(label, e, rec, whole_sphere=True):
    """every class figure against the record; the l2 norm of a harmonic over the whole sphere does not grow (over some ranks alone it may: what leaves them is not
    seen)"""
    assert set(e) == set(rec), set(e) ^ set(rec)
    for k in sorted(e):
        if k.endswith(".l2"):
            print(f"{label} {k}: 1 {e[k] - 1.0:+.3e}")
            ac.require(not whole_sphere or e[k] <= 1.0 + 4.0 * EPS, f"{label} {k}: the harmonic grew by {e[k] - 1.0:.3e} in one damped call")
        elif k.endswith(".size"):
            check_size(f"{label} {k}", e[k], rec[k])
        elif k.endswith(".top"):
            assert abs(e[k] - rec[k]) <= 1e-9 * rec[k], (k, e[k], rec[k])  # (the exact change: the same closed form here and in the record)
        else:
            ac.check_bound(f"{label} {k}", e[k], rec[k])


@pytest.mark.parametrize("kind", ["mass", "fields"])
@pytest.mark.parametrize("shape", list(ac.SHAPES))
def test_del_n_damping_of_a_state_at_rest(backend, shape, kind):
    """pin 13, the default configuration on five levels (three sponge levels, two regular ones): "mass" a harmonic delp, "fields" harmonic pt, q_con, w over a
    uniform delp and a rotational wind.  "centre" is the closed form (module docstring); no harmonic grows"""
    e = memo(("pin13", backend, shape), lambda: library_rest(backend, shape, kind)) if kind == "fields" else library_rest(backend, shape, kind)
    check_rest(f"d_sw at rest {shape} {kind}", e, REC["pin13"][shape][kind], whole_sphere=shape in ("c24", "c48"))


def test_del_n_damping_without_a_sponge(backend):
    """n_sponge = -1: every level takes the regular (order 2, vtdm4) pair"""
    check_rest("d_sw at rest c24, n_sponge -1", library_rest(backend, "c24", "fields", n_sponge=-1), REC["pin13"]["c24"]["fields_no_sponge"])


def test_fp32_del_n_damping_of_a_state_at_rest(backend32):
    """pin 13 in fp32, C24, the default sponge over nord = 1 (the fp32 context refuses the default order): the one-pass levels (damping_case.ONE_PASS) on
    "centre" within the fp64 bound plus 8 eps32 x the field over the largest exact change (a few roundings of a field of which the call changes 1e-4 ..
    2e-3), "size" within 1.5 x either way with the same allowance.  The order-1 levels change the fields by less than eps32 and are only asked to be finite
    (errors raises otherwise)"""
    for kind in ("fields", "mass"):
        e, rec = library_rest(backend32, "c24", kind, dtype=torch.float32, nord=1), REC["pin13"]["c24"][kind + "_nord1"]
        for key in dm.ONE_PASS:
            if key.startswith("delp") != (kind == "mass"):
                continue  # ("mass" carries the harmonic delp alone, "fields" everything else over a uniform delp)
            extra = 8.0 * EPS32 / rec[key + ".top"]
            got, size = e[key + ".centre"], e[key + ".size"]
            print(f"fp32 {key}: centre {got:.3e} (fp64 oracle {rec[key + '.centre']:.3e}, allowance {extra:.1e}), size {size:.4f} ({rec[key + '.size']:.4f})")
            ac.require(got <= ac.SLACK * rec[key + ".centre"] + extra, f"fp32 {key}.centre: {got:.3e} above 1.5 x {rec[key + '.centre']:.3e} + {extra:.1e}")
            ac.require(rec[key + ".size"] / ac.SLACK - extra <= size <= ac.SLACK * rec[key + ".size"] + extra, f"fp32 {key}.size: {size:.4e} against {rec[key + '.size']:.4e}")


def test_del_n_damping_converges_at_the_tile_centre(backend):
    """pin 15 for pin 13: "centre" reaches two cells from the tile's centre at every resolution, where FV3's operator deviates from the Laplacian as the square of
    the distance; the vorticity's one-pass levels fall by >= 3.5 from C24 to C48 (oracle 4.1), the scalars' by >= 1.8 (oracle 2.4: P_3's own curvature there)"""
    e24, e48 = (memo(("pin13", backend, s), lambda s=s: library_rest(backend, s, "fields")) for s in ("c24", "c48"))
    for key in ("vort.0", "vort.1"):
        ac.check_convergence(f"d_sw at rest {key} centre", e24[key + ".centre"], e48[key + ".centre"])
    for key in ("pt.0", "pt.1", "w.0", "w.1", "w.2"):
        ac.check_convergence(f"d_sw at rest {key} centre", e24[key + ".centre"], e48[key + ".centre"], ratio=1.8)


# ---------------------------------------------------------------------------------------------------------------------------
# pin 14: the damping heat, del2_cubed, apply_diffusive_heating
# ---------------------------------------------------------------------------------------------------------------------------
HELD14 = ("interior", "edge", "corner", "centre")


def check_pin14(label, e, rec):
    check_all(label, e, rec, HELD14)
    check_size(f"{label} size", e["size"], rec["size"])


def library_heat(backend, shape):
    n, layout, ranks = ac.SHAPES[shape]
    part, grids, _, c = ac.make(n, layout, ranks, dm.DAMP_NZ)
    rc = dm.heat_case(grids, c.RADIUS)
    return dm.heat_errors(rc, library_d_sw(backend, shape, dm.heat_config(grids[0], rc.lam), rc.ins, rc.dt, dm.DAMP_NZ))


def heat(backend, shape):
    return memo(("pin14", backend, shape), lambda: library_heat(backend, shape))


@pytest.mark.parametrize("shape", list(ac.SHAPES))
def test_damping_heat_is_the_kinetic_energy_taken(backend, shape):
    """pin 14: d_sw at rest with every damping one pass (nord 0, n_sponge -1), d_con = 1, ke_bg = 0 and a share of 0.2 per call: heat_source == delp [(s - s^2 / 2)
    |V|^2 + s w' (w - s w' / 2)] on "centre" (1.3e-2 at C24, 3.2e-3 at C48); the other classes carry restatement 13 and are held to the record"""
    check_pin14(f"damping heat {shape}", heat(backend, shape), REC["pin14_heat"][shape])


def test_damping_heat_converges_at_the_tile_centre(backend):
    ac.check_convergence("damping heat centre", heat(backend, "c24")["centre"], heat(backend, "c48")["centre"])
    for k in dm.SPONGE_HEAT_LEVELS:
        ac.check_convergence(f"damping heat under the sponge, level {k} centre", sponge_heat(backend, "c24")[f"{k}.centre"], sponge_heat(backend, "c48")[f"{k}.centre"])


def library_sponge_heat(backend, shape):
    n, layout, ranks = ac.SHAPES[shape]
    part, grids, _, c = ac.make(n, layout, ranks, dm.DAMP_NZ)
    rc = dm.heat_case(grids, c.RADIUS)
    return dm.sponge_heat_errors(rc, library_d_sw(backend, shape, dm.sponge_heat_config(), rc.ins, rc.dt, dm.DAMP_NZ))


def sponge_heat(backend, shape):
    return memo(("pin14 sponge", backend, shape), lambda: library_sponge_heat(backend, shape))


def check_sponge_heat(label, e, rec, keys=None):
    assert set(e) == set(rec), set(e) ^ set(rec)
    for k in sorted(e) if keys is None else keys:
        (check_size if k.endswith(".size") else ac.check_bound)(f"{label} {k}", e[k], rec[k])


@pytest.mark.parametrize("shape", list(ac.SHAPES))
def test_damping_heat_under_the_default_sponge(backend, shape):
    """pin 14 with the column's d_con: the default configuration (n_sponge 48, nord 3, d_con = 1, ke_bg = 0) on five levels.  On levels 0 - 2 d_con is off: the
    wind heat is 0 although the wind is damped, and heat_source == s_k w' (w - s_k w' / 2), the heat of w alone, one pass, without the delp weight (FV3 weighs by
    delp inside the block that the level's d_con guards): "centre" 1.1e-2 (C24), 2.9e-3 (C48).  Levels 3 - 4 (order 2, wind heat on) are recorded"""
    check_sponge_heat(f"damping heat under the sponge {shape}", sponge_heat(backend, shape), REC["pin14_sponge_heat"][shape])


def library_del2(backend, shape):
    n, layout, ranks = ac.SHAPES[shape]
    cs = Case(n, layout, ranks, nz=dm.DAMP_NZ, backend=backend)
    d2 = dm.Del2Case(cs.grids, cs.c.RADIUS)
    out = {}
    for nmax in (1, 2, 3):
        Q = cs.q([_pad(x) for x in d2.ins])
        cs.sf.call("del2_cubed", Q.fref, float(d2.cd), nmax)
        _sync(backend)
        out[f"nmax{nmax}"] = d2.errors([Q.numpy(r) for r in range(len(cs.grids))], nmax)
    return out


@pytest.mark.parametrize("shape", list(ac.SHAPES))
def test_del2_cubed_damps_a_harmonic_by_its_eigenvalue(backend, shape):
    """pin 14: fv3_del2_cubed with nmax 1, 2, 3 and cd = 0.2 da_min multiplies the harmonic part by (1 - cd lam)^nmax, on "centre" (1.9e-2 at C24, 9.5e-3 at C48)"""
    e = library_del2(backend, shape)
    for nmax in (1, 2, 3):
        check_pin14(f"del2_cubed {shape} nmax {nmax}", e[f"nmax{nmax}"], REC["pin14_del2"][shape][f"nmax{nmax}"])


def library_heating(backend, shape, dtype=torch.float64):
    n, layout, ranks = ac.SHAPES[shape]
    cs = Case(n, layout, ranks, nz=dm.DAMP_NZ, backend=backend, cfg_kw=dict(nord=1), dtype=dtype)
    cases = [dm.heating_case(ac.Geometry(g), cs.c) for g in cs.grids]
    Q = {k: cs.q([_pad(x[k]) for x, _, _ in cases]) for k in ("delp", "delz", "cappa", "heat_source", "pt")}
    cs.sf.call("apply_diffusive_heating", *[Q[k].fref for k in ("delp", "delz", "cappa", "heat_source", "pt")], dm.HEATING_FACTOR)
    _sync(backend)
    return max(dm.heating_error(ac.Geometry(g), x, want, dpt, Q["pt"].numpy(r)) for r, (g, (x, want, dpt)) in enumerate(zip(cs.grids, cases)))


@pytest.mark.parametrize("shape", ["c24", "c65"])
def test_diffusive_heating_is_the_limited_temperature_change_over_pkz(backend, shape):
    """pin 14: apply_diffusive_heating is pointwise; pt += sign(dT) min(lim_k, |dT|) / pkz with dT = heat / (cv delp), lim = (0.1, 0.5, 1, ..) x the factor and
    pkz from the gas law, to round-off (4 eps |pt| + 32 eps |dpt|), on inputs that put limited and free points of both signs on every level.  This is the staged
    operator; the fused form has no entry of its own and is held bitwise to the staged one inside fv3_acoustic_step by tests/test_parity.py"""
    worst = library_heating(backend, shape)
    print(f"apply_diffusive_heating {shape}: {worst:.3f} of the round-off bound")
    ac.require(worst <= 1.0, f"apply_diffusive_heating {shape}: {worst:.3f} x the round-off bound")


def test_fp32_diffusive_heating_is_the_limited_temperature_change_over_pkz(backend32):
    """the same bound in eps32; the closed form is evaluated in fp64 on the unrounded inputs, whose rounding to fp32 (half an eps32 of pt, less of dpt) the
    bound covers"""
    worst = library_heating(backend32, "c24", dtype=torch.float32)
    print(f"fp32 apply_diffusive_heating c24: {worst:.3f} of the round-off bound")
    ac.require(worst <= 1.0, f"fp32 apply_diffusive_heating: {worst:.3f} x the round-off bound")


# ---------------------------------------------------------------------------------------------------------------------------
# the record, and the controls: every checker has teeth (CPU, oracle only)
# ---------------------------------------------------------------------------------------------------------------------------
def test_control_pin10_divergence_of_the_other_sign_fails():
    n, layout, ranks = ac.SHAPES["c24"]
    part, grids, doms, c = ac.make(n, layout, ranks, ac.DYN_NZ)
    dc = dm.DivergenceCase(grids, c.RADIUS, 3)
    outs = [o["divgd"] for o in dm.oracle_c_sw(doms, dc.ins)]
    check_all("oracle divgd c24", dc.errors(outs), REC["pin10"]["c24"]["l3"], HELD10)
    with pytest.raises(ac.CheckFailed):
        check_all("oracle divgd c24 (+div V)", dc.errors(outs, sign=-1.0), REC["pin10"]["c24"]["l3"], ("interior",))


def test_control_pin11_wrong_way_and_missing_coriolis_fail():
    n, layout, ranks = ac.SHAPES["c24"]
    part, grids, doms, c = ac.make(n, layout, ranks, ac.DYN_NZ)
    cc = dm.CswCase(n, grids, c.RADIUS, c.OMEGA)
    half, zero = dm.oracle_c_sw(doms, cc.ins, cc.dt2), dm.oracle_c_sw(doms, cc.ins, 0.0)
    check_all("oracle c_sw half step c24", cc.errors(half, zero), REC["pin11"]["c24"], HELD11)
    bad = cc.errors(half, zero, way=-1.0)
    for k in dm.CSW_SCALARS:
        with pytest.raises(ac.CheckFailed):
            ac.check_bound(f"oracle c_sw c24 (wrong way) {k}", bad[k], REC["pin11"]["c24"][k])
    cc.rot = 0.0
    bad = cc.errors(half, zero)
    for k in dm.FACE_KEYS.values():
        with pytest.raises(ac.CheckFailed):
            ac.check_bound(f"oracle c_sw c24 (no Coriolis term) {k}", bad[k], REC["pin11"]["c24"][k])


def test_control_pin14_heat_without_the_half_dv_squared_term_fails():
    n, layout, ranks = ac.SHAPES["c24"]
    part, grids, doms, c = ac.make(n, layout, ranks, dm.DAMP_NZ)
    rc = dm.heat_case(grids, c.RADIUS)
    outs = dm.oracle_rest(doms, ac.dyn_config(n, layout, dm.DAMP_NZ, **dm.heat_config(grids[0], rc.lam)), rc)
    check_pin14("oracle damping heat c24", dm.heat_errors(rc, outs), REC["pin14_heat"]["c24"])
    for spoil in ("half", "half_w"):
        with pytest.raises(ac.CheckFailed):
            check_all(f"oracle damping heat c24 ({spoil})", dm.heat_errors(rc, outs, spoil), REC["pin14_heat"]["c24"], ("centre",))


def test_control_pin14_wind_heat_left_on_at_the_sponge_levels_fails():
    """the wind heat left on at the sponge levels (the global d_con for the column's), and the heat of w weighted by delp there"""
    n, layout, ranks = ac.SHAPES["c24"]
    part, grids, doms, c = ac.make(n, layout, ranks, dm.DAMP_NZ)
    rc = dm.heat_case(grids, c.RADIUS)
    outs = dm.oracle_rest(doms, ac.dyn_config(n, layout, dm.DAMP_NZ, **dm.sponge_heat_config()), rc)
    rec = REC["pin14_sponge_heat"]["c24"]
    check_sponge_heat("oracle damping heat under the sponge c24", dm.sponge_heat_errors(rc, outs), rec)
    for spoil, keys in (("wind_on", ("0.centre", "1.centre", "0.size", "1.size")), ("delp", ("0.centre", "1.centre", "2.centre", "2.size"))):
        bad = dm.sponge_heat_errors(rc, outs, spoil)
        for k in keys:
            with pytest.raises(ac.CheckFailed):
                check_sponge_heat(f"oracle damping heat under the sponge c24 ({spoil})", bad, rec, (k,))


def test_control_pin14_one_pass_too_few_and_an_unlimited_heating_fail():
    from fv3_oracle import nh as o_nh

    n, layout, ranks = ac.SHAPES["c24"]
    part, grids, doms, c = ac.make(n, layout, ranks, dm.DAMP_NZ)
    d2 = dm.Del2Case(grids, c.RADIUS)
    qs = [x.copy() for x in d2.ins]
    for D, q in zip(doms, qs):
        o_nh.del2_cubed(D, q, d2.cd, 3)
    check_pin14("oracle del2_cubed c24 nmax 3", d2.errors(qs, 3), REC["pin14_del2"]["c24"]["nmax3"])
    with pytest.raises(ac.CheckFailed):
        check_all("oracle del2_cubed c24 nmax 3 (two passes expected)", d2.errors(qs, 3, "passes"), REC["pin14_del2"]["c24"]["nmax3"], ("centre",))
    G = ac.Geometry(grids[0])
    x, want, dpt = dm.heating_case(G, c)
    pt = x["pt"].copy()
    o_nh.apply_diffusive_heating(doms[0], x["delp"], x["delz"], x["cappa"], x["heat_source"], pt, dm.HEATING_FACTOR)
    assert dm.heating_error(G, x, want, dpt, pt) <= 1.0
    free = x["heat_source"] / (c.CV_AIR * x["delp"]) / (want - x["pt"]) * dpt  # (dT / pkz: the change without its limit)
    assert dm.heating_error(G, x, x["pt"] + free, free, pt) > 1e6


def _oracle_divdamp(run):
    n, layout, ranks = ac.SHAPES["c24"]
    part, grids, doms, c = ac.make(n, layout, ranks, ac.DYN_NZ)
    dc = dm.DivDampCase(n, grids, c.RADIUS, c.OMEGA, l=dm.DIVDAMP_L.get(run, 3))
    on, off = dm.oracle_d_sw_pair(doms, ac.dyn_config(n, layout, **dm.DIVDAMP_RUNS[run]), ac.dyn_config(n, layout), dc)
    return lambda spoil=None: dc.errors(on, off, dm.damp_config(run), spoil)


@pytest.mark.parametrize("run, spoil, key", [("nord1", "exponent", "centre"), ("nord2", "exponent", "centre"), ("nord3", "exponent", "centre"), ("nord0", "da_min", "class2"),
                                             ("smag", "da_min", "class2"), ("nord0_l1", "da_min", "class2"), ("nord1", "sign", "centre"), ("nord3", "sign", "centre")])
def test_control_pin12_wrong_coefficient_fails(run, spoil, key):
    """the exponent n for n + 1, da_min for da_min_c, a (-1)^n put in: the oracle meets its record with the right closed form and misses it with the wrong one"""
    errors = _oracle_divdamp(run)
    check_divdamp(f"oracle {run}", errors(), REC["pin12"]["c24"][run])
    with pytest.raises(ac.CheckFailed):
        check_all(f"oracle {run} ({spoil})", errors(spoil), REC["pin12"]["c24"][run], (key,))


@pytest.mark.parametrize("spoil, keys", [("exponent", ("pt.0.centre", "w.2.centre", "vort.1.centre")), ("half", ("pt.0.centre", "pt.1.centre")),
                                         ("shift", ("pt.1.centre", "w.0.centre", "w.2.centre", "vort.1.centre"))])
def test_control_pin13_wrong_share_fails(spoil, keys):
    """the exponent n for n + 1, the mass-weighted flux without its 1/2, the sponge table one level down -- on the one-pass (order 0) levels, where "centre" is
    a closed-form pin; the order-2 levels' 0.51 is none (module docstring)"""
    n, layout, ranks = ac.SHAPES["c24"]
    part, grids, doms, c = ac.make(n, layout, ranks, dm.DAMP_NZ)
    rc = dm.RestCase(grids, c.RADIUS, "fields")
    outs = dm.oracle_rest(doms, dm.rest_config(n, layout), rc)
    check_rest("oracle d_sw at rest c24", rc.errors(outs), REC["pin13"]["c24"]["fields"])
    bad = rc.errors(outs, spoil=spoil)
    for k in keys:
        with pytest.raises(ac.CheckFailed):
            ac.check_bound(f"oracle d_sw at rest c24 ({spoil}) {k}", bad[k], REC["pin13"]["c24"]["fields"][k])
