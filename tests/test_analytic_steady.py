"""The whole acoustic call (fv3_acoustic_step) and the whole model step (DynamicalCore.step_dynamics) on steady analytic atmospheres (builders, exact solutions, checkers,
oracle measurement and the poison list: tests/steady_case.py), continuing tests/test_analytic_pins.py, test_analytic_dynamics.py and test_analytic_damping.py, which hold
the operators one at a time, under the same ground rule: inputs and expected values come from corner positions, cell centres, the sphere radius, the hybrid coefficients
and closed-form functions of position; no metric array that a kernel reads enters either (pin 17's Courant number times the upwind area is pin 6's stated exception).
What sits between the operators is what these pins hold: which dt each stage gets, the signs and factors with which gz, pkc, pk3 and pp go from the height chain and the
Riemann solvers to the pressure-gradient operators, set_gz / compute_geopotential, the accumulators over several sub-steps, the thermodynamic bookends, the remap as the identity.

State A: isothermal (300 K) solid-body rotation over flat ground in gradient-wind balance, ln ps = ln p0 - (a OMEGA U0 (axis . z) + U0^2 / 2) s^2 / (R T0), about the z axis
with the project's constants (A-z) and about analytic_case.AXIS on a planet that does not turn (A-oblique: OMEGA = 0 in the constants of the grids, the oracle's domains and
the stencil factory).  State B: the same atmosphere at rest over analytic_case.terrain.  delz = -(R T0 / g) d ln pe, pt = T0 / pm^kappa: the Riemann solvers' own equilibrium.
Every damping term off (DSW_OFF, n_sponge = -1, no rf_fast), 8 levels (16 in the refined pair), sub-step dt = analytic_case.dyn_dt: Courant number 0.1 at C24, falling as 1 / n.

  16  one acoustic call, n_split = 3 (and 1 at C24), A-z and A-oblique   max |x_after - x_before| / (n_split dt): the winds per class of faces (analytic_case.face_classes, and
                    "core": a quarter of the tile or more from every tile edge) over max |(zeta + f) V|; delp, pt, delz over max |x| U0 / a; w over U0^2 / a
  17  the accumulators of that call   mfxd, mfyd == n_split delp(face mid-point) x the exact swept area; cxd, cyd x the upwind area == n_split x the swept area
  18  step_dynamics, two steps, k_split = 2, n_split = 2, remap, temperature, latlon winds, hord_tr = 8, A-oblique   pt == T0, ps and delp == dak + dbk ps, w == omga == 0,
                    pkz == pm^kappa, ua / va == the eastward / northward wind, three tracers (a constant, q0 (1 + P2(s) / 2), that times a profile linear in pressure) unchanged
  19  three acoustic calls of n_split = 2 on state B   max |u|, |v|, |w| / (6 dt): the spurious acceleration over a 3 km mountain; delp, pt unchanged
  poison            two calls at c24_2x2 with NaN over every workspace field and over the state fields the sequence stores before it reads (steady_case.POISON_STATE, derived
                    from the oracle): the prognostic outputs bitwise those of the clean run

Thresholds; nothing is fitted to the library.  Every figure <= 1.5 x the numpy oracle's on the same input (tests/golden/analytic_pins.json, ``python tests/analytic_case.py
--record steady``, half a minute on the CPU); c48_2x2 is held to the whole tile's figures; pin 19's delp and pt to the oracle's figure itself (x (1 + 1e-6)); the constant tracer
to 1e-13 as pin 2.  Second order (error(C24) / error(C48) >= 3.5) is asserted for every figure and pair of which the record shows a ratio >= 3.6, C65 <= C48 for every figure for
which the record shows it, pin 19's ratio only from 3.8 (the record shows 2.4 .. 3.2: printed, not asserted).  fp32 (C24, pins 16 and 18): the fp64 bound plus 64 eps32 max |x| /
(n_split dt), one storing of the field.  pt of pin 16 is the one figure below 1e3 eps32 max |x| / (n_split dt) in the fp64 record; its K (8 x the smallest integer with which the
fp64 oracle meets K eps64 S, recorded as fp32_K) is 7.5e9 / 1.6e11, because the fp64 figure is a truncation error and not a rounding: K eps32 S is looser than the first bound by
nine orders, so both are asserted and the first one binds.

Which pair is asserted, and why.  The wind tendency of the core faces is 1.27e-2 (C24 L8), 1.39e-2 (C48 L8), 1.42e-2 (C65 L8) about z and 1.18e-2, 1.03e-2, 1.03e-2 about the
oblique axis: the horizontal-only ratio (0.92 / 1.15) stalls on the vertical truncation of the pressure-gradient bracket on isothermal columns.  On the pair C24 L8 -> C48 L16 it is
3.63 / 4.41, and that pair is asserted (the test fails if the record stops showing it).  Outside the core no figure of pin 16 converges: the tile-edge kinetic-energy term of pin 7
(restatement 12; class 1 grows as 1 / dx) is carried inwards by the sound waves of three sub-steps -- class 2+ is 1.9e-2 / 4.3e-2 after one sub-step at C24 and
2.8e-2 / 0.30 after three -- and delp, w and the edge classes grow with resolution.  This is DESIGN.md section 2, restatement 15, held by the record; no arithmetic was changed.

Controls (CPU, oracle only), each asserting that the same checker raises CheckFailed: A-z with the Coriolis term left out of ps; the wind turned the other way under the same ps
(A-oblique: the balance is quadratic in V without Coriolis, so pin 16 cannot see it and pin 17's checker raises on all four accumulators; A-z: pin 16's raises); delz x 1.03 (w's
figure after one sub-step, delz's after three: by then the implicit solver has brought w back); pin 17 against n_split - 1; pin 18 with T0 handed in as the loop's pt.

Measured (fp64).  Oracle, host emulation and MI355X agree to the five digits printed on every figure of every pin.  Pin 16, A-z at C24 / C48 / C65 / C48 L16: class 0 0.103 / 0.216 /
0.307 / 0.216, class 1 0.107 / 0.235 / 0.326 / 0.222, second line 5.5e-2 / 3.4e-2 / 3.4e-2 / 2.4e-2, class 2+ 2.8e-2 / 3.0e-2 / 2.9e-2 / 1.9e-2, core as above with 3.5e-3 at C48 L16,
delp 4.0e-2 / 7.6e-2 / 0.10 / 7.6e-2, pt 3.2e-4 / 2.0e-4 / 1.5e-4 / 1.7e-4, delz 4.6e-2 / 3.4e-2 / 3.9e-2 / 3.9e-2, w 1.0e-2 / 9.0e-2 / 0.22 / 0.10.  A-oblique (the balance term is
13 times smaller without Coriolis): class 0 2.06 / 4.57 / 6.44, class 1 2.06 / 4.47 / 6.29, second line 0.68 / 0.51 / 0.53, class 2+ 0.30 / 0.40 / 0.36, core 2.7e-3 at C48 L16, delp
7.0e-2 / 0.14 / 0.16, pt 1.5e-5 / 8.7e-6 / 6.5e-6, delz 6.4e-2 / 5.4e-2 / 6.4e-2, w 1.9e-2 / 0.14 / 0.33.  Pin 17, mfx = mfy and cx = cy to six digits: A-z 2.2e-3, 3.3e-3 (C24), 1.3e-3,
1.5e-3 (C48), 1.1e-3, 1.2e-3 (C65), ratios 1.66 and 2.25; A-oblique 2.6e-3, 2.9e-3, then 2.2e-3, 2.4e-3, then 1.9e-3, 2.0e-3, ratios 1.16 and 1.22; none asserted.  Pin 18 at C24 / C48: pt 3.8e-3 /
4.8e-4 (ratio 7.8, asserted), tracers 1 and 2 2.5e-3 / 6.5e-4 (3.77, asserted), ps 2.6e-3 / 1.7e-3, delp 3.1e-3 / 2.1e-3, pkz 1.0e-3 / 4.9e-4, w 9.5e-4 / 4.3e-4 U0, omga 7.8e-5 / 9.8e-5,
ua 0.106 / 3.1e-2 and va 9.4e-2 / 3.0e-2 of U0 (ratios 3.48 and 3.16: not asserted), the constant tracer 1.1e-15 / 1.3e-15; on the default damping pt 4.9e-3 / 4.8e-4, ua 5.0e-2 / 2.8e-2.
Pin 19 at C24 L8 / C48 L16: u 1.61e-4 / 6.8e-5 m/s^2, v 1.71e-4 / 6.7e-5, w 2.8e-6 / 8.9e-7 (ratios 2.38, 2.55, 3.18), delp 4.0e-3 / 9.8e-5, pt 2.5e-5 / 5.0e-7.
fp32 at C24, host emulation / MI355X against the fp64 oracle: pin 16 A-z core 1.2729e-2 / 1.2728e-2 (1.2728e-2), pt 3.247e-4 / 3.249e-4 (3.229e-4), w 1.0225e-2 / 1.0216e-2 (1.0183e-2);
A-oblique core 1.191e-2 / 1.205e-2 (1.183e-2), pt 2.15e-5 / 2.15e-5 (1.51e-5), class 2+ 0.2912 / 0.2903 (0.2971); pin 18 within 3 % of the fp64 figures on both, the constant tracer
6.3e-7 (bound 1e-13 + 64 eps32 = 7.6e-6).  The poison run is bitwise the clean run on both backends.
No pin failed on its first run on either backend.  Of the controls, "delz x 1.03 against w's figure after three sub-steps" did not raise on its first run (2.5e-2 against 1.5 x
1.9e-2); it is asserted on the one-sub-step run and, after three, on delz's figure.
"""
import numpy as np
import pytest
import torch

import analytic_case as ac
import steady_case as sc
from test_analytic_pins import backend32, memo  # noqa: F401  (backend32 is a fixture)

REC = ac.recorded()
EPS32 = float(np.finfo(np.float32).eps)
SHOWS = 3.6  # a recorded ratio at or above this "shows second order"; the library is then held to ac.RATIO (3.5)
WITHIN = 1.0 + 1.0e-6  # "within the oracle's figure": to the six digits at which the two agree
WHOLE = {"c48_2x2": "c48"}  # the 2 x 2 ranks are held to the whole tile's figures
RUNS = dict(sc.PIN16_RUNS, c48_2x2=("c48_2x2", sc.NZ, sc.N_SPLIT))
PAIRS = {"ratio_c24_c48": ("c24", "c48"), "ratio_c24_c48_l16": ("c24", "c48_l16")}


def _rec(pin, which, run):
    return REC[pin][which][WHOLE.get(run, run)]


# ---------------------------------------------------------------------------------------------------------------------------
# pins 16 and 17: one acoustic call on states A-z and A-oblique
# ---------------------------------------------------------------------------------------------------------------------------
def acoustic_call(backend, which, run, dtype=torch.float64):
    def measure():
        shape, nz, n_split = RUNS[run]
        case = sc.SteadyCase(shape, nz, which)
        assert abs(case.dt - _rec("pin16", which, run)["dt"]) <= 1e-12 * case.dt
        outs = sc.library_call(backend, case, sc.config_for(shape, nz, n_split), dtype=dtype)
        return case, case.tendencies(outs, n_split), case.accumulator_errors(outs, n_split)

    return memo(("pin16", backend, which, run, dtype), measure)


def check_figures(label, fig, rec, keys, addend=None, slack=ac.SLACK):
    for k in keys:
        a = 0.0 if addend is None else addend[k]
        print(f"{label} {k}: {fig[k]:.4e}, oracle {rec[k]:.4e}" + (f", fp32 addend {a:.2e}" if addend else ""))
        ac.require(np.isfinite(fig[k]) and fig[k] <= slack * rec[k] + a, f"{label} {k}: {fig[k]:.4e} above {slack} x the oracle's {rec[k]:.4e} + {a:.2e}")


def check_recorded_convergence(label, rec, fig_of, must=()):
    """second order asserted for every figure and pair of which the oracle's record shows it; ``must``: (pair, figure) that the record has to show"""
    shown = [(pair, k) for pair in PAIRS for k, ratio in rec[pair].items() if ratio >= SHOWS]
    for m in must:
        ac.require(m in shown, f"{label}: the record no longer shows second order for {m}")
    for pair, k in shown:
        coarse, fine = PAIRS[pair]
        ac.check_convergence(f"{label} {k} {coarse} -> {fine}", fig_of(coarse)[k], fig_of(fine)[k])
    for pair in PAIRS:
        print(f"{label} {pair}, recorded:", {k: round(v, 2) for k, v in rec[pair].items()})
    return shown


@pytest.mark.parametrize("run", list(RUNS))
@pytest.mark.parametrize("which", list(sc.AXES))
def test_one_acoustic_call_keeps_the_balanced_rotation(backend, which, run):
    """pin 16: n_split = 3 on every shape (a first, a middle and a last sub-step), n_split = 1 at C24, and C48 with 16 levels"""
    case, fig, _ = acoustic_call(backend, which, run)
    check_figures(f"acoustic call {which} {run}", fig, _rec("pin16", which, run), sc.PIN16_FIGURES)


@pytest.mark.parametrize("which", list(sc.AXES))
def test_the_balanced_rotation_converges_where_the_record_shows_it(backend, which):
    """the wind tendency of the core faces from C24 L8 to C48 L16 (the pair asserted: at 8 levels the ratio stalls on the vertical truncation of the pressure-gradient
    bracket), and every other figure and pair of which the record shows second order; C65 is no worse than C48 on the figures on which the oracle's is not"""
    rec = REC["pin16"][which]
    check_recorded_convergence(f"acoustic call {which}", rec, lambda run: acoustic_call(backend, which, run)[1], must=[("ratio_c24_c48_l16", "core")])
    f48, f65 = acoustic_call(backend, which, "c48")[1], acoustic_call(backend, which, "c65")[1]
    for k in sc.PIN16_FIGURES:
        if rec["c65"][k] <= rec["c48"][k]:
            ac.require(f65[k] <= f48[k], f"acoustic call {which} {k}: C65's {f65[k]:.3e} above C48's {f48[k]:.3e}")


@pytest.mark.parametrize("run", list(RUNS))
@pytest.mark.parametrize("which", list(sc.AXES))
def test_the_call_accumulates_n_split_times_the_exact_mass_flux(backend, which, run):
    """pin 17: the first-sub-step store, the once-per-call sum and the read-modify-write form against one closed-form number"""
    _, _, fig = acoustic_call(backend, which, run)
    check_figures(f"accumulators {which} {run}", fig, _rec("pin17", which, run), ("mfx", "mfy", "cx", "cy"))


@pytest.mark.parametrize("which", list(sc.AXES))
def test_the_accumulators_converge_where_the_record_shows_it(backend, which):
    check_recorded_convergence(f"accumulators {which}", REC["pin17"][which], lambda run: acoustic_call(backend, which, run)[2])


@pytest.mark.parametrize("which", list(sc.AXES))
def test_fp32_one_acoustic_call_keeps_the_balanced_rotation(backend32, which):
    """C24 in fp32: the fp64 bounds plus 64 eps32 max |x| / (n_split dt).  A figure that the record lists under fp32_K (below 1e3 eps32 max |x| / (n_split dt) in fp64) is
    also held to K eps32 max |x| / (n_split dt); the K of a truncation error is large, so it is the first bound that binds (module docstring)."""
    case, fig, acc = acoustic_call(backend32, which, "c24", torch.float32)
    scale = case.store_scale(sc.N_SPLIT)
    check_figures(f"fp32 acoustic call {which} c24", fig, _rec("pin16", which, "c24"), sc.PIN16_FIGURES, {k: 64.0 * EPS32 * v for k, v in scale.items()})
    for k, K in REC["pin16"][which]["fp32_K"].items():
        print(f"fp32 acoustic call {which} c24 {k}: K = {K}, K eps32 S = {K * EPS32 * scale[k]:.3e}")
        ac.require(fig[k] <= K * EPS32 * scale[k], f"fp32 acoustic call {which} c24 {k}: {fig[k]:.4e} above K eps32 S = {K * EPS32 * scale[k]:.3e}")


# ---------------------------------------------------------------------------------------------------------------------------
# pin 18: DynamicalCore.step_dynamics on state A-oblique
# ---------------------------------------------------------------------------------------------------------------------------
CONSTANT_TRACER = 1.0e-13  # as pin 2


def model_steps(backend, variant, shape, dtype=torch.float64):
    def measure():
        case = sc.StepCase(shape)
        assert abs(case.dt - REC["pin18"][variant][shape]["dt"]) <= 1e-12 * case.dt
        return case.step_errors(*sc.library_step(backend, case, damping=variant == "default", dtype=dtype))

    return memo(("pin18", backend, variant, shape, dtype), measure)


def check_step(label, fig, rec, addend=0.0):
    check_figures(label, fig, rec, [k for k in sc.STEP_FIGURES if k != "tracer0"], dict.fromkeys(sc.STEP_FIGURES, addend) if addend else None)
    print(f"{label} tracer0: {fig['tracer0']:.3e}")
    ac.require(fig["tracer0"] <= CONSTANT_TRACER + addend, f"{label}: the constant tracer is off by {fig['tracer0']:.3e}")


@pytest.mark.parametrize("shape", ["c24", "c48"])
def test_two_model_steps_return_the_steady_state(backend, shape):
    """pin 18, every damping term off: k_split = 2, n_split = 2, remap, temperature bookends, latlon winds, hord_tr = 8, three tracers"""
    check_step(f"step_dynamics {shape}", model_steps(backend, "off", shape), REC["pin18"]["off"][shape])


def test_two_model_steps_converge_where_the_record_shows_it(backend):
    rec = REC["pin18"]["off"]
    shown = check_recorded_convergence("step_dynamics", {"ratio_c24_c48": rec["ratio_c24_c48"], "ratio_c24_c48_l16": {}}, lambda run: model_steps(backend, "off", run),
                                       must=[("ratio_c24_c48", "pt"), ("ratio_c24_c48", "tracer1"), ("ratio_c24_c48", "tracer2")])
    assert shown


@pytest.mark.parametrize("shape", ["c24", "c48"])
def test_two_model_steps_on_the_default_damping_stay_with_the_oracle(backend, shape):
    """PARITY, not a closed-form pin: the default configuration (sponge, d_con, vtdm4, rf_fast) damps the rotation, so the figures are held to the oracle's record alone.
    Its value is that the default sequencer forms run on a state whose answer is "almost nothing"."""
    check_step(f"step_dynamics, default damping, {shape}", model_steps(backend, "default", shape), REC["pin18"]["default"][shape])


def test_fp32_two_model_steps_return_the_steady_state(backend32):
    """C24 in fp32: the fp64 bounds plus 64 eps32 of each figure's scale"""
    check_step("fp32 step_dynamics c24", model_steps(backend32, "off", "c24", torch.float32), REC["pin18"]["off"]["c24"], 64.0 * EPS32)


# ---------------------------------------------------------------------------------------------------------------------------
# pin 19: state B through three calls
# ---------------------------------------------------------------------------------------------------------------------------
def rest(backend, run):
    def measure():
        shape, nz = sc.REST_RUNS[run]
        case = sc.SteadyCase(shape, nz, "terrain")
        assert abs(case.dt - REC["pin19"][run]["dt"]) <= 1e-12 * case.dt
        return case.rest_figures(sc.library_call(backend, case, sc.config_for(shape, nz, sc.REST_N_SPLIT), sc.REST_CALLS), sc.REST_N_SPLIT, sc.REST_CALLS)

    return memo(("pin19", backend, run), measure)


def check_rest(label, fig, rec):
    check_figures(label, fig, rec, ("u", "v", "w"))
    check_figures(label, fig, rec, ("delp", "pt"), slack=WITHIN)


@pytest.mark.parametrize("run", list(sc.REST_RUNS))
def test_the_atmosphere_at_rest_over_terrain_stays_at_rest(backend, run):
    """pin 19: the spurious acceleration over a 3 km mountain, three calls of n_split = 2; C24 L8 and C48 L16"""
    check_rest(f"rest over terrain {run}", rest(backend, run), REC["pin19"][run])


def test_the_spurious_acceleration_over_terrain_falls_with_the_grid(backend):
    """asserted only where the record shows a ratio >= 3.8 (it shows 2.4 for the winds: recorded, not asserted)"""
    ratio = REC["pin19"]["ratio_c24_c48_l16"]
    for k in ("u", "v", "w"):
        coarse, fine = rest(backend, "c24")[k], rest(backend, "c48_l16")[k]
        print(f"rest over terrain {k}: {coarse:.3e} / {fine:.3e} = {coarse / fine:.2f}, recorded {ratio[k]:.2f}")
        if ratio[k] >= 3.8:
            ac.check_convergence(f"rest over terrain {k}", coarse, fine, ratio=3.8)


# ---------------------------------------------------------------------------------------------------------------------------
# the poison
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_poison_list_is_the_oracles():
    assert sc.derive_poison_list() == sc.POISON_STATE


def test_the_call_reads_nothing_it_has_not_been_given(backend):
    """two calls (n_map 1, 2) of n_split = 3 at c24_2x2; before each, NaN over every workspace field and over the state fields the sequence stores before it reads"""
    case = sc.SteadyCase(sc.POISON_SHAPE, sc.NZ, "oblique")
    cfg = sc.config_for(sc.POISON_SHAPE, sc.NZ, sc.N_SPLIT)
    clean = sc.library_call(backend, case, cfg, sc.POISON_CALLS)
    spoiled = sc.library_call(backend, case, cfg, sc.POISON_CALLS, before_call=sc.library_poison)
    what = sc.same_prognostics(case, spoiled, clean)
    assert what is None, what
    assert max(np.abs(clean[0]["mfxd"]).max(), np.abs(clean[0]["mfyd"]).max()) > 0.0


# ---------------------------------------------------------------------------------------------------------------------------
# freshness
# ---------------------------------------------------------------------------------------------------------------------------
def test_recorded_oracle_figures_are_fresh():
    """the C24 entries of pins 16, 17 and 19 measured again with the oracle: the json is stale if any differs by more than 1 %"""
    now = sc.measure_steady(only_c24=True)
    pairs = [(f"{pin} {which} {run} {k}", v, REC[pin][which][run][k]) for pin in ("pin16", "pin17") for which in sc.AXES for run, fig in now[pin][which].items() for k, v in fig.items()]
    pairs += [(f"pin19 {run} {k}", v, REC["pin19"][run][k]) for run, fig in now["pin19"].items() for k, v in fig.items()]
    assert len(pairs) > 50
    stale = [(label, v, r) for label, v, r in pairs if abs(v - r) > 0.01 * abs(r)]
    assert not stale, stale


# ---------------------------------------------------------------------------------------------------------------------------
# the controls: every checker has teeth (CPU, oracle only)
# ---------------------------------------------------------------------------------------------------------------------------
def _oracle_pin16(which, n_split=sc.N_SPLIT, **spoil):
    _, _, p16, p17 = sc.measure_pin16_17("c24", which, sc.NZ, n_split, **spoil)
    return p16, p17


def test_control_pin16_surface_pressure_without_the_coriolis_term_fails():
    check_figures("oracle, A-z", _oracle_pin16("z")[0], REC["pin16"]["z"]["c24"], sc.PIN16_FIGURES)
    with pytest.raises(ac.CheckFailed):
        check_figures("oracle, A-z (no Coriolis term in ps)", _oracle_pin16("z", coriolis=False)[0], REC["pin16"]["z"]["c24"], ("core",))


def test_control_pin16_wind_turned_the_other_way_fails():
    """A-oblique under the same ps: on a planet that does not turn the balance is quadratic in V, so -V is as steady as V and pin 16's figures cannot tell them apart;
    pin 17's do (the mass crosses every face the other way).  On A-z the Coriolis term makes the turned wind unbalanced, and pin 16's checker raises too."""
    p16, p17 = _oracle_pin16("oblique")
    check_figures("oracle, A-oblique", p16, REC["pin16"]["oblique"]["c24"], sc.PIN16_FIGURES)
    check_figures("oracle, A-oblique", p17, REC["pin17"]["oblique"]["c24"], ("mfx", "mfy", "cx", "cy"))
    for k in ("mfx", "mfy", "cx", "cy"):
        with pytest.raises(ac.CheckFailed):
            check_figures("oracle, A-oblique (wind turned)", _oracle_pin16("oblique", way=-1.0)[1], REC["pin17"]["oblique"]["c24"], (k,))
    with pytest.raises(ac.CheckFailed):
        check_figures("oracle, A-z (wind turned)", _oracle_pin16("z", way=-1.0)[0], REC["pin16"]["z"]["c24"], ("core",))


def test_control_pin16_stretched_layers_fail():
    """delz x 1.03: after one sub-step (the C24 n_split = 1 run) w's figure is 8.05 against a bound of 1.5 x 6.7e-3.  After three the implicit solver has brought the
    columns back and w with them (2.5e-2 against 1.5 x 1.9e-2: w's figure alone would pass); what it has undone is then delz's figure, 2.2 against 1.5 x 6.4e-2."""
    with pytest.raises(ac.CheckFailed):
        check_figures("oracle, A-oblique, n_split 1 (delz x 1.03)", _oracle_pin16("oblique", 1, delz_factor=1.03)[0], REC["pin16"]["oblique"]["c24_n1"], ("w",))
    with pytest.raises(ac.CheckFailed):
        check_figures("oracle, A-oblique (delz x 1.03)", _oracle_pin16("oblique", delz_factor=1.03)[0], REC["pin16"]["oblique"]["c24"], ("delz",))


def test_control_pin17_one_sub_step_less_fails():
    case = sc.SteadyCase("c24", sc.NZ, "oblique")
    outs = sc.oracle_call(case, sc.config_for("c24", sc.NZ, sc.N_SPLIT))
    keys = ("mfx", "mfy", "cx", "cy")
    check_figures("oracle accumulators", case.accumulator_errors(outs, sc.N_SPLIT), REC["pin17"]["oblique"]["c24"], keys)
    for k in keys:
        with pytest.raises(ac.CheckFailed):
            check_figures("oracle accumulators (n_split - 1)", case.accumulator_errors(outs, sc.N_SPLIT - 1), REC["pin17"]["oblique"]["c24"], (k,))


def test_control_pin18_skipped_bookend_fails():
    case = sc.StepCase("c24")
    check_step("oracle step_dynamics", case.step_errors(*sc.oracle_step(case)), REC["pin18"]["off"]["c24"])
    with pytest.raises(ac.CheckFailed), np.errstate(all="ignore"):  # (300 as the loop's pt is 8000 K: the columns do not survive it, and the checker says "non-finite")
        check_figures("oracle step_dynamics (T0 as the loop's pt)", case.step_errors(*sc.oracle_step(case, skip_bookend=True)), REC["pin18"]["off"]["c24"], ("pt",))
