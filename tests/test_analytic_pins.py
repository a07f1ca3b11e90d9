"""The transport, wind and pressure-gradient kernels against analytic solutions (builders, exact solutions and checkers: tests/analytic_case.py).
Every other GPU test of the numerics compares a kernel with the oracle, so an error the two share passes; nothing below needs the oracle at run
time.  Inputs and expected values are built from the corner positions, the cell centres, the sphere radius and closed-form functions of position
only -- no metric term a kernel reads enters an expected value (area weights the norms of pin 2; the Courant number handed to the tracer advection is
the stated exception, which the operator multiplies back).  The flow is solid-body rotation once round in 12 days.

  1   fxadv         x_area_flux / y_area_flux == dt (psi(B) - psi(A)), the stream-function difference of a face's two corners
  2   tracer_2d_1l  a cosine bell, a Gaussian and a constant (three tracers: the pair march and the single march) carried once round the sphere on
                    the exact fluxes; level 0 rides a great circle obliquely through cube corners, level 1 turns about the z axis through four tile edges
  3   c_sw, dt2 = 0 the D-to-C wind conversion (d2a2c_vect) against the analytic covariant components, the edge normal on tile-edge faces
  4   a2b_ord4      a smooth function from the cell centres to the corners: interior, tile-edge and cube corners apart
  5a  nh_p_grad, p_grad_c   no force on an isentropic atmosphere at rest over a 3 km mountain (gz linear in pk3, pp linear in gz: every four-point
                    bracket cancels), against a control state (isothermal gz) on which the same call moves the wind
  5b  remap         tracers and D-grid winds linear in pressure on random non-uniform Lagrangian layers come back linear in pressure

Thresholds; nothing is fitted to the library.  Pins 1 - 4: error(C24) / error(C48) >= 3.5 (second order gives 4; for pin 2 this is the l2 error of every
tracer, level and hord -- the linf error of the monotone scheme at a clipped peak falls more slowly, 3.0 for the oracle's bell, and is held by the bound
alone), and error <= 1.5 x what the numpy oracle gives on the same input, read from tests/golden/analytic_pins.json
(``python tests/analytic_case.py --record``, CPU only); C65's error does not exceed C48's.  test_recorded_oracle_figures_are_fresh re-measures the C24
entries and fails if the file is stale by more than 1 %.  Pin 2 in fp64: tracer mass to 1e-12, the constant to 1e-13, hord 8 within 0 .. the initial
maximum (at Courant number 0.5; with two sub-cycles the oracle itself leaves -3.8e-17), hord 6's undershoot within 1.5 x the oracle's, n_split as
recorded.  Pin 5a: max |du| on the isentropic state <= 1e-9 x that on the control state.  Pin 5b: 1e-13 x the profile's range.
fp32 (pin 2, C24, hord 8): the l2 / linf bounds unchanged (truncation error >= 1e-2 dominates), mass and the constant to 8 eps32 n_calls (a few roundings
per call, accumulating linearly at worst).  Pin 5a in fp32: K eps32 S, S = dt rdx max|gz| max|delta_k pk3| / min(delta_k pk3 pair), K = 8 x the smallest
integer with which the fp64 oracle meets K eps64 S (recorded: K = 8).

Pin 5b leaves w out: the remap's profile for w (iv = -2, FV3's cs_profile) solves its edge values with the uniform-grid weights 3 (a[k-1] + a[k]) and the
top closure q = 1.5 a[0], so it does not reproduce a profile linear in pressure on non-uniform layers (the oracle's remap_column: 3e-2 of the range;
iv = -1, 0, 1, 2 are exact to 1e-15).  u / v (iv = -1) are exact and are tested against the edge-averaged pressure.

The C48 revolution (384 calls) takes about 10 s on the host emulation, so every parametrisation runs in the CPU suite too.

Controls (CPU, oracle only), each asserting that the same checker raises: pin 1 with sin_sg1 / sin_sg3 exchanged, pin 4 with edge_w x 1.05, pin 2 against the
solution turned the wrong way, pin 5a's control state, pin 5b on a quadratic profile.

Measured, host emulation and MI355X alike (fp64): every error of pins 1 - 4 equals the oracle's recorded figure to the five digits printed (fxadv C24 3.9931e-04,
C48 1.0649e-04, ratio 3.75; d2a2c 1.4592e-03, 3.6177e-04, 4.03; a2b_ord4 2.6427e-03, 6.4713e-04, 4.08; the bell's l2 ratios 3.90 .. 7.40); crx x the upwind area
against x_area_flux 3.6e-16 .. 3.9e-16; tracer mass 1.1e-14 .. 2.2e-14, the constant exactly 1; hord 6 undershoot -3.1e-02 (C24), -1.0e-02 (C48), as the oracle's;
pin 5a 3.7e-15 (nh_p_grad) and 2.2e-19 (p_grad_c) against controls of 2.9e-02 and 2.8e-05; pin 5b 1.8e-15 .. 8.9e-15 of ranges 3 .. 27.  fp32 bell: l2 / linf as
fp64 to four digits, tracer mass 9.2e-07 .. 9.5e-07 against 8 eps32 x 192 = 1.8e-04, the constant exactly 1.  No pin failed on its first run.
"""
import os

import numpy as np
import pytest
import torch

import analytic_case as ac
from helpers import DIMS3, Case
from pace_amd.constants import get_constants

REC = ac.recorded()
EPS32 = float(np.finfo(np.float32).eps)
KAPPA = get_constants().KAPPA


@pytest.fixture(params=["hostemu", pytest.param("hip:gfx950", marks=pytest.mark.gpu)])
def backend32(request):
    """The fp32 library: its host emulation (CPU suite) or the HIP build (-m gpu)."""
    from pace_amd import build, lib

    if request.param == "hostemu":
        build.build(32, hostemu=True, verbose=False)
    else:
        request.getfixturevalue("gpu_backend")
        if not os.path.exists(build.lib_path(32)):
            build.build(32)
        lib.load(32)
    return request.param


def _sync(backend):
    if backend != "hostemu":
        torch.cuda.synchronize()


NZ = 3  # the context's fewest levels; the pins fill two (the bell) or copy one field onto all of them


def _pad(a, depth=None):
    """to the storage's nz + 1 levels (or ``depth``) by repeating the last one"""
    depth = a.shape[2] + 1 if depth is None else depth
    return np.concatenate([a] + [a[:, :, -1:]] * (depth - a.shape[2]), axis=2)


def _case(shape, backend, nz=NZ, cfg_kw=None, dtype=torch.float64):
    n, layout, ranks = ac.SHAPES[shape]
    return Case(n, layout, ranks, nz=nz, backend=backend, cfg_kw=cfg_kw, dtype=dtype)


_MEMO = {}


def memo(key, fn):
    """one measurement per (pin, backend, shape), shared by the bound, the convergence and the C65 tests"""
    if key not in _MEMO:
        _MEMO[key] = fn()
    return _MEMO[key]


# ---------------------------------------------------------------------------------------------------------------------------
# pin 1: fxadv
# ---------------------------------------------------------------------------------------------------------------------------
def library_flux_errors(backend, shape):
    cs = _case(shape, backend)
    flow = ac.Flow(cs.c.RADIUS)
    dt = REC["pin1"][shape]["dt"]
    fc = ac.flux_case(cs.grids, flow, cs.nz)
    uc, vc = cs.q([_pad(x[1]) for x in fc]), cs.q([_pad(x[2]) for x in fc])
    out = {k: cs.q() for k in ("crx", "cry", "xfx", "yfx", "ut", "vt")}
    cs.sf.call("fxadv", uc.fref, vc.fref, *[out[k].fref for k in ("crx", "cry", "xfx", "yfx", "ut", "vt")], dt)
    _sync(backend)
    R = range(len(cs.grids))
    got = {k: [out[k].numpy(r)[:, :, : cs.nz] for r in R] for k in ("crx", "cry", "xfx", "yfx")}
    e_all, e_edge = ac.flux_errors(fc, flow, dt, got["xfx"], got["yfx"])
    top = max(max(np.abs(got["crx"][r][G.X]).max(), np.abs(got["cry"][r][G.Y]).max()) for r, (G, _, _) in enumerate(fc))
    metric = max(ac.courant_consistency(g, got["crx"][r], got["cry"][r], got["xfx"][r], got["yfx"][r]) for r, g in enumerate(cs.grids))
    return {"all": e_all, "edge": e_edge, "courant": float(top), "metric": metric}


def flux_errors(backend, shape):
    return memo(("pin1", backend, shape), lambda: library_flux_errors(backend, shape))


@pytest.mark.parametrize("shape", list(ac.SHAPES))
def test_area_fluxes_are_the_stream_function_differences(backend, shape):
    """every compute face, the tile-edge faces and those next to cube corners included; the largest Courant number is about 0.5"""
    e = flux_errors(backend, shape)
    assert 0.4 <= e["courant"] <= 0.6, e
    ac.check_bound(f"fxadv {shape} all faces", e["all"], REC["pin1"][shape]["all"])
    ac.check_bound(f"fxadv {shape} tile-edge faces", e["edge"], REC["pin1"][shape]["edge"])
    print(f"crx x upwind (dxa dy sin_sg) against x_area_flux: {e['metric']:.2e}")
    assert e["metric"] <= 1e-14, e


def test_area_fluxes_converge_at_second_order(backend):
    ac.check_convergence("fxadv", flux_errors(backend, "c24")["all"], flux_errors(backend, "c48")["all"])
    ac.require(flux_errors(backend, "c65")["all"] <= flux_errors(backend, "c48")["all"], "fxadv: C65's error above C48's")


# ---------------------------------------------------------------------------------------------------------------------------
# pin 3: the D-to-C wind conversion
# ---------------------------------------------------------------------------------------------------------------------------
def library_wind_errors(backend, shape):
    cs = _case(shape, backend, cfg_kw=dict(nord=0))
    flow = ac.Flow(cs.c.RADIUS)
    wc = ac.wind_case(cs.grids, flow, cs.nz)
    one = cs.qf.ones(DIMS3)
    Q = {"delp": one, "pt": cs.qf.ones(DIMS3), "u": cs.q([_pad(x[1]) for x in wc]), "v": cs.q([_pad(x[2]) for x in wc])}
    Q.update({k: cs.q() for k in ("w", "uc", "vc", "ua", "va", "ut", "vt", "divgd", "omga", "delpc", "ptc")})
    cs.sf.call("c_sw", *[Q[k].fref for k in ("delp", "pt", "u", "v", "w", "uc", "vc", "ua", "va", "ut", "vt", "divgd", "omga", "delpc", "ptc")], 0.0)
    _sync(backend)
    R = range(len(cs.grids))
    e_all, e_edge = ac.wind_errors(wc, flow, [Q["uc"].numpy(r)[:, :, : cs.nz] for r in R], [Q["vc"].numpy(r)[:, :, : cs.nz] for r in R])
    return {"all": e_all, "edge": e_edge}


def wind_errors(backend, shape):
    return memo(("pin3", backend, shape), lambda: library_wind_errors(backend, shape))


@pytest.mark.parametrize("shape", list(ac.SHAPES))
def test_c_grid_winds_are_the_covariant_components(backend, shape):
    """c_sw with dt2 = 0 returns d2a2c_vect's winds; the worst faces are those on the tile edges"""
    e = wind_errors(backend, shape)
    ac.check_bound(f"d2a2c {shape} all faces", e["all"], REC["pin3"][shape]["all"])
    ac.check_bound(f"d2a2c {shape} tile-edge faces", e["edge"], REC["pin3"][shape]["edge"])


def test_c_grid_winds_converge_at_second_order(backend):
    ac.check_convergence("d2a2c", wind_errors(backend, "c24")["all"], wind_errors(backend, "c48")["all"])
    ac.require(wind_errors(backend, "c65")["all"] <= wind_errors(backend, "c48")["all"], "d2a2c: C65's error above C48's")


# ---------------------------------------------------------------------------------------------------------------------------
# pin 4: a2b_ord4
# ---------------------------------------------------------------------------------------------------------------------------
def library_corner_errors(backend, shape):
    cs = _case(shape, backend)
    cc = ac.corner_case(cs.grids, cs.nz)
    Q, O = cs.q([_pad(x[1]) for x in cc]), cs.q()
    cs.sf.call("a2b_ord4", Q.fref, O.fref, 0, cs.nz, 0)
    _sync(backend)
    return ac.corner_errors(cc, [O.numpy(r)[:, :, : cs.nz] for r in range(len(cs.grids))])


def corner_errors(backend, shape):
    return memo(("pin4", backend, shape), lambda: library_corner_errors(backend, shape))


@pytest.mark.parametrize("shape", list(ac.SHAPES))
def test_a_smooth_function_reaches_the_corners(backend, shape):
    e = corner_errors(backend, shape)
    for k in ("interior", "edge", "corner", "all"):
        ac.check_bound(f"a2b_ord4 {shape} {k}", e[k], REC["pin4"][shape][k])


def test_corner_interpolation_converges_at_second_order(backend):
    for k in ("interior", "edge", "corner", "all"):
        ac.check_convergence(f"a2b_ord4 {k}", corner_errors(backend, "c24")[k], corner_errors(backend, "c48")[k])
    ac.require(corner_errors(backend, "c65")["all"] <= corner_errors(backend, "c48")["all"], "a2b_ord4: C65's error above C48's")


# ---------------------------------------------------------------------------------------------------------------------------
# pin 2: the bell round the sphere
# ---------------------------------------------------------------------------------------------------------------------------
def library_bell(backend, run, dtype=torch.float64):
    """the run through TracerAdvection: a cell halo update of the tracers before every call; dp1, the fluxes and the Courant numbers, which the
    operator changes in place, restored from pristine device copies"""
    from pace_amd.halo import HaloExchanger, Layout
    from pace_amd.stencils import FiniteVolumeTransport, TracerAdvection

    n, layout, hord, cfl, turn = ac.BELL_RUNS[run]
    cs = Case(n, layout, range(6 * layout[0] * layout[1]), nz=NZ, backend=backend, cfg_kw=dict(nord=1), dtype=dtype)
    bc = ac.bell_run(run, cs.part, cs.grids, cs.c.RADIUS)
    T = {name: cs.q([_pad(q[name], NZ + 1) for q in bc.q0]) for name in ac.TRACERS}
    keep = {k: cs.q([_pad(a, NZ + 1) for a in getattr(bc, k)]) for k in ("mfx", "mfy", "cx", "cy")}
    keep["dp1"] = cs.qf.ones(DIMS3)
    work = {k: cs.q() for k in keep}
    lay = Layout(cs.part, 1, 0)
    op = TracerAdvection(cs.sf, cs.qf, FiniteVolumeTransport(cs.sf, cs.qf, cs.grids, hord=hord), cs.grids, lay, T)
    halo = HaloExchanger.shared(cs.sf, lay).updater("cell", [(q,) for q in T.values()])
    splits = set()
    for _ in range(bc.n_calls):
        for k in keep:
            work[k].storage.copy_(keep[k].storage)
        halo.update()
        op(T, work["dp1"], work["mfx"], work["mfy"], work["cx"], work["cy"])
        splits.add(op.n_split)
    _sync(backend)
    tr = [{name: T[name].numpy(r) for name in ac.TRACERS} for r in range(len(cs.grids))]
    err, side = bc.errors(tr)
    return {"err": err, "side": side, "splits": splits, "calls": bc.n_calls}


def bell(backend, run):
    return memo(("pin2", backend, run), lambda: library_bell(backend, run))


def check_bell(label, got, rec, way_label=""):
    """l2 and linf of every tracer on both levels against 1.5 x the oracle's"""
    for t in ("bell", "gauss"):
        for k in range(2):
            ac.check_bound(f"{label} {t} level {k} l2{way_label}", got[(t, k)][0], rec["l2"][t][k])
            ac.check_bound(f"{label} {t} level {k} linf{way_label}", got[(t, k)][1], rec["linf"][t][k])


def check_bell_side(label, res, rec, hord, cfl):
    side = res["side"]
    assert res["splits"] == {rec["n_split"]}, (label, res["splits"])
    for t in ac.TRACERS:
        print(f"{label} {t}: mass {side[t]['mass']:.2e}, min {side[t]['min']:.3e}, max {side[t]['max']:.6f}")
        ac.require(side[t]["mass"] <= 1e-12, f"{label} {t}: tracer mass changed by {side[t]['mass']:.2e}")
    ac.require(max(abs(side["one"]["min"] - 1.0), abs(side["one"]["max"] - 1.0)) <= 1e-13, f"{label}: the constant left 1: {side['one']}")
    for t in ("bell", "gauss"):
        if hord == 8 and cfl == 0.5:
            ac.require(side[t]["min"] >= 0.0 and side[t]["max"] <= 1.0, f"{label} {t}: hord 8 left 0 .. the initial maximum: {side[t]}")
        if hord == 6:
            ac.require(side[t]["min"] >= 1.5 * min(rec["min"][t], 0.0), f"{label} {t}: undershoot {side[t]['min']:.3e} beyond 1.5 x the oracle's {rec['min'][t]:.3e}")


def _bell_test(backend, run):
    n, layout, hord, cfl, turn = ac.BELL_RUNS[run]
    res, rec = bell(backend, run), REC["pin2"][run]
    assert res["calls"] == rec["calls"]
    check_bell(run, res["err"], rec)
    check_bell_side(run, res, rec, hord, cfl)


@pytest.mark.parametrize("run", ["c24_h6", "c24_h8", "c48_h6", "c48_h8", "c24_2x2_h8", "c24_cfl13_h8"])
def test_bell_carried_once_round_the_sphere(backend, run):
    """192 calls at C24 and 384 at C48 at Courant number 0.5 (n_split 1), C24 also on 2 x 2 ranks per tile; 74 calls at 1.3 (n_split 2)"""
    _bell_test(backend, run)


@pytest.mark.parametrize("hord", [6, 8])
def test_bell_converges_at_second_order(backend, hord):
    """the l2 error of every tracer on both levels falls by >= 3.5 from C24 to C48"""
    coarse, fine = bell(backend, f"c24_h{hord}")["err"], bell(backend, f"c48_h{hord}")["err"]
    for t in ("bell", "gauss"):
        for k in range(2):
            ac.check_convergence(f"tracer_2d_1l hord {hord} {t} level {k} l2", coarse[(t, k)][0], fine[(t, k)][0])


def test_fp32_bell_carried_once_round_the_sphere(backend32):
    """C24, hord 8 in fp32: the l2 / linf bounds of fp64; tracer mass and the constant to 8 eps32 n_calls"""
    run = "c24_h8"
    res, rec = library_bell(backend32, run, dtype=torch.float32), REC["pin2"][run]
    check_bell("fp32 " + run, res["err"], rec)
    assert res["splits"] == {1}
    bound = 8.0 * EPS32 * res["calls"]
    side = res["side"]
    for t in ac.TRACERS:
        print(f"fp32 {t}: mass {side[t]['mass']:.2e}, min {side[t]['min']:.3e}, max {side[t]['max']:.7f} (bound {bound:.2e})")
        ac.require(side[t]["mass"] <= bound, f"fp32 {t}: tracer mass changed by {side[t]['mass']:.2e}, above 8 eps32 n_calls = {bound:.2e}")
    ac.require(max(abs(side["one"]["min"] - 1.0), abs(side["one"]["max"] - 1.0)) <= bound, f"fp32: the constant left 1 by more than {bound:.2e}: {side['one']}")


# ---------------------------------------------------------------------------------------------------------------------------
# pin 5a: no force on an isentropic atmosphere at rest
# ---------------------------------------------------------------------------------------------------------------------------
PGF_SHAPES = {"c24": (24, (1, 1), tuple(range(6))), "c24_2x2": (24, (2, 2), (0,))}


def library_pgf(cs, backend, isentropic, which):
    """max |du| per rank of nh_p_grad ("d") or p_grad_c ("c") on the resting state, from u = v = 0"""
    nz = cs.nz
    st = [ac.resting_state(g, cs.c, isentropic) for g in cs.grids]
    Q = {k: cs.q([s[k] for s in st]) for k in ("delp", "pk3", "gz", "pp")}
    u, v = cs.q(), cs.q()
    if which == "d":
        cs.sf.call("nh_p_grad", u.fref, v.fref, Q["pp"].fref, Q["gz"].fref, Q["pk3"].fref, Q["delp"].fref, ac.PGF_DT, float(cs.grids[0].ptop), cs.c.KAPPA)
    else:
        cs.sf.call("p_grad_c", u.fref, v.fref, Q["delp"].fref, Q["pk3"].fref, Q["gz"].fref, ac.PGF_DT)
    _sync(backend)
    out = []
    for r, g in enumerate(cs.grids):
        G = ac.Geometry(g)
        a, b = (u.numpy(r), v.numpy(r)) if which == "d" else (v.numpy(r), u.numpy(r))  # (p_grad_c's first wind lives on the x faces)
        assert np.all(np.isfinite(a[G.Y][..., :nz])) and np.all(np.isfinite(b[G.X][..., :nz]))
        out.append(ac.force(G, a, b, nz))
    return out, st


@pytest.mark.parametrize("which", ["d", "c"])
@pytest.mark.parametrize("shape", list(PGF_SHAPES))
def test_no_pressure_gradient_force_on_an_isentropic_atmosphere_at_rest(backend, shape, which):
    """nh_p_grad (with its four corner interpolations) and p_grad_c over a 3 km mountain: the wind stays 0 to round-off on the isentropic state, and
    moves on the control state of the same call"""
    n, layout, ranks = PGF_SHAPES[shape]
    cs = Case(n, layout, ranks, nz=ac.PGF_NZ, backend=backend)
    rest, _ = library_pgf(cs, backend, True, which)
    control, _ = library_pgf(cs, backend, False, which)
    for r, (a, b) in enumerate(zip(rest, control)):
        ac.check_no_force(f"{'nh_p_grad' if which == 'd' else 'p_grad_c'} {shape} rank {cs.ranks[r]}", a, b)


def test_fp32_no_pressure_gradient_force_on_an_isentropic_atmosphere_at_rest(backend32):
    """nh_p_grad in fp32, C24: max |du| <= K eps32 S (module docstring).  Measured, host emulation and MI355X alike: 1.5e-06 .. 1.8e-06 per rank
    against bounds of 3.8e-05 .. 4.7e-05 (the control state's force is 2.9e-02)."""
    cs = Case(24, (1, 1), range(6), nz=ac.PGF_NZ, backend=backend32, cfg_kw=dict(nord=1), dtype=torch.float32)
    rest, st = library_pgf(cs, backend32, True, "d")
    for r, g in enumerate(cs.grids):
        bound = REC["pin5a"]["K"] * EPS32 * ac.pgf_scale(g, cs.c, st[r])
        print(f"fp32 nh_p_grad rank {r}: max |du| {rest[r]:.3e}, bound {bound:.3e}")
        ac.require(rest[r] <= bound, f"fp32 nh_p_grad rank {r}: |du| {rest[r]:.3e} above K eps32 S = {bound:.3e}")


# ---------------------------------------------------------------------------------------------------------------------------
# pin 5b: profiles linear in pressure through the remap
# ---------------------------------------------------------------------------------------------------------------------------
def _remap_inputs(cs, nz):
    g, s = cs.grids[0], {k: v.copy() for k, v in cs.states[0].items()}
    s["delp"] = ac.lagrangian_delp(s["delp"], nz)
    tr, want = {}, {}
    for name, prof in ac.LINEAR.items():
        q1, q2, pe1, pe2 = ac.linear_columns(g, s["delp"], nz, prof)
        tr[name], want[name] = _pad(q1), q2
    s["u"], want["u"], s["v"], want["v"] = ac.linear_winds(g, s["delp"], nz, ac.LINEAR_UV)
    s["u"], s["v"] = _pad(s["u"]), _pad(s["v"])
    s["pkz"] = np.ones_like(s["delp"])
    s["pe"] = pe1  # the Lagrangian interfaces of the stretched layers, and what hangs on them
    s["peln"], s["pk"] = np.log(pe1), pe1**KAPPA
    return s, tr, want, pe2


def _ranges(s, tr, nz):
    return {k: float(np.ptp(a[3:-4, 3:-4, :nz])) for k, a in list(tr.items()) + [("u", s["u"]), ("v", s["v"])]}


@pytest.mark.parametrize("nz", [6, 79])
def test_oracle_remap_is_exact_for_profiles_linear_in_pressure(nz):
    """the whole-rank oracle on the same input: exact to 1e-13 for the tracers, u and v (which is why the library is asked for them); w is not
    (module docstring) and is left out"""
    from fv3_oracle import remap as o_remap

    from pace_amd.init import synthetic_state

    part, grids, doms, c = ac.make(12, (1, 1), (0,), nz)
    fake = type("CS", (), {"grids": grids, "states": [synthetic_state(grids[0], seed=7, rank=0)]})
    s, tr, want, _ = _remap_inputs(fake, nz)
    rng = _ranges(s, tr, nz)
    D, G = doms[0], ac.Geometry(grids[0])
    s = {k: np.ascontiguousarray(v) for k, v in s.items()}
    tl = [np.ascontiguousarray(tr[k]) for k in ac.LINEAR]
    o_remap.lagrangian_to_eulerian(D, c, s, np.zeros(s["delp"].shape[:2]), tl)
    for k, a in zip(ac.LINEAR, tl):
        ac.check_linear(f"oracle remap nz {nz} {k}", a[G.cells][..., :nz], want[k][G.cells], rng[k])
    ac.check_linear(f"oracle remap nz {nz} u", s["u"][G.Y][..., :nz], want["u"][G.Y], rng["u"])
    ac.check_linear(f"oracle remap nz {nz} v", s["v"][G.X][..., :nz], want["v"][G.X], rng["v"])


@pytest.mark.parametrize("nz", [6, 79])
def test_remap_keeps_profiles_linear_in_pressure(backend, nz):
    """C12, 6 and 79 levels: tracers linear in the mid-layer pressure of the Lagrangian delp come back linear in the mid-layer pressure of the Eulerian
    pe the operator returns; u / v likewise in the edge-averaged pressure"""
    from pace_amd.stencils import LagrangianToEulerian

    cs = Case(12, (1, 1), (0,), nz=nz, backend=backend)
    s, tr, want, pe2 = _remap_inputs(cs, nz)
    rng = _ranges(s, tr, nz)
    names = ("pt", "delp", "delz", "peln", "pe", "pk", "pkz", "u", "v", "w", "cappa")
    Q = {k: cs.q([s[k]]) for k in names}
    T = {k: cs.q([tr[k]]) for k in ac.LINEAR}
    ps, wsd = cs.qf.zeros(("x", "y")), cs.qf.zeros(("x", "y"))
    LagrangianToEulerian(cs.sf, cs.qf, cs.grids)(T, *[Q[k] for k in names], ps, wsd)
    _sync(backend)
    G = ac.Geometry(cs.grids[0])
    pe = Q["pe"].numpy(0)[G.cells]
    assert np.abs(pe - pe2[G.cells]).max() <= 1e-13 * pe.max()  # the Eulerian interfaces are ak + bk ps
    for k, (a, b) in ac.LINEAR.items():
        ac.check_linear(f"remap nz {nz} {k}", T[k].numpy(0)[G.cells][..., :nz], a + b * 0.5 * (pe[..., 1:] + pe[..., :-1]), rng[k])
    ac.check_linear(f"remap nz {nz} u", Q["u"].numpy(0)[G.Y][..., :nz], want["u"][G.Y], rng["u"])
    ac.check_linear(f"remap nz {nz} v", Q["v"].numpy(0)[G.X][..., :nz], want["v"][G.X], rng["v"])


# ---------------------------------------------------------------------------------------------------------------------------
# the recorded figures, and the controls: every checker has teeth (CPU, oracle only)
# ---------------------------------------------------------------------------------------------------------------------------
def test_recorded_oracle_figures_are_fresh():
    """the C24 entries of pins 1, 3 and 4, of pins 6, 7 and 9 (tests/test_analytic_dynamics.py) and of pins 10 - 13 (tests/test_analytic_damping.py),
    re-measured with the oracle: within 1 % of tests/golden/analytic_pins.json (figures that are round-off, below 1e-12, are not compared)"""
    import damping_case

    now = ac.measure_single_call_pins("c24")
    now.update(ac.measure_d_sw("c24"))
    now["pin9"] = ac.measure_heights("c24")
    for pin, d in now.items():
        for k, v in d.items():
            want = REC[pin]["c24"][k]
            if max(abs(v), abs(want)) < 1e-12:
                continue
            assert abs(v - want) <= 0.01 * abs(want), f"{pin} c24 {k}: {v} now, {want} recorded -- run python tests/analytic_case.py --record"
    stale = damping_case.stale_entries(REC)
    assert not stale, f"{stale} -- run python tests/analytic_case.py --record damping"


def _oracle_pin(shape, pin, spoil):
    n, layout, ranks = ac.SHAPES[shape]
    part, grids, doms, c = ac.make(n, layout, ranks, 1)
    for D in doms:
        spoil(D)
    flow = ac.Flow(c.RADIUS)
    if pin == 1:
        dt, fc = REC["pin1"][shape]["dt"], ac.flux_case(grids, flow)
        xs, ys, _ = ac.oracle_fluxes(doms, fc, dt)
        return ac.flux_errors(fc, flow, dt, xs, ys)[0]
    cc = ac.corner_case(grids)
    return ac.corner_errors(cc, ac.oracle_corners(doms, cc))


def _pin1_checks(e24, e48):
    ac.check_bound("fxadv c48", e48, REC["pin1"]["c48"]["all"])
    ac.check_convergence("fxadv", e24, e48)


def test_control_pin1_exchanged_sines_fail():
    def swap(D):
        D.m.sin_sg1, D.m.sin_sg3 = D.m.sin_sg3, D.m.sin_sg1

    _pin1_checks(_oracle_pin("c24", 1, lambda D: None), _oracle_pin("c48", 1, lambda D: None))
    with pytest.raises(ac.CheckFailed):
        _pin1_checks(_oracle_pin("c24", 1, swap), _oracle_pin("c48", 1, swap))


def test_control_pin4_scaled_edge_factor_fails():
    def scale(D):
        D.edge_w = D.edge_w * 1.05

    ac.check_bound("a2b_ord4 c48 edge", _oracle_pin("c48", 4, lambda D: None)["edge"], REC["pin4"]["c48"]["edge"])
    with pytest.raises(ac.CheckFailed):
        ac.check_bound("a2b_ord4 c48 edge", _oracle_pin("c48", 4, scale)["edge"], REC["pin4"]["c48"]["edge"])


def test_control_pin2_solution_turned_the_wrong_way_fails():
    """a quarter revolution (after a whole one both directions agree): the oracle meets its own record the right way and misses it the wrong way"""
    run = "c24_quarter_h8"
    n, layout, hord, cfl, turn = ac.BELL_RUNS[run]
    part, grids, doms, c = ac.make(n, layout, range(6), 2)
    bc = ac.bell_run(run, part, grids, c.RADIUS)
    tr, _ = ac.oracle_bell(doms, bc, hord)
    check_bell(run, bc.errors(tr)[0], REC["pin2"][run])
    with pytest.raises(ac.CheckFailed):
        check_bell(run, bc.errors(tr, way=-1.0)[0], REC["pin2"][run], " (wrong way)")


def test_control_pin5a_control_state_fails():
    part, grids, doms, c = ac.make(24, (1, 1), (0,), ac.PGF_NZ)
    g, D, G = grids[0], doms[0], ac.Geometry(grids[0])
    rest = ac.force(G, *ac.oracle_pgf(D, c, ac.resting_state(g, c)), ac.PGF_NZ)
    control = ac.force(G, *ac.oracle_pgf(D, c, ac.resting_state(g, c, False)), ac.PGF_NZ)
    ac.check_no_force("oracle nh_p_grad", rest, control)
    with pytest.raises(ac.CheckFailed):
        ac.check_no_force("oracle nh_p_grad, control state", control, control)
    rest_c = ac.force(G, *ac.oracle_pgf_c(D, ac.resting_state(g, c))[::-1], ac.PGF_NZ)
    control_c = ac.force(G, *ac.oracle_pgf_c(D, ac.resting_state(g, c, False))[::-1], ac.PGF_NZ)
    ac.check_no_force("oracle p_grad_c", rest_c, control_c)
    with pytest.raises(ac.CheckFailed):
        ac.check_no_force("oracle p_grad_c, control state", control_c, control_c)


@pytest.mark.parametrize("iv", [-1, 0, 1, 2])
def test_control_pin5b_quadratic_profile_fails(iv):
    """remap_column on 20 layers of random thickness: a linear profile to 1e-13 of its range, end layers included; the exact layer means of a quadratic
    one are missed"""
    from fv3_oracle import remap as o_remap

    rng = np.random.default_rng(3)
    pe1 = 300.0 + np.concatenate([[0.0], np.cumsum(rng.uniform(200.0, 8000.0, 20))])
    pe2 = 300.0 + (pe1[-1] - 300.0) * np.linspace(0.0, 1.0, 21) ** 1.2

    def means(pe, curve):
        return 5.0 - 3.0e-5 * ac._mid(pe) + curve * (pe[1:] ** 2 + pe[1:] * pe[:-1] + pe[:-1] ** 2) / 3.0

    q1 = means(pe1, 0.0)
    ac.check_linear(f"remap_column iv {iv} linear", o_remap.remap_column(pe1, q1, pe2, iv=iv), means(pe2, 0.0), np.ptp(q1))
    q1 = means(pe1, 2.0e-10)
    with pytest.raises(ac.CheckFailed):
        ac.check_linear(f"remap_column iv {iv} quadratic", o_remap.remap_column(pe1, q1, pe2, iv=iv), means(pe2, 2.0e-10), np.ptp(q1))
