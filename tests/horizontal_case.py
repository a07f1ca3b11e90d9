"""Input builders of tests/test_horizontal_operator_edges.py: the families of inputs the horizontal operators (c_sw, d_sw, fxadv,
fv_tp_2d, a2b_ord4) are run on alone.  Every builder works on a helpers.Case and returns, per rank, a dict of [i, j, k] arrays on
the case's nz levels; the operator gets the same arrays in the library and in the oracle, so no halo exchange is needed and the
inputs need not be a balanced state -- the tests assert that the oracle's outputs are finite and the new air mass positive.

  smooth   the recipe of test_parity.test_d_sw: the synthetic state, C-grid winds 0.7 x the D-grid ones (Courant numbers ~1e-3)
  strong   the advecting winds uc / vc as (1 + 0.1 x the smooth state's, normalised) x the local cell width x sign-changing waves in tile-index space (11 and 13 cells long, across the flow, so
           that every tile edge sees both upwind signs and the flow stays weakly divergent) and scaled so that max(|crx|, |cry|) of the
           oracle's fxadv is ``cfl``
  rough    strong winds at Courant number 0.2 (or ``cfl``); u / v with a 2-dx checkerboard of random amplitude up to amp[k] dx / dt, growing with
           level; a divgd input with dt |divgd| uniform in 0 .. lin[k]
  still    smooth, with a rectangle of exactly zero wind and exactly constant scalars over the SW cube corner: halo and compute cells
  front    strong winds; the 0 / 1 front of test_tracer_remap_edges._front in pt, q_con and w
  real     the C12 L63 restart: c_sw's / d_sw's own inputs in one recorded oracle call (test_column_solver_edges.real_calls)
"""
import numpy as np

from fv3_oracle import d_sw as o_dsw

NH = 3
D_SW_IN = ("delp", "pt", "u", "v", "w", "uc", "vc", "ua", "va", "divgd", "mfxd", "mfyd", "cxd", "cyd", "q_con")
D_SW_ARGS = ("delpc",) + D_SW_IN[:-1] + ("crx", "cry", "xfx", "yfx", "q_con", "zh", "heat_source", "diss_est")  # the operator's argument order
C_SW_IN = ("delp", "pt", "u", "v", "w", "uc", "vc", "ua", "va", "omga")
STILL = 7  # compute cells of the still rectangle in each direction (plus the halo before them)


def _index(cs, r):
    """global tile indices [i, 1, 1], [1, j, 1] and the level [1, 1, k] of rank r's storage"""
    ox, oy = cs.part.origin(r)
    i = (np.arange(cs.part.nx + 2 * NH + 1) - NH + ox)[:, None, None]
    j = (np.arange(cs.part.ny + 2 * NH + 1) - NH + oy)[None, :, None]
    return i, j, np.arange(cs.nz)[None, None, :]


def smooth(cs):
    nz, out = cs.nz, []
    for s in cs.states:
        x = {k: v[:, :, :nz].copy() for k, v in s.items() if k != "phis"}
        x["uc"], x["vc"] = 0.7 * x["v"], 0.7 * x["u"]
        x["ua"], x["va"] = 0.9 * np.roll(x["u"], 1, 1), 0.9 * np.roll(x["v"], 1, 0)
        x["divgd"] = 1e-6 * x["w"]
        out.append(x)
    return out


def max_courant(cs, ins, dt):
    """max(|crx|, |cry|) of the oracle's fxadv on the faces d_sw's outputs are compared on, over the ranks; and whether both signs occur"""
    worst, neg, pos = 0.0, False, False
    for D, x in zip(cs.doms, ins):
        z = [np.zeros_like(x["uc"]) for _ in range(6)]
        o_dsw.fxadv(D, x["uc"].copy(), x["vc"].copy(), *z, dt)
        for a in (z[0][D.sl(1, D.nx + 1, D.jsd, D.jed)], z[1][D.sl(D.isd, D.ied, 1, D.ny + 1)]):
            worst, neg, pos = max(worst, float(np.abs(a).max())), neg or bool((a < 0).any()), pos or bool((a > 0).any())
    return worst, neg and pos


def strong(cs, dt, cfl=0.85):
    ins = smooth(cs)
    for r, (D, x) in enumerate(zip(cs.doms, ins)):
        i, j, k = _index(cs, r)
        x["uc"] = (1.0 + 0.1 * x["uc"] / np.abs(x["uc"]).max()) * np.cos(2 * np.pi * (j + 0.2 * i) / 11.0 + 0.9 * k) / D.m.rdxa
        x["vc"] = (1.0 + 0.1 * x["vc"] / np.abs(x["vc"]).max()) * np.sin(2 * np.pi * (i - 0.2 * j) / 13.0 + 0.5 * k) / D.m.rdya
    scale = cfl / max_courant(cs, ins, dt)[0]
    for x in ins:
        x["uc"] *= scale
        x["vc"] *= scale
    return ins


def rough(cs, dt, amp_top=0.15, seed=11, cfl=0.2):
    ins = strong(cs, dt, cfl=cfl)
    nz = cs.nz
    amp, lin = np.linspace(0.0, amp_top, nz)[None, None, :], np.linspace(0.1, 1.0, nz)[None, None, :]
    for r, (g, x) in enumerate(zip(cs.grids, ins)):
        rng = np.random.default_rng(seed + cs.ranks[r])
        i, j, _ = _index(cs, r)
        board = np.where((i + j) % 2 == 0, 1.0, -1.0) * np.sqrt(g.da_min) / dt
        x["u"] = x["u"] + amp * rng.uniform(0.0, 1.0, x["u"].shape) * board
        x["v"] = x["v"] + amp * rng.uniform(0.0, 1.0, x["v"].shape) * board
        x["divgd"] = lin * rng.uniform(-1.0, 1.0, x["u"].shape) / dt
    return ins


def still_box(D):
    """the still rectangle of a rank with the SW cube corner: storage slices (halo + STILL compute cells; fewer on a narrower rank)"""
    return (slice(0, NH + min(STILL, D.nx - 2)), slice(0, NH + min(STILL, D.ny - 2)))


def still(cs, names=D_SW_IN):
    ins = smooth(cs)
    for D, x in zip(cs.doms, ins):
        if not D.sw:
            continue
        box = still_box(D)
        for n in names:
            if n in ("delp", "pt", "q_con"):
                x[n][box] = {"delp": 1000.0, "pt": 300.0, "q_con": 1.0e-4}[n]
            elif n not in ("mfxd", "mfyd", "cxd", "cyd"):
                x[n][box] = 0.0
    return ins


def front(cs, dt, cfl=0.85):
    from test_tracer_remap_edges import _front

    ins = strong(cs, dt, cfl=cfl)
    for g, x in zip(cs.grids, ins):
        f = _front(g, cs.nz)
        x["pt"], x["q_con"], x["w"] = 280.0 + 40.0 * f, 0.01 * f, 1.0 * f
    return ins


def strong_c(cs, dt2, cfl=0.2):
    """c_sw: the D-grid winds themselves modulated as in ``strong`` and scaled so that dt2 max(|u|, |v|) / dx is ``cfl`` -- the
    first-order upwind transport keeps the air mass positive while the outflow of a cell through its four faces stays below 1"""
    out = []
    for r, (g, s) in enumerate(zip(cs.grids, cs.states)):
        x = {k: v.copy() for k, v in s.items() if k in C_SW_IN}
        i, j, _ = _index(cs, r)
        k = np.arange(x["u"].shape[2])[None, None, :]
        x["u"] = (1.0 + 0.3 * x["u"] / np.abs(x["u"]).max()) * np.sin(2 * np.pi * (i - 0.2 * j) / 13.0 + 0.5 * k)
        x["v"] = (1.0 + 0.3 * x["v"] / np.abs(x["v"]).max()) * np.cos(2 * np.pi * (j + 0.2 * i) / 11.0 + 0.9 * k)
        out.append(x)
    top = max(max(np.abs(x["u"]).max(), np.abs(x["v"]).max()) for x in out)
    scale = cfl * min(np.sqrt(g.da_min) for g in cs.grids) / dt2 / top
    for x in out:
        x["u"] *= scale
        x["v"] *= scale
    return out


def smooth_c(cs):
    return [{k: v.copy() for k, v in s.items() if k in C_SW_IN} for s in cs.states]


def still_c(cs):
    out = smooth_c(cs)
    for D, x in zip(cs.doms, out):
        if D.sw:
            box = still_box(D)
            for n in ("u", "v", "w"):
                x[n][box] = 0.0
            x["delp"][box], x["pt"][box] = 1000.0, 300.0
    return out
