"""Input builders of tests/test_height_pgf_operator_edges.py: the families of inputs the height advection (update_dz_c, update_dz_d), the pressure-gradient
operators (nh_p_grad, p_grad_c) and del2_cubed are run on alone.  Every builder works on a helpers.Case and returns one dict of [i, j, k] arrays per rank;
the operator gets the same arrays in the library and in the oracle, so no halo exchange is needed and the inputs need not be a balanced state -- the tests assert
from the oracle alone that its outputs are finite, the new heights strictly decreasing and the switches taken on both sides.

  heights_strong   crx / cry / xfx / yfx from the oracle's fxadv on horizontal_case.strong (Courant numbers up to ``cfl`` in both signs on every tile edge); zh from a
                   terrain (a 400 m wave in tile-index space; 40 m from 79 levels on) and the state's delz, plus a 2-dx checkerboard of 5 % of the layer thickness; for update_dz_c
                   ut / vt = 0.5 x xfx / yfx with dt2 = dt / 2
  heights_still    horizontal_case.still: exactly zero winds over the SW cube corner's rectangle (still_box), there zs = 256 m and every
                   interface height a power of two (256 m x 2^(levels below it): z area / area is then exact, which a general height is not)
  heights_front    strong, with 300 m x the 0 / 1 front of test_tracer_remap_edges._front added to every interface
  pgf_rough        delp x (1 + 0.5 front), pk3 hydrostatic from it, gz = g x (heights over the terrain + a 2-dx checkerboard of random amplitude up to 300 m),
                   pp a 2-dx checkerboard of random amplitude up to 200 Pa; u / v of the state, uc / vc = 0.7 x v / u; pkc = pk3 and delpc = delp for p_grad_c
  heat_rough       a 2-dx checkerboard of random amplitude 0.5 .. 1 as the heat source, cd = 0.2 da_min
"""
import copy

import numpy as np

import horizontal_case as hc
from fv3_oracle import d_sw as o_dsw
from fv3_oracle.util import Dom

NH = hc.NH
FLUXES = ("crx", "cry", "xfx", "yfx", "ut", "vt")
STILL_ZS = 256.0


def board(cs, r):
    """the 2-dx checkerboard +-1 [i, j, 1] in global tile indices"""
    i, j, _ = hc._index(cs, r)
    return np.where((i + j) % 2 == 0, 1.0, -1.0)


def terrain(cs, r, hill=400.0):
    """zs [i, j, 1]: ``hill`` (1 + a wave 17 x 19 cells long in tile-index space)"""
    i, j, _ = hc._index(cs, r)
    return hill * (1.0 + np.sin(2 * np.pi * i / 17.0) * np.cos(2 * np.pi * j / 19.0))


def fluxes(cs, ins, dt):
    """the oracle's fxadv on the winds of ``ins``: ([{crx, cry, xfx, yfx, ut, vt} per rank], [fxadv's branch counts per rank])"""
    out, counts = [], []
    for D, x in zip(cs.doms, ins):
        z = {k: np.zeros_like(x["uc"]) for k in FLUXES}
        o_dsw.reset_counters()
        o_dsw.fxadv(D, x["uc"].copy(), x["vc"].copy(), *[z[k] for k in FLUXES], dt)
        counts.append(o_dsw.counters())
        out.append(z)
    return out, counts


def layer_heights(cs, r, zs):
    """interface heights [i, j, nz + 1] from zs and the state's delz, summed from the ground"""
    nz = cs.nz
    delz = cs.states[r]["delz"]
    zh = np.zeros(delz.shape[:2] + (nz + 1,))
    zh[:, :, nz] = zs[:, :, 0]
    for k in range(nz - 1, -1, -1):
        zh[:, :, k] = zh[:, :, k + 1] - delz[:, :, k]
    return zh


def rough_heights(cs, r, zs, amp=0.05):
    zh = layer_heights(cs, r, zs)
    thick = zh[:, :, :-1] - zh[:, :, 1:]
    thick = np.concatenate([thick, thick[:, :, -1:]], axis=2)
    return zh + amp * board(cs, r) * thick


def _heights(cs, ins, dt, add=None, hill=400.0):
    F, counts = fluxes(cs, ins, dt)
    out = []
    for r, f in enumerate(F):
        zs = terrain(cs, r, hill)
        zh = rough_heights(cs, r, zs)
        if add is not None:
            zh = zh + add(r)
        z2 = np.zeros(zs.shape)
        out.append(dict(f, zs=zs, zh=zh, ws=z2, ut_c=0.5 * f["xfx"], vt_c=0.5 * f["yfx"]))
    return out, counts


def heights_strong(cs, dt, cfl=0.85, hill=400.0):
    """(hill: the terrain's height.  Where the lowest layers are 18 .. 30 m thick -- 79 levels and more -- a 400 m hill under Courant numbers that change sign from
    level to level makes neighbouring interfaces cross; 40 m keeps the thinnest new layer at 9 m)"""
    return _heights(cs, hc.strong(cs, dt, cfl=cfl), dt, hill=hill)


def heights_front(cs, dt, cfl=0.85):
    from test_tracer_remap_edges import _front

    return _heights(cs, hc.strong(cs, dt, cfl=cfl), dt, add=lambda r: 300.0 * _front(cs.grids[r], cs.nz + 1))


def heights_still(cs, dt):
    """the smooth winds with the still rectangle: there the Courant numbers, the area fluxes and ut / vt are exactly 0, the terrain flat, every interface level"""
    out, counts = _heights(cs, hc.still(cs), dt)
    k = np.arange(cs.nz + 1)[None, None, :]
    for D, x in zip(cs.doms, out):
        if D.sw:
            box = hc.still_box(D)
            x["zs"][box] = STILL_ZS
            x["zh"][box] = STILL_ZS * 2.0 ** (cs.nz - k)
    return out, counts


def pgf_rough(cs, seed=23):
    from test_tracer_remap_edges import _front

    c, nz, out = cs.c, cs.nz, []
    for r, (g, s) in enumerate(zip(cs.grids, cs.states)):
        rng = np.random.default_rng(seed + cs.ranks[r])
        b = board(cs, r)
        delp = s["delp"][:, :, :nz] * (1.0 + 0.5 * _front(g, nz))
        pe = np.concatenate([np.full(delp.shape[:2] + (1,), g.ptop), g.ptop + np.cumsum(delp, axis=2)], axis=2)
        pk3 = np.exp(c.KAPPA * np.log(pe))
        zh = layer_heights(cs, r, terrain(cs, r))
        gz = c.GRAV * (zh + 300.0 * b * rng.uniform(0.0, 1.0, zh.shape))
        pp = 200.0 * b * rng.uniform(0.0, 1.0, zh.shape)
        u, v = s["u"][:, :, :nz].copy(), s["v"][:, :, :nz].copy()
        out.append(dict(u=u, v=v, uc=0.7 * v, vc=0.7 * u, pp=pp, gz=gz, pk3=pk3, delp=delp))
    return out


def heat_rough(cs, seed=31):
    """([q [i, j, nz] per rank], cd)"""
    qs = []
    for r in range(len(cs.ranks)):
        rng = np.random.default_rng(seed + cs.ranks[r])
        qs.append(board(cs, r) * rng.uniform(0.5, 1.0, cs.states[r]["u"][:, :, : cs.nz].shape))
    return qs, 0.2 * cs.grids[0].da_min


def dom_as(D, dtype):
    """the rank's Dom with every metric array, the tile-edge weights and the corner extrapolation factors in ``dtype``"""
    g = copy.copy(D.grid)
    g.fields = {k: v.astype(dtype) for k, v in D.grid.fields.items()}
    for n in ("edge_w", "edge_e", "edge_s", "edge_n", "corner_extrap"):
        setattr(g, n, getattr(g, n).astype(dtype))
    return Dom(g, D.c)


def as_dtype(args, dtype):
    return [a.astype(dtype) if isinstance(a, np.ndarray) and a.dtype.kind == "f" else a for a in args]
