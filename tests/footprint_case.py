"""Read and write footprints of the acoustic operators (tests/test_operator_footprints.py): region masks, guarded storage, the
per-operator adapters, the poison tables and the engine that runs one case.

One case = one operator on one shape.  Per rank the ORACLE runs twice -- clean, and with NaN in every cell of the operator's poison
table -- and must give the same bits on the regions the parity tests compare: that validates the table.  Then the LIBRARY is called
three times in one context on guarded fields (clean, poisoned, clean) and is compared with itself, bit for bit.  No tolerance anywhere.

  python tests/footprint_case.py --discover OP [SHAPE ...]   which regions of which input the oracle does not need (prints a table row;
                                                             the intersection over the shapes and their ranks); no test calls it
  python tests/footprint_case.py --run OP[,OP...] SHAPE[,SHAPE...] --backend hostemu|hip:gfx950
                                                             one case in a process of its own: the kernel forms that are chosen once
                                                             per process (FV3_TP2D_MODE, FV3_RIEM_MODE, FV3_EDGE_PROFILE_*)

Region names of a table (all horizontal, applied to every level of the storage, except ``pad``):
  pad                  level nz of a cell-level field
  corner_blocks        the halo block beyond each cube corner the rank has, out to the end of the storage
  depth>=d             halo cells at Chebyshev distance >= d from the field's own compute box (its staggered end belongs to the box)
  diagonal             halo cells outside the compute range in both directions
  side:W,depth>=d      halo cells d or more columns west of the box (E, S, N alike)
  all                  the field is not read on entry
"""
import argparse
import contextlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "oracle"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import horizontal_case as hc  # noqa: E402
from helpers import Case  # noqa: E402
from pace_amd._testing import stencil_factory_for  # noqa: E402
from pace_amd.constants import get_constants  # noqa: E402
from pace_amd.quantity import Quantity  # noqa: E402

from fv3_oracle import a2b_ord4 as o_a2b  # noqa: E402
from fv3_oracle import c_sw as o_csw  # noqa: E402
from fv3_oracle import d_sw as o_dsw  # noqa: E402
from fv3_oracle import fvtp2d as o_tp  # noqa: E402
from fv3_oracle import nh as o_nh  # noqa: E402
from fv3_oracle import ppm as o_ppm  # noqa: E402

GUARD = 4096  # elements on either side of a field; a multiple of 64, so the base alignment of an ordinary allocation is kept
GUARD_VALUE = -1.2345678e30  # one fixed bit pattern per precision (what the value rounds to)
DT, DT2 = 60.0, 30.0

# ---------------------------------------------------------------------------------------------------------------------------
# regions
# ---------------------------------------------------------------------------------------------------------------------------
X_STAG = {"v", "uc", "mfxd", "cxd", "mfx", "cx", "crx", "xfx", "ut", "fx"}  # an extra x interface in the field's own compute box
Y_STAG = {"u", "vc", "mfyd", "cyd", "mfy", "cy", "cry", "yfx", "vt", "fy"}
XY_STAG = {"divgd", "qout"}


def _halo_depths(D, name):
    """cells west / east of the box [ni, 1] and south / north of it [1, nj]; 0 inside"""
    ni, nj = D.shape2()
    ex, ey = int(name in X_STAG or name in XY_STAG), int(name in Y_STAG or name in XY_STAG)
    i, j = (np.arange(ni) - D.o)[:, None], (np.arange(nj) - D.o)[None, :]
    return np.maximum(1 - i, 0), np.maximum(i - (D.nx + ex), 0), np.maximum(1 - j, 0), np.maximum(j - (D.ny + ey), 0)


def region(D, name, spec):
    """boolean [ni, nj] mask of one named horizontal region of field ``name`` on rank D"""
    w, e, s, n = _halo_depths(D, name)
    if spec == "corner_blocks":
        m = np.zeros(D.shape2(), dtype=bool)
        for has, a, b in ((D.sw, w, s), (D.se, e, s), (D.ne, e, n), (D.nw, w, n)):
            if has:
                m |= (a > 0) & (b > 0)
        return m
    if spec == "diagonal":
        return ((w + e) > 0) & ((s + n) > 0)
    if spec.startswith("depth>="):
        return np.maximum(np.maximum(w, e), np.maximum(s, n)) >= int(spec[7:])
    if spec.startswith("side:"):
        side, depth = spec[5:].split(",")
        return np.broadcast_to({"W": w, "E": e, "S": s, "N": n}[side] >= int(depth[7:]), D.shape2()).copy()
    raise ValueError(spec)


CANDIDATES = ("all", "depth>=1", "depth>=2", "depth>=3", "diagonal", "corner_blocks") + tuple(f"side:{s},depth>={d}" for s in "WESN" for d in (1, 2, 3))


def _implied(spec, have):
    """is region ``spec`` contained in one of the accepted regions ``have``?"""
    if "all" in have:
        return True
    d_of = lambda x: int(x.split(">=")[1])  # noqa: E731
    if spec.startswith("depth>="):
        return any(h.startswith("depth>=") and d_of(h) <= d_of(spec) for h in have)
    if spec == "diagonal":
        return "depth>=1" in have
    if spec == "corner_blocks":
        return "depth>=1" in have or "diagonal" in have
    if spec.startswith("side:"):
        return any((h.startswith("depth>=") or h[:6] == spec[:6]) and d_of(h) <= d_of(spec) for h in have)
    return False


def box_mask(D, i0, i1, j0, j1):
    m = np.zeros(D.shape2(), dtype=bool)
    m[D.sl(i0, i1, j0, j1)] = True
    return m


CELLS = lambda D: box_mask(D, 1, D.nx, 1, D.ny)  # noqa: E731
U = lambda D: box_mask(D, 1, D.nx, 1, D.ny + 1)  # noqa: E731
V = lambda D: box_mask(D, 1, D.nx + 1, 1, D.ny)  # noqa: E731
XF = lambda D: box_mask(D, 1, D.nx + 1, D.jsd, D.jed)  # noqa: E731
YF = lambda D: box_mask(D, D.isd, D.ied, 1, D.ny + 1)  # noqa: E731
CORNERS = lambda D: box_mask(D, 1, D.nx + 1, 1, D.ny + 1)  # noqa: E731
RING2 = lambda D: box_mask(D, -1, D.nx + 2, -1, D.ny + 2)  # noqa: E731
UT_C = lambda D: box_mask(D, 0, D.nx + 2, 0, D.ny + 1)  # noqa: E731
VT_C = lambda D: box_mask(D, 0, D.nx + 1, 0, D.ny + 2)  # noqa: E731


def C1(D):
    return box_mask(D, 0, D.nx + 1, 0, D.ny + 1)


def RING1(D):
    """compute domain + 1 ring without the cube-corner halo cell, which belongs to no neighbour (test_operator_parity._cmp, test_parity.test_c_sw)"""
    m = C1(D)
    for (ci, cj), has in (((0, 0), D.sw), ((D.nx + 1, 0), D.se), ((D.nx + 1, D.ny + 1), D.ne), ((0, D.ny + 1), D.nw)):
        if has:
            m[D.sl(ci, ci, cj, cj)] = False
    return m


DSW_OUT = {"delp": CELLS, "pt": CELLS, "w": CELLS, "q_con": CELLS, "u": U, "v": V, "heat_source": CELLS, "mfxd": V, "mfyd": U, "cxd": XF, "cyd": YF, "crx": XF, "cry": YF,
           "xfx": XF, "yfx": YF, "divgd": CORNERS}  # test_horizontal_operator_edges.DSW_OUT
FXADV_OUT = {"crx": XF, "xfx": XF, "ut": XF, "cry": YF, "yfx": YF, "vt": YF}  # test_horizontal_operator_edges.FXADV_OUT
CSW_OUT = {"delpc": RING1, "ptc": RING1, "omga": RING1, "divgd": CORNERS, "uc": V, "vc": U, "ut": UT_C, "vt": VT_C, "ua": C1}  # test_parity.test_c_sw

# ---------------------------------------------------------------------------------------------------------------------------
# the poison tables: input -> regions the oracle does not read (found with --discover on every shape of the operator, validated again
# by every test case before the library is called).  ``pad`` is added to every cell-level 3-D input by the engine.
# ---------------------------------------------------------------------------------------------------------------------------
TABLES = {
    "a2b_ord4": {
        "qin": ("depth>=3", "corner_blocks"),
    },
    "apply_diffusive_heating": {
        "delp": ("depth>=1",),
        "delz": ("depth>=1",),
        "cappa": ("depth>=1",),
        "heat_source": ("depth>=1",),
        "pt": ("depth>=1",),
    },
    "c_sw": {
        "delp": ("depth>=3", "corner_blocks"),
        "pt": ("depth>=3", "corner_blocks"),
        "u": ("side:S,depth>=3", "side:N,depth>=3"),
        "v": ("side:W,depth>=3", "side:E,depth>=3"),
        "w": ("depth>=3", "corner_blocks"),
        "uc": ("all",),
        "vc": ("all",),
        "ua": ("all",),
        "va": ("all",),
        "omga": ("all",),
    },
    "d_sw": {
        "delp": ("corner_blocks",),
        "pt": ("corner_blocks",),
        "u": ("corner_blocks",),
        "v": ("corner_blocks",),
        "w": ("corner_blocks",),
        "uc": ("corner_blocks",),
        "vc": ("corner_blocks",),
        "ua": ("depth>=2", "corner_blocks"),
        "va": ("depth>=2", "corner_blocks"),
        "divgd": ("corner_blocks",),
        "mfxd": ("depth>=1",),
        "mfyd": ("depth>=1",),
        "cxd": ("diagonal", "side:W,depth>=1", "side:E,depth>=1"),
        "cyd": ("diagonal", "side:S,depth>=1", "side:N,depth>=1"),
        "q_con": ("corner_blocks",),
        "heat_source": ("depth>=1",),
    },
    "del2_cubed": {
        "q": ("corner_blocks",),
    },
    "edge_pe": {
        "pe": ("depth>=1",),
        "delp": ("depth>=2", "corner_blocks"),
    },
    "fv_tp_2d_hord5": {
        "q": ("corner_blocks",),
        "crx": ("diagonal", "side:W,depth>=1", "side:E,depth>=1"),
        "cry": ("diagonal", "side:S,depth>=1", "side:N,depth>=1"),
        "xfx": ("diagonal", "side:W,depth>=1", "side:E,depth>=1"),
        "yfx": ("diagonal", "side:S,depth>=1", "side:N,depth>=1"),
        "mfx": ("depth>=1",),
        "mfy": ("depth>=1",),
        "mass": ("depth>=2", "diagonal"),
    },
    "fv_tp_2d_hord5_plain": {
        "q": ("corner_blocks",),
        "crx": ("diagonal", "side:W,depth>=1", "side:E,depth>=1"),
        "cry": ("diagonal", "side:S,depth>=1", "side:N,depth>=1"),
        "xfx": ("diagonal", "side:W,depth>=1", "side:E,depth>=1"),
        "yfx": ("diagonal", "side:S,depth>=1", "side:N,depth>=1"),
    },
    "fv_tp_2d_hord6": {
        "q": ("corner_blocks",),
        "crx": ("diagonal", "side:W,depth>=1", "side:E,depth>=1"),
        "cry": ("diagonal", "side:S,depth>=1", "side:N,depth>=1"),
        "xfx": ("diagonal", "side:W,depth>=1", "side:E,depth>=1"),
        "yfx": ("diagonal", "side:S,depth>=1", "side:N,depth>=1"),
        "mfx": ("depth>=1",),
        "mfy": ("depth>=1",),
        "mass": ("depth>=2", "diagonal"),
    },
    "fv_tp_2d_hord6_plain": {
        "q": ("corner_blocks",),
        "crx": ("diagonal", "side:W,depth>=1", "side:E,depth>=1"),
        "cry": ("diagonal", "side:S,depth>=1", "side:N,depth>=1"),
        "xfx": ("diagonal", "side:W,depth>=1", "side:E,depth>=1"),
        "yfx": ("diagonal", "side:S,depth>=1", "side:N,depth>=1"),
    },
    "fxadv": {
        "uc": ("corner_blocks",),
        "vc": ("corner_blocks",),
    },
    "nh_p_grad": {
        "u": ("depth>=1",),
        "v": ("depth>=1",),
        "pp": ("depth>=3", "corner_blocks"),
        "gz": ("depth>=3", "corner_blocks"),
        "pk3": ("depth>=3", "corner_blocks"),
        "delp": ("depth>=3", "corner_blocks"),
    },
    "p_grad_c": {
        "uc": ("depth>=1",),
        "vc": ("depth>=1",),
        "delpc": ("depth>=2", "diagonal"),
        "pkc": ("depth>=2", "diagonal"),
        "gz": ("depth>=2", "diagonal"),
    },
    "pk3_halo": {
        "pk3": ("depth>=1",),
        "delp": ("depth>=3",),
    },
    "ray_fast": {
        "u": ("depth>=1",),
        "v": ("depth>=1",),
        "w": ("depth>=1",),
    },
    "riem_solver3": {
        "cappa": ("depth>=1",),
        "zs": ("depth>=1",),
        "ws": ("depth>=1",),
        "delz": ("depth>=1",),
        "q_con": ("depth>=1",),
        "delp": ("depth>=1",),
        "pt": ("depth>=1",),
        "zh": ("depth>=1",),
        "pe": ("all",),
        "ppe": ("all",),
        "pk3": ("all",),
        "pk": ("all",),
        "peln": ("all",),
        "w": ("depth>=1",),
    },
    "riem_solver_c": {
        "cappa": ("depth>=2", "corner_blocks"),
        "phis": ("depth>=2", "corner_blocks"),
        "ws": ("depth>=2", "corner_blocks"),
        "ptc": ("depth>=2", "corner_blocks"),
        "q_con": ("depth>=2", "corner_blocks"),
        "delpc": ("depth>=2", "corner_blocks"),
        "gz": ("depth>=2", "corner_blocks"),
        "pef": ("all",),
        "w3": ("depth>=2", "corner_blocks"),
    },
    "update_dz_c": {
        "zs": ("depth>=2", "corner_blocks"),
        "ut": ("depth>=2", "corner_blocks"),
        "vt": ("depth>=2", "corner_blocks"),
        "gz": ("depth>=3", "corner_blocks"),
        "ws": ("all",),
    },
    "update_dz_d": {
        "zs": ("depth>=1",),
        "zh": ("corner_blocks",),
        "crx": ("diagonal", "side:W,depth>=1", "side:E,depth>=1"),
        "cry": ("diagonal", "side:S,depth>=1", "side:N,depth>=1"),
        "xfx": ("diagonal", "side:W,depth>=1", "side:E,depth>=1"),
        "yfx": ("diagonal", "side:S,depth>=1", "side:N,depth>=1"),
        "ws": ("all",),
    },
}

# fields any cell of which the LIBRARY may change, with the place that says so
WORK = {
    "d_sw": {
        "delpc": "include/fv3_mi355x.h, fv3_d_sw: delpc is the work array of the divergence damping (the reference's argument of that name)",
        "uc": "INTEGRATION.md, 'C-grid winds after d_sw' / 'the reference's d_sw uses uc/vc as work arrays ... unchanged except in the 12 x 12 windows at cube corners'",
        "vc": "INTEGRATION.md, 'C-grid winds after d_sw' / 'the reference's d_sw uses uc/vc as work arrays ... unchanged except in the 12 x 12 windows at cube corners'",
    },
}
# fields the ORACLE changes outside the compared region beyond its corner fills: whole-array numpy evaluates an intermediate on a wider range than
# the loop that stores it in the Fortran original, or the reference works in place (observed with the cross-check of check_oracle, all shapes)
ORACLE_WORK = {
    "d_sw": ("delpc", "uc", "vc", "divgd"),  # the work arrays of the divergence damping; divgd: the iterated divergence on the halo corners it still needs
    "c_sw": ("uc", "vc", "ua", "va"),  # d2a2c_vect forms the A- and C-grid winds on the halo rows the later stages read
    "fxadv": ("ut", "vt"),  # the contravariant winds on the rows / columns beside the faces of crx / cry
    "nh_p_grad": ("pp", "gz", "pk3"),  # "the reference's nh_p_grad interpolates pp/pk3/gz to corners in place"
    "del2_cubed": ("q",),  # the iterations before the last work on a domain one / two cells wider
}
# fields the LIBRARY may change wherever the oracle changes them ("Read and write footprints of the
# stand-alone operator entries": these operators store an intermediate on the halo rows a later stage or operator reads, as the reference does)
REFERENCE_WRITES = {"c_sw": ("uc", "vc", "ua", "va"), "fxadv": ("ut", "vt"), "del2_cubed": ("q",)}
# outputs the oracle RETURNS as new arrays (the adapters copy them whole): no in-place change to cross-check
RETURNED = {"c_sw": ("delpc", "ptc"), "a2b_ord4": ("qout",), "fv_tp_2d": ("fx", "fy")}


# ---------------------------------------------------------------------------------------------------------------------------
# set-ups: everything one case needs, per operator
# ---------------------------------------------------------------------------------------------------------------------------
class Setup:
    """names: the operator's field arguments in ABI order; kind[name]: 'L' (cell levels: the oracle sees nz levels, the storage has the
    pad level), 'I' (nz + 1 interfaces) or '2' (2-D); ins[r][name]: the oracle-shaped input (None: not read on entry);
    lib(F): the library call on {name: fref}; oracle(r, A): the oracle in place on {name: array}; out[name]: mask function of the
    compared region, or (mask function, first level)"""

    def __init__(self, op, doms, sf, nz, names, kind, ins, lib, oracle, out, cfg=None):
        self.op, self.doms, self.sf, self.nz, self.names, self.kind, self.ins, self.lib, self.oracle, self.out, self.cfg = op, doms, sf, nz, list(names), kind, ins, lib, oracle, out, cfg
        self.oracle_wrote = {}
        self.table = {n: tuple(TABLES.get(op, {}).get(n, ())) for n in self.names}
        for n in self.names:
            if ins[0][n] is None:
                self.table[n] = ("all",)

    def out_of(self, name):
        o = self.out[name]
        return o if isinstance(o, tuple) else (o, 0)

    def oshape(self, r, name):
        D = self.doms[r]
        if self.ins[r][name] is not None:
            return self.ins[r][name].shape
        return D.shape2() + ((self.nz,) if self.kind[name] == "L" else (self.nz + 1,) if self.kind[name] == "I" else ())


@contextlib.contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _shapes():
    import test_horizontal_operator_edges as the

    return the.SHAPES


def _hcase(shape, backend, dtype, cfg_kw):
    n, layout, ranks, seg, nz = _shapes()[shape]
    return Case(n, layout, ranks, nz=nz, backend=backend, cfg_kw=dict(n_split=1, **(cfg_kw or {})), dtype=dtype)


def seg_of(shape):
    return _shapes()[shape][3] if shape in _shapes() else REC_SHAPES[shape][4]


def _assert_both_signs_on_every_tile_edge(cs, ins):
    """the assertion of test_horizontal_operator_edges.test_fxadv_on_strong_winds_matches_the_oracle, on the oracle's fxadv"""
    import test_horizontal_operator_edges as the

    counts = []
    for m in (o_dsw, o_csw, o_ppm):
        m.enable_counters(True)
    try:
        for D, x in zip(cs.doms, ins):
            the._reset()
            o_dsw.fxadv(D, x["uc"].copy(), x["vc"].copy(), *[np.zeros_like(x["uc"]) for _ in range(6)], DT)
            counts.append(the._counted())
    finally:
        for m in (o_dsw, o_csw, o_ppm):
            m.enable_counters(False)
    the.edges_two_sided(cs, counts, the.FXADV_EDGES)
    top, both = hc.max_courant(cs, ins, DT)
    assert 0.5 <= top <= 0.9 and both, (top, both)


def setup_d_sw(shape, backend, dtype, cfg_kw):
    cs = _hcase(shape, backend, dtype, cfg_kw)
    strong = hc.strong(cs, DT)
    _assert_both_signs_on_every_tile_edge(cs, strong)
    names = hc.D_SW_ARGS
    rng = np.random.default_rng(3)
    ins = []
    for x in strong:
        d = {n: x[n] if n in hc.D_SW_IN else None for n in names}
        for n in ("heat_source", "mfxd", "mfyd", "cxd", "cyd"):  # accumulated (zero in the strong family): ordinary magnitude, so that a read-modify-write shows
            d[n] = rng.uniform(1.0, 2.0, x["u"].shape)
        ins.append(d)
    col = o_dsw.get_column_namelist(cs.cfg, cs.nz)

    def oracle(r, A):
        o_dsw.d_sw(cs.doms[r], cs.cfg, col, *[None if n == "zh" else A[n] for n in names], DT)

    return Setup("d_sw", cs.doms, cs.sf, cs.nz, names, dict.fromkeys(names, "L"), ins, lambda F: cs.sf.call("d_sw", *[F[n] for n in names], DT), oracle, DSW_OUT, cs.cfg)


def setup_c_sw(shape, backend, dtype, cfg_kw):
    import test_horizontal_operator_edges as the

    cs = _hcase(shape, backend, dtype, cfg_kw)
    strong = hc.strong_c(cs, DT2)
    names = ("delp", "pt", "u", "v", "w", "uc", "vc", "ua", "va", "ut", "vt", "divgd", "omga", "delpc", "ptc")
    ins = [{n: x[n][:, :, : cs.nz] if n in hc.C_SW_IN else None for n in names} for x in strong]
    counts = {}

    def oracle(r, A):
        for m in (o_dsw, o_csw, o_ppm):
            m.enable_counters(True)
        try:
            the._reset()
            A["delpc"][...], A["ptc"][...] = o_csw.c_sw(cs.doms[r], *[A[n] for n in names[:13]], DT2, nord=cs.cfg.nord)
            counts[r] = the._counted()
        finally:
            for m in (o_dsw, o_csw, o_ppm):
                m.enable_counters(False)

    out = {k: v for k, v in CSW_OUT.items() if not (k == "divgd" and cs.cfg.nord == 0)}
    S = Setup("c_sw", cs.doms, cs.sf, cs.nz, names, dict.fromkeys(names, "L"), ins, lambda F: cs.sf.call("c_sw", *[F[n] for n in names], DT2), oracle, out, cs.cfg)
    S.after_oracle = lambda: the.assert_c_sw_switches(cs, [counts[r] for r in range(len(cs.doms))])
    return S


def setup_fxadv(shape, backend, dtype, cfg_kw):
    cs = _hcase(shape, backend, dtype, cfg_kw)
    strong = hc.strong(cs, DT)
    _assert_both_signs_on_every_tile_edge(cs, strong)
    names = ("uc", "vc", "crx", "cry", "xfx", "yfx", "ut", "vt")
    ins = [{n: x[n] if n in ("uc", "vc") else None for n in names} for x in strong]
    return Setup("fxadv", cs.doms, cs.sf, cs.nz, names, dict.fromkeys(names, "L"), ins, lambda F: cs.sf.call("fxadv", *[F[n] for n in names], DT),
                 lambda r, A: o_dsw.fxadv(cs.doms[r], *[A[n] for n in names], DT), FXADV_OUT, cs.cfg)


def _setup_fv_tp_2d(hord, plain):
    def setup(shape, backend, dtype, cfg_kw):
        cs = _hcase(shape, backend, dtype, cfg_kw)
        strong = hc.strong(cs, DT)
        _assert_both_signs_on_every_tile_edge(cs, strong)
        names = ("q", "crx", "cry", "xfx", "yfx", "fx", "fy") + (() if plain else ("mfx", "mfy", "mass"))
        ins, ra = [], []
        for D, x in zip(cs.doms, strong):
            f = {k: np.zeros_like(x["uc"]) for k in ("crx", "cry", "xfx", "yfx", "ut", "vt")}
            ra.append(o_dsw.fxadv(D, x["uc"].copy(), x["vc"].copy(), *[f[k] for k in ("crx", "cry", "xfx", "yfx", "ut", "vt")], DT))
            d = {"q": x["pt"].copy(), "crx": f["crx"], "cry": f["cry"], "xfx": f["xfx"], "yfx": f["yfx"], "fx": None, "fy": None}
            if not plain:
                d.update(mfx=f["xfx"] * 1.1, mfy=f["yfx"] * 0.9, mass=x["delp"].copy())
            ins.append(d)

        def lib(F):
            extra = (None, None, None, hord, -1, 0.0) if plain else (F["mfx"], F["mfy"], F["mass"], hord, 2, 0.06)
            cs.sf.call("fv_tp_2d", *[F[n] for n in names[:7]], *extra)

        def oracle(r, A):
            kw = {} if plain else dict(mfx=A["mfx"], mfy=A["mfy"], mass=A["mass"], nord=2, damp_c=0.06)
            A["fx"][...], A["fy"][...] = o_tp.fv_tp_2d(cs.doms[r], A["q"], A["crx"], A["cry"], A["xfx"], A["yfx"], ra[r][0], ra[r][1], hord, **kw)

        return Setup(f"fv_tp_2d_hord{hord}" + ("_plain" if plain else ""), cs.doms, cs.sf, cs.nz, names, dict.fromkeys(names, "L"), ins, lib, oracle, {"fx": V, "fy": U}, cs.cfg)

    return setup


def setup_a2b_ord4(shape, backend, dtype, cfg_kw):
    import test_horizontal_operator_edges as the

    cs = _hcase(shape, backend, dtype, cfg_kw)
    ins = [{"qin": a, "qout": None} for a in the._a2b_input(cs)]

    def oracle(r, A):
        A["qout"][...] = o_a2b.a2b_ord4(cs.doms[r], A["qin"])

    return Setup("a2b_ord4", cs.doms, cs.sf, cs.nz, ("qin", "qout"), {"qin": "L", "qout": "L"}, ins, lambda F: cs.sf.call("a2b_ord4", F["qin"], F["qout"], 0, cs.nz, 0), oracle,
                 {"qout": CORNERS}, cs.cfg)


# ---- the operators of the recorded oracle sequence (test_operator_parity.recorded): arguments by position
# name: (shape, cells per tile, layout, ranks, FV3_SEG, levels)
REC_SHAPES = {"c12_2x2": (12, (2, 2), (0, 5, 10, 15), 8, None), "c24_2x2": (24, (2, 2), (0, 5, 10, 15), 8, "8"), "c48_3x1": (48, (3, 1), (0, 1, 2), 8, None),
              "c12_L79": (12, (1, 1), (0, 1, 2, 3, 4, 5), 79, None)}
_REC = {}


def recorded_calls(shape, cfg_kw=None):
    """one recorded oracle call (n_split = 1) on the whole cube of ``shape``: (cfg, grids, calls[name][rank])"""
    import test_operator_parity as top
    from helpers import oracle_cube

    n, layout, ranks, nz, _ = REC_SHAPES[shape]
    key = (shape, tuple(sorted((cfg_kw or {}).items())))
    if key not in _REC:
        if n == 12 and not cfg_kw:
            _, cfg, grids, calls, _ = top.recorded(layout, nz)
        else:
            _, cfg, grids, ost, _, odyn = oracle_cube(n, layout, nz, dict(n_split=1, **(cfg_kw or {})))
            with top.Recorder() as rec, np.errstate(all="ignore"):
                odyn(ost, 225.0, 1)
            calls = rec.calls
        _REC[key] = (cfg, grids, calls)
    return _REC[key]


# operator: (oracle function, {field: position in the oracle's arguments after D}, library call on (sf, F, a), outputs)
REC_OPS = {
    "update_dz_c": ("update_dz_c", dict(zs=1, ut=2, vt=3, gz=4, ws=5), lambda sf, F, a: sf.call("update_dz_c", F["zs"], F["ut"], F["vt"], F["gz"], F["ws"], float(a[6])), {"gz": RING1, "ws": RING1}),
    "riem_solver_c": ("riem_solver_c", dict(cappa=1, phis=3, ws=4, ptc=5, q_con=6, delpc=7, gz=8, pef=9, w3=10),
                      lambda sf, F, a: sf.call("riem_solver_c", float(a[0]), F["cappa"], float(a[2]), *[F[n] for n in ("phis", "ws", "ptc", "q_con", "delpc", "gz", "pef", "w3")]), {"gz": RING1, "pef": RING1}),
    "p_grad_c": ("p_grad_c", dict(uc=2, vc=3, delpc=4, pkc=5, gz=6), lambda sf, F, a: sf.call("p_grad_c", *[F[n] for n in ("uc", "vc", "delpc", "pkc", "gz")], float(a[7])), {"uc": V, "vc": U}),
    "update_dz_d": ("update_dz_d", dict(zs=3, zh=4, crx=5, cry=6, xfx=7, yfx=8, ws=9), lambda sf, F, a: sf.call("update_dz_d", *[F[n] for n in ("zs", "zh", "crx", "cry", "xfx", "yfx", "ws")], float(a[10])),
                    {"zh": CELLS, "ws": CELLS}),
    "riem_solver3": ("riem_solver3", dict(cappa=2, zs=4, ws=5, delz=6, q_con=7, delp=8, pt=9, zh=10, pe=11, ppe=12, pk3=13, pk=14, peln=15, w=16),
                     lambda sf, F, a: sf.call("riem_solver3", int(bool(a[0])), float(a[1]), F["cappa"], float(a[3]), *[F[n] for n in ("zs", "ws", "delz", "q_con", "delp", "pt", "zh", "pe", "ppe", "pk3", "pk", "peln", "w")]),
                     dict.fromkeys(("w", "delz", "zh", "ppe", "pk3", "pe", "pk", "peln"), CELLS)),
    "pk3_halo": ("pk3_halo", dict(pk3=0, delp=1), lambda sf, F, a: sf.call("pk3_halo", F["pk3"], F["delp"], float(a[2]), float(a[3])), {"pk3": (RING2, 1)}),
    "edge_pe": ("pe_halo", dict(pe=0, delp=1), lambda sf, F, a: sf.call("edge_pe", F["pe"], F["delp"], float(a[2])), {"pe": RING1}),
    "nh_p_grad": ("nh_p_grad", dict(u=0, v=1, pp=2, gz=3, pk3=4, delp=5), lambda sf, F, a: sf.call("nh_p_grad", *[F[n] for n in ("u", "v", "pp", "gz", "pk3", "delp")], float(a[6]), float(a[7]), float(a[8])),
                  {"u": U, "v": V}),
    "ray_fast": ("ray_fast", dict(u=1, v=2, w=3), lambda sf, F, a: sf.call("ray_fast", F["u"], F["v"], F["w"], float(a[6]), float(a[7])), {"u": U, "v": V, "w": CELLS}),
    "del2_cubed": ("del2_cubed", dict(q=0), lambda sf, F, a: sf.call("del2_cubed", F["q"], float(a[1]), 3), {"q": CELLS}),
    "apply_diffusive_heating": ("apply_diffusive_heating", dict(delp=0, delz=1, cappa=2, heat_source=3, pt=4),
                                lambda sf, F, a: sf.call("apply_diffusive_heating", *[F[n] for n in ("delp", "delz", "cappa", "heat_source", "pt")], float(a[5])), {"pt": CELLS}),
}


def _setup_recorded(op):
    fn_name, pos, lib, out = REC_OPS[op]

    def setup(shape, backend, dtype, cfg_kw):
        n, layout, ranks, nz, _ = REC_SHAPES[shape]
        cfg, grids, calls = recorded_calls(shape, cfg_kw)
        cl = [calls[fn_name][r] for r in ranks]
        sf = stencil_factory_for(backend)([grids[r] for r in ranks], cfg, get_constants(), dtype=dtype)
        doms = [c["D"] for c in cl]
        names = list(pos)
        a0 = cl[0]["ins"]
        kind = {}
        for nme, i in pos.items():
            a = np.asarray(a0[i])
            kind[nme] = "2" if a.ndim == 2 or a.shape[2] == 1 else "L" if a.shape[2] == nz else "I"
        ins = [{nme: np.array(c["ins"][i], dtype=np.float64) for nme, i in pos.items()} for c in cl]
        if op == "ray_fast":
            assert max(np.abs(c["outs"][1] - c["ins"][1]).max() for c in cl) > 0.0, "the recorded case does not exercise the Rayleigh layer"
        if op == "del2_cubed":
            assert max(np.abs(c["ins"][0]).max() for c in cl) > 0.0

        def oracle(r, A):
            args = list(cl[r]["ins"])
            for nme, i in pos.items():
                args[i] = A[nme]
            getattr(o_nh, fn_name)(doms[r], *args, **({"nmax": 3} if op == "del2_cubed" and len(args) < 3 else {}))

        return Setup(op, doms, sf, nz, names, kind, ins, lambda F: lib(sf, F, a0), oracle, out, cfg)

    return setup


SETUPS = {"d_sw": setup_d_sw, "c_sw": setup_c_sw, "fxadv": setup_fxadv, "a2b_ord4": setup_a2b_ord4}
for _h in (5, 6):
    SETUPS[f"fv_tp_2d_hord{_h}"] = _setup_fv_tp_2d(_h, False)
    SETUPS[f"fv_tp_2d_hord{_h}_plain"] = _setup_fv_tp_2d(_h, True)
for _op in REC_OPS:
    SETUPS[_op] = _setup_recorded(_op)
HORIZONTAL = ("d_sw", "c_sw", "fxadv", "a2b_ord4", "fv_tp_2d_hord5", "fv_tp_2d_hord6", "fv_tp_2d_hord5_plain", "fv_tp_2d_hord6_plain")


def make(op, shape, backend, dtype=torch.float64, cfg_kw=None):
    S = SETUPS[op](shape, backend, dtype, cfg_kw)
    for n in S.names:  # ``pad`` for every cell-level 3-D input
        if S.kind[n] == "L" and "all" not in S.table[n]:
            S.table[n] = S.table[n] + ("pad",)
    return S


# ---------------------------------------------------------------------------------------------------------------------------
# host side: oracle-shaped arrays, poisoned or clean
# ---------------------------------------------------------------------------------------------------------------------------
def _prefill(S, r, name):
    """a field that is not read on entry: finite values of ordinary magnitude that differ from element to element"""
    rng = np.random.default_rng(1000 * (r + 1) + S.names.index(name))
    return rng.uniform(1.0, 2.0, S.oshape(r, name))


def hmask(S, r, name, specs):
    m = np.zeros(S.doms[r].shape2(), dtype=bool)
    for spec in specs:
        if spec not in ("pad", "all"):
            m |= region(S.doms[r], name, spec)
    return m


def host_inputs(S, r, poisoned, table=None):
    """{name: oracle-shaped array} of rank r; poisoned: NaN in every horizontal region of the table, on every level"""
    table = S.table if table is None else table
    A = {}
    for n in S.names:
        a = S.ins[r][n]
        a = _prefill(S, r, n) if a is None else np.array(a, dtype=np.float64)
        if poisoned:
            if "all" in table[n]:
                a[...] = np.nan
            else:
                a[hmask(S, r, n, table[n])] = np.nan
        A[n] = a
    return A


def to_storage(S, name, a, poisoned, table=None):
    """oracle-shaped array -> the (i, j[, k]) contents of the library's storage: the pad level of a cell-level field is a copy of
    level nz - 1 (as in test_operator_parity.Dev.q), NaN when poisoned"""
    table = S.table if table is None else table
    if S.kind[name] == "2":
        return a.reshape(a.shape[0], a.shape[1])
    if S.kind[name] == "I":
        return a
    pad = a[:, :, -1:].copy()
    if poisoned and ("pad" in table[name] or "all" in table[name]):
        pad[...] = np.nan
    return np.concatenate([a, pad], axis=2)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def oracle_pair(S, r, table=None):
    """(inputs before, clean after, poisoned after) of the oracle on rank r"""
    with np.errstate(all="ignore"):
        before = host_inputs(S, r, False, table)
        clean = {k: v.copy() for k, v in before.items()}
        S.oracle(r, clean)
        dirty = host_inputs(S, r, True, table)
        S.oracle(r, dirty)
    return before, clean, dirty


def out_region(S, r, name, a):
    """the compared cells of output ``name`` in an oracle-shaped (or storage-shaped) array: levels first .. nz - 1 (cell levels) or .. nz"""
    mask, k0 = S.out_of(name)
    m = mask(S.doms[r])
    if a.ndim == 2 or S.kind[name] == "2":
        return a.reshape(a.shape[0], a.shape[1])[m]
    k1 = S.nz if S.kind[name] == "L" else S.nz + 1
    return a[m][:, k0:k1]


def check_oracle(S, msgs):
    """the table is honest (the oracle gives the same, finite bits with all of it poisoned at once), it is not vacuous (every named region
    is non-empty on some rank), and the oracle itself changes nothing outside the compared regions but its in-place corner fills"""
    for n, specs in S.table.items():
        for spec in specs:
            if spec in ("pad", "all"):
                continue
            if not any(region(D, n, spec).any() for D in S.doms):
                msgs.append(f"table: region {spec} of {n} is empty on every rank of the case")
    for r, D in enumerate(S.doms):
        before, clean, dirty = oracle_pair(S, r)
        for n in S.out:
            a, b = out_region(S, r, n, clean[n]), out_region(S, r, n, dirty[n])
            if not np.all(np.isfinite(a)):
                msgs.append(f"oracle {n} rank {r}: not finite on the compared region")
            if not same(a, b):
                msgs.append(f"oracle {n} rank {r}: {int((bits(a) != bits(b)).sum())} compared cells depend on the poison table: the table names a cell the oracle reads")
        for n in S.names:
            ch = bits(before[n]) != bits(clean[n])
            ch = ch.reshape(ch.shape[0], ch.shape[1], -1).any(axis=2)
            S.oracle_wrote[r, n] = ch
            if n in ORACLE_WORK.get(S.op, ()) or n in RETURNED.get(S.op[:8], ()):
                continue
            allowed = S.out_of(n)[0](D) if n in S.out else np.zeros(D.shape2(), dtype=bool)
            allowed = allowed | region(D, n, "corner_blocks") | (C1(D) & ~RING1(D))
            if (ch & ~allowed).any():
                ii, jj = np.nonzero(ch & ~allowed)
                msgs.append(f"oracle {n} rank {r}: changes {len(ii)} columns outside the compared region and the corner fills, e.g. (i, j) = {(int(ii[0]) - D.o, int(jj[0]) - D.o)}")
    if hasattr(S, "after_oracle"):
        S.after_oracle()


# ---------------------------------------------------------------------------------------------------------------------------
# device side: guarded fields, three calls
# ---------------------------------------------------------------------------------------------------------------------------
class Guarded:
    """a Quantity over buf[G : G + n].view(shape) with guard bands of one fixed bit pattern on either side"""

    def __init__(self, sf, two_d):
        qf = sf.quantity_factory
        ni, nj, nk = qf.sizer.storage_shape
        shape = (qf.sizer.n_sub, nj, ni) if two_d else (qf.sizer.n_sub, nk, nj, ni)
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * GUARD,), GUARD_VALUE, dtype=qf.dtype, device=qf.device)
        self.n = n
        self.q = Quantity(self.buf[GUARD : GUARD + n].view(shape), ("x", "y") if two_d else ("x", "y", "z"), n_halo=qf.sizer.n_halo)
        assert self.q.storage.data_ptr() == self.buf.data_ptr() + GUARD * self.buf.element_size()
        self.pattern = bits(self.buf[:1].cpu().numpy())[0]

    def guards_intact(self):
        b = bits(self.buf.cpu().numpy())
        return bool(np.all(b[:GUARD] == self.pattern) and np.all(b[GUARD + self.n :] == self.pattern))

    def host(self, r):
        """(i, j[, k]) copy of the whole storage of sub-domain r"""
        return self.q.numpy(r)


def library_call(S, G, poisoned, backend):
    """upload, call, download: ([{name: storage before}], [{name: storage after}]) per rank"""
    for r in range(len(S.doms)):
        A = host_inputs(S, r, poisoned)
        for n in S.names:
            G[n].q.set_numpy(to_storage(S, n, A[n], poisoned), r)
    before = [{n: G[n].host(r) for n in S.names} for r in range(len(S.doms))]
    S.lib({n: G[n].q.fref for n in S.names})
    if backend != "hostemu":
        torch.cuda.synchronize()
    after = [{n: G[n].host(r) for n in S.names} for r in range(len(S.doms))]
    return before, after, [n for n in S.names if not G[n].guards_intact()]


def allowed_writes(S, r, name, shape):
    """the cells of the storage the library may change: the compared region on levels 0 .. nz - 1 (interfaces: 0 .. nz); of a ring-1 output
    the whole rectangle (the cube-corner halo cell holds no defined value); of REFERENCE_WRITES also where the oracle changes the field"""
    m = np.zeros(shape, dtype=bool)
    h = np.zeros(S.doms[r].shape2(), dtype=bool)
    if name in S.out:
        mask = S.out_of(name)[0]
        h |= C1(S.doms[r]) if mask is RING1 else mask(S.doms[r])
    if name in REFERENCE_WRITES.get(S.op, ()):
        h |= S.oracle_wrote[r, name]
    if len(shape) == 2:
        m |= h
    else:
        m[:, :, : S.nz if S.kind[name] == "L" else S.nz + 1] = h[:, :, None]
    return m


def _where(D, m):
    idx = np.argwhere(m)
    lo, hi = idx.min(axis=0), idx.max(axis=0)
    f = lambda v: [int(v[0]) - D.o, int(v[1]) - D.o] + [int(x) for x in v[2:]]  # noqa: E731
    return f"{len(idx)} cells, (i, j[, k]) from {f(lo)} to {f(hi)}"


def check_library(S, backend, msgs):
    G = {n: Guarded(S.sf, S.kind[n] == "2") for n in S.names}
    b1, a1, g1 = library_call(S, G, False, backend)
    _, a2, g2 = library_call(S, G, True, backend)
    _, a3, g3 = library_call(S, G, False, backend)
    for call, bad in (("clean", g1), ("poisoned", g2), ("second clean", g3)):
        if bad:
            msgs.append(f"guard bands overwritten by the {call} call: {bad}")
    for r, D in enumerate(S.doms):
        for n in S.out:
            a, b = out_region(S, r, n, a1[r][n]), out_region(S, r, n, a2[r][n])
            if not np.all(np.isfinite(a)):
                msgs.append(f"{n} rank {r}: the clean call is not finite on the compared region")
            if not same(a, b):
                mask, k0 = S.out_of(n)
                x, y = a1[r][n], a2[r][n]
                d = (bits(x) != bits(y)) & allowed_writes(S, r, n, x.shape)
                if x.ndim == 3:
                    d[:, :, :k0] = False
                msgs.append(f"{n} rank {r}: the poisoned call differs from the clean one on the compared region ({_where(D, d)}; not finite: {int((~np.isfinite(b)).sum())}): a cell of the poison table is read")
        for n in S.names:
            if not same(a1[r][n], a3[r][n]):
                msgs.append(f"{n} rank {r}: the third call differs from the first ({_where(D, bits(a1[r][n]) != bits(a3[r][n]))}): state kept between calls")
            if n in WORK.get(S.op, {}):
                continue
            wrote = (bits(b1[r][n]) != bits(a1[r][n])) & ~allowed_writes(S, r, n, a1[r][n].shape)
            if wrote.any():
                msgs.append(f"{n} rank {r}: written outside the allowed set ({_where(D, wrote)})")
        if S.op == "nh_p_grad":
            for n in ("pp", "gz", "pk3"):
                if not same(b1[r][n], a1[r][n]):
                    msgs.append(f"nh_p_grad changed its input {n} on rank {r}")


def run_case(op, shape, backend, dtype=torch.float64, cfg_kw=None):
    """one case: the oracle's validation of the table, then the three library calls; raises AssertionError with every finding"""
    with env(FV3_SEG=seg_of(shape)):
        S = make(op, shape, backend, dtype, cfg_kw)
        msgs = []
        check_oracle(S, msgs)
        assert not msgs, f"{op} {shape}: the oracle side fails before the library is called:\n  " + "\n  ".join(msgs)
        check_library(S, backend, msgs)
        assert not msgs, f"{op} {shape} on {backend}:\n  " + "\n  ".join(msgs)
    return S


# ---------------------------------------------------------------------------------------------------------------------------
# discovery (run by hand): which regions of which input does the oracle not need?
# ---------------------------------------------------------------------------------------------------------------------------
def discover(op, shapes):
    accepted = None
    for shape in shapes:
        with env(FV3_SEG=seg_of(shape)):
            S = make(op, shape, "hostemu")
        found = {}
        for n in S.names:
            if S.ins[0][n] is None:
                continue
            have = []
            for spec in CANDIDATES:
                if _implied(spec, have):
                    continue
                if spec != "all" and not any(region(D, n, spec).any() for D in S.doms):
                    continue
                table = {m: (("all",) if S.ins[0][m] is None else ()) for m in S.names}
                table[n] = (spec,)
                ok = True
                for r in range(len(S.doms)):
                    _, clean, dirty = oracle_pair(S, r, table)
                    for o in S.out:
                        a, b = out_region(S, r, o, clean[o]), out_region(S, r, o, dirty[o])
                        ok = ok and same(a, b) and bool(np.all(np.isfinite(a)))
                    if not ok:
                        break
                if ok:
                    have.append(spec)
            found[n] = have
        print(f"# {op} {shape}: {found}", file=sys.stderr)
        if accepted is None:
            accepted = found
        else:  # a region stays when every shape accepts it or a region that contains it
            accepted = {n: [s for s in set(accepted[n]) | set(found[n]) if _implied_or_in(s, accepted[n]) and _implied_or_in(s, found[n])] for n in accepted}
    accepted = {n: tuple(s for s in CANDIDATES if s in v and not _implied(s, [x for x in v if x != s])) for n, v in accepted.items() if v}
    print(f'TABLES["{op}"] = {accepted!r}')
    return accepted


def _implied_or_in(spec, have):
    return spec in have or _implied(spec, have)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--discover", nargs="+", metavar=("OP", "SHAPE"))
    ap.add_argument("--run", nargs=2, metavar=("OPS", "SHAPES"))
    ap.add_argument("--backend", default="hostemu")
    a = ap.parse_args(argv)
    if a.discover:
        op, shapes = a.discover[0], a.discover[1:]
        from pace_amd import build

        build.build(64, hostemu=True, verbose=False)
        discover(op, shapes or SHAPES_OF(op))
        return 0
    ops, shapes = a.run
    from pace_amd import build, lib

    if a.backend == "hostemu":
        build.build(64, hostemu=True, verbose=False)
    else:
        lib.load(64)
    for shape in shapes.split(","):
        for op in ops.split(","):
            run_case(op, shape, a.backend)
            if a.backend != "hostemu":
                torch.cuda.synchronize()
            print(f"footprint case {op} {shape} on {a.backend}: passed", flush=True)
    return 0


H_SHAPES = ("c12_2x2", "c24_2x2", "c72_3x3", "c48_3x1")
COLUMN_SHAPES = ("c12_2x2", "c48_3x1")


def SHAPES_OF(op):
    return H_SHAPES if op in HORIZONTAL else ("c12_L79",) if op == "ray_fast" else COLUMN_SHAPES


if __name__ == "__main__":
    sys.exit(main())
