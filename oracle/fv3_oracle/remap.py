"""ORACLE (test infrastructure, never the shipped path) -- ctypes wrapper of oracle/remap_oracle.c, the plain-C restatement of
the Lagrangian-to-Eulerian vertical remapping (pyFV3 ``LagrangianToEulerian``; see the header of the C file for the reference
evidence and what is restated).  ``build_lib()`` compiles it with gcc into oracle/_build/ (git-ignored; it travels to the GPU
box like the other built libraries)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import Dict, List, Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(os.path.dirname(_HERE), "remap_oracle.c")
_OUT = os.path.join(os.path.dirname(_HERE), "_build", "libremap_oracle.so")
_lib = None


class _Geom(C.Structure):
    _fields_ = [(n, C.c_int) for n in "ni nj nz nh nx ny".split()] + [(n, C.c_double) for n in "ptop akap rrg t_min".split()]


def build_lib(force: bool = False) -> str:
    if force or not os.path.exists(_OUT) or os.path.getmtime(_OUT) < os.path.getmtime(_SRC):
        os.makedirs(os.path.dirname(_OUT), exist_ok=True)
        subprocess.run(["gcc", "-O2", "-std=c99", "-ffp-contract=off", "-shared", "-fPIC", "-o", _OUT, _SRC, "-lm"], check=True)
    return _OUT


def _load():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build_lib())
        _lib.remap_one.argtypes = [C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.c_double, C.c_int, C.c_double]
        _lib.remap_rank.argtypes = [C.POINTER(_Geom)] + [C.c_void_p] * 15 + [C.c_int, C.c_void_p]
        _lib.remap_counters_enable.argtypes = [C.c_int]
        _lib.remap_counters.argtypes = [C.c_void_p]
        _lib.remap_counters.restype = C.c_int
    return _lib


# names of the oracle's branch counters, in the order of the C enum (remap_oracle.c, RC_*)
COUNTERS = ("iv0_nonpos", "iv0_negmin_flat", "iv0_negmin_top", "iv0_negmin_bot", "iv12_flat", "iv12_a6da_lo", "iv12_a6da_hi", "constrain_iv0",
            "top_iv0", "top_ivm1", "bot_iv0", "bot_ivm1", "flat_2dz", "flat_qmin", "span3")


def enable_counters(on: bool = True) -> None:
    """Count the limiter branches the oracle takes (tests only; off by default, never changes a result)."""
    _load().remap_counters_enable(int(bool(on)))


def reset_counters() -> None:
    _load().remap_counters_reset()


def counters() -> Dict[str, int]:
    """Branch counts since the last reset: cs_limiters iv = 0 (mean <= 0; negative local minimum: flat / refit from the top / from
    the bottom edge) and iv = 1 / 2 (flat; a6da < -da2; a6da > da2), the iv = 0 large-scale constraint clamping an edge to 0, the
    top / bottom edge clamps for iv = 0 and iv = -1, interior flattening as a 2-delta-z wave and by the qmin clause alone, and
    target layers that cover 3 or more source layers."""
    lib = _load()
    out = (C.c_long * lib.remap_counters(None))()
    lib.remap_counters(C.cast(out, C.c_void_p))
    return dict(zip(COUNTERS, (int(x) for x in out)))


def _p(a):
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"], "oracle arrays are contiguous float64 [i, j, k]"
    return a.ctypes.data_as(C.c_void_p)


def remap_column(pe1, q1, pe2, iv=1, qs=0.0, qmin: Optional[float] = None):
    """map1_ppm / map_scalar of one column: layer means q1 on interfaces pe1 -> interfaces pe2 (kord 9)."""
    pe1, q1, pe2 = (np.ascontiguousarray(x, dtype=np.float64) for x in (pe1, q1, pe2))
    q2 = np.zeros_like(q1)
    _load().remap_one(len(q1), _p(pe1), _p(q1), _p(pe2), _p(q2), int(iv), float(qs), int(qmin is not None), float(qmin or 0.0))
    return q2


def lagrangian_to_eulerian(D, consts, state: Dict[str, np.ndarray], wsd: np.ndarray, tracers: Optional[List[np.ndarray]] = None, t_min: float = 184.0):
    """One rank, in place: delp, pt, delz, w, u, v, tracers remapped to the Eulerian levels ak + bk * ps; pe, peln, pk, pkz rebuilt;
    returns ps [i, j].  ``state`` holds the oracle's [i, j, k] arrays (cappa read-only); ``wsd`` [i, j, 1] or [i, j]."""
    g = D.grid
    geo = _Geom(state["delp"].shape[0], state["delp"].shape[1], g.nz, g.n_halo, g.nx, g.ny, float(g.ptop), float(consts.KAPPA), float(-consts.RDGAS / consts.GRAV), float(t_min))
    ak, bk = np.ascontiguousarray(g.ak, dtype=np.float64), np.ascontiguousarray(g.bk, dtype=np.float64)
    ps = np.zeros(state["delp"].shape[:2])
    ws = np.ascontiguousarray(np.asarray(wsd, dtype=np.float64).reshape(ps.shape))
    tr = tracers or []
    arr = (C.c_void_p * max(len(tr), 1))(*[t.ctypes.data for t in tr])
    _load().remap_rank(C.byref(geo), _p(ak), _p(bk), *[_p(state[n]) for n in ("delp", "pt", "delz", "w", "u", "v", "cappa", "pe", "peln", "pk", "pkz")], _p(ps), _p(ws),
                       len(tr), arr)
    return ps
