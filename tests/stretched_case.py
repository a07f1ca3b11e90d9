"""Stretched (Schmidt-transformed) grids for the tests: the transform of the reference's example configs, a second one, whole cubes with
the oracle beside them, and a switch that makes the case builders of the other test modules build their grids stretched.

The grid is the first one without symmetries: the six tiles differ and no tile is symmetric in itself, so a kernel that read dx for a
transposed dy, or a west-edge coefficient on the east, cannot pass on it by accident.
"""
import contextlib
import functools

import numpy as np

import helpers
from pace_amd import grid as _grid
from pace_amd.config import AcousticDynamicsConfig
from pace_amd.grid import SchmidtTransform, make_grid
from pace_amd.topology import CubedSpherePartitioner

STRETCH = SchmidtTransform(3.0, 172.5, 17.5)  # tropicalcyclone_c128.yaml, tropical_read_restart_fortran.yml
STRETCH_B = SchmidtTransform(1.5, 10.0, -40.0)
N, NZ = 12, 8
REFINED_TILE, COARSE_TILE = 5, 2  # tile 5 is centred on the target, tile 2 lies opposite


def target_vector(stretch):
    lon, lat = np.deg2rad(stretch.lon_target), np.deg2rad(stretch.lat_target)
    return np.array([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)])


@functools.lru_cache(maxsize=None)
def grids(layout=(1, 1), nz=NZ, n=N, stretch=STRETCH):
    """every rank's stretched grid (shared, read-only)"""
    part = CubedSpherePartitioner(n, tuple(layout))
    return part, tuple(make_grid(part, r, nz=nz, stretch=stretch) for r in range(part.total_ranks))


def stretched_make_grid(stretch=STRETCH):
    def mk(*a, **kw):
        kw.setdefault("stretch", stretch)
        return _grid.make_grid(*a, **kw)

    return mk


@contextlib.contextmanager
def stretched(*modules, stretch=STRETCH):
    """Inside the block the ``make_grid`` that ``modules`` (default: tests/helpers.py -- ``Case``, ``oracle_cube``) hold builds stretched
    grids, so the case builders and comparisons written for the uniform grid run unchanged on the stretched one."""
    modules = modules or (helpers,)
    saved = [(m, m.make_grid) for m in modules]
    for m in modules:
        m.make_grid = stretched_make_grid(stretch)
    try:
        yield
    finally:
        for m, fn in saved:
            m.make_grid = fn


def oracle_cube(layout, nz=NZ, cfg_kw=None, n=N, stretch=STRETCH, seed=7, noise=0.01):
    """``helpers.oracle_cube`` on the stretched grid: (part, cfg, grids, states, phis, OracleAcousticDynamics)"""
    with stretched(stretch=stretch):
        return helpers.oracle_cube(n, tuple(layout), nz, cfg_kw, seed=seed, noise=noise)


def equivalent_d4_bg(g, d4_bg, nord):
    """The d4_bg with which the congruent form (da_min_c d4_bg')^(nord + 1) equals the stretched form da_min d4_bg^(nord + 1)."""
    return (g.da_min * d4_bg ** (nord + 1)) ** (1.0 / (nord + 1)) / g.da_min_c


def config(layout, nz=NZ, n=N, **kw):
    return AcousticDynamicsConfig(**{**dict(npx=n + 1, npy=n + 1, npz=nz, layout=tuple(layout)), **kw})
