"""Writers of the driver diagnostics: ``ZarrMonitor`` and ``NetCDFMonitor``.

The reference driver hands its diagnostics to ``ndsl.monitor.ZarrMonitor`` / ``NetCDFMonitor``
[REF driver/pace/driver/diagnostics.py:101-139].  Those writers are not part of the reference tree this build was restated from (an
un-vendored submodule), and neither ``zarr`` nor ``xarray`` / ``netCDF4`` is a dependency of this package: the ON-DISK LAYOUT BELOW IS
THIS BUILD'S OWN.  It keeps what the reference's configuration promises -- a Zarr v2 directory store that ``zarr`` / ``xarray`` open, or
``state_<chunk>_tile<t>.nc`` files with ``time_chunk_size`` records each -- and needs json, numpy and ``scipy.io.netcdf_file`` only.

Common to both writers

* every variable has the dims ``time, tile, [z | z_interface,] y | y_interface, x | x_interface`` (constants: without ``time``);
* ``time`` is float64 seconds with ``units = "seconds since <start_time>"`` (default 2000-01-01 00:00:00, the reference's);
* ``units`` come from the Quantity;
* a variable arrives as one host array ``[n_sub, (nk,) nj, ni]`` -- the compute domains of the sub-domains this process owns -- and is
  consumed before the next one is produced (``store(time, variables)`` takes an iterator: the caller reuses one staging buffer).

``ZarrMonitor(path, layout)``: Zarr v2 directory store, written by hand

* ``.zgroup`` at the root; ``<name>/.zarray`` (``zarr_format 2``, ``order "C"``, ``compressor null``, ``filters null``,
  ``fill_value "NaN"``, dtype ``<f8`` / ``<f4``, chunks ``(1, 1, [nz_e,] ny_sub, nx_sub)``); ``<name>/.zattrs`` with
  ``_ARRAY_DIMENSIONS`` and ``units``;
* chunk files ``<name>/t.tile[.0].jy.ix``: one chunk per sub-domain, so every process writes the chunks of its own sub-domains and
  nothing is gathered;
* a staggered dimension of length ``n * l + 1`` keeps chunk length ``n``: each sub-domain writes its first ``n`` rows (the interface
  row it shares with its neighbour is the neighbour's first), and the last sub-domain of the tile in that direction also writes the one
  remaining row as the single valid row of an extra chunk whose rest is fill;
* after a record's chunks are written (a ``torch.distributed.barrier()`` when a process group exists) process 0 writes the ``time`` array
  (chunk length 1) and rewrites every ``.zarray`` with the grown time length (temporary name, then rename): a reader never sees a time
  length whose chunks are missing;
* ``store_constant`` writes ``lat``, ``lon``, ``lat_agrid``, ``lon_agrid`` with dims ``tile, y*, x*``.
* a store always starts at record 0 (an existing directory is written over, not appended to).

``NetCDFMonitor(path, layout, time_chunk_size)``: classic netCDF (64-bit offsets) through scipy

* ``state_<chunk:04d>_tile<t>.nc`` holds ``time_chunk_size`` records of every variable on the whole tile (dims as above, ``tile`` of
  length 1 with the tile number as its coordinate); the last file is written partial on ``cleanup``;
* ``constants_tile<t>.nc`` holds the grid constants;
* the records of a file are kept in host memory until it is written, and a tile is assembled by the process that writes it: the format
  is supported when every tile is wholly owned by one process, otherwise the constructor refuses and names ``output_format: zarr`` (the
  reference's documentation has the same warning: the format needs the whole tile on one rank).
"""
from __future__ import annotations

import json
import os
from datetime import datetime, timedelta
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from .constants import X_DIM, X_INTERFACE_DIM, Y_DIM, Y_INTERFACE_DIM, Z_DIM, Z_INTERFACE_DIM

DEFAULT_START_TIME = datetime(2000, 1, 1)
_HORIZONTAL = (X_DIM, X_INTERFACE_DIM, Y_DIM, Y_INTERFACE_DIM)


def as_datetime(t) -> datetime:
    """``start_time`` of a yaml: a datetime (PyYAML parses time stamps), an ISO string, or None (the reference's default)."""
    if t is None:
        return DEFAULT_START_TIME
    if isinstance(t, datetime):
        return t
    return datetime.fromisoformat(str(t))


def storage_dims(dims: Sequence[str]) -> Tuple[str, ...]:
    """Quantity dims ``(x*, y*[, z*])`` -> the dims of the packed array without the leading sub-domain axis: ``([z*,] y*, x*)``."""
    dims = tuple(dims)
    if len(dims) not in (2, 3) or dims[0] not in (X_DIM, X_INTERFACE_DIM) or dims[1] not in (Y_DIM, Y_INTERFACE_DIM) or (len(dims) == 3 and dims[2] not in (Z_DIM, Z_INTERFACE_DIM)):
        raise ValueError(f"monitor: dims {dims} (expected (x | x_interface, y | y_interface[, z | z_interface]))")
    return tuple(reversed(dims))


class _Monitor:
    def __init__(self, path: str, layout, start_time=None):
        self.path = str(path)
        self.layout = layout
        self.part = layout.part
        self.start_time = as_datetime(start_time)
        self.time_units = f"seconds since {self.start_time:%Y-%m-%d %H:%M:%S}"
        os.makedirs(self.path, exist_ok=True)

    def _seconds(self, time) -> float:
        if isinstance(time, datetime):
            return (time - self.start_time).total_seconds()
        if isinstance(time, timedelta):
            return time.total_seconds()
        return float(time)

    def _barrier(self):
        if self.layout.world_size > 1:
            import torch.distributed as dist

            if dist.is_available() and dist.is_initialized():
                dist.barrier(group=getattr(self.layout, "group", None))

    def _check(self, name, a: np.ndarray, dims):
        """(sdims, nk-or-None, staggered y, staggered x) of a packed variable, its shape checked against the layout."""
        sdims = storage_dims(dims)
        nx, ny = self.part.nx, self.part.ny
        ey, ex = int(sdims[-2] == Y_INTERFACE_DIM), int(sdims[-1] == X_INTERFACE_DIM)
        want = (len(self.layout.local_ranks),) + ((a.shape[1],) if len(sdims) == 3 else ()) + (ny + ey, nx + ex)
        if a.shape != want:
            raise ValueError(f"monitor: variable {name!r} has shape {a.shape}, dims {tuple(dims)} on this layout need {want}")
        return sdims, (a.shape[1] if len(sdims) == 3 else None), ey, ex

    def _global_shape(self, nk, ey, ex):
        lx, ly = self.part.layout
        return (6,) + (() if nk is None else (nk,)) + (self.part.ny * ly + ey, self.part.nx * lx + ex)


# ------------------------------------------------------------------------------------------------------------------------------------
class ZarrMonitor(_Monitor):
    """Zarr v2 directory store written by hand (layout: the module docstring)."""

    def __init__(self, path: str, layout, start_time=None):
        super().__init__(path, layout, start_time)
        self._n = 0  # records written
        self._meta: Dict[str, dict] = {}  # time-dependent variables, in first-seen order
        if layout.proc == 0:
            self._write_json(os.path.join(self.path, ".zgroup"), {"zarr_format": 2})

    @staticmethod
    def _write_json(path, obj):
        tmp = path + ".tmp"
        with open(tmp, "w") as f:
            json.dump(obj, f, indent=1, sort_keys=True)
        os.replace(tmp, path)

    def _zarray(self, shape, chunks, dtype):
        return {"zarr_format": 2, "shape": list(shape), "chunks": list(chunks), "dtype": dtype, "order": "C", "compressor": None, "filters": None, "fill_value": "NaN"}

    def _write_chunks(self, name, a, nk, ey, ex, prefix):
        """The chunks of this process's sub-domains: ``prefix`` = the leading chunk indices before ``tile`` (the record number, or nothing)."""
        d = os.path.join(self.path, name)
        os.makedirs(d, exist_ok=True)
        nx, ny = self.part.nx, self.part.ny
        lx, ly = self.part.layout
        mid = [] if nk is None else ["0"]

        def put(tile, jy, ix, block):
            key = ".".join(prefix + [str(tile)] + mid + [str(jy), str(ix)])
            np.ascontiguousarray(block).tofile(os.path.join(d, key))

        for i, rank in enumerate(self.layout.local_ranks):
            tile = self.part.tile_index(rank)
            sx, sy = self.part.subtile_index(rank)
            s = a[i]
            put(tile, sy, sx, s[..., :ny, :nx])
            north, east = bool(ey) and sy == ly - 1, bool(ex) and sx == lx - 1
            if north or east:
                fill = np.full(s.shape[:-2] + (ny, nx), np.nan, dtype=s.dtype)
            if north:  # the tile's last interface row: the single valid row of an extra chunk
                b = fill.copy()
                b[..., 0, :] = s[..., ny, :nx]
                put(tile, ly, sx, b)
            if east:
                b = fill.copy()
                b[..., :, 0] = s[..., :ny, nx]
                put(tile, sy, lx, b)
            if north and east:
                b = fill.copy()
                b[..., 0, 0] = s[..., ny, nx]
                put(tile, ly, lx, b)

    @staticmethod
    def _dtype(a):
        if a.dtype not in (np.float64, np.float32):
            raise ValueError(f"monitor: dtype {a.dtype} (float64 / float32 are written)")
        return "<f8" if a.dtype == np.float64 else "<f4"

    def store(self, time, variables: Iterable[Tuple[str, np.ndarray, Sequence[str], str]]):
        """One record: ``variables`` yields ``(name, array [n_sub, (nk,) nj, ni], quantity dims, units)``; every array is written before
        the next is asked for."""
        n = self._n
        for name, a, dims, units in variables:
            sdims, nk, ey, ex = self._check(name, a, dims)
            a = a.astype(a.dtype.newbyteorder("<"), copy=False)
            m = self._meta.get(name)
            chunks = (1, 1) + (() if nk is None else (nk,)) + (self.part.ny, self.part.nx)
            new = {"shape": self._global_shape(nk, ey, ex), "chunks": chunks, "dtype": self._dtype(a), "dims": ("time", "tile") + sdims, "units": units}
            if m is None:
                self._meta[name] = new
            elif m != new:
                raise ValueError(f"monitor: variable {name!r} changed between records ({m} -> {new})")
            self._write_chunks(name, a, nk, ey, ex, [str(n)])
        self._barrier()  # every process's chunks of the record exist
        if self.layout.proc == 0:
            d = os.path.join(self.path, "time")
            os.makedirs(d, exist_ok=True)
            np.array([self._seconds(time)], dtype="<f8").tofile(os.path.join(d, str(n)))
            if n == 0:
                self._write_json(os.path.join(d, ".zattrs"), {"_ARRAY_DIMENSIONS": ["time"], "units": self.time_units})
            self._write_json(os.path.join(d, ".zarray"), self._zarray((n + 1,), (1,), "<f8"))
            for name, m in self._meta.items():
                d = os.path.join(self.path, name)
                if n == 0:
                    self._write_json(os.path.join(d, ".zattrs"), {"_ARRAY_DIMENSIONS": list(m["dims"]), "units": m["units"]})
                self._write_json(os.path.join(d, ".zarray"), self._zarray((n + 1,) + m["shape"], m["chunks"], m["dtype"]))
        self._n = n + 1

    def store_constant(self, name: str, a: np.ndarray, dims: Sequence[str], units: str = ""):
        """A time-independent 2-D variable (the grid's ``lat`` ...): dims ``tile, y*, x*``."""
        sdims, nk, ey, ex = self._check(name, a, dims)
        if nk is not None:
            raise ValueError(f"monitor: constant {name!r} must be 2-D")
        a = a.astype(a.dtype.newbyteorder("<"), copy=False)
        self._write_chunks(name, a, None, ey, ex, [])
        if self.layout.proc == 0:
            d = os.path.join(self.path, name)
            self._write_json(os.path.join(d, ".zattrs"), {"_ARRAY_DIMENSIONS": ["tile"] + list(sdims), "units": units})
            self._write_json(os.path.join(d, ".zarray"), self._zarray(self._global_shape(None, ey, ex), (1, self.part.ny, self.part.nx), self._dtype(a)))

    def cleanup(self):
        self._barrier()


# ------------------------------------------------------------------------------------------------------------------------------------
class NetCDFMonitor(_Monitor):
    """``state_<chunk:04d>_tile<t>.nc`` with ``time_chunk_size`` records each, ``constants_tile<t>.nc`` (layout: the module docstring)."""

    def __init__(self, path: str, layout, time_chunk_size: int = 1, start_time=None):
        per_tile = layout.part.tile.ranks_per_tile
        if layout.per_proc % per_tile:
            raise ValueError(f"NetCDFMonitor: the {per_tile} sub-domains of a tile are split over processes ({layout.per_proc} sub-domains per process): the netcdf format "
                             "assembles a whole tile in one process -- use 'output_format: zarr', which writes per sub-domain")
        if int(time_chunk_size) < 1:
            raise ValueError(f"NetCDFMonitor: time_chunk_size {time_chunk_size}")
        super().__init__(path, layout, start_time)
        self.time_chunk_size = int(time_chunk_size)
        self.tiles = sorted({self.part.tile_index(r) for r in layout.local_ranks})
        self._chunk = 0
        self._times: List[float] = []
        self._meta: Dict[str, tuple] = {}
        self._records: Dict[str, Dict[int, list]] = {}
        self._constants: Dict[str, tuple] = {}

    def _assemble(self, a, nk, ey, ex) -> Dict[int, np.ndarray]:
        """{tile: [(nk,) ny_tile, nx_tile]} (own copies) from the packed sub-domains; a shared interface row is taken once, as in the zarr store."""
        nx, ny = self.part.nx, self.part.ny
        lx, ly = self.part.layout
        shape = self._global_shape(nk, ey, ex)[1:]
        out = {t: np.empty(shape, dtype=a.dtype) for t in self.tiles}
        for i, rank in enumerate(self.layout.local_ranks):
            sx, sy = self.part.subtile_index(rank)
            nj = ny + (1 if (ey and sy == ly - 1) else 0)
            ni = nx + (1 if (ex and sx == lx - 1) else 0)
            out[self.part.tile_index(rank)][..., sy * ny : sy * ny + nj, sx * nx : sx * nx + ni] = a[i][..., :nj, :ni]
        return out

    def store(self, time, variables):
        self._times.append(self._seconds(time))
        for name, a, dims, units in variables:
            sdims, nk, ey, ex = self._check(name, a, dims)
            meta = (sdims, units)
            if self._meta.setdefault(name, meta) != meta:
                raise ValueError(f"monitor: variable {name!r} changed between records")
            tiles = self._assemble(a, nk, ey, ex)
            rec = self._records.setdefault(name, {t: [] for t in self.tiles})
            for t in self.tiles:
                rec[t].append(tiles[t])
        if len(self._times) == self.time_chunk_size:
            self._flush()

    @staticmethod
    def _put(f, name, a, dims, units):
        for d, n in zip(dims, a.shape):
            if d not in f.dimensions:
                f.createDimension(d, n)
            elif f.dimensions[d] != n:
                raise ValueError(f"monitor: dimension {d!r} has length {f.dimensions[d]}, variable {name!r} needs {n}")
        v = f.createVariable(name, a.dtype, tuple(dims))
        v[:] = a
        v.units = units
        return v

    def _flush(self):
        from scipy.io import netcdf_file

        if not self._times:
            return
        for t in self.tiles:
            with netcdf_file(os.path.join(self.path, f"state_{self._chunk:04d}_tile{t}.nc"), "w", version=2) as f:
                f.history = "pace_amd.monitor.NetCDFMonitor"
                self._put(f, "time", np.asarray(self._times, dtype=np.float64), ("time",), self.time_units)
                self._put(f, "tile", np.asarray([t], dtype=np.int32), ("tile",), "")
                for name, (sdims, units) in self._meta.items():
                    a = np.stack(self._records[name][t])[:, None]
                    self._put(f, name, a, ("time", "tile") + sdims, units)
        self._chunk += 1
        self._times = []
        self._records = {}

    def store_constant(self, name, a, dims, units=""):
        sdims, nk, ey, ex = self._check(name, a, dims)
        if nk is not None:
            raise ValueError(f"monitor: constant {name!r} must be 2-D")
        self._constants[name] = (sdims, units, self._assemble(a, None, ey, ex))

    def cleanup(self):
        """Write the last, partial file of records and the constants."""
        from scipy.io import netcdf_file

        self._flush()
        if self._constants:
            for t in self.tiles:
                with netcdf_file(os.path.join(self.path, f"constants_tile{t}.nc"), "w", version=2) as f:
                    f.history = "pace_amd.monitor.NetCDFMonitor"
                    self._put(f, "tile", np.asarray([t], dtype=np.int32), ("tile",), "")
                    for name, (sdims, units, tiles) in self._constants.items():
                        self._put(f, name, tiles[t][None], ("tile",) + sdims, units)
            self._constants = {}
