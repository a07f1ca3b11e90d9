"""A minimal Zarr v2 directory-store reader (json + np.fromfile) for the diagnostics tests: uncompressed C-order chunks, '.' as
the chunk-key separator, missing chunks = fill value.  Where ``zarr`` or ``xarray`` import, ``open_with_library`` opens the same
store with them as a cross-check; this image has neither, so the reader below is what the tests rely on."""
import itertools
import json
import os

import numpy as np


def names(store):
    return sorted(n for n in os.listdir(store) if os.path.exists(os.path.join(store, n, ".zarray")))


def attrs(store, name):
    with open(os.path.join(store, name, ".zattrs")) as f:
        return json.load(f)


def meta(store, name):
    with open(os.path.join(store, name, ".zarray")) as f:
        return json.load(f)


def read(store, name):
    m = meta(store, name)
    assert m["zarr_format"] == 2 and m["order"] == "C" and m["compressor"] is None and m["filters"] is None, m
    shape, chunks, dt = tuple(m["shape"]), tuple(m["chunks"]), np.dtype(m["dtype"])
    fill = {"NaN": np.nan, None: 0}.get(m["fill_value"], m["fill_value"])
    out = np.full(shape, fill, dtype=dt)
    for idx in itertools.product(*[range(-(-s // c)) for s, c in zip(shape, chunks)]):
        p = os.path.join(store, name, ".".join(str(i) for i in idx))
        if not os.path.exists(p):
            continue
        block = np.fromfile(p, dtype=dt).reshape(chunks)
        sl = tuple(slice(i * c, min((i + 1) * c, s)) for i, c, s in zip(idx, chunks, shape))
        out[sl] = block[tuple(slice(0, s.stop - s.start) for s in sl)]
    return out


def chunk(store, name, key):
    m = meta(store, name)
    return np.fromfile(os.path.join(store, name, key), dtype=np.dtype(m["dtype"])).reshape(m["chunks"])


def open_with_library(store):
    """{name: array} through zarr or xarray when one of them imports, else None."""
    try:
        import zarr

        g = zarr.open_group(store, mode="r")
        return {n: np.asarray(g[n]) for n in names(store)}
    except ImportError:
        pass
    try:
        import xarray as xr

        ds = xr.open_zarr(store, consolidated=False, decode_times=False)
        return {n: ds[n].values for n in names(store)}
    except ImportError:
        return None
