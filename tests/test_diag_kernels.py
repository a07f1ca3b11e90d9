"""fv3_diag_pack / fv3_diag_column_integral (pace_amd/csrc/fv3_diag.hip) through the FieldPack / ColumnIntegral operators, on the
host-emulation build and -- the same tests, ``-m gpu`` -- on hip:gfx950, in fp64 and fp32.

Shapes: sub-domains of 12 x 6 cells with nz 5 (C12, layout (1, 2): non-square and odd in nz, so a swapped i / j or k stride shows);
72 x 72 with nz 3 (rows wider than one 64-lane wavefront, more than one workgroup tile per plane); 6 x 6 with nz 3 (the smallest
context: fv3_ctx_create refuses fewer than 6 cells per side or fewer than 3 levels, so "nx_tile 6, nz 2" cannot be built).
Every field is filled with a value that is distinct per element, and every halo cell and the pad level are NaN before each call: a NaN
in the output means the kernel read outside the compute box.

Tolerances (column integral; u = unit roundoff, S = RGRAV * sum_k |q delp| of the column):
  fp64 vs the sequential restatement: bitwise (same operations in the same order, no contraction);
  fp64 vs RGRAV * np.sum(q * delp, axis=2): (nz + 1) 2^-52 S -- both sides are dot products of length nz plus one scaling, each within
      (nz + 1) 2^-53 S of the exact value;
  fp32 vs the fp64 restatement of the fp32-rounded inputs: (nz + 2) 2^-24 S -- nz product roundings and additions, the scaling, and the
      rounding of rgrav itself to fp32.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from pace_amd import build, lib
from pace_amd.constants import get_constants
from pace_amd.stencils import ColumnIntegral, FieldPack

SHAPES = [(12, (1, 2), 5, (0, 1, 2)), (72, (1, 1), 3, (0, 4)), (6, (1, 1), 3, (0, 3))]
SHAPE_IDS = ["c12_1x2_nz5", "c72_nz3", "c6_nz3"]
NH = 3
SENTINEL = -777.0


@pytest.fixture(params=[64, 32], ids=["fp64", "fp32"])
def precision(request):
    return request.param


@functools.lru_cache(maxsize=None)
def _case(backend, precision, nx_tile, layout, nz, ranks):
    from helpers import Case

    if backend == "hostemu":
        build.build(precision, hostemu=True, verbose=False)
    dtype = torch.float64 if precision == 64 else torch.float32
    # (fp32: the default del-8 damping tables overflow the float range on coarse grids and the context refuses them -- nord 1 fits;
    #  the damping order plays no part in these kernels)
    return Case(nx_tile, layout, ranks, nz=nz, backend=backend, dtype=dtype, cfg_kw=None if precision == 64 else dict(nord=1))


def _sync(cs):
    if not cs.sf.hostemu:
        torch.cuda.synchronize(cs.sf.device)


def _fill(q, ni, nj, nk, values=None):
    """Fill the compute box (ni x nj x nk) of every sub-domain with distinct values (default: 1 + the element's storage index, exact in
    fp32 at these sizes), NaN everywhere else (halo, the unused staggered ends, the pad level)."""
    shape = tuple(q.storage.shape)
    s = np.full(shape, np.nan)
    idx = 1.0 + np.arange(int(np.prod(shape)), dtype=np.float64).reshape(shape)
    if q.is_2d:
        s[:, NH : NH + nj, NH : NH + ni] = idx[:, NH : NH + nj, NH : NH + ni] if values is None else values
    else:
        s[:, :nk, NH : NH + nj, NH : NH + ni] = idx[:, :nk, NH : NH + nj, NH : NH + ni] if values is None else values
    q.storage.copy_(torch.from_numpy(s).to(q.storage.dtype))


def _out(cs, n):
    return torch.full((n,), SENTINEL, dtype=cs.sf.dtype, device=cs.sf.device)


def _expected_pack(q, ni, nj, k0=None, nk=None):
    per = []
    for t in range(q.n_sub):
        a = q.numpy(t)
        per.append(a[NH : NH + ni, NH : NH + nj].T if q.is_2d else a[NH : NH + ni, NH : NH + nj, k0 : k0 + nk].transpose(2, 1, 0))
    return np.stack(per)


FIELDS = {  # name: (dims, staggered x, staggered y, interface z)
    "cell": (("x", "y", "z"), 0, 0, 0),
    "u": (("x", "y_interface", "z"), 0, 1, 0),
    "v": (("x_interface", "y", "z"), 1, 0, 0),
    "pe": (("x", "y", "z_interface"), 0, 0, 1),
    "phis": (("x", "y"), 0, 0, 0),
}


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("field", list(FIELDS))
def test_pack_equals_the_compute_domain_bitwise(backend, precision, shape, field):
    nx_tile, layout, nz, ranks = shape
    cs = _case(backend, precision, nx_tile, layout, nz, ranks)
    nx, ny = cs.part.nx, cs.part.ny
    dims, ex, ey, ez = FIELDS[field]
    ni, nj, nk = nx + ex, ny + ey, nz + ez
    q = cs.qf.zeros(dims)
    _fill(q, ni, nj, nk)
    pack = FieldPack(cs.sf)
    two_d = len(dims) == 2
    assert pack.shape(q) == ((len(ranks), nj, ni) if two_d else (len(ranks), nk, nj, ni))
    n = len(ranks) * nj * ni * (1 if two_d else nk)
    out = _out(cs, n + 5)  # (room to spare: the operator passes the packed size, the tail must stay untouched)
    got = pack(q, out)
    _sync(cs)
    got = got.cpu().numpy()
    want = _expected_pack(q, ni, nj, 0, nk)
    assert got.dtype == want.dtype and got.shape == want.shape
    assert not np.isnan(got).any(), "the kernel read a halo cell or the pad level"
    assert np.array_equal(got, want)
    assert np.all(out[n:].cpu().numpy() == SENTINEL)
    if two_d:
        return
    for level in sorted({0, nz - 1}):  # single levels: the same entry with nk = 1
        out = _out(cs, len(ranks) * nj * ni)
        got = pack(q, out, level=level)
        _sync(cs)
        got = got.cpu().numpy()
        assert got.shape == (len(ranks), nj, ni)
        assert np.array_equal(got, _expected_pack(q, ni, nj, level, 1)[:, 0]), level


def _integral_inputs(cs, nz, seed=11):
    nx, ny, n_sub = cs.part.nx, cs.part.ny, len(cs.ranks)
    rng = np.random.default_rng(seed)
    delp = cs.qf.zeros(("x", "y", "z"))
    q = cs.qf.zeros(("x", "y", "z"))
    _fill(delp, nx, ny, nz, 1.0e3 * (1.0 + 0.5 * rng.random((n_sub, nz, ny, nx))))  # positive, ~1e3 Pa
    _fill(q, nx, ny, nz, 1.0e-3 * rng.standard_normal((n_sub, nz, ny, nx)))  # both signs: the bound is not vacuous
    return q, delp


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_column_integral(backend, precision, shape):
    nx_tile, layout, nz, ranks = shape
    cs = _case(backend, precision, nx_tile, layout, nz, ranks)
    nx, ny = cs.part.nx, cs.part.ny
    q, delp = _integral_inputs(cs, nz)
    op = ColumnIntegral(cs.sf)
    out = _out(cs, len(ranks) * ny * nx)
    got = op(q, delp, out)
    _sync(cs)
    got = got.cpu().numpy()
    assert got.shape == (len(ranks), ny, nx) and not np.isnan(got).any()
    grav = get_constants().GRAV
    rgrav = 1.0 / grav
    for t in range(len(ranks)):
        # (i, j, k) host arrays of the rounded inputs, in fp64
        qa = q.numpy(t)[NH : NH + nx, NH : NH + ny, :nz].astype(np.float64)
        da = delp.numpy(t)[NH : NH + nx, NH : NH + ny, :nz].astype(np.float64)
        assert (da > 0).all() and (qa > 0).any() and (qa < 0).any()
        s = np.zeros((nx, ny))
        for k in range(nz):
            s = s + qa[:, :, k] * da[:, :, k]
        s *= 1.0 / grav
        scale = rgrav * np.sum(np.abs(qa * da), axis=2)
        g = got[t].T.astype(np.float64)
        if precision == 64:
            assert np.array_equal(g, s), np.abs(g - s).max()  # bitwise: the sequential restatement
            ref = rgrav * np.sum(qa * da, axis=2)  # the reference's expression
            err = np.abs(g - ref)
            print(f"column integral fp64 vs np.sum: max err / bound = {(err / ((nz + 1) * 2.0 ** -52 * scale)).max():.3f}")
            assert (err <= (nz + 1) * 2.0**-52 * scale).all()
        else:
            err = np.abs(g - s)
            print(f"column integral fp32 vs fp64 restatement: max err / bound = {(err / ((nz + 2) * 2.0 ** -24 * scale)).max():.3f}")
            assert (err <= (nz + 2) * 2.0**-24 * scale).all()


def test_bad_arguments_are_refused_and_nothing_is_written(backend, precision):
    nx_tile, layout, nz, ranks = SHAPES[0]
    cs = _case(backend, precision, nx_tile, layout, nz, ranks)
    nx, ny, n_sub = cs.part.nx, cs.part.ny, len(ranks)
    q3 = cs.qf.zeros(("x", "y", "z"))
    q2 = cs.qf.zeros(("x", "y"))
    _fill(q3, nx, ny, nz)
    _fill(q2, nx, ny, 1)
    out = _out(cs, n_sub * (nz + 1) * (ny + 1) * (nx + 1))
    ptr = out.data_ptr()

    def refused(match, name, *args):
        with pytest.raises(lib.Fv3Error, match=match):
            cs.sf.call(name, *args)
        _sync(cs)
        assert np.all(out.cpu().numpy() == SENTINEL), "a refused call wrote to the output"

    n = n_sub * nz * ny * nx
    refused("out is null", "diag_pack", q3.fref, nx, ny, 0, nz, None, n)
    refused("ni must be nx or nx\\+1", "diag_pack", q3.fref, nx + 2, ny, 0, nz, ptr, n_sub * nz * ny * (nx + 2))
    refused("nj must be ny or ny\\+1", "diag_pack", q3.fref, nx, ny - 1, 0, nz, ptr, n_sub * nz * (ny - 1) * nx)
    refused("level range", "diag_pack", q3.fref, nx, ny, -1, 1, ptr, n_sub * ny * nx)
    refused("level range", "diag_pack", q3.fref, nx, ny, nz, 2, ptr, n_sub * 2 * ny * nx)  # (level nz itself is the interface fields' last)
    refused("level range", "diag_pack", q3.fref, nx, ny, 0, 0, ptr, 0)
    refused("level range", "diag_pack", q2.fref, nx, ny, 1, 1, ptr, n_sub * ny * nx)  # a 2-D field takes k0 = 0, nk = 1
    refused("level range", "diag_pack", q2.fref, nx, ny, 0, 2, ptr, n_sub * 2 * ny * nx)
    refused("out_elems", "diag_pack", q3.fref, nx, ny, 0, nz, ptr, n + 1)
    refused("out_elems", "diag_pack", q3.fref, nx, ny, 0, nz, ptr, n - 1)
    refused("field 'src'", "diag_pack", None, nx, ny, 0, nz, ptr, n)
    refused("out is null", "diag_column_integral", q3.fref, q3.fref, None, n_sub * ny * nx)
    refused("out_elems", "diag_column_integral", q3.fref, q3.fref, ptr, n_sub * ny * nx + 1)
    refused("field", "diag_column_integral", q3.fref, q2.fref, ptr, n_sub * ny * nx)  # delp must be 3-D
    # the operators check before they call: a buffer that is too small, a level outside the field, a level for a 2-D field
    with pytest.raises(ValueError, match="are needed"):
        FieldPack(cs.sf)(q3, out[: n - 1])
    with pytest.raises(ValueError, match="outside"):
        FieldPack(cs.sf)(q3, out, level=nz)
    with pytest.raises(ValueError, match="2-D"):
        FieldPack(cs.sf)(q2, out, level=0)
    with pytest.raises(NotImplementedError):
        ColumnIntegral(cs.sf)(cs.qf.zeros(("x", "y", "z_interface")), q3, out)
    assert lib.load(precision, hostemu=cs.sf.hostemu).fv3_version() == 2
    assert C.sizeof(C.c_long) == 8
