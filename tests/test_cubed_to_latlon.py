"""CubedToLatLon (FV3 c2l_ord4 / c2l_ord2): D-grid u, v -> eastward / northward cell-centre winds ua, va.

Analytic recovery of the JW2006 zonal jet on every compute cell of the six tiles, parity with the numpy restatement
(tests/c2l_reference.py) on both builds of the kernel, the step's opt-in switch, and the two-process decomposition."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from c2l_reference import cubed_to_latlon as ref_c2l
from pace_amd._testing import harness_for, stencil_factory_for
from pace_amd.config import AcousticDynamicsConfig
from pace_amd.constants import get_constants
from pace_amd.grid import make_grid
from pace_amd.init import baroclinic_state, jw_zonal_wind, synthetic_state
from pace_amd.stencils import CubedToLatLon
from pace_amd.topology import CubedSpherePartitioner

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NH = 3


def _cube(backend, nx_tile, layout, nz, dtype=torch.float64, **cfg_kw):
    c = get_constants()
    part = CubedSpherePartitioner(nx_tile, layout)
    cfg = AcousticDynamicsConfig(npx=nx_tile + 1, npy=nx_tile + 1, npz=nz, layout=layout, **cfg_kw)
    grids = [make_grid(part, r, nz=nz) for r in range(part.total_ranks)]
    sf = stencil_factory_for(backend)(grids, cfg, c, dtype=dtype)
    return c, part, grids, sf


def _jw_errors(backend, nx_tile, order, nz=3):
    """max |ua - u_JW| and max |va| over the compute cells of the cube, from the JW2006 state without perturbation."""
    c, part, grids, sf = _cube(backend, nx_tile, (1, 1), nz)
    qf = sf.quantity_factory
    sts = [baroclinic_state(g, c, perturbation=False) for g in grids]
    u = qf.from_array([s["u"] for s in sts], ("x", "y", "z"))
    v = qf.from_array([s["v"] for s in sts], ("x", "y", "z"))
    ua, va = qf.zeros(("x", "y", "z")), qf.zeros(("x", "y", "z"))
    CubedToLatLon(sf, qf, grids, order=order)(u, v, ua, va)
    if not sf.hostemu:
        torch.cuda.synchronize()
    pe = grids[0].ak + grids[0].bk * 1.0e5
    eta = 0.5 * (pe[1:] + pe[:-1]) / 1.0e5
    eu = ev = 0.0
    cs = (slice(NH, NH + nx_tile), slice(NH, NH + nx_tile))
    for r, g in enumerate(grids):
        want = jw_zonal_wind(g.lon_agrid[cs][:, :, None], g.lat_agrid[cs][:, :, None], eta[None, None, :], c, perturbation=False)
        a, b = ua.numpy(r)[cs + (slice(0, nz),)], va.numpy(r)[cs + (slice(0, nz),)]
        assert np.all(np.isfinite(a)) and np.all(np.isfinite(b))
        eu = max(eu, float(np.abs(a - want).max()))
        ev = max(ev, float(np.abs(b).max()))
    return eu, ev


@pytest.mark.parametrize("order", [2, 4])
def test_jw_zonal_jet_recovered_and_converges(backend, order):
    """ua -> the JW2006 zonal wind (35 m/s jets), va -> 0 on all six tiles, cube corners included; the error falls about 4x per
    doubling of the resolution.  Measured (C12 / C24 / C48, max over the cube): order 2 ua 0.774 / 0.209 / 0.0544 m/s (ratios 3.71,
    3.83), va 0.129 / 0.0327 / 0.0083 (3.93, 3.94); order 4 ua 0.488 / 0.120 / 0.0300 (4.05, 4.02), va 0.0717 / 0.0170 / 0.0043
    (4.23, 3.91).  (The D-grid components are point values projected on the edge directions, which differ from the cell-centre
    unit vectors to second order: that geometry error sets the rate of both orders; order 4 halves its size.  The interpolants
    themselves converge at their own orders: test_interior_interpolant_order.)"""
    errs = [_jw_errors(backend, n, order) for n in (12, 24, 48)]
    bound_c12 = {2: (0.85, 0.14), 4: (0.55, 0.08)}[order]
    assert errs[0][0] < bound_c12[0] and errs[0][1] < bound_c12[1], errs
    for (u0, v0), (u1, v1) in zip(errs[:-1], errs[1:]):
        assert u0 / u1 > 3.4 and v0 / v1 > 3.4, errs
    if order == 4:
        two = [_jw_errors(backend, 24, 2)]
        assert errs[1][0] < 0.7 * two[0][0] and errs[1][1] < 0.7 * two[0][1], (errs, two)


def _index_space_errors(backend, nx_tile, order):
    """D-grid u, v sampled from smooth functions F, G of the tile's index coordinates (u at the x-edge mid-points, v at the y-edge
    mid-points); the kernel's interpolants utmp / 2, vtmp / 2 recovered from ua, va through the inverse of the a11 .. a22 rotation and
    compared with F, G at the cell centres, on the cells off the tile-edge rows / columns (where order 4 takes the four-point form)."""
    nz = 3
    c, part, grids, sf = _cube(backend, nx_tile, (1, 1), nz)
    qf = sf.quantity_factory
    n, m = nx_tile, nx_tile + 2 * NH + 1
    X, Y = np.meshgrid(np.arange(m) - NH, np.arange(m) - NH, indexing="ij")  # tile corner index of the storage point

    def F(x, y):
        return np.cos(2 * np.pi * x) * np.sin(2 * np.pi * y + 0.3) + 0.5 * np.sin(2 * np.pi * (x + 2 * y))

    def G(x, y):
        return np.sin(2 * np.pi * x + 0.7) * np.cos(2 * np.pi * y)

    u = np.repeat(F((X + 0.5) / n, Y / n)[:, :, None], nz + 1, axis=2)
    v = np.repeat(G(X / n, (Y + 0.5) / n)[:, :, None], nz + 1, axis=2)
    uq = qf.from_array([u] * len(grids), ("x", "y", "z"))
    vq = qf.from_array([v] * len(grids), ("x", "y", "z"))
    ua, va = qf.zeros(("x", "y", "z")), qf.zeros(("x", "y", "z"))
    CubedToLatLon(sf, qf, grids, order=order)(uq, vq, ua, va)
    if not sf.hostemu:
        torch.cuda.synchronize()
    cs = (slice(NH, NH + n), slice(NH, NH + n))
    inner = (slice(1, n - 1), slice(1, n - 1))
    xc, yc = (X[cs] + 0.5) / n, (Y[cs] + 0.5) / n
    eu = ev = 0.0
    for r, g in enumerate(grids):
        a11, a12, a21, a22 = (g.fields[k][cs] for k in ("a11", "a12", "a21", "a22"))
        det = a11 * a22 - a12 * a21
        for k in range(nz):
            e, w = ua.numpy(r)[cs + (k,)], va.numpy(r)[cs + (k,)]
            ut = (a22 * e - a12 * w) / det
            vt = (a11 * w - a21 * e) / det
            eu = max(eu, float(np.abs(0.5 * ut - F(xc, yc))[inner].max()))
            ev = max(ev, float(np.abs(0.5 * vt - G(xc, yc))[inner].max()))
    return eu, ev


@pytest.mark.parametrize("order", [2, 4])
def test_interior_interpolant_order(backend, order):
    """Inside the tile the order-4 interpolant is fourth-order and the order-2 one second-order, when the D-grid values are samples of
    smooth functions of the index coordinates.  Measured (C12 / C24 / C48, max over the interior cells): order 4 utmp 1.39e-2 /
    9.55e-4 / 6.09e-5 (ratios 14.5, 15.7), vtmp 1.66e-3 / 1.08e-4 / 6.86e-6 (15.3, 15.8); order 2 9.16e-2 / 2.43e-2 / 6.19e-3
    (3.77, 3.92) and 3.34e-2 / 8.79e-3 / 2.22e-3 (3.80, 3.96).  So the about-4x rate of the JW2006 test is that of the D-grid
    sampling itself (winds projected on the edge directions), not of the interpolation."""
    errs = [_index_space_errors(backend, n, order) for n in (12, 24, 48)]
    lo, hi = {2: (3.5, 4.5), 4: (13.5, 17.0)}[order]
    for (u0, v0), (u1, v1) in zip(errs[:-1], errs[1:]):
        assert lo < u0 / u1 < hi and lo < v0 / v1 < hi, errs


@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("nx_tile, layout", [(12, (1, 1)), (12, (2, 2)), (24, (1, 1)), (24, (2, 2))])
def test_matches_numpy_restatement(backend, nx_tile, layout, order):
    """fp64 kernel = tests/c2l_reference.py to round-off on every sub-domain of the cube (the restatement reads the halo the
    operator's own D-grid update left in u, v)."""
    nz = 5
    c, part, grids, sf = _cube(backend, nx_tile, layout, nz)
    qf = sf.quantity_factory
    sts = [synthetic_state(g, seed=11, rank=r) for r, g in enumerate(grids)]
    u = qf.from_array([s["u"] for s in sts], ("x", "y", "z"))
    v = qf.from_array([s["v"] for s in sts], ("x", "y", "z"))
    ua = qf.from_array([np.full_like(s["u"], 7.0) for s in sts], ("x", "y", "z"))
    va = qf.from_array([np.full_like(s["u"], 7.0) for s in sts], ("x", "y", "z"))
    CubedToLatLon(sf, qf, grids, order=order)(u, v, ua, va)
    if not sf.hostemu:
        torch.cuda.synchronize()
    n = part.nx
    cs = (slice(NH, NH + n), slice(NH, NH + n), slice(0, nz))
    worst = 0.0
    for r, g in enumerate(grids):
        want_u, want_v = ref_c2l(u.numpy(r), v.numpy(r), g, order)
        for got, want in ((ua.numpy(r), want_u), (va.numpy(r), want_v)):
            scale = np.abs(want).max()
            err = float(np.abs(got[cs] - want).max() / scale)
            worst = max(worst, err)
            # only the compute cells of levels 0 .. nz-1 are written
            outside = np.ones(got.shape, dtype=bool)
            outside[cs] = False
            assert np.all(got[outside] == 7.0)
    assert worst < 1.0e-14, worst


def test_fp32_tracks_fp64(backend):
    """The fp32 build of the same kernel against the fp64 restatement: the terms are O(1) products of a few roundings, so the
    field-relative error stays near the fp32 epsilon (bound 1e-6 = about 8 ulp of the largest wind)."""
    nz, nx_tile, layout = 4, 12, (2, 2)
    # (nord = 0: the fp32 context refuses the C12 del-6 damping tables, which overflow the float range; CubedToLatLon reads none)
    c, part, grids, sf = _cube(backend, nx_tile, layout, nz, dtype=torch.float32, nord=0)
    qf = sf.quantity_factory
    sts = [synthetic_state(g, seed=5, rank=r) for r, g in enumerate(grids)]
    u = qf.from_array([s["u"] for s in sts], ("x", "y", "z"))
    v = qf.from_array([s["v"] for s in sts], ("x", "y", "z"))
    ua, va = qf.zeros(("x", "y", "z")), qf.zeros(("x", "y", "z"))
    CubedToLatLon(sf, qf, grids, order=4)(u, v, ua, va)
    if not sf.hostemu:
        torch.cuda.synchronize()
    n = part.nx
    cs = (slice(NH, NH + n), slice(NH, NH + n), slice(0, nz))
    worst = 0.0
    for r, g in enumerate(grids):
        want_u, want_v = ref_c2l(u.numpy(r).astype(np.float64), v.numpy(r).astype(np.float64), g, 4)
        for got, want in ((ua.numpy(r), want_u), (va.numpy(r), want_v)):
            worst = max(worst, float(np.abs(got[cs].astype(np.float64) - want).max() / np.abs(want).max()))
    assert worst < 1.0e-6, worst


def test_operator_refuses_other_orders(hostemu):
    c, part, grids, sf = _cube("hostemu", 12, (1, 1), 3)
    with pytest.raises(ValueError):
        CubedToLatLon(sf, sf.quantity_factory, grids, order=3)
    with pytest.raises(NotImplementedError):
        AcousticDynamicsConfig(c2l_ord=3).validate()
    assert AcousticDynamicsConfig().c2l_ord == 4  # the reference's default


def _all_sums(h):
    return {n: [float(getattr(h.state, n).sub(i).storage.double().sum().item()) for i in range(len(h.grids))] for n in h.state.__dict__ if hasattr(getattr(h.state, n), "sub")}


def test_latlon_winds_is_opt_in(backend):
    """latlon_winds=False is today's step (every state field, ua / va included, bit for bit); with it on, the prognostic compute
    cells are unchanged and only ua / va differ -- they hold the eastward / northward winds of the step's end state."""
    mk = harness_for(backend)
    kw = dict(nz=4, layout=(1, 1), dt_atmos=225.0, k_split=2, n_split=2, init="baroclinic")
    runs = {}
    for name, extra in (("default", {}), ("off", dict(latlon_winds=False)), ("on", dict(latlon_winds=True))):
        h = mk(12, **kw, **extra)
        h.step()
        h.synchronize()
        runs[name] = h
    assert runs["default"].cubed_to_latlon is None and runs["off"].cubed_to_latlon is None
    s_def, s_off = _all_sums(runs["default"]), _all_sums(runs["off"])
    assert "ua" in s_def and "phis" in s_def
    assert s_def == s_off
    on = runs["on"]
    cs = (slice(NH, NH + 12), slice(NH, NH + 12), slice(0, 4))
    for r in range(6):
        for n in ("delp", "pt", "w", "delz", "q_con"):
            assert np.array_equal(getattr(on.state, n).numpy(r)[cs], getattr(runs["default"].state, n).numpy(r)[cs]), n
        want_u, want_v = ref_c2l(on.state.u.numpy(r), on.state.v.numpy(r), on.grids[r], 4)
        assert np.abs(on.state.ua.numpy(r)[cs] - want_u).max() <= 1.0e-13 * np.abs(want_u).max()
        assert np.abs(on.state.va.numpy(r)[cs] - want_v).max() <= 1.0e-13 * np.abs(want_u).max()
        assert not np.array_equal(on.state.ua.numpy(r)[cs], runs["default"].state.ua.numpy(r)[cs])


def _poison_halo(q, nx, ny, ex, ey):
    """NaN everywhere outside the compute cells (+ the staggered interface ex / ey) of every sub-domain: stale-halo stand-in."""
    keep = torch.zeros(q.storage.shape[-2:], dtype=torch.bool, device=q.storage.device)  # [j, i]
    keep[NH : NH + ny + ey, NH : NH + nx + ex] = True
    q.storage.masked_fill_(~keep, float("nan"))


@pytest.mark.parametrize("order", [2, 4])
def test_layout_2x2_with_poisoned_halo_matches_the_whole_tile(backend, order):
    """Sub-domains cut from tile-global fields, their halos NaN: the 2 x 2 result must equal the 1 x 1 result on the same window.
    The 1 x 1 run never reads halo (the tile-edge rows / columns take the two-point form); the 2 x 2 order-4 run reads u one row and
    v one column into the neighbouring sub-domains, so it is right only if the operator's D-grid halo update filled them."""
    nx_tile, nz = 12, 4
    c, part1, grids1, sf1 = _cube(backend, nx_tile, (1, 1), nz)
    tiles = [synthetic_state(g, seed=3, rank=r) for r, g in enumerate(grids1)]
    q1 = sf1.quantity_factory
    u1 = q1.from_array([s["u"] for s in tiles], ("x", "y", "z"))
    v1 = q1.from_array([s["v"] for s in tiles], ("x", "y", "z"))
    ua1, va1 = q1.zeros(("x", "y", "z")), q1.zeros(("x", "y", "z"))
    CubedToLatLon(sf1, q1, grids1, order=order)(u1, v1, ua1, va1)

    _, part2, grids2, sf2 = _cube(backend, nx_tile, (2, 2), nz)
    n = part2.nx
    q2 = sf2.quantity_factory

    def window(a, r, ex, ey):
        out = np.zeros_like(tiles[0]["u"], shape=(n + 2 * NH + 1, n + 2 * NH + 1, a.shape[2]))
        x0, y0 = part2.origin(r)
        out[NH : NH + n + ex, NH : NH + n + ey] = a[NH + x0 : NH + x0 + n + ex, NH + y0 : NH + y0 + n + ey]
        return out

    u2 = q2.from_array([window(tiles[part2.tile_index(r)]["u"], r, 0, 1) for r in range(part2.total_ranks)], ("x", "y", "z"))
    v2 = q2.from_array([window(tiles[part2.tile_index(r)]["v"], r, 1, 0) for r in range(part2.total_ranks)], ("x", "y", "z"))
    _poison_halo(u2, n, n, 0, 1)
    _poison_halo(v2, n, n, 1, 0)
    ua2, va2 = q2.zeros(("x", "y", "z")), q2.zeros(("x", "y", "z"))
    CubedToLatLon(sf2, q2, grids2, order=order)(u2, v2, ua2, va2)
    if not sf2.hostemu:
        torch.cuda.synchronize()
    cs = (slice(NH, NH + n), slice(NH, NH + n), slice(0, nz))
    for r in range(part2.total_ranks):
        x0, y0 = part2.origin(r)
        t = part2.tile_index(r)
        tw = (slice(NH + x0, NH + x0 + n), slice(NH + y0, NH + y0 + n), slice(0, nz))
        for got, want in ((ua2.numpy(r)[cs], ua1.numpy(t)[tw]), (va2.numpy(r)[cs], va1.numpy(t)[tw])):
            assert np.all(np.isfinite(got)), (r, "a halo value the operator reads was not exchanged")
            assert np.abs(got - want).max() <= 1.0e-13 * np.abs(want).max(), (r, np.abs(got - want).max())


# ---------------------------------------------------------------------------------------------------------------------------------
# decomposition: two processes (gloo; on the GPU both share device 0 -- three processes with the GPU open) = one process, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------------
def _latlon_from_poisoned_halo(h):
    """one step, then the u / v halos set to NaN and CubedToLatLon again: the result is finite only if its halo update refills them"""
    h.step()
    n = h.part.nx
    _poison_halo(h.state.u, n, n, 0, 1)
    _poison_halo(h.state.v, n, n, 1, 0)
    h.cubed_to_latlon(h.state.u, h.state.v, h.state.ua, h.state.va)
    h.synchronize()


def _worker(rank, world, init_file, out_dir, backend, nx_tile, layout, nz):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist

    from pace_amd._testing import harness_for as hf

    torch.set_num_threads(1)
    os.environ["OMP_NUM_THREADS"] = "2"
    dist.init_process_group("gloo", init_method=f"file://{init_file}", rank=rank, world_size=world)
    h = hf(backend)(nx_tile, nz, layout, dt_atmos=225.0, k_split=1, n_split=2, world_size=world, proc=rank, group=None, latlon_winds=True)
    _latlon_from_poisoned_halo(h)
    out = h.state.to_arrays(["ua", "va"])
    np.savez(os.path.join(out_dir, f"proc{rank}.npz"), **{f"{n}_{i}": a[n] for i, a in enumerate(out) for n in a})
    dist.barrier()
    h.close()
    dist.destroy_process_group()


def test_two_process_latlon_winds_match_single_process(backend, tmp_path):
    """Layout 2 x 2 over two processes: every sub-domain's order-4 interpolant reads u / v one row / column into its neighbours, a
    quarter of them in the other process.  Before the compared call the u / v halos are set to NaN in both runs, so finite values equal
    to the one-process run's bits show that the operator's D-grid halo update brought the neighbours' rows across the processes."""
    nx_tile, layout, nz, world = 12, (2, 2), 4, 2
    h = harness_for(backend)(nx_tile, nz, layout, dt_atmos=225.0, k_split=1, n_split=2, world_size=1, proc=0, latlon_winds=True)
    _latlon_from_poisoned_halo(h)
    ref = h.state.to_arrays(["ua", "va"])
    init_file = str(tmp_path / "init")
    mp.spawn(_worker, args=(world, init_file, str(tmp_path), backend, nx_tile, layout, nz), nprocs=world, join=True)
    per = len(ref) // world
    sl = (slice(NH, NH + nx_tile // 2), slice(NH, NH + nx_tile // 2), slice(0, nz))
    for p in range(world):
        got = np.load(tmp_path / f"proc{p}.npz")
        for i in range(per):
            for n in ("ua", "va"):
                a, b = got[f"{n}_{i}"][sl], ref[p * per + i][n][sl]
                assert np.all(np.isfinite(b)) and np.array_equal(a, b), (p, i, n, np.abs(a - b).max())
