"""Parity of the kernel sources with the oracle, through the C ABI.

backend "hostemu": the same .hip sources compiled with g++ (runs in the GPU-less container);
backend "hip:gfx950" (-m gpu): the product library on the MI355X.  Tolerances are field-scale
relative (|a-b| <= tol * max|b|); fp64 target 1e-10, observed ~1e-15 except the
fields behind exp/log of the semi-implicit solver (w, omga: ~1e-11).
"""
import numpy as np
import pytest
import torch

from helpers import Case, assert_close, compare_cubes, oracle_cube, run_device_cube
from pace_amd.config import AcousticDynamicsConfig
from pace_amd.constants import get_constants
from pace_amd._testing import stencil_factory_for
from pace_amd.context import StencilFactory
from pace_amd.grid import make_grid
from pace_amd.topology import CubedSpherePartitioner

from fv3_oracle import a2b_ord4 as o_a2b
from fv3_oracle import c_sw as o_csw
from fv3_oracle import d_sw as o_dsw
from fv3_oracle import fvtp2d as o_tp
from fv3_oracle import nh as o_nh

TOL = {"default": 1e-12, "w": 1e-10, "omga": 1e-10, "delz": 1e-11, "u": 1e-11, "v": 1e-11, "uc": 1e-11, "vc": 1e-11}
# uc / vc are not compared after a full call: d_sw's divergence damping uses them as scratch in the
# reference, so what they hold afterwards is dead work data (c_sw recomputes them before any use);
# the marching divergence-damping kernel keeps its iterates in registers and leaves uc / vc alone.
# c_sw's uc / vc outputs are checked in test_c_sw.
STATE = "u v w ua va delp delz pt pe pk peln q_con omga mfxd mfyd cxd cyd".split()
# The BASELINE target is 1e-10 field-scale relative.  w (and omga, the C-grid w) come out of the semi-implicit solver behind
# exp / log of O(1e5 Pa) pressures: libm (numpy) and the device's ocml differ in the last bit there, which is an ABSOLUTE error of
# ~1e-12 m/s in w whatever its size (tests/pair_debug.py: riem_solver3 w 4e-12 of a 0.1 m/s field).  For states whose w is tiny
# (the balanced baroclinic wave: |w| ~ 1e-3 m/s; real restart data) the relative measure alone would be a test of libm, so
# those tests add this absolute floor instead of loosening the relative tolerance:
W_ATOL = {"w": 2e-12, "omga": 2e-12}  # m/s


@pytest.fixture(params=["hostemu", pytest.param("hip:gfx950", marks=pytest.mark.gpu)])
def backend(request):
    if request.param == "hostemu":
        request.getfixturevalue("hostemu")
    else:
        request.getfixturevalue("gpu_backend")
    return request.param


def _pad(a):
    return np.concatenate([a, a[:, :, -1:]], axis=2)


def _winds_and_fluxes(D, s, nz, dt=30000.0):
    V = lambda a: a[:, :, :nz].copy()  # noqa: E731
    uc, vc = V(s["v"]), V(s["u"])
    z = lambda: np.zeros_like(uc)  # noqa: E731
    crx, cry, xfx, yfx, ut, vt = z(), z(), z(), z(), z(), z()
    ra_x, ra_y = o_dsw.fxadv(D, uc, vc, crx, cry, xfx, yfx, ut, vt, dt)
    return dict(uc=uc, vc=vc, crx=crx, cry=cry, xfx=xfx, yfx=yfx, ut=ut, vt=vt, ra_x=ra_x, ra_y=ra_y)


# the C192 case has workgroup tiles away from every cube-tile edge (the LDS interior paths)
@pytest.mark.parametrize("n, layout, ranks", [(12, (1, 1), (0, 1)), (12, (2, 2), (0, 3, 5, 6)), (192, (1, 1), (2,))])
def test_fxadv_and_fv_tp_2d(backend, n, layout, ranks):
    nz = 4 if n == 12 else 3
    cs = Case(n, layout, ranks, nz=nz, backend=backend)
    w = [_winds_and_fluxes(D, s, nz) for D, s in zip(cs.doms, cs.states)]
    # fxadv
    Q = {k: cs.q([_pad(x[k]) for x in w]) for k in ("uc", "vc")}
    out = {k: cs.q() for k in ("crx", "cry", "xfx", "yfx", "ut", "vt")}
    cs.sf.call("fxadv", Q["uc"].fref, Q["vc"].fref, out["crx"].fref, out["cry"].fref, out["xfx"].fref, out["yfx"].fref, out["ut"].fref, out["vt"].fref, 30000.0)
    for r, D in enumerate(cs.doms):
        for k, R in (("crx", D.sl(1, D.nx + 1, D.jsd, D.jed)), ("xfx", D.sl(1, D.nx + 1, D.jsd, D.jed)), ("cry", D.sl(D.isd, D.ied, 1, D.ny + 1)), ("yfx", D.sl(D.isd, D.ied, 1, D.ny + 1)), ("ut", D.sl(1, D.nx + 1, D.jsd, D.jed)), ("vt", D.sl(D.isd, D.ied, 1, D.ny + 1))):
            assert_close(k, out[k].numpy(r)[:, :, :nz][R], w[r][k][R], 1e-13, 1e-13)
    # fv_tp_2d: plain, damped, mass-flux weighted + damped
    q = [s["pt"][:, :, :nz].copy() for s in cs.states]
    mass = [s["delp"][:, :, :nz].copy() for s in cs.states]
    F = {k: cs.q([_pad(x[k]) for x in w]) for k in ("crx", "cry", "xfx", "yfx")}
    Qq, Qm = cs.q([_pad(a) for a in q]), cs.q([_pad(a) for a in mass])
    mfx, mfy = cs.q([_pad(x["xfx"] * 1.1) for x in w]), cs.q([_pad(x["yfx"] * 0.9) for x in w])
    fx, fy = cs.q(), cs.q()
    for variant in range(3):
        if variant == 0:
            cs.sf.call("fv_tp_2d", Qq.fref, F["crx"].fref, F["cry"].fref, F["xfx"].fref, F["yfx"].fref, fx.fref, fy.fref, None, None, None, 6, -1, 0.0)
        elif variant == 1:
            cs.sf.call("fv_tp_2d", Qq.fref, F["crx"].fref, F["cry"].fref, F["xfx"].fref, F["yfx"].fref, fx.fref, fy.fref, None, None, None, 6, 2, 0.06)
        else:
            cs.sf.call("fv_tp_2d", Qq.fref, F["crx"].fref, F["cry"].fref, F["xfx"].fref, F["yfx"].fref, fx.fref, fy.fref, mfx.fref, mfy.fref, Qm.fref, 6, 2, 0.06)
        for r, D in enumerate(cs.doms):
            x = w[r]
            kw = [dict(), dict(nord=2, damp_c=0.06), dict(mfx=x["xfx"] * 1.1, mfy=x["yfx"] * 0.9, mass=mass[r], nord=2, damp_c=0.06)][variant]
            efx, efy = o_tp.fv_tp_2d(D, q[r].copy(), x["crx"], x["cry"], x["xfx"], x["yfx"], x["ra_x"], x["ra_y"], 6, **kw)
            Rx, Ry = D.sl(1, D.nx + 1, 1, D.ny), D.sl(1, D.nx, 1, D.ny + 1)
            assert_close("fx", fx.numpy(r)[:, :, :nz][Rx], efx[Rx], 1e-13, 1e-13)
            assert_close("fy", fy.numpy(r)[:, :, :nz][Ry], efy[Ry], 1e-13, 1e-13)


@pytest.mark.parametrize("n, layout, ranks", [(12, (1, 1), (0,)), (12, (2, 2), (1, 2, 4, 7)), (192, (1, 1), (4,))])
def test_a2b_ord4(backend, n, layout, ranks):
    nz = 3
    cs = Case(n, layout, ranks, nz=nz, backend=backend)
    qin = [s["pt"][:, :, :nz].copy() for s in cs.states]
    Q, O = cs.q([_pad(a) for a in qin]), cs.q()
    cs.sf.call("a2b_ord4", Q.fref, O.fref, 0, nz, 0)
    for r, D in enumerate(cs.doms):
        want = o_a2b.a2b_ord4(D, qin[r].copy())
        R = D.sl(1, D.nx + 1, 1, D.ny + 1)
        assert_close("qout", O.numpy(r)[:, :, :nz][R], want[R], 1e-13, 1e-13)


# n = 12: the generic per-point stage kernels everywhere; n >= 16 per sub-domain: the marching interior kernel (stages A + B + C) +
# the boundary windows -- 24 / 48: one strip, sub-domains with 0-2 cube-tile edges; 72 with 16-row segments: 2 strips x 5 segments
@pytest.mark.parametrize("n, layout, ranks, seg", [(12, (1, 1), (0, 3), None), (12, (2, 2), (0, 5, 10, 15), None), (24, (1, 1), (0, 4), None),
                                                   (48, (2, 2), (0, 5, 10, 15), "8"), (72, (1, 1), (2,), "16")])
def test_c_sw(backend, n, layout, ranks, seg, monkeypatch):
    nz = 4
    if seg:
        monkeypatch.setenv("FV3_SEG", seg)
    cs = Case(n, layout, ranks, nz=nz, backend=backend)
    names = ("delp", "pt", "u", "v", "w", "uc", "vc", "ua", "va", "omga")
    Q = {n: cs.q([s[n] for s in cs.states]) for n in names}
    ut, vt, divgd, delpc, ptc = cs.q(), cs.q(), cs.q(), cs.q(), cs.q()
    cs.sf.call("c_sw", *[Q[n].fref for n in ("delp", "pt", "u", "v", "w", "uc", "vc", "ua", "va")], ut.fref, vt.fref, divgd.fref, Q["omga"].fref, delpc.fref, ptc.fref, 56.25)
    for r, D in enumerate(cs.doms):
        s = {k: v[:, :, :nz].copy() for k, v in cs.states[r].items() if k != "phis"}
        o_ut, o_vt, o_div = np.zeros_like(s["u"]), np.zeros_like(s["u"]), np.zeros_like(s["u"])
        e_delpc, e_ptc = o_csw.c_sw(D, s["delp"], s["pt"], s["u"], s["v"], s["w"], s["uc"], s["vc"], s["ua"], s["va"], o_ut, o_vt, o_div, s["omga"], 56.25, nord=cs.cfg.nord)
        C1 = D.sl(0, D.nx + 1, 0, D.ny + 1)
        checks = [("delpc", delpc, e_delpc, C1), ("ptc", ptc, e_ptc, C1), ("omga", Q["omga"], s["omga"], C1), ("divgd", divgd, o_div, D.sl(1, D.nx + 1, 1, D.ny + 1)),
                  ("uc", Q["uc"], s["uc"], D.sl(1, D.nx + 1, 1, D.ny)), ("vc", Q["vc"], s["vc"], D.sl(1, D.nx, 1, D.ny + 1)),
                  ("ut", ut, o_ut, D.sl(0, D.nx + 2, 0, D.ny + 1)), ("vt", vt, o_vt, D.sl(0, D.nx + 1, 0, D.ny + 2)),
                  ("ua", Q["ua"], s["ua"], D.sl(0, D.nx + 1, 0, D.ny + 1))]
        for name, q, want, R in checks:
            got, wnt = q.numpy(r)[:, :, :nz][R].copy(), want[R].copy()
            # the (never used) cube-corner halo cell of cell-centred outputs is excluded
            if name in ("delpc", "ptc", "omga"):
                for (ci, cj), has in (((0, 0), D.sw), ((-1, 0), D.se), ((-1, -1), D.ne), ((0, -1), D.nw)):
                    if has:
                        got[ci, cj] = wnt[ci, cj] = 0.0
            assert_close(name, got, wnt, 1e-12, 1e-12)


def test_d_sw(backend):
    nz = 5
    cs = Case(12, (1, 1), (0, 4), nz=nz, backend=backend, cfg_kw=dict(n_split=1))
    names = ("delp", "pt", "u", "v", "w", "uc", "vc", "ua", "va", "q_con", "mfxd", "mfyd", "cxd", "cyd")
    ins = []
    for D, s in zip(cs.doms, cs.states):
        x = {k: v.copy() for k, v in s.items()}
        x["uc"][:, :, :] = s["v"] * 0.7
        x["vc"][:, :, :] = s["u"] * 0.7
        x["ua"][:, :, :] = np.roll(s["u"], 1, 1) * 0.9
        x["va"][:, :, :] = np.roll(s["v"], 1, 0) * 0.9
        x["divgd"] = 1e-6 * s["w"]
        ins.append(x)
    Q = {n: cs.q([x[n] for x in ins]) for n in names + ("divgd",)}
    T = {n: cs.q() for n in ("delpc", "crx", "cry", "xfx", "yfx", "zh", "heat", "diss")}
    dt = 112.5
    cs.sf.call("d_sw", T["delpc"].fref, *[Q[n].fref for n in ("delp", "pt", "u", "v", "w", "uc", "vc", "ua", "va", "divgd", "mfxd", "mfyd", "cxd", "cyd")],
               T["crx"].fref, T["cry"].fref, T["xfx"].fref, T["yfx"].fref, Q["q_con"].fref, T["zh"].fref, T["heat"].fref, T["diss"].fref, dt)
    col = o_dsw.get_column_namelist(cs.cfg, nz)
    for r, D in enumerate(cs.doms):
        x = {k: v[:, :, :nz].copy() for k, v in ins[r].items() if k != "phis"}
        z = lambda: np.zeros_like(x["u"])  # noqa: E731
        o = dict(delpc=z(), crx=z(), cry=z(), xfx=z(), yfx=z(), heat=z(), diss=z())
        o_dsw.d_sw(D, cs.cfg, col, o["delpc"], x["delp"], x["pt"], x["u"], x["v"], x["w"], x["uc"], x["vc"], x["ua"], x["va"], x["divgd"], x["mfxd"], x["mfyd"], x["cxd"], x["cyd"],
                   o["crx"], o["cry"], o["xfx"], o["yfx"], x["q_con"], None, o["heat"], o["diss"], dt)
        C = D.sl(1, D.nx, 1, D.ny)
        for name in ("delp", "pt", "w", "q_con"):
            assert_close(name, Q[name].numpy(r)[:, :, :nz][C], x[name][C], 1e-12, 1e-12)
        assert_close("u", Q["u"].numpy(r)[:, :, :nz][D.sl(1, D.nx, 1, D.ny + 1)], x["u"][D.sl(1, D.nx, 1, D.ny + 1)], 1e-12, 1e-12)
        assert_close("v", Q["v"].numpy(r)[:, :, :nz][D.sl(1, D.nx + 1, 1, D.ny)], x["v"][D.sl(1, D.nx + 1, 1, D.ny)], 1e-12, 1e-12)
        assert_close("heat_source", T["heat"].numpy(r)[:, :, :nz][C], o["heat"][C], 1e-11, 1e-11)
        assert_close("mfxd", Q["mfxd"].numpy(r)[:, :, :nz][D.sl(1, D.nx + 1, 1, D.ny)], x["mfxd"][D.sl(1, D.nx + 1, 1, D.ny)], 1e-12, 1e-12)
        assert_close("divgd", Q["divgd"].numpy(r)[:, :, :nz][D.sl(1, D.nx + 1, 1, D.ny + 1)], x["divgd"][D.sl(1, D.nx + 1, 1, D.ny + 1)], 1e-11, 1e-11)


def test_riem_solver3_and_column_ops(backend):
    nz = 10
    cs = Case(12, (1, 1), (2,), nz=nz, backend=backend)
    D, s = cs.doms[0], cs.states[0]
    c = cs.c
    x = {k: v.copy() for k, v in s.items()}
    zs = x["phis"] * c.RGRAV
    zh = np.zeros_like(x["u"])
    zh[:, :, nz] = zs[:, :, 0]
    for k in range(nz - 1, -1, -1):
        zh[:, :, k] = zh[:, :, k + 1] - x["delz"][:, :, k]
    wsd = np.full_like(zs, 0.01)
    names = ("cappa", "delz", "q_con", "delp", "pt", "pe", "pk", "peln", "w")
    Q = {n: cs.q([x[n]]) for n in names}
    Qzh, Qzs, Qws = cs.q([zh]), cs.q([zs], ("x", "y")), cs.q([wsd], ("x", "y"))
    ppe, pk3 = cs.q(), cs.q()
    ptop = cs.grids[0].ptop
    cs.sf.call("riem_solver3", 1, 18.75, Q["cappa"].fref, ptop, Qzs.fref, Qws.fref, Q["delz"].fref, Q["q_con"].fref, Q["delp"].fref, Q["pt"].fref, Qzh.fref,
               Q["pe"].fref, ppe.fref, pk3.fref, Q["pk"].fref, Q["peln"].fref, Q["w"].fref)
    e_ppe, e_pk3 = np.zeros_like(zh), np.zeros_like(zh)
    o_nh.riem_solver3(D, True, 18.75, x["cappa"], ptop, zs, wsd, x["delz"], x["q_con"], x["delp"], x["pt"], zh, x["pe"], e_ppe, e_pk3, x["pk"], x["peln"], x["w"], cs.cfg.p_fac)
    C = D.sl(1, D.nx, 1, D.ny)
    for name, got, want, tol in (("w", Q["w"], x["w"], 1e-10), ("delz", Q["delz"], x["delz"], 1e-12), ("zh", Qzh, zh, 1e-13), ("ppe", ppe, e_ppe, 1e-9), ("pk3", pk3, e_pk3, 1e-13),
                                 ("pe", Q["pe"], x["pe"], 1e-14), ("peln", Q["peln"], x["peln"], 1e-14)):
        kk = nz if name in ("w", "delz") else nz + 1
        assert_close(name, got.numpy(0)[C][:, :, :kk], want[C][:, :, :kk], tol, tol)
    # pk3_halo / edge_pe on the halo ring
    cs.sf.call("pk3_halo", pk3.fref, Q["delp"].fref, ptop, c.KAPPA)
    cs.sf.call("edge_pe", Q["pe"].fref, Q["delp"].fref, ptop)
    o_nh.pk3_halo(D, e_pk3, x["delp"], ptop, c.KAPPA)
    o_nh.pe_halo(D, x["pe"], x["delp"], ptop)
    R2 = D.sl(-1, D.nx + 2, -1, D.ny + 2)
    assert_close("pk3 ring", pk3.numpy(0)[R2][:, :, 1:], e_pk3[R2][:, :, 1:], 1e-13, 1e-13)
    R1 = D.sl(0, D.nx + 1, 0, D.ny + 1)
    assert_close("pe ring", Q["pe"].numpy(0)[R1], x["pe"][R1], 1e-14, 1e-14)


@pytest.mark.parametrize("n, layout, ranks", [(48, (2, 2), (0, 5, 10, 15)), (16, (1, 1), (0,))], ids=["c48_2x2", "c16_1x1"])
def test_c_sw_forms_are_bitwise_equal(backend, monkeypatch, n, layout, ranks):
    """The four forms of c_sw (the whole interior as one marching kernel / stages A - C as a marching kernel + stage kernels /
    two-row stage kernel + stage kernels / generic stage kernels everywhere) evaluate the same expressions in the same order:
    every output is bitwise equal.  C16 1x1: nx = 16 is the smallest size with an interior kernel, the one sub-domain has all four
    tile edges, the interior rectangle is 7 x 7 and the W and E windows nearly meet."""
    nz, outs, nr = 3, {}, len(ranks)
    for form, env in (("march", {}), ("abc", {"FV3_CSW_MARCH": "abc"}), ("two_row", {"FV3_CSW_MARCH": "0"}), ("generic", {"FV3_CSW_B_GENERIC": "1"})):
        for k in ("FV3_CSW_MARCH", "FV3_CSW_B_GENERIC"):
            monkeypatch.delenv(k, raising=False)
        for k, v_ in env.items():
            monkeypatch.setenv(k, v_)
        monkeypatch.setenv("FV3_SEG", "8")
        cs = Case(n, layout, ranks, nz=nz, backend=backend)
        names = ("delp", "pt", "u", "v", "w", "uc", "vc", "ua", "va", "omga")
        Q = {k: cs.q([s[k] for s in cs.states]) for k in names}
        extra = [cs.q() for _ in range(5)]
        cs.sf.call("c_sw", *[Q[k].fref for k in names[:9]], extra[0].fref, extra[1].fref, extra[2].fref, Q["omga"].fref, extra[3].fref, extra[4].fref, 56.25)
        outs[form] = [Q[k].numpy(r).copy() for k in ("uc", "vc", "ua", "va", "omga") for r in range(nr)] + [e.numpy(r).copy() for e in extra for r in range(nr)]
    for form in ("abc", "two_row", "generic"):
        for a, b in zip(outs["march"], outs[form]):
            assert np.array_equal(a, b), form


@pytest.mark.parametrize("layout, n_split", [((1, 1), 2), ((2, 2), 1)])
def test_full_acoustic_call(backend, layout, n_split):
    nz = 8
    part, cfg, grids, ost, phis, odyn = oracle_cube(12, layout, nz, dict(n_split=n_split))
    init = [{k: v.copy() for k, v in s.items()} for s in ost]
    odyn(ost, 225.0, 1)
    got, *_ = run_device_cube(backend, part, cfg, grids, init, phis, 225.0)
    compare_cubes(got, ost, part, nz, STATE, TOL)


@pytest.mark.parametrize("n_split", [1, 3])
def test_scalar_pingpong_leaves_every_array_as_the_in_place_sequence_does(backend, n_split, monkeypatch):
    """FV3_PINGPONG=0 (d_sw's copy-back form) against the default (the new delp / pt / w / q_con become the state, an odd sub-step
    count copies them home): the WHOLE storages agree bit for bit -- halos, cube-corner blocks, padding and the level nz of the
    allocation, which belongs to the caller (an edge-replicated plane there must survive the home-coming copy)."""
    nz = 6
    part, cfg, grids, ost, phis, _ = oracle_cube(12, (1, 1), nz, dict(n_split=n_split))
    res = {}
    for pp in ("0", "1"):
        monkeypatch.setenv("FV3_PINGPONG", pp)
        init = [{k: v.copy() for k, v in s.items()} for s in ost]
        from pace_amd.dyn_core import AcousticDynamics, DycoreState
        from pace_amd.halo import Layout

        sf = stencil_factory_for(backend)(grids, cfg, get_constants())
        st = DycoreState.from_arrays(sf.quantity_factory, [dict(s_, phis=p) for s_, p in zip(init, phis)])
        for n in ("delp", "pt", "w", "q_con"):
            getattr(st, n).storage[:, nz] = 12345.0 + len(n)  # the caller's level-nz plane (e.g. what restart_state puts there)
        dyn = AcousticDynamics(Layout(part, 1, 0), grids, sf, config=cfg, phis=st.phis, state=st)
        dyn(st, 225.0, n_map=1)
        if backend != "hostemu":
            torch.cuda.synchronize()
        res[pp] = {n: getattr(st, n).storage.detach().cpu().numpy().copy() for n in STATE}
        assert sf.scratch_bytes > 0
        res[pp + "bytes"] = sf.scratch_bytes
    for n in STATE:
        assert np.array_equal(res["0"][n], res["1"][n]), n
    for n in ("delp", "pt", "w", "q_con"):
        assert np.all(res["1"][n][:, nz] == 12345.0 + len(n)), n
    assert res["1bytes"] > res["0bytes"]  # the alternate buffers exist only in the context that used them


def test_operator_contexts_do_not_allocate_the_pingpong_buffers(backend):
    """The four alternate buffers of fv3_acoustic_step are allocated by the first sequencer call that is eligible for the
    ping-pong, not with the context: a context that only runs single operators stays at the 24 + scratch fields."""
    from helpers import Case

    cs = Case(nx_tile=12, nz=8, backend=backend)
    before = cs.sf.scratch_bytes
    s0 = cs.states[0]
    cs.sf.call("ray_fast", cs.q([s0["u"]]).fref, cs.q([s0["v"]]).fref, cs.q([s0["w"]]).fref, 10.0, float(cs.grids[0].ptop))
    ni, nj, nk = cs.sf.sizer.storage_shape
    assert cs.sf.scratch_bytes - before < ni * nj * nk * 8  # (small per-operator tables may appear; no full 3-D field)


@pytest.mark.parametrize("name", ["dz_damp_scaled", "heat_dt_full", "smt5_lim_fac", "ray_fast_plain", "heat_zero_first_call"])
def test_named_alternatives_switch_oracle_and_library_together(backend, name, monkeypatch):
    """FV3_ALT=<name> selects the alternative form of a restatement DESIGN §2 lists as uncertain in the oracle AND in the library
    (native sequencer and its Python twin): under the switch the two still agree to the usual tolerances, and the switch does
    change the result where it is expected to (so that a run against reference savepoints can tell the forms apart)."""
    nz = 8
    base = None
    for env in ("", name):
        if env:
            monkeypatch.setenv("FV3_ALT", env)
        else:
            monkeypatch.delenv("FV3_ALT", raising=False)
        n_calls = 2 if name == "heat_zero_first_call" else 1  # (two acoustic calls of one step: n_map = 1, 2)
        part, cfg, grids, ost, phis, odyn = oracle_cube(12, (1, 1), nz, dict(n_split=2, k_split=n_calls))
        init = [{k: v.copy() for k, v in s.items()} for s in ost]
        for n in range(n_calls):
            odyn(ost, 225.0, n + 1)
        got, *_ = run_device_cube(backend, part, cfg, grids, init, phis, 225.0, n_calls=n_calls)
        compare_cubes(got, ost, part, nz, STATE, TOL)
        got_py, *_ = run_device_cube(backend, part, cfg, grids, init, phis, 225.0, n_calls=n_calls, native=False)
        for r in range(part.total_ranks):
            for n in ("delz", "w", "pt"):
                assert np.array_equal(got[r][n], got_py[r][n]), n
        if not env:
            base = ost
        elif name == "dz_damp_scaled":  # the interface-height damping changes: the thickness differs from the default form
            assert max(np.abs(a["delz"] - b["delz"]).max() for a, b in zip(ost, base)) > 1e-9
        elif name == "smt5_lim_fac":  # more cells take the linear scheme: every transported field moves
            assert max(np.abs(a["pt"] - b["pt"]).max() for a, b in zip(ost, base)) > 1e-9
        elif name == "ray_fast_plain":  # the damped momentum is not given back to the column: the winds of the top levels differ
            assert max(np.abs(a["u"] - b["u"]).max() for a, b in zip(ost, base)) > 1e-9
        elif name == "heat_zero_first_call":  # the second call's heating includes the first call's heat source: pt differs
            assert max(np.abs(a["pt"] - b["pt"]).max() for a, b in zip(ost, base)) > 1e-12
    monkeypatch.setenv("FV3_ALT", "no_such_form")
    with pytest.raises(ValueError, match="unknown alternative"):
        oracle_cube(12, (1, 1), 3, dict(n_split=1))[5]([{k: v.copy() for k, v in s.items()} for s in oracle_cube(12, (1, 1), 3, dict(n_split=1))[3]], 10.0, 1)


@pytest.mark.parametrize("layout", [(1, 2), (3, 1)])
def test_full_acoustic_call_non_square_subdomains(backend, layout):
    """Layouts with nx != ny per sub-domain (24 x 12, 8 x 24)."""
    nz = 5
    part, cfg, grids, ost, phis, odyn = oracle_cube(24, layout, nz, dict(n_split=2))
    init = [{k: v.copy() for k, v in s.items()} for s in ost]
    odyn(ost, 112.5, 1)
    got, *_ = run_device_cube(backend, part, cfg, grids, init, phis, 112.5)
    compare_cubes(got, ost, part, nz, STATE, TOL)


VARIANTS = [dict(nord=0), dict(nord=1), dict(nord=2), dict(d_con=0.0), dict(do_vort_damp=False), dict(vtdm4=0.0), dict(hord_dp=5, hord_mt=5, hord_tm=5, hord_vt=5),
            dict(rf_fast=False), dict(d2_bg=0.02, d4_bg=0.0), dict(dddmp=0.0), dict(n_sponge=0), dict(ke_bg=1e-4), dict(p_fac=0.1), dict(d2_bg_k1=0.0, d2_bg_k2=0.0)]


@pytest.mark.parametrize("kw", VARIANTS, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_full_acoustic_call_config_variants(backend, kw):
    """Every dycore_config switch the acoustic path reads, away from the reference defaults
    (damping orders, heating / vorticity damping off, hord 5, Rayleigh damping off, sponge variants)."""
    nz = 8
    part, cfg, grids, ost, phis, odyn = oracle_cube(12, (1, 1), nz, dict(n_split=2, **kw))
    init = [{k: v.copy() for k, v in s.items()} for s in ost]
    odyn(ost, 112.5, 1)
    got, *_ = run_device_cube(backend, part, cfg, grids, init, phis, 112.5)
    compare_cubes(got, ost, part, nz, STATE, TOL)


@pytest.mark.parametrize("nz", [3, 127])
def test_full_acoustic_call_level_counts(backend, nz):
    """Smallest supported and largest configured level count (BASELINE cfg-5 uses L127)."""
    part, cfg, grids, ost, phis, odyn = oracle_cube(12, (1, 1), nz, dict(n_split=1))
    init = [{k: v.copy() for k, v in s.items()} for s in ost]
    odyn(ost, 112.5, 1)
    got, *_ = run_device_cube(backend, part, cfg, grids, init, phis, 112.5)
    compare_cubes(got, ost, part, nz, STATE, TOL)


@pytest.mark.parametrize("n", [65, 96])
def test_full_acoustic_call_multi_tile(backend, n):
    """C96 / C65: sub-domains span several strips (58 / 61 columns) and row segments (64) of the marching
    kernels -- interior waves, tile-edge waves, cube-corner patches, partial strips and a one-row last
    segment are all exercised."""
    nz = 4
    part, cfg, grids, ost, phis, odyn = oracle_cube(n, (1, 1), nz, dict(n_split=1))
    init = [{k: v.copy() for k, v in s.items()} for s in ost]
    odyn(ost, 60.0, 1)
    got, *_ = run_device_cube(backend, part, cfg, grids, init, phis, 60.0)
    compare_cubes(got, ost, part, nz, STATE, TOL)


@pytest.mark.parametrize("n, layout", [(65, (1, 1)), (24, (2, 2))])
def test_fused_scalar_march_is_bitwise_the_four_transports(backend, monkeypatch, n, layout):
    """d_sw's fused four-tracer march (fv3_tp4.hip) against the four single-tracer launches + the division kernel it
    replaces (FV3_DSW_SCALARS=separate): same expressions in the same order, so every field is bitwise equal -- on
    multi-strip sub-domains (C65: two strips, two row segments) and on 2 x 2 ranks."""
    nz = 4
    part, cfg, grids, ost, phis, _ = oracle_cube(n, layout, nz, dict(n_split=2))
    init = [{k: v.copy() for k, v in s.items()} for s in ost]
    res = {}
    for mode in ("pair", "quad", "separate"):  # pair (default): delp + w, then q_con + pt; quad: all four in one wave
        monkeypatch.setenv("FV3_DSW_SCALARS", mode)
        res[mode], *_ = run_device_cube(backend, part, cfg, grids, init, phis, 60.0)
    for r in range(part.total_ranks):
        for name in STATE:
            assert np.array_equal(res["pair"][r][name], res["separate"][r][name]), f"{name} rank {r} (pair)"
            assert np.array_equal(res["quad"][r][name], res["separate"][r][name]), f"{name} rank {r} (quad)"


@pytest.mark.parametrize("n, layout", [(65, (1, 1)), (24, (2, 2)), (12, (1, 1))])
def test_del_n_chains_inside_the_marches_are_bitwise_the_del6_launches(backend, monkeypatch, n, layout):
    """d_sw's scalar marches with the del-n damping chains run inside them (fv3_tp4.hip FD: levels below the sponge layers)
    against the same marches reading the damping fluxes four del6_stream launches wrote (FV3_DSW_DELN=arrays): same expressions
    in the same order, cube-corner patches from the staged chain in both, so every field is bitwise equal -- on multi-strip
    sub-domains, on 2 x 2 ranks (interior sub-domain edges, one cube corner each) and on sub-domains narrower than a strip."""
    nz = 6  # (levels 0..2 are the sponge layers: the array form inside the fused run; 3..5 run the chains in the march)
    part, cfg, grids, ost, phis, _ = oracle_cube(n, layout, nz, dict(n_split=2))
    init = [{k: v.copy() for k, v in s.items()} for s in ost]
    res = {}
    for mode in ("fused", "arrays"):
        monkeypatch.setenv("FV3_DSW_DELN", mode)
        res[mode], *_ = run_device_cube(backend, part, cfg, grids, init, phis, 60.0)
    for r in range(part.total_ranks):
        for name in STATE:
            assert np.array_equal(res["fused"][r][name], res["arrays"][r][name]), f"{name} rank {r}"


@pytest.mark.parametrize("n, layout, seg", [(130, (1, 1), "0"), (140, (2, 2), "0"), (24, (2, 2), "0"), (65, (1, 1), "0"), (200, (1, 1), "96"), (200, (1, 1), "32")])
def test_pair_march_is_bitwise_the_round4_march(backend, monkeypatch, n, layout, seg):
    """d_sw's two-tracer marches in their round-5 form (fv3_tp4x.hip: branch-free row step unrolled by three, general steps at the ends
    of a segment and on the cube-corner patches; every tile) against the round-4 kernels on every tile (FV3_DSW_MARCH=old): the same
    expressions in the same order, so every field is bitwise equal -- on sub-domains with interior strips between tile-edge strips,
    with S / N tile edges in the first / last segment, with several segments (whole triples, and segment lengths that leave one or
    two rows to the general steps) and on 2 x 2 ranks (one cube corner per sub-domain)."""
    nz = 6  # (levels 0..2 are the sponge layers: the round-4 kernel without the chains; 3..5 run the round-5 march)
    part, cfg, grids, ost, phis, _ = oracle_cube(n, layout, nz, dict(n_split=2))
    init = [{k: v.copy() for k, v in s.items()} for s in ost]
    if seg != "0":
        monkeypatch.setenv("FV3_SEG", seg)
    res = {}
    # "coupled" (round 6, measured and not the default): the two roles as wave pairs of one workgroup per tile on the device, the air-mass fluxes / the old air
    # mass / the rows both roles read handed over through LDS (the host emulation runs the two roles one after the other)
    for mode in ("new", "coupled", "old"):
        monkeypatch.setenv("FV3_DSW_MARCH", mode)
        res[mode], *_ = run_device_cube(backend, part, cfg, grids, init, phis, 60.0)
    for r in range(part.total_ranks):
        for name in STATE:
            assert np.array_equal(res["new"][r][name], res["old"][r][name]), f"{name} rank {r}"
            assert np.array_equal(res["coupled"][r][name], res["old"][r][name]), f"{name} rank {r} (coupled wave pairs)"


@pytest.mark.parametrize("n, layout, seg", [(130, (1, 1), "0"), (140, (2, 2), "0"), (24, (2, 2), "0"), (200, (1, 1), "96"), (200, (1, 1), "32"), (250, (2, 2), "0")])
def test_single_march_is_bitwise_the_round4_march(backend, monkeypatch, n, layout, seg):
    """The single-tracer transports with their del-n chain inside -- d_sw's vorticity transport with the wind update, update_dz_d's
    interface-height transport -- in their round-5 form (fv3_tp2x.hip; every tile: W / E one-sided formulas in the lanes, cube-corner
    remaps and patch fluxes in the general steps) against the round-4 kernel on every tile (FV3_TP2D_MARCH=old): bitwise equal
    states, on sub-domains with interior strips between tile-edge strips, several row segments and 2 x 2 ranks."""
    nz = 6
    part, cfg, grids, ost, phis, _ = oracle_cube(n, layout, nz, dict(n_split=2))
    init = [{k: v.copy() for k, v in s.items()} for s in ost]
    if seg != "0":
        monkeypatch.setenv("FV3_SEG", seg)
    res = {}
    for mode in ("new", "old"):
        monkeypatch.setenv("FV3_TP2D_MARCH", mode)
        res[mode], *_ = run_device_cube(backend, part, cfg, grids, init, phis, 60.0)
    for r in range(part.total_ranks):
        for name in STATE:
            assert np.array_equal(res["new"][r][name], res["old"][r][name]), f"{name} rank {r}"


@pytest.mark.parametrize("n, layout, seg", [(130, (1, 1), "0"), (140, (2, 2), "0"), (24, (2, 2), "0"), (200, (1, 1), "32")])
def test_damping_heat_in_the_vorticity_march_is_bitwise_the_heat_kernel(backend, monkeypatch, n, layout, seg):
    """d_sw's damping heat formed as the epilogue of the vorticity march (fv3_tp2x.hip HEAT: the pre-damping winds and the damping increments
    never stored) against the round-4 sequence (the march stores them, the damping-heat kernel reads them back; FV3_DSW_HEAT=separate): the
    heat enters pt through the diffusive heating at the end of the call -- every field bitwise equal."""
    nz = 6
    part, cfg, grids, ost, phis, _ = oracle_cube(n, layout, nz, dict(n_split=2))
    init = [{k: v.copy() for k, v in s.items()} for s in ost]
    if seg != "0":
        monkeypatch.setenv("FV3_SEG", seg)
    res = {}
    for mode in ("fused", "separate"):
        monkeypatch.setenv("FV3_DSW_HEAT", mode)
        res[mode], *_ = run_device_cube(backend, part, cfg, grids, init, phis, 60.0)
    for r in range(part.total_ranks):
        for name in STATE:
            assert np.array_equal(res["fused"][r][name], res["separate"][r][name]), f"{name} rank {r}"


@pytest.mark.parametrize("n, layout, seg, kw", [(24, (2, 2), "0", {}), (130, (1, 1), "0", {}), (140, (2, 2), "32", {}), (48, (1, 1), "0", dict(nord=2)), (12, (1, 1), "0", {}),
                                                (70, (1, 1), "0", dict(nord=1, dddmp=0.0)), (16, (2, 2), "0", {})])
def test_fused_wind_stage_is_bitwise_the_staged_kernels(backend, monkeypatch, n, layout, seg, kw):
    """d_sw's wind-branch stage kernels -- cell-mean vorticity, corner kinetic energy, the divergence-damping iteration, the corner interpolation of the vorticity
    and the Smagorinsky-type damping -- as ONE march (fv3_wind.hip; the tile-edge corners by one per-point launch, the chain's cube-corner patches from the staged
    chain) against the five staged launches (FV3_DSW_WINDSTAGE=staged): every field bitwise equal over two calls.  wk feeds the vorticity transport, ke and the
    damping field the wind update and the damping heat, so a wrong or missing cell / corner shows in u / v / pt.  Sub-domains with and without tile edges on
    every side (2 x 2 layouts), one and several strips / row segments, damping orders 1 - 3, the Smagorinsky term switched off."""
    nz = 6  # (levels 0..2 are the sponge layers: staged kernels either way; 3..5 run the fused march)
    part, cfg, grids, ost, phis, _ = oracle_cube(n, layout, nz, dict(n_split=2, **kw))
    init = [{k: v.copy() for k, v in s.items()} for s in ost]
    if seg != "0":
        monkeypatch.setenv("FV3_SEG", seg)
    res = {}
    for mode in ("fused", "staged"):
        monkeypatch.setenv("FV3_DSW_WINDSTAGE", mode)
        res[mode], *_ = run_device_cube(backend, part, cfg, grids, init, phis, 60.0, n_calls=2)
    for r in range(part.total_ranks):
        for name in STATE + ["uc", "vc"]:  # (uc / vc: the work values the damping chain leaves next to the cube corners -- FVDynamics-Out carries them)
            assert np.array_equal(res["fused"][r][name], res["staged"][r][name]), f"{name} rank {r}"


@pytest.mark.parametrize("n, layout, seg", [(130, (1, 1), "0"), (140, (2, 2), "32"), (70, (1, 1), "16")])
def test_side_copies_by_the_wind_stage_are_bitwise_the_copy_launches(backend, monkeypatch, n, layout, seg):
    """The damping-heat epilogue of d_sw's vorticity march differentiates the winds as they were before the march updates them in place; on the boundaries
    between its row segments / column strips it reads copies of them.  Default: the fused wind stage, which has every row of u and v in registers, stores
    those rows / columns (WindStage::u_side; the levels under it by sx_side_copy); FV3_DSW_SIDE=copy: two copy launches on every level.  Every field bitwise
    equal over two calls -- several strips (n = 130), several row segments of either march, both with different lengths (FV3_SEG), 2 x 2 sub-domains."""
    nz = 6
    part, cfg, grids, ost, phis, _ = oracle_cube(n, layout, nz, dict(n_split=2))
    init = [{k: v.copy() for k, v in s.items()} for s in ost]
    if seg != "0":
        monkeypatch.setenv("FV3_SEG", seg)
    res = {}
    for mode in ("march", "copy"):
        monkeypatch.setenv("FV3_DSW_SIDE", mode)
        res[mode], *_ = run_device_cube(backend, part, cfg, grids, init, phis, 60.0, n_calls=2)
    for r in range(part.total_ranks):
        for name in STATE:
            assert np.array_equal(res["march"][r][name], res["copy"][r][name]), f"{name} rank {r}"


@pytest.mark.parametrize("n, layout, seg", [(24, (2, 2), "0"), (130, (1, 1), "0"), (140, (2, 2), "32"), (48, (1, 1), "0")])
def test_vorticity_inside_the_corner_ke_march_is_bitwise_the_vorticity_launch(backend, monkeypatch, n, layout, seg):
    """d_sw's cell-mean relative vorticity formed by the corner-KE march for the cells under its corners (the march reads u and v anyway; the vorticity
    launch then only serves the frame around them; FV3_DSW_VORT_IN_KE=1, measured neutral and off by default) against the launch on the whole padded plane:
    every field bitwise equal -- the
    vorticity feeds the wind update, the Smagorinsky damping and the damping heat, so a wrong or missing cell shows in u / v / pt.  Sub-domains with and
    without tile edges on every side (2 x 2 layouts), one and several strips and row segments."""
    nz = 5
    part, cfg, grids, ost, phis, _ = oracle_cube(n, layout, nz, dict(n_split=2))
    init = [{k: v.copy() for k, v in s.items()} for s in ost]
    if seg != "0":
        monkeypatch.setenv("FV3_SEG", seg)
    res = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("FV3_DSW_VORT_IN_KE", mode)
        res[mode], *_ = run_device_cube(backend, part, cfg, grids, init, phis, 60.0)
    for r in range(part.total_ranks):
        for name in STATE:
            assert np.array_equal(res["1"][r][name], res["0"][r][name]), f"{name} rank {r}"


@pytest.mark.parametrize("n, layout", [(24, (2, 2)), (48, (1, 1))])
def test_heights_of_a_call_straight_into_zh_is_bitwise_the_reference_order(backend, monkeypatch, n, layout):
    """First sub-step of fv3_acoustic_step: set_gz -> zh, zh's halo update, update_dz_c in its zh -> gz form (no gz -> zh copy, no in-place update_dz_c)
    against the reference's order (gz filled, halo-updated, copied to zh, updated in place; FV3_GZ_FIRST=copy): every field bitwise equal over two calls."""
    nz = 6
    part, cfg, grids, ost, phis, _ = oracle_cube(n, layout, nz, dict(n_split=2))
    init = [{k: v.copy() for k, v in s.items()} for s in ost]
    res = {}
    for mode in ("direct", "copy"):
        monkeypatch.setenv("FV3_GZ_FIRST", mode)
        res[mode], *_ = run_device_cube(backend, part, cfg, grids, init, phis, 60.0, n_calls=2)
    for r in range(part.total_ranks):
        for name in STATE:
            assert np.array_equal(res["direct"][r][name], res["copy"][r][name]), f"{name} rank {r}"


@pytest.mark.parametrize("n, layout, n_split", [(24, (2, 2), 3), (48, (1, 1), 2)])
def test_layer_thickness_stored_by_the_last_sub_step_only_is_bitwise_every_sub_step(backend, monkeypatch, n, layout, n_split):
    """Inside fv3_acoustic_step riem_solver3 stores delz in the last sub-step of a call only: the sub-steps between work from zh, and everything that reads delz
    (the heights of the next call, the diffusive heating, the remap) comes after the last one.  FV3_SEQ_DELZ=every: the store in every sub-step, as the
    stand-alone operator does.  Every field -- delz included -- bitwise equal over two calls."""
    nz = 6
    part, cfg, grids, ost, phis, _ = oracle_cube(n, layout, nz, dict(n_split=n_split))
    init = [{k: v.copy() for k, v in s.items()} for s in ost]
    res = {}
    for mode in ("last", "every"):
        monkeypatch.setenv("FV3_SEQ_DELZ", mode)
        res[mode], *_ = run_device_cube(backend, part, cfg, grids, init, phis, 60.0, n_calls=2)
    for r in range(part.total_ranks):
        for name in STATE:
            assert np.array_equal(res["last"][r][name], res["every"][r][name]), f"{name} rank {r}"


@pytest.mark.parametrize("n, layout, n_split, kw", [(24, (2, 2), 3, {}), (48, (1, 1), 2, {}), (70, (1, 1), 2, dict(nord=0)), (32, (2, 2), 2, dict(nord=2))])
def test_a_grid_winds_stored_in_full_by_the_last_sub_step_only_is_bitwise_every_sub_step(backend, monkeypatch, n, layout, n_split, kw):
    """Inside fv3_acoustic_step the c_sw march of every sub-step but the last stores ua / va in full only on the levels where d_sw forms the divergence from
    them (no damping chain there) and, on the others, on the two cells next to its rectangle's boundary (c_sw's own boundary windows read those); the last
    sub-step stores everything -- ua / va are outputs of the call.  FV3_SEQ_UAVA=every: full stores in every sub-step.  Every field bitwise equal over two
    calls, with damping chains of order 0 (every level reads ua / va), 1 (the reference's) and 2, on sub-domains with and without tile edges on every side."""
    nz = 6
    part, cfg, grids, ost, phis, _ = oracle_cube(n, layout, nz, dict(n_split=n_split, **kw))
    init = [{k: v.copy() for k, v in s.items()} for s in ost]
    res = {}
    for mode in ("last", "every"):
        monkeypatch.setenv("FV3_SEQ_UAVA", mode)
        res[mode], *_ = run_device_cube(backend, part, cfg, grids, init, phis, 60.0, n_calls=2)
    for r in range(part.total_ranks):
        for name in STATE + ["uc", "vc"]:
            assert np.array_equal(res["last"][r][name], res["every"][r][name]), f"{name} rank {r}"


@pytest.mark.parametrize("n, layout, n_split, kw", [(24, (2, 2), 3, {}), (48, (1, 1), 2, {}), (130, (1, 1), 2, {}), (32, (2, 2), 4, dict(hord=5))])
def test_accumulators_formed_once_per_call_are_bitwise_the_read_modify_write_of_every_sub_step(backend, monkeypatch, n, layout, n_split, kw):
    """Inside fv3_acoustic_step the Courant numbers of every sub-step stay in arrays of their own and cxd / cyd are formed once, at the end of the last d_sw of the
    call, as ((0 + s1) + s2) + ... (acc_sum); FV3_ACC_DEFER=0: fxadv reads and writes them in every sub-step.  Every field -- the accumulators on their whole
    storages included -- bitwise equal over two calls; several strips / segments, sub-domains with and without tile edges, another PPM order."""
    nz = 6
    kw = dict(kw)
    if "hord" in kw:
        h = kw.pop("hord")
        kw.update(hord_dp=h, hord_tm=h, hord_vt=h, hord_mt=h)
    part, cfg, grids, ost, phis, _ = oracle_cube(n, layout, nz, dict(n_split=n_split, **kw))
    init = [{k: v.copy() for k, v in s.items()} for s in ost]
    res = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("FV3_ACC_DEFER", mode)
        res[mode], *_ = run_device_cube(backend, part, cfg, grids, init, phis, 60.0, n_calls=2)
    for r in range(part.total_ranks):
        for name in STATE:
            assert np.array_equal(res["1"][r][name], res["0"][r][name]), f"{name} rank {r}"


@pytest.mark.parametrize("n, layout, dz_min", [(24, (2, 2), None), (48, (1, 1), None), (24, (1, 1), 2500.0), (70, (1, 1), 4000.0)])
def test_height_scan_as_the_pre_sweep_of_riem_solver3_is_bitwise_the_scan_kernel(backend, monkeypatch, n, layout, dz_min):
    """Inside fv3_acoustic_step update_dz_d leaves its closing kernel -- the bottom-up scan that keeps the marched interface heights dz_min apart and forms the
    surface vertical velocity -- to riem_solver3, whose wave form runs it as a pre-sweep of each column: the limited heights go to the solver's LDS line for its
    first sweep and, only where the limit changed them, back into the marched field its third sweep reads (FV3_DZ_SCAN=separate: the scan kernel).  Every field
    bitwise equal over two calls; with the reference's dz_min (2 m: the limit never acts on these states) and with dz_min of the order of the layer thickness,
    where it acts in most columns (the case that exercises the conditional write-back)."""
    import dataclasses

    nz = 6
    part, cfg, grids, ost, phis, _ = oracle_cube(n, layout, nz, dict(n_split=2))
    init = [{k: v.copy() for k, v in s.items()} for s in ost]
    cst = dataclasses.replace(get_constants(), DZ_MIN=dz_min) if dz_min else None
    res = {}
    for mode in ("presweep", "separate"):
        monkeypatch.setenv("FV3_DZ_SCAN", mode)
        res[mode], *_ = run_device_cube(backend, part, cfg, grids, init, phis, 60.0, n_calls=2, constants=cst)
    for r in range(part.total_ranks):
        for name in STATE:
            assert np.array_equal(res["presweep"][r][name], res["separate"][r][name], equal_nan=True), f"{name} rank {r}"
    if dz_min:  # (the limit must have acted: the same run with the reference's dz_min gives other heights)
        ref, *_ = run_device_cube(backend, part, cfg, grids, init, phis, 60.0, n_calls=2)
        assert any(not np.array_equal(res["presweep"][r]["delz"], ref[r]["delz"]) for r in range(part.total_ranks))
        assert all(np.isfinite(res["presweep"][r]["delz"]).all() for r in range(part.total_ranks))


@pytest.mark.parametrize("n, layout, alt", [(12, (1, 1), ""), (24, (2, 2), ""), (59, (1, 1), ""), (140, (2, 2), ""), (130, (1, 1), ""), (24, (1, 1), "heat_zero_first_call")])
def test_fused_smoothing_and_heating_is_bitwise_the_staged_operators(backend, monkeypatch, n, layout, alt):
    """fv3_acoustic_step's damping-heat tail as one pass (fv3_del2x.hip: three del2_cubed iterations in LDS + apply_diffusive_heating) against the staged
    operators (three launches + the heating kernel, FV3_DEL2_FUSED=0): every field bitwise equal.  The sizes put tile boundaries of the fused kernel at
    their natural places (C130, C24) and at the shifted ones next to the far tile edge (12 and 70 rows: boundary moved in j; 59 columns: in i), with one
    and with several cube corners per tile; under FV3_ALT=heat_zero_first_call the smoothed heat is kept and carried into a second call."""
    nz = 5
    if alt:
        monkeypatch.setenv("FV3_ALT", alt)
    part, cfg, grids, ost, phis, _ = oracle_cube(n, layout, nz, dict(n_split=2))
    init = [{k: v.copy() for k, v in s.items()} for s in ost]
    res = {}
    for mode in ("tiles", "tiles+heat", "staged"):  # (default: LDS-tile smoothing + heating launch; heating as the tile kernel's epilogue; round-4 operators)
        monkeypatch.setenv("FV3_DEL2_FUSED", "0" if mode == "staged" else "1")
        monkeypatch.setenv("FV3_DEL2_HEAT", "fused" if mode == "tiles+heat" else "split")
        res[mode], *_ = run_device_cube(backend, part, cfg, grids, init, phis, 60.0, n_calls=2 if alt else 1)
    for r in range(part.total_ranks):
        for name in STATE:
            assert np.array_equal(res["tiles"][r][name], res["staged"][r][name]), f"{name} rank {r}"
            assert np.array_equal(res["tiles+heat"][r][name], res["staged"][r][name]), f"{name} rank {r} (heating in the tile kernel)"


@pytest.mark.parametrize("n, layout, kw, n_calls, alt", [(24, (2, 2), dict(n_split=3), 2, ""), (130, (1, 1), dict(n_split=2), 1, ""), (24, (1, 1), dict(n_split=2), 3, "heat_zero_first_call")])
def test_first_sub_step_store_of_the_flux_accumulators_is_bitwise_zero_plus_accumulate(backend, monkeypatch, n, layout, kw, n_calls, alt):
    """fv3_acoustic_step's first sub-step has d_sw STORE 0 + flux into mfx / mfy / cx / cy (the zero read from a 4 KB block; four zero launches and
    four field reads less per call) against zeroing the four fields and accumulating on every sub-step as the reference does (FV3_ACC_STORE=0):
    every field bitwise equal, the accumulators included -- over two calls (the second one finds arrays the first call has filled).  The accumulated
    damping heat (heat_source) is treated the same way; under FV3_ALT=heat_zero_first_call it is reset by the first call only and carried through the others."""
    nz = 5
    if alt:
        monkeypatch.setenv("FV3_ALT", alt)
    part, cfg, grids, ost, phis, _ = oracle_cube(n, layout, nz, kw)
    init = [{k: v.copy() for k, v in s.items()} for s in ost]
    res = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("FV3_ACC_STORE", mode)
        res[mode], *_ = run_device_cube(backend, part, cfg, grids, init, phis, 60.0, n_calls=n_calls)
    for r in range(part.total_ranks):
        for name in STATE:
            assert np.array_equal(res["1"][r][name], res["0"][r][name]), f"{name} rank {r}"
        assert np.abs(res["1"][r]["mfxd"]).max() > 0.0 and np.abs(res["1"][r]["cxd"]).max() > 0.0


@pytest.mark.parametrize("n, layout, kw", [(24, (2, 2), dict(n_split=3)), (12, (1, 1), dict(n_split=2)), (70, (1, 1), dict(n_split=1))])
def test_acoustic_call_does_not_depend_on_what_the_accumulators_held(backend, monkeypatch, n, layout, kw):
    """Statelessness of the call [REF tests/main/fv3core/test_dycore_call.py:169-190]: the reference empties mfxd / mfyd / cxd / cyd (and its heat_source work
    array) in full at the start of every call.  Here the first sub-step stores 0 + flux on the cells d_sw writes and the sequencer zeroes the REST of every plane
    (frame, padding level) on every call -- no "already zeroed" flag.  Between two calls the host overwrites the whole storages with NaN (a restart load, a
    debugger's poison, an allocator handing the address to someone else in between): the second call must leave every element of the storages -- halos, the 3 x 3
    blocks beyond a cube corner, the padding level -- bitwise what zero + accumulate (FV3_ACC_STORE=0) leaves, and no NaN anywhere."""
    from pace_amd.dyn_core import AcousticDynamics, DycoreState
    from pace_amd.halo import Layout

    nz = 5
    part, cfg, grids, ost, phis, _ = oracle_cube(n, layout, nz, kw)
    init = [dict({k: v.copy() for k, v in s.items()}, phis=p) for s, p in zip(ost, phis)]
    raw = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("FV3_ACC_STORE", mode)
        sf = stencil_factory_for(backend)(grids, cfg, get_constants())
        st = DycoreState.from_arrays(sf.quantity_factory, init)
        dyn = AcousticDynamics(Layout(part, 1, 0), grids, sf, config=cfg, phis=st.phis, state=st)
        dyn(st, 60.0, n_map=1)
        for q in (st.mfxd, st.mfyd, st.cxd, st.cyd, dyn._heat_source):
            q.storage.fill_(float("nan"))
        dyn(st, 60.0, n_map=2)
        if backend != "hostemu":
            torch.cuda.synchronize()
        raw[mode] = {name: getattr(st, name).storage.cpu().numpy().copy() for name in STATE}
        raw[mode]["heat_source"] = dyn._heat_source.storage.cpu().numpy().copy()
    for name, a in raw["1"].items():
        assert np.all(np.isfinite(a)), f"{name}: the call left cells it did not define"
        assert np.array_equal(a, raw["0"][name]), f"{name}: differs from zero + accumulate somewhere in the storage"
    assert np.abs(raw["1"]["mfxd"]).max() > 0.0 and np.abs(raw["1"]["cyd"]).max() > 0.0


@pytest.mark.parametrize("n, layout", [(130, (1, 1)), (140, (2, 2)), (24, (2, 2))])
def test_height_del_n_chain_inside_the_transport_march_is_bitwise_the_del6_launch(backend, monkeypatch, n, layout):
    """update_dz_d: the del-n chain of the interface heights run inside the transport march (tp2d_stream_t TF_FD, strips away from
    the W / E tile edges; tile-edge strips and corner patches still from del6_stream) against the chain as its own launch
    (FV3_DZ_DELN=arrays).  C130: an interior strip between two tile-edge strips; C140 2 x 2: sub-domains whose second strip is
    interior or tile-edge depending on the side; two row segments."""
    nz = 3
    part, cfg, grids, ost, phis, _ = oracle_cube(n, layout, nz, dict(n_split=1, k_split=1))
    init = [{k: v.copy() for k, v in s.items()} for s in ost]
    res = {}
    for mode in ("fused", "arrays"):
        monkeypatch.setenv("FV3_DZ_DELN", mode)
        res[mode], *_ = run_device_cube(backend, part, cfg, grids, init, phis, 60.0)
    for r in range(part.total_ranks):
        for name in STATE:
            assert np.array_equal(res["fused"][r][name], res["arrays"][r][name]), f"{name} rank {r}"


@pytest.mark.parametrize("n, layout", [(130, (1, 1)), (140, (2, 2)), (24, (2, 2))])
def test_vorticity_del_n_chain_inside_the_transport_march_is_bitwise_the_del6_launch(backend, monkeypatch, n, layout):
    """d_sw's vorticity transport with the relative vorticity's del-n chain run inside the march and the absolute vorticity formed
    on load (wk + f0; tp2d_stream_t TF_WIND | TF_FD) against the round-2 form (absolute-vorticity field + del6_stream launch,
    FV3_DSW_VORT_DELN=arrays): bitwise equal states."""
    nz = 4
    part, cfg, grids, ost, phis, _ = oracle_cube(n, layout, nz, dict(n_split=1, k_split=1))
    init = [{k: v.copy() for k, v in s.items()} for s in ost]
    res = {}
    for mode in ("fused", "arrays"):
        monkeypatch.setenv("FV3_DSW_VORT_DELN", mode)
        res[mode], *_ = run_device_cube(backend, part, cfg, grids, init, phis, 60.0)
    for r in range(part.total_ranks):
        for name in STATE:
            assert np.array_equal(res["fused"][r][name], res["arrays"][r][name]), f"{name} rank {r}"


@pytest.mark.parametrize("n, layout", [(130, (1, 1)), (140, (2, 2)), (24, (2, 2)), (12, (1, 1))])
def test_fused_nh_p_grad_is_bitwise_the_staged_form(backend, monkeypatch, n, layout):
    """nh_p_grad as one marching kernel (fv3_pgf.hip: the four corner interpolations + the wind update, corner fields never
    stored; per-point evaluation next to the tile edges) against the staged form (four a2b_ord4 launches + the level-walking
    update, FV3_NH_PGF=staged) -- also split into the sequencer's frame-first passes: bitwise equal states."""
    nz = 4
    part, cfg, grids, ost, phis, _ = oracle_cube(n, layout, nz, dict(n_split=2, k_split=1))
    init = [{k: v.copy() for k, v in s.items()} for s in ost]
    res = {}
    for mode, pgf, ff in (("fused", "fused", "0"), ("fused, frame-first", "fused", "1"), ("staged", "staged", "0")):
        monkeypatch.setenv("FV3_NH_PGF", pgf)
        monkeypatch.setenv("FV3_FRAME_FIRST", ff)
        res[mode], *_ = run_device_cube(backend, part, cfg, grids, init, phis, 60.0)
    for mode in ("fused", "fused, frame-first"):
        for r in range(part.total_ranks):
            for name in STATE:
                assert np.array_equal(res[mode][r][name], res["staged"][r][name]), f"{name} rank {r} ({mode})"


@pytest.mark.parametrize("n, layout, n_split", [(24, (2, 2), 3), (12, (1, 1), 2)])
def test_frame_first_passes_are_bitwise_neutral(backend, monkeypatch, n, layout, n_split):
    """fv3_acoustic_step with the operators that feed a halo update split into frame + interior passes (p_grad_c -> uc / vc;
    nh_p_grad + ray_fast -> u / v / w, whose updates then start before the interior is computed: the multi-process overlap) against
    the unsplit sequence: every array equal including its halos, for even and odd sub-step counts."""
    nz = 5
    part, cfg, grids, ost, phis, _ = oracle_cube(n, layout, nz, dict(n_split=n_split, k_split=1))
    init = [{k: v.copy() for k, v in s.items()} for s in ost]
    res = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("FV3_FRAME_FIRST", mode)
        res[mode], *_ = run_device_cube(backend, part, cfg, grids, init, phis, 60.0, n_calls=2)
    for r in range(part.total_ranks):
        for name in STATE + ["uc", "vc"]:
            assert np.array_equal(res["1"][r][name], res["0"][r][name]), f"{name} rank {r}"


def test_native_and_python_sequencers_are_identical(backend):
    """fv3_acoustic_step (C, the product path) and its Python twin in dyn_core.py issue the same
    operator / halo sequence: bitwise equal states, and the per-operator profile is populated."""
    nz = 5
    part, cfg, grids, ost, phis, _ = oracle_cube(12, (1, 1), nz, dict(n_split=2, k_split=2))
    init = [{k: v.copy() for k, v in s.items()} for s in ost]
    a, dyn, _, sf = run_device_cube(backend, part, cfg, grids, init, phis, 112.5, n_calls=2, native=True)
    sf.set_profiling(True)
    b, *_ = run_device_cube(backend, part, cfg, grids, init, phis, 112.5, n_calls=2, native=False)
    for r in range(part.total_ranks):
        for name in STATE + ["uc", "vc"]:
            assert np.array_equal(a[r][name], b[r][name]), f"{name} rank {r} differs between the sequencers"
    st = dyn._updaters and dyn  # the first run's dynamics object: profile it for one more call
    from pace_amd.dyn_core import DycoreState

    state = DycoreState.from_arrays(sf.quantity_factory, [dict(s, phis=p) for s, p in zip(init, phis)])
    st(state, 112.5, n_map=1)
    prof = sf.profile()
    assert prof["d_sw"][1] == 2 and prof["c_sw"][1] == 2 and prof["halo"][1] > 10, prof


# (the real-model-data test lives in tests/test_restart_six_tiles.py: all six tiles of the reference's FV3 restart, not tile 1 replicated)


def test_baroclinic_wave_state(backend):
    """JW2006 baroclinic wave (the reference's default analytic init): the balanced zonal flow must
    stay put over an acoustic call -- tendencies are truncation-error small -- and the HIP path must
    agree with the oracle on it like on the synthetic state."""
    from fv3_oracle.dyn_core import OracleAcousticDynamics
    from pace_amd.init import baroclinic_state

    nx, nz = 24, 79
    part = CubedSpherePartitioner(nx, (1, 1))
    cfg = AcousticDynamicsConfig(npx=nx + 1, npy=nx + 1, npz=nz, layout=(1, 1), n_split=2)
    grids = [make_grid(part, r, nz=nz) for r in range(6)]
    init = [baroclinic_state(g) for g in grids]
    phis = [s.pop("phis") for s in init]
    ost = [{k: v.copy() for k, v in s.items()} for s in init]
    odyn = OracleAcousticDynamics(part, grids, cfg, get_constants(), phis)
    odyn(ost, 225.0, 1)
    got, *_ = run_device_cube(backend, part, cfg, grids, init, phis, 225.0)
    # w / omga are ~1e-3 m/s here (balanced state): the absolute floor W_ATOL covers the solver's exp / log round-off
    compare_cubes(got, ost, part, nz, STATE, TOL, atol=W_ATOL)
    # balance: after 225 s the wind changed by a small fraction of u0 = 35 m/s, w stays small, pt within 1e-3 relative
    for r in range(6):
        sl = (slice(3, 3 + nx), slice(3, 3 + nx), slice(0, nz))
        du = np.abs(got[r]["u"][sl] - init[r]["u"][sl]).max()
        assert du < 2.0, f"rank {r}: zonal flow drifted by {du} m/s in one step"
        assert np.abs(got[r]["w"][sl]).max() < 1.0
        assert np.abs(got[r]["pt"][sl] / init[r]["pt"][sl] - 1.0).max() < 5e-3


_SEQUENCER_STATE_REFERENCE = {}  # backend -> what a fresh context gives (computed once, never changed)


def _standalone_operators_and_a_full_call(sf, part, cfg, grids, init, phis, nz):
    """c_sw and riem_solver3 on their own (the `stencils` wrappers) and one complete acoustic call on context `sf`, each on fresh copies of the
    inputs: every output as its WHOLE storage (halos, padding and the level nz included)."""
    from helpers import DIMS3
    from pace_amd import stencils
    from pace_amd.dyn_core import AcousticDynamics, DycoreState
    from pace_amd.halo import Layout

    qf, c = sf.quantity_factory, get_constants()
    q3 = lambda arrays: qf.from_array([np.array(a) for a in arrays], DIMS3)  # noqa: E731
    q2 = lambda arrays: qf.from_array([np.array(a) for a in arrays], ("x", "y"))  # noqa: E731
    out = {}
    # c_sw: inside the sequencer it may thin out its ua / va stores and leave windows running on the auxiliary stream
    names = ("delp", "pt", "u", "v", "w", "uc", "vc", "ua", "va", "omga")
    Q = {n: q3([s[n] for s in init]) for n in names}
    T = {n: qf.zeros(DIMS3) for n in ("ut", "vt", "divgd")}
    delpc, ptc = stencils.CGridShallowWaterDynamics(sf)(*[Q[n] for n in names[:9]], T["ut"], T["vt"], T["divgd"], Q["omga"], 56.25)
    out.update({"c_sw " + n: x for n, x in list(Q.items()) + list(T.items()) + [("delpc", delpc), ("ptc", ptc)]})
    # riem_solver3: inside the sequencer it may skip the delz store, run one frame-first pass only, or take update_dz_d's scan as a pre-sweep
    zs = [p * c.RGRAV for p in phis]
    zh = []
    for s, z in zip(init, zs):
        h = np.zeros_like(s["u"])
        h[:, :, nz] = z[:, :, 0]
        for k in range(nz - 1, -1, -1):
            h[:, :, k] = h[:, :, k + 1] - s["delz"][:, :, k]
        zh.append(h)
    names = ("cappa", "delz", "q_con", "delp", "pt", "pe", "pk", "peln", "w")
    Q = {n: q3([s[n] for s in init]) for n in names}
    Q.update(zh=q3(zh), ppe=qf.zeros(DIMS3), pk3=qf.zeros(DIMS3))
    stencils.RiemannSolver3(sf)(1, 18.75, Q["cappa"], grids[0].ptop, q2(zs), q2([np.full_like(z, 0.01) for z in zs]), Q["delz"], Q["q_con"], Q["delp"], Q["pt"],
                                Q["zh"], Q["pe"], Q["ppe"], Q["pk3"], Q["pk"], Q["peln"], Q["w"])
    out.update({"riem_solver3 " + n: x for n, x in Q.items()})
    # one complete call from the initial state, the way every other test makes it
    st = DycoreState.from_arrays(qf, [dict({k: v.copy() for k, v in s.items()}, phis=p) for s, p in zip(init, phis)])
    AcousticDynamics(Layout(part, 1, 0), grids, sf, config=cfg, phis=st.phis, state=st)(st, 225.0, n_map=1)
    out.update({"acoustic " + n: getattr(st, n) for n in STATE})
    if not sf.hostemu:
        torch.cuda.synchronize()
    return {n: x.storage.detach().cpu().numpy().copy() for n, x in out.items()}


# (update, phase, which request of that kind) at which the halo callback reports an error: the very first request of the call; the start of
# delp / pt / q_con behind the first sub-step's d_sw (about its middle); the start of zh behind the first sub-step's riem_solver3 (the first
# start of zh belongs to the heights of the call); the first request of the second sub-step
@pytest.mark.parametrize("fail_at", [("q_con__cappa", 0, 1), ("delp__pt__q_con", 0, 1), ("zh", 0, 2), ("w", 0, 2)], ids=lambda f: f"{f[0]}.{f[1]}#{f[2]}")
def test_failed_acoustic_call_leaves_no_sequencer_state(backend, fail_at):
    """fv3_acoustic_step tells its operators about the call they are part of (fv3_seq_hints: not the last sub-step, first sub-step, frame-first
    pass, ...).  None of it may outlive the call, also when the call ends early: after an acoustic call that a failing halo request cut short,
    c_sw and riem_solver3 on their own and a complete acoustic call give, on the SAME context, bitwise what a fresh context gives -- ua, va and
    delz (the stores the sequencer's hints thin out or skip) over their whole storages like everything else."""
    from pace_amd import lib as _lib
    from pace_amd.dyn_core import AcousticDynamics, DycoreState
    from pace_amd.halo import Layout

    nz = 5
    part, cfg, grids, init, phis, _ = oracle_cube(12, (1, 1), nz, dict(n_split=2))
    make_sf = lambda: stencil_factory_for(backend)(grids, cfg, get_constants())  # noqa: E731
    if backend not in _SEQUENCER_STATE_REFERENCE:
        _SEQUENCER_STATE_REFERENCE[backend] = _standalone_operators_and_a_full_call(make_sf(), part, cfg, grids, init, phis, nz)
    want = _SEQUENCER_STATE_REFERENCE[backend]

    sf = make_sf()
    st = DycoreState.from_arrays(sf.quantity_factory, [dict({k: v.copy() for k, v in s.items()}, phis=p) for s, p in zip(init, phis)])
    dyn = AcousticDynamics(Layout(part, 1, 0), grids, sf, config=cfg, phis=st.phis, state=st)
    dyn._build_native_args(st)
    c_state, c_work, _, errors = dyn._native_args
    ups = [dyn._updaters[n] for n in _lib.HALO_UPDATES]
    seen = []

    def halo(_user, update, phase, stream):  # the test's own callback: forwards to the updaters, reports an error at the chosen request
        seen.append((_lib.HALO_UPDATES[update], phase))
        if seen[-1] == fail_at[:2] and seen.count(seen[-1]) == fail_at[2]:
            return 1
        (ups[update].start if phase == 0 else ups[update].wait)(stream)
        return 0

    dyn._native_args = (c_state, c_work, _lib.fv3_halo_fn(halo), errors)
    with pytest.raises(_lib.Fv3Error, match="halo callback reported an error"):
        dyn(st, 225.0, n_map=1)
    assert seen[-1] == fail_at[:2]  # (the call ended at that request ...)
    assert (len(seen) == 1) == (fail_at[0] == "q_con__cappa") and seen.count(("w", 0)) == {"q_con__cappa": 0, "w": 2}.get(fail_at[0], 1)  # (... in that sub-step)
    for u in ups:
        u.wait()  # (what the cut-short call started and never waited for)

    got = _standalone_operators_and_a_full_call(sf, part, cfg, grids, init, phis, nz)
    assert set(got) == set(want)
    for n in want:
        assert np.array_equal(got[n], want[n], equal_nan=True), n
