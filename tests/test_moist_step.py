"""Moist thermodynamics inside the step: fv3_remap_moist (pace_amd/csrc/fv3_remap.hip) against fv3_remap (+ fv3_fillz) and the numpy
restatement of moist_cv (tests/moist_reference.py), its argument checks, DynamicalCore(water_species=...) /
DycoreHarness(moist=True) against the same operators called by hand, the decomposition, the neutrality of the default paths and the
driver's --moist.  The operator and step cases run on the host emulation (CPU suite) and on the HIP library (-m gpu).

The inputs of the remap cases are the state a moist harness holds right before its first remap (preamble, acoustic call, tracer
advection: genuinely Lagrangian levels), with a few negative condensate values planted in the species so that the filling has work
on every shape.  Errors are max-normalised (tests/helpers.py: assert_close)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
import yaml

import fillz_reference as fref
import moist_reference as mref
import test_thermo as tt
import zarr_v2_read as zr
from pace_amd import driver, lib as _lib
from pace_amd._testing import harness_for
from pace_amd.constants import get_constants
from pace_amd.dyn_core import STATE_NAMES
from pace_amd.harness import WATER_NAMES
from pace_amd.stencils import FillNegativeTracerValues, LagrangianToEulerian, MoistCV, PotentialToTemperature, TemperatureToPotential, WaterSpecies
from test_thermo import real  # noqa: F401  (the (backend, dtype) fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "c12_restart_6tiles.npz")
NH = 3
CONDENSATE = ("qliquid", "qrain", "qice", "qsnow", "qgraupel")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _compute(q, r):
    """the compute domain of sub-domain r (the staggered / interface end included where the quantity has one), host copy"""
    return q.sub(r).view[...].detach().cpu().numpy().copy()  # (on the host emulation .numpy() is a view of the live storage)


def _snapshot(h, ps):
    out = {n: [_compute(getattr(h.state, n), r) for r in range(len(h.grids))] for n in STATE_NAMES}
    for n, q in h.tracers.items():
        out[n] = [_compute(q, r) for r in range(len(h.grids))]
    out["ps"] = [_compute(ps, r) for r in range(len(h.grids))]
    return out


def _assert_same(a, b, what, skip=()):
    assert set(a) == set(b)
    for n in a:
        if n in skip:
            continue
        for r, (x, y) in enumerate(zip(a[n], b[n])):
            assert x.shape == y.shape and np.array_equal(_bits(x), _bits(y)), (what, n, r, float(np.abs(x - y).max()))


def _restated(snap, r, nz):
    """(q_con, cappa) of the restatement from the species of a snapshot"""
    sp = {role: snap[role][r][..., :nz] for role in mref.ROLES}
    q_con, cappa, _ = mref.moist_cv(**sp)
    return q_con, cappa


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. fv3_remap_moist against fv3_remap (+ fv3_fillz) on copies of the same inputs
# ---------------------------------------------------------------------------------------------------------------------------------
class BeforeRemap:
    """A moist harness advanced to the point right before its first remap, every field saved: `restore()` puts the saved inputs back,
    so that several remaps run on copies of the same inputs."""

    def __init__(self, backend, n, layout, nz, dtype=torch.float64, plant=True, **kw):
        over = dict(config_overrides=dict(nord=0)) if dtype == torch.float32 else {}  # (fp32: the C12 del-6 tables leave the float range)
        self.h = h = harness_for(backend)(n, nz=nz, layout=layout, dt_atmos=225.0, k_split=1, n_split=2, n_tracers=7, hord_tr=8, remap=True, temperature=True, moist=True,
                                          dtype=dtype, **over, **kw)
        self.nz, self.n = nz, h.part.nx
        s, d = h.state, h.dycore
        d.temperature_to_potential(s.pt, s.pkz, s.delp, s.delz, s.q_con, s.cappa, water=d.water)
        d.dp1.storage.copy_(s.delp.storage)
        d.acoustic_dynamics(s, 225.0, n_map=1)
        d._tracer_halo.update()
        d.tracer_advection(d.tracers, d.dp1, s.mfxd, s.mfyd, s.cxd, s.cyd)
        h.synchronize()
        if plant:  # slightly negative condensate means in one cell in forty, at every level: what a remap leaves for fillz
            rng = np.random.default_rng(7 + nz)
            for role in CONDENSATE:
                q = d.tracers[role]
                for r in range(len(h.grids)):
                    a = q.numpy(r)
                    m = rng.random(a.shape) < 0.025
                    a[m] = -np.abs(a[m]) * 0.3 - 1.0e-9
                    q.set_numpy(a, r)
        self.fields = {n: getattr(s, n) for n in STATE_NAMES}
        self.fields.update(d.tracers)
        self.fields["ps"], self.fields["wsd"] = d.ps, d.acoustic_dynamics._wsd
        self.saved = {k: q.storage.clone() for k, q in self.fields.items()}

    def restore(self):
        for k, q in self.fields.items():
            q.storage.copy_(self.saved[k])

    def run(self, moist, fill):
        """One remap on the saved inputs: the moist entry with its own `fill`, or the dry entry (given the incoming cappa) followed by
        fv3_fillz where `fill`.  Returns the snapshot of every state field, the tracers and ps."""
        h = self.h
        s, d = h.state, h.dycore
        self.restore()
        args = (d.tracers, s.pt, s.delp, s.delz, s.peln, s.pe, s.pk, s.pkz, s.u, s.v, s.w, s.cappa, d.ps, d.acoustic_dynamics._wsd)
        if moist:
            LagrangianToEulerian(h.sf, fill=fill)(*args, q_con=s.q_con, water=d.water)
        else:
            LagrangianToEulerian(h.sf)(*args)
            if fill:
                FillNegativeTracerValues(h.sf)(s.delp, d.tracers)
        h.synchronize()
        return _snapshot(h, d.ps)


SAME_AS_DRY = ("w", "delz", "u", "v", "delp", "pe", "peln", "pk", "ps")
REMAP_SHAPES = [(12, (1, 1), 5), (12, (1, 1), 6), (12, (1, 1), 8), (24, (2, 2), 7)]


def _check_moist_against_dry(B, fill, npd, worst):
    h, nz = B.h, B.nz
    c = get_constants()
    wet, dry = B.run(True, fill), B.run(False, fill)
    for name in SAME_AS_DRY + tuple(h.tracers):
        for r, (x, y) in enumerate(zip(wet[name], dry[name])):
            assert np.array_equal(_bits(x), _bits(y)), (name, r, fill)
    rrg = npd(-c.RDGAS / c.GRAV)
    for r in range(len(h.grids)):
        q_con, cappa = _restated(wet, r, nz)
        assert np.array_equal(_bits(wet["q_con"][r][..., :nz]), _bits(q_con)), ("q_con", r, fill)
        assert np.array_equal(_bits(wet["cappa"][r][..., :nz]), _bits(cappa)), ("cappa", r, fill)
        # pkz / pt with the new cappa, from the dry entry's outputs: the device's T_v is pt_dry * pkz_dry to a rounding
        own, r64 = [], []
        for dt, out in ((npd, own), (np.float64, r64)):
            f = lambda k: dry[k][r][..., :nz].astype(dt)  # noqa: E731
            tv = f("pt") * f("pkz")
            pz = np.exp(cappa.astype(dt) * np.log(dt(rrg) * f("delp") / f("delz") * tv))
            out += [pz, tv / pz]
        tt._bound("pkz", wet["pkz"][r][..., :nz], own[0], r64[0], npd, worst)
        tt._bound("pt", wet["pt"][r][..., :nz], own[1], r64[1], npd, worst)
    return wet, dry


@pytest.mark.parametrize("n, layout, nz", REMAP_SHAPES, ids=[f"c{s[0]}_{s[1][0]}x{s[1][1]}_l{s[2]}" for s in REMAP_SHAPES])
def test_remap_moist_against_the_dry_remap(real, n, layout, nz):  # noqa: F811
    backend, dtype = real
    npd = tt.NP_OF[dtype]
    B = BeforeRemap(backend, n, layout, nz, dtype)
    worst = {}
    for fill in (False, True):
        wet, dry = _check_moist_against_dry(B, fill, npd, worst)
        if fill:  # the planted negatives gave the filling something to do
            nofill = B.run(False, False)
            assert any(not np.array_equal(_bits(a), _bits(b)) for role in CONDENSATE for a, b in zip(dry[role], nofill[role]))
    print(f"remap_moist {backend} {npd.__name__} C{n} {layout} L{nz}: (error, E_ref) " + ", ".join(f"{k} ({v[0]:.2e}, {v[1]:.2e})" for k, v in worst.items()))
    B.h.close()


def test_remap_moist_fills_before_moist_cv_on_the_real_restart_state(backend):
    """Order control: the fixture's liq_wat has negative layer means, and FV3 derives q_con after the filling.  With fill the condensate
    is non-negative below the top level in every column that got the non-local fix, and it differs from the fill = 0 result."""
    data = np.load(FIXTURE)
    nz = data["T"].shape[1]
    B = BeforeRemap(backend, 12, (1, 1), nz, plant=False, init="restart", init_data=data, ak=data["ak"], bk=data["bk"])
    worst = {}
    wet0, dry0 = _check_moist_against_dry(B, False, np.float64, worst)
    # (on the CPU, first) the remapped condensate really gives fillz something to change, the non-local fix included
    nonlocal_cols, changed = [], 0
    for r in range(6):
        q, dp = dry0["qliquid"][r][..., :nz].reshape(-1, nz), dry0["delp"][r][..., :nz].reshape(-1, nz)
        filled, br = fref.fillz(q, dp)
        changed += int((_bits(filled) != _bits(q)).sum())
        nonlocal_cols.append(br["nonlocal"].reshape(12, 12))
    assert changed > 0 and sum(int(m.sum()) for m in nonlocal_cols) > 0, (changed, [int(m.sum()) for m in nonlocal_cols])
    wet1, _ = _check_moist_against_dry(B, True, np.float64, worst)
    differs = 0
    for r in range(6):
        q0, q1 = wet0["q_con"][r][..., :nz], wet1["q_con"][r][..., :nz]
        differs += int((_bits(q0) != _bits(q1)).sum())
        assert (q1[nonlocal_cols[r]][:, 1:] >= 0.0).all()
        assert (q0[nonlocal_cols[r]][:, 1:] < 0.0).any()  # ... which the unfilled condensate is not
    assert differs > 0
    print(f"remap_moist real data {backend}: fillz changes {changed} values, {sum(int(m.sum()) for m in nonlocal_cols)} columns take the non-local fix, q_con differs in {differs} cells; "
          + ", ".join(f"{k} {v[0]:.2e}" for k, v in worst.items()))
    B.h.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. argument checks of fv3_remap_moist through the C ABI
# ---------------------------------------------------------------------------------------------------------------------------------
def test_remap_moist_argument_checks(backend):
    B = BeforeRemap(backend, 12, (1, 1), 5)
    h = B.h
    s, d, sf = h.state, h.dycore, h.sf
    qf = sf.quantity_factory
    lib, ctx, stream = sf.lib, sf.ctx, sf.stream_handle
    flat, loose = qf.zeros(("x", "y")), qf.zeros(("x", "y", "z"))  # (loose: a well-formed field that is no tracer)
    short = _lib.fv3_field()
    C.memmove(C.byref(short), C.byref(loose.field), C.sizeof(_lib.fv3_field))
    short.shape[2] -= 1
    B.restore()
    before = {k: q.storage.clone() for k, q in B.fields.items()}
    ARG = -1
    names = ("pt", "delp", "delz", "peln", "pe", "pk", "pkz", "u", "v", "w", "cappa", "q_con")

    def ref(v):
        return None if v is None else (C.pointer(v) if isinstance(v, _lib.fv3_field) else C.pointer(v.field))

    def call(no_water=False, tracers=None, n_tracers=None, null_list=False, **swap):
        trs = list(d.tracers.values()) if tracers is None else tracers
        arr = (_lib.F * max(len(trs), 1))(*[ref(q) for q in trs])
        f = {k: swap.get(k, getattr(s, k)) for k in names}
        sp = {role: swap.get(role, d.tracers[role]) for role in mref.ROLES}
        water = None if no_water else C.byref(_lib.fv3_water(*[ref(sp[role]) for role in mref.ROLES], 1384.5, 4185.5, 1972.0))
        return lib.fv3_remap_moist(ctx, len(trs) if n_tracers is None else n_tracers, None if null_list else arr, *[ref(f[k]) for k in names], d.ps.fref, d.acoustic_dynamics._wsd.fref, water, 1, stream)

    trs = list(d.tracers.values())
    cases = [
        ("null water", dict(no_water=True), b"remap_moist: the fv3_water is null"),
        ("negative n_tracers", dict(n_tracers=-1), b"remap_moist: n_tracers = -1 is negative"),
        ("null tracer list", dict(null_list=True), b"remap_moist: the tracer list is null with n_tracers = 7"),
        ("null qvapor", dict(qvapor=None), b"'qvapor': null"),
        ("2-D qice", dict(qice=flat), b"'qice': vertical shape"),
        ("mis-shaped qrain", dict(qrain=short), b"'qrain': vertical shape"),
        ("qsnow is no tracer", dict(qsnow=loose), b"qsnow is not among the tracers"),
        ("qvapor is no tracer", dict(tracers=trs[1:]), b"qvapor is not among the tracers"),
        ("a tracer twice", dict(tracers=trs + [trs[2]]), b"tracers 2 and 7 are the same field"),
        ("null q_con", dict(q_con=None), b"'q_con_': null"),
        ("2-D q_con", dict(q_con=flat), b"'q_con_': vertical shape"),
        ("q_con is cappa", dict(q_con=s.cappa), b"q_con is the cappa field"),
        ("q_con is pt", dict(q_con=s.pt), b"q_con is the pt field"),
        ("q_con is delz", dict(q_con=s.delz), b"q_con is the delz field"),
        ("q_con is a tracer", dict(q_con=d.tracers["qliquid"]), b"q_con is tracer 1"),
        ("cappa is a tracer", dict(cappa=d.tracers["qgraupel"]), b"cappa is tracer 5"),
    ]
    for what, kw, word in cases:
        assert call(pt=flat) == ARG and b"'pt_': vertical shape" in lib.fv3_last_error(ctx)  # (another message in between: the one below is this case's own)
        st = call(**kw)
        msg = lib.fv3_last_error(ctx)
        assert st == ARG, (what, st)
        assert msg and word in msg, (what, msg)
        h.synchronize()
        for k, b in before.items():
            assert torch.equal(B.fields[k].storage, b), (what, k)
    args = (d.tracers, s.pt, s.delp, s.delz, s.peln, s.pe, s.pk, s.pkz, s.u, s.v, s.w, s.cappa, d.ps, d.acoustic_dynamics._wsd)
    with pytest.raises(ValueError, match="water needs q_con"):
        LagrangianToEulerian(sf)(*args, water=d.water)
    with pytest.raises(_lib.Fv3Error, match="q_con is the cappa field"):
        LagrangianToEulerian(sf)(*args, q_con=s.cappa, water=d.water)
    with pytest.raises(_lib.Fv3Error, match="qvapor is not among the tracers"):
        LagrangianToEulerian(sf)(*args, q_con=s.q_con, water=WaterSpecies(loose))
    h.synchronize()
    for k, b in before.items():
        assert torch.equal(B.fields[k].storage, b), k
    h.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. sequencing: the moist step_dynamics is the operators of fv_dynamics.py's docstring called by hand, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------------
N, NZ = 12, 8
CASE = dict(nz=NZ, layout=(1, 1), dt_atmos=225.0, k_split=2, n_split=2, n_tracers=7, hord_tr=8, remap=True, temperature=True)


@pytest.mark.parametrize("fill", [False, True], ids=["nofill", "fill"])
def test_moist_step_dynamics_is_its_operators_called_by_hand_bitwise(backend, fill):
    A = harness_for(backend)(N, moist=True, fill=fill, **CASE)
    B = harness_for(backend)(N, moist=True, fill=fill, **CASE)
    assert list(A.tracers) == list(WATER_NAMES) + ["tracer6"] and A.dycore.vapor == "qvapor" and A.dycore.water is not None and A.dycore.fill is fill
    s, tr = B.state, B.tracers
    water = WaterSpecies.from_tracers(tr, {role: role for role in mref.ROLES})
    moist_cv, to_pt, to_t, remap = MoistCV(B.sf), TemperatureToPotential(B.sf), PotentialToTemperature(B.sf), LagrangianToEulerian(B.sf, fill=fill)
    dt = 225.0 / 2
    for step in range(2):
        A.step()
        # the preamble as the two-kernel sequence: what the fused entry must equal
        moist_cv(water, s.q_con, s.cappa)
        to_pt(s.pt, s.pkz, s.delp, s.delz, s.q_con, s.cappa, tr["qvapor"])
        for k in range(2):
            B.dp1.storage.copy_(s.delp.storage)
            B.dyn(s, dt, n_map=k + 1)
            B._tracer_halo.update()
            B.tracer_advection(tr, B.dp1, s.mfxd, s.mfyd, s.cxd, s.cyd)
            remap(tr, s.pt, s.delp, s.delz, s.peln, s.pe, s.pk, s.pkz, s.u, s.v, s.w, s.cappa, B.ps, B.dyn._wsd, q_con=s.q_con, water=water)
        to_t(s.pt, s.pkz, s.delp, s.delz, s.q_con, s.cappa, s.w, s.pe, qvapor=tr["qvapor"], omga=s.omga, ps=B.ps, recompute_pkz=False)
        A.synchronize()
        B.synchronize()
        snap = _snapshot(A, A.dycore.ps)
        _assert_same(snap, _snapshot(B, B.ps), f"step {step}")
        # state.q_con / state.cappa are moist_cv of the final species
        for r in range(len(A.grids)):
            q_con, cappa = _restated(snap, r, NZ)
            assert np.array_equal(_bits(snap["q_con"][r][..., :NZ]), _bits(q_con)) and np.array_equal(_bits(snap["cappa"][r][..., :NZ]), _bits(cappa))
        assert max(float(x.max()) for x in snap["q_con"]) > 0.0
        t = np.concatenate([x[..., :NZ].ravel() for x in snap["pt"]])
        assert np.isfinite(t).all() and 100.0 < t.min() and t.max() < 380.0
    A.close()
    B.close()


def test_the_moist_harness_starts_from_the_temperature_mode_temperature(backend):
    """to_temperature() runs with the init's own q_con / cappa: T at step 0 is bitwise the non-moist temperature harness's T (the restart
    state, whose specific humidity both modes read from the same array), and the species are the restart's."""
    data = np.load(FIXTURE)
    kw = dict(nz=NZ, layout=(1, 1), dt_atmos=225.0, k_split=1, n_split=2, n_tracers=6, hord_tr=8, remap=True, temperature=True, init="restart", init_data=data)
    A = harness_for(backend)(N, moist=True, **kw)
    B = harness_for(backend)(N, vapor="tracer0", **kw)
    A.synchronize()
    B.synchronize()
    cs = (slice(NH, NH + N), slice(NH, NH + N), slice(0, NZ))
    for r in range(6):
        tile = A.part.tile_index(r)
        assert np.array_equal(_bits(_compute(A.state.pt, r)), _bits(_compute(B.state.pt, r)))
        assert np.array_equal(_bits(_compute(A.state.pkz, r)), _bits(_compute(B.state.pkz, r)))
        assert np.array_equal(A.tracers["qvapor"].numpy(r)[cs], np.transpose(data["sphum"][tile], (2, 1, 0))[:, :, :NZ])
        assert np.array_equal(A.tracers["qliquid"].numpy(r)[cs], np.transpose(data["liq_wat"][tile], (2, 1, 0))[:, :, :NZ])
        for role in ("qice", "qrain", "qsnow", "qgraupel"):
            assert not A.tracers[role].numpy(r).any()
    A.close()
    B.close()


def test_moist_needs_temperature(backend):
    with pytest.raises(ValueError, match="moist=True needs temperature=True"):
        harness_for(backend)(N, moist=True, **{**CASE, "temperature": False})


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. decomposition: one sub-domain per tile against four over one moist step
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", [False, True], ids=["nofill", "fill"])
def test_the_moist_step_does_not_depend_on_the_decomposition(backend, fill):
    n = 24
    runs = {}
    for layout in ((1, 1), (2, 2)):
        h = harness_for(backend)(n, moist=True, fill=fill, init="baroclinic", **{**CASE, "layout": layout, "n_tracers": 6})
        # the moist baroclinic wave has vapour only: give every condensate species a share of it (the same arithmetic in every cell)
        for share, role in zip((0.02, 0.004, 0.01, 0.003, 0.002), CONDENSATE):
            h.tracers[role].storage.copy_(h.tracers["qvapor"].storage * share)
        h.step()
        h.synchronize()
        runs[layout] = (h, _snapshot(h, h.dycore.ps))
    h1, one = runs[(1, 1)]
    h4, four = runs[(2, 2)]
    for r in range(len(h4.grids)):
        tile, (ox, oy) = h4.part.tile_index(r), h4.part.origin(r)
        for name in ("q_con", "cappa", "pt", "pkz") + mref.ROLES:
            a = four[name][r]
            want = one[name][tile][ox : ox + a.shape[0], oy : oy + a.shape[1]]
            assert np.array_equal(_bits(a), _bits(want)), (name, r, float(np.abs(a - want).max()))
    assert max(float(x.max()) for x in one["q_con"]) > 1.0e-5 and 100.0 < min(x[..., :NZ].min() for x in one["pt"]) and max(x[..., :NZ].max() for x in one["pt"]) < 380.0
    h1.close()
    h4.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. the default paths do not notice that the moist ones exist
# ---------------------------------------------------------------------------------------------------------------------------------
# the default step in a process of its own, where no moist object has ever existed: the compute domains of every state field, the
# tracers and ps after one step, written to the npz file named on the command line
FRESH_PROCESS = """
import sys
import numpy as np
from pace_amd._testing import harness_for
from pace_amd.dyn_core import STATE_NAMES
backend, path, n, kw = sys.argv[1], sys.argv[2], int(sys.argv[3]), eval(sys.argv[4])
h = harness_for(backend)(n, vapor="tracer0", **kw)
h.step()
h.synchronize()
fields = {k: getattr(h.state, k) for k in STATE_NAMES}
fields.update(h.tracers)
fields["ps"] = h.dycore.ps
np.savez(path, **{f"{k}:{r}": q.sub(r).view[...].detach().cpu().numpy() for k, q in fields.items() for r in range(len(h.grids))})
h.close()
"""


def test_default_paths_are_bitwise_what_they_were_after_a_moist_object_was_built(backend, tmp_path):
    import subprocess
    import sys

    from pace_amd.fv_dynamics import DynamicalCore

    kw = dict(fill=True, **{**CASE, "n_tracers": 6})
    path = str(tmp_path / "fresh.npz")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT] + [p for p in os.environ.get("PYTHONPATH", "").split(os.pathsep) if p]))
    subprocess.run([sys.executable, "-c", FRESH_PROCESS, backend, path, str(N), repr(kw)], check=True, env=env, cwd=ROOT)
    data = np.load(path)

    def default_run(through_core):
        h = harness_for(backend)(N, vapor="tracer0", **kw)
        assert h.moist is False and h.dycore.water is None and list(h.tracers)[0] == "tracer0"
        if through_core:  # a DynamicalCore of one's own, without water_species, on the harness's state
            core = DynamicalCore(h.layout, h.grids, h.sf, None, None, h.cfg, 225.0, h.state.phis, h.state, tracers=h.tracers, hord_tr=8, vapor="tracer0", cubed_to_latlon=False)
            assert core.water is None
            core.step_dynamics(h.state)
            ps = core.ps
        else:
            h.step()
            ps = h.dycore.ps
        h.synchronize()
        out = _snapshot(h, ps)
        h.close()
        return out

    first = default_run(False)
    fresh = {k: [data[f"{k}:{r}"] for r in range(len(v))] for k, v in first.items()}
    _assert_same(fresh, first, "a process without a moist object")
    m = harness_for(backend)(N, moist=True, **kw)
    m.step()
    m.synchronize()
    m.close()
    _assert_same(first, default_run(False), "harness")
    _assert_same(first, default_run(True), "DynamicalCore")


# ---------------------------------------------------------------------------------------------------------------------------------
# 9. driver
# ---------------------------------------------------------------------------------------------------------------------------------
def _yaml(tmp_path, name="c.yaml", store=None, **dycore):
    """examples/c48_dycore_only.yaml at a reduced size (C12, two sub-steps), with a diagnostics block that lists all six species"""
    y = yaml.safe_load(open(os.path.join(ROOT, "examples", "c48_dycore_only.yaml")))
    y.update(nx_tile=12, seconds=450)
    y["dycore_config"].update(n_split=2, **dycore)
    for k, v in list(y["dycore_config"].items()):
        if v is None:
            del y["dycore_config"][k]
    y["performance_config"] = {"experiment_name": "c12_moist"}
    if store is not None:
        y["output_frequency"] = 1
        y["diagnostics_config"] = {"path": str(store), "output_format": "zarr", "names": ["pt", "delp", "q_con", "cappa"] + list(WATER_NAMES)}
    p = tmp_path / name
    p.write_text(yaml.safe_dump(y))
    return str(p)


def test_driver_moist_refusals_are_one_sentence(tmp_path):
    for argv, word in (([_yaml(tmp_path), "--moist", "--remap"], "--moist needs --temperature --remap"),
                       ([_yaml(tmp_path), "--moist", "--temperature"], "--temperature needs --remap"),
                       ([_yaml(tmp_path, "n3.yaml", nwat=3), "--moist", "--temperature", "--remap"], "--moist needs dycore_config.nwat: 6 in the yaml (it has nwat: 3)"),
                       ([_yaml(tmp_path, "n0.yaml", nwat=None), "--moist", "--temperature", "--remap"], "--moist needs dycore_config.nwat: 6 in the yaml (it has nwat: None)")):
        with pytest.raises(SystemExit) as e:
            driver.main(argv)
        msg = str(e.value)
        assert word in msg and msg.count(". ") == 0, msg


@pytest.mark.gpu
def test_driver_moist_run_and_restart_round_trip(tmp_path, gpu_backend, capsys):
    store, out = tmp_path / "store", tmp_path / "perf.json"
    p = _yaml(tmp_path, store=store)
    common = ["--moist", "--temperature", "--remap", "--fill", "on"]
    r1 = str(tmp_path / "restart_1")
    assert driver.main([p, "--steps", "1", "--out", str(out), "--save-restart", r1] + common) == 0
    said = capsys.readouterr().out
    assert '"thermodynamics": "moist_cv"' in said and "advection of 6 tracers" in said
    assert "does not hold" not in said  # no species name is dropped from the diagnostics block
    assert "keys not read" not in said  # nwat, the yaml's only key outside AcousticDynamicsConfig, is read by --moist
    d = json.load(open(out))
    assert d["setup"]["thermodynamics"] == "moist_cv" and d["setup"]["tracers"] == 6 and d["setup"]["pt"] == "temperature" and d["setup"]["finite"]
    assert set(WATER_NAMES) | {"pt", "q_con", "cappa"} <= set(zr.names(str(store)))
    sp = {role: zr.read(str(store), role)[-1] for role in mref.ROLES}
    q_con, cappa, _ = mref.moist_cv(**sp)
    assert np.array_equal(_bits(zr.read(str(store), "q_con")[-1]), _bits(q_con)) and np.array_equal(_bits(zr.read(str(store), "cappa")[-1]), _bits(cappa))
    assert sp["qvapor"].max() > 1.0e-3 and 100.0 <= zr.read(str(store), "pt").min()
    # two steps in one run against one step, a restart, one more step: the same files, bit for bit
    p2 = _yaml(tmp_path, "nodiag.yaml")
    two, again = str(tmp_path / "restart_2"), str(tmp_path / "restart_1_1")
    assert driver.main([p2, "--steps", "2", "--out", str(out), "--save-restart", two] + common) == 0
    assert driver.main([p2, "--steps", "1", "--out", str(out), "--restart", r1, "--save-restart", again] + common) == 0
    from scipy.io import netcdf_file

    for rank in range(6):
        with netcdf_file(os.path.join(two, f"restart_dycore_state_{rank}.nc"), "r", mmap=False) as a, netcdf_file(os.path.join(again, f"restart_dycore_state_{rank}.nc"), "r", mmap=False) as b:
            assert set(WATER_NAMES) <= set(a.variables) and set(a.variables) == set(b.variables)
            for name in a.variables:
                x, y = np.array(a.variables[name][:]), np.array(b.variables[name][:])
                if x.dtype.kind != "f":
                    continue
                assert np.array_equal(x, y, equal_nan=True), (rank, name)
    # without --moist the driver says so and keeps dropping the species
    sub = tmp_path / "default"
    sub.mkdir()
    assert driver.main([_yaml(sub, store=sub / "store"), "--steps", "1", "--tracers", "2", "--remap", "--temperature", "--out", str(sub / "perf.json")]) == 0
    said = capsys.readouterr().out
    assert '"thermodynamics": "given"' in said and "does not hold qvapor" in said
    assert "keys not read by the acoustic path: nwat" in said  # ... and nwat stays on the list of keys nobody read
    assert json.load(open(sub / "perf.json"))["setup"]["thermodynamics"] == "given"
