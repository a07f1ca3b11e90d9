"""``AcousticDynamics`` -- the n_split acoustic loop of the FV3 dynamical core on MI355X.

Drop-in for ``pyFV3.stencils.dyn_core.AcousticDynamics`` as reached from
``Driver._critical_path_step_all -> DynamicalCore.step_dynamics`` [REF driver/pace/driver/driver.py:641];
sequencing per SURVEY §3.3 (checkpoint names C_SW-In/Out, D_SW-In/Out
[REF tests/savepoint/thresholds/fv_dynamics.yaml:2,39,76,125]).  The constructor takes the
reference's objects (comm, grid_data, stencil_factory, quantity_factory, damping_coefficients,
..., config, phis, state) where ``stencil_factory`` is this build's :class:`StencilFactory`.

MI355X-first: all sub-domains of the process are one batched set of launches; halo updates of
co-resident sub-domains are device gathers on the compute stream, cross-process ones are packed
RCCL point-to-point messages (``pace_amd.halo``).
"""
from __future__ import annotations

import os

from typing import Dict, List, Optional

import numpy as np
import torch

from . import stencils as st
from .config import AcousticDynamicsConfig
from .constants import X_DIM, X_INTERFACE_DIM, Y_DIM, Y_INTERFACE_DIM, Z_DIM, Z_INTERFACE_DIM
from .context import StencilFactory
from .halo import HaloExchanger, Layout
from .quantity import Quantity

_DIMS = {
    "u": (X_DIM, Y_INTERFACE_DIM, Z_DIM),
    "v": (X_INTERFACE_DIM, Y_DIM, Z_DIM),
    "uc": (X_INTERFACE_DIM, Y_DIM, Z_DIM),
    "vc": (X_DIM, Y_INTERFACE_DIM, Z_DIM),
    "mfxd": (X_INTERFACE_DIM, Y_DIM, Z_DIM),
    "mfyd": (X_DIM, Y_INTERFACE_DIM, Z_DIM),
    "cxd": (X_INTERFACE_DIM, Y_DIM, Z_DIM),
    "cyd": (X_DIM, Y_INTERFACE_DIM, Z_DIM),
    "pe": (X_DIM, Y_DIM, Z_INTERFACE_DIM),
    "pk": (X_DIM, Y_DIM, Z_INTERFACE_DIM),
    "peln": (X_DIM, Y_DIM, Z_INTERFACE_DIM),
}
STATE_NAMES = "u v w ua va uc vc delp delz pt pe pk peln pkz q_con omga cappa mfxd mfyd cxd cyd diss_estd".split()


def _alt(name: str) -> bool:
    """Is ``name`` among the comma-separated alternatives of FV3_ALT?  (read per call, as the library's fv3_alt and fv3_oracle/util.py: alt do)"""
    return name in [x.strip() for x in os.environ.get("FV3_ALT", "").split(",")]


class DycoreState:
    """The fields of ``pyFV3.DycoreState`` the acoustic path touches
    [REF tests/main/fv3core/test_init_from_geos.py:128-199; driver/pace/driver/state.py:131-139]."""

    def __init__(self, quantity_factory):
        self.quantity_factory = quantity_factory
        for n in STATE_NAMES:
            setattr(self, n, quantity_factory.zeros(_DIMS.get(n, (X_DIM, Y_DIM, Z_DIM))))
        self.phis = quantity_factory.zeros((X_DIM, Y_DIM), "m^2 s^-2")

    @classmethod
    def init_zeros(cls, quantity_factory):
        return cls(quantity_factory)

    @classmethod
    def from_arrays(cls, quantity_factory, per_rank: List[Dict[str, np.ndarray]]):
        """``per_rank[r][name]`` are (i, j, k) host arrays (e.g. from ``pace_amd.init.synthetic_state``)."""
        s = cls(quantity_factory)
        for n in STATE_NAMES + ["phis"]:
            q = getattr(s, n)
            for r, d in enumerate(per_rank):
                q.set_numpy(d[n], r)
        return s

    def to_arrays(self, names=None) -> List[Dict[str, np.ndarray]]:
        names = names or (STATE_NAMES + ["phis"])
        n_sub = self.u.n_sub
        return [{n: getattr(self, n).numpy(r) for n in names} for r in range(n_sub)]


class AcousticDynamics:
    def __init__(
        self,
        comm,
        grid_data,
        stencil_factory: StencilFactory,
        quantity_factory=None,
        damping_coefficients=None,
        grid_type: int = 0,
        nested: bool = False,
        stretched_grid: Optional[bool] = None,
        config: Optional[AcousticDynamicsConfig] = None,
        phis: Optional[Quantity] = None,
        wsd: Optional[Quantity] = None,
        state: Optional[DycoreState] = None,
        checkpointer=None,
    ):
        """``comm``: a :class:`pace_amd.halo.Layout` (which ranks live here) or None for "all ranks local"."""
        self.sf = stencil_factory
        self.qf = quantity_factory or stencil_factory.quantity_factory
        self.config = (config or stencil_factory.config).validate()
        # (None: the config's flag; either way it has to be the form the context's divergence damping table was made in)
        st.check_stretched_grid("AcousticDynamics", self.config.stretched_grid if stretched_grid is None else stretched_grid, stencil_factory)
        self.checkpointer = checkpointer
        self.native = True  # sequence the call with fv3_acoustic_step (C) rather than the Python twin below
        self.grid_data = grid_data
        c = stencil_factory.constants
        self.c = c
        g0 = stencil_factory.grids[0]
        self._ptop = g0.ptop
        self._akap = c.KAPPA
        self._da_min = g0.da_min
        self._dp_ref = g0.dp_ref
        self._pfull = g0.pfull
        qf = self.qf
        cell = (X_DIM, Y_DIM, Z_DIM)
        iface = (X_DIM, Y_DIM, Z_INTERFACE_DIM)
        self._gz = qf.zeros(iface, "m^2 s^-2")
        self._zh = qf.zeros(iface, "m")
        self._pkc = qf.zeros(iface)
        self._pk3 = qf.zeros(iface)
        self._crx = qf.zeros(_DIMS["cxd"])
        self._cry = qf.zeros(_DIMS["cyd"])
        self._xfx = qf.zeros(_DIMS["cxd"])
        self._yfx = qf.zeros(_DIMS["cyd"])
        self._divgd = qf.zeros((X_INTERFACE_DIM, Y_INTERFACE_DIM, Z_DIM))
        self._ut = qf.zeros(cell)
        self._vt = qf.zeros(cell)
        self._vt_scratch = qf.zeros(cell)
        self._heat_source = qf.zeros(cell)
        self._ws3 = qf.zeros((X_DIM, Y_DIM))
        self._wsd = wsd if wsd is not None else qf.zeros((X_DIM, Y_DIM))
        self._zs = qf.zeros((X_DIM, Y_DIM), "m")
        self._phis = phis
        # operators (same objects the reference builds in AcousticDynamics.__init__)
        sf = stencil_factory
        self.cgrid_shallow_water_lagrangian_dynamics = st.CGridShallowWaterDynamics(sf, qf, grid_data)
        self.update_geopotential_height_on_c_grid = st.UpdateGeopotentialHeightOnCGrid(sf, qf, grid_data)
        self.vertical_solver_cgrid = st.RiemannSolverC(sf, qf, grid_data)
        self._p_grad_c = st.PGradC(sf, qf, grid_data)
        self.dgrid_shallow_water_lagrangian_dynamics = st.DGridShallowWaterLagrangianDynamics(sf, qf, grid_data, damping_coefficients)
        self.update_height_on_d_grid = st.UpdateHeightOnDGrid(sf, qf, grid_data)
        self.vertical_solver = st.RiemannSolver3(sf, qf, grid_data)
        self._pk3_halo = st.PK3Halo(sf, qf, grid_data)
        self._edge_pe = st.EdgePE(sf, qf, grid_data)
        self.nonhydrostatic_pressure_gradient = st.NonHydrostaticPressureGradient(sf, qf, grid_data)
        self._rayleigh_damping = st.RayleighDamping(sf, qf, grid_data)
        self._hyperdiffusion = st.HyperdiffusionDamping(sf, qf, damping_coefficients, nmax=min(3, self.config.nord + 1))
        self._apply_diffusive_heating = st.ApplyDiffusiveHeating(sf, qf, grid_data)
        # halo updaters
        if comm is None:
            from .topology import CubedSpherePartitioner

            comm = Layout(CubedSpherePartitioner(self.config.npx - 1, tuple(self.config.layout)), 1, 0)
        self.layout = comm
        if len(comm.local_ranks) != sf.sizer.n_sub:
            raise ValueError("stencil factory holds a different number of sub-domains than the layout assigns to this process")
        self.halo = HaloExchanger.shared(sf, comm, group=getattr(comm, "group", None))
        self._updaters = None
        if phis is not None and state is not None:
            self._bind(state)

    # ------------------------------------------------------------------------------------------
    def _bind(self, state: DycoreState):
        h = self.halo
        self._updaters = {
            "q_con__cappa": h.updater("cell", [(state.q_con,), (state.cappa,)]),
            "delp__pt": h.updater("cell", [(state.delp,), (state.pt,)]),
            "u__v": h.updater("dgrid", [(state.u, state.v)]),
            "w": h.updater("cell", [(state.w,)]),
            "gz": h.updater("cell", [(self._gz,)]),
            "divgd": h.updater("corner", [(self._divgd,)]),
            "uc__vc": h.updater("cgrid", [(state.uc, state.vc)]),
            "delp__pt__q_con": h.updater("cell", [(state.delp,), (state.pt,), (state.q_con,)]),
            "zh": h.updater("cell", [(self._zh,)]),
            "pkc": h.updater("cell", [(self._pkc,)]),
            "heat_source": h.updater("cell", [(self._heat_source,)]),
            "interface_u__v": h.updater("sync_dgrid", [(state.u, state.v)], n_halo=0),
            "zs": h.updater("cell", [(self._zs,)]),
        }
        self._state_id = id(state)
        self._native_args = None
        phis = self._phis if self._phis is not None else state.phis
        self._phis = phis
        self._zs.storage.copy_(phis.storage * self.c.RGRAV)
        self._updaters["zs"].update()

    # ------------------------------------------------------------------------------------------
    def _build_native_args(self, state: DycoreState):
        """fv3_state / fv3_workspace views + the halo callback for ``fv3_acoustic_step``."""
        import ctypes as C

        from . import lib as _lib

        cs = self.cgrid_shallow_water_lagrangian_dynamics
        st = _lib.fv3_state()
        for n in _lib.STATE_FIELDS:
            q = self._phis if n == "phis" else getattr(state, n)
            setattr(st, n, q.field)
        work = dict(gz=self._gz, zh=self._zh, pkc=self._pkc, pk3=self._pk3, crx=self._crx, cry=self._cry, xfx=self._xfx, yfx=self._yfx, divgd=self._divgd,
                    ut=self._ut, vt=self._vt, delpc=cs.delpc, ptc=cs.ptc, dsw_delpc=self._vt_scratch, heat_source=self._heat_source, ws3=self._ws3,
                    wsd=self._wsd, zs=self._zs)
        ws = _lib.fv3_workspace()
        for n in _lib.WORK_FIELDS:
            setattr(ws, n, work[n].field)
        ups = [self._updaters[n] for n in _lib.HALO_UPDATES]
        errors = []

        def halo(_user, update, phase, _stream):
            try:
                if phase == 0:
                    ups[update].start(_stream)
                else:
                    ups[update].wait(_stream)
                return 0
            except Exception as e:  # never let an exception cross the C frame
                errors.append(e)
                return 1

        if self.halo.native:
            # the updaters as fv3_halo_plans registered with the context: fv3_acoustic_step runs without a callback
            plans = (C.c_void_p * len(ups))(*[u._native_plan() for u in ups])
            rc = self.sf.lib.fv3_ctx_set_halo_plans(self.sf.ctx, plans, len(ups))
            if rc != 0:
                raise _lib.Fv3Error("fv3_ctx_set_halo_plans failed: " + self.sf.lib.fv3_last_error(self.sf.ctx).decode())
            self._native_args = (st, ws, _lib.fv3_halo_fn(), errors)
        else:
            self._native_args = (st, ws, _lib.fv3_halo_fn(halo), errors)

    def _call_native(self, state: DycoreState, timestep: float, n_map: int):
        import ctypes as C

        if self._native_args is None:
            self._build_native_args(state)
        st, ws, cb, errors = self._native_args
        sf = self.sf
        rc = sf.lib.fv3_acoustic_step(sf.ctx, C.byref(st), C.byref(ws), float(timestep), int(n_map), cb, None, sf.stream_handle)
        if errors:
            e = errors.pop()
            errors.clear()
            raise e
        xe = getattr(self.halo, "_xfer_error", None)
        if xe is not None:
            self.halo._xfer_error = None
            raise xe
        if rc != 0:
            from . import lib as _lib

            raise _lib.Fv3Error(f"fv3_acoustic_step failed ({rc}): {sf.lib.fv3_last_error(sf.ctx).decode()}")

    def _checkpoint(self, name, **kw):
        if self.checkpointer is not None:
            self.checkpointer(name, **kw)

    # ------------------------------------------------------------------------------------------
    def __call__(self, state: DycoreState, timestep: float, n_map: int = 1, update_temporaries: bool = True):
        if self._updaters is None or self._state_id != id(state):
            self._bind(state)
        # product path: the C sequencer (fv3_acoustic_step).  The Python sequence below is its twin,
        # kept for checkpointed runs (per-operator savepoints) and selectable with native=False.
        if self.native and self.checkpointer is None and update_temporaries and not self.config.breed_vortex_inline:
            self._call_native(state, timestep, n_map)
            return
        cfg, up, sf = self.config, self._updaters, self.sf
        n_split = cfg.n_split
        dt = timestep / n_split
        dt2 = 0.5 * dt
        end_step = n_map == cfg.k_split
        up["q_con__cappa"].start()
        up["delp__pt"].start()
        up["u__v"].start()
        up["q_con__cappa"].wait()
        if update_temporaries:
            for q in (state.mfxd, state.mfyd, state.cxd, state.cyd):  # every call ("empty the flux capacitors")
                sf.call("zero", q.fref)
            if n_map == 1 or not _alt("heat_zero_first_call"):  # (FV3_ALT: DESIGN §2, restatement 5)
                sf.call("zero", self._heat_source.fref)
            sf.call("zero", state.diss_estd.fref)
        for it in range(n_split):
            remap_step = cfg.breed_vortex_inline or (it == n_split - 1)
            up["w"].start()
            if it == 0:
                sf.call("set_gz", self._zs.fref, state.delz.fref, self._gz.fref)
                up["gz"].start()
                up["delp__pt"].wait()
            up["u__v"].wait()
            up["w"].wait()
            self._checkpoint("C_SW-In", delpd=state.delp, ptd=state.pt, ud=state.u, vd=state.v, wd=state.w)
            delpc, ptc = self.cgrid_shallow_water_lagrangian_dynamics(
                state.delp, state.pt, state.u, state.v, state.w, state.uc, state.vc, state.ua, state.va, self._ut, self._vt, self._divgd, state.omga, dt2
            )
            # (omgad / delpcd / ptcd: beyond the reference's variable list -- the remaining c_sw outputs, for single-rank oracle spot checks)
            self._checkpoint("C_SW-Out", delpd=state.delp, ptd=state.pt, ucd=state.uc, vcd=state.vc, uad=state.ua, vad=state.va, utd=self._ut, vtd=self._vt, divgdd=self._divgd,
                             omgad=state.omga, delpcd=delpc, ptcd=ptc)
            if cfg.nord > 0:
                up["divgd"].start()
            if it == 0:
                up["gz"].wait()
                sf.call("copy", self._gz.fref, self._zh.fref)
            else:
                sf.call("copy", self._zh.fref, self._gz.fref)
            self.update_geopotential_height_on_c_grid(self._dp_ref, self._zs, self._ut, self._vt, self._gz, self._ws3, dt2)
            self.vertical_solver_cgrid(dt2, state.cappa, self._ptop, self._phis, self._ws3, ptc, state.q_con, delpc, self._gz, self._pkc, state.omga)
            self._p_grad_c(None, None, state.uc, state.vc, delpc, self._pkc, self._gz, dt2)
            up["uc__vc"].start()
            if cfg.nord > 0:
                up["divgd"].wait()
            up["uc__vc"].wait()
            # (q_cond .. heat_sourced: beyond the reference's variable list -- the remaining d_sw inputs / outputs)
            self._checkpoint("D_SW-In", ucd=state.uc, vcd=state.vc, wd=state.w, delpcd=self._vt_scratch, delpd=state.delp, ud=state.u, vd=state.v, ptd=state.pt, uad=state.ua, vad=state.va, zhd=self._zh, divgdd=self._divgd,
                             q_cond=state.q_con, mfxd=state.mfxd, mfyd=state.mfyd, cxd=state.cxd, cyd=state.cyd, heat_sourced=self._heat_source)
            self.dgrid_shallow_water_lagrangian_dynamics(
                self._vt_scratch, state.delp, state.pt, state.u, state.v, state.w, state.uc, state.vc, state.ua, state.va, self._divgd,
                state.mfxd, state.mfyd, state.cxd, state.cyd, self._crx, self._cry, self._xfx, self._yfx, state.q_con, self._zh,
                self._heat_source, state.diss_estd, dt,
            )  # fmt: skip
            self._checkpoint("D_SW-Out", ucd=state.uc, vcd=state.vc, wd=state.w, delpcd=self._vt_scratch, delpd=state.delp, ud=state.u, vd=state.v, ptd=state.pt, uad=state.ua, vad=state.va, divgdd=self._divgd, mfxd=state.mfxd, mfyd=state.mfyd, xfxd=self._xfx, yfxd=self._yfx,
                             q_cond=state.q_con, cxd=state.cxd, cyd=state.cyd, crxd=self._crx, cryd=self._cry, heat_sourced=self._heat_source)
            up["delp__pt__q_con"].update()
            self.update_height_on_d_grid(self._zs, self._zh, self._crx, self._cry, self._xfx, self._yfx, self._wsd, dt)
            self.vertical_solver(remap_step, dt, state.cappa, self._ptop, self._zs, self._wsd, state.delz, state.q_con, state.delp, state.pt, self._zh, state.pe, self._pkc, self._pk3, state.pk, state.peln, state.w)
            up["zh"].start()
            up["pkc"].start()
            if remap_step:
                self._edge_pe(state.pe, state.delp, self._ptop)
            self._pk3_halo(self._pk3, state.delp, self._ptop, self._akap)
            up["zh"].wait()
            sf.call("compute_geopotential", self._zh.fref, self._gz.fref)
            up["pkc"].wait()
            self.nonhydrostatic_pressure_gradient(state.u, state.v, self._pkc, self._gz, self._pk3, state.delp, dt, self._ptop, self._akap)
            if cfg.rf_fast:
                self._rayleigh_damping(state.u, state.v, state.w, self._dp_ref, self._pfull, dt, self._ptop)
            if it != n_split - 1:
                up["u__v"].start()
            else:
                up["interface_u__v"].update()
        if cfg.d_con > 1.0e-5:
            up["heat_source"].update()
            cd = self.c.CNST_0P20 * self._da_min
            self._hyperdiffusion(self._heat_source, cd)
            heat_dt = timestep if _alt("heat_dt_full") else dt  # (FV3_ALT: fv3_oracle/util.py)
            self._apply_diffusive_heating(state.delp, state.delz, state.cappa, self._heat_source, state.pt, abs(heat_dt * cfg.delt_max))
