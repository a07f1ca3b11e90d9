"""Dycore-only harness: builds grid, synthetic state and the acoustic dynamics for the ranks
one process owns and steps them -- the slice of ``Driver._critical_path_step_all`` that reaches
the hot path with ``dycore_only: true, disable_step_physics: true``
[REF driver/pace/driver/driver.py:627-662; .jenkins/driver_configs/baroclinic_c48_6ranks_dycore_only.yaml:1-2].
One "step" = ``k_split`` calls of AcousticDynamics, timed like the reference ("mainloop" timer, first step dropped
[REF .jenkins/print_performance_number.py:13-14]).  The headline workload is the acoustic loop alone; ``n_tracers`` adds the
sub-cycled tracer advection after every acoustic call and ``remap`` the Lagrangian-to-Eulerian remap after that (SURVEY §8f-3:
together the body of ``DynamicalCore.step_dynamics``; no physics, no moist thermodynamics), ``fill`` the vertical filling of negative
tracer values at the end of the remap (the namelist's ``fill``); ``latlon_winds`` the CubedToLatLon that
ends ``fv_dynamics`` (eastward / northward ``ua``, ``va``); ``temperature`` (needs ``remap``) makes the step
``DynamicalCore.step_dynamics`` (pace_amd/fv_dynamics.py): ``state.pt`` is then a temperature in K between steps, ``omga`` and ``ps`` are
diagnosed, ``vapor`` names the tracer that is the specific humidity; ``moist`` (needs ``temperature``) names the first six tracers
after the water species and lets ``q_con`` / ``cappa`` follow them (``moist_cv`` in the preamble and in every remap); ``neg_adj``
(needs ``moist``) ends the thermodynamic part of the step with FV3's ``neg_adj3`` on the temperature and the six species.
``stretch_factor`` / ``lon_target`` / ``lat_target`` (degrees; the reference's ``grid_config.config`` keys): a factor other than 1 refines the
grid about the target with a Schmidt transform (``pace_amd.grid.SchmidtTransform``) and sets ``stretched_grid`` in the config.
``held_suarez`` (needs ``temperature``, ``remap`` and ``latlon_winds``; ``held_suarez_config``: a ``pace_amd.stencils.HeldSuarezConfig``) adds the
second half of the reference driver's step [REF driver/pace/driver/driver.py:494-530]: after ``step_dynamics`` the Held-Suarez forcing forms
``u_dt``, ``v_dt``, ``pt_dt`` from the end state and ``ApplyPhysicsToDycore`` applies them with ``dt_atmos`` (timer clocks "HeldSuarez", "ApplyPhysics").
``dry_convective_adjustment`` (needs ``temperature``, ``remap`` and ``latlon_winds``; not together with ``held_suarez``: both assign ``u_dt``, ``v_dt``) is the
reference's ``fv_sg_adj > 0``: after ``step_dynamics`` ``DryConvectiveAdjustment`` (``fv_subgrid_z`` on the top ``n_sponge`` levels, time scale
``config.fv_sg_adj``; with ``moist`` the six water species are passed, otherwise it runs dry) mixes ``pt``, ``w`` and the tracers and forms ``u_dt``, ``v_dt``,
which ``ApplyPhysicsToDycore`` applies with ``dt_atmos`` and a zero ``pt_dt`` (timer clocks "DryConvectiveAdjustment", "ApplyPhysics").
``constants`` (a ``pace_amd.constants.ConstantSet``; None: the project's): the constants the grids and the kernels are made with, e.g. ``OMEGA = 0`` for a planet that does not turn.
"""
from __future__ import annotations

import time
from typing import Optional

import numpy as np
import torch

from .config import AcousticDynamicsConfig
from .constants import get_constants
from .context import StencilFactory
from .dyn_core import STATE_NAMES, AcousticDynamics, DycoreState
from .grid import SchmidtTransform, make_grid
from .halo import Layout
from .init import synthetic_state, synthetic_state_device
from .topology import CubedSpherePartitioner

# dt_atmos / k_split / n_split per configuration
CONFIGS = {
    "c12": dict(nx_tile=12, nz=79, layout=(1, 1), dt_atmos=225.0, k_split=1, n_split=1),
    "c48": dict(nx_tile=48, nz=79, layout=(1, 1), dt_atmos=225.0, k_split=1, n_split=1),
    "c192": dict(nx_tile=192, nz=79, layout=(1, 1), dt_atmos=200.0, k_split=7, n_split=8),
    # not a reference config: 6 sub-domains of 384^2 = the per-GPU share of the C768 run on 4 GPUs (scaling studies on one GPU)
    "c384": dict(nx_tile=384, nz=79, layout=(1, 1), dt_atmos=225.0, k_split=2, n_split=6),
    # likewise 6 sub-domains of 272^2 ~ 3 of 384^2 = the per-GPU cell count of the C768 run on 8 GPUs
    "c272": dict(nx_tile=272, nz=79, layout=(1, 1), dt_atmos=225.0, k_split=2, n_split=6),
    "c768": dict(nx_tile=768, nz=79, layout=(2, 2), dt_atmos=225.0, k_split=2, n_split=6),
}


# moist=True: the names of the first six tracers (the reference's tracer order) and, for the synthetic state, each one's multiple of q_con
WATER_NAMES = ("qvapor", "qliquid", "qice", "qrain", "qsnow", "qgraupel")
SYNTHETIC_WATER = dict(qvapor=20.0, qliquid=0.5, qice=0.2, qrain=0.15, qsnow=0.1, qgraupel=0.05)


class DycoreHarness:
    def __init__(
        self,
        nx_tile: int,
        nz: int = 79,
        layout=(1, 1),
        dt_atmos: float = 225.0,
        k_split: int = 1,
        n_split: int = 1,
        world_size: int = 1,
        proc: int = 0,
        backend: str = "hip:gfx950",
        device: Optional[str] = None,
        dtype=torch.float64,
        group=None,
        seed: int = 20261002,
        noise: float = 0.01,
        verbose: bool = False,
        config_overrides: Optional[dict] = None,
        init: str = "synthetic",
        n_tracers: int = 0,
        hord_tr: int = 8,
        remap: bool = False,
        fill: bool = False,
        init_data=None,
        ak=None,
        bk=None,
        loopback: bool = False,
        latlon_winds: bool = False,
        temperature: bool = False,
        vapor: Optional[str] = None,
        moist: bool = False,
        neg_adj: bool = False,
        sat_adj: bool = False,
        sat_adjust_config=None,
        stretch_factor: float = 1.0,
        lon_target: float = 350.0,
        lat_target: float = -90.0,
        held_suarez: bool = False,
        held_suarez_config=None,
        dry_convective_adjustment: bool = False,
        constants=None,
        _testing_token=None,
    ):
        if held_suarez and not (temperature and remap and latlon_winds):
            raise ValueError("held_suarez=True needs temperature=True, remap=True and latlon_winds=True: the forcing reads the temperature and the eastward / northward winds of the step's end state")
        if dry_convective_adjustment and not (temperature and remap and latlon_winds):
            raise ValueError("dry_convective_adjustment=True needs temperature=True, remap=True and latlon_winds=True: fv_subgrid_z reads the temperature and the eastward / northward winds of the step's end state")
        if dry_convective_adjustment and held_suarez:
            raise ValueError("dry_convective_adjustment=True and held_suarez=True exclude each other: both assign the wind tendencies u_dt, v_dt that ApplyPhysicsToDycore applies")
        if fill and not remap:
            raise ValueError("fill=True needs remap=True: the vertical filling of negative tracer values is the last tracer step of the remap")
        if temperature and not remap:
            raise ValueError("temperature=True needs remap=True: the conversion back to temperature is the last step of the remap")
        if vapor is not None and not temperature:
            raise ValueError("vapor names the specific-humidity tracer of the temperature conversion: it needs temperature=True")
        if moist and not temperature:
            raise ValueError("moist=True needs temperature=True: moist_cv sits in the preamble and the remap of DynamicalCore.step_dynamics")
        if neg_adj and not moist:
            raise ValueError("neg_adj=True needs moist=True: neg_adj3 works on the six water species of the moist step")
        if sat_adj and not moist:
            raise ValueError("sat_adj=True needs moist=True: the saturation adjustment works on the six water species of the moist step")
        self.neg_adj = bool(neg_adj)
        self.sat_adj, self.sat_adjust_config = bool(sat_adj), sat_adjust_config
        if moist:
            if vapor not in (None, "qvapor"):
                raise ValueError(f"moist=True: the specific humidity is the species qvapor (vapor={vapor!r})")
            vapor = "qvapor"
            n_tracers = max(int(n_tracers), len(WATER_NAMES))
        self.moist = bool(moist)
        self.c = constants or get_constants()  # (constants: another ConstantSet for the grids and the kernels, e.g. a planet that does not turn)
        self.part = CubedSpherePartitioner(nx_tile, tuple(layout))
        # a stretch factor other than 1 gives the Schmidt-transformed grid AND the stretched form of the divergence damping
        # (the two are separate inputs below this class: make_grid's stretch, the config's stretched_grid)
        stretch = SchmidtTransform(float(stretch_factor), float(lon_target), float(lat_target))
        self.stretch = stretch if stretch.active else None
        self.cfg = AcousticDynamicsConfig(npx=nx_tile + 1, npy=nx_tile + 1, npz=nz, layout=tuple(layout), dt_atmos=dt_atmos, k_split=k_split, n_split=n_split,
                                          **{**(config_overrides or {}), "fill": bool(fill), **({"stretched_grid": True} if self.stretch else {})})
        self.layout = Layout(self.part, world_size, proc)
        self.layout.group = group
        self.layout.loopback = bool(loopback)  # this process plays `proc` of `world_size` alone, its messages looped back (timing runs)
        t0 = time.time()
        self.grids = [make_grid(self.part, r, nz=nz, ak=ak, bk=bk, stretch=self.stretch, constants=self.c) for r in self.layout.local_ranks]
        if verbose:
            print(f"[harness] grid for ranks {self.layout.local_ranks} in {time.time() - t0:.1f}s", flush=True)
        self.sf = StencilFactory(self.grids, self.cfg, self.c, backend=backend, device=device, dtype=dtype, _testing_token=_testing_token)
        self.state = DycoreState(self.sf.quantity_factory)
        t0 = time.time()
        on_device = not self.sf.hostemu
        if init not in ("synthetic", "baroclinic", "restart"):
            raise ValueError(f"init {init!r}: 'synthetic' (SURVEY §8d recipe), 'baroclinic' (JW2006 wave) or 'restart' (init_data = the six-tile FV3 restart arrays)")
        for i, (g, r) in enumerate(zip(self.grids, self.layout.local_ranks)):
            if init == "baroclinic":
                from .init import baroclinic_state

                s = baroclinic_state(g, self.c)
                for n in STATE_NAMES + ["phis"]:
                    getattr(self.state, n).set_numpy(s[n], i)
            elif init == "restart":
                from .init import restart_state

                s = restart_state(g, init_data, self.part.tile_index(r), self.part.origin(r), self.c)
                for n in STATE_NAMES + ["phis"]:
                    getattr(self.state, n).set_numpy(s[n], i)
            elif on_device:
                # evaluate the recipe with torch on the GPU (numpy needs ~1 min per 384^2 x 79 rank)
                s = synthetic_state_device(g, self.sf.device, seed=seed, rank=r, noise=noise)
                for n in STATE_NAMES + ["phis"]:
                    q = getattr(self.state, n)
                    src = s[n]
                    q.storage[i].copy_((src.permute(1, 0) if src.dim() == 2 else src.permute(2, 1, 0)).to(q.storage.dtype))
            else:
                s = synthetic_state(g, seed=seed, rank=r, noise=noise)
                for n in STATE_NAMES + ["phis"]:
                    getattr(self.state, n).set_numpy(s[n], i)
            del s
        if verbose:
            print(f"[harness] {init} state in {time.time() - t0:.1f}s", flush=True)
        self.tracers = {}
        self.temperature = bool(temperature)
        self.dycore = None
        self.cells_local = self.part.nx * self.part.ny * nz * len(self.grids)
        self.cells_global = nx_tile * nx_tile * 6 * nz
        if temperature:
            self._make_tracers(n_tracers)
            if moist:
                self._init_water_species(init, init_data)
            elif vapor is not None and init == "restart":  # the specific humidity the restart's T_v was formed with
                self._load_restart_tracer(vapor, init_data, "sphum")
            self._init_temperature(vapor, hord_tr, latlon_winds)
            self._init_held_suarez(held_suarez, held_suarez_config)
            self._init_dry_adjust(dry_convective_adjustment)
            return
        self.held_suarez = self.apply_physics = self.dry_adjust = None
        self.dyn =AcousticDynamics(self.layout, self.grids, self.sf, config=self.cfg, phis=self.state.phis, state=self.state)
        # shared D-grid interface winds must be single-valued across sub-domains (they are in any
        # physical state; the per-rank white noise of the synthetic recipe breaks it)
        if not loopback:
            self.dyn._updaters["interface_u__v"].update()
        # tracers advected after every acoustic call with the mass fluxes / Courant numbers it accumulated
        if n_tracers:
            from .stencils import FiniteVolumeTransport, TracerAdvection

            qf = self.sf.quantity_factory
            self._make_tracers(n_tracers)
            self.dp1 = qf.zeros(("x", "y", "z"), "Pa")
            self.tracer_advection = TracerAdvection(self.sf, qf, FiniteVolumeTransport(self.sf, qf, self.grids, hord=hord_tr), self.grids, self.layout, self.tracers)
            self._tracer_halo = self.dyn.halo.updater("cell", [(q,) for q in self.tracers.values()])
        self.remap = None
        if remap:
            from .stencils import LagrangianToEulerian

            self.remap = LagrangianToEulerian(self.sf, self.sf.quantity_factory, self.grids, fill=fill)
            self.ps = self.sf.quantity_factory.zeros(("x", "y"), "Pa")
        # CubedToLatLon once per step, after the k_split loop (where fv_dynamics runs it): state.ua / state.va become the eastward /
        # northward cell-centre winds.  Off by default: without it ua / va keep what the last c_sw left (local A-grid components).
        self.cubed_to_latlon = None
        if latlon_winds:
            from .stencils import CubedToLatLon

            self.cubed_to_latlon = CubedToLatLon(self.sf, self.sf.quantity_factory, self.grids, order=self.cfg.c2l_ord, comm=self.layout)

    def _make_tracers(self, n_tracers):
        qf = self.sf.quantity_factory
        for t in range(n_tracers):
            q = qf.zeros(("x", "y", "z"), "kg/kg")
            q.storage.copy_(self.state.q_con.storage * (10.0 * (t + 1)) + 1.0e-3 * (t + 1))
            self.tracers[WATER_NAMES[t] if self.moist and t < len(WATER_NAMES) else f"tracer{t}"] = q

    def _init_water_species(self, init, data):
        """moist=True: the first six tracers are the water species.  ``restart``: qvapor = sphum, qliquid = liq_wat; ``baroclinic``:
        the humidity of the moist baroclinic wave (pace_amd.init.baroclinic_humidity); the other species zero.  ``synthetic``:
        fixed positive multiples of the state's q_con field (the condensate shares add up to 1)."""
        tr, s = self.tracers, self.state
        if init == "synthetic":
            for name, share in SYNTHETIC_WATER.items():
                tr[name].storage.copy_(s.q_con.storage * share)
            return
        for name in WATER_NAMES:
            tr[name].storage.zero_()
        if init == "restart":
            self._load_restart_tracer("qvapor", data, "sphum")
            self._load_restart_tracer("qliquid", data, "liq_wat")
            return
        from .init import baroclinic_humidity

        nz = self.cfg.npz
        for i, g in enumerate(self.grids):
            delp, peln = s.delp.numpy(i).astype(np.float64), s.peln.numpy(i).astype(np.float64)
            q = np.zeros(delp.shape)
            q[:, :, :nz] = baroclinic_humidity(g.lat_agrid, delp[:, :, :nz], peln[:, :, : nz + 1])
            tr["qvapor"].set_numpy(q, i)

    def _load_restart_tracer(self, name, data, key):
        """Tracer ``name`` from the six-tile restart arrays (``data[key][tile][k, y, x]``), placed like the state's cell fields
        (``pace_amd.init.restart_state``: the compute cells, everything else edge-replicated)."""
        if name not in self.tracers:
            raise ValueError(f"vapor={name!r} is not among the tracers ({', '.join(self.tracers) or 'none'})")
        nh, nx, ny, nz = self.grids[0].n_halo, self.part.nx, self.part.ny, self.cfg.npz
        for i, r in enumerate(self.layout.local_ranks):
            ox, oy = self.part.origin(r)
            a = np.transpose(np.asarray(data[key][self.part.tile_index(r)], dtype=np.float64), (2, 1, 0))[ox : ox + nx, oy : oy + ny, :nz]
            self.tracers[name].set_numpy(np.pad(a, ((nh, nh + 1), (nh, nh + 1), (0, 1)), mode="edge"), i)

    def _init_temperature(self, vapor, hord_tr, latlon_winds):
        """temperature=True: the step is ``DynamicalCore.step_dynamics`` over the harness's own state and tracers, and the state
        holds T between steps.  The core owns the operators and buffers the default harness builds itself; they are reachable
        under the same names (``dyn``, ``remap``, ``ps``, ...)."""
        from .fv_dynamics import DynamicalCore

        self.dycore = DynamicalCore(self.layout, self.grids, self.sf, self.sf.quantity_factory, None, self.cfg, self.cfg.dt_atmos, self.state.phis, self.state,
                                    tracers=self.tracers, hord_tr=hord_tr, vapor=vapor, cubed_to_latlon=latlon_winds,
                                    water_species={n: n for n in WATER_NAMES} if self.moist else None, adjust_negative_water=self.neg_adj,
                                    saturation_adjustment=self.sat_adj, sat_adjust_config=self.sat_adjust_config)
        d = self.dycore
        self.dyn = d.acoustic_dynamics
        if not self.layout.loopback:
            self.dyn._updaters["interface_u__v"].update()
        self.remap, self.ps, self.cubed_to_latlon = d.remap, d.ps, d.cubed_to_latlon
        if self.tracers:
            self.dp1, self.tracer_advection, self._tracer_halo = d.dp1, d.tracer_advection, d._tracer_halo
        self.to_temperature()

    def _init_held_suarez(self, held_suarez, config):
        """held_suarez=True: the step ends with the Held-Suarez forcing (tendencies from the end state's ``ua``, ``va``, ``pt``, ``delp``) and
        ``ApplyPhysicsToDycore`` with ``dt_atmos``; the operators and the three tendency buffers are made here."""
        self.held_suarez = self.apply_physics = None
        if not held_suarez:
            return
        from .stencils import ApplyPhysicsToDycore, HeldSuarezForcing

        qf = self.sf.quantity_factory
        self.held_suarez = HeldSuarezForcing(self.sf, qf, self.grids, config=config)
        self.apply_physics = ApplyPhysicsToDycore(self.sf, qf, self.grids, comm=self.layout)
        self.u_dt, self.v_dt, self.pt_dt = qf.zeros(("x", "y", "z"), "m/s**2"), qf.zeros(("x", "y", "z"), "m/s**2"), qf.zeros(("x", "y", "z"), "K/s")

    def _init_dry_adjust(self, on):
        """dry_convective_adjustment=True: the step ends with ``DryConvectiveAdjustment`` on the end state and ``ApplyPhysicsToDycore`` with
        ``dt_atmos``; the operators, the work fields and the three tendency buffers (``pt_dt`` stays zero) are made here."""
        self.dry_adjust = None
        if not on:
            return
        from .stencils import ApplyPhysicsToDycore, DryConvectiveAdjustment

        qf = self.sf.quantity_factory
        self.dry_adjust = DryConvectiveAdjustment(self.sf, qf, self.grids, n_sponge=self.cfg.n_sponge, fv_sg_adj=self.cfg.fv_sg_adj,
                                                  water_species=self.dycore.water if self.moist else None, tracers=self.tracers)
        self.apply_physics = ApplyPhysicsToDycore(self.sf, qf, self.grids, comm=self.layout)
        self.u_dt, self.v_dt, self.pt_dt = qf.zeros(("x", "y", "z"), "m/s**2"), qf.zeros(("x", "y", "z"), "m/s**2"), qf.zeros(("x", "y", "z"), "K/s")

    def to_temperature(self):
        """The state's ``pt`` from the loop's form ``T_v / pkz`` (what every ``init`` and a default-mode restart file hold) to the
        temperature in K, ``pkz`` rebuilt from the state, ``ps`` from ``pe``; ``omga`` is not touched.  It reads the state's own
        ``q_con`` / ``cappa`` (also with ``moist``: the species define them from the first preamble on)."""
        s, d = self.state, self.dycore
        d.potential_to_temperature(s.pt, s.pkz, s.delp, s.delz, s.q_con, s.cappa, s.w, s.pe, qvapor=d.qvapor, ps=d.ps, recompute_pkz=True)

    def step(self, timer=None):
        """One model step of the dycore-only driver: k_split acoustic-dynamics calls (each followed by tracer advection and the
        vertical remap where the harness was built with them), then -- with ``latlon_winds`` -- CubedToLatLon once.  ``timer`` (pace_amd.timer.Timer): the reference's timer names inside
        ``DynamicalCore.step_dynamics`` -- "DynCore" around the acoustic dynamics, "TracerAdvection", "Remapping"
        [REF tests/main/driver/test_driver.py:77-121]."""
        from .timer import NullTimer

        timer = timer or NullTimer()
        if self.dycore is not None:  # temperature=True: pt is a temperature before and after the step
            self.dycore.step_dynamics(self.state, timer)
            if self.held_suarez is not None:  # the second half of the reference driver's step: tendencies, then their application
                s = self.state
                with timer.clock("HeldSuarez"):
                    self.held_suarez(s.ua, s.va, s.pt, s.delp, self.u_dt, self.v_dt, self.pt_dt, self.cfg.dt_atmos)
                with timer.clock("ApplyPhysics"):
                    self.apply_physics(s, self.u_dt, self.v_dt, self.pt_dt, self.cfg.dt_atmos)
            if self.dry_adjust is not None:  # the reference's fv_sg_adj > 0: DycoreToPhysics runs fv_subgrid_z, ApplyPhysicsToDycore its wind tendencies
                s = self.state
                with timer.clock("DryConvectiveAdjustment"):
                    self.dry_adjust(s, self.u_dt, self.v_dt, self.cfg.dt_atmos)
                with timer.clock("ApplyPhysics"):
                    self.apply_physics(s, self.u_dt, self.v_dt, self.pt_dt, self.cfg.dt_atmos)
            return
        dt = self.cfg.dt_atmos / self.cfg.k_split
        for k in range(self.cfg.k_split):
            if self.tracers:
                self.dp1.storage.copy_(self.state.delp.storage)  # the air mass the accumulated mass fluxes start from
            with timer.clock("DynCore"):
                self.dyn(self.state, dt, n_map=k + 1)
            if self.tracers:
                with timer.clock("TracerAdvection"):
                    self._tracer_halo.update()
                    self.tracer_advection(self.tracers, self.dp1, self.state.mfxd, self.state.mfyd, self.state.cxd, self.state.cyd)
            if self.remap is not None:
                s = self.state
                with timer.clock("Remapping"):
                    self.remap(self.tracers, s.pt, s.delp, s.delz, s.peln, s.pe, s.pk, s.pkz, s.u, s.v, s.w, s.cappa, self.ps, self.dyn._wsd)
        if self.cubed_to_latlon is not None:
            with timer.clock("CubedToLatLon"):
                self.cubed_to_latlon(self.state.u, self.state.v, self.state.ua, self.state.va)

    def close(self):
        """Destroy the library context now (scratch, streams, the RCCL communicator) instead of at garbage collection -- the end of a
        multi-process run, while the process group still exists."""
        self.sf.close()

    def synchronize(self):
        if not self.sf.hostemu:
            torch.cuda.synchronize(self.sf.device)

    def checksum_parts(self):
        """Per-sub-domain float64 sums of the prognostic fields (local sub-domains, in rank order)."""
        out = {}
        for n in ("delp", "pt", "u", "v", "w", "delz", "q_con"):
            q = getattr(self.state, n)
            out[n] = [float(q.sub(i).view[...][..., : self.cfg.npz].double().sum().item()) for i in range(q.n_sub)]
        return out

    def checksum(self, gather=None):
        """Order-fixed float64 sums of the prognostic fields: the per-sub-domain sums added in global rank order, so the value is
        bitwise comparable between runs of one build whatever the number of processes (`gather`: a callable that returns the
        list of every process's `checksum_parts()` in process order; None = single process)."""
        parts = [self.checksum_parts()] if gather is None else gather(self.checksum_parts())
        out = {}
        for n in parts[0]:
            tot = 0.0
            for p in parts:
                for v in p[n]:
                    tot += v
            out[n] = tot
        return out

    def sanity(self):
        """SafetyChecker-style bounds [REF driver/pace/driver/driver.py:557-560] on the local state."""
        out = {}
        for n in ("delp", "pt", "u", "v", "w"):
            q = getattr(self.state, n)
            v = q.view[...]
            v = v[..., : self.cfg.npz]
            out[n] = (float(v.min()), float(v.max()), bool(torch.isfinite(v).all()))
        return out
