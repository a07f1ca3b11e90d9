"""``DynamicalCore`` -- the public entry of the path: ``DynamicalCore(...).step_dynamics(state, timer)``, the one call through
which the reference reaches the dynamical core [REF driver/pace/driver/driver.py:494-504, 639-644].

The contract of the call is the reference's: ``state.pt`` holds the temperature in K before and after a step.  Inside the step

1. :class:`~pace_amd.stencils.TemperatureToPotential` takes ``pt`` to the form the acoustic loop transports (``T_v / pkz``) and
   rebuilds ``pkz``,
2. ``k_split`` times: the ``dp1`` copy, :class:`~pace_amd.dyn_core.AcousticDynamics` ("DynCore"), the tracer halo update and
   :class:`~pace_amd.stencils.TracerAdvection` ("TracerAdvection"), :class:`~pace_amd.stencils.LagrangianToEulerian` with the
   vertical filling where ``config.fill`` asks for it and the saturation adjustment where ``saturation_adjustment`` does
   ("Remapping") -- the sequence of ``DycoreHarness.step``,
3. :class:`~pace_amd.stencils.PotentialToTemperature` takes ``pt`` back to K with the ``pkz`` the last remap left, diagnoses
   ``state.omga = delp / delz * w`` and the surface pressure ``DynamicalCore.ps``,
4. :class:`~pace_amd.stencils.AdjustNegativeTracerMixingRatio`, where asked (``adjust_negative_water``; "NegAdj3"): FV3's
   ``neg_adj3`` on the temperature and the six water species,
5. :class:`~pace_amd.stencils.CubedToLatLon`, where asked ("CubedToLatLon").

Without ``water_species`` ``q_con`` and ``cappa`` are fields of the state that the caller provides.  With it they are derived from
the six water species by FV3's ``moist_cv`` where FV3 derives them: step 1 becomes the moist preamble
(``fv3_pt_from_temperature_moist``: ``q_con``, ``cappa`` from the species, then the conversion) and the remap of step 2 the moist remap
(``fv3_remap_moist``: remap, fill, ``q_con`` / ``cappa`` from the remapped and filled species, ``pkz`` with the new ``cappa``); step 3 is
unchanged and reads the ``q_con`` the last remap wrote.  With ``saturation_adjustment`` every remap of step 2 is the adjusting one
(``fv3_remap_moist_sat``: FV3's ``fv_sat_adj`` between the fill and ``moist_cv``, with ``mdt = timestep / k_split`` and its second pass
to full saturation in the last remap of the step).  The energy fixer is outside this build; the physics coupling is the caller's second call after the step
(:class:`~pace_amd.stencils.ApplyPhysicsToDycore`, which ``DycoreHarness(held_suarez=True)`` runs with the Held-Suarez forcing).  Every buffer (``dp1``, ``ps``, the operators' own) is allocated by the
constructor; ``step_dynamics`` allocates nothing.
"""
from __future__ import annotations

from typing import Dict, Optional

from . import stencils as st
from .constants import X_DIM, Y_DIM, Z_DIM
from .dyn_core import AcousticDynamics, DycoreState
from .quantity import Quantity


class DynamicalCore:
    def __init__(
        self,
        comm,
        grid_data,
        stencil_factory,
        quantity_factory=None,
        damping_coefficients=None,
        config=None,
        timestep=None,
        phis: Optional[Quantity] = None,
        state: Optional[DycoreState] = None,
        checkpointer=None,
        *,
        tracers: Optional[Dict[str, Quantity]] = None,
        hord_tr: int = 8,
        vapor: Optional[str] = None,
        cubed_to_latlon: bool = True,
        water_species: Optional[Dict[str, str]] = None,
        adjust_negative_water: bool = False,
        saturation_adjustment: bool = False,
        sat_adjust_config: Optional[st.SatAdjustConfig] = None,
    ):
        """Arguments as the reference's call.  ``comm``: a :class:`pace_amd.halo.Layout` (None: every rank in this process);
        ``timestep``: the model step ``dt_atmos`` in seconds or as a ``timedelta`` (None: ``config.dt_atmos``); ``tracers``:
        ``{name: Quantity}`` advected and remapped with the step (may be empty); ``vapor``: the name of the tracer that is the
        specific humidity (None: a dry conversion between temperature and virtual temperature); ``hord_tr``: the tracers'
        transport scheme; ``cubed_to_latlon``: end the step with the eastward / northward ``ua``, ``va``; ``water_species``:
        ``{role: tracer name}`` for the roles ``qvapor``, ``qliquid``, ``qrain``, ``qice``, ``qsnow``, ``qgraupel`` (a missing role is a
        field of zeros; ``qvapor`` is required and becomes ``vapor``) -- ``q_con`` and ``cappa`` are then derived from these tracers
        (``moist_cv``) in the preamble and in every remap; None: they are the state's fields as the caller left them;
        ``adjust_negative_water``: run ``neg_adj3`` on ``state.pt`` and the species after the conversion back to temperature (FV3 does
        whenever ``nwat == 6``); it needs ``water_species`` with all six roles; ``saturation_adjustment``: run FV3's ``fv_sat_adj`` inside
        every remap (the namelist's ``do_sat_adj``; ``sat_adjust_config``: its parameters, None: FV3's defaults); it needs
        ``water_species`` with all six roles."""
        sf = stencil_factory
        qf = quantity_factory or sf.quantity_factory
        self.sf, self.qf = sf, qf
        self.config = (config or sf.config).validate()
        if timestep is None:
            timestep = self.config.dt_atmos
        self.timestep = float(timestep.total_seconds()) if hasattr(timestep, "total_seconds") else float(timestep)
        self.tracers = dict(tracers or {})
        self.water = None
        if water_species is not None:
            self.water = st.WaterSpecies.from_tracers(self.tracers, dict(water_species))
            if vapor is not None and vapor != water_species["qvapor"]:
                raise ValueError(f"vapor={vapor!r} differs from water_species['qvapor']={water_species['qvapor']!r}")
            vapor = water_species["qvapor"]
        if vapor is not None and vapor not in self.tracers:
            raise ValueError(f"vapor={vapor!r} is not among the tracers ({', '.join(self.tracers) or 'none'})")
        self.vapor = vapor
        self.fill = bool(getattr(self.config, "fill", False))
        self.acoustic_dynamics = AcousticDynamics(comm, grid_data, sf, qf, damping_coefficients, config=self.config, phis=phis, state=state, checkpointer=checkpointer)
        self.layout = self.acoustic_dynamics.layout
        cell = (X_DIM, Y_DIM, Z_DIM)
        self.tracer_advection = None
        self.dp1 = None
        self._tracer_halo = None
        if self.tracers:
            self.dp1 = qf.zeros(cell, "Pa")
            self.tracer_advection = st.TracerAdvection(sf, qf, st.FiniteVolumeTransport(sf, qf, grid_data, hord=hord_tr), grid_data, self.layout, self.tracers)
            self._tracer_halo = self.acoustic_dynamics.halo.updater("cell", [(q,) for q in self.tracers.values()])
        self.remap = st.LagrangianToEulerian(sf, qf, grid_data, fill=self.fill)
        self.ps = qf.zeros((X_DIM, Y_DIM), "Pa")
        self.temperature_to_potential = st.TemperatureToPotential(sf, qf, grid_data)
        self.potential_to_temperature = st.PotentialToTemperature(sf, qf, grid_data)
        self.cubed_to_latlon = st.CubedToLatLon(sf, qf, grid_data, order=self.config.c2l_ord, comm=self.layout) if cubed_to_latlon else None
        self.adjust_negative_water = None
        if adjust_negative_water:
            missing = [r for r in st.WATER_ROLES if r not in (water_species or {})]
            if missing:
                raise ValueError(f"adjust_negative_water=True needs water_species with all six roles (missing: {', '.join(missing)})")
            self.adjust_negative_water = st.AdjustNegativeTracerMixingRatio(sf, qf, grid_data)
        self.saturation_adjustment = None
        if saturation_adjustment:
            missing = [r for r in st.WATER_ROLES if r not in (water_species or {})]
            if missing:
                raise ValueError(f"saturation_adjustment=True needs water_species with all six roles (missing: {', '.join(missing)})")
            self.saturation_adjustment = st.SaturationAdjustment(sf, qf, grid_data, sat_adjust_config)

    @property
    def qvapor(self) -> Optional[Quantity]:
        return None if self.vapor is None else self.tracers[self.vapor]

    def step_dynamics(self, state: DycoreState, timer=None):
        """One model step: ``state.pt`` is a temperature (K) on entry and on return.  ``timer`` (pace_amd.timer.Timer): the
        reference's clocks "DynCore", "TracerAdvection", "Remapping", "CubedToLatLon" [REF tests/main/driver/test_driver.py:77-121] and this
        build's "NegAdj3"."""
        from .timer import NullTimer

        timer = timer or NullTimer()
        s, dyn, tracers, qv = state, self.acoustic_dynamics, self.tracers, self.qvapor
        water = self.water
        self.temperature_to_potential(s.pt, s.pkz, s.delp, s.delz, s.q_con, s.cappa, qv, water=water)
        k_split = self.config.k_split
        dt = self.timestep / k_split
        for k in range(k_split):
            if tracers:
                self.dp1.storage.copy_(s.delp.storage)  # the air mass the accumulated mass fluxes start from
            with timer.clock("DynCore"):
                dyn(s, dt, n_map=k + 1)
            if tracers:
                with timer.clock("TracerAdvection"):
                    self._tracer_halo.update()
                    self.tracer_advection(tracers, self.dp1, s.mfxd, s.mfyd, s.cxd, s.cyd)
            with timer.clock("Remapping"):
                if self.saturation_adjustment is not None:
                    self.remap(tracers, s.pt, s.delp, s.delz, s.peln, s.pe, s.pk, s.pkz, s.u, s.v, s.w, s.cappa, self.ps, dyn._wsd, q_con=s.q_con, water=water,
                               sat_adjust=self.saturation_adjustment, mdt=dt, last_step=(k == k_split - 1))
                else:
                    self.remap(tracers, s.pt, s.delp, s.delz, s.peln, s.pe, s.pk, s.pkz, s.u, s.v, s.w, s.cappa, self.ps, dyn._wsd, q_con=s.q_con, water=water)
        # the last-step conversion of the remap: pkz is the one the remap has just formed with these delp, delz and T_v
        self.potential_to_temperature(s.pt, s.pkz, s.delp, s.delz, s.q_con, s.cappa, s.w, s.pe, qvapor=qv, omga=s.omga, ps=self.ps, recompute_pkz=False)
        if self.adjust_negative_water is not None:
            with timer.clock("NegAdj3"):
                self.adjust_negative_water(pt=s.pt, delp=s.delp, water=water)
        if self.cubed_to_latlon is not None:
            with timer.clock("CubedToLatLon"):
                self.cubed_to_latlon(s.u, s.v, s.ua, s.va)
