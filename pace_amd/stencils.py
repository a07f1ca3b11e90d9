"""Operator classes of the acoustic path -- same names, constructor shape and ``__call__``
argument order as the pyFV3 operators the reference constructs
(ctor/call evidence [REF examples/notebooks/functions.py:877-891,935-951],
class names [REF tests/main/fv3core/test_config.py:10-16]).  Each call is one C-ABI entry of
``libfv3_mi355x`` enqueued on the factory's HIP stream; nothing is allocated or compiled at
call time [REF tests/main/fv3core/test_dycore_call.py:193-211].
"""
from __future__ import annotations

import dataclasses
from typing import Optional

from .constants import SAT_ADJ_DEFAULTS as _SAT
from .constants import X_DIM, X_INTERFACE_DIM, Y_DIM, Y_INTERFACE_DIM, Z_DIM, Z_INTERFACE_DIM
from .context import StencilFactory
from .quantity import Quantity

_CELL = (X_DIM, Y_DIM, Z_DIM)


def _ref(q: Optional[Quantity]):
    return None if q is None else q.fref


def _as_numpy(x):
    """Host values of a 1-D / 2-D argument given as numpy array, torch tensor or Quantity; None when it cannot be inspected cheaply."""
    import numpy as np

    if isinstance(x, Quantity):
        return None  # (per-sub-domain device field: see _check_metric)
    if hasattr(x, "detach"):
        return x.detach().cpu().numpy()
    try:
        return np.asarray(x, dtype=np.float64)
    except Exception:
        return None


def _check_owned(sf: StencilFactory, op: str, name: str, given, expected, rtol=1.0e-12):
    """The C side owns the level columns (``dp_ref``, ``pfull``, ``ks``) and the metric terms (``rdxc``, ``rdyc``): they are uploaded
    once with the context and the kernels read them there.  The reference passes them at every call; a caller that passes
    DIFFERENT values would silently get the context's -- refuse instead.  ``None`` = "use the context's" (accepted)."""
    import numpy as np

    if given is None:
        return
    if isinstance(given, Quantity):
        own = sf.grid_fields.get(name)
        if own is not None and given.storage.data_ptr() == own.storage.data_ptr():
            return  # the context's own field
        if own is not None and given.storage.shape == own.storage.shape:
            import torch

            if bool(torch.allclose(given.storage.double(), own.storage.double(), rtol=rtol, atol=0.0)):
                return
        raise ValueError(f"{op}: argument {name!r} differs from the metric term the context was created with (the kernels read the context's copy)")
    g = _as_numpy(given)
    if g is None or expected is None:
        return
    e = np.asarray(expected, dtype=np.float64)
    if g.shape != e.shape or not np.allclose(g, e, rtol=rtol, atol=0.0):
        raise ValueError(f"{op}: argument {name!r} differs from the values the context was created with (GridData.{name}; the kernels read the context's copy)")


class _Op:
    def __init__(self, stencil_factory: StencilFactory, quantity_factory=None, grid_data=None, *_, **__):
        self.sf = stencil_factory
        self.qf = quantity_factory or stencil_factory.quantity_factory
        self.grid_data = grid_data


class CGridShallowWaterDynamics(_Op):
    """``c_sw``; returns (delpc, ptc) like the reference."""

    def __init__(self, stencil_factory, quantity_factory=None, grid_data=None, nested=False, grid_type=0, nord=None):
        super().__init__(stencil_factory, quantity_factory, grid_data)
        self.delpc = self.qf.zeros(_CELL, "Pa")
        self.ptc = self.qf.zeros(_CELL, "K")

    def __call__(self, delp, pt, u, v, w, uc, vc, ua, va, ut, vt, divgd, omga, dt2):
        self.sf.call("c_sw", delp.fref, pt.fref, u.fref, v.fref, w.fref, uc.fref, vc.fref, ua.fref, va.fref, ut.fref, vt.fref, divgd.fref, omga.fref, self.delpc.fref, self.ptc.fref, float(dt2))
        return self.delpc, self.ptc


class UpdateGeopotentialHeightOnCGrid(_Op):
    def __call__(self, dp_ref, zs, ut, vt, gz, ws, dt):
        _check_owned(self.sf, "update_dz_c", "dp_ref", dp_ref, self.sf.grids[0].dp_ref)
        self.sf.call("update_dz_c", zs.fref, ut.fref, vt.fref, gz.fref, ws.fref, float(dt))


class RiemannSolverC(_Op):
    def __call__(self, dt2, cappa, ptop, phis, ws, ptc, q_con, delpc, gz, pef, w3):
        self.sf.call("riem_solver_c", float(dt2), cappa.fref, float(ptop), phis.fref, ws.fref, ptc.fref, q_con.fref, delpc.fref, gz.fref, pef.fref, w3.fref)


class PGradC(_Op):
    """The ``p_grad_c`` stencil of dyn_core."""

    def __call__(self, rdxc, rdyc, uc, vc, delpc, pkc, gz, dt2):
        _check_owned(self.sf, "p_grad_c", "rdxc", rdxc, None)
        _check_owned(self.sf, "p_grad_c", "rdyc", rdyc, None)
        self.sf.call("p_grad_c", uc.fref, vc.fref, delpc.fref, pkc.fref, gz.fref, float(dt2))


class FiniteVolumeFluxPrep(_Op):
    def __init__(self, stencil_factory, grid_data=None, grid_type=0):
        super().__init__(stencil_factory, None, grid_data)

    def __call__(self, uc, vc, crx, cry, x_area_flux, y_area_flux, uc_contra, vc_contra, dt):
        self.sf.call("fxadv", uc.fref, vc.fref, crx.fref, cry.fref, x_area_flux.fref, y_area_flux.fref, uc_contra.fref, vc_contra.fref, float(dt))


class FiniteVolumeTransport(_Op):
    """``fv_tp_2d``.  ``nord``/``damp_c`` enable the del-n damping fluxes (scalars here; the
    per-level columns of d_sw are handled inside ``fv3_d_sw``)."""

    def __init__(self, stencil_factory, quantity_factory=None, grid_data=None, damping_coefficients=None, grid_type=0, hord=6, nord=None, damp_c=None):
        super().__init__(stencil_factory, quantity_factory, grid_data)
        self.hord = int(hord)
        self.nord = -1 if nord is None else int(nord)
        self.damp_c = 0.0 if damp_c is None else float(damp_c)

    def __call__(self, q, crx, cry, x_area_flux, y_area_flux, q_x_flux, q_y_flux, x_mass_flux=None, y_mass_flux=None, mass=None):
        self.sf.call("fv_tp_2d", q.fref, crx.fref, cry.fref, x_area_flux.fref, y_area_flux.fref, q_x_flux.fref, q_y_flux.fref, _ref(x_mass_flux), _ref(y_mass_flux), _ref(mass), self.hord, self.nord, self.damp_c)


class AGrid2BGridFourthOrder(_Op):
    def __init__(self, stencil_factory, quantity_factory=None, grid_data=None, grid_type=0, z_dim=Z_DIM, replace=False):
        super().__init__(stencil_factory, quantity_factory, grid_data)
        self.replace = bool(replace)
        self.nk = stencil_factory.sizer.nz + (1 if z_dim == Z_INTERFACE_DIM else 0)

    def __call__(self, qin, qout, kstart=0, nk=None):
        self.sf.call("a2b_ord4", qin.fref, qout.fref, int(kstart), int(self.nk if nk is None else nk), int(self.replace))


def check_stretched_grid(who, stretched_grid, stencil_factory):
    """The ``stretched_grid`` keyword of an operator against the flag its context was created with (the context formed the divergence
    damping table in that form): None follows the context, anything else must agree."""
    have = bool(stencil_factory.config.stretched_grid)
    if stretched_grid is not None and bool(stretched_grid) != have:
        raise ValueError(f"{who}(stretched_grid={bool(stretched_grid)}): the stencil factory's config has stretched_grid={have}, and its damping tables were formed for that.")


class DGridShallowWaterLagrangianDynamics(_Op):
    def __init__(self, stencil_factory, quantity_factory=None, grid_data=None, damping_coefficients=None, column_namelist=None, nested=False, stretched_grid=None, config=None):
        super().__init__(stencil_factory, quantity_factory, grid_data)
        check_stretched_grid("DGridShallowWaterLagrangianDynamics", stretched_grid, stencil_factory)

    def __call__(self, delpc, delp, pt, u, v, w, uc, vc, ua, va, divgd, mfx, mfy, cx, cy, crx, cry, xfx, yfx, q_con, zh, heat_source, diss_est, dt):
        a = (delpc, delp, pt, u, v, w, uc, vc, ua, va, divgd, mfx, mfy, cx, cy, crx, cry, xfx, yfx, q_con, zh, heat_source, diss_est)
        self.sf.call("d_sw", *[x.fref for x in a], float(dt))


class UpdateHeightOnDGrid(_Op):
    def __call__(self, surface_height, height, courant_number_x, courant_number_y, x_area_flux, y_area_flux, ws, dt):
        self.sf.call("update_dz_d", surface_height.fref, height.fref, courant_number_x.fref, courant_number_y.fref, x_area_flux.fref, y_area_flux.fref, ws.fref, float(dt))


class RiemannSolver3(_Op):
    def __call__(self, last_call, dt, cappa, ptop, zs, wsd, delz, q_con, delp, pt, zh, pe, ppe, pk3, pk, peln, w):
        self.sf.call("riem_solver3", int(bool(last_call)), float(dt), cappa.fref, float(ptop), zs.fref, wsd.fref, delz.fref, q_con.fref, delp.fref, pt.fref, zh.fref, pe.fref, ppe.fref, pk3.fref, pk.fref, peln.fref, w.fref)


class PK3Halo(_Op):
    def __call__(self, pk3, delp, ptop, akap):
        self.sf.call("pk3_halo", pk3.fref, delp.fref, float(ptop), float(akap))


class EdgePE(_Op):
    def __call__(self, pe, delp, ptop):
        self.sf.call("edge_pe", pe.fref, delp.fref, float(ptop))


class NonHydrostaticPressureGradient(_Op):
    def __call__(self, u, v, pp, gz, pk3, delp, dt, ptop, akap):
        self.sf.call("nh_p_grad", u.fref, v.fref, pp.fref, gz.fref, pk3.fref, delp.fref, float(dt), float(ptop), float(akap))


class RayleighDamping(_Op):
    def __call__(self, u, v, w, dp, pfull, dt, ptop, ks=None):
        _check_owned(self.sf, "ray_fast", "dp_ref", dp, self.sf.grids[0].dp_ref)
        _check_owned(self.sf, "ray_fast", "pfull", pfull, self.sf.grids[0].pfull)
        if ks is not None and int(ks) != int(self.sf.grids[0].ks):
            raise ValueError(f"ray_fast: ks = {ks} differs from the context's ({self.sf.grids[0].ks}: number of pure-pressure layers of ak / bk)")
        self.sf.call("ray_fast", u.fref, v.fref, w.fref, float(dt), float(ptop))


class HyperdiffusionDamping(_Op):
    def __init__(self, stencil_factory, quantity_factory=None, damping_coefficients=None, rarea=None, nmax=3):
        super().__init__(stencil_factory, quantity_factory, None)
        self.nmax = int(nmax)

    def __call__(self, qdel, cd):
        self.sf.call("del2_cubed", qdel.fref, float(cd), self.nmax)


class ApplyDiffusiveHeating(_Op):
    def __call__(self, delp, delz, cappa, heat_source, pt, delt_time_factor):
        self.sf.call("apply_diffusive_heating", delp.fref, delz.fref, cappa.fref, heat_source.fref, pt.fref, float(delt_time_factor))


class TracerAdvection(_Op):
    """``tracer_2d_1l``: sub-cycled 2-D advection of the tracers with the mass fluxes / Courant numbers the
    acoustic sub-steps accumulated.  Constructor and call as the reference's
    ``TracerAdvection(stencil_factory, quantity_factory, transport, grid_data, comm, tracers)`` /
    ``tracer_advection(tracers, dp1, mfxd, mfyd, cxd, cyd)`` [REF examples/notebooks/functions.py:916-951, 1037-1044].
    ``transport`` is a :class:`FiniteVolumeTransport` (its ``hord`` is used: 5 / 6, or 8 = the monotone scheme of the
    reference's dycore configs, ``hord_tr: 8``), ``comm`` a :class:`pace_amd.halo.Layout` (or None: all ranks local)."""

    def __init__(self, stencil_factory, quantity_factory=None, transport=None, grid_data=None, comm=None, tracers=None):
        super().__init__(stencil_factory, quantity_factory, grid_data)
        self.hord = int(getattr(transport, "hord", 6))
        self.comm = comm
        self._halo = None
        self._updater = None
        self._bound = None
        self.n_split = None  # of the last call

    def _tracer_updater(self, tracers):
        from .halo import HaloExchanger, Layout
        from .topology import CubedSpherePartitioner

        key = tuple(id(q) for q in tracers.values())
        if self._bound != key:
            lay = self.comm
            if lay is None:
                cfg = self.sf.config
                lay = Layout(CubedSpherePartitioner(cfg.npx - 1, tuple(cfg.layout)), 1, 0)
            if self._halo is None:
                # the context's one exchanger (the acoustic dynamics' own when it exists): it owns the transport
                self._halo = HaloExchanger.shared(self.sf, lay, group=getattr(lay, "group", None))
            self._updater = self._halo.updater("cell", [(q,) for q in tracers.values()])
            self._bound = key
        return self._updater

    def __call__(self, tracers, dp1, x_mass_flux, y_mass_flux, x_courant, y_courant):
        import ctypes as C

        import torch

        from . import lib as _lib

        sf = self.sf
        cmax = C.c_double()
        st = sf.lib.fv3_tracer_2d_1l_cmax(sf.ctx, x_courant.fref, y_courant.fref, C.byref(cmax), sf.stream_handle)
        if st != 0:
            raise _lib.Fv3Error("fv3_tracer_2d_1l_cmax failed: " + sf.lib.fv3_last_error(sf.ctx).decode())
        cm = cmax.value
        lay = self.comm
        if lay is not None and lay.world_size > 1:  # the operator's one global quantity: all-reduce MAX over the processes
            import torch.distributed as dist

            t = torch.tensor([cm], dtype=torch.float64, device=sf.device if dist.get_backend(getattr(lay, "group", None)) == "nccl" else "cpu")
            dist.all_reduce(t, op=dist.ReduceOp.MAX, group=getattr(lay, "group", None))
            cm = float(t.item())
        n_split = int(1.0 + cm)
        self.n_split = n_split
        qs = list(tracers.values())
        arr = (_lib.F * max(len(qs), 1))(*[C.pointer(q.field) for q in qs])
        plan = None
        if n_split > 1:
            up = self._tracer_updater(tracers)
            if not up.ex.native:
                raise _lib.Fv3Error("tracer_2d_1l with sub-cycles needs the native halo plans (FV3_HALO_NATIVE=1)")
            plan = up._native_plan()
        st = sf.lib.fv3_tracer_2d_1l(sf.ctx, len(qs), arr, dp1.fref, x_mass_flux.fref, y_mass_flux.fref, x_courant.fref, y_courant.fref, n_split, self.hord, plan,
                                     sf.stream_handle)
        if st != 0:
            raise _lib.Fv3Error(f"fv3_tracer_2d_1l failed ({st}): " + sf.lib.fv3_last_error(sf.ctx).decode())


class FillNegativeTracerValues(_Op):
    """``fillz`` (FV3 ``fv_fill.F90``; the pyFV3 operator of this name): negative layer means of the tracers are filled, column by
    column, with mass borrowed from the neighbouring layers and -- where that does not suffice -- by rescaling the positive
    part of the column (``fv3_fillz`` in include/fv3_mi355x.h holds the algorithm).  In place on the compute cells; ``dp2`` (the
    layer thickness the mixing ratios refer to) is only read.  Call as the reference's ``fillz(dp2, tracers)`` with ``tracers``
    a dict of quantities."""

    def __call__(self, dp2, tracers):
        import ctypes as C

        from . import lib as _lib

        qs = list(tracers.values()) if tracers else []
        arr = (_lib.F * max(len(qs), 1))(*[C.pointer(q.field) for q in qs])
        st = self.sf.lib.fv3_fillz(self.sf.ctx, len(qs), arr, dp2.fref, self.sf.stream_handle)
        if st != 0:
            raise _lib.Fv3Error(f"fv3_fillz failed ({st}): " + self.sf.lib.fv3_last_error(self.sf.ctx).decode())


class LagrangianToEulerian(_Op):
    """The vertical remap that closes ``DynamicalCore.step_dynamics`` (reference operator pyFV3
    ``LagrangianToEulerian``, savepoint ``Remapping`` [REF tests/savepoint/thresholds/fv_dynamics.yaml:227-326]).  Call with the
    state's quantities; everything is remapped in place (see ``fv3_remap`` in include/fv3_mi355x.h for the configuration).
    ``fill`` (the namelist's ``fill``, default off): after the remap the negative tracer means are filled in the vertical
    (:class:`FillNegativeTracerValues` with the Eulerian ``delp``) on the same stream, where the reference runs its ``fillz``.
    ``water`` (a :class:`WaterSpecies` whose species are among ``tracers``) with ``q_con``: the moist remap ``fv3_remap_moist`` --
    remap, fill, ``q_con`` / ``cappa`` from the filled species (``moist_cv``), ``pkz`` with the new ``cappa``, FV3's order.
    ``sat_adjust`` (a :class:`SaturationAdjustment`; needs ``water`` with all six species and ``mdt``, the remap interval in seconds):
    ``fv3_remap_moist_sat`` -- the saturation adjustment between the fill and ``moist_cv``, in the same closing kernel; ``last_step``
    asks for its second pass to full saturation."""

    def __init__(self, stencil_factory, quantity_factory=None, grid_data=None, *args, fill: bool = False, **kw):
        super().__init__(stencil_factory, quantity_factory, grid_data, *args, **kw)
        self.fill = bool(fill)
        self._fillz = FillNegativeTracerValues(stencil_factory, quantity_factory, grid_data) if self.fill else None

    def __call__(self, tracers, pt, delp, delz, peln, pe, pk, pkz, u, v, w, cappa, ps, wsd, q_con=None, water=None, *, sat_adjust=None, mdt=None, last_step=False):
        import ctypes as C

        from . import lib as _lib

        qs = list(tracers.values()) if tracers else []
        arr = (_lib.F * max(len(qs), 1))(*[C.pointer(q.field) for q in qs])
        if sat_adjust is not None:
            # (sat_adjust: a SaturationAdjustment) FV3's order with do_sat_adj: remap, fill, fv_sat_adj, moist_cv, pkz -- all inside the entry
            if water is None or q_con is None:
                raise ValueError("LagrangianToEulerian: sat_adjust needs water and q_con (the adjustment works on the six water species)")
            if mdt is None:
                raise ValueError("LagrangianToEulerian: sat_adjust needs mdt (the remap interval in seconds)")
            st = self.sf.lib.fv3_remap_moist_sat(self.sf.ctx, len(qs), arr, pt.fref, delp.fref, delz.fref, peln.fref, pe.fref, pk.fref, pkz.fref, u.fref, v.fref, w.fref,
                                                 cappa.fref, q_con.fref, ps.fref, wsd.fref, water.cref, 1 if self.fill else 0, sat_adjust.latent_ref, sat_adjust.params_ref,
                                                 float(mdt), 1 if last_step else 0, self.sf.stream_handle)
            if st != 0:
                raise _lib.Fv3Error(f"fv3_remap_moist_sat failed ({st}): " + self.sf.lib.fv3_last_error(self.sf.ctx).decode())
            return
        if water is not None:
            # FV3's order: remap, fill, moist_cv from the filled species, pkz with the new cappa -- all inside the entry
            if q_con is None:
                raise ValueError("LagrangianToEulerian: water needs q_con (the moist remap writes it)")
            st = self.sf.lib.fv3_remap_moist(self.sf.ctx, len(qs), arr, pt.fref, delp.fref, delz.fref, peln.fref, pe.fref, pk.fref, pkz.fref, u.fref, v.fref, w.fref,
                                             cappa.fref, q_con.fref, ps.fref, wsd.fref, water.cref, 1 if self.fill else 0, self.sf.stream_handle)
            if st != 0:
                raise _lib.Fv3Error(f"fv3_remap_moist failed ({st}): " + self.sf.lib.fv3_last_error(self.sf.ctx).decode())
            return
        st = self.sf.lib.fv3_remap(self.sf.ctx, len(qs), arr, pt.fref, delp.fref, delz.fref, peln.fref, pe.fref, pk.fref, pkz.fref, u.fref, v.fref, w.fref, cappa.fref,
                                   ps.fref, wsd.fref, self.sf.stream_handle)
        if st != 0:
            raise _lib.Fv3Error(f"fv3_remap failed ({st}): " + self.sf.lib.fv3_last_error(self.sf.ctx).decode())
        if self._fillz is not None and qs:
            self._fillz(delp, tracers)  # delp is the Eulerian layer thickness by now: the reference's dp2


WATER_ROLES = ("qvapor", "qliquid", "qrain", "qice", "qsnow", "qgraupel")


class WaterSpecies:
    """The six water species of ``moist_cv`` (``fv3_water`` in include/fv3_mi355x.h): ``qvapor`` and up to five optional Quantities
    (None: a field of zeros) plus the heat capacities ``cv_vap``, ``c_liq``, ``c_ice`` (J/kg/K; defaults: pace_amd.constants)."""

    def __init__(self, qvapor, qliquid=None, qrain=None, qice=None, qsnow=None, qgraupel=None, cv_vap=None, c_liq=None, c_ice=None):
        import ctypes as C

        from . import constants as _c
        from . import lib as _lib

        if qvapor is None:
            raise ValueError("WaterSpecies: qvapor is required (the other five species are optional)")
        self.species = dict(qvapor=qvapor, qliquid=qliquid, qrain=qrain, qice=qice, qsnow=qsnow, qgraupel=qgraupel)
        self.cv_vap = float(_c.CV_VAP if cv_vap is None else cv_vap)
        self.c_liq = float(_c.C_LIQ if c_liq is None else c_liq)
        self.c_ice = float(_c.C_ICE if c_ice is None else c_ice)
        self.struct = _lib.fv3_water(*[None if q is None else C.pointer(q.field) for q in self.species.values()], self.cv_vap, self.c_liq, self.c_ice)
        self.cref = C.byref(self.struct)

    @classmethod
    def from_tracers(cls, tracers, roles, **constants):
        """``roles``: {role: tracer name} for the roles of ``WATER_ROLES`` that exist (a missing role is a field of zeros)."""
        unknown = sorted(set(roles) - set(WATER_ROLES))
        if unknown:
            raise ValueError(f"water species roles {unknown}: the roles are {', '.join(WATER_ROLES)}")
        missing = sorted(n for n in roles.values() if n not in tracers)
        if missing:
            raise ValueError(f"water species {missing} are not among the tracers ({', '.join(tracers) or 'none'})")
        if "qvapor" not in roles:
            raise ValueError("water species: the role qvapor is required")
        return cls(**{r: tracers[n] for r, n in roles.items()}, **constants)

    def __getattr__(self, name):
        if name in WATER_ROLES:
            return self.species[name]
        raise AttributeError(name)


class MoistCV(_Op):
    """FV3's ``moist_cv`` for six water species (``fv3_moist_cv``; include/fv3_mi355x.h holds the formulas): ``q_con`` and ``cappa``
    (and the moist heat capacity ``cvm`` where given) from the species, on the compute cells."""

    def __call__(self, water, q_con, cappa, cvm=None):
        from . import lib as _lib

        sf = self.sf
        st = sf.lib.fv3_moist_cv(sf.ctx, water.cref, q_con.fref, cappa.fref, _ref(cvm), sf.stream_handle)
        if st != 0:
            raise _lib.Fv3Error(f"fv3_moist_cv failed ({st}): " + sf.lib.fv3_last_error(sf.ctx).decode())


class AdjustNegativeTracerMixingRatio(_Op):
    """``neg_adj3`` (FV3 ``fv_sg.F90``; the pyFV3 operator of this name), which ``fv_dynamics`` runs between the last remap and
    ``CubedToLatLon`` when ``nwat = 6``: a negative condensate is paid for out of another phase with the latent heat booked on the
    temperature ``pt`` (K), negative vapour is repaid from the layer below (``fv3_neg_adj3`` in include/fv3_mi355x.h holds the
    algorithm).  In place on the compute cells; ``delp`` is only read.  The non-hydrostatic form only.  ``hlv``, ``hlf``, ``t_ice``:
    the latent heats of vaporisation and fusion (J/kg) and the freezing point (K) (defaults: pace_amd.constants).

    Call as the reference's ``(qvapor, qliquid, qrain, qsnow, qice, qgraupel, qcld, pt, delp, delz, peln)``: ``qcld`` must be None
    (the cloud-fraction fix is not part of this build); ``delz`` and ``peln`` are accepted and not read.  ``water=`` (a
    :class:`WaterSpecies` with all six species) takes the place of the six positional species."""

    def __init__(self, stencil_factory, quantity_factory=None, grid_data=None, *, hydrostatic=False, hlv=None, hlf=None, t_ice=None):
        import ctypes as C

        from . import constants as _c
        from . import lib as _lib

        super().__init__(stencil_factory, quantity_factory, grid_data)
        if hydrostatic:
            raise NotImplementedError("AdjustNegativeTracerMixingRatio: only the non-hydrostatic form of neg_adj3 is built")
        self.hlv = float(_c.HLV if hlv is None else hlv)
        self.hlf = float(_c.HLF if hlf is None else hlf)
        self.t_ice = float(_c.T_ICE if t_ice is None else t_ice)
        self.latent = _lib.fv3_latent(self.hlv, self.hlf, self.t_ice)
        self._lref = C.byref(self.latent)

    def __call__(self, qvapor=None, qliquid=None, qrain=None, qsnow=None, qice=None, qgraupel=None, qcld=None, pt=None, delp=None, delz=None, peln=None, *, water=None):
        from . import lib as _lib

        if qcld is not None:
            raise NotImplementedError("AdjustNegativeTracerMixingRatio: the cloud-fraction fix of neg_adj3 is not built, so qcld must be None")
        species = (qvapor, qliquid, qrain, qsnow, qice, qgraupel)
        if water is None:
            water = WaterSpecies(qvapor, qliquid=qliquid, qrain=qrain, qice=qice, qsnow=qsnow, qgraupel=qgraupel)
        elif any(q is not None for q in species):
            raise ValueError("AdjustNegativeTracerMixingRatio: give the six species or water=, not both")
        if pt is None or delp is None:
            raise ValueError("AdjustNegativeTracerMixingRatio: pt and delp are required")
        sf = self.sf
        st = sf.lib.fv3_neg_adj3(sf.ctx, water.cref, self._lref, pt.fref, delp.fref, sf.stream_handle)
        if st != 0:
            raise _lib.Fv3Error(f"fv3_neg_adj3 failed ({st}): " + sf.lib.fv3_last_error(sf.ctx).decode())


@dataclasses.dataclass
class SatAdjustConfig:
    """The namelist parameters of the saturation adjustment (``fv3_sat_params`` in include/fv3_mi355x.h); the field names are the
    yaml keys of ``dycore_config``, the defaults FV3's (``pace_amd.constants.SAT_ADJ_DEFAULTS``)."""

    tau_i2s: float = _SAT["tau_i2s"]
    tau_v2l: float = _SAT["tau_v2l"]
    tau_l2v: float = _SAT["tau_l2v"]
    tau_imlt: float = _SAT["tau_imlt"]
    tau_r2g: float = _SAT["tau_r2g"]
    tau_smlt: float = _SAT["tau_smlt"]
    tau_l2r: float = _SAT["tau_l2r"]
    ql_gen: float = _SAT["ql_gen"]
    qi_gen: float = _SAT["qi_gen"]
    qi_lim: float = _SAT["qi_lim"]
    ql_mlt: float = _SAT["ql_mlt"]
    qs_mlt: float = _SAT["qs_mlt"]
    ql0_max: float = _SAT["ql0_max"]
    qi0_max: float = _SAT["qi0_max"]
    sat_adj0: float = _SAT["sat_adj0"]
    t_sub: float = _SAT["t_sub"]


class SaturationAdjustment(_Op):
    """``fv_sat_adj`` (FV3 ``fv_cmp.F90``, the non-hydrostatic form; pyFV3 ``SatAdjust3d``), which the remap runs when ``do_sat_adj`` is
    set: phase changes between the six water species with the latent heat booked on the temperature (``fv3_sat_adj`` in
    include/fv3_mi355x.h holds the algorithm).  Call as ``(water, tv, delp, delz, q_con, cappa, pkz, mdt, last_step=False)``: in place
    on the compute cells of the levels below 10 hPa (``level0`` is the first); ``tv`` is ``T (1 + zvir qv)(1 - q_con)`` in and out,
    ``q_con``, ``cappa`` and ``pkz`` are written, ``delp`` and ``delz`` only read; ``mdt``: the remap interval in seconds;
    ``last_step``: the second pass to full saturation.  Handed to :class:`LagrangianToEulerian` as ``sat_adjust=`` it runs inside
    the moist remap (``fv3_remap_moist_sat``).  Not built: the energy fixer, the ``out_dt`` tendency, the cloud fraction."""

    def __init__(self, stencil_factory, quantity_factory=None, grid_data=None, config=None, *, hydrostatic=False, do_qa=False, hlv=None, hlf=None, t_ice=None):
        import ctypes as C

        from . import constants as _c
        from . import lib as _lib

        super().__init__(stencil_factory, quantity_factory, grid_data)
        if hydrostatic:
            raise NotImplementedError("SaturationAdjustment: only the non-hydrostatic form of fv_sat_adj is built")
        if do_qa:
            raise NotImplementedError("SaturationAdjustment: the cloud fraction of fv_sat_adj (do_qa) is not built")
        self.config = config or SatAdjustConfig()
        self.latent = _lib.fv3_latent(float(_c.HLV if hlv is None else hlv), float(_c.HLF if hlf is None else hlf), float(_c.T_ICE if t_ice is None else t_ice))
        self.params = _lib.fv3_sat_params(*[float(getattr(self.config, n)) for n in _lib.SAT_PARAMS])
        self.latent_ref, self.params_ref = C.byref(self.latent), C.byref(self.params)

    @property
    def level0(self) -> int:
        import ctypes as C

        k = C.c_int()
        _lib_check(self.sf, self.sf.lib.fv3_sat_adj_level0(self.sf.ctx, C.byref(k)), "fv3_sat_adj_level0")
        return k.value

    def tables(self):
        """(4, 2621) float64: tablew, table2, desw, des2 as the kernels hold them (after the context's first adjusting call)."""
        import ctypes as C

        import numpy as np

        from . import lib as _lib

        out = np.empty((4, _lib.SAT_NTAB), dtype=np.float64)
        _lib_check(self.sf, self.sf.lib.fv3_sat_adj_tables(self.sf.ctx, out.ctypes.data_as(C.POINTER(C.c_double)), out.size), "fv3_sat_adj_tables")
        return out

    def __call__(self, water, tv, delp, delz, q_con, cappa, pkz, mdt, last_step=False):
        sf = self.sf
        st = sf.lib.fv3_sat_adj(sf.ctx, water.cref, self.latent_ref, self.params_ref, tv.fref, delp.fref, delz.fref, q_con.fref, cappa.fref, pkz.fref, float(mdt),
                                1 if last_step else 0, sf.stream_handle)
        _lib_check(sf, st, "fv3_sat_adj")


def _lib_check(sf, st, what):
    from . import lib as _lib

    if st != 0:
        raise _lib.Fv3Error(f"{what} failed ({st}): " + sf.lib.fv3_last_error(sf.ctx).decode())


class TemperatureToPotential(_Op):
    """The preamble of ``fv_dynamics`` (``fv3_pt_from_temperature`` in include/fv3_mi355x.h holds the formulas): ``pt`` goes from
    the temperature (K) the model state holds between steps to the form the acoustic loop transports, ``T_v / pkz``, and
    ``pkz`` is rebuilt from the full (non-hydrostatic) pressure.  In place on the compute cells; ``delp``, ``delz``, ``q_con``,
    ``cappa`` and ``qvapor`` (the specific humidity, None: a dry conversion) are only read.  With ``water`` (a
    :class:`WaterSpecies`) ``q_con`` and ``cappa`` are formed from the species in the same kernel and written
    (``fv3_pt_from_temperature_moist``: bit for bit :class:`MoistCV` followed by the dry call with ``qvapor = water.qvapor``)."""

    def __call__(self, pt, pkz, delp, delz, q_con, cappa, qvapor=None, water=None):
        from . import lib as _lib

        sf = self.sf
        if water is not None:
            # moist_cv inside the cell: q_con and cappa are outputs, qvapor is the species' own
            if qvapor is not None and qvapor is not water.qvapor:
                raise ValueError("TemperatureToPotential: qvapor differs from water.qvapor")
            st = sf.lib.fv3_pt_from_temperature_moist(sf.ctx, pt.fref, pkz.fref, delp.fref, delz.fref, q_con.fref, cappa.fref, water.cref, sf.stream_handle)
            if st != 0:
                raise _lib.Fv3Error(f"fv3_pt_from_temperature_moist failed ({st}): " + sf.lib.fv3_last_error(sf.ctx).decode())
            return
        st = sf.lib.fv3_pt_from_temperature(sf.ctx, pt.fref, pkz.fref, delp.fref, delz.fref, q_con.fref, cappa.fref, _ref(qvapor), sf.stream_handle)
        if st != 0:
            raise _lib.Fv3Error(f"fv3_pt_from_temperature failed ({st}): " + sf.lib.fv3_last_error(sf.ctx).decode())


class PotentialToTemperature(_Op):
    """The last-step conversion of the remap (``fv3_temperature_from_pt``): ``pt`` goes from the loop's form back to the
    temperature (K); ``omga`` (where given) becomes ``delp / delz * w`` and the 2-D ``ps`` (where given) the surface pressure
    ``pe[.., nz]``.  ``recompute_pkz=False`` is FV3's own form ``T_v = pt * pkz``, valid right after a remap; ``True`` derives
    ``T_v`` from the state alone and rebuilds ``pkz`` (a state whose ``pkz`` may be stale, e.g. one that was just initialised)."""

    def __call__(self, pt, pkz, delp, delz, q_con, cappa, w, pe, qvapor=None, omga=None, ps=None, recompute_pkz=False):
        from . import lib as _lib

        sf = self.sf
        st = sf.lib.fv3_temperature_from_pt(sf.ctx, pt.fref, pkz.fref, delp.fref, delz.fref, q_con.fref, cappa.fref, _ref(qvapor), w.fref, _ref(omga), pe.fref, _ref(ps),
                                            1 if recompute_pkz else 0, sf.stream_handle)
        if st != 0:
            raise _lib.Fv3Error(f"fv3_temperature_from_pt failed ({st}): " + sf.lib.fv3_last_error(sf.ctx).decode())


class CubedToLatLon(_Op):
    """``CubedToLatLon`` (FV3 ``fv_grid_utils.F90``: ``c2l_ord4`` / ``c2l_ord2``), the last operator of ``fv_dynamics``: the D-grid
    winds ``u``, ``v`` become the cell-centre winds ``ua`` (eastward) and ``va`` (northward) on the compute cells.  ``order``
    is ``c2l_ord`` (4, the reference's default, or 2).  Order 4 reads one row / column of halo: like the reference, the call
    starts with a D-grid vector halo update of ``u``, ``v`` (``comm``: a :class:`pace_amd.halo.Layout`, None = every rank in this
    process).  Call as the reference's ``cubed_to_latlon(u, v, ua, va)``."""

    def __init__(self, stencil_factory, quantity_factory=None, grid_data=None, order=4, comm=None):
        super().__init__(stencil_factory, quantity_factory, grid_data)
        self.order = int(order)
        if self.order not in (2, 4):
            raise ValueError(f"CubedToLatLon: order {order} (c2l_ord is 2 or 4)")
        self.comm = comm
        # the rotation terms of the context's sub-domains, uploaded once (2-D fields like phis)
        qf = self.qf
        self.a11, self.a12, self.a21, self.a22 = (qf.from_array([g.fields[n] for g in self.sf.grids], ("x", "y")) for n in ("a11", "a12", "a21", "a22"))
        self._updater = None
        self._bound = None

    def _uv_updater(self, u, v):
        from .halo import HaloExchanger, Layout
        from .topology import CubedSpherePartitioner

        key = (id(u), id(v))
        if self._bound != key:
            lay = self.comm
            if lay is None:
                cfg = self.sf.config
                lay = Layout(CubedSpherePartitioner(cfg.npx - 1, tuple(cfg.layout)), 1, 0)
            ex = HaloExchanger.shared(self.sf, lay, group=getattr(lay, "group", None))
            self._updater = ex.updater("dgrid", [(u, v)])
            self._bound = key
        return self._updater

    def __call__(self, u, v, ua, va):
        if self.order == 4:
            self._uv_updater(u, v).update()  # mpp_update_domains(u, v, DGRID_NE) inside c2l_ord4
        self.sf.call("cubed_to_latlon", self.order, u.fref, v.fref, ua.fref, va.fref, self.a11.fref, self.a12.fref, self.a21.fref, self.a22.fref)


@dataclasses.dataclass
class HeldSuarezConfig:
    """The constants of the Held-Suarez (1994) forcing (``fv3_held_suarez`` in include/fv3_mi355x.h); the defaults are the paper's:
    ``sigma_b`` the top of the boundary layer in sigma, ``k_f`` the friction rate at the surface (1/s), ``k_a`` / ``k_s`` the relaxation
    rates of the free atmosphere / at the surface on the equator (1/s), ``delta_t_y`` the equator-to-pole difference (K),
    ``delta_theta_z`` the static-stability parameter (K), ``p0`` the reference pressure (Pa), ``kappa = R / cp``, ``t_min`` the floor
    of the equilibrium temperature (K)."""

    sigma_b: float = 0.7
    k_f: float = 1.0 / 86400.0
    k_a: float = 1.0 / (40.0 * 86400.0)
    k_s: float = 1.0 / (4.0 * 86400.0)
    delta_t_y: float = 60.0
    delta_theta_z: float = 10.0
    p0: float = 1.0e5
    kappa: float = 2.0 / 7.0
    t_min: float = 200.0

    def validate(self):
        if not 0.0 <= self.sigma_b < 1.0:
            raise ValueError(f"HeldSuarezConfig: sigma_b = {self.sigma_b} (0 <= sigma_b < 1)")
        if not self.p0 > 0.0:
            raise ValueError(f"HeldSuarezConfig: p0 = {self.p0} (a pressure in Pa)")
        for n in ("k_f", "k_a", "k_s"):
            if not getattr(self, n) >= 0.0:
                raise ValueError(f"HeldSuarezConfig: {n} = {getattr(self, n)} (a rate in 1/s, >= 0)")
        return self


class HeldSuarezForcing(_Op):
    """The Held-Suarez (1994) forcing as cell-centre tendencies (``fv3_held_suarez_tend`` in include/fv3_mi355x.h holds the formulas):
    Rayleigh friction on the eastward / northward winds ``ua``, ``va`` below ``sigma_b`` and Newtonian relaxation of the temperature
    ``pt`` (K) to the paper's equilibrium, in the implicit form ``-k / (1 + dt k)``.  Call as
    ``(ua, va, pt, delp, u_dt, v_dt, pt_dt, dt, ptop=None)``: the three tendencies are written on the compute cells, nothing else is
    touched; ``ptop`` defaults to the grid's.  The operator is stateless: the pressure is formed from ``ptop`` and ``delp``."""

    def __init__(self, stencil_factory, quantity_factory=None, grid_data=None, config: Optional[HeldSuarezConfig] = None):
        import ctypes as C

        from . import lib as _lib

        super().__init__(stencil_factory, quantity_factory, grid_data)
        self.config = (config or HeldSuarezConfig()).validate()
        self.params = _lib.fv3_held_suarez(*[float(getattr(self.config, n)) for n in _lib.HS_PARAMS])
        self._pref = C.byref(self.params)
        self.lat = self.qf.from_array([g.fields["lat_agrid"] for g in self.sf.grids], ("x", "y"))
        self.ptop = float(self.sf.grids[0].ptop)

    def __call__(self, ua, va, pt, delp, u_dt, v_dt, pt_dt, dt, ptop=None):
        self.sf.call("held_suarez_tend", self._pref, ua.fref, va.fref, pt.fref, delp.fref, self.lat.fref, u_dt.fref, v_dt.fref, pt_dt.fref,
                     float(self.ptop if ptop is None else ptop), float(dt))


class DryConvectiveAdjustment(_Op):
    """The dry convective adjustment of the sponge layers (FV3 ``fv_subgrid_z``, ``fv_sg.F90``; pyFV3's ``DryConvectiveAdjustment``,
    which the reference driver runs after every ``step_dynamics`` when ``fv_sg_adj > 0``): on the top ``n_sponge`` levels a pair of
    neighbouring levels whose Richardson number is below a reference value mixes momentum, total energy, ``w`` and every tracer, in
    three passes, and the change is relaxed with ``timestep / fv_sg_adj`` (``fv3_subgrid_z`` in include/fv3_mi355x.h holds the
    algorithm).  Call as the reference's ``(state, u_dt, v_dt, timestep)``: it reads ``state.ua``, ``va`` (eastward / northward),
    ``w``, ``pt`` (the temperature in K, so the call belongs after ``DynamicalCore.step_dynamics``), ``delp``, ``delz``, ``peln``,
    ``pkz`` and the tracers; ``u_dt``, ``v_dt`` are assigned, not accumulated (zero below the sponge and in columns that did not
    mix); ``pt``, ``w`` and the tracers change in place on the top levels.  ``q_con``, ``cappa`` and ``pkz`` of the state are left as
    they are, as in FV3: the preamble of the next step rebuilds them.  The non-hydrostatic form only.

    ``tracers``: the dict (or list) of tracer quantities that are mixed; ``water_species``: a :class:`WaterSpecies` whose species
    are among them (None: dry -- constant heat capacity, no virtual effect).  ``kbot = min(n_sponge, nz)`` (below 3 the operator
    only zeroes the tendencies), ``t_min`` = 160 K where the model top ``ptop`` is below 2 Pa, else 165 K, ``t_max`` = 315 K where
    ``kbot < min(nz, 24)``, else 325 K.  The work fields (one per tracer, two for ``pt`` and ``w``, three more when a tracer is not
    a water species) are allocated here, once."""

    def __init__(self, stencil_factory, quantity_factory=None, grid_data=None, *, n_sponge, fv_sg_adj, water_species=None, tracers=None, hydrostatic=False, ptop=None):
        import ctypes as C

        from . import lib as _lib

        super().__init__(stencil_factory, quantity_factory, grid_data)
        if not float(fv_sg_adj) > 0.0:
            raise ValueError(f"DryConvectiveAdjustment: fv_sg_adj = {fv_sg_adj} must be a positive time scale in seconds (0 or less turns the adjustment off in the namelist)")
        if hydrostatic or getattr(self.sf.config, "hydrostatic", False):
            raise NotImplementedError("DryConvectiveAdjustment: only the non-hydrostatic form of fv_subgrid_z is built")
        nz = int(self.sf.grids[0].nz)
        self.tau = float(fv_sg_adj)
        self.kbot = min(int(n_sponge), nz)
        self.ptop = float(self.sf.grids[0].ptop if ptop is None else ptop)
        self.t_min = 160.0 if self.ptop < 2.0 else 165.0
        self.t_max = 315.0 if self.kbot < min(nz, 24) else 325.0
        self.water = water_species
        self.tracers = list(tracers.values()) if isinstance(tracers, dict) else list(tracers or [])
        species = [] if water_species is None else [q for q in water_species.species.values() if q is not None]
        n_passive = sum(1 for q in self.tracers if not any(q is w for w in species))
        self.n_work = 2 + len(self.tracers) + (3 if n_passive else 0)
        self.work = [self.qf.zeros(_CELL, "") for _ in range(self.n_work)]
        self._work = (_lib.F * self.n_work)(*[C.pointer(q.field) for q in self.work])
        self._tracers = (_lib.F * max(len(self.tracers), 1))(*[C.pointer(q.field) for q in self.tracers])
        self.params = _lib.fv3_subgridz_params(0.0, self.tau, self.t_min, self.t_max, max(self.kbot, 0))
        self._pref = C.byref(self.params)

    def __call__(self, state, u_dt, v_dt, timestep):
        self.params.dt = float(timestep)
        self.sf.call("subgrid_z", self._pref, None if self.water is None else self.water.cref, len(self.tracers), self._tracers,
                     state.ua.fref, state.va.fref, state.w.fref, state.pt.fref, state.delp.fref, state.delz.fref, state.peln.fref, state.pkz.fref,
                     u_dt.fref, v_dt.fref, self.n_work, self._work)


class ApplyPhysicsToDycore(_Op):
    """Cell-centre tendencies applied to the D-grid state (FV3 ``fv_update_phys``; pyFV3's ``ApplyPhysicsToDycore``): call as the
    reference's ``(state, u_dt, v_dt, pt_dt, dt)`` with ``u_dt``, ``v_dt`` the eastward / northward wind tendencies (m/s^2) and
    ``pt_dt`` the temperature tendency (K/s) on the compute cells.  ``state.pt += dt * pt_dt``: ``pt`` is the temperature in K, so the
    call belongs after ``DynamicalCore.step_dynamics``; the ``cp / cvm`` scaling that turns a heating at constant pressure into the
    tendency of this model's temperature is the caller's.  The wind tendencies go to the D-grid faces the rank updates
    (``update_dwinds_phys``, ``fv3_apply_tendencies`` in include/fv3_mi355x.h holds the form, tile-edge interpolation included); the
    call starts with a one-cell halo update of ``u_dt``, ``v_dt`` -- geographic components, exchanged as two scalars (``comm``: a
    :class:`pace_amd.halo.Layout`, None = every rank in this process).

    Not built, and refused where they can be asked for: tracer tendencies, the moist ``delp`` adjustment, nudging.  ``do_sg_conv``
    (FV3's flag for a convection scheme inside ``fv_update_phys``) is refused too: the dry convective adjustment of ``fv_sg_adj`` is the
    caller's step before this one, :class:`DryConvectiveAdjustment`."""

    def __init__(self, stencil_factory, quantity_factory=None, grid_data=None, comm=None, *, tracer_tendencies=None, nudge=False, do_sg_conv=False):
        from .grid import UPDPHYS_FIELDS

        super().__init__(stencil_factory, quantity_factory, grid_data)
        if tracer_tendencies:
            raise NotImplementedError("ApplyPhysicsToDycore: tracer tendencies (and the delp adjustment that goes with them) are not built")
        if nudge:
            raise NotImplementedError("ApplyPhysicsToDycore: nudging is not built")
        if do_sg_conv:
            raise NotImplementedError("ApplyPhysicsToDycore: do_sg_conv is not built here, the dry convective adjustment (fv_subgridz) is the caller's DryConvectiveAdjustment before this call")
        missing = [n for n in UPDPHYS_FIELDS if n not in self.sf.grids[0].fields]
        if missing:
            raise ValueError(f"ApplyPhysicsToDycore: the grid data lacks {', '.join(missing)} (pace_amd.grid.make_grid forms them)")
        self.comm = comm
        # the metric terms of the context's sub-domains, uploaded once (2-D fields like phis)
        self.metrics = [self.qf.from_array([g.fields[n] for g in self.sf.grids], ("x", "y")) for n in UPDPHYS_FIELDS]
        self._updater = None
        self._bound = None

    def _tendency_updater(self, u_dt, v_dt):
        from .halo import HaloExchanger, Layout
        from .topology import CubedSpherePartitioner

        key = (id(u_dt), id(v_dt))
        if self._bound != key:
            lay = self.comm
            if lay is None:
                cfg = self.sf.config
                lay = Layout(CubedSpherePartitioner(cfg.npx - 1, tuple(cfg.layout)), 1, 0)
            ex = HaloExchanger.shared(self.sf, lay, group=getattr(lay, "group", None))
            self._updater = ex.updater("cell", [(u_dt,), (v_dt,)], n_halo=1)
            self._bound = key
        return self._updater

    def __call__(self, state, u_dt, v_dt, pt_dt, dt):
        self._tendency_updater(u_dt, v_dt).update()
        self.sf.call("apply_tendencies", state.u.fref, state.v.fref, state.pt.fref, u_dt.fref, v_dt.fref, pt_dt.fref, *[m.fref for m in self.metrics], float(dt))


def _box_extent(sf, q: Quantity, op: str):
    """(ni, nj, nk) of the compute box of ``q`` from its dims: ``x_interface`` / ``y_interface`` / ``z_interface`` add one; nk is
    None for a 2-D quantity."""
    s = sf.sizer
    if len(q.dims) < 2 or q.dims[0] not in (X_DIM, X_INTERFACE_DIM) or q.dims[1] not in (Y_DIM, Y_INTERFACE_DIM):
        raise ValueError(f"{op}: dims {q.dims} (the first two must be x | x_interface, y | y_interface)")
    ni = s.nx + (1 if q.dims[0] == X_INTERFACE_DIM else 0)
    nj = s.ny + (1 if q.dims[1] == Y_INTERFACE_DIM else 0)
    if len(q.dims) == 2:
        if not q.is_2d:
            raise ValueError(f"{op}: dims {q.dims} on a 3-D storage")
        return ni, nj, None
    if q.is_2d or q.dims[2] not in (Z_DIM, Z_INTERFACE_DIM):
        raise ValueError(f"{op}: dims {q.dims} (the third must be z | z_interface, on a 3-D storage)")
    return ni, nj, s.nz + (1 if q.dims[2] == Z_INTERFACE_DIM else 0)


def _out_ptr(sf, out, n: int, op: str):
    """Device pointer of the caller's output buffer (a contiguous torch tensor of the context's dtype and device, at least n elements)."""
    if out.dtype != sf.dtype or out.device.type != sf.device.type or not out.is_contiguous():
        raise ValueError(f"{op}: out must be a contiguous {sf.dtype} tensor on {sf.device}")
    if out.numel() < n:
        raise ValueError(f"{op}: out holds {out.numel()} elements, {n} are needed")
    return out.data_ptr()


class FieldPack(_Op):
    """The compute domain of a Quantity, packed on the device into ``out[n_sub, (nk,) nj, ni]`` (i fastest) -- what the driver's
    diagnostics move to the host instead of the padded storage (``fv3_diag_pack``).  The box follows the Quantity's dims
    (``x_interface`` / ``y_interface`` / ``z_interface`` add one); ``level`` packs that single level of a 3-D quantity as a 2-D
    array.  ``out`` is the caller's buffer (a contiguous device tensor with room for the box; nothing is allocated); the
    call returns the view of ``out`` with the packed shape."""

    def shape(self, q: Quantity, level: Optional[int] = None):
        ni, nj, nk = _box_extent(self.sf, q, "FieldPack")
        if nk is None:
            if level is not None:
                raise ValueError("FieldPack: level given for a 2-D quantity")
            return (q.n_sub, nj, ni)
        if level is not None:
            if not 0 <= int(level) < nk:
                raise ValueError(f"FieldPack: level {level} outside [0, {nk}) of dims {q.dims}")
            return (q.n_sub, nj, ni)
        return (q.n_sub, nk, nj, ni)

    def __call__(self, q: Quantity, out, level: Optional[int] = None):
        shape = self.shape(q, level)
        ni, nj = shape[-1], shape[-2]
        k0, nk = (0, shape[1]) if len(shape) == 4 else (int(level or 0), 1)
        n = 1
        for e in shape:
            n *= e
        self.sf.call("diag_pack", q.fref, ni, nj, k0, nk, _out_ptr(self.sf, out, n, "FieldPack"), n)
        return out.view(-1)[:n].view(shape)


class ColumnIntegral(_Op):
    """``rgrav * sum_k q * delp`` on the compute cells (``fv3_diag_column_integral``; the reference driver's
    ``column_integrated_<tracer>`` [REF driver/pace/driver/diagnostics.py:226-249], kg/m**2), into ``out[n_sub, ny, nx]`` of the
    caller's buffer; returns that view."""

    units = "kg/m**2"

    def shape(self, q: Quantity):
        if tuple(q.dims) != _CELL:
            raise NotImplementedError(f"ColumnIntegral: dims {q.dims} (a cell-centre quantity (x, y, z) is expected)")
        return (q.n_sub, self.sf.sizer.ny, self.sf.sizer.nx)

    def __call__(self, q: Quantity, delp: Quantity, out):
        shape = self.shape(q)
        self.shape(delp)
        n = shape[0] * shape[1] * shape[2]
        self.sf.call("diag_column_integral", q.fref, delp.fref, _out_ptr(self.sf, out, n, "ColumnIntegral"), n)
        return out.view(-1)[:n].view(shape)
