"""Driver diagnostics: the state variables, level slices and column integrals the driver stores every ``output_frequency`` steps.

The surface is the reference driver's [REF driver/pace/driver/diagnostics.py]: ``ZSelect``, ``DiagnosticsConfig`` (the yaml's
``diagnostics_config`` block: ``path, output_format, time_chunk_size, names, derived_names, z_select``), ``Diagnostics`` with
``store(time, state)`` / ``store_grid(grids)`` / ``cleanup()``, ``NullDiagnostics`` without a path, ``MonitorDiagnostics`` otherwise.

What differs from the reference, stated:

* The writers (``pace_amd.monitor``) are this build's own: the reference's ``ndsl.monitor`` is not part of its tree, and the on-disk
  layout is described in that module's docstring.
* A variable leaves the device as its compute domain only: ``FieldPack`` / ``ColumnIntegral`` (``fv3_diag_pack`` /
  ``fv3_diag_column_integral``) write it into ONE device staging buffer, one device-to-host copy moves it into ONE pinned host buffer,
  and the monitor consumes that view before the next variable is packed.  Both buffers are allocated at construction, sized for the
  largest requested variable; ``store`` allocates nothing.  (The copy is not overlapped with the next model step.)
* Names are resolved at construction, strictly, like ``restart.load_state``: against ``STATE_NAMES + ["phis"]``, then against the
  harness's tracers; an unknown name is a ``ValueError`` that lists what exists (the reference fails at the first ``store``).
* ``z_select``: a 2-D field raises ``AssertionError`` and a 3-D field whose third dim is not ``"z"`` raises ``ValueError`` -- the
  reference's checks -- and a ``level`` outside ``[0, nz)`` is a ``ValueError``: the reference's raw slice ``data[:, :, level]`` would hand
  back the pad level (or wrap around) without a word.
* ``derived_names``: ``column_integrated_<tracer>`` = ``rgrav * sum_k q * delp`` in kg/m**2; any other derived name gets
  ``warnings.warn`` and is skipped, as in the reference.
"""
from __future__ import annotations

import abc
import dataclasses
import warnings
from typing import Dict, List, Optional

import numpy as np

from .constants import X_DIM, X_INTERFACE_DIM, Y_DIM, Y_INTERFACE_DIM, Z_DIM
from .dyn_core import STATE_NAMES
from .quantity import Quantity

COLUMN_INTEGRATED = "column_integrated_"
GRID_CONSTANTS = {"lat": (X_INTERFACE_DIM, Y_INTERFACE_DIM), "lon": (X_INTERFACE_DIM, Y_INTERFACE_DIM), "lon_agrid": (X_DIM, Y_DIM), "lat_agrid": (X_DIM, Y_DIM)}


class Diagnostics(abc.ABC):
    @abc.abstractmethod
    def store(self, time, state=None):
        ...

    @abc.abstractmethod
    def store_grid(self, grids=None):
        ...

    @abc.abstractmethod
    def cleanup(self):
        ...


class NullDiagnostics(Diagnostics):
    """Diagnostics that do nothing."""

    def store(self, time, state=None):
        pass

    def store_grid(self, grids=None):
        pass

    def cleanup(self):
        pass


@dataclasses.dataclass
class ZSelect:
    """One level of 3-D state variables: the variable ``<name>_z<level>``."""

    level: int
    names: List[str]

    def check(self, name: str, q: Quantity, nz: int):
        assert len(q.dims) > 2, f"z_select: {name} is a 2-D field (dims {q.dims})"
        if q.dims[2] != Z_DIM:
            raise ValueError(f"z_select only works for state variables with dimension (x, y, z).\n {name} has dimension {q.dims}")
        if not 0 <= int(self.level) < nz:
            raise ValueError(f"z_select: level {self.level} of {name} is outside [0, {nz}) (the storage's level {nz} is padding, not data)")
        return f"{name}_z{int(self.level)}"


@dataclasses.dataclass(frozen=True)
class DiagnosticsConfig:
    """
    Attributes:
        path: directory to save diagnostics if given, otherwise no diagnostics will be stored
        output_format: one of "zarr" or "netcdf"; "netcdf" keeps ``time_chunk_size`` records of every variable in host memory and needs
            every tile wholly owned by one process
        time_chunk_size: number of records stored in each netcdf file, only used if output_format is "netcdf"
        names: state variables to save as diagnostics
        derived_names: derived diagnostics to save
        z_select: save a vertical slice of a 3-D state variable
    """

    path: Optional[str] = None
    output_format: str = "zarr"
    time_chunk_size: int = 1
    names: List[str] = dataclasses.field(default_factory=list)
    derived_names: List[str] = dataclasses.field(default_factory=list)
    z_select: List[ZSelect] = dataclasses.field(default_factory=list)

    def __post_init__(self):
        if (len(self.names) > 0 or len(self.derived_names) > 0) and self.path is None:
            raise ValueError("DiagnosticsConfig.path must be given to enable diagnostics")
        if self.output_format not in ["zarr", "netcdf"]:
            raise ValueError(f"output_format must be one of 'zarr' or 'netcdf', got {self.output_format}")

    @classmethod
    def from_dict(cls, block: Optional[dict]) -> "DiagnosticsConfig":
        """The yaml's ``diagnostics_config`` block (None / empty: no diagnostics); ``z_select`` entries are ``{level, names}``."""
        block = dict(block or {})
        known = {f.name for f in dataclasses.fields(cls)}
        unknown = sorted(set(block) - known)
        if unknown:
            raise ValueError(f"diagnostics_config: unknown keys {unknown} (known: {sorted(known)})")
        zs = [z if isinstance(z, ZSelect) else ZSelect(level=int(z["level"]), names=list(z["names"])) for z in (block.pop("z_select", None) or [])]
        for k in ("names", "derived_names"):
            if k in block:
                block[k] = list(block[k] or [])
        return cls(z_select=zs, **block)

    def diagnostics_factory(self, harness, start_time=None) -> Diagnostics:
        """``NullDiagnostics`` without a path; otherwise a ``MonitorDiagnostics`` bound to the harness's state, tracers, layout and
        stencil factory.  Every process of a run calls this (the writers coordinate through the harness's process group)."""
        if self.path is None:
            return NullDiagnostics()
        from .monitor import NetCDFMonitor, ZarrMonitor

        if self.output_format == "zarr":
            monitor = ZarrMonitor(self.path, harness.layout, start_time=start_time)
        else:
            monitor = NetCDFMonitor(self.path, harness.layout, time_chunk_size=self.time_chunk_size, start_time=start_time)
        # a harness that steps through DynamicalCore (temperature=True) also holds the surface pressure its last step diagnosed
        dycore = getattr(harness, "dycore", None)
        extra = {"ps": dycore.ps} if dycore is not None else None
        return MonitorDiagnostics(monitor, self.names, self.derived_names, self.z_select, state=harness.state, tracers=harness.tracers, stencil_factory=harness.sf,
                                  grids=harness.grids, extra=extra)


def diagnostics_factory(harness, config: Optional[DiagnosticsConfig] = None, start_time=None) -> Diagnostics:
    return (config or DiagnosticsConfig()).diagnostics_factory(harness, start_time=start_time)


@dataclasses.dataclass
class _Var:
    name: str  # as written
    source: str  # state attribute or tracer name
    kind: str  # "field" | "level" | "integral"
    level: Optional[int]
    shape: tuple
    dims: tuple
    units: str


class MonitorDiagnostics(Diagnostics):
    """Diagnostics that save to a monitor of ``pace_amd.monitor`` (module docstring: what is packed, copied and checked, and when)."""

    def __init__(self, monitor, names, derived_names, z_select, state=None, tracers=None, stencil_factory=None, grids=None, extra=None):
        import torch

        from .restart import _UNITS
        from .stencils import ColumnIntegral, FieldPack

        if state is None or stencil_factory is None:
            raise ValueError("MonitorDiagnostics: state and stencil_factory are required (DiagnosticsConfig.diagnostics_factory(harness) passes the harness's)")
        self.monitor = monitor
        self.names = list(names)
        self.derived_names = list(derived_names)
        self.z_select = list(z_select)
        self.state = state
        self.tracers = dict(tracers or {})
        self.extra = dict(extra or {})  # fields held beside the state ({"ps": DynamicalCore.ps})
        self.sf = stencil_factory
        self.grids = grids
        self._pack = FieldPack(stencil_factory)
        self._integral = ColumnIntegral(stencil_factory)
        nz = stencil_factory.sizer.nz

        def units(name, q):
            return q.units or _UNITS.get(name, "")

        plan: List[_Var] = []
        for name in self.names:
            q = self._resolve(name, state)
            plan.append(_Var(name, name, "field", None, self._pack.shape(q), tuple(q.dims), units(name, q)))
        for name in self.derived_names:
            if name.startswith(COLUMN_INTEGRATED):
                tracer = name[len(COLUMN_INTEGRATED):]
                q = self._resolve(tracer, state)
                plan.append(_Var(name, tracer, "integral", None, self._integral.shape(q), tuple(q.dims[:2]), ColumnIntegral.units))
            else:
                warnings.warn(f"{name} is not a supported diagnostic variable.")
        for zs in self.z_select:
            for name in zs.names:
                q = self._resolve(name, state)
                out = zs.check(name, q, nz)
                plan.append(_Var(out, name, "level", int(zs.level), self._pack.shape(q, int(zs.level)), tuple(q.dims[:2]), units(name, q)))
        seen = set()
        for v in plan:
            if v.name in seen:
                raise ValueError(f"diagnostics: variable {v.name!r} is requested twice")
            seen.add(v.name)
        self._plan = plan
        n = max([int(np.prod(v.shape)) for v in plan] + [1])
        sf = stencil_factory
        self._dev = torch.empty(n, dtype=sf.dtype, device=sf.device)  # the one device staging buffer
        self._host = torch.empty(n, dtype=sf.dtype, pin_memory=not sf.hostemu)  # the one host buffer (plain memory on the host emulation)

    @property
    def variables(self) -> List[str]:
        return [v.name for v in self._plan]

    def _known(self) -> List[str]:
        return STATE_NAMES + ["phis"] + list(self.tracers) + list(self.extra)

    def _resolve(self, name: str, state) -> Quantity:
        if name in STATE_NAMES or name == "phis":
            return getattr(state, name)
        if name in self.tracers:
            return self.tracers[name]
        if name in self.extra:
            return self.extra[name]
        raise ValueError(f"diagnostics: unknown variable {name!r}; this build's state holds: {', '.join(self._known())}")

    def _stream(self):
        """The stream the operators of the factory run on, as a torch stream (the copy and the wait go there too)."""
        import torch

        sf = self.sf
        if sf.stream is None:
            return torch.cuda.current_stream(sf.device)
        return torch.cuda.ExternalStream(sf.stream, device=sf.device)

    def _variables(self, state):
        import torch

        sf = self.sf
        for v in self._plan:
            q = self._resolve(v.source, state)
            if sf.hostemu:
                packed = self._integral(q, state.delp, self._dev) if v.kind == "integral" else self._pack(q, self._dev, v.level)
                n = packed.numel()
                self._host[:n].copy_(self._dev[:n])
            else:
                s = self._stream()
                with torch.cuda.stream(s):
                    packed = self._integral(q, state.delp, self._dev) if v.kind == "integral" else self._pack(q, self._dev, v.level)
                    n = packed.numel()
                    self._host[:n].copy_(self._dev[:n], non_blocking=True)  # the one device-to-host copy
                s.synchronize()
            yield v.name, self._host[:n].numpy().reshape(v.shape), v.dims, v.units

    def store(self, time, state=None):
        """``time``: datetime, timedelta since the start time, or seconds.  ``state``: default the one bound at construction."""
        self.monitor.store(time, self._variables(state if state is not None else self.state))

    def store_grid(self, grids=None):
        grids = grids if grids is not None else self.grids
        if grids is None:
            raise ValueError("store_grid: no grids (pass the harness's per-sub-domain GridData list)")
        for name in ("lat", "lon", "lon_agrid", "lat_agrid"):
            dims = GRID_CONSTANTS[name]
            arrs = []
            for g in grids:
                h = g.n_halo
                ni = g.nx + (1 if dims[0] == X_INTERFACE_DIM else 0)
                nj = g.ny + (1 if dims[1] == Y_INTERFACE_DIM else 0)
                arrs.append(np.ascontiguousarray(g.fields[name][h : h + ni, h : h + nj].T))
            self.monitor.store_constant(name, np.stack(arrs), dims, "radians")

    def cleanup(self):
        self.monitor.cleanup()
