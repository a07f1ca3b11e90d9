"""Dycore-only driver: runs the acoustic dynamics from a pace driver yaml.

    python -m pace_amd.driver driver/examples/configs/baroclinic_c12.yaml [--steps N] [--out perf.json]

It reproduces the reference's time loop for ``dycore_only: true`` + ``disable_step_physics: true``
[REF driver/pace/driver/driver.py:627-662]: one timer entry per model step, a step being ``k_split`` x
[AcousticDynamics (+ tracer advection with ``--tracers N``, + the vertical remap with ``--remap``, +
the vertical filling of negative tracer values at the end of the remap with ``dycore_config.fill: true`` or ``--fill on``)] -- with
``--temperature`` (needs ``--remap``) the step is ``DynamicalCore.step_dynamics``: ``pt`` is a temperature in K before and after it,
``omga`` and ``ps`` are diagnosed, and the start-up line and the json ``setup`` say ``"pt": "temperature"`` (otherwise ``"loop"``); with ``--moist``
(needs ``--temperature --remap`` and ``nwat: 6``) the first six tracers are the water species, ``q_con`` and ``cappa`` follow them through
``moist_cv`` and the start-up line and the json say ``"thermodynamics": "moist_cv"`` (otherwise ``"given"``); with ``--neg-adj`` (needs
``--moist``) FV3's ``neg_adj3`` fixes negative water species after the conversion back to temperature and the start-up line and the json
say ``"neg_adj": true`` (otherwise ``false``); with ``--moist`` and ``do_sat_adj: true`` in the yaml (or ``--sat-adj on``; ``--sat-adj off``
overrides the yaml) FV3's saturation adjustment runs inside every remap with the yaml's ``tau_*`` / ``ql_gen`` ... keys
(``pace_amd.stencils.SatAdjustConfig``) and the start-up line and the json say ``"sat_adj": true`` (otherwise ``false``); with ``--held-suarez``
(needs ``--temperature --remap --latlon-winds``) every step ends with the Held-Suarez forcing and ``ApplyPhysicsToDycore`` and the start-up line and
the json say ``"forcing": "held_suarez"`` (otherwise ``"none"``); with ``fv_sg_adj`` above 0 in the yaml's ``dycore_config`` (``--dry-adjust yaml``, the default; ``on`` / ``off`` override
the yaml; needs ``--temperature --remap --latlon-winds``, and with ``yaml`` the driver says in one line that the key is ignored where they are absent) every step
ends with the dry convective adjustment of the sponge layers (``DryConvectiveAdjustment``, FV3's ``fv_subgrid_z``) and ``ApplyPhysicsToDycore``, and the start-up line and
the json say ``"dry_convective_adjustment": true`` (otherwise ``false``) -- and writes
the per-step times in the layout the reference's performance collector uses
(``{"times": {<timer>: {"hits": n, "times": [[...per step...] per rank]}}}``, timers ``mainloop``, ``DynCore``,
``TracerAdvection``, ``Remapping`` [REF tests/main/driver/test_driver.py:77-121]).  With ``--tracers N --remap`` the step is the
body of ``DynamicalCore.step_dynamics`` and the outer timer is called ``mainloop``:
[REF .jenkins/print_performance_number.py:13-14] (mean of steps 2..N per rank) then runs on the file unchanged.  Without them
the outer timer is ``acoustic_mainloop`` (it times less than the reference's ``mainloop`` does).
The number of steps comes from ``seconds`` / ``minutes`` / ``hours`` / ``days`` and ``dt_atmos`` as in
the reference [REF driver/pace/driver/driver.py:305-337 (total_time / n_steps)].

Keys read from the yaml: ``nx_tile, nz, layout, dt_atmos, seconds|minutes|hours|days,
grid_config`` (``type: generated`` with ``config.{stretch_factor, lon_target, lat_target}``: a factor other than 1 runs on the
Schmidt-transformed grid with ``stretched_grid`` set, and the start-up line and the json ``setup`` say ``"grid": {"stretch_factor": ..,
"lon_target": .., "lat_target": ..}``, otherwise ``"grid": "uniform"``; another ``type`` or ``grid_type != 0`` is refused),
``dycore_config.*`` (the fields of ``AcousticDynamicsConfig``), ``stencil_config.compilation_config.
{backend, device_sync}``, ``initialization.type`` (``analytic``/anything else -> the synthetic
recipe of SURVEY §8d; the analytic baroclinic state is not part of this build and the driver says
so).  ``backend`` values other than ``hip:gfx950`` are reported and replaced: this build has one
backend.  Multi-process runs take RANK / WORLD_SIZE / LOCAL_RANK from the environment like bench.py.

Diagnostics [REF driver/pace/driver/driver.py:551-552, 588-611, 702-705]: with a ``diagnostics_config`` block in the yaml
(``pace_amd.diagnostics.DiagnosticsConfig``) the driver stores the initial state when ``output_initial_state`` is set, stores after
every ``output_frequency``-th step -- outside the step clock -- and ends with ``store_grid`` and ``cleanup``.  Names of the block that
this build's state does not hold (``qvapor`` ... ``qgraupel``, ``ps``: the reference's yamls ask for them) are dropped and reported in
one line; with ``--moist`` the six species are tracers of the step and are stored; with ``--temperature`` ``ps`` is known and stored from ``DynamicalCore.ps``.  ``--diagnostics-path DIR`` overrides the block's ``path``, ``--no-diagnostics`` turns the block off.  Without a block
nothing changes.
"""
from __future__ import annotations

import argparse
import dataclasses
import json
import os
import sys

import yaml


def _sat_adj_keys():
    from .constants import SAT_ADJ_DEFAULTS

    return ("do_sat_adj",) + tuple(SAT_ADJ_DEFAULTS)


SAT_ADJ_KEYS = _sat_adj_keys()


def resolve_sat_adj(option: str, sat_block: dict, moist: bool) -> bool:
    """Whether every remap of the step runs the saturation adjustment: the yaml's ``dycore_config.do_sat_adj`` (absent = false) unless
    ``--sat-adj on|off`` overrides it; it works on the six water species of ``--moist`` and is off without it."""
    if option not in ("yaml", "on", "off"):
        raise ValueError(f"--sat-adj {option!r}: yaml, on or off")
    want = bool(sat_block.get("do_sat_adj", False)) if option == "yaml" else option == "on"
    return bool(want and moist)


def read_grid_config(block) -> dict:
    """The yaml's ``grid_config`` block [REF driver/pace/driver/grid.py:94-96, 288-319] -> ``{"stretch_factor", "lon_target",
    "lat_target"}`` (the reference's defaults where a key is absent; factor 1 = the uniform grid).  This build generates its grids:
    any other ``type``, and a ``grid_type`` other than 0, is refused instead of being ignored."""
    block = block or {}
    kind = block.get("type", "generated")
    if kind != "generated":
        raise ValueError(f"grid_config.type: {kind!r} is not available in this build: it generates its grids (type: generated) and reads none.")
    cfg = block.get("config") or {}
    if int(cfg.get("grid_type", 0) or 0) != 0:
        raise ValueError(f"grid_config.config.grid_type: {cfg['grid_type']} is not available in this build: the grid is the cubed sphere (grid_type: 0), uniform or stretched.")
    return {"stretch_factor": float(cfg.get("stretch_factor", 1.0)), "lon_target": float(cfg.get("lon_target", 350.0)), "lat_target": float(cfg.get("lat_target", -90.0))}


def grid_entry(grid: dict):
    """What the start-up line and the json say about the grid: the three numbers of a stretched grid, or ``"uniform"``."""
    return dict(grid) if float(grid["stretch_factor"]) != 1.0 else "uniform"


def harness_grid_kwargs(grid: dict) -> dict:
    """The ``DycoreHarness`` keywords of the yaml's grid: none for the uniform grid; the harness sets the config's ``stretched_grid`` with them."""
    return dict(grid) if float(grid["stretch_factor"]) != 1.0 else {}


def load_config(path: str):
    with open(path) as f:
        y = yaml.safe_load(f)
    from .config import AcousticDynamicsConfig

    known = {f.name for f in dataclasses.fields(AcousticDynamicsConfig)}
    dy = {k: v for k, v in (y.get("dycore_config") or {}).items() if k in known}
    ignored = sorted(k for k in (y.get("dycore_config") or {}) if k not in known)
    total = 0.0
    for key, mult in (("seconds", 1.0), ("minutes", 60.0), ("hours", 3600.0), ("days", 86400.0)):
        total += float(y.get(key, 0) or 0) * mult
    dt_atmos = float(y["dt_atmos"])
    run = dict(
        nwat=(y.get("dycore_config") or {}).get("nwat", None),
        # the saturation adjustment: do_sat_adj and the keys of SatAdjustConfig as the yaml has them (read with --moist only)
        sat_adj={k: v for k, v in (y.get("dycore_config") or {}).items() if k in SAT_ADJ_KEYS},
        nx_tile=int(y["nx_tile"]),
        nz=int(y["nz"]),
        layout=tuple(int(v) for v in y.get("layout", (1, 1))),
        dt_atmos=dt_atmos,
        n_steps=max(1, int(round(total / dt_atmos))) if total > 0 else 1,
        backend=((y.get("stencil_config") or {}).get("compilation_config") or {}).get("backend", "hip:gfx950"),
        device_sync=bool(((y.get("stencil_config") or {}).get("compilation_config") or {}).get("device_sync", False)),
        init=(y.get("initialization") or {}).get("type", "analytic"),
        case=(((y.get("initialization") or {}).get("config") or {}).get("case", "baroclinic")),
        dycore_only=bool(y.get("dycore_only", False)),
        disable_step_physics=bool(y.get("disable_step_physics", False)),
        experiment=((y.get("performance_config") or {}).get("experiment_name", os.path.splitext(os.path.basename(path))[0])),
        # diagnostics [REF driver/pace/driver/driver.py:88-93, 132-133; initialization.config.start_time, default 2000-01-01]
        diagnostics_config=y.get("diagnostics_config") or None,
        output_initial_state=bool(y.get("output_initial_state", False)),
        output_frequency=int(y.get("output_frequency", 1)),
        start_time=(((y.get("initialization") or {}).get("config") or {}).get("start_time", None)),
        grid=read_grid_config(y.get("grid_config")),
    )
    return run, dy, ignored


def filter_diagnostics(block, known):
    """The yaml's ``diagnostics_config`` block without the names this build's state does not hold (``known``: state fields + tracers):
    (block, dropped names).  ``column_integrated_<tracer>`` is dropped with its tracer; other derived names are left to the diagnostics
    (they warn, like the reference's)."""
    from .diagnostics import COLUMN_INTEGRATED

    block = dict(block or {})
    known = set(known)
    dropped = []

    def keep(names, is_known=lambda n: n in known):
        out = []
        for n in names or []:
            (out if is_known(n) else dropped).append(n)
        return out

    if "names" in block:
        block["names"] = keep(block["names"])
    if "derived_names" in block:
        block["derived_names"] = keep(block["derived_names"], lambda n: not n.startswith(COLUMN_INTEGRATED) or n[len(COLUMN_INTEGRATED):] in known)
    if "z_select" in block:
        zs = []
        for z in block["z_select"] or []:
            names = keep(z["names"])
            if names:
                zs.append({"level": z["level"], "names": names})
        block["z_select"] = zs
    return block, dropped


DRY_ADJUST_NEEDS = "--temperature --remap --latlon-winds: fv_subgrid_z reads the temperature and the eastward / northward winds of the step's end state"


def resolve_dry_adjust(option: str, dycore_config: dict, prerequisites: bool):
    """Whether every step ends with the dry convective adjustment: the yaml's ``dycore_config.fv_sg_adj > 0`` (absent = 0 = off) unless
    ``--dry-adjust on|off`` overrides it -> (on, ignored): ``ignored`` when the yaml asks for it and ``--temperature --remap
    --latlon-winds`` are not all given (the driver says so and goes on); ``on`` without them is refused by the caller."""
    if option not in ("yaml", "on", "off"):
        raise ValueError(f"--dry-adjust {option!r}: yaml, on or off")
    asked = int(dycore_config.get("fv_sg_adj", 0) or 0) > 0
    want = asked if option == "yaml" else option == "on"
    return bool(want and prerequisites), bool(option == "yaml" and asked and not prerequisites)


def resolve_fill(option: str, dycore_config: dict, tracers: int, remap: bool) -> bool:
    """Whether the step fills negative tracer values in the vertical (``fillz`` at the end of the remap): the yaml's
    ``dycore_config.fill`` (absent = false, FV3's namelist default) unless ``--fill on|off`` overrides it; without ``--remap`` or
    without tracers there is nothing to fill and the key is ignored."""
    if option not in ("yaml", "on", "off"):
        raise ValueError(f"--fill {option!r}: yaml, on or off")
    want = bool(dycore_config.get("fill", False)) if option == "yaml" else option == "on"
    return bool(want and tracers and remap)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("config")
    ap.add_argument("--steps", type=int, default=None, help="override the number of model steps from the yaml")
    ap.add_argument("--out", default=None, help="performance json (default: <experiment>_fv3_mi355x.json)")
    ap.add_argument("--precision", type=int, default=64)
    ap.add_argument("--restart", default=None, help="start from restart_dycore_state_<rank>.nc files in this directory [REF driver/pace/driver/state.py:154-172]")
    ap.add_argument("--save-restart", default=None, help="write restart_dycore_state_<rank>.nc files there after the last step [REF state.py:114-123]")
    ap.add_argument("--tracers", type=int, default=0, help="advect N synthetic tracers after every acoustic call (TracerAdvection, hord_tr from the yaml)")
    ap.add_argument("--remap", action="store_true", help="Lagrangian-to-Eulerian remap after every acoustic call (with --tracers: the body of DynamicalCore.step_dynamics)")
    ap.add_argument("--fill", choices=("yaml", "on", "off"), default="yaml",
                    help="fill negative tracer values in the vertical at the end of the remap (needs --tracers N --remap): yaml = dycore_config.fill (absent: off); on / off override it")
    ap.add_argument("--latlon-winds", action="store_true",
                    help="CubedToLatLon at the end of every step (c2l_ord from the yaml, default 4): state ua / va become the eastward / northward cell-centre winds")
    ap.add_argument("--temperature", action="store_true",
                    help="step through DynamicalCore.step_dynamics (needs --remap): state pt is a temperature in K before and after every step, omga = delp / delz * w and ps are diagnosed")
    ap.add_argument("--moist", action="store_true",
                    help="derive q_con and cappa from six water species with moist_cv in the preamble and in every remap (needs --temperature --remap and nwat: 6 in the yaml; "
                         "the first six tracers are qvapor, qliquid, qice, qrain, qsnow, qgraupel and --tracers is raised to at least 6)")
    ap.add_argument("--neg-adj", action="store_true",
                    help="neg_adj3 at the end of the thermodynamic part of every step (needs --moist): negative condensate is paid for out of another phase with the latent heat "
                         "booked on the temperature, negative vapour is repaid from the layer below")
    ap.add_argument("--sat-adj", choices=("yaml", "on", "off"), default="yaml",
                    help="saturation adjustment (FV3 fv_sat_adj) inside every remap (needs --moist): yaml = dycore_config.do_sat_adj (absent: off) with the yaml's tau_* / ql_gen ... keys; "
                         "on / off override it")
    ap.add_argument("--held-suarez", action="store_true",
                    help="end every step with the Held-Suarez (1994) forcing and ApplyPhysicsToDycore (needs --temperature --remap --latlon-winds): Newtonian relaxation of the "
                         "temperature and Rayleigh friction on the low-level winds, applied to the D-grid state with dt_atmos")
    ap.add_argument("--dry-adjust", choices=("yaml", "on", "off"), default="yaml",
                    help="end every step with the dry convective adjustment of the sponge layers (FV3 fv_subgrid_z) and ApplyPhysicsToDycore (needs --temperature --remap --latlon-winds): "
                         "yaml = dycore_config.fv_sg_adj > 0 (absent: off), the key being the relaxation time in seconds; on / off override it")
    ap.add_argument("--diagnostics-path", default=None, help="directory of the diagnostics (overrides diagnostics_config.path of the yaml)")
    ap.add_argument("--no-diagnostics", action="store_true", help="ignore the yaml's diagnostics_config block")
    a = ap.parse_args(argv)
    if a.temperature and not a.remap:
        sys.exit("--temperature needs --remap: the conversion back to temperature is the last step of the remap")
    if a.moist and not (a.temperature and a.remap):
        sys.exit("--moist needs --temperature --remap: moist_cv sits in the preamble and the remap of DynamicalCore.step_dynamics")
    if a.held_suarez and not (a.temperature and a.remap and a.latlon_winds):
        sys.exit("--held-suarez needs --temperature --remap --latlon-winds: the forcing reads the temperature and the eastward / northward winds of the step's end state")
    dry_prerequisites = bool(a.temperature and a.remap and a.latlon_winds)
    if a.dry_adjust == "on" and not dry_prerequisites:
        sys.exit("--dry-adjust on needs " + DRY_ADJUST_NEEDS)
    if a.neg_adj and not a.moist:
        sys.exit("--neg-adj needs --moist: neg_adj3 works on the six water species of the moist step")
    if a.sat_adj == "on" and not a.moist:
        sys.exit("--sat-adj on needs --moist: the saturation adjustment works on the six water species of the moist step")
    try:
        run, dy, ignored = load_config(a.config)
    except ValueError as e:
        sys.exit(str(e))
    if a.moist:
        if run["nwat"] is None or int(run["nwat"]) != 6:
            sys.exit(f"--moist needs dycore_config.nwat: 6 in the yaml (it has nwat: {run['nwat']}): moist_cv is built for the six-species formula only")
        a.tracers = max(a.tracers, 6)
        ignored = [k for k in ignored if k != "nwat" and k not in SAT_ADJ_KEYS]  # (read here; without --moist they stay in the list of keys not read)
    sat_adj = resolve_sat_adj(a.sat_adj, run["sat_adj"], a.moist)
    sat_cfg = None
    if sat_adj:
        from .stencils import SatAdjustConfig

        sat_cfg = SatAdjustConfig(**{k: float(v) for k, v in run["sat_adj"].items() if k != "do_sat_adj"})

    dry_adjust, dry_ignored = resolve_dry_adjust(a.dry_adjust, dy, dry_prerequisites)
    if dry_adjust and a.held_suarez:
        sys.exit("--held-suarez and the dry convective adjustment exclude each other: both assign the wind tendencies that ApplyPhysicsToDycore applies (--dry-adjust off turns the yaml's fv_sg_adj off)")
    if dry_adjust and int(dy.get("fv_sg_adj", 0) or 0) <= 0:
        sys.exit("--dry-adjust on needs dycore_config.fv_sg_adj > 0 in the yaml: the key is the relaxation time of the adjustment in seconds")

    import torch

    from .harness import DycoreHarness

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    say = (lambda *x: print("[driver]", *x, flush=True)) if rank == 0 else (lambda *x: None)
    if run["backend"] not in ("hip:gfx950", "hip"):
        say(f"backend {run['backend']!r} requested by the yaml -> running 'hip:gfx950' (the only backend of this build)")
    if not (run["dycore_only"] and run["disable_step_physics"]):
        say("physics is outside this build: running the dycore-only loop")
    fill = resolve_fill(a.fill, dy, a.tracers, a.remap)
    pt_form = "temperature" if a.temperature else "loop"
    say("step = k_split x [acoustic dynamics" + (f", advection of {a.tracers} tracers" if a.tracers else "") + (", vertical remap" if a.remap else "") + (" + fillz" if fill else "") + "]" + (", then CubedToLatLon" if a.latlon_winds else "")
        + ("" if (a.tracers and a.remap) else "  (--tracers N --remap add the rest of step_dynamics)"))
    say(f'"fill": {str(fill).lower()}' + ("" if a.fill == "yaml" else f" (--fill {a.fill})")
        + ("  (ignored without --tracers N --remap)" if (not fill and (a.fill == "on" or (a.fill == "yaml" and dy.get("fill")))) else ""))
    say(f'"pt": "{pt_form}"' + ("  (DynamicalCore.step_dynamics: temperature in K in and out, omga and ps diagnosed)" if a.temperature else "  (the acoustic loop's T_v / pkz; --temperature --remap: temperature in K)"))
    thermo = "moist_cv" if a.moist else "given"
    say(f'"thermodynamics": "{thermo}"' + ("  (q_con and cappa from qvapor, qliquid, qice, qrain, qsnow, qgraupel in the preamble and in every remap)" if a.moist
                                         else "  (q_con and cappa are the state's fields as initialised; --moist --temperature --remap: moist_cv of six water species)"))
    say(f'"neg_adj": {str(bool(a.neg_adj)).lower()}' + ("  (neg_adj3 on the temperature and the six water species after the last remap of every step)" if a.neg_adj
                                                         else "  (negative water species stay as the remap leaves them; --moist --neg-adj: neg_adj3)"))
    say(f'"sat_adj": {str(sat_adj).lower()}' + ("" if a.sat_adj == "yaml" else f" (--sat-adj {a.sat_adj})")
        + ("  (fv_sat_adj on the six water species inside every remap, between the fill and moist_cv)" if sat_adj
           else "  (no phase changes; --moist with do_sat_adj: true in the yaml or --sat-adj on: fv_sat_adj inside every remap)"))
    forcing = "held_suarez" if a.held_suarez else "none"
    say(f'"forcing": "{forcing}"' + ("  (Held-Suarez tendencies from the step's end state, applied to u, v, pt by ApplyPhysicsToDycore with dt_atmos)" if a.held_suarez
                                     else "  (an unforced initial-value problem; --held-suarez with --temperature --remap --latlon-winds: Held-Suarez forcing)"))
    say(f'"dry_convective_adjustment": {str(dry_adjust).lower()}' + ("" if a.dry_adjust == "yaml" else f" (--dry-adjust {a.dry_adjust})")
        + (f"  (fv_subgrid_z on the top {min(int(dy.get('n_sponge', 48)), run['nz'])} levels with fv_sg_adj = {int(dy.get('fv_sg_adj', 0))} s after every step_dynamics, its wind tendencies applied by ApplyPhysicsToDycore)" if dry_adjust
           else (f"  (fv_sg_adj: {dy.get('fv_sg_adj')} of the yaml is ignored without " + DRY_ADJUST_NEEDS.split(":")[0] + ")" if dry_ignored
                 else "  (no convective adjustment; fv_sg_adj > 0 in the yaml with --temperature --remap --latlon-winds: fv_subgrid_z on the sponge layers)")))
    say(f'"grid": {json.dumps(grid_entry(run["grid"]))}' + ("  (Schmidt transform of the generated corner positions; divergence damping in its stretched form)" if grid_entry(run["grid"]) != "uniform"
                                                            else "  (grid_config.config.stretch_factor / lon_target / lat_target: a grid refined about a target point)"))
    if run["init"] == "analytic" and str(run["case"]).startswith("baroclinic"):
        init = "baroclinic"
        say("initialization: JW2006 baroclinic wave (pace_amd.init.baroclinic_state; restated from the paper, see its docstring)")
    else:
        init = "synthetic"
        say(f"initialization {run['init']!r}/{run['case']!r} is not available in this build: using the synthetic recipe of SURVEY §8d")
    if ignored:
        say("dycore_config keys not read by the acoustic path:", ", ".join(ignored))
    if world > 1:
        import torch.distributed as dist

        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        torch.cuda.set_device(local_rank)
        dist.init_process_group("nccl", device_id=torch.device(f"cuda:{local_rank}"))
    n_ranks = 6 * run["layout"][0] * run["layout"][1]
    if n_ranks % world:
        sys.exit(f"{n_ranks} sub-domains are not divisible over {world} processes")
    dtype = torch.float64 if a.precision == 64 else torch.float32
    kw = {k: dy[k] for k in ("k_split", "n_split") if k in dy}
    h = DycoreHarness(nx_tile=run["nx_tile"], nz=run["nz"], layout=run["layout"], dt_atmos=run["dt_atmos"], world_size=world, proc=rank,
                      device=f"cuda:{local_rank}", dtype=dtype, verbose=(rank == 0), init=init, config_overrides={k: v for k, v in dy.items() if k not in ("k_split", "n_split", "fill")},
                      n_tracers=a.tracers, hord_tr=int(dy.get("hord_tr", 8)), remap=a.remap, fill=fill, latlon_winds=a.latlon_winds, temperature=a.temperature, moist=a.moist, neg_adj=a.neg_adj, sat_adj=sat_adj, sat_adjust_config=sat_cfg, held_suarez=a.held_suarez, dry_convective_adjustment=dry_adjust, **harness_grid_kwargs(run["grid"]), **kw)
    if run["device_sync"]:
        h.sf.set_device_sync(True)
    if a.restart:
        from . import restart

        try:
            restart.check_pt_form(h.layout.local_ranks, a.restart, a.temperature)
            restart.check_grid(h.layout.local_ranks, a.restart, h.stretch)
        except ValueError as e:
            sys.exit(f"--restart: {e}")
        restart.load_state(h.state, h.layout.local_ranks, a.restart, extra=h.tracers)
        h.dyn._bind(h.state)
        say(f"state loaded from {a.restart}")
    n_steps = a.steps or run["n_steps"]
    # diagnostics: built after the harness (the reference's order), bound to its state, tracers, layout and stencil factory
    from .diagnostics import DiagnosticsConfig, NullDiagnostics
    from .dyn_core import STATE_NAMES

    diagnostics = NullDiagnostics()
    if run["diagnostics_config"] and not a.no_diagnostics:
        block, dropped = filter_diagnostics(run["diagnostics_config"], STATE_NAMES + ["phis"] + list(h.tracers) + (["ps"] if a.temperature else []))
        if a.diagnostics_path:
            block["path"] = a.diagnostics_path
        if dropped:
            say("diagnostics: this build's state does not hold " + ", ".join(dropped) + " -- dropped from the output")
        dcfg = DiagnosticsConfig.from_dict(block)
        diagnostics = dcfg.diagnostics_factory(h, start_time=run["start_time"])
        if dcfg.path is not None:
            say(f"diagnostics: {dcfg.output_format} -> {dcfg.path}: {', '.join(diagnostics.variables)}; every {run['output_frequency']} step(s)"
                + (", initial state included" if run["output_initial_state"] else ""))
    from datetime import timedelta

    from .monitor import as_datetime

    start_time = as_datetime(run["start_time"])
    if run["output_initial_state"]:
        diagnostics.store(start_time)
    from .timer import Timer

    # The reference's timestep timer: one "mainloop" entry per model step [REF driver/pace/driver/driver.py:640], and inside it the
    # dycore's own clocks ("DynCore" = the acoustic dynamics, "TracerAdvection", "Remapping"), collected per step like its
    # performance collector does (times_per_step / hits_per_step [REF tests/main/driver/test_driver.py:77-121]).  When the step is
    # not the whole body of step_dynamics (no --tracers / --remap) the outer clock is called "acoustic_mainloop" instead, so that
    # nobody compares it with the reference's "mainloop".
    full_step = bool(a.tracers and a.remap)
    loop_name = "mainloop" if full_step else ("acoustic_mainloop" if not (a.tracers or a.remap) else "dynamics_mainloop")
    # (device synchronisation on the OUTER clock only: a synchronising nested clock would serialise the streams inside the timed step -- the nested
    #  dycore clocks then measure host-side enqueue intervals, and the json says so)
    timer = Timer(sync=h.synchronize, sync_names=(loop_name,))
    times_per_step, hits_per_step = [], []
    for step in range(n_steps):
        timer.reset()
        with timer.clock(loop_name):
            h.step(timer)  # dycore.step_dynamics for dycore_only + disable_step_physics
        times_per_step.append(timer.times)
        hits_per_step.append(timer.hits)
        if (step + 1) % run["output_frequency"] == 0:  # (outside the step clock)
            diagnostics.store(start_time + timedelta(seconds=(step + 1) * run["dt_atmos"]))
    times = [t[loop_name] for t in times_per_step]
    ok = all(v[2] for v in h.sanity().values())
    diagnostics.store_grid(h.grids)
    diagnostics.cleanup()
    if a.save_restart:
        from . import restart

        restart.save_state(h.state, h.layout.local_ranks, a.save_restart, extra=h.tracers, stretch=h.stretch, **({"pt_form": restart.PT_TEMPERATURE} if a.temperature else {}))
        say(f"restart files written to {a.save_restart}")
    # per reference rank (the ranks a process owns step together: they share its clocks)
    local = {r: {n: [t.get(n, 0.0) for t in times_per_step] for n in times_per_step[0]} for r in h.layout.local_ranks}
    hits = {n: sum(hh.get(n, 0) for hh in hits_per_step) for n in hits_per_step[0]}
    if world > 1:
        import torch.distributed as dist

        gathered = [None] * world
        dist.all_gather_object(gathered, local)
        local = {}
        for g in gathered:
            local.update(g)
        dist.destroy_process_group()
    if rank == 0:
        names = list(local[min(local)])
        report = {n: {"hits": hits[n], "times": [local[r][n] for r in sorted(local)]} for n in names}  # TimeReport(hits, times[rank][step])
        per_rank = report[loop_name]["times"]
        mean = sum(per_rank[0][1:]) / max(1, len(per_rank[0]) - 1) if n_steps > 1 else per_rank[0][0]
        sdpd = run["dt_atmos"] / mean
        out = a.out or f"{run['experiment']}_fv3_mi355x.json"
        json.dump({"setup": {"experiment": run["experiment"], "nx_tile": run["nx_tile"], "nz": run["nz"], "layout": list(run["layout"]), "dt_atmos": run["dt_atmos"],
                             "k_split": h.cfg.k_split, "n_split": h.cfg.n_split, "n_gpus": world, "backend": "hip:gfx950", "dycore_only": True, "acoustic_only": not (a.tracers or a.remap), "tracers": a.tracers, "remap": bool(a.remap), "fill": fill, "pt": pt_form, "thermodynamics": thermo, "neg_adj": bool(a.neg_adj), "sat_adj": sat_adj, "forcing": forcing, "dry_convective_adjustment": dry_adjust, "grid": grid_entry(run["grid"]), "finite": ok,
                             "note": ("a step here is k_split AcousticDynamics calls; the reference's dycore_only mainloop (DynamicalCore.step_dynamics) also runs tracer "
                                      "advection and the Lagrangian-to-Eulerian remap (--tracers N --remap add them): not comparable with the reference's 'mainloop' timer")
                             if not (a.tracers and a.remap) else
                             "a step is k_split x [AcousticDynamics, tracer advection, vertical remap] = the body of DynamicalCore.step_dynamics without physics and "
                             + ((("the energy fixer (fv_sat_adj runs inside every remap; q_con and cappa follow" if sat_adj else "the saturation adjustment (q_con and cappa follow") + " the six water species: moist_cv" + ("; neg_adj3 fixes negative species)" if a.neg_adj else "; neg_adj3 is left out: --neg-adj)"))
                                if a.moist else "moist thermodynamics")},
                   # the reference collector's layout: times.<timer> = {hits, times[rank][step]}; "mainloop" only when the step is the
                   # whole body of step_dynamics (--tracers N --remap), then .jenkins/print_performance_number.py runs on this file as is
                   "times": report,
                   "times_note": ("only the outer clock ('" + loop_name + "') synchronises the device; the nested clocks (DynCore / TracerAdvection / Remapping) are host-side "
                                  "enqueue intervals. " + (("'mainloop' here = the body of step_dynamics with moist_cv of six water species" + (" and neg_adj3" if a.neg_adj else "") + (" and fv_sat_adj inside every remap: " if sat_adj else ": no saturation adjustment, ") + ("" if a.neg_adj else "no neg_adj3, ") + "no physics coupling "
                                                            "-- the reference's mainloop does more per step." if a.moist else
                                                            "'mainloop' here = the dry body of step_dynamics with N synthetic tracers: no moist thermodynamics, no physics coupling "
                                                            "-- the reference's mainloop does more per step.") if full_step else "")),
                   ("acoustic_simulated_days_per_day" if not (a.tracers or a.remap) else "dynamics_simulated_days_per_day"): sdpd}, open(out, "w"))
        say(f"{n_steps} steps of dt_atmos={run['dt_atmos']:g}s: acoustic mainloop mean (first step dropped) {mean * 1e3:.2f} ms -> {sdpd:.2f} simulated-days/day ({'acoustic dynamics only' if not (a.tracers or a.remap) else 'acoustic dynamics' + (f' + {a.tracers} tracers' if a.tracers else '') + (' + remap' if a.remap else '')}); state finite: {ok}; wrote {out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
