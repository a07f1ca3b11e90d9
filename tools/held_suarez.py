#!/usr/bin/env python3
"""The Held-Suarez (1994) dry climate test run forward from rest: DynamicalCore.step_dynamics followed by the Held-Suarez forcing and
ApplyPhysicsToDycore every step (``DycoreHarness(held_suarez=True)``) [Held & Suarez, Bull. Amer. Meteor. Soc. 75 (1994) 1825-1830].

The start is a resting, isothermal (300 K), hydrostatic atmosphere over a flat surface with ps = 1000 hPa and a small seeded temperature
perturbation that breaks the zonal symmetry.  The forcing cools the poles and the upper levels towards the paper's equilibrium; within
some tens of days the thermal wind spins up westerly jets, baroclinic eddies set in after that, and the statistics of the paper's figures
(jets of about 30 m/s near 45 degrees and 250 hPa, surface easterlies in the tropics, a 200 K stratosphere) are those of days 200 - 1200.
The run prints, every ``--every`` hours, the zonal means of the eastward wind ``ua`` and the temperature at a few latitudes and levels,
the extremes of the surface pressure and whether the state is finite.  A tool, not a test: the tests hold the operators to the paper
(tests/test_held_suarez.py) and to the geometry (tests/test_apply_tendencies.py).

    python tools/held_suarez.py --nx 48 --days 30 --out held_suarez.json
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from pace_amd.harness import DycoreHarness  # noqa: E402

# (dt_atmos, k_split, n_split) per resolution, as tools/jw_wave.py
STEPPING = {12: (3600.0, 2, 6), 24: (3600.0, 2, 6), 48: (1800.0, 2, 6), 96: (900.0, 2, 6), 192: (450.0, 2, 6)}
LATITUDES = (-60.0, -45.0, -15.0, 0.0, 15.0, 45.0, 60.0)
PRESSURES = (250.0e2, 500.0e2, 850.0e2, 975.0e2)
T0 = 300.0


def rest_state(h, seed=1994, amplitude=0.1):
    """Overwrite the harness's state with the resting isothermal atmosphere: ps = 1e5 Pa (delp, pe, peln, pk are level-only and stay as the
    JW2006 start left them, which has the same ps), T = T0 + amplitude * noise, hydrostatic delz, no wind, no topography."""
    c, s = h.c, h.state
    g0 = h.grids[0]
    nz = h.cfg.npz
    pe = g0.ak + g0.bk * 1.0e5
    delp = pe[1:] - pe[:-1]
    pm = delp / np.log(pe[1:] / pe[:-1])
    for i, (g, r) in enumerate(zip(h.grids, h.layout.local_ranks)):
        shape = (g.nx + 2 * g.n_halo + 1, g.ny + 2 * g.n_halo + 1, nz + 1)
        rng = np.random.default_rng(seed + r)
        t = np.full(shape, T0) + amplitude * rng.standard_normal(shape)
        delz = np.zeros(shape)
        delz[:, :, :nz] = -c.RDGAS * t[:, :, :nz] * delp / (c.GRAV * pm)
        delz[:, :, nz] = delz[:, :, nz - 1]
        zero = np.zeros(shape)
        for name, a in (("pt", t), ("delz", delz), ("u", zero), ("v", zero), ("w", zero), ("ua", zero), ("va", zero)):
            getattr(s, name).set_numpy(a, i)
        s.phis.set_numpy(np.zeros(shape[:2]), i)
    h.dyn._bind(s)  # (the surface height the acoustic dynamics holds follows phis)
    return pe


def zonal_means(h, pe):
    """{"ua": [lat][level], "t": ...}: area-weighted means over the compute cells within 5 degrees of each latitude, at the model level whose
    reference pressure is nearest to each of PRESSURES; plus the extremes of ps."""
    nh, nz = h.grids[0].n_halo, h.cfg.npz
    pmid = 0.5 * (pe[1:] + pe[:-1])
    levels = [int(np.argmin(np.abs(pmid - p))) for p in PRESSURES]
    num = {n: np.zeros((len(LATITUDES), len(levels))) for n in ("ua", "t")}
    den = np.zeros(len(LATITUDES))
    ps_min, ps_max, finite = np.inf, -np.inf, True
    for i, g in enumerate(h.grids):
        cs = (slice(nh, nh + g.nx), slice(nh, nh + g.ny))
        lat, area = np.degrees(g.lat_agrid[cs]), g.area[cs]
        ua, t = h.state.ua.numpy(i)[cs].astype(np.float64), h.state.pt.numpy(i)[cs].astype(np.float64)
        ps = pe[0] + h.state.delp.numpy(i)[cs][:, :, :nz].astype(np.float64).sum(axis=2)
        ps_min, ps_max = min(ps_min, float(ps.min())), max(ps_max, float(ps.max()))
        finite = finite and bool(np.isfinite(ua[:, :, :nz]).all() and np.isfinite(t[:, :, :nz]).all() and np.isfinite(ps).all())
        for a, la in enumerate(LATITUDES):
            w = area * (np.abs(lat - la) <= 5.0)
            den[a] += w.sum()
            for b, k in enumerate(levels):
                num["ua"][a, b] += float((w * ua[:, :, k]).sum())
                num["t"][a, b] += float((w * t[:, :, k]).sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        out = {n: (num[n] / den[:, None]).tolist() for n in num}
    out.update(levels=levels, level_pressures_hPa=[float(pmid[k]) / 100.0 for k in levels], ps_min_hPa=ps_min / 100.0, ps_max_hPa=ps_max / 100.0, finite=finite)
    return out


def run(nx, days=None, steps=None, nz=79, every_h=24.0, device="cuda:0", make_harness=DycoreHarness, say=print):
    dt, ks, ns = STEPPING[nx]
    kw = {} if make_harness is not DycoreHarness else {"device": device}
    h = make_harness(nx, nz=nz, layout=(1, 1), dt_atmos=dt, k_split=ks, n_split=ns, init="baroclinic", n_tracers=1, remap=True, temperature=True, latlon_winds=True,
                     held_suarez=True, **kw)
    pe = rest_state(h)
    n_steps = int(steps) if steps is not None else int(round(days * 86400.0 / dt))
    per_out = max(1, int(round(every_h * 3600.0 / dt)))
    rec = []
    t0 = time.time()
    for step in range(1, n_steps + 1):
        h.step()
        if step % per_out == 0 or step == n_steps:
            h.synchronize()
            z = zonal_means(h, pe)
            z["day"] = step * dt / 86400.0
            z["wall_s"] = time.time() - t0
            rec.append(z)
            say(f"C{nx} day {z['day']:7.2f}  ps [{z['ps_min_hPa']:8.2f}, {z['ps_max_hPa']:8.2f}] hPa  finite {z['finite']}  ({z['wall_s']:.0f} s)")
            for b, p in enumerate(z["level_pressures_hPa"]):
                say(f"   {p:6.1f} hPa  ua " + " ".join(f"{z['ua'][a][b]:7.2f}" for a in range(len(LATITUDES))) + "   T " + " ".join(f"{z['t'][a][b]:7.2f}" for a in range(len(LATITUDES))))
            if not z["finite"]:
                break
    h.close()
    return {"nx": nx, "nz": nz, "dt_atmos": dt, "k_split": ks, "n_split": ns, "steps": n_steps, "latitudes": list(LATITUDES), "records": rec}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--nx", type=int, default=48, choices=sorted(STEPPING))
    ap.add_argument("--days", type=float, default=30.0)
    ap.add_argument("--steps", type=int, default=None, help="number of model steps (overrides --days)")
    ap.add_argument("--nz", type=int, default=79)
    ap.add_argument("--every", type=float, default=24.0, help="hours between printed records")
    ap.add_argument("--out", default=None)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    print("latitudes: " + " ".join(f"{la:7.1f}" for la in LATITUDES))
    res = run(a.nx, days=a.days, steps=a.steps, nz=a.nz, every_h=a.every, device=a.device)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    return 0 if res["records"] and res["records"][-1]["finite"] else 1


if __name__ == "__main__":
    sys.exit(main())
