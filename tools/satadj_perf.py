"""Times of the moist remap with and without the saturation adjustment ("Saturation adjustment"): event times of the whole
entry on one GPU, six sub-domains, L79 fp64; under `rocprofv3 --kernel-trace --stats` the closing kernel's own duration (remap_close<true, false>
against remap_close<true, true>).

    python tools/satadj_perf.py [nx_tile = 192] [calls = 5]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pace_amd.harness import DycoreHarness
from pace_amd.stencils import LagrangianToEulerian, SaturationAdjustment

n = int(sys.argv[1]) if len(sys.argv) > 1 else 192
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
h = DycoreHarness(n, nz=79, layout=(1, 1), dt_atmos=225.0, k_split=1, n_split=2, n_tracers=6, hord_tr=8, remap=True, fill=True, temperature=True, moist=True, init="baroclinic")
h.tracers["qvapor"].storage.mul_(3.0)
for share, role in zip((0.02, 0.004, 0.01, 0.003, 0.002), ("qliquid", "qrain", "qice", "qsnow", "qgraupel")):
    h.tracers[role].storage.copy_(h.tracers["qvapor"].storage * share)
s, d = h.state, h.dycore
d.temperature_to_potential(s.pt, s.pkz, s.delp, s.delz, s.q_con, s.cappa, water=d.water)
d.dp1.storage.copy_(s.delp.storage)
d.acoustic_dynamics(s, 225.0, n_map=1)
d._tracer_halo.update()
d.tracer_advection(d.tracers, d.dp1, s.mfxd, s.mfyd, s.cxd, s.cyd)
h.synchronize()
fields = {k: getattr(s, k) for k in ("pt", "delp", "delz", "peln", "pe", "pk", "pkz", "u", "v", "w", "cappa", "q_con")}
fields.update(d.tracers)
saved = {k: q.storage.clone() for k, q in fields.items()}
op = SaturationAdjustment(h.sf)
rm = LagrangianToEulerian(h.sf, fill=True)
args = (d.tracers, s.pt, s.delp, s.delz, s.peln, s.pe, s.pk, s.pkz, s.u, s.v, s.w, s.cappa, d.ps, d.acoustic_dynamics._wsd)
variants = {"moist": {}, "sat_mid": dict(sat_adjust=op, mdt=225.0, last_step=False), "sat_last": dict(sat_adjust=op, mdt=225.0, last_step=True)}
for name, kw in variants.items():
    ms = []
    for r in range(reps + 1):
        for k, q in fields.items():
            q.storage.copy_(saved[k])
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(torch.cuda.current_stream())
        rm(*args, q_con=s.q_con, water=d.water, **kw)
        e1.record(torch.cuda.current_stream())
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    ok = bool(torch.isfinite(s.pt.storage[:, :79]).all())
    print(f"C{n} L79 fp64 remap entry {name}: first {ms[0]:.3f} ms, then {' '.join(f'{x:.3f}' for x in ms[1:])} ms; qliquid max {float(d.tracers['qliquid'].storage.max()):.3e}; finite {ok}", flush=True)
print("kmp", op.level0, "stream", h.sf.stream_handle)
h.close()
