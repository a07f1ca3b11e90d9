"""Time one diagnostics store on the GPU: the packed path (FieldPack -> one staging buffer -> one pinned host buffer, what
``MonitorDiagnostics.store`` does) against the path the tools used before it (``Quantity.numpy(i)`` per sub-domain: the whole padded
storage, halo and pad level included, copied and sliced on the host).  Both run in the same process on the same state; wall time from
the call to the host arrays being ready, median of ``--repeats`` after one warm-up.  One ``fv3_copy`` of a field runs in the same
process, so a ``rocprofv3 --kernel-trace --stats`` run of this script shows the pack kernel next to it.

    python tools/diag_store_timing.py [--config c384] [--names u v ua va w delp pt] [--repeats 5] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class _Consume:
    """A monitor that takes every array and writes nothing (the store's cost without the file system)."""

    bytes = 0

    def store(self, time, variables):
        self.bytes = 0
        for _, a, _, _ in variables:
            self.bytes += a.nbytes

    def store_constant(self, *a, **k):
        pass

    def cleanup(self):
        pass


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", default="c384")
    ap.add_argument("--names", nargs="*", default="u v ua va w delp pt".split())
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)

    from pace_amd.diagnostics import MonitorDiagnostics
    from pace_amd.harness import CONFIGS, DycoreHarness

    h = DycoreHarness(**CONFIGS[a.config])
    mon = _Consume()
    d = MonitorDiagnostics(mon, a.names, [], [], state=h.state, tracers=h.tracers, stencil_factory=h.sf, grids=h.grids)
    nx, ny, nz, nh = h.part.nx, h.part.ny, h.cfg.npz, 3

    def packed():
        d.store(0.0)
        return mon.bytes

    def padded():
        n = 0
        for name in a.names:
            q = getattr(h.state, name)
            ni, nj = nx + (q.dims[0] == "x_interface"), ny + (q.dims[1] == "y_interface")
            for i in range(q.n_sub):
                n += q.numpy(i)[nh : nh + ni, nh : nh + nj, :nz].nbytes  # (a view: the host slicing itself is free)
        return n

    out = {"config": a.config, "names": a.names, "repeats": a.repeats, "n_sub": len(h.grids), "nx": nx, "nz": nz, "dtype": str(h.sf.dtype)}
    for label, fn in (("packed", packed), ("padded_numpy", padded)):
        h.synchronize()
        fn()  # warm-up
        ts = []
        for _ in range(a.repeats):
            h.synchronize()
            t0 = time.perf_counter()
            nbytes = fn()
            ts.append(time.perf_counter() - t0)
        out[label] = {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts), "payload_bytes": nbytes}
    out["padded_bytes_moved"] = sum(getattr(h.state, n).storage.numel() * getattr(h.state, n).storage.element_size() for n in a.names)
    # one fv3_copy of a whole field (padded storage: read + write) beside the pack kernels, for the kernel trace
    scratch = h.sf.quantity_factory.zeros(("x", "y", "z"))
    h.sf.call("copy", h.state.pt.fref, scratch.fref)
    h.synchronize()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
