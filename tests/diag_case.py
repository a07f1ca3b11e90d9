"""The case of the diagnostics output tests (tests/test_diagnostics_output.py on the host emulation, tests/test_driver_diagnostics.py on
the GPU): a C12 cube with layout (1, 2) -- 12 sub-domains of 12 x 6 cells, nz 8, two tracers, remap -- the driver's loop around the
diagnostics, and the two-process run whose store must equal the one-process store byte for byte."""
import filecmp
import os
import sys
from datetime import timedelta

import torch
import torch.multiprocessing as mp

from pace_amd.diagnostics import DiagnosticsConfig
from pace_amd.monitor import DEFAULT_START_TIME

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NX, NZ, LAYOUT, DT = 12, 8, (1, 2), 225.0
NAMES = "u v ua va w delp pt phis tracer0".split()
DERIVED = ["column_integrated_tracer1"]
ZSEL = [{"level": 3, "names": ["pt"]}]
HARNESS = dict(nz=NZ, layout=LAYOUT, dt_atmos=DT, n_tracers=2, remap=True)


def config(path, fmt, time_chunk_size=1):
    return DiagnosticsConfig.from_dict(dict(path=str(path), output_format=fmt, time_chunk_size=time_chunk_size, names=NAMES, derived_names=DERIVED, z_select=ZSEL))


def run(h, diags, n_steps, output_frequency=1, output_initial_state=False, step0=0):
    """The driver's loop around the diagnostics [REF driver/pace/driver/driver.py:551-552, 588-611, 702-705]."""
    if output_initial_state:
        for d in diags:
            d.store(DEFAULT_START_TIME + timedelta(seconds=step0 * DT))
    for step in range(n_steps):
        h.step()
        if (step + 1) % output_frequency == 0:
            for d in diags:
                d.store(DEFAULT_START_TIME + timedelta(seconds=(step0 + step + 1) * DT))
    for d in diags:
        d.store_grid(h.grids)
        d.cleanup()


def worker(rank, world, init_file, out_dir, backend):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist

    from pace_amd._testing import harness_for

    torch.set_num_threads(1)
    os.environ["OMP_NUM_THREADS"] = "2"
    dist.init_process_group("gloo", init_method=f"file://{init_file}", rank=rank, world_size=world)
    h = harness_for(backend)(NX, world_size=world, proc=rank, group=None, **HARNESS)
    run(h, [config(out_dir, "zarr").diagnostics_factory(h)], 2, output_initial_state=True)
    dist.barrier()
    h.close()
    dist.destroy_process_group()




def assert_two_process_store_is_byte_identical(backend, store, tmp_path):
    """Two gloo processes with 6 sub-domains each (on the GPU both share device 0: three processes with the GPU open) write a store
    whose every file equals the one-process store's."""
    out = tmp_path / "zarr2"
    mp.spawn(worker, args=(2, str(tmp_path / "init"), str(out), backend), nprocs=2, join=True)

    def listing(root):
        return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)

    files = listing(store)
    assert listing(str(out)) == files and len(files) > 100
    match, mismatch, errors = filecmp.cmpfiles(store, str(out), files, shallow=False)
    assert not mismatch and not errors and len(match) == len(files), (mismatch[:5], errors[:5])
