"""Coded fields, the case list and the checker of tests/test_halo_exchange.py, tests/test_distributed.py and the two-process GPU case of
tests/test_gpu_invariants.py: a HaloExchanger update against the geometric reference (tests/halo_reference.py), bit for bit.

Every compute-domain value is a distinct positive integer code of (field, component, tile, tile-global i, tile-global j, k) below 2^24 - 1 (exact in
fp32); ranks that share an interface inside a tile hold the same code.  Everything else in a storage -- halo, the blocks beyond cube corners, the unused
last row and column, the level beyond a 3-D field's own -- holds SENTINEL = -(2^24 - 1), which no signed code equals.  After an update the WHOLE storage
of every rank must equal what halo_reference.apply_update gives: halo points with a source hold sign x code(source), everything else is unchanged.

Run as a program it checks the whole case list in this (fresh) process: ``python tests/halo_exchange_case.py --backend B --precisions 64,32`` (the
FV3_GATHER_BATCH=0 child: the switch is read once per process), or, under torch.distributed.run, the multi-process cases (``--distributed``).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import halo_reference as hr  # noqa: E402

SENTINEL = -float(2**24 - 1)
NH = 3

_DIMS = {
    "cell": (("x", "y"),),
    "corner": (("x_interface", "y_interface"),),
    "dgrid": (("x", "y_interface"), ("x_interface", "y")),
    "cgrid": (("x_interface", "y"), ("x", "y_interface")),
}
_DIMS["sync_dgrid"] = _DIMS["dgrid"]

_SOURCES = {}


def sources(n, layout, rank, kind, depth):
    """halo_reference.halo_sources, computed once per argument set (read only)"""
    key = (n, tuple(layout), rank, kind, depth)
    if key not in _SOURCES:
        _SOURCES[key] = hr.halo_sources(n, layout, rank, kind, depth, NH)
    return _SOURCES[key]


def coded_globals(n, kind, field, nk, own):
    """G[comp][tile][gi, gj, k]: the code on the field's own levels, SENTINEL beyond"""
    G = []
    for comp in range(len(hr.KINDS[kind])):
        gx, gy = hr.global_shape(n, kind, comp)
        gi, gj, k = np.meshgrid(np.arange(gx), np.arange(gy), np.arange(nk), indexing="ij")
        tiles = []
        for t in range(6):
            code = 1.0 + ((((field * 2 + comp) * 6 + t) * (n + 1) + gi) * (n + 1) + gj) * nk + k
            assert code.max() < 2**24 - 1, "codes must stay exact in fp32 and apart from the sentinel"
            code[:, :, own:] = SENTINEL
            tiles.append(code)
        G.append(tiles)
    return G


_FACTORIES = {}


def factory(backend, dtype, n, layout, nz, world=1, proc=0, fresh=False):
    """(StencilFactory over the local ranks of process ``proc``, partitioner, Layout); kept per argument set"""
    import torch  # noqa: F401

    from pace_amd._testing import stencil_factory_for
    from pace_amd.config import AcousticDynamicsConfig
    from pace_amd.grid import make_grid
    from pace_amd.halo import Layout
    from pace_amd.topology import CubedSpherePartitioner

    key = (backend, dtype, n, tuple(layout), nz, world, proc)
    if fresh or key not in _FACTORIES:
        part = CubedSpherePartitioner(n, tuple(layout))
        lay = Layout(part, world, proc)
        # (nord = 1 in fp32: the default damping order's coefficient overflows fp32 on a grid this coarse; no halo code reads it)
        cfg = AcousticDynamicsConfig(npx=n + 1, npy=n + 1, npz=nz, layout=tuple(layout), **({} if dtype == torch.float64 else {"nord": 1}))
        grids = [make_grid(part, r, nz=nz) for r in lay.local_ranks]
        made = (stencil_factory_for(backend)(grids, cfg, None, dtype=dtype), part, lay)
        if fresh:
            return made
        _FACTORIES[key] = made
    return _FACTORIES[key]


def sync_device(sf):
    if not sf.hostemu:
        import torch

        torch.cuda.synchronize(sf.device)


class Coded:
    """The coded fields of one update on the local ranks of a process: host storages, expected storages, and the device quantities."""

    def __init__(self, sf, lay, n, layout, kind, depth, groups=1, two_d=False, first_field=0):
        self.sf, self.lay, self.n, self.layout, self.kind, self.depth = sf, lay, n, tuple(layout), kind, depth
        ni, nj, nk3 = sf.sizer.storage_shape
        self.nk = 1 if two_d else nk3
        self.own = 1 if two_d else sf.sizer.nz
        self.ncomp = len(hr.KINDS[kind])
        self.G, self.init, self.want = [], [], []
        self.written = 0
        local = lay.local_ranks
        src = {r: sources(n, layout, r, kind, depth) for r in local}
        for g in range(groups):
            G = coded_globals(n, kind, first_field + g, self.nk, self.own)
            st = hr.scatter(n, layout, kind, G, SENTINEL, ranks=local, n_halo=NH)
            if kind == "sync_dgrid":  # without this the sync is a no-op on consistent data and proves nothing
                for r in local:
                    R = hr.Rank(n, layout, r, NH)
                    st[r][0][NH : NH + R.nx, NH + R.ny, :] = SENTINEL
                    st[r][1][NH + R.nx, NH : NH + R.ny, :] = SENTINEL
            want, written = hr.apply_update(n, layout, kind, depth, G, st, sources=src, n_halo=NH)
            self.G.append(G)
            self.init.append(st)
            self.want.append(want)
            self.written += written
        # the count of section 2, from the closed form
        self.count = groups * sum(hr.expected_count(n, layout, r, kind, depth, NH) for r in local)
        assert self.written == self.count, (self.written, self.count)
        self.q = None

    def host_tensor(self, g, comp, which="init"):
        """[n_sub, (nk,) nj, ni] host array of one component of one group"""
        src = self.init if which == "init" else self.want
        a = np.stack([np.ascontiguousarray(src[g][r][comp].transpose(2, 1, 0)) for r in self.lay.local_ranks])
        return a[:, 0] if self.nk == 1 else a

    def quantities(self, fill=True):
        """one tuple of device quantities per group"""
        import torch

        qf = self.sf.quantity_factory
        self.q = []
        for g in range(len(self.G)):
            gp = []
            for comp in range(self.ncomp):
                q = qf.empty(_DIMS[self.kind][comp] + (() if self.nk == 1 else ("z",)))
                assert q.is_2d == (self.nk == 1)
                if fill:
                    q.storage.copy_(torch.from_numpy(self.host_tensor(g, comp)).to(q.storage.dtype))
                else:
                    q.storage.fill_(0.0)
                gp.append(q)
            self.q.append(tuple(gp))
        return self.q

    def check(self, storages=None):
        """Bitwise: the whole storage of every local rank, group and component against the reference.  Returns the number of halo points (per level)
        that were compared against a source."""
        checked = 0
        for g in range(len(self.G)):
            for comp in range(self.ncomp):
                t = self.q[g][comp].storage if storages is None else storages[g][comp]
                got = t.detach().cpu().numpy().astype(np.float64)
                want = self.host_tensor(g, comp, "want")
                init = self.host_tensor(g, comp, "init")
                bad = np.argwhere(got != want)
                assert bad.size == 0, (f"{self.kind} depth {self.depth} layout {self.layout} group {g} component {comp}: {len(bad)} values differ; first at "
                                       f"[sub, (k,) j, i] = {bad[0].tolist()}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}")
                # the points the update had to write, on the field's own levels: everywhere the expected storage differs from the initial one
                # (on the level beyond, a source holds the sentinel and only its sign can change)
                own = (slice(None), slice(0, self.own)) if self.nk > 1 else (slice(None),)
                checked += int((want[own] != init[own]).sum())
        assert checked == self.count * self.own, (checked, self.count, self.own)
        return checked // self.own


def run_update(cd, ex):
    groups = cd.quantities()
    if cd.kind == "sync_dgrid":
        ex.synchronize_vector_interfaces(*groups[0])
    else:
        ex.updater(cd.kind, groups, n_halo=cd.depth).update()
    sync_device(cd.sf)
    return cd.check()


# ---------------------------------------------------------------------------------------------------------------------------
# The case list: (name, nx_tile, layout, nz, kind, depth, groups, two_d).  The exchanger moves all storage levels, nz + 1 of them.
# ---------------------------------------------------------------------------------------------------------------------------
def case_list():
    cases = []
    for layout in ((1, 1), (2, 2), (1, 2)):
        for kind in ("cell", "corner", "dgrid", "cgrid"):
            for depth in (3, 1):
                cases.append((12, layout, 7, kind, depth, 1, False))
        cases.append((12, layout, 7, "sync_dgrid", 0, 1, False))
    # level counts around the 8-level thread tile of the gather kernels: storage_shape[2] = 7, 8 (above), 9, 16, 17; and nk = 1
    for nz in (6, 8, 15, 16):
        cases.append((12, (1, 1), nz, "dgrid", 3, 1, False))
        cases.append((12, (2, 2), nz, "cell", 3, 1, False))
    for layout in ((1, 1), (2, 2)):
        cases.append((12, layout, 7, "cell", 3, 1, True))
        cases.append((12, layout, 7, "dgrid", 3, 2, True))
    # The batch boundary (FV3_GATHER_MAXOPS = 12 gathers per launch).  In one process an update is one LOCAL gather per group and (destination component,
    # source component) pair that occurs: a scalar group is 1 job, a vector pair on a cube 4 (u<-u, v<-v and, across rotated tile edges, u<-v, v<-u; the
    # swapped plans are shorter).  13 scalar groups = 13 jobs (12 + a flush of 1); 4 vector pairs = 16 jobs of unequal lengths (12 + 4); 1 group = 1 job.
    cases.append((12, (1, 1), 7, "cell", 3, 13, False))
    cases.append((12, (2, 2), 7, "cell", 3, 13, False))
    cases.append((12, (1, 1), 7, "dgrid", 3, 4, False))
    cases.append((12, (2, 2), 8, "cgrid", 3, 4, False))
    cases.append((12, (1, 1), 7, "cell", 3, 1, False))
    return cases


def case_id(c):
    n, layout, nz, kind, depth, groups, two_d = c
    return f"c{n}-{layout[0]}x{layout[1]}-L{nz}-{kind}-d{depth}-g{groups}" + ("-2d" if two_d else "")


def run_case(backend, dtype, case):
    from pace_amd.halo import HaloExchanger

    n, layout, nz, kind, depth, groups, two_d = case
    sf, part, lay = factory(backend, dtype, n, layout, nz)
    ex = HaloExchanger.shared(sf, lay)
    cd = Coded(sf, lay, n, layout, kind, depth, groups, two_d)
    return run_update(cd, ex)


# ---------------------------------------------------------------------------------------------------------------------------
# Several processes: every worker checks its own ranks
# ---------------------------------------------------------------------------------------------------------------------------
def run_distributed(backend, dtype, n, layout, nz, world, proc, group=None):
    """One scalar updater with two groups, one dgrid updater, one corner updater and the sync on the local ranks of ``proc``; returns the points checked."""
    from pace_amd.halo import HaloExchanger

    sf, part, lay = factory(backend, dtype, n, layout, nz, world, proc)
    ex = HaloExchanger.shared(sf, lay, group=group)
    checked = {}
    for name, kind, depth, groups in (("cell", "cell", 3, 2), ("dgrid", "dgrid", 3, 1), ("corner", "corner", 3, 1), ("sync", "sync_dgrid", 0, 1)):
        checked[name] = run_update(Coded(sf, lay, n, layout, kind, depth, groups), ex)
    return checked


def distributed_counts(n, layout, world, proc):
    """what run_distributed must report, from the closed form"""
    per = hr.total_ranks(layout) // world
    local = range(proc * per, (proc + 1) * per)
    return {name: groups * sum(hr.expected_count(n, layout, r, kind, depth, NH) for r in local)
            for name, kind, depth, groups in (("cell", "cell", 3, 2), ("dgrid", "dgrid", 3, 1), ("corner", "corner", 3, 1), ("sync", "sync_dgrid", 0, 1))}


def main(argv=None):
    import argparse
    import json

    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--backend", default="hostemu")
    ap.add_argument("--precisions", default="64")
    ap.add_argument("--distributed", action="store_true")
    ap.add_argument("--nx", type=int, default=12)
    ap.add_argument("--layout", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    from pace_amd import build, lib

    precisions = [int(p) for p in a.precisions.split(",")]
    for p in precisions:
        if a.backend == "hostemu":
            build.build(p, hostemu=True, verbose=False)
        else:
            lib.load(p)
    if a.distributed:
        import torch.distributed as dist

        world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
        if a.backend != "hostemu":
            torch.cuda.set_device(int(os.environ.get("FV3_FORCE_DEVICE", os.environ.get("LOCAL_RANK", "0"))))
        dist.init_process_group("gloo")
        got = run_distributed(a.backend, torch.float64, a.nx, (a.layout, a.layout), 7, world, rank)
        want = distributed_counts(a.nx, (a.layout, a.layout), world, rank)
        assert got == want, (got, want)
        gathered = [None] * world
        dist.all_gather_object(gathered, got)
        dist.barrier()
        dist.destroy_process_group()
        if rank == 0 and a.out:
            json.dump(gathered, open(a.out, "w"))
        print(f"rank {rank} of {world}: checked {got}", flush=True)
        return 0
    total = 0
    for p in precisions:
        dtype = torch.float64 if p == 64 else torch.float32
        for c in case_list():
            total += run_case(a.backend, dtype, c)
    print(f"checked {total} halo points in {len(case_list())} cases x {len(precisions)} precisions", flush=True)
    if a.out:
        json.dump({"checked": total}, open(a.out, "w"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
