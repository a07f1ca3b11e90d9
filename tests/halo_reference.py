"""Where every halo point of a cubed-sphere rank comes from, derived from POSITIONS ON THE SPHERE -- the reference the halo layer
(pace_amd/topology.py, pace_amd/halo.py, the gather kernels) is pinned to in tests/test_halo_exchange.py and tests/test_distributed.py.

Nothing here goes through the library's frame algebra: the only import from the package is ``pace_amd.grid.tile_point`` (the closed-form unit vector
of the grid corner with integer tile coordinates), everything else is numpy, and the rank arithmetic (``rank = tile * lx * ly + sy * lx + sx``, origin
``(sx * nx, sy * ny)``) is written out below.

The edge table.  For every tile the unit vectors of its boundary corners (x, y), x, y in 0..N, are indexed by rounded position; an edge point then has
two owners and a cube corner three.  For tile t and edge d the corners at along-edge index 1 and 2 are looked up: their coordinates in the other owner's
frame are q1 and q2, that owner is the neighbour n, ``da = q2 - q1`` is the image of the destination's along-edge axis, ``q0 = q1 - da`` the image of
along-edge coordinate 0, and ``w`` -- the image of the destination's outward direction -- is the unit vector perpendicular to da for which q1 + w lies
inside [0, N]^2.

A destination point with tile coordinates (x, y) beyond exactly one tile edge, at depth dep > 0 and along-edge coordinate s, comes from
``q0 + s da + dep w`` of tile n; beyond two tile edges (the blocks beyond a cube corner) it has no source; inside the tile it is itself.  A vector
component's direction maps as along-edge axis -> da, outward axis -> w: the image's non-zero entry is the sign and its position the source component.
The interface sync is the same map at depth 0 for a rank's north row (u) and east column (v): the other owner of that point.

Storage convention (the package's): index i of a component with staggering offset ox sits at x = x0 + (i - n_halo) + ox, ox = 0.5 for a cell centre and 0
for an interface; arrays are [i, j, k].
"""
import numpy as np

from pace_amd.grid import tile_point

WEST, EAST, SOUTH, NORTH = 0, 1, 2, 3
CELL, IFACE = 0.5, 0.0
# staggering offsets (x, y) of each component of a kind
KINDS = {
    "cell": ((CELL, CELL),),
    "corner": ((IFACE, IFACE),),
    "dgrid": ((CELL, IFACE), (IFACE, CELL)),  # u on y-interfaces, v on x-interfaces
    "cgrid": ((IFACE, CELL), (CELL, IFACE)),
    "sync_dgrid": ((CELL, IFACE), (IFACE, CELL)),
}
_ALONG = {WEST: (0, 1), EAST: (0, 1), SOUTH: (1, 0), NORTH: (1, 0)}
_OUT = {WEST: (-1, 0), EAST: (1, 0), SOUTH: (0, -1), NORTH: (0, 1)}

_TABLES = {}


def _edge_point(n, d, s):
    """tile coordinates of the point at along-edge coordinate s on edge d"""
    return {WEST: (0, s), EAST: (n, s), SOUTH: (s, 0), NORTH: (s, n)}[d]


def edge_table(n):
    """{(tile, edge): (neighbour tile, q0, da, w)} of a C<n> cube, from corner positions alone"""
    if n in _TABLES:
        return _TABLES[n]
    owners = {}
    for t in range(6):
        for x in range(n + 1):
            for y in range(n + 1):
                if x in (0, n) or y in (0, n):
                    p = tile_point(t, np.array(x), np.array(y), n)
                    key = tuple(int(v) for v in np.rint(np.asarray(p, dtype=np.float64).ravel() * 1e6))
                    owners.setdefault(key, []).append((t, x, y))
    by_point = {}
    for lst in owners.values():
        for o in lst:
            by_point[o] = [q for q in lst if q[0] != o[0]]
    n_owners = sorted(len(v) for v in owners.values())
    assert n_owners.count(3) == 8 and n_owners.count(2) == 12 * (n - 1) and len(n_owners) == 8 + 12 * (n - 1), "the cube does not close"
    table = {}
    for t in range(6):
        for d in (WEST, EAST, SOUTH, NORTH):
            (o1,), (o2,) = by_point[(t,) + _edge_point(n, d, 1)], by_point[(t,) + _edge_point(n, d, 2)]
            assert o1[0] == o2[0]
            q1, q2 = np.array(o1[1:], dtype=np.int64), np.array(o2[1:], dtype=np.int64)
            da = q2 - q1
            assert abs(da).sum() == 1
            q0 = q1 - da
            ws = [w for w in (np.array([-da[1], da[0]]), np.array([da[1], -da[0]])) if ((q1 + w >= 0) & (q1 + w <= n)).all()]
            assert len(ws) == 1
            table[(t, d)] = (o1[0], q0, da, ws[0])
    _TABLES[n] = table
    return table


class Rank:
    """the rank arithmetic, written out"""

    def __init__(self, n, layout, rank, n_halo=3):
        lx, ly = layout
        self.n, self.lx, self.ly, self.nh = n, lx, ly, n_halo
        self.nx, self.ny = n // lx, n // ly
        self.rank = rank
        self.tile = rank // (lx * ly)
        self.sx, self.sy = (rank % (lx * ly)) % lx, (rank % (lx * ly)) // lx
        self.x0, self.y0 = self.sx * self.nx, self.sy * self.ny
        self.shape = (self.nx + 2 * n_halo + 1, self.ny + 2 * n_halo + 1)

    def extent(self, stagger):
        return self.nx + (1 if stagger[0] == IFACE else 0), self.ny + (1 if stagger[1] == IFACE else 0)

    def tile_corners(self):
        """how many of this rank's four corners are cube corners"""
        w, e, s, nn = self.sx == 0, self.sx == self.lx - 1, self.sy == 0, self.sy == self.ly - 1
        return int(w and s) + int(w and nn) + int(e and s) + int(e and nn)


def total_ranks(layout):
    return 6 * layout[0] * layout[1]


def _across(n, tile, staggers, comp, x, y, force_edge=None):
    """Sources of the points (x, y) (tile coordinates, possibly outside [0, n]^2) of component comp: arrays (has source, source tile, source component,
    tile-global i, tile-global j, sign).  ``force_edge``: every point lies ON that tile edge (depth 0: the interface sync) and is mapped across it."""
    table = edge_table(n)
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    bx = np.where(x < 0, -1, np.where(x > n, 1, 0))
    by = np.where(y < 0, -1, np.where(y > n, 1, 0))
    has = ~((bx != 0) & (by != 0))
    st = np.full(x.shape, tile, dtype=np.int64)
    sc = np.full(x.shape, comp, dtype=np.int64)
    sg = np.ones(x.shape, dtype=np.int64)
    px, py = x.copy(), y.copy()
    e = np.zeros(2, dtype=np.int64)
    e[comp if len(staggers) == 2 else 0] = 1
    for d, mask in ((WEST, (bx == -1) & (by == 0)), (EAST, (bx == 1) & (by == 0)), (SOUTH, (by == -1) & (bx == 0)), (NORTH, (by == 1) & (bx == 0))):
        if force_edge is not None:
            mask = np.full(x.shape, d == force_edge)
        if not mask.any():
            continue
        nb, q0, da, w = table[(tile, d)]
        if d == WEST:
            s, dep = y[mask], -x[mask]
        elif d == EAST:
            s, dep = y[mask], x[mask] - n
        elif d == SOUTH:
            s, dep = x[mask], -y[mask]
        else:
            s, dep = x[mask], y[mask] - n
        st[mask] = nb
        px[mask] = q0[0] + s * da[0] + dep * w[0]
        py[mask] = q0[1] + s * da[1] + dep * w[1]
        if len(staggers) == 2:
            a, o = np.array(_ALONG[d]), np.array(_OUT[d])
            img = int(e @ a) * da + int(e @ o) * w  # (a, o is an orthonormal basis of the destination frame)
            c2 = 0 if img[0] != 0 else 1
            sc[mask] = c2
            sg[mask] = img[c2]
    ox = np.array([s_[0] for s_ in staggers])[sc]
    oy = np.array([s_[1] for s_ in staggers])[sc]
    gi, gj = px - ox, py - oy
    ri, rj = np.rint(gi).astype(np.int64), np.rint(gj).astype(np.int64)
    if has.any():
        assert np.array_equal(ri[has], gi[has]) and np.array_equal(rj[has], gj[has]), "a source that is no storage point of its component"
        ex = n + (ox[has] == IFACE)
        ey = n + (oy[has] == IFACE)
        assert (ri[has] >= 0).all() and (ri[has] < ex).all() and (rj[has] >= 0).all() and (rj[has] < ey).all(), "a source outside its tile"
    return has, st, sc, ri, rj, sg


def halo_sources(n, layout, rank, kind, depth, n_halo=3):
    """{(component, i, j): (source tile, source component, tile-global i, tile-global j, sign) or None} for EVERY point of the depth-wide halo frame of
    ``rank`` (storage indices i, j); None: no source (beyond a cube corner).  kind 'sync_dgrid': the north row of u and the east column of v (depth is
    ignored), each from the other owner of the point."""
    R = Rank(n, layout, rank, n_halo)
    staggers = KINDS[kind]
    out = {}
    for comp, (ox, oy) in enumerate(staggers):
        ex, ey = R.extent((ox, oy))
        nh = n_halo
        if kind == "sync_dgrid":
            if comp == 0:  # u: north row
                i = np.arange(nh, nh + ex)
                j = np.full(i.shape, nh + R.ny)
                edge = NORTH if R.sy == R.ly - 1 else None
            else:  # v: east column
                j = np.arange(nh, nh + ey)
                i = np.full(j.shape, nh + R.nx)
                edge = EAST if R.sx == R.lx - 1 else None
            x, y = R.x0 + (i - nh) + ox, R.y0 + (j - nh) + oy
            if edge is None:  # the same tile-global point, held by the rank to the north / east
                has, st, sc = np.ones(i.shape, bool), np.full(i.shape, R.tile), np.full(i.shape, comp)
                gi, gj, sg = R.x0 + (i - nh), R.y0 + (j - nh), np.ones(i.shape, np.int64)
            else:
                has, st, sc, gi, gj, sg = _across(n, R.tile, staggers, comp, x, y, force_edge=edge)
        else:
            ii, jj = np.meshgrid(np.arange(nh - depth, nh + ex + depth), np.arange(nh - depth, nh + ey + depth), indexing="ij")
            i, j = ii.ravel(), jj.ravel()
            frame = (i < nh) | (i >= nh + ex) | (j < nh) | (j >= nh + ey)
            i, j = i[frame], j[frame]
            x, y = R.x0 + (i - nh) + ox, R.y0 + (j - nh) + oy
            has, st, sc, gi, gj, sg = _across(n, R.tile, staggers, comp, x, y)
        for m in range(len(i)):
            key = (comp, int(i[m]), int(j[m]))
            assert key not in out
            out[key] = (int(st[m]), int(sc[m]), int(gi[m]), int(gj[m]), int(sg[m])) if has[m] else None
    return out


def expected_count(n, layout, rank, kind, depth, n_halo=3):
    """Closed form: the halo frame of each component's extent, (ex + 2 d)(ey + 2 d) - ex ey, minus d^2 points for every corner of the rank that is a cube
    corner (the points beyond two tile edges); the sync: the nx faces of the north row and the ny faces of the east column."""
    R = Rank(n, layout, rank, n_halo)
    if kind == "sync_dgrid":
        return R.nx + R.ny
    total = 0
    for stagger in KINDS[kind]:
        ex, ey = R.extent(stagger)
        total += (ex + 2 * depth) * (ey + 2 * depth) - ex * ey - R.tile_corners() * depth * depth
    return total


def frame_count(n, layout, rank, kind, depth, n_halo=3):
    """every point of the frame, with or without a source"""
    R = Rank(n, layout, rank, n_halo)
    if kind == "sync_dgrid":
        return R.nx + R.ny
    return sum((R.extent(s)[0] + 2 * depth) * (R.extent(s)[1] + 2 * depth) - R.extent(s)[0] * R.extent(s)[1] for s in KINDS[kind])


def global_shape(n, kind, comp):
    ox, oy = KINDS[kind][comp]
    return n + (1 if ox == IFACE else 0), n + (1 if oy == IFACE else 0)


def scatter(n, layout, kind, G, fill, ranks=None, n_halo=3):
    """Per-rank storages from per-tile global arrays: ``G[comp][tile]`` is [i, j, k] over the component's whole tile (interfaces included, so ranks that
    share an interface hold the same value); everything outside a rank's compute domain holds ``fill``.  Returns {rank: [array per component]}."""
    out = {}
    for r in range(total_ranks(layout)) if ranks is None else ranks:
        R = Rank(n, layout, r, n_halo)
        comps = []
        for comp, stagger in enumerate(KINDS[kind]):
            ex, ey = R.extent(stagger)
            g = G[comp][R.tile]
            a = np.full(R.shape + (g.shape[2],), fill, dtype=g.dtype)
            a[n_halo : n_halo + ex, n_halo : n_halo + ey, :] = g[R.x0 : R.x0 + ex, R.y0 : R.y0 + ey, :]
            comps.append(a)
        out[r] = comps
    return out


def apply_update(n, layout, kind, depth, G, storages, sources=None, n_halo=3):
    """The update in numpy: a signed copy.  ``storages``: {rank: [array per component]} as ``scatter`` returns them (not modified); ``sources``: {rank:
    halo_sources(...)} to apply a mutated table instead of the reference's own.  Returns (expected storages, number of points written per level)."""
    out, written = {}, 0
    for r, comps in storages.items():
        src = sources[r] if sources is not None else halo_sources(n, layout, r, kind, depth, n_halo)
        new = [a.copy() for a in comps]
        for (comp, i, j), s in src.items():
            if s is None:
                continue
            t, c2, gi, gj, sign = s
            new[comp][i, j, :] = sign * G[c2][t][gi, gj, :]
            written += 1
        out[r] = new
    return out, written
