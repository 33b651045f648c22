"""The clearance field restated from the exported rows (include/gndt.h "clearance field"): a dict of columns, the flood's three gates
in numpy on every (slope, neighbour row) pair, a breadth-first search on the reversed step graph for hops, and nearest by its rule —
the smallest source exactly hops steps away — layer by layer of that search.  Shares no code with grid_ndt_amd/csrc/gndt_clearance.hpp.
Also reports how close any angle decision came to its threshold (acosf is the one step that is not IEEE arithmetic), as the cost tests'
angle_margin_deg does.  Test infrastructure only."""
from collections import deque

import numpy as np

BLOCKED, OPEN, OVERHEAD = 1, 2, 4
BEYOND = 0xFFFFFFFF
NO_ROW = 0xFFFFFFFF
MAX_XY = 65535
ROBOT = dict(radius=0.25, reachable_height=0.15, max_rough=100.0, max_angle_deg=30.0)       # the flood's defaults


def step(v, d):
    """one step along an axis of signed indices: there is no index 0"""
    r = v + d
    return r + d if r == 0 else r


def sides_of(x, y):
    """the four neighbour columns in the flood's order: left, right, forward, back"""
    return (x, step(y, -1)), (x, step(y, 1)), (step(x, 1), y), (step(x, -1), y)


def angle_deg(n1, n2):
    """the flood's angle between normals, [P, 3] float32 each: fp32 products summed as a + (b + c), norms in double, the quotient
    rounded to fp32, arc cosine, degrees through a double division, folded at 90"""
    p = n1 * n2
    dot = p[:, 0] + (p[:, 1] + p[:, 2])
    a, b = n1.astype(np.float64) ** 2, n2.astype(np.float64) ** 2
    l1, l2 = np.sqrt((a[:, 0] + a[:, 1]) + a[:, 2]), np.sqrt((b[:, 0] + b[:, 1]) + b[:, 2])
    with np.errstate(invalid="ignore", divide="ignore"):
        res = (dot.astype(np.float64) / (l1 * l2)).astype(np.float32)
        ac = np.arccos(res).astype(np.float32) * np.float32(180.0)
    an = (ac.astype(np.float64) / np.pi).astype(np.float32)
    return np.where(an > np.float32(90.0), np.float32(180.0) - an, an)


# ---- clouds the clearance tests draw their maps with ----------------------------------------------------------------------------------
CORRIDOR_P = dict(grid_len=0.5, z_len=0.25, slope_interval=0.08, demand="slope")


def corridor_cloud(seed=3):
    """A corridor seven columns wide between two plateaus a metre higher: columns ix = -3 .. 9 by iy = 0 .. 11, twelve points each, z =
    0.05 + U(0, 0.01) for 0 <= ix < 7 and a metre more elsewhere; the origin point first.  156 rows, all slopes; under BLOCKED the 48
    slopes on either side of the two steps are the sources."""
    rng = np.random.default_rng(seed)
    pts = [[0.01, 0.01, 0.01]]
    for ix in range(-3, 10):
        for iy in range(12):
            for a in (0.1, 0.25, 0.4):
                for b in (0.08, 0.19, 0.3, 0.41):
                    z = 0.05 + rng.uniform(0.0, 0.01) + (0.0 if 0 <= ix < 7 else 1.0)
                    pts.append([0.01 + ix * 0.5 + a, 0.01 + iy * 0.5 + b, z])
    return np.ascontiguousarray(np.float32(pts))


def pit_cloud(depth=36):
    """A line of cells ix = 0 .. 7 at iy = 0 (tests/frontier_ref.cells_cloud's cells), the last one a metre higher — under BLOCKED cells 6
    and 7 are the sources — with `depth` single points stacked under cell 3, one per level: nodes without statistics, seen BEFORE the
    cell's floor points, so that its column has depth + 1 rows of which the floor's slope is the last."""
    from tests import frontier_ref as fr
    floor = fr.cells_cloud([(ix, 0) for ix in range(8) if ix not in (3, 7)] + [(7, 0, fr.Z_FLOOR + 1.0), (3, 0)])
    pit = [[3 * fr.GL + 0.25, 0.25, fr.Z_FLOOR - fr.ZL * j] for j in range(1, depth + 1)]
    return np.ascontiguousarray(np.concatenate([floor[:1], np.float32(pit), floor[1:]]))


def lattice_cloud(W, H, walls=(), P=None):
    """A W x H floor of tests/frontier_ref.cells_cloud's cells, one per column (ix = 0 .. W-1, iy = 0 .. H-1), the cells of `walls`
    a metre higher: exactly W * H rows, every one a slope (a wall's top is as level as the floor), and under BLOCKED the sources are
    the slopes on either side of a wall's outline.  P: the parameters the map is built with, which have to be the cells' own."""
    from tests import frontier_ref as fr
    P = fr.P if P is None else P
    assert (P["grid_len"], P["z_len"], P["slope_interval"]) == (fr.GL, fr.ZL, fr.IV), "cells_cloud draws cells of frontier_ref.P"
    walls = set(walls)
    assert all(0 <= ix < W and 0 <= iy < H for ix, iy in walls)
    return fr.cells_cloud([(ix, iy, fr.Z_FLOOR + 1.0) if (ix, iy) in walls else (ix, iy) for ix in range(W) for iy in range(H)])


def wall(xs, ys):
    """the cells of a straight wall: every (ix, iy) of the two ranges"""
    return frozenset((ix, iy) for ix in xs for iy in ys)


# The lattices of the kernel-edge tests by row count: (W, H, walls).  9216 = kClrLdsRows fills k_clearance_wg, 9217 is the first
# launch-a-hop size, 1023 / 1024 / 1025 lie around the slot edge of its 1024 threads, 131 769 is 697 rows into the second grid-stride
# trip of k_clearance_finish (and 4 n far into that of the steps and the rounds), 14 641 and the 41 x 25 map are the large and the
# small map of tests/test_gpu_scratch_reuse.py.  The short walls stand near a corner, so that the far corner is many hops away.
LATTICES = {
    1023: (31, 33, wall([1], range(1, 4))),
    1024: (32, 32, wall([1], range(1, 4))),
    1025: (25, 41, wall([1], range(1, 4))),
    2048: (32, 64, wall([1], range(1, 4))),          # kWalkTableRowsPerWaypoint: the walk's table choice at T = 1, to the row
    9216: (96, 96, wall([1], range(1, 4))),
    9217: (13, 709, wall([1], range(1, 4))),
    131769: (363, 363, wall([60], range(40, 300)) | wall(range(150, 330), [200])),
    14641: (121, 121, wall([60], range(10, 111)) | wall(range(5, 40), [30])),
    "41x25": (41, 25, wall(range(8, 30), [12])),
}


def lattice(name, P=None):
    W, H, walls = LATTICES[name]
    return lattice_cloud(W, H, walls, P)


class Field:
    """The step graph of the exported rows for one robot; the answers per (sources, max_hops)."""

    def __init__(self, cells, robot=None):
        rb = dict(ROBOT)
        rb.update(robot or {})
        self.robot = {k: np.float32(v) for k, v in rb.items()}
        n = self.n = int(cells["num_nodes"])
        sx, sy, sz = ([int(v) for v in cells[k][:n]] for k in ("sx", "sy", "sz"))
        flags = np.asarray(cells["flags"][:n])
        self.slope = (flags & 2) != 0
        mean = np.asarray(cells["mean"], np.float32).reshape(-1, 3)[:n]
        normal = np.asarray(cells["normal"], np.float32).reshape(-1, 3)[:n]
        rough = np.asarray(cells["rough"], np.float32)[:n]
        cols = {}
        for r in range(n):
            cols.setdefault((sx[r], sy[r]), []).append(r)
        # every (slope q, side k, row t of that side's column) pair; sides without a column are open
        pq, pk, pt = [], [], []
        self.open = np.zeros((n, 4), bool)
        present = np.zeros((n, 4), bool)
        for q in range(n):
            if not self.slope[q]:
                continue
            for k, (nx, ny) in enumerate(sides_of(sx[q], sy[q])):
                rows = None if abs(nx) > MAX_XY or abs(ny) > MAX_XY else cols.get((nx, ny))
                if rows is None:
                    self.open[q, k] = True
                    continue
                present[q, k] = True
                pq += [q] * len(rows); pk += [k] * len(rows); pt += rows
        pq, pk, pt = (np.array(a, np.int64) for a in (pq, pk, pt))
        ang = angle_deg(normal[pt], normal[pq]) if len(pq) else np.zeros(0, np.float32)
        ok = self.slope[pt] & (rough[pt] <= self.robot["max_rough"]) & (ang <= self.robot["max_angle_deg"]) & \
            (np.abs(mean[pt, 2] - mean[pq, 2]) <= self.robot["reachable_height"])
        asked = self.slope[pt] & np.isfinite(ang)
        self.angle_margin_deg = float(np.abs(ang[asked].astype(np.float64) - float(self.robot["max_angle_deg"])).min()) if asked.any() else 90.0
        self.edge_from, self.edge_to = pq[ok], pt[ok]           # the steps q -> t
        passable = np.zeros((n, 4), bool)
        passable[pq[ok], pk[ok]] = True
        self.blocked = present & ~passable
        w = 1 << np.arange(4)
        self.sides = np.where(self.slope, (self.blocked * w).sum(1) | ((self.open * w).sum(1) << 4), 0xFF).astype(np.uint8)
        self.steps = [[] for _ in range(n)]
        self.back = [[] for _ in range(n)]
        for q, t in zip(self.edge_from.tolist(), self.edge_to.tolist()):
            self.steps[q].append(t)
            self.back[t].append(q)
        # OVERHEAD: the next slope above in the row's own cell, within 2 r and more than the reach above (fp32, as the flood computes)
        self.overhead = np.zeros(n, bool)
        two_r = np.float32(2.0) * self.robot["radius"]
        for rows in cols.values():
            for q in rows:
                if not self.slope[q]:
                    continue
                above = [t for t in rows if self.slope[t] and sz[t] > sz[q]]
                if not above:
                    continue
                t = min(above, key=lambda t: sz[t])
                mz, nz = mean[q, 2], mean[t, 2]
                self.overhead[q] = bool((nz < np.float32(mz + two_r)) and (np.float32(nz - mz) > self.robot["reachable_height"]))
        self._full = {}

    def sources(self, mask):
        mask = mask or BLOCKED
        s = np.zeros(self.n, bool)
        if mask & BLOCKED:
            s |= self.blocked.any(1)
        if mask & OPEN:
            s |= self.open.any(1)
        if mask & OVERHEAD:
            s |= self.overhead
        return s & self.slope

    def full(self, mask):
        """hops and nearest without a limit -> (hops int64, -1 = none; nearest int64, -1 = none)"""
        mask = mask or BLOCKED
        if mask not in self._full:
            n = self.n
            hops = np.full(n, -1, np.int64)
            near = np.full(n, -1, np.int64)
            src = np.flatnonzero(self.sources(mask))
            hops[src] = 0
            near[src] = src
            queue = deque(src.tolist())
            order = []
            while queue:                                    # reversed graph: who steps INTO p is one further away
                p = queue.popleft()
                order.append(p)
                for q in self.back[p]:
                    if hops[q] < 0:
                        hops[q] = hops[p] + 1
                        queue.append(q)
            for q in order:                                 # ascending hops: a walk of hops(q) steps goes through a step one nearer
                if hops[q] > 0:
                    near[q] = min(int(near[p]) for p in self.steps[q] if hops[p] == hops[q] - 1)
            self._full[mask] = (hops, near)
        return self._full[mask]

    def clearance(self, mask=BLOCKED, max_hops=32):
        """-> dict(hops uint32, nearest uint32, sides uint8, counts uint32 [4]) as gndt_clearance writes them"""
        max_hops = max_hops or 32
        h, nr = self.full(mask)
        ok = (h >= 0) & (h <= max_hops)
        hops = np.where(ok, h, BEYOND).astype(np.uint32)
        nearest = np.where(ok, nr, NO_ROW).astype(np.uint32)
        counts = np.array([int((h == 0).sum()), int(ok.sum()), int(h[ok].max()) if ok.any() else 0, 0], np.uint32)
        return dict(hops=hops, nearest=nearest, sides=self.sides, counts=counts)

    def nearest_by_search(self, mask=BLOCKED):
        """nearest from one forward search per row (small maps): the sources in the first layer that holds any"""
        src = self.sources(mask)
        out = np.full(self.n, -1, np.int64)
        for q in np.flatnonzero(self.slope):
            layer, seen = {int(q)}, {int(q)}
            while layer:
                hit = [r for r in layer if src[r]]
                if hit:
                    out[q] = min(hit)
                    break
                layer = {t for r in layer for t in self.steps[r]} - seen
                seen |= layer
        return out
