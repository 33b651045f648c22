"""Frontier extraction restated from the exported rows (include/gndt.h "frontier extraction"): a dict of columns, Python loops and a
breadth-first search for the components.  Shares no code with grid_ndt_amd/csrc/gndt_frontier.hpp.  Also the cell-list clouds the
frontier tests draw their maps with.  Test infrastructure only."""
from collections import deque

import numpy as np

REACHED, SLOPES = 0, 1
OPEN_COLUMN, OPEN_LEVEL = 0, 1
NO_ROW = 0xFFFFFFFF
FLT_MAX_BITS = 0x7F7FFFFF
MAX_XY = 65535
RECORD = np.dtype([("label", np.uint32), ("size", np.uint32), ("best_row", np.uint32), ("best_h", np.float32),
                   ("sx_min", np.int32), ("sx_max", np.int32), ("sy_min", np.int32), ("sy_max", np.int32),
                   ("sum_px", np.int64), ("sum_py", np.int64), ("sum_pz", np.int64), ("open_sides", np.uint32), ("reserved", np.uint32)])
assert RECORD.itemsize == 64


def lin(s):
    """the position of a signed index on a line without the hole at 0"""
    return s - 1 if s > 0 else s


def step(v, d):
    """one step along an axis of signed indices: there is no index 0"""
    r = v + d
    return r + d if r == 0 else r


class Map:
    """The exported rows with their column dict; the open sides of every slope are kept per (open_rule, level_reach)."""

    def __init__(self, cells):
        self.n = int(cells["num_nodes"])
        self.sx, self.sy, self.sz = ([int(v) for v in cells[k][:self.n]] for k in ("sx", "sy", "sz"))
        self.slope = [bool(int(f) & 2) for f in cells["flags"][:self.n]]
        self.cols = {}
        for r in range(self.n):
            self.cols.setdefault((self.sx[r], self.sy[r]), []).append(r)
        self._open = {}

    def side_open(self, nx, ny, z, open_rule, level_reach):
        if abs(nx) > MAX_XY or abs(ny) > MAX_XY:
            return True
        rows = self.cols.get((nx, ny))
        if rows is None:
            return True
        if open_rule == OPEN_COLUMN:
            return False
        return not any(abs(lin(self.sz[t]) - lin(z)) <= level_reach for t in rows)

    def open_sides(self, open_rule, level_reach):
        key = (open_rule, level_reach if open_rule == OPEN_LEVEL else 0)
        if key not in self._open:
            out = np.zeros(self.n, np.int64)
            for r in range(self.n):
                if not self.slope[r]:
                    continue
                x, y, z = self.sx[r], self.sy[r], self.sz[r]
                out[r] = sum(self.side_open(nx, ny, z, open_rule, level_reach)
                             for nx, ny in ((step(x, -1), y), (step(x, 1), y), (x, step(y, -1)), (x, step(y, 1))))
            self._open[key] = out
        return self._open[key]

    def frontiers(self, candidates=REACHED, open_rule=OPEN_COLUMN, level_reach=1, min_open=1, link_dz=1, box=None, h_bits=None, state=None):
        """-> dict(label [n] uint32, open [n] (the frontier rows' open sides, 0 elsewhere), clusters: RECORD array of EVERY cluster
        in ascending label, rows: the number of frontier rows)"""
        n = self.n
        min_open = max(int(min_open), 1)
        opens = self.open_sides(open_rule, level_reach)
        front = []
        for r in range(n):
            if not self.slope[r] or opens[r] < min_open:
                continue
            if box is not None and not (box[0] <= self.sx[r] <= box[1] and box[2] <= self.sy[r] <= box[3]):
                continue
            if candidates == REACHED and int(state[r]) != 1:
                continue
            front.append(r)
        is_front = np.zeros(n, bool)
        is_front[front] = True
        label = np.full(n, NO_ROW, np.uint32)
        clusters = []
        for r0 in front:                                  # ascending: a component is found from its smallest row
            if label[r0] != NO_ROW:
                continue
            members, queue = [], deque([r0])
            label[r0] = r0
            while queue:
                a = queue.popleft()
                members.append(a)
                x, y, z = self.sx[a], self.sy[a], self.sz[a]
                for dx in (-1, 0, 1):
                    for dy in (-1, 0, 1):
                        if dx == 0 and dy == 0:
                            continue
                        nx, ny = (step(x, dx) if dx else x), (step(y, dy) if dy else y)
                        for t in self.cols.get((nx, ny), ()):
                            if is_front[t] and label[t] == NO_ROW and abs(lin(self.sz[t]) - lin(z)) <= link_dz:
                                label[t] = r0
                                queue.append(t)
            rec = np.zeros((), RECORD)
            rec["label"], rec["size"] = r0, len(members)
            hb = (lambda r: int(h_bits[r])) if candidates == REACHED else (lambda r: FLT_MAX_BITS)
            best = min(members, key=lambda r: (hb(r), r))
            rec["best_row"] = best
            rec["best_h"] = np.array([hb(best)], np.uint32).view(np.float32)[0]
            xs, ys = [self.sx[r] for r in members], [self.sy[r] for r in members]
            rec["sx_min"], rec["sx_max"], rec["sy_min"], rec["sy_max"] = min(xs), max(xs), min(ys), max(ys)
            rec["sum_px"], rec["sum_py"] = sum(lin(v) for v in xs), sum(lin(v) for v in ys)
            rec["sum_pz"] = sum(lin(self.sz[r]) for r in members)
            rec["open_sides"] = sum(int(opens[r]) for r in members)
            clusters.append(rec)
        records = np.zeros(len(clusters), RECORD)
        for i, rec in enumerate(clusters):
            records[i] = rec
        return dict(label=label, open=np.where(is_front, opens, 0), rows=len(front), clusters=records)


def listed(ref, min_size=1):
    """the clusters of `ref` the call lists, and its four counts"""
    keep = ref["clusters"][ref["clusters"]["size"] >= max(int(min_size), 1)]
    return keep, np.array([len(keep), ref["rows"], len(ref["clusters"]), 0], np.uint32)


def same_records(got, want):
    """bytes for bytes (best_h as its bit pattern)"""
    return got.shape == want.shape and got.tobytes() == want.tobytes()


def diff_records(got, want):
    """what differs, for an assertion's message"""
    if got.shape != want.shape:
        return f"{got.shape[0]} records, want {want.shape[0]}"
    for k in RECORD.names:
        bad = np.flatnonzero(got[k].view(np.uint32 if RECORD[k].itemsize == 4 else np.uint64) != want[k].view(np.uint32 if RECORD[k].itemsize == 4 else np.uint64))
        if len(bad):
            return f"{k}: records {bad[:5]} got {got[k][bad[:5]]} want {want[k][bad[:5]]}"
    return ""


# ---- cell-list clouds ---------------------------------------------------------------------------------------------------------------
GL, ZL, IV = 0.5, 0.25, 0.08
P = dict(grid_len=GL, z_len=ZL, slope_interval=IV, demand="slope")
ORIGIN = np.float32([0.013, -0.021, 0.05])
Z_FLOOR = 0.06          # level 1 above the origin; a storey `k` levels higher: Z_FLOOR + k * ZL


def cells_cloud(cells, seed=None):
    """9 points per cell (3 x 3 inside the cell, with a ripple so that every cell has a proper normal), in the manner of
    tests/test_planner_hand_routes._cells_to_cloud.  cells: (ix, iy) or (ix, iy, z); cell ix covers x in [ix * GL, (ix + 1) * GL), so
    its signed index is ix + 1 for ix >= 0 and ix for ix < 0: lin(sx) = ix.  The same (ix, iy) at two z draws two storeys.  seed: the
    cells in a shuffled order — row order follows first sight, so it is then unrelated to geometry."""
    cells = [tuple(c) if len(c) == 3 else (c[0], c[1], Z_FLOOR) for c in cells]
    if seed is not None:
        cells = [cells[i] for i in np.random.default_rng(seed).permutation(len(cells))]
    pts = [ORIGIN]
    for ix, iy, z in cells:
        for a in (0.12, 0.25, 0.38):
            for b in (0.12, 0.25, 0.38):
                x, y = ix * GL + a, iy * GL + b
                pts.append([x, y, z + 0.002 * np.sin(7 * x) * np.cos(5 * y)])
    return np.ascontiguousarray(np.float32(pts))


def serpentine(half=32, connectors=True):
    """one-cell-wide lines on every second y of a (2 half + 1)^2 area centred on the origin, joined alternately at the ends"""
    cells = [(ix, iy) for iy in range(-half, half + 1, 2) for ix in range(-half, half + 1)]
    if connectors:
        cells += [(half if k % 2 == 0 else -half, iy) for k, iy in enumerate(range(-half + 1, half, 2))]
    return cells
