"""The obstacle field restated from the exported rows (include/gndt.h "obstacle field"): void, window, budget, covered and in reach by
brute force over rows x boxes (a box at a time, every row of the map), a breadth-first search over clearance_ref.Field.back for hops,
the owner by its rule — the smallest box index among the covered slopes exactly hops steps away — layer by layer of that search, and
the counts.  owner_by_search is a second owner from one forward search per row.  Shares no code with
grid_ndt_amd/csrc/gndt_obstacle.hpp.  Test infrastructure only."""
from collections import deque

import numpy as np

BEYOND = 0xFFFFFFFF
NO_ROW = 0xFFFFFFFF
MAX_XY = 65535
# every index that exists on x or y, ascending, and its lin
EXISTS = np.concatenate([np.arange(-MAX_XY, 0), np.arange(1, MAX_XY + 1)]).astype(np.int64)
EXISTS_LIN = np.where(EXISTS > 0, EXISTS - 1, EXISTS)


def lin(v):
    v = np.asarray(v, np.int64)
    return np.where(v > 0, v - 1, v)


def axis_count(lo, hi, K):
    """how many indices that exist have lin in [lin(lo) - K, lin(hi) + K]"""
    a, b = int(lin(lo)) - K, int(lin(hi)) + K
    return int(((EXISTS_LIN >= a) & (EXISTS_LIN <= b)).sum())


def resolve(boxes, n_boxes_dev=None):
    """the boxes of a call: [n_boxes, 6] cut to B = min(n_boxes_dev, n_boxes)"""
    boxes = np.asarray(boxes, np.int64).reshape(-1, 6)
    return boxes if n_boxes_dev is None else boxes[:min(int(n_boxes_dev), len(boxes))]


def budget(boxes, inflate, max_hops, max_columns=0):
    """-> (void [B], admitted [B], dropped [B], w [B], W [B]) by rules 1 and 2"""
    max_columns = max_columns or 1 << 24
    K = inflate + max_hops
    B = len(boxes)
    void = (boxes[:, 0] > boxes[:, 1]) | (boxes[:, 2] > boxes[:, 3]) | (boxes[:, 4] > boxes[:, 5]) if B else np.zeros(0, bool)
    w = np.zeros(B, np.int64)
    for b in range(B):
        if not void[b]:
            w[b] = axis_count(boxes[b, 0], boxes[b, 1], K) * axis_count(boxes[b, 2], boxes[b, 3], K)
    W = np.cumsum(w)
    admitted = ~void & (W <= max_columns)
    return void, admitted, ~void & ~admitted, w, W


def field(f, cells, boxes, inflate=0, max_hops=8, levels_above=0, levels_below=0, max_columns=0, base=None, n_boxes_dev=None):
    """f: the clearance_ref.Field of `cells`.  -> dict(hops uint32, obstacle uint32, counts uint32 [8], covered bool [n], in_reach bool
    [n], admitted, dropped bool [B], raw_hops int64 (-1: no walk at all, no limit applied))"""
    max_hops = max_hops or 8
    boxes = resolve(boxes, n_boxes_dev)
    B, n = len(boxes), f.n
    void, admitted, dropped, w, W = budget(boxes, inflate, max_hops, max_columns)
    lx, ly, lz = (lin(np.asarray(cells[k][:n])) for k in ("sx", "sy", "sz"))
    K = inflate + max_hops
    owner0 = np.full(n, -1, np.int64)                     # the least admitted box that covers the row
    in_reach = np.zeros(n, bool)
    covering = 0
    by_x = np.argsort(lx, kind="stable")                  # (the rows ordered by x: a box is compared with the rows of its x range only)
    xs = lx[by_x]
    for b in np.flatnonzero(admitted)[::-1]:              # descending: the least index is written last
        x0, x1, y0, y1, z0, z1 = (int(v) for v in lin(boxes[b]))
        r = by_x[np.searchsorted(xs, x0 - K, "left"):np.searchsorted(xs, x1 + K, "right")]
        r = r[f.slope[r] & (ly[r] >= y0 - K) & (ly[r] <= y1 + K)]
        in_reach[r] = True
        cov = r[(lx[r] >= x0 - inflate) & (lx[r] <= x1 + inflate) & (ly[r] >= y0 - inflate) & (ly[r] <= y1 + inflate) &
                (z0 <= lz[r] + levels_above) & (z1 >= lz[r] - levels_below)]
        covering += bool(len(cov))
        owner0[cov] = b
    covered = owner0 >= 0
    hops = np.full(n, -1, np.int64)
    owner = owner0.copy()
    src = np.flatnonzero(covered)
    hops[src] = 0
    queue, order = deque(src.tolist()), []
    while queue:                                           # reversed graph: who steps INTO p is one further away
        p = queue.popleft()
        order.append(p)
        for q in f.back[p]:
            if hops[q] < 0:
                hops[q] = hops[p] + 1
                queue.append(q)
    for q in order:                                        # ascending hops
        if hops[q] > 0:
            owner[q] = min(int(owner[p]) for p in f.steps[q] if hops[p] == hops[q] - 1)
    ok = (hops >= 0) & (hops <= max_hops)
    out_hops = np.where(ok, hops, BEYOND).astype(np.uint32)
    merged = out_hops
    if base is not None:                                   # (a clearance field's hops, as uint32 or as the int32 the wrappers hand out)
        bs = np.asarray(base)
        merged = np.minimum(bs.view(np.uint32) if bs.dtype == np.int32 else bs.astype(np.uint32), out_hops)
    counts = np.zeros(8, np.uint32)
    counts[3] = B
    if n and B:
        counts[:3] = int(covered.sum()), int(ok.sum()), int(hops[ok].max()) if ok.any() else 0
        counts[4:7] = covering, int(in_reach.sum()), int(dropped.sum())
    return dict(hops=merged, obstacle=np.where(ok, owner, NO_ROW).astype(np.uint32), counts=counts, covered=covered, in_reach=in_reach,
                admitted=admitted, dropped=dropped, raw_hops=hops, own_hops=out_hops, W=W, w=w)


def owner_by_search(f, covered_owner):
    """covered_owner: int64 [n], the least covering box of a covered slope, -1 elsewhere.  Per slope one forward search: the least
    owner in the first layer that holds a covered slope (-1: no walk)."""
    out = np.full(f.n, -1, np.int64)
    for q in np.flatnonzero(f.slope):
        layer, seen = {int(q)}, {int(q)}
        while layer:
            hit = [int(covered_owner[r]) for r in layer if covered_owner[r] >= 0]
            if hit:
                out[q] = min(hit)
                break
            layer = {t for r in layer for t in f.steps[r]} - seen
            seen |= layer
    return out
