"""The route field restated from the exported rows (include/gndt.h "route field"): the step graph of tests/clearance_ref.Field
(edge_from / edge_to: a column dict and the flood's gates in numpy), the travel cost as fp32 differences, fp64 squares and root rounded
once, and Dijkstra's algorithm with fp32 additions on the reversed graph — valid because fl(c + a) is monotone in a and never below a —
then `next` by its rule: the smallest row among the steps that give the least cost.  Also `descend`, the chain of next.  Shares no code
with grid_ndt_amd/csrc/gndt_route_field.hpp.  Test infrastructure only."""
import heapq

import numpy as np

from tests import clearance_ref as cr

NO_ROW = 0xFFFFFFFF
FLT_MAX = np.finfo(np.float32).max
FOUND, NO_START, NO_ROUTE, LIMIT = 0, 1, 2, 3
LDS_ROWS = 20448             # kRouteLdsRows: 144 x 142

# The lattices of the kernel-edge tests that clearance_ref.LATTICES does not hold: the one-workgroup kernel's limit and the first size
# beyond it, (W, H, walls) as there.  The wall stands across most of the map, so that the least-cost walks go round its ends.
LATTICES = {
    20448: (144, 142, cr.wall([70], range(0, 120))),
    20449: (143, 143, cr.wall([70], range(0, 120))),
}


def lattice(name, P=None):
    W, H, walls = LATTICES[name] if name in LATTICES else cr.LATTICES[name]
    return cr.lattice_cloud(W, H, walls, P)


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def travel(mean, q, t):
    """TravelCost(mean q, mean t) for arrays of rows: fp32 differences, squares and root in fp64, rounded to fp32 once"""
    d = (mean[q] - mean[t]).astype(np.float32).astype(np.float64)
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(np.float32)


class Route:
    """The field for one set of goals and one rule, on the step graph `f` (a clearance_ref.Field of the same cells)."""

    def __init__(self, f, cells, goals, goal_costs=None, hops=None, min_hops=0, soft_hops=0, soft_weight=0.0, overhead=False, max_cost=0.0):
        n = self.n = f.n
        self.f = f
        mean = self.mean = np.asarray(cells["mean"], np.float32).reshape(-1, 3)[:n]
        hp = None if hops is None else np.asarray(hops).astype(np.int64) & 0xFFFFFFFF
        enter = f.slope.copy()
        if hp is not None:
            enter &= hp >= min_hops
        if overhead:
            enter &= ~f.overhead
        w = np.ones(n, np.float32)
        if hp is not None and soft_hops:
            soft = hp < soft_hops
            pen = np.float32(soft_weight) * (soft_hops - hp[soft]).astype(np.float32)
            w[soft] = np.float32(1.0) + pen.astype(np.float32)
        self.enter, self.w = enter, w
        q, t = f.edge_from, f.edge_to
        keep = enter[t]
        self.eq, self.et = q[keep], t[keep]
        with np.errstate(over="ignore"):
            self.ec = (travel(mean, self.eq, self.et) * w[self.et]).astype(np.float32)
        self.max_cost = np.float32(max_cost)
        # goals
        goals = np.asarray(goals).astype(np.int64) & 0xFFFFFFFF
        gc = np.zeros(len(goals), np.float32) if goal_costs is None else np.asarray(goal_costs, np.float32)
        seed = np.full(n, np.inf)
        self.accepted = self.ignored = 0
        for g, c in zip(goals.tolist(), gc.tolist()):
            if g >= n or not enter[g] or not np.isfinite(c) or c < 0:
                self.ignored += 1
                continue
            self.accepted += 1
            seed[g] = min(seed[g], float(np.float32(abs(c) if c == 0 else c)))
        self.seed = seed
        self._solve()

    def _ok(self, s):
        return s < FLT_MAX and not (self.max_cost > 0 and s > self.max_cost)

    def _solve(self):
        n = self.n
        back = [[] for _ in range(n)]
        for i, t in enumerate(self.et.tolist()):
            back[t].append(i)
        dist = np.full(n, np.inf)
        heap = []
        for g in np.flatnonzero(np.isfinite(self.seed)).tolist():
            dist[g] = self.seed[g]
            heapq.heappush(heap, (dist[g], g))
        eq, ec = self.eq.tolist(), self.ec
        done = np.zeros(n, bool)
        while heap:
            d, t = heapq.heappop(heap)
            if done[t] or d != dist[t]:
                continue
            done[t] = True
            dt = np.float32(d)
            for i in back[t]:
                with np.errstate(over="ignore"):
                    s = np.float32(ec[i] + dt)
                if self._ok(s) and s < dist[eq[i]]:
                    dist[eq[i]] = float(s)
                    heapq.heappush(heap, (float(s), eq[i]))
        fin = np.isfinite(dist)
        self.cost = np.where(fin, dist, FLT_MAX).astype(np.float32)
        # next: the least (cost, row) among the steps, against the seed (whose low word is NO_ROW: a step at the same cost wins)
        key = np.where(np.isfinite(self.seed), (bits(np.where(np.isfinite(self.seed), self.seed, 0)).astype(np.uint64) << np.uint64(32)) | np.uint64(NO_ROW),
                       np.uint64(0xFFFFFFFFFFFFFFFF))
        live = fin[self.et]
        with np.errstate(over="ignore"):
            s = (self.ec[live] + self.cost[self.et[live]]).astype(np.float32)
        good = s < FLT_MAX
        if self.max_cost > 0:
            good &= ~(s > self.max_cost)
        cand = (bits(s[good]).astype(np.uint64) << np.uint64(32)) | self.et[live][good].astype(np.uint64)
        np.minimum.at(key, self.eq[live][good], cand)
        self.key = key
        assert np.array_equal((key >> np.uint64(32)).astype(np.uint32)[fin], bits(self.cost)[fin]) and (key[~fin] == np.uint64(0xFFFFFFFFFFFFFFFF)).all()
        self.next = np.where(fin, (key & np.uint64(0xFFFFFFFF)).astype(np.uint32), NO_ROW).astype(np.uint32)
        self.finite = fin
        self.counts = np.array([self.accepted, self.ignored, int(fin.sum()), int(bits(self.cost)[fin].max()) if fin.any() else 0, 1], np.uint32)

    def answer(self):
        return dict(cost=self.cost, next=self.next, counts=self.counts)

    def depth(self):
        """L: the steps of the deepest chain of next"""
        steps = np.full(self.n, -1, np.int64)
        for q0 in np.flatnonzero(self.finite).tolist():
            chain, q = [], q0
            while steps[q] < 0 and self.next[q] != NO_ROW:
                chain.append(q)
                q = int(self.next[q])
                assert len(chain) <= self.n, "next runs in a circle"
            if steps[q] < 0:
                steps[q] = 0
            for i, r in enumerate(reversed(chain)):
                steps[r] = steps[q] + i + 1
        self.steps = steps
        return int(steps.max()) if self.finite.any() else 0


def chain_cost(mean, w, cost, nxt, q, limit):
    """Follow next from q: -> (rows of the chain, the cost recomputed from its end backwards with the end's own stored cost as v(g)).
    Raises if a row repeats or the chain exceeds `limit` rows."""
    rows = [q]
    seen = {q}
    while nxt[rows[-1]] != NO_ROW:
        t = int(nxt[rows[-1]])
        assert t not in seen and len(rows) <= limit, (rows[:8], t)
        rows.append(t)
        seen.add(t)
    v = np.float32(cost[rows[-1]])
    for p, t in zip(rows[-2::-1], rows[:0:-1]):
        c = np.float32(travel(mean, np.array([p]), np.array([t]))[0] * w[t])
        v = np.float32(c + v)
    return rows, v


def descend(cost, nxt, start, route_cap, max_steps=0):
    """gndt_descend_routes for one start row (-1 / NO_ROW: none) -> (status, length, rows [route_cap], expansions, cost, h_start)"""
    n = len(cost)
    max_steps = max_steps or 65536
    rows = np.full(route_cap, NO_ROW, np.uint32)
    if start in (-1, NO_ROW):
        return NO_START, 0, rows, 0, FLT_MAX, FLT_MAX
    if cost[start] == FLT_MAX:
        return NO_ROUTE, 0, rows, 0, FLT_MAX, FLT_MAX
    chain, q, steps = [start], start, 0
    while True:
        nx = int(nxt[q]) & 0xFFFFFFFF
        if nx == NO_ROW:
            break
        if nx >= n or steps == max_steps:
            return LIMIT, 0, rows, steps, FLT_MAX, cost[start]
        steps += 1
        q = nx
        chain.append(q)
    m = min(len(chain), route_cap)
    rows[:m] = chain[:m]
    return FOUND, len(chain), rows, steps, cost[start], cost[start]
