"""CPU tier: the route field's per-row code (grid_ndt_amd/csrc/gndt_route_field.hpp: weights, seeds, the sides' first steps, the
sweeps over packed keys, the finish, the descent), compiled with g++ into tests/_route_field_shim.so and run one row after another —
as copy-to-copy sweeps and in place in both row orders — against the restatement from the rows (tests/route_field_ref.py: Dijkstra
with fp32 additions on clearance_ref.Field's edges) on maps the oracle builds, on 240 random cell tables with random goals, hops,
penalties and cuts, and on a column taller than the step mask: cost bits, next and counts 0-4 for equality; the field's properties on
every map; what is promised of a call that ran out of sweeps; and the product entry points refuse to run without a GPU."""
import ctypes as C

import numpy as np
import pytest

from tests import clearance_ref as cr
from tests import route_field_ref as rr
from tests.host_emulation import MAP, load_shim
from tests.test_clearance_host import FUZZ_ROBOT, MARGIN, Table, _map, lattice_field, random_table, tall_corridor
from tests.test_raster_host import SCENES

_shim = None
MODES = (0, 1, 2)


def shim():
    global _shim
    if _shim is None:
        vp, u32 = C.c_void_p, C.c_uint32
        _shim = load_shim("route_field_shim.cpp", "_route_field_shim.so", {
            "rfshim_lds_rows": ([], u32),
            "rfshim_field": ([C.c_int, vp, vp, vp, MAP, vp, u32, vp, vp, vp, vp, vp], C.c_int),
            "rfshim_descend": ([MAP, C.c_int, u32, vp, vp, vp, u32, u32, vp, u32, vp], C.c_int),
        })
    return _shim


def run(t, goals, goal_costs=None, robot=None, hops=None, min_hops=0, soft_hops=0, soft_weight=0.0, overhead=False, max_cost=0.0, max_rounds=0,
        mode=0):
    """the shim's passes on t (a Table, or a HostMap) -> dict(cost, next, counts)"""
    rb = dict(cr.ROBOT)
    rb.update(robot or {})
    r4 = np.array([rb["radius"], rb["reachable_height"], rb["max_rough"], rb["max_angle_deg"]], np.float32)
    rule = np.array([1 if overhead else 0, min_hops, soft_hops, max_rounds], np.uint32)
    fr = np.array([soft_weight, max_cost], np.float32)
    n = t.n
    g = np.ascontiguousarray(np.asarray(goals).astype(np.int64) & 0xFFFFFFFF, np.uint32)
    gc = None if goal_costs is None else np.ascontiguousarray(goal_costs, np.float32)
    hp = None if hops is None else np.ascontiguousarray(hops, np.uint32)
    cost = np.full(max(n, 1), np.float32(-7.0), np.float32)
    nxt = np.full(max(n, 1), 0xDEADBEEF, np.uint32)
    counts = np.full(8, 0xDEADBEEF, np.uint32)
    p = lambda a: None if a is None else a.ctypes.data
    rc = shim().rfshim_field(mode, p(r4), p(rule), p(fr), t.shim_map(), p(g), len(g), p(gc), p(hp), p(cost), p(nxt), p(counts))
    assert rc == 0 and counts[6] == 0 and counts[7] == 0
    return dict(cost=cost[:n], next=nxt[:n], counts=counts)


def same(got, want, what):
    assert np.array_equal(got["counts"][:5], want["counts"][:5]), (what, got["counts"], want["counts"])
    for k in ("cost", "next"):
        a, b = got[k].view(np.uint32), want[k].view(np.uint32)
        assert np.array_equal(a, b), (what, k, np.flatnonzero(a != b)[:8], got[k][a != b][:8], want[k][a != b][:8])


def chain_steps(nxt, fin):
    """steps to the end of the chain of next for every row of `fin`; asserts that no chain repeats a row"""
    n = len(nxt)
    steps = np.full(n, -1, np.int64)
    for q0 in np.flatnonzero(fin).tolist():
        chain, q = [], q0
        while steps[q] < 0 and nxt[q] != rr.NO_ROW:
            chain.append(q)
            q = int(nxt[q])
            assert len(chain) <= n, "next runs in a circle"
        if steps[q] < 0:
            steps[q] = 0
        for i, r in enumerate(reversed(chain)):
            steps[r] = steps[q] + i + 1
    return steps


def properties(r, got, what):
    """what holds at the fixed point on every map (r: the restatement's graph, weights and seeds; got: the kernels' answer)"""
    cost, nxt = got["cost"], got["next"]
    fin = cost != rr.FLT_MAX
    assert np.array_equal(fin, nxt != rr.NO_ROW) or (np.isfinite(r.seed) & fin & (nxt == rr.NO_ROW)).any(), what
    assert not fin[~r.f.slope].any(), what
    # cost[q] == fl(c(q, next[q]) + cost[next[q]]), next[q] a step of q that may be entered
    edge = {(a, b): c for a, b, c in zip(r.eq.tolist(), r.et.tolist(), r.ec.tolist())}
    for q in np.flatnonzero(fin & (nxt != rr.NO_ROW)).tolist():
        t = int(nxt[q])
        assert (q, t) in edge and np.float32(np.float32(edge[(q, t)]) + cost[t]) == cost[q], (what, q, t)
    ends = fin & (nxt == rr.NO_ROW)
    assert np.array_equal(cost[ends], r.seed[ends].astype(np.float32)) and np.isfinite(r.seed[ends]).all(), what
    # no step that may be taken improves a key
    key = (rr.bits(cost).astype(np.uint64) << np.uint64(32)) | nxt.astype(np.uint64)
    live = fin[r.et]
    with np.errstate(over="ignore"):
        s = (r.ec[live] + cost[r.et[live]]).astype(np.float32)
    good = (s < rr.FLT_MAX) & ~((r.max_cost > 0) & (s > r.max_cost))
    cand = (rr.bits(s[good]).astype(np.uint64) << np.uint64(32)) | r.et[live][good].astype(np.uint64)
    assert (key[r.eq[live][good]] <= cand).all(), what
    # descending from every finite row ends on an accepted goal in fewer than num_slopes steps
    steps = chain_steps(nxt, fin)
    assert (steps[fin] < max(int(r.f.slope.sum()), 1)).all(), what
    return int(steps.max()) if fin.any() else 0


def promises(r, got, full, what):
    """what is promised of a call that ran out of sweeps (full: the fixed point)"""
    cost, nxt = got["cost"], got["next"]
    fin = cost != rr.FLT_MAX
    assert (cost[fin] >= full["cost"][fin]).all() and (full["cost"][fin] != rr.FLT_MAX).all(), what
    chain_steps(nxt, fin)
    for q in np.flatnonzero(fin).tolist():
        rows, v = rr.chain_cost(r.mean, r.w, cost, nxt, q, r.n)
        assert np.isfinite(r.seed[rows[-1]]) and cost[rows[-1]] == np.float32(r.seed[rows[-1]]), (what, q)
        assert v <= cost[q], (what, q, v, cost[q])


def pick_goals(rng, f, count):
    slopes = np.flatnonzero(f.slope)
    return rng.choice(slopes, size=min(count, len(slopes)), replace=False)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_oracle_scenes_goals_hops_and_checks(name):
    t, f = _map(name)
    assert f.angle_margin_deg > MARGIN, f.angle_margin_deg
    rng = np.random.default_rng(7)
    hops = f.clearance(cr.BLOCKED, 32)["hops"]
    finite = 0
    for case in range(6):
        goals = pick_goals(rng, f, 1 + case % 3)
        kw = [dict(), dict(hops=hops, min_hops=1), dict(hops=hops, soft_hops=3, soft_weight=0.5), dict(overhead=True),
              dict(hops=hops, min_hops=2, soft_hops=4, soft_weight=2.0, overhead=True), dict(max_cost=3.0)][case]
        gc = None if case % 2 == 0 else rng.uniform(0.0, 2.0, len(goals)).astype(np.float32)
        r = rr.Route(f, t.cells, goals, gc, **kw)
        for mode in MODES:
            got = run(t, goals, gc, mode=mode, **kw)
            same(got, r.answer(), (name, case, mode))
        properties(r, got, (name, case))
        finite += int(r.counts[2])
    assert finite > 0


def test_fuzz_240_random_cell_tables():
    rng = np.random.default_rng(20241020)
    skipped = one_way = cut_by_hops = penalty_turns = ties = ignored = finite = 0
    tables = 240
    for k in range(tables):
        t = random_table(rng)
        if k % 4 == 0:                                # level floors: walks of the same steps in another order cost the same to the bit
            mean = t.mean.reshape(-1, 3).copy()
            mean[:, 2] = np.where(t.sz > 0, t.sz - 1, t.sz) * 0.25 + 0.05
            t = Table(t.sx, t.sy, t.sz, t.flags, t.row_ncol, mean, t.normal.reshape(-1, 3), t.rough)
        f = cr.Field(t.cells, FUZZ_ROBOT)
        if f.angle_margin_deg <= MARGIN:
            skipped += 1
            continue
        hops = f.clearance(cr.BLOCKED, 32)["hops"]
        goals = pick_goals(rng, f, int(rng.integers(1, 5)))
        if rng.random() < 0.2:                        # a goal that is ignored: out of range, or a row without a slope
            bad = [t.n + 5] + np.flatnonzero(~f.slope)[:1].tolist()
            goals = np.concatenate([goals, bad])
        gc = None if rng.random() < 0.4 else rng.choice([0.0, 0.25, 1.0, 3.5], len(goals)).astype(np.float32)
        kw = dict(min_hops=int(rng.integers(0, 4)), soft_hops=int(rng.choice([0, 2, 3])), soft_weight=float(rng.choice([0.0, 0.5, 1.0])),
                  overhead=bool(rng.random() < 0.5), max_cost=float(rng.choice([0.0, 0.0, 2.5, 6.0])))
        use_hops = hops if rng.random() < 0.8 else None
        r = rr.Route(f, t.cells, goals, gc, hops=use_hops, **kw)
        want = r.answer()
        for mode in MODES:
            got = run(t, goals, gc, robot=FUZZ_ROBOT, hops=use_hops, mode=mode, **kw)
            same(got, want, (k, mode, kw))
        properties(r, got, (k, kw))
        # the restatement alone: the fuzz cannot pass on empty or trivial answers
        edges = set(zip(f.edge_from.tolist(), f.edge_to.tolist()))
        one_way += int(any((b, a) not in edges for a, b in edges))
        free = rr.Route(f, t.cells, goals, gc, hops=None, min_hops=0, overhead=kw["overhead"], max_cost=kw["max_cost"])
        cut_by_hops += int(use_hops is not None and kw["min_hops"] > 0 and int(free.counts[2]) > int(r.counts[2]))
        if use_hops is not None and kw["soft_hops"] and kw["soft_weight"] > 0:
            plain = rr.Route(f, t.cells, goals, gc, hops=use_hops, min_hops=kw["min_hops"], overhead=kw["overhead"], max_cost=kw["max_cost"])
            both = r.finite & plain.finite
            penalty_turns += int((r.next[both] != plain.next[both]).any())
        # an equal-cost tie that the smallest row decides: two steps of a row whose candidates have the same cost bits
        fin = r.finite[r.et]
        with np.errstate(over="ignore"):
            s = (r.ec[fin] + r.cost[r.et[fin]]).astype(np.float32)
        at_least = s == r.cost[r.eq[fin]]
        ties += int((np.bincount(r.eq[fin][at_least], minlength=r.n) > 1).any())
        ignored += int(r.counts[1])
        finite += int(r.counts[2])
    assert skipped <= tables * 5 // 100, skipped
    print("fuzz:", dict(skipped=skipped, one_way=one_way, cut_by_hops=cut_by_hops, penalty_turns=penalty_turns, ties=ties, ignored=ignored,
                        finite=finite))
    assert one_way > tables // 2 and cut_by_hops > 10 and penalty_turns > 10 and ties > 10 and ignored > 10 and finite > 20 * tables


def test_a_step_through_a_column_taller_than_the_step_mask():
    t = tall_corridor()
    f = cr.Field(t.cells)
    slopes = np.flatnonzero(f.slope)
    assert t.row_ncol[slopes[2] - 35] == 40                      # column 3's slope is its 36th node: beyond its neighbours' step masks
    for goal in (slopes[0], slopes[4]):
        r = rr.Route(f, t.cells, [goal])
        for mode in MODES:
            got = run(t, [goal], mode=mode)
            same(got, r.answer(), ("tall", int(goal), mode))
        properties(r, got, "tall")
    # from column 1 the walk to column 5 crosses the tall column both into and out of it; column 6 stands a metre higher: no walk
    got = run(t, [slopes[4]])
    assert [int(v) for v in got["next"][slopes]] == [slopes[1], slopes[2], slopes[3], slopes[4], rr.NO_ROW, rr.NO_ROW]
    assert got["cost"][slopes[5]] == rr.FLT_MAX and tuple(got["counts"][:5]) == (1, 0, 5, rr.bits(got["cost"][slopes[0]]), 1)


_lat = {}


def lattice_route(name):
    """a lattice through the oracle with the goal on the slope deepest inside (most BLOCKED hops, the smallest such row)"""
    if name not in _lat:
        if name == 156:
            from tests.host_emulation import HostMap
            m = HostMap(cr.corridor_cloud(), cr.CORRIDOR_P, seed=13)
            t, cells, f = m, m.cells, cr.Field(m.cells)
        else:
            cells, f = lattice_field(name)
            t = Table(cells["sx"], cells["sy"], cells["sz"], cells["flags"], np.ones(f.n), cells["mean"], cells["normal"], cells["rough"])
        hops = f.clearance(cr.BLOCKED, 1024)["hops"]
        inside = np.where(hops == cr.BEYOND, 0, hops)
        _lat[name] = (t, cells, f, hops, int(np.argmax(inside)))
    return _lat[name]


@pytest.mark.parametrize("name,finite,deep", [(156, 84, 12), (1025, 1022, 64), ("41x25", 1003, 60)])
def test_lattices_finite_slopes_depth_and_sweeps(name, finite, deep):
    t, cells, f, hops, goal = lattice_route(name)
    assert f.angle_margin_deg >= 27.9
    r = rr.Route(f, cells, [goal])
    L = r.depth()
    assert int(r.counts[2]) == finite and L >= deep, (r.counts, L)
    got = run(t, [goal], mode=0, max_rounds=L + 1)              # L + 1 copy-to-copy sweeps: L to reach the deepest row, one to see it
    same(got, r.answer(), (name, "L + 1"))
    assert properties(r, got, name) == L and got["counts"][5] == L
    short = run(t, [goal], mode=0, max_rounds=L)
    assert short["counts"][4] == 0 and np.array_equal(short["cost"], r.cost)
    for mode in (1, 2):                                        # in place: never more sweeps
        got = run(t, [goal], mode=mode, max_rounds=L + 1)
        same(got, r.answer(), (name, mode))
        assert got["counts"][5] <= L
    if name == 156:
        for min_hops, left in ((1, 84), (2, 60), (3, 36)):
            rh = rr.Route(f, cells, [goal], hops=hops, min_hops=min_hops)
            assert int(rh.counts[2]) == left, (min_hops, rh.counts)
            same(run(t, [goal], hops=hops, min_hops=min_hops), rh.answer(), (name, min_hops))


def test_out_of_sweeps_the_three_promises_hold():
    t, cells, f, hops, _ = lattice_route(1025)
    slopes = np.flatnonzero(f.slope)
    # the goal on the highest-numbered slope: relaxing in ascending row order carries a key one step a sweep (descending order would
    # carry it through the map in one, so that order gets the lowest-numbered slope)
    for mode, goal in ((0, int(slopes[-1])), (1, int(slopes[-1])), (2, int(slopes[0]))):
        r = rr.Route(f, cells, [goal])
        assert r.depth() >= 60
        got = run(t, [goal], mode=mode, max_rounds=2)
        assert got["counts"][4] == 0 and got["counts"][5] == 2 and 0 < got["counts"][2] < r.counts[2], (mode, got["counts"])
        promises(r, got, r.answer(), mode)


def test_goals_that_are_ignored_and_empty_calls():
    t, cells, f, hops, goal = lattice_route(156)
    n = t.n
    closed = int(np.flatnonzero(hops == 0)[0])
    goals = [goal, n, 0xFFFFFFFF, closed, goal, goal, goal]
    gc = np.float32([1.0, 0.0, 0.0, 0.0, np.inf, -1.0, np.nan])
    r = rr.Route(f, cells, goals, gc, hops=hops, min_hops=1)
    assert tuple(r.counts[:2]) == (1, 6)
    same(run(t, goals, gc, hops=hops, min_hops=1), r.answer(), "ignored")
    twice = run(t, [goal, goal], np.float32([2.0, -0.0]))        # the same row twice keeps its least cost; -0 is 0
    assert twice["counts"][0] == 2 and rr.bits(twice["cost"][goal]) == 0 and twice["next"][goal] == rr.NO_ROW
    none = run(t, [])
    assert tuple(none["counts"]) == (0, 0, 0, 0, 1, 0, 0, 0) and (none["cost"] == rr.FLT_MAX).all() and (none["next"] == rr.NO_ROW).all()


def descend(t, cost, nxt, starts, route_cap, max_steps=0, node=False):
    starts = np.ascontiguousarray(starts, np.float32)
    K = len(starts)
    rows = np.full(K * route_cap + 3, 0xDEADBEEF, np.uint32)
    info = np.full((K + 1, 8), 0xDEADBEEF, np.uint32)
    cost, nxt = np.ascontiguousarray(cost, np.float32), np.ascontiguousarray(nxt, np.uint32)
    rc = shim().rfshim_descend(t.shim_map(), int(node), max_steps, cost.ctypes.data, nxt.ctypes.data, starts.ctypes.data, starts.shape[1], K,
                               rows.ctypes.data if route_cap else None, route_cap, info.ctypes.data)
    assert rc == 0 and (rows[K * route_cap:] == 0xDEADBEEF).all() and (info[K] == 0xDEADBEEF).all()
    return rows[:K * route_cap].reshape(K, route_cap), info[:K]


def test_descend_is_the_chain_of_next_with_its_guards():
    t, cells, f, hops, goal = lattice_route(156)
    r = rr.Route(f, cells, [goal], hops=hops, min_hops=2)
    mean = np.asarray(cells["mean"], np.float32).reshape(-1, 3)
    starts = np.concatenate([mean[:t.n], [[1e6, 0, 0], [np.nan, 0, 0]]]).astype(np.float32)
    want_row = np.concatenate([np.arange(t.n), [-1, -1]])
    L = r.depth()
    seen = set()
    for cap, max_steps in ((L + 1, 0), (3, 0), (L + 1, L), (L + 1, L - 1), (0, 0)):
        rows, info = descend(t, r.cost, r.next, starts, cap, max_steps)
        for k, q in enumerate(want_row.tolist()):
            st, ln, wr, ex, c, hs = rr.descend(r.cost, r.next, q, cap, max_steps)
            assert tuple(info[k][:5]) == (st, ln, q & 0xFFFFFFFF, ex, 0) and info[k][7] == 0, (cap, max_steps, k, info[k])
            assert info[k][5] == rr.bits(c) and info[k][6] == rr.bits(hs) and np.array_equal(rows[k], wr), (cap, max_steps, k)
            seen.add(st)
    assert seen == {rr.FOUND, rr.NO_START, rr.NO_ROUTE, rr.LIMIT}
    # a corrupted next: a circle and an entry out of range end with LIMIT, and nothing outside the arrays is read or written
    bad = r.next.copy()
    far = int(np.argmax(r.steps))
    a, b = far, int(r.next[far])
    bad[b] = a
    rows, info = descend(t, r.cost, bad, mean[[a]], 8, 50)
    assert info[0][0] == rr.LIMIT and info[0][1] == 0 and info[0][3] == 50 and (rows == rr.NO_ROW).all()
    bad[b] = t.n
    rows, info = descend(t, r.cost, bad, mean[[a]], 8)
    assert info[0][0] == rr.LIMIT and info[0][3] == 1 and (rows == rr.NO_ROW).all()


def test_the_one_workgroup_limit_is_a_lattice():
    W, H, _ = rr.LATTICES[rr.LDS_ROWS]
    assert shim().rfshim_lds_rows() == rr.LDS_ROWS == W * H and rr.LDS_ROWS * 8 + 64 <= 160 * 1024
    W, H, _ = rr.LATTICES[rr.LDS_ROWS + 1]
    assert W * H == rr.LDS_ROWS + 1


def test_no_cpu_fallback_for_the_route_field(native_lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import grid_ndt_amd as g
    m = g.TwoDmap(0.5, 0.5)
    m.setCloudFirst((0, 0, 0))
    with pytest.raises(g.GndtError) as e:
        m.route_field(np.zeros(1, np.int32), host=True)
    assert e.value.code == 2   # GNDT_ERR_NO_DEVICE
    with pytest.raises(g.GndtError) as e:
        m.descend_routes(np.zeros((1, 3), np.float32), dict(cost=np.zeros(0, np.float32), next=np.zeros(0, np.int32)), host=True)
    assert e.value.code == 2
