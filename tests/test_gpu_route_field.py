"""GPU tier: the route field (gndt_route_field_device / gndt_route_field, gndt_descend_routes_device / gndt_descend_routes,
TwoDmap.route_field / descend_routes).  Every map is built on the device; cost bits, next and counts 0-4 are compared for equality with
the restatement (tests/route_field_ref.py) on the handle's own export, every scene once with the one-workgroup kernel allowed and once
without it, and the two answers byte for byte.  Outputs are sentinel-padded.  A corridor with a box across it through obstacle_field,
two storeys, the site with the frontiers' goals and against the planner, lattices with exact row counts at the kernels' edges, the
descent at the wavefront's and the grid's edges of K and under its guards, routes straight into shortcut_routes, repeat calls, streams,
crop and update, scratch reuse, the Python interface and every refused argument.  No tolerance anywhere but in the comparison with the
planner, whose bound is the rounding of two sums of the same terms in opposite orders."""
import ctypes as C

import numpy as np
import pytest

from grid_ndt_amd import scenes
from tests import clearance_ref as cr
from tests import frontier_ref as fr
from tests import obstacle_ref as ob
from tests import route_field_ref as rr
from tests.gpu_kit import Padded, PaddedCall, build, debug_option, dev, robot_arg, to_np
from tests.gpu_kit import tails_untouched as untouched

pytestmark = pytest.mark.gpu

ERR_INVALID = 1
SENTINEL = 0x5A5A5A5A
PAD = 5                      # sentinel entries behind num_nodes
OVERHEAD = 1                 # GNDT_WALK_CHECK_OVERHEAD


def _tgc():
    from tests import test_gpu_clearance as tgc
    return tgc


def one_workgroup(on):
    """gndt_debug_set_option(GNDT_DEBUG_ROUTE_FIELD_ONE_WORKGROUP, .) for a block; the default comes back whatever happens in it"""
    return debug_option("DEBUG_ROUTE_FIELD_ONE_WORKGROUP", 1 if on else 0, 1)


def raw(m, goals, goal_costs=None, hops=None, robot=None, outs=("cost", "next"), stream=None, host=False, reserved=(0, 0), counts=True, G=None,
        checks=0, min_hops=0, soft_hops=0, soft_weight=0.0, max_cost=0.0, max_rounds=0):
    """The C entry points, every output num_nodes + PAD entries of sentinel -> (rc, dict(cost, next: the outputs asked for, cut to
    num_nodes; counts; tails: what lies behind num_nodes))"""
    from grid_ndt_amd._lib import RouteFieldParams
    n = int(m.sync()[0])
    prm = RouteFieldParams(checks, min_hops, soft_hops, soft_weight, max_cost, max_rounds, (C.c_uint32 * 2)(*reserved))
    g = np.ascontiguousarray(np.asarray(goals).astype(np.int64) & 0xFFFFFFFF, np.uint32)
    gc = None if goal_costs is None else np.ascontiguousarray(goal_costs, np.float32)
    hp = None if hops is None else np.ascontiguousarray(hops, np.uint32)
    buf = {k: Padded(n, back=PAD, fill=SENTINEL) for k in outs}
    cnt = Padded(8, fill=SENTINEL)
    rc = PaddedCall(host, stream)(m._L.gndt_route_field, m._L.gndt_route_field_device, m._h, robot_arg(robot, cr.ROBOT), C.byref(prm), g,
                                  len(g) if G is None else G, gc, hp, buf.get("cost"), buf.get("next"), cnt if counts else None)
    out = {k: p.body for k, p in buf.items()}
    out.update(counts=cnt.a, tails={k: p.tail for k, p in buf.items()})
    return rc, out


def check(m, r, goals, goal_costs=None, what="", **kw):
    """one call against the restatement r -> the call's answer"""
    rc, got = raw(m, goals, goal_costs, **kw)
    assert rc == 0, (what, m._L.gndt_last_error(m._h))
    assert np.array_equal(got["counts"][:5], r.counts) and not got["counts"][6:].any(), (what, got["counts"], r.counts)
    want = dict(cost=rr.bits(r.cost), next=r.next)
    for k in kw.get("outs", ("cost", "next")):
        assert np.array_equal(got[k], want[k]), (what, k, np.flatnonzero(got[k] != want[k])[:8], got[k][:8], want[k][:8])
    assert untouched(got), what
    return got


def both_paths(m, r, goals, goal_costs=None, what="", **kw):
    """the call with the one-workgroup kernel allowed and without it: the restatement's answer and the same bytes"""
    with one_workgroup(True):
        a = check(m, r, goals, goal_costs, what=(what, "one workgroup"), **kw)
    with one_workgroup(False):
        b = check(m, r, goals, goal_costs, what=(what, "a launch a sweep"), **kw)
    for k in ("cost", "next"):
        if k in a:
            assert a[k].tobytes() == b[k].tobytes(), (what, k)
    assert a["counts"][:5].tobytes() == b["counts"][:5].tobytes(), what
    return a


def row_at(cells, sx, sy, top=False):
    rows = np.flatnonzero((cells["sx"] == sx) & (cells["sy"] == sy) & ((cells["flags"] & 2) != 0))
    return int(rows[np.argmax(cells["mean"][rows, 2])] if top else rows[0])


def raw_descend(m, starts, cost, nxt, route_cap, max_steps=0, start_mode=0, stream=None, host=False, reserved=(0,) * 6, stride=12):
    """the C entry points with sentinel behind rows and info -> (rc, rows [K, cap], info [K, 8] uint32, untouched)"""
    from grid_ndt_amd._lib import DescendParams
    prm = DescendParams(start_mode, max_steps, (C.c_uint32 * 6)(*reserved))
    s = np.ascontiguousarray(starts, np.float32)
    if stride == 16:
        s = np.ascontiguousarray(np.concatenate([s[:, :3], np.full((len(s), 1), 7.0, np.float32)], 1))
    K = len(s)
    rows, info = Padded(K * route_cap, back=PAD, fill=SENTINEL), Padded(K, words=8, back=1, fill=SENTINEL)
    rc = PaddedCall(host, stream)(m._L.gndt_descend_routes, m._L.gndt_descend_routes_device, m._h, s, K, stride, C.byref(prm),
                                  np.ascontiguousarray(cost, np.float32), np.ascontiguousarray(nxt, np.uint32), rows if route_cap else None, route_cap,
                                  info)
    return rc, rows.body.reshape(K, route_cap), info.body.reshape(K, 8), rows.untouched() and info.untouched()


def check_descend(m, cells, r, start_rows, route_cap, max_steps=0, cost=None, nxt=None, what="", **kw):
    """starts at the means of start_rows (-1: a point off the map) against the restatement's descent, record for record"""
    cost = r.cost if cost is None else cost
    nxt = r.next if nxt is None else nxt
    start_rows = np.asarray(start_rows)
    pts = np.where(start_rows[:, None] >= 0, cells["mean"][np.maximum(start_rows, 0)], np.float32([1e6, 1e6, 0.0])).astype(np.float32)
    rc, rows, info, ok = raw_descend(m, pts, cost, nxt, route_cap, max_steps, **kw)
    assert rc == 0 and ok, (what, rc, m._L.gndt_last_error(m._h))
    memo = {}
    for k, q in enumerate(start_rows.tolist()):
        if q not in memo:
            memo[q] = rr.descend(cost, nxt, q, route_cap, max_steps)
        st, ln, wr, ex, c, hs = memo[q]
        assert tuple(info[k][:5]) == (st, ln, q & 0xFFFFFFFF, ex, 0) and info[k][7] == 0, (what, k, q, info[k])
        assert info[k][5] == rr.bits(c) and info[k][6] == rr.bits(hs) and np.array_equal(rows[k], wr), (what, k, q)
    return rows, info


# ---- the corridor with a box across it ---------------------------------------------------------------------------------------------

def corridor():
    return _tgc().drawn("corridor", cr.corridor_cloud, cr.CORRIDOR_P)


def box_hops(m, f, cells, box):
    """obstacle_field's hops for one box, asserted against tests/obstacle_ref.py first"""
    got = m.obstacle_field(np.int32([box]), max_hops=8, levels_above=0)
    hops = to_np(got["hops"]).view(np.uint32)
    assert np.array_equal(hops, ob.field(f, cells, [box], max_hops=8)["hops"])
    return hops


def test_a_box_in_the_corridor_the_way_round_no_way_round_and_the_way_out():
    m, f, cells = corridor()
    assert cells["num_nodes"] == 156 and ((cells["flags"] & 2) != 0).all()
    goal = row_at(cells, 4, 1)
    far = [row_at(cells, sx, 12) for sx in (1, 4, 6)]
    near = [row_at(cells, sx, 3) for sx in (1, 4, 7)]
    free = rr.Route(f, cells, [goal])
    both_paths(m, free, [goal], what="no box")
    assert free.finite[far].all() and int(free.counts[2]) == 84
    # the box leaves column 7 free: the routes exist, pass through the gap and cost more
    hops = box_hops(m, f, cells, [1, 6, 6, 6, 1, 1])
    assert (hops[[row_at(cells, sx, 6) for sx in range(1, 7)]] == 0).all() and hops[row_at(cells, 7, 6)] == 1
    r = rr.Route(f, cells, [goal], hops=hops, min_hops=1)
    got = both_paths(m, r, [goal], hops=hops, min_hops=1, what="gap")
    gap = row_at(cells, 7, 6)
    rows, info = check_descend(m, cells, r, far + near, 40, what="gap")
    for k in range(3):
        assert info[k][0] == rr.FOUND and gap in rows[k][:info[k][1]] and r.cost[far[k]] > free.cost[far[k]]
        assert (hops[rows[k][:info[k][1]]] >= 1).all() and rows[k][info[k][1] - 1] == goal
    assert np.array_equal(r.cost[near], free.cost[near])
    # a soft zone round the box: the routes keep further from it where they can, and cost more still
    soft = rr.Route(f, cells, [goal], hops=hops, min_hops=1, soft_hops=3, soft_weight=1.5)
    both_paths(m, soft, [goal], hops=hops, min_hops=1, soft_hops=3, soft_weight=1.5, what="soft")
    assert (soft.cost[far] > r.cost[far]).all()
    # the box across all seven columns: no way round
    hops = box_hops(m, f, cells, [1, 7, 6, 6, 1, 1])
    r = rr.Route(f, cells, [goal], hops=hops, min_hops=1)
    both_paths(m, r, [goal], hops=hops, min_hops=1, what="closed")
    rows, info = check_descend(m, cells, r, far + near, 40, what="closed")
    assert (info[:3, 0] == rr.NO_ROUTE).all() and (info[3:, 0] == rr.FOUND).all() and np.array_equal(r.cost[near], free.cost[near])
    # a start inside the forbidden zone is led out of it, on the goal's side
    inside = row_at(cells, 3, 6)
    assert hops[inside] == 0 and r.finite[inside] and hops[r.next[inside]] >= 1 and cells["sy"][r.next[inside]] == 5
    # a zone two hops deep: its rim is led out, its core has no step that may be taken
    with_zone = rr.Route(f, cells, [goal], hops=hops, min_hops=2)
    got = both_paths(m, with_zone, [goal], hops=hops, min_hops=2, what="zone")
    rim = row_at(cells, 3, 5)
    rows, info = check_descend(m, cells, with_zone, [rim, inside], 40, what="led out")
    assert hops[rim] == 1 and info[0][0] == rr.FOUND and (hops[rows[0][1:info[0][1]]] >= 2).all() and info[1][0] == rr.NO_ROUTE
    # a goal inside the zone is ignored
    r0 = rr.Route(f, cells, [inside, goal], hops=hops, min_hops=1)
    assert tuple(r0.counts[:2]) == (1, 1)
    both_paths(m, r0, [inside, goal], hops=hops, min_hops=1, what="goal in the zone")


def test_two_storeys_a_goal_on_the_bridge():
    m, f, cells = _tgc().site("bridge")
    slope = (cells["flags"] & 2) != 0
    cols = {}
    for row in np.flatnonzero(slope).tolist():
        cols.setdefault((int(cells["sx"][row]), int(cells["sy"][row])), []).append(row)
    double = [v for v in cols.values() if len(v) >= 2]
    assert len(double) > 20
    goal = max((max(v, key=lambda t: cells["mean"][t, 2]) for v in double), key=lambda t: cells["mean"][t, 2])
    r = rr.Route(f, cells, [goal])
    both_paths(m, r, [goal], what="bridge")
    both_paths(m, rr.Route(f, cells, [goal], overhead=True), [goal], checks=OVERHEAD, what="bridge, overhead")
    assert int(r.counts[2]) > 1000
    # the deck and the ground under it are different places: wherever both have a cost it differs
    both = [v for v in double if r.finite[v[0]] and r.finite[v[-1]]]
    assert all(r.cost[v[0]] != r.cost[v[-1]] for v in both)


# ---- the site ----------------------------------------------------------------------------------------------------------------------

def test_site_the_frontiers_goals_and_the_planner_on_the_same_map():
    import torch
    m, f, cells = _tgc().site("site")
    n = int(cells["num_nodes"])
    assert rr.LDS_ROWS >= n > 16000                            # the one-workgroup kernel holds the site
    assert m.computeCost(scenes.DRIVABLE_GOAL)["rc"] == 0
    fro = m.frontiers()
    goals = to_np(fro["best_row"]).astype(np.int64)
    assert len(goals) >= 3
    gc = np.linspace(0.0, 2.0, len(goals)).astype(np.float32)
    r = rr.Route(f, cells, goals, gc)
    both_paths(m, r, goals, gc, what="frontiers")
    assert int(r.counts[0]) >= 3 and int(r.counts[2]) > n // 2
    hops = f.clearance(cr.BLOCKED, 32)["hops"]
    rh = rr.Route(f, cells, goals, gc, hops=hops, min_hops=1, soft_hops=3, soft_weight=0.5, overhead=True)
    both_paths(m, rh, goals, gc, hops=hops, min_hops=1, soft_hops=3, soft_weight=0.5, checks=OVERHEAD, what="frontiers, hops")
    assert int(rh.counts[2]) < int(r.counts[2])
    # one goal, the flood's: every planned route along the field's edges costs at least what the field says, up to two sums' rounding
    goal = int(to_np(m.query(np.float32([scenes.DRIVABLE_GOAL]), "node"))[0])
    one = rr.Route(f, cells, [goal])
    got = both_paths(m, one, [goal], what="one goal")
    rng = np.random.default_rng(5)
    starts = rng.choice(np.flatnonzero(f.slope), 64, replace=False)
    prow, pinfo = m.plan_routes(cells["mean"][starts], start_mode="nearest_slope", route_cap=512, host=True)
    edges = set(zip(f.edge_from.tolist(), f.edge_to.tolist()))
    qualified = 0
    for k in range(64):
        ln = int(pinfo["length"][k])
        if int(pinfo["status"][k]) != 0 or ln > 512:
            continue
        route = prow[k][:ln].tolist()
        if not all((a, b) in edges for a, b in zip(route[:-1], route[1:])) or route[-1] != goal:
            continue
        qualified += 1
        bound = np.float64(pinfo["cost"][k]) * (1.0 + 2.0 * ln * 2.0 ** -24)
        assert one.cost[route[0]] <= bound, (k, one.cost[route[0]], pinfo["cost"][k], ln)
    assert qualified >= 1, qualified


# ---- kernel-edge shapes ------------------------------------------------------------------------------------------------------------

def lattice(name):
    if name in rr.LATTICES:
        return _tgc().drawn(("route lattice", name), lambda: rr.lattice(name, fr.P))
    return _tgc().lattice(name)


@pytest.mark.parametrize("rows", [1023, 1024, 1025, rr.LDS_ROWS, rr.LDS_ROWS + 1])
def test_lattices_at_the_slot_edges_and_the_limit_of_the_one_workgroup_kernel(rows):
    """k_route_wg's `row = threadIdx.x + j * kRouteWgThreads; if (row >= n) break` with its one-bit-a-slot `slopes`: 1023 / 1024 / 1025
    rows end a slot one thread short, exactly and one thread into the next; 20 448 rows use all the LDS the kernel may ask for with
    the flag words right behind the keys; 20 449 is the first map that takes a launch a sweep whatever the option says."""
    m, f, cells = lattice(rows)
    n = int(cells["num_nodes"])
    assert n == rows and ((cells["flags"] & 2) != 0).all()
    W, H, _ = rr.LATTICES[rows] if rows in rr.LATTICES else cr.LATTICES[rows]
    goal, mid = n - 1, row_at(cells, W // 2 + 4, H // 2 + 1)            # (clear of the wall and of the edge)
    r = rr.Route(f, cells, [goal, 0], np.float32([0.0, 40.0]))
    got = both_paths(m, r, [goal, 0], np.float32([0.0, 40.0]), what=rows)
    assert int(r.counts[2]) > n * 9 // 10 and r.depth() >= 30 and got["counts"][5] >= 2
    hops = f.clearance(cr.BLOCKED | cr.OPEN, 32)["hops"]
    rh = rr.Route(f, cells, [goal, mid], hops=hops, min_hops=1, soft_hops=4, soft_weight=0.25, max_cost=30.0)
    both_paths(m, rh, [goal, mid], hops=hops, min_hops=1, soft_hops=4, soft_weight=0.25, max_cost=30.0, what=(rows, "hops"))
    assert hops[mid] >= 1 and 0 < int(rh.counts[2]) < int(r.counts[2])


def test_the_second_trip_of_the_grid_stride_loops_inside_the_default_sweeps():
    """k_route_steps and k_route_sweep with 2048 workgroups of 256 threads (four lanes a row), k_route_enter with 2048 and
    k_route_finish with 512 (one lane a row): on 131 769 rows all go into their second trip.  The goal in the middle: the field is
    hundreds of steps deep, inside the 1024 sweeps of a call that names none."""
    m, f, cells = lattice(131769)
    n = int(cells["num_nodes"])
    assert 4 * n > 2048 * 256 and n > 512 * 256 and n > rr.LDS_ROWS
    goal = row_at(cells, 182, 182)
    r = rr.Route(f, cells, [goal])
    got = check(m, r, [goal], what="second trip")
    tail = r.cost[512 * 256:]
    assert (tail != rr.FLT_MAX).any() and got["counts"][4] == 1 and 100 < got["counts"][5] < 1024 and r.depth() > 300
    check(m, r, [goal], host=True, what="second trip, host")


# ---- the descent -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [1, 63, 64, 65, 4097])
def test_descend_at_the_wavefront_and_grid_edges_of_K(K):
    m, f, cells = lattice("41x25")
    n = int(cells["num_nodes"])
    r = rr.Route(f, cells, [n - 1])
    starts = (np.arange(K) * 37) % (n + 3) - 3                   # every seventh pass or so a point off the map
    starts = np.where(starts < 0, -1, starts)
    for host, stride in ((False, 12), (True, 16)):
        rows, info = check_descend(m, cells, r, starts, 48, host=host, stride=stride, what=(K, host))
    assert K < 63 or {int(s) for s in info[:, 0]} >= {rr.FOUND, rr.NO_START}


def test_descend_a_short_cap_the_step_guard_to_the_step_and_a_corrupted_next():
    m, f, cells = lattice("41x25")
    n = int(cells["num_nodes"])
    r = rr.Route(f, cells, [n - 1])
    L = r.depth()
    far = int(np.argmax(r.steps))
    assert L >= 40
    for host in (False, True):
        rows, info = check_descend(m, cells, r, [far, far, n - 1], 7, host=host, what="short cap")
        assert info[0][1] == L + 1 > 7 and info[2][1] == 1
        rows, info = check_descend(m, cells, r, [far], L + 1, max_steps=L, host=host, what="exactly")
        assert info[0][0] == rr.FOUND and info[0][3] == L
        rows, info = check_descend(m, cells, r, [far], L + 1, max_steps=L - 1, host=host, what="one fewer")
        assert info[0][0] == rr.LIMIT and info[0][1] == 0 and (rows == rr.NO_ROW).all()
        check_descend(m, cells, r, [far, 5], 0, host=host, what="no rows")
        # a circle and an entry out of range: LIMIT, and nothing outside the arrays is touched
        a, b = far, int(r.next[far])
        bad = r.next.copy()
        bad[b] = a
        rows, info = check_descend(m, cells, r, [a, n - 1], 16, max_steps=1000, nxt=bad, host=host, what="circle")
        assert info[0][0] == rr.LIMIT and info[0][3] == 1000 and info[1][0] == rr.FOUND
        for wrong in (n, n + 1, 0xFFFFFFFE, 0x80000000):
            bad[b] = wrong
            rows, info = check_descend(m, cells, r, [a], 16, nxt=bad, host=host, what=("out of range", wrong))
            assert info[0][0] == rr.LIMIT and info[0][3] == 1
    tree = rr.Route(f, cells, [n - 1], max_cost=5.0)             # rows without a route
    rows, info = check_descend(m, cells, tree, [far, n - 1], 8, start_mode=2, what="node mode")
    assert info[0][0] == rr.NO_ROUTE and info[1][0] == rr.FOUND


def test_routes_go_straight_into_shortcut_routes():
    import torch
    m, f, cells = corridor()
    goal = row_at(cells, 4, 1)
    hops = box_hops(m, f, cells, [1, 6, 6, 6, 1, 1])
    starts = np.array([row_at(cells, sx, sy) for sx in range(1, 8) for sy in (12, 9, 7)])
    for host in (False, True):
        fld = m.route_field(np.int32([goal]) if host else dev([goal], np.int32), hops=hops, min_hops=1, host=host)
        pts = cells["mean"][starts]
        rows, info = m.descend_routes(pts if host else dev(pts), fld, route_cap=40, host=host)
        got = m.shortcut_routes((rows, info), hops=hops, min_hops=1, host=host)
        torch.cuda.synchronize()
        assert (to_np(info["status"]) == rr.FOUND).all() and (to_np(got["status"]) == 0).all()         # SHORTCUT_STATUS ok: never bad_route
        way = to_np(got["waypoint_rows"])
        for k in range(len(starts)):
            w = way[k][:int(to_np(got["waypoints"])[k])]
            assert len(w) >= 2 and w[0] == starts[k] and w[-1] == goal and (hops[w] >= 1).all()
        xyz = m.route_waypoints(rows)
        assert tuple(xyz.shape) == (len(starts), 40, 3)


# ---- other conditions --------------------------------------------------------------------------------------------------------------

def test_repeat_calls_a_side_stream_and_a_larger_call_first():
    import torch
    big = lattice(rr.LDS_ROWS + 1)
    bn = int(big[2]["num_nodes"])
    m, f, cells = _tgc().site("bridge")
    before = m.export()
    goals = [int(np.flatnonzero(f.slope)[7])]
    r = rr.Route(f, cells, goals)
    first = check(m, r, goals, what="first")
    s = torch.cuda.Stream()
    for on in (True, False):
        with one_workgroup(on):
            for stream in (None, s, None, s):
                rc, got = raw(m, goals, stream=stream)
                assert rc == 0 and all(got[k].tobytes() == first[k].tobytes() for k in ("cost", "next")), (stream, on)
            # an answer of another shape in between (the scratch is reused), and a larger map's call on its own handle
            other = [int(np.flatnonzero(f.slope)[-3])]
            check(m, rr.Route(f, cells, other, max_cost=4.0), other, max_cost=4.0, max_rounds=4096, what="between")
            rc, got = raw(m, goals, host=True)
            assert rc == 0 and all(got[k].tobytes() == first[k].tobytes() for k in ("cost", "next"))
    # the same handle after a call on a larger map: a small lattice's handle is given the large lattice's rows, then its own again
    small = lattice(1025)
    rs = rr.Route(small[1], small[2], [3])
    a = check(small[0], rs, [3], what="small")
    check(big[0], rr.Route(big[1], big[2], [bn - 1]), [bn - 1], what="big")
    b = check(small[0], rs, [3], what="small again")
    assert a["cost"].tobytes() == b["cost"].tobytes()
    after = m.export()
    for k in ("sx", "sy", "sz", "mean", "normal", "flags"):
        assert np.asarray(after[k]).tobytes() == np.asarray(before[k]).tobytes(), k


def test_first_builder_of_the_index_after_a_crop_and_after_an_update():
    cloud = scenes.drivable_site(200_000)
    for on in (True, False):
        m = build(cloud, scenes.COST_PARAMS, 1)

        def fresh(what):
            cells = m.export()
            f = cr.Field(cells)
            assert f.angle_margin_deg > 1e-3, what
            goals = np.flatnonzero(f.slope)[[0, -1]]
            r = rr.Route(f, cells, goals)
            with one_workgroup(on):
                got = check(m, r, goals, what=(what, on))
            assert got["counts"][2] > 100
            return cells

        with one_workgroup(on):                                   # nothing has asked for the column index yet
            cells = fresh("first")
        x0, x1 = int(cells["sx"].min()), int(cells["sx"].max())
        m.crop_box((x0 + 5, x1 - 5, -1000, 1000), "keep_inside")
        assert fresh("crop")["num_nodes"] < cells["num_nodes"]
        m.change2DMap("slope", dev(cloud[1:1000, :3] + np.float32([0.0, 0.0, 0.02])))
        fresh("update")
        # everything cropped away: zero counts but "converged", nothing else written
        m.crop_box((x1 + 50, x1 + 60, 1, 2), "keep_inside")
        assert m.sync()[0] == 0
        for host in (False, True):
            rc, got = raw(m, [0, 1], host=host)
            assert rc == 0 and tuple(got["counts"]) == (0, 0, 0, 0, 1, 0, 0, 0) and untouched(got)
            fld = m.route_field(np.int32([0]) if host else dev([0], np.int32), host=host)
            assert len(fld["cost"]) == 0 and len(fld["next"]) == 0 and int(fld["converged"]) == 1
            rows, info = m.descend_routes(np.zeros((2, 3), np.float32) if host else dev(np.zeros((2, 3))), fld, route_cap=4, host=host)
            assert (to_np(info["status"]) == rr.NO_START).all() and (to_np(rows) == -1).all()


def test_outputs_are_optional_no_goals_and_out_of_sweeps():
    m, f, cells = lattice(1025)
    n = int(cells["num_nodes"])
    r = rr.Route(f, cells, [n - 1])
    L = r.depth()
    for on in (True, False):
        with one_workgroup(on):
            for host in (False, True):
                for outs in (("cost",), ("next",)):
                    got = check(m, r, [n - 1], outs=outs, host=host, what=(outs, host, on))
                    assert set(got) == set(outs) | {"counts", "tails"}
                rc, got = raw(m, [], host=host)
                assert rc == 0 and tuple(got["counts"]) == (0, 0, 0, 0, 1, 0, 0, 0) and untouched(got)
                assert (got["cost"] == rr.bits(rr.FLT_MAX)).all() and (got["next"] == rr.NO_ROW).all()
                check(m, r, [n - 1], max_rounds=L + 1, host=host, what=("L + 1", on))
                # out of sweeps: what is promised, and no more
                rc, got = raw(m, [n - 1], max_rounds=2, host=host)
                assert rc == 0 and got["counts"][4] == 0 and got["counts"][5] == 2 and untouched(got)
                cost, nxt = got["cost"].view(np.float32), got["next"]
                fin = cost != rr.FLT_MAX
                assert 0 < fin.sum() == got["counts"][2] and (cost[fin] >= r.cost[fin]).all() and r.finite[fin].all()
                for q in np.flatnonzero(fin)[::7].tolist():
                    chain, v = rr.chain_cost(r.mean, r.w, cost, nxt, q, n)
                    assert chain[-1] == n - 1 and v <= cost[q]


def test_refused_arguments():
    import torch
    m, f, cells = corridor()
    n = int(cells["num_nodes"])
    goal = [row_at(cells, 4, 1)]
    for host in (False, True):
        assert raw(m, goal, host=host)[0] == 0
        for bad in (dict(checks=2), dict(checks=0x80000001), dict(max_rounds=4097), dict(max_rounds=0xFFFFFFFF), dict(soft_weight=-1.0),
                    dict(soft_weight=float("inf")), dict(soft_weight=float("nan")), dict(max_cost=-1.0), dict(max_cost=float("nan")),
                    dict(max_cost=float("inf")), dict(reserved=(1, 0)), dict(reserved=(0, 1)), dict(outs=()), dict(counts=False),
                    dict(G=(1 << 20) + 1)):
            assert raw(m, goal, host=host, **bad)[0] == ERR_INVALID, bad
        assert raw(m, [], G=1, host=host)[0] == ERR_INVALID          # null goals with G > 0
        rc, got = raw(m, goal, max_rounds=4096, host=host)
        assert rc == 0 and got["counts"][4] == 1
        r = rr.Route(f, cells, goal)
        pts = cells["mean"][:3]
        assert raw_descend(m, pts, r.cost, r.next, 4, host=host)[0] == 0
        for bad in (dict(max_steps=(1 << 20) + 1), dict(start_mode=3), dict(start_mode=-1), dict(stride=8), dict(reserved=(0, 0, 0, 0, 0, 1)),
                    dict(reserved=(1, 0, 0, 0, 0, 0))):
            rc = raw_descend(m, pts, r.cost, r.next, 4, host=host, **bad)[0]
            assert rc == ERR_INVALID, bad
    # device pointers: alignment, NULL fields, rows without a cap
    from grid_ndt_amd._lib import DescendParams, RouteFieldParams
    prm, dp = RouteFieldParams(), DescendParams()
    g = dev(goal, np.int32)
    cost, nxt, cnt = (torch.zeros(n + 4, dtype=torch.int32, device="cuda") for _ in range(3))
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    L = m._L
    assert L.gndt_route_field_device(m._h, None, C.byref(prm), p(g), 1, None, None, p(cost), p(nxt), p(cnt), None) == 0
    for args in ((p(g, 2), 1, None, None, p(cost), p(nxt), p(cnt)), (p(g), 1, p(cost, 1), None, p(cost), p(nxt), p(cnt)),
                 (p(g), 1, None, p(nxt, 2), p(cost), p(nxt), p(cnt)), (p(g), 1, None, None, p(cost, 2), p(nxt), p(cnt)),
                 (p(g), 1, None, None, p(cost), p(nxt, 1), p(cnt)), (p(g), 1, None, None, p(cost), p(nxt), p(cnt, 2))):
        assert L.gndt_route_field_device(m._h, None, C.byref(prm), *args, None) == ERR_INVALID
    assert L.gndt_route_field_device(m._h, None, None, p(g), 1, None, None, p(cost), p(nxt), p(cnt), None) == ERR_INVALID
    assert L.gndt_route_field_device(None, None, C.byref(prm), p(g), 1, None, None, p(cost), p(nxt), p(cnt), None) == ERR_INVALID
    s = dev(cells["mean"][:2])
    rows, info = torch.zeros(16, dtype=torch.int32, device="cuda"), torch.zeros(32, dtype=torch.int32, device="cuda")
    ok = (p(s), 2, 12, C.byref(dp), p(cost), p(nxt), p(rows), 4, p(info))
    assert L.gndt_descend_routes_device(m._h, *ok, None) == 0
    for i, v in ((8, p(info, 8)), (8, None), (4, None), (5, None), (6, None), (7, 0), (0, p(s, 2)), (4, p(cost, 2)), (5, p(nxt, 1)), (6, p(rows, 2)),
                 (0, None), (3, None), (1, 1 << 31)):
        args = list(ok)
        args[i] = v
        assert L.gndt_descend_routes_device(m._h, *args, None) == ERR_INVALID, i
    assert L.gndt_descend_routes_device(m._h, p(s), 0, 12, C.byref(dp), p(cost), p(nxt), None, 0, p(info), None) == 0
    # a capturing stream: refused, and the capture goes on
    import grid_ndt_amd as g_
    cap = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    x = torch.zeros(16, device="cuda")
    with g_.graph_capture(graph, stream=cap):
        rc1 = L.gndt_route_field_device(m._h, None, C.byref(prm), p(g), 1, None, None, p(cost), p(nxt), p(cnt), C.c_void_p(cap.cuda_stream))
        rc2 = L.gndt_descend_routes_device(m._h, *ok, C.c_void_p(cap.cuda_stream))
        x.add_(1.0)
    assert rc1 == ERR_INVALID and rc2 == ERR_INVALID
    graph.replay()
    torch.cuda.synchronize()
    assert float(x[0]) == 1.0
    both_paths(m, rr.Route(f, cells, goal), goal, what="after the refused capture")


def test_python_interface_rows_points_numpy_torch_and_streams():
    import torch
    m, f, cells = corridor()
    goal = row_at(cells, 4, 1)
    hops = f.clearance(cr.BLOCKED, 32)["hops"]
    r = rr.Route(f, cells, [goal, 10], np.float32([0.0, 1.0]), hops=hops, min_hops=1, soft_hops=2, soft_weight=0.5, overhead=True, max_cost=20.0)
    s = torch.cuda.Stream()
    kw = dict(hops=dict(hops=hops), min_hops=1, soft_hops=2, soft_weight=0.5, overhead=True, max_cost=20.0)
    pts = cells["mean"][[goal, 10]]
    for goals, extra in ((np.int32([goal, 10]), dict(host=True)), (dev([goal, 10], np.int32), dict()), (pts, dict(host=True)),
                         (dev(pts), dict(stream=s)), (dev(pts), dict(max_rounds=4096))):
        gc = np.float32([0.0, 1.0]) if extra.get("host") else dev([0.0, 1.0])
        fld = m.route_field(goals, gc, **kw, **extra)
        if "stream" in extra:
            s.synchronize()
        torch.cuda.synchronize()
        assert set(fld) == {"cost", "next", "counts", "converged"} and isinstance(fld["cost"], np.ndarray) == bool(extra.get("host"))
        assert np.array_equal(rr.bits(to_np(fld["cost"])), rr.bits(r.cost)) and np.array_equal(to_np(fld["next"]).view(np.uint32), r.next)
        assert np.array_equal(to_np(fld["counts"]).view(np.uint32)[:5], r.counts) and int(fld["converged"]) == 1
        assert (to_np(fld["next"])[r.next == rr.NO_ROW] == m.NO_ROW).all()
    assert set(m.route_field(np.int32([goal]), next=False, host=True)) == {"cost", "counts", "converged"}
    starts = cells["mean"][[0, 40, 100, 155]]
    for host in (False, True):
        rows, info = m.descend_routes(starts if host else dev(starts), fld, host=host)
        torch.cuda.synchronize()
        assert tuple(rows.shape) == (4, 156) and isinstance(rows, np.ndarray) == host
        for k, q in enumerate((0, 40, 100, 155)):
            st, ln, wr, ex, c, hs = rr.descend(r.cost, r.next, q, 156)
            got = {key: to_np(v)[k] for key, v in info.items()}
            assert (got["status"], got["length"], got["start_row"], got["expansions"], got["queue_peak"]) == (st, ln, q, ex, 0)
            assert rr.bits(got["cost"]) == rr.bits(c) and np.array_equal(to_np(rows)[k].view(np.uint32), wr)
    with pytest.raises(ValueError):
        m.route_field(np.int32([goal]), hops=hops[:10], host=True)
    with pytest.raises(ValueError):
        m.descend_routes(starts, dict(cost=r.cost[:5], next=r.next[:5]), host=True)
