"""CPU tier: route shortcutting's per-route code (grid_ndt_amd/csrc/gndt_shortcut.hpp: the link, the group choice, the sums), compiled
with g++ into tests/_shortcut_shim.so and run one route after another with the wavefront's collectives lane after lane, against the
restatement (tests/shortcut_ref.py) on maps the oracle builds — the planner's own routes (tests/plan_ref.py) — and on 200 random cell
tables with random 4-neighbour staircases: every info field and every row of both outputs for equality.  The properties of every answer;
the waypoints driven again as a polyline by the walks' restatement; every status; and the product entry points refuse to run without a
GPU.  (The link finds its steps with the gates only: there is no steps-table variant to run a second way.)"""
import ctypes as C

import numpy as np
import pytest

from tests import clearance_ref as cr
from tests import plan_ref as pr
from tests import shortcut_ref as sr
from tests import walk_ref as wr
from tests.host_emulation import MAP, load_shim
from tests.test_clearance_host import FUZZ_ROBOT, MARGIN, random_table
from tests.test_raster_host import SCENES
from tests.test_walk_host import _map, plateau

_shim = None
SENTINEL = 0xDEADBEEF


def shim():
    global _shim
    if _shim is None:
        vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
        head = [vp, vp, MAP, vp]
        _shim = load_shim("shortcut_shim.cpp", "_shortcut_shim.so",
                          {"sshim_shortcut": (head + [vp, u64, u32, vp, u64, vp, u32, vp, u32, vp], C.c_int),
                           "sshim_link": (head + [u32, u32], C.c_int)})
    return _shim


def _head(t, origin, grid_len, z_len, robot, window, overhead, hops, min_hops, max_links):
    rb = dict(cr.ROBOT)
    rb.update(robot or {})
    r4 = np.array([rb["radius"], rb["reachable_height"], rb["max_rough"], rb["max_angle_deg"]], np.float32)
    rule = np.array([window or sr.DEFAULT_WINDOW, 1 if overhead else 0, min_hops, max_links or sr.DEFAULT_LINKS], np.uint32)
    hp = None if hops is None else np.ascontiguousarray(hops, np.uint32)
    p = lambda a: a.ctypes.data if a is not None and a.size else None
    keep = (r4, rule, hp)
    return keep, [p(r4), p(rule), t.shim_map(origin=origin, grid_len=grid_len, z_len=z_len), p(hp)]


def run(t, origin, grid_len, z_len, routes, lengths, robot=None, window=0, overhead=False, hops=None, min_hops=0, max_links=0, waypoint_cap=None,
        path_cap=0, stride=4):
    """the shim's routes on Table t -> (info, waypoint_rows, path_rows); lengths at `stride` bytes"""
    routes = np.ascontiguousarray(routes, np.uint32)
    K, route_cap = routes.shape
    wcap = route_cap if waypoint_cap is None else waypoint_cap
    ln = np.zeros((max(K, 1), stride // 4), np.uint32)
    ln[:K, 0] = lengths
    info = np.zeros(max(K, 1), sr.INFO_DTYPE)
    info.view(np.uint32)[:] = SENTINEL
    wp = np.full((K, wcap), SENTINEL, np.uint32)
    path = np.full((K, path_cap), SENTINEL, np.uint32)
    keep, head = _head(t, origin, grid_len, z_len, robot, window, overhead, hops, min_hops, max_links)
    p = lambda a: a.ctypes.data if a is not None and a.size else None
    rc = shim().sshim_shortcut(*head, p(routes), K, route_cap, ln.ctypes.data, stride, wp.ctypes.data, wcap, p(path), path_cap, info.ctypes.data)
    assert rc == 0
    return info[:K], wp, path


def pack(routes, cap=None, fill=sr.NO_ROW):
    """lists of rows -> (rows [K, cap] uint32, lengths)"""
    cap = max([len(r) for r in routes] + [1]) if cap is None else cap
    rows = np.full((len(routes), cap), fill, np.uint32)
    for k, r in enumerate(routes):
        rows[k, :min(len(r), cap)] = r[:cap]
    return rows, np.array([len(r) for r in routes], np.uint32)


def staircase(rng, w, steps):
    """a random 4-neighbour walk along the steps the walks would take (Walker.pick) from a slope that has one, straight back only out
    of a dead end"""
    if not hasattr(w, "_with_steps"):
        w._with_steps = sorted({q for q, _ in w.steps})
    q = int(w._with_steps[rng.integers(0, len(w._with_steps))])
    route, back = [q], None
    heading = int(rng.integers(0, 4))
    for _ in range(steps):
        sides = [heading] * 3 + list(range(4))
        rng.shuffle(sides)
        for k in sides:
            t, _ = w.pick(q, k)
            if t is not None and k != back:
                break
        else:
            k = back
            t, _ = w.pick(q, k) if k is not None else (None, None)
            if t is None:
                break
        heading = k if rng.random() < 0.7 else int(rng.integers(0, 4))
        back = k ^ 1
        q = t
        route.append(q)
    return route


def properties(s, routes, lengths, info, full, window, what):
    """what holds for every answer: no more waypoints than rows; the ends are the route's; an accepted link's slopes are 4-neighbour
    steps of the clearance graph and lie within the window; window 1 tests each of the route's own steps"""
    w = s.w
    edges = set(zip(w.f.edge_from.tolist(), w.f.edge_to.tolist()))
    for k, (wp, path, fb) in enumerate(full):
        n = int(lengths[k])
        if info["status"][k] in (sr.EMPTY, sr.BAD_ROUTE):
            assert not wp and not path and info["waypoints"][k] == 0, (what, k)
            continue
        assert len(wp) <= n and wp[0] == routes[k][0] and wp[-1] == routes[k][n - 1] and path[0] == wp[0] and path[-1] == wp[-1], (what, k)
        assert info["fallback_links"][k] == len(fb) and info["path_slopes"][k] == len(path), (what, k)
        it = iter(routes[k][:n])
        assert all(any(r == v for v in it) for r in wp), (what, k, "the waypoints are a subsequence of the route")
        for i in range(1, len(path)):
            if i in fb:
                continue
            a, b = path[i - 1], path[i]
            assert (a, b) in edges and (w.sx[b], w.sy[b]) in cr.sides_of(w.sx[a], w.sy[a]), (what, k, i)
        if window == 1 and info["status"][k] == sr.OK:
            assert info["links_tested"][k] == n - 1 and wp == list(routes[k][:n]), (what, k)


def both(t, s, routes, lengths, what, **kw):
    """the shim against the restatement, with all rows kept and with the caps cut -> (info, full)"""
    want = s.shortcut(routes, lengths, path_cap=routes.shape[1] * 2, **kw)
    got = run(t, s.origin, s.grid_len, s.z_len, routes, lengths, robot=s.w.robot, path_cap=routes.shape[1] * 2, **kw)
    sr.same(*got, *want[:3], what)
    cut = s.shortcut(routes, lengths, waypoint_cap=2, path_cap=3, **kw)
    got = run(t, s.origin, s.grid_len, s.z_len, routes, lengths, robot=s.w.robot, waypoint_cap=2, path_cap=3, stride=32, **kw)
    sr.same(*got, *cut[:3], (what, "cut"))
    cw, cp = want[1][:, :2], want[2][:, :3]                 # (a route_cap of 1 leaves less than the cut caps)
    assert np.array_equal(cut[1][:, :cw.shape[1]], cw) and np.array_equal(cut[2][:, :cp.shape[1]], cp), what
    got = run(t, s.origin, s.grid_len, s.z_len, routes, lengths, robot=s.w.robot, **kw)
    sr.same(*got, want[0], want[1], None, (what, "no path"))
    properties(s, [list(r) for r in routes], lengths, want[0], want[3], kw.get("window", 0) or sr.DEFAULT_WINDOW, what)
    return want[0], want[3]


_goals = {"bridge_ground": pr.BRIDGE_GOALS["under"]}


def _planned(name):
    """the planner's routes (tests/plan_shim.cpp on the oracle's flood) from starts spread over the scene's traversable slopes"""
    m, t, w = _map(name)
    goal = _goals.get(name)
    if goal is None:                                        # the centroid of a slope with steps around it: the end of a staircase
        goal = tuple(float(v) for v in m.mean[staircase(np.random.default_rng(1), w, 60)[-1]])
    pm = pr.PlanMap(m.cells, m.origin, m.P, goal)
    if pm.rc != 0:
        return m, t, w, []
    trav = np.flatnonzero(((pm.flags & 2) != 0) & (pm.state == 1))
    starts = trav[np.linspace(0, len(trav) - 1, min(10, len(trav))).astype(np.int64)]
    rows, info, _ = pm.shim_routes(pm.start_points(starts))
    return m, t, w, [r for r in (pr.route_of(rows, info, k) for k in range(len(starts))) if r]


@pytest.mark.parametrize("name", sorted(SCENES))
def test_oracle_scenes_planned_routes_and_staircases_are_the_restatement(name):
    m, t, w, planned = _planned(name)
    assert w.f.angle_margin_deg > MARGIN, w.f.angle_margin_deg
    s = sr.Shortcutter(m.cells, m.origin, m.P["grid_len"], m.P["z_len"], walker=w)
    rng = np.random.default_rng(31)
    routes = planned + [staircase(rng, w, int(rng.integers(2, 150))) for _ in range(8)]
    rows, lengths = pack(routes)
    hops = rng.integers(0, 6, t.n).astype(np.uint32)
    shorter = 0
    for kw in (dict(), dict(window=7), dict(window=130), dict(window=1), dict(overhead=True, hops=hops, min_hops=1), dict(window=70, max_links=200)):
        info, _ = both(t, s, rows, lengths, (name, kw), **kw)
        shorter += int((info["waypoints"] < info["length_in"]).sum())
    print(name, dict(planned=len(planned), longest=int(lengths.max()), routes_made_shorter=shorter))
    assert shorter > 0


def test_fuzz_200_random_cell_tables():
    rng = np.random.default_rng(20251020)
    skipped, tables = 0, 200
    seen, cut, fallbacks, long_links = {}, 0, 0, 0
    for k in range(tables):
        t = random_table(rng)
        w = wr.Walker(t.cells, (0.0, 0.0, 0.0), 0.5, 0.25, FUZZ_ROBOT)
        if w.f.angle_margin_deg <= MARGIN:
            skipped += 1
            continue
        s = sr.Shortcutter(t.cells, (0.0, 0.0, 0.0), 0.5, 0.25, walker=w)
        routes = [staircase(rng, w, int(rng.integers(0, 90))) for _ in range(5)]
        routes.append([])                                                      # EMPTY
        bad = list(routes[0]) + [int(rng.choice([sr.NO_ROW, t.n, t.n + 7] + np.flatnonzero(~w.slope)[:1].tolist()))] + list(routes[1])
        routes.append(bad)                                                     # BAD_ROUTE: a row out of range or without a slope
        jump = [int(r) for r in rng.choice(np.flatnonzero(w.slope), 6)]        # any sequence of slope rows is a route
        routes.append(jump)
        rows, lengths = pack(routes)
        if k % 7 == 0:
            lengths[2] = rows.shape[1] + 1                                     # BAD_ROUTE: longer than route_cap
        hops = rng.integers(0, 5, t.n).astype(np.uint32)
        kw = [dict(), dict(window=int(rng.integers(1, 12))), dict(hops=hops, min_hops=int(rng.integers(0, 3)), window=66),
              dict(overhead=True, window=20, max_links=int(rng.integers(1, 60)))][k % 4]
        info, full = both(t, s, rows, lengths, (k, kw), **kw)
        for st in info["status"].tolist():
            seen[st] = seen.get(st, 0) + 1
        cut += int((info["waypoints"] < info["length_in"]).sum())
        fallbacks += int(info["fallback_links"].sum())
        long_links += int((info["path_slopes"] > info["length_in"]).sum())
    print("fuzz:", dict(skipped=skipped, statuses=seen, routes_made_shorter=cut, fallback_links=fallbacks, paths_longer_than_routes=long_links))
    assert skipped <= tables * 5 // 100, skipped
    assert all(seen.get(st, 0) > 0 for st in range(4)), seen
    assert cut > tables and fallbacks > tables, (cut, fallbacks)


def _plateau():
    t = plateau(np.random.default_rng(5), side=16)
    w = wr.Walker(t.cells, (0.0, 0.0, 0.0), 0.5, 0.25)
    return t, w, sr.Shortcutter(t.cells, (0.0, 0.0, 0.0), 0.5, 0.25, walker=w)


def test_the_waypoints_drive_as_a_polyline_on_a_single_storey():
    """route_waypoints' points (the columns' centres, the rows' mean z; NaN behind the end) through the walks' restatement: on one
    storey the start lookup finds the route's first row, every segment is the link again (the walk holds waypoint 0's z where the link
    held the anchor's: z only picks levels, which the walks ignore) — DONE on the goal over the same slopes as path_rows"""
    t, w, s = _plateau()
    rng = np.random.default_rng(8)
    routes = [staircase(rng, w, int(rng.integers(3, 60))) for _ in range(24)]
    rows, lengths = pack(routes)
    info, wp, path, full = s.shortcut(rows, lengths, path_cap=128)
    got = run(t, s.origin, 0.5, 0.25, rows, lengths, path_cap=128)
    sr.same(*got, info, wp, path, "plateau")
    assert (info["status"] == sr.OK).all() and (info["fallback_links"] == 0).all() and (info["waypoints"] < info["length_in"]).any()
    K, cap = wp.shape
    poly = np.full((K, cap, 3), np.nan, np.float32)
    for k in range(K):
        for i in range(int(info["waypoints"][k])):
            poly[k, i] = s.point(int(wp[k, i]), w.mean[int(wp[k, i]), 2])
    winfo, wrows, walked = w.walk(poly, row_cap=128)
    assert (winfo["status"] == wr.DONE).all()
    for k in range(K):
        assert winfo["start_row"][k] == routes[k][0] and winfo["end_row"][k] == routes[k][-1], k
        assert walked[k] == full[k][1] and winfo["steps"][k] + 1 == info["path_slopes"][k], k
        assert winfo["length"][k].view(np.uint32) == info["cost_out"][k].view(np.uint32), k


def test_window_one_returns_the_route_and_a_single_link_agrees():
    t, w, s = _plateau()
    rng = np.random.default_rng(9)
    routes = [staircase(rng, w, 30) for _ in range(6)]
    rows, lengths = pack(routes)
    info, full = both(t, s, rows, lengths, "window 1", window=1)
    assert (info["fallback_links"] == 0).all() and np.array_equal(info["waypoints"], lengths) and np.array_equal(info["links_tested"], lengths - 1)
    assert np.array_equal(info["cost_in"].view(np.uint32), info["cost_out"].view(np.uint32))
    # Link(a, b) on its own, either side of the window
    keep, head = _head(t, s.origin, 0.5, 0.25, None, 5, False, None, 0, 0)
    slopes = np.flatnonzero(w.slope)
    held = 0
    for a, b in rng.choice(slopes, (200, 2)):
        want = s.links(int(a), [int(b)], 5)[0][0]
        assert shim().sshim_link(*head, int(a), int(b)) == int(want), (a, b)
        held += int(want)
    assert 0 < held < 200
    assert shim().sshim_link(*head, t.n, int(slopes[0])) == 0 and shim().sshim_link(*head, int(slopes[0]), sr.NO_ROW) == 0


def test_every_status_and_the_limit_to_the_link():
    t, w, s = _plateau()
    rng = np.random.default_rng(10)
    route = staircase(rng, w, 40)
    assert len(route) == 41
    rows, lengths = pack([route, [], route[:1], route + [t.n], route[:20] + [sr.NO_ROW] + route[20:], route])
    assert rows.shape[1] == 42
    lengths[5] = 43                                                            # one more than route_cap
    info, full = both(t, s, rows, lengths, "statuses")
    assert info["status"].tolist() == [sr.OK, sr.EMPTY, sr.OK, sr.BAD_ROUTE, sr.BAD_ROUTE, sr.BAD_ROUTE]
    assert info["length_in"].tolist() == [41, 0, 1, 42, 42, 43]
    assert info["waypoints"].tolist()[1:] == [0, 1, 0, 0, 0] and info["path_slopes"][2] == 1 and info["links_tested"][2] == 0
    tested = int(info["links_tested"][0])
    rows, lengths = pack([route])
    exact, _ = both(t, s, rows, lengths, "max_links exact", max_links=tested)
    assert exact["status"][0] == sr.OK and exact["links_tested"][0] == tested
    short, full = both(t, s, rows, lengths, "max_links one short", max_links=tested - 1)
    assert short["status"][0] == sr.LIMIT and short["links_tested"][0] < tested and short["fallback_links"][0] > 0
    wp, path, fb = full[0]
    tail = int(short["fallback_links"][0])
    assert wp[-tail:] == route[-tail:] and path[-tail:] == route[-tail:]


def test_no_cpu_fallback_for_shortcuts(native_lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import grid_ndt_amd as g
    m = g.TwoDmap(0.5, 0.5)
    m.setCloudFirst((0, 0, 0))
    with pytest.raises(g.GndtError) as e:
        m.shortcut_routes(np.zeros((2, 3), np.int32), np.array([3, 3], np.int32), host=True)
    assert e.value.code == 2   # GNDT_ERR_NO_DEVICE
