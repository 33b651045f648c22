"""GPU tier: route shortcutting (gndt_shortcut_routes_device / gndt_shortcut_routes, TwoDmap.shortcut_routes / route_waypoints).  Every
map is hand-drawn and built on the device; every info field and every row of both outputs is compared for equality with the
restatement (tests/shortcut_ref.py) on the handle's own export, through both entry points, with the rows kept and with both caps cut,
into outputs over-allocated with a sentinel tail that must stay untouched.  Maps whose answer is known beforehand — an open floor, an
L-corridor, a wall with a gap, two storeys, a pillar with its clearance field, a low ceiling — then the group and window edges on a
corridor of 300 cells, the wavefront, workgroup and grid-stride edges of K, mixed statuses in one call, lengths out of a device-side
plan_routes info, the handle's lifetime, every refused argument, and a poisoned tier of this file's own.  No tolerance anywhere: the
one step that is not IEEE arithmetic is the gates' acosf, and every map keeps its angle decisions more than 1e-3 degrees from the
threshold.  (The link finds its steps with the gates only: there is no steps-table variant to run a second way.)"""
import ctypes as C
import numpy as np
import pytest

from tests import clearance_ref as cr
from tests import frontier_ref as fr
from tests import poison_tier
from tests import shortcut_ref as sr
from tests import walk_ref as wr
from tests.gpu_kit import Padded, PaddedCall, build, dev, robot_arg, to_np

pytestmark = pytest.mark.gpu

ERR_INVALID = 1
ATOMIC = 1
SENTINEL = 0x5A5A5A5A
PAD = 3                      # sentinel entries behind the outputs
MARGIN = 1e-3
WAVES = 4                    # kShortcutWaves: wavefronts (routes) a workgroup
MAX_BLOCKS = 1024            # kShortcutMaxBlocks: one trip of the grid-stride loop holds WAVES * MAX_BLOCKS routes
_scenes = {}


def raw(m, routes, lengths, robot=None, window=0, overhead=False, hops=None, min_hops=0, max_links=0, waypoint_cap=None, path_cap=0, stride=4,
        stream=None, host=False, reserved=(0,) * 4, checks=None):
    """The C entry points; info K + PAD entries, both row outputs K * cap + PAD words of sentinel -> (rc, info [K], waypoint_rows,
    path_rows, untouched: the tails still hold the sentinel).  lengths lie `stride` bytes apart, sentinel between them."""
    from grid_ndt_amd._lib import ShortcutParams
    routes = np.ascontiguousarray(routes, np.uint32)
    K, route_cap = routes.shape
    wcap = route_cap if waypoint_cap is None else waypoint_cap
    prm = ShortcutParams(window, (1 if overhead else 0) if checks is None else checks, min_hops, max_links, (C.c_uint32 * 4)(*reserved))
    ln = np.full((max(K, 1), stride // 4), SENTINEL, np.uint32)
    ln[:K, 0] = lengths
    info, wp, path = (Padded(n, words=w, back=PAD, fill=SENTINEL) for n, w in ((K, 12), (K * wcap, 1), (K * path_cap, 1)))
    hp = None if hops is None else np.ascontiguousarray(hops).view(np.uint32)
    rc = PaddedCall(host, stream, wait_for_current=True)(m._L.gndt_shortcut_routes, m._L.gndt_shortcut_routes_device, m._h, routes, K, route_cap, ln,
                                                         stride, robot_arg(robot, cr.ROBOT), C.byref(prm), hp, wp, wcap,
                                                         path if path_cap else None, path_cap, info)
    untouched = info.untouched() and wp.untouched() and path.untouched()
    return rc, info.body.view(sr.INFO_DTYPE), wp.body.reshape(K, wcap), path.body.reshape(K, path_cap), untouched


def check(m, s, routes, lengths, what="", entries=(False, True), stream=None, caps=True, **kw):
    """both entry points against the restatement: every row kept, then (caps) both outputs cut and the lengths 32 bytes apart
    -> (the restatement's info, waypoints, path rows, the full lists)"""
    ref_kw = {k: v for k, v in kw.items() if k != "robot"}
    routes = np.ascontiguousarray(routes, np.uint32)
    pcap = 2 * routes.shape[1] + 2
    want = s.shortcut(routes, lengths, path_cap=pcap, **ref_kw)
    cut = s.shortcut(routes, lengths, waypoint_cap=2, path_cap=3, **ref_kw) if caps else None
    for host in entries:
        tag = (what, "host" if host else "device")
        rc, info, wp, path, untouched = raw(m, routes, lengths, path_cap=pcap, host=host, stream=None if host else stream, **kw)
        assert rc == 0, (tag, m._L.gndt_last_error(m._h))
        sr.same(info, wp, path, *want[:3], tag)
        assert untouched, tag
        if caps:
            rc, info, wp, path, untouched = raw(m, routes, lengths, waypoint_cap=2, path_cap=3, stride=32, host=host, **kw)
            assert rc == 0 and untouched, tag
            sr.same(info, wp, path, *cut[:3], (tag, "cut"))
            rc, info, wp, path, untouched = raw(m, routes, lengths, host=host, **kw)
            assert rc == 0 and untouched and path.size == 0, tag
            sr.same(info, wp, path, want[0], want[1], None, (tag, "no path"))
    return want


def drawn(name, make, P=fr.P, robot=None):
    """a map drawn from a cloud -> (m, restatement, export)"""
    key = (name, tuple(sorted((robot or {}).items())))
    if key not in _scenes:
        base = [v for k, v in _scenes.items() if k[0] == name]
        if base:
            m, _, cells, cloud = base[0]
        else:
            cloud = make()
            m = build(cloud, P)
            cells = m.export()
        s = sr.Shortcutter(cells, cloud[0, :3], P["grid_len"], P["z_len"], robot)
        assert s.w.f.angle_margin_deg > MARGIN, (name, s.w.f.angle_margin_deg)
        _scenes[key] = (m, s, cells, cloud)
    return _scenes[key][:3]


def row_of(cells, ix, iy, nth=0):
    """the nth row of the column of cell (ix, iy) (tests/frontier_ref.cells_cloud: signed index ix + 1 for ix >= 0, else ix)"""
    sx, sy = (ix + 1 if ix >= 0 else ix), (iy + 1 if iy >= 0 else iy)
    return int(np.flatnonzero((cells["sx"] == sx) & (cells["sy"] == sy))[nth])


def floor_row(cells, ix, iy):
    """the lowest slope of the column of cell (ix, iy)"""
    sx, sy = (ix + 1 if ix >= 0 else ix), (iy + 1 if iy >= 0 else iy)
    rows = np.flatnonzero((cells["sx"] == sx) & (cells["sy"] == sy) & ((cells["flags"] & 2) != 0))
    return int(rows[np.argmin(cells["mean"][rows][:, 2])])


def route(cells, *xy):
    return [row_of(cells, ix, iy) for ix, iy in xy]


def pack(routes, cap=None):
    cap = max([len(r) for r in routes] + [1]) if cap is None else cap
    rows = np.full((len(routes), cap), sr.NO_ROW, np.uint32)
    for k, r in enumerate(routes):
        rows[k, :min(len(r), cap)] = r[:cap]
    return rows, np.array([len(r) for r in routes], np.uint32)


def line(a, b):
    """the cells of a straight run, both ends included"""
    (ax, ay), (bx, by) = a, b
    n = max(abs(bx - ax), abs(by - ay))
    return [(ax + (bx - ax) * i // n, ay + (by - ay) * i // n) for i in range(n + 1)] if n else [a]


def legs(*corners):
    out = [corners[0]]
    for a, b in zip(corners[:-1], corners[1:]):
        out += line(a, b)[1:]
    return out


# ---- maps whose answer is known beforehand -------------------------------------------------------------------------------------------

def _floor():
    return fr.cells_cloud([(ix, iy) for ix in range(10) for iy in range(10)])


def test_open_floor_a_staircase_and_a_straight_run():
    m, s, cells = drawn("floor", _floor)
    stairs = [(0, 0)]
    while stairs[-1] != (9, 9):
        x, y = stairs[-1]
        stairs.append((x + 1, y) if x == y else (x, y + 1))
    rows, lengths = pack([route(cells, *stairs), route(cells, *line((0, 4), (9, 4)))])
    assert lengths.tolist() == [19, 10]
    info, wp, path, full = check(m, s, rows, lengths, "floor")
    assert info["status"].tolist() == [sr.OK, sr.OK] and info["waypoints"].tolist() == [2, 2] and info["fallback_links"].tolist() == [0, 0]
    assert info["path_slopes"].tolist() == [19, 10] and info["links_tested"].tolist() == [18, 9]
    assert wp[0, :3].tolist() == [rows[0, 0], rows[0, 18], sr.NO_ROW] and wp[1, :3].tolist() == [rows[1, 0], rows[1, 9], sr.NO_ROW]
    assert full[1][1] == rows[1, :10].tolist()
    assert info["cost_out"][1] == info["cost_in"][1] and (info["hops_min"] == sr.BEYOND).all()


def _ell():
    return fr.cells_cloud(legs((0, 0), (5, 0), (5, 5)))


def test_l_corridor_one_cell_wide_keeps_its_corner():
    m, s, cells = drawn("ell", _ell)
    r = route(cells, *legs((0, 0), (5, 0), (5, 5)))
    rows, lengths = pack([r, r[::-1]])
    info, wp, path, full = check(m, s, rows, lengths, "ell")
    corner = row_of(cells, 5, 0)
    assert info["waypoints"].tolist() == [3, 3] and wp[0, :3].tolist() == [r[0], corner, r[-1]] and wp[1, :3].tolist() == [r[-1], corner, r[0]]
    assert info["fallback_links"].tolist() == [0, 0] and full[0][1] == r and info["links_tested"].tolist() == [15, 15]
    # a link past the corner leaves the map: the same two points as a path walk
    pts = m.route_waypoints(np.int32([[r[0], r[6]], [r[0], r[5]]]))
    got = m.walk_paths(pts, host=True)
    assert got["status"].tolist() == [wr.LEFT_MAP, wr.DONE] and got["end_row"][1] == corner


def _gap():
    return fr.cells_cloud([(ix, iy, fr.Z_FLOOR + (1.0 if iy == 3 and ix != 3 else 0.0)) for ix in range(7) for iy in range(7)])


GAP_ROUTE = legs((1, 0), (3, 0), (3, 6), (1, 6))             # 11 rows


def test_a_wall_with_a_gap_puts_the_waypoint_into_the_gap():
    """the wall's columns are in the map, a metre up: they offer no step.  From (1, 0) the line to the gap (3, 3) enters it from below
    (it meets y = 3 at x = 3.17); every row behind the gap is seen through the wall ((3, 4): the line meets y = 3 at x = 2.75); from
    the gap the line to (1, 6) leaves it upwards at x = 3.17 and is free.  The way back is the mirror image."""
    m, s, cells = drawn("gap", _gap)
    r = route(cells, *GAP_ROUTE)
    rows, lengths = pack([r, r[::-1]])
    info, wp, path, full = check(m, s, rows, lengths, "gap")
    gap = row_of(cells, 3, 3)
    assert info["waypoints"].tolist() == [3, 3] and wp[0, :3].tolist() == [r[0], gap, r[-1]] and wp[1, :3].tolist() == [r[-1], gap, r[0]]
    assert info["path_slopes"].tolist() == [11, 11] and info["fallback_links"].tolist() == [0, 0] and info["links_tested"].tolist() == [15, 15]
    assert len(set(full[0][1])) == 11 and full[0][1][5] == gap


def _storeys():
    return fr.cells_cloud([(ix, 0) for ix in range(5)] + [(ix, 0, fr.Z_FLOOR + 1.0) for ix in range(2, 5)])


def test_two_storeys_a_link_that_ends_on_the_other_storey_is_refused():
    m, s, cells = drawn("storeys", _storeys)
    ground = [row_of(cells, ix, 0, 0) for ix in range(5)]
    upper = [row_of(cells, ix, 0, 1) for ix in range(2, 5)]
    assert cells["mean"][upper[0]][2] > cells["mean"][ground[2]][2] + 0.9
    r = ground[:2] + upper                                   # no drive leads up: the walk from ground[1] enters column 3 on the ground
    rows, lengths = pack([r, ground, upper])
    info, wp, path, full = check(m, s, rows, lengths, "storeys")
    assert info["waypoints"].tolist() == [4, 2, 2] and info["fallback_links"].tolist() == [1, 0, 0] and info["status"].tolist() == [sr.OK] * 3
    assert wp[0, :4].tolist() == [ground[0], ground[1], upper[0], upper[2]] and full[0][2] == [2]
    assert info["links_tested"].tolist() == [4 + 3 + 2, 4, 2]


def _pillar():
    return fr.cells_cloud([(ix, iy, fr.Z_FLOOR + (1.0 if (ix, iy) == (4, 4) else 0.0)) for ix in range(9) for iy in range(9)])


def test_a_pillar_with_a_real_clearance_field():
    m, s, cells = drawn("pillar", _pillar)
    cl = m.clearance(host=True)
    hops = cl["hops"].view(np.uint32)
    assert np.array_equal(hops, s.w.f.clearance(cr.BLOCKED, 32)["hops"])
    # the line from (2, 2) to (6, 4) passes under the pillar (4, 4) and to the right of it: it meets y = 3 at x = 3.5, x = 4 at y =
    # 3.25, x = 5 at y = 3.75, y = 4 at x = 5.5 — no lattice corner, and the cells it crosses are the route
    diag = [(2, 2), (3, 2), (3, 3), (4, 3), (5, 3), (5, 4), (6, 4)]
    r = route(cells, *diag)
    assert [int(hops[t]) for t in r] == [3, 2, 1, 0, 1, 0, 1]
    rows, lengths = pack([r])
    info, wp, _, full = check(m, s, rows, lengths, "pillar, min_hops 0", hops=hops)
    assert info["waypoints"][0] == 2 and info["hops_min"][0] == 0 and info["fallback_links"][0] == 0 and full[0][1] == r
    info, wp, _, full = check(m, s, rows, lengths, "pillar, min_hops 2", hops=hops, min_hops=2)
    # (2, 2) -> (3, 2) holds (3 and 2 hops); every other link stands on a slope with fewer than 2
    assert info["waypoints"][0] == 7 and info["fallback_links"][0] == 5 and info["hops_min"][0] == 0 and wp[0].tolist() == r
    info, _, _, _ = check(m, s, rows, lengths, "pillar, min_hops 1", hops=hops, min_hops=1)
    assert info["hops_min"][0] == 0 and 2 < info["waypoints"][0] <= 7
    # the Python interface takes what clearance() returned, on the device and on the host
    for host in (False, True):
        field = m.clearance(host=host)
        got = m.shortcut_routes(rows.view(np.int32) if host else dev(rows.view(np.int32), np.int32), lengths.view(np.int32), hops=field, min_hops=2,
                                host=host)
        assert to_np(got["waypoints"]).tolist() == [7] and to_np(got["hops_min"]).tolist() == [0]
    with pytest.raises(ValueError):
        m.shortcut_routes(rows.view(np.int32), lengths.view(np.int32), hops=hops[:-1], host=True)


def _ceiling():
    floor = [(ix, iy, 0.26) for ix in range(-4, 4) for iy in range(-3, 3)]
    lid = [(ix, iy, 0.56) for ix in range(-4, -1) for iy in range(-3, 3)]           # 0.3 m above the floor's first three lines
    return fr.cells_cloud(floor + lid, 5)


def test_a_low_ceiling_with_and_without_the_overhead_check():
    m, s, cells = drawn("ceiling", _ceiling)
    r = [floor_row(cells, ix, iy) for ix, iy in line((3, 0), (-4, 0))]
    rows, lengths = pack([r])
    info, wp, _, _ = check(m, s, rows, lengths, "ceiling, check off")
    assert info["waypoints"][0] == 2 and info["fallback_links"][0] == 0
    info, wp, _, _ = check(m, s, rows, lengths, "ceiling, check on", overhead=True)
    assert info["waypoints"][0] == 5 and info["fallback_links"][0] == 3 and wp[0, :5].tolist() == [r[0]] + r[4:]
    slim = dict(radius=0.1)                                                           # 0.3 m is not within 0.2 m
    ms, ss, _ = drawn("ceiling", _ceiling, robot=slim)
    info, _, _, _ = check(ms, ss, rows, lengths, "ceiling, slim", overhead=True, robot=slim)
    assert info["waypoints"][0] == 2


# ---- group and window edges ------------------------------------------------------------------------------------------------------------

def _corridor():
    return fr.cells_cloud(line((0, 0), (299, 0)) + line((39, 1), (39, 90)) + line((69, 1), (69, 60)))


@pytest.mark.parametrize("window", [1, 2, 63, 64, 65, 128, 256])
def test_group_and_window_edges_on_a_corridor(window):
    m, s, cells = drawn("corridor", _corridor)
    along = route(cells, *line((100, 0), (299, 0)))
    ns = [1, 2, 3, 64, 65, 66, 129, 130]
    rows, lengths = pack([along[:n] for n in ns])
    info, wp, _, _ = check(m, s, rows, lengths, ("corridor", window), window=window, caps=window in (1, 65))
    for k, n in enumerate(ns):
        anchors = list(range(0, n - 1, window)) + [n - 1]
        assert info["waypoints"][k] == len(anchors) and wp[k, :len(anchors)].tolist() == [along[i] for i in anchors], (window, n)
        # every candidate of an anchor's window holds: only the farthest group is evaluated
        tested = sum((min(window, n - 1 - a) - 1) % 64 + 1 for a in anchors[:-1])
        assert info["links_tested"][k] == tested and info["fallback_links"][k] == 0 and info["path_slopes"][k] == n, (window, n)


def test_a_bend_leaves_the_far_group_empty_and_max_links_to_the_link():
    m, s, cells = drawn("corridor", _corridor)
    bend70 = route(cells, *legs((0, 0), (69, 0), (69, 60)))
    bend40 = route(cells, *legs((0, 0), (39, 0), (39, 90)))
    assert len(bend70) == len(bend40) == 130
    rows, lengths = pack([bend70, bend40])
    info, wp, _, full = check(m, s, rows, lengths, "bends", window=128)
    # bend after 70: candidates 65 .. 128 hold up to the corner (row 69), the near group is never looked at; then 60 up the branch
    # bend after 40: of 65 .. 128 none holds, of 1 .. 64 the rows up to the corner do; then 90 up the branch in two groups, 65 .. 90 first
    assert info["links_tested"].tolist() == [64 + 60, 64 + 64 + 26] and info["waypoints"].tolist() == [3, 3]
    assert wp[0, :3].tolist() == [bend70[0], bend70[69], bend70[129]] and wp[1, :3].tolist() == [bend40[0], bend40[39], bend40[129]]
    one = rows[1:], lengths[1:]
    exact, _, _, _ = check(m, s, *one, "max_links exact", window=128, max_links=154)
    assert exact["status"][0] == sr.OK and exact["links_tested"][0] == 154
    short, wp, path, full = check(m, s, *one, "max_links one short", window=128, max_links=153)
    assert short["status"][0] == sr.LIMIT and short["links_tested"][0] == 128 and short["fallback_links"][0] == 90 and short["waypoints"][0] == 92
    assert full[0][0][1:] == bend40[39:] and full[0][1] == bend40 and short["cost_out"][0] == short["cost_in"][0]
    first, _, _, full = check(m, s, *one, "max_links below the first group", window=128, max_links=63)
    assert first["status"][0] == sr.LIMIT and first["links_tested"][0] == 0 and full[0][0] == bend40 and first["fallback_links"][0] == 129


# ---- K ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [1, 2, WAVES - 1, WAVES, WAVES + 1])
def test_wavefront_and_workgroup_edges_of_K(K):
    m, s, cells = drawn("gap", _gap)
    r = route(cells, *GAP_ROUTE)
    routes = [r[k % 5:] if k % 2 == 0 else r[::-1][:len(r) - k] for k in range(K)]
    rows, lengths = pack(routes)
    info, _, _, _ = check(m, s, rows, lengths, ("K", K))
    assert (info["status"] == sr.OK).all() and (info["waypoints"] >= 2).all()


def test_more_routes_than_one_trip_of_the_grid_stride_loop():
    """k_shortcut_routes `for (k = blockIdx.x * kShortcutWaves + wave; k < K; k += waves)` with at most 1024 workgroups of 4 wavefronts:
    one route more than a trip holds, so the first wavefront comes round again.  The batch repeats 7 distinct short routes (a prime:
    no repeat shares its wavefront slot with its original), the restatement answers those once and is tiled the same way."""
    m, s, cells = drawn("gap", _gap)
    r = route(cells, *GAP_ROUTE)
    D, K = 7, WAVES * MAX_BLOCKS + 1
    base, base_len = pack([r[i:i + 2 + i % 4] for i in range(D)], cap=5)
    want = s.shortcut(base, base_len, path_cap=5)
    assert (want[0]["status"] == sr.OK).all() and len(set(want[0]["links_tested"].tolist())) > 1
    tile = np.arange(K) % D
    rc, info, wp, path, untouched = raw(m, base[tile], base_len[tile], path_cap=5)
    assert rc == 0 and untouched
    sr.same(info, wp, path, want[0][tile], want[1][tile], want[2][tile], "grid stride")


def test_one_call_mixes_every_status():
    """lengths 0 and 1, the three kinds of BAD_ROUTE, a LIMIT and good routes side by side; cr.pit_cloud's column under cell 3 holds 36
    rows without a slope"""
    m, s, cells = drawn("pit", cr.pit_cloud)
    r = [row_of(cells, ix, 0, 36 if ix == 3 else 0) for ix in range(7)]
    bare = row_of(cells, 3, 0, 0)
    assert (cells["flags"][r] & 2).all() and not cells["flags"][bare] & 2
    rows, lengths = pack([r, [], r[:1], r, r[:3] + [sr.NO_ROW] + r[3:], r[:2] + [bare] + r[2:], r[:3] + [int(cells["num_nodes"])], r[::-1], r], cap=8)
    lengths[3] = 9                                           # more rows than route_cap holds
    info, wp, path, full = check(m, s, rows[:8], lengths[:8], "mixed")
    assert info["status"].tolist() == [sr.OK, sr.EMPTY, sr.OK, sr.BAD_ROUTE, sr.BAD_ROUTE, sr.BAD_ROUTE, sr.BAD_ROUTE, sr.OK]
    assert info["waypoints"].tolist() == [2, 0, 1, 0, 0, 0, 0, 2] and info["length_in"].tolist() == [7, 0, 1, 9, 8, 8, 4, 7]
    assert (wp[[1, 3, 4, 5, 6]] == sr.NO_ROW).all() and (path[[1, 3, 4, 5, 6]] == sr.NO_ROW).all() and info["links_tested"][[1, 2, 3, 4, 5, 6]].sum() == 0
    info, _, _, _ = check(m, s, rows, lengths, "mixed, a limit", max_links=5)
    assert info["status"].tolist() == [sr.LIMIT, sr.EMPTY, sr.OK, sr.BAD_ROUTE, sr.BAD_ROUTE, sr.BAD_ROUTE, sr.BAD_ROUTE, sr.LIMIT, sr.LIMIT]


# ---- lengths, the planner, the walks ---------------------------------------------------------------------------------------------------

def test_routes_straight_out_of_a_device_side_plan_and_driven_by_the_walks():
    """flood -> plan_routes on the device -> shortcut_routes reads the lengths out of the plan's info records (stride 32, no copy) ->
    route_waypoints -> walk_paths drives every answer to the goal"""
    import torch
    m, s, cells = drawn("gap", _gap)
    goal = cells["mean"][row_of(cells, 6, 6)]
    assert m.computeCost(tuple(float(v) for v in goal))["rc"] == 0
    starts = cells["mean"][[row_of(cells, ix, iy) for ix, iy in ((0, 0), (1, 2), (6, 0), (3, 1), (0, 6), (6, 6), (2, 5))]]
    prow, pinfo = m.plan_routes(dev(starts), route_cap=24)
    assert pinfo["length"].stride(0) == 8 and (pinfo["status"] == 0).all()
    got = m.shortcut_routes((prow, pinfo), path_cap=32)
    torch.cuda.synchronize()
    lengths = to_np(pinfo["length"]).astype(np.uint32)
    want = s.shortcut(to_np(prow).view(np.uint32), lengths, path_cap=32)
    named = {k: to_np(got[k]).view(want[0][k].dtype) for k in sr.INFO_FIELDS}
    named["reserved"] = np.zeros(1, np.uint32)
    sr.same(named, to_np(got["waypoint_rows"]), to_np(got["path_rows"]), *want[:3], "planned")
    assert (want[0]["status"] == sr.OK).all() and want[0]["waypoints"][5] == 1 and (want[0]["waypoints"] < want[0]["length_in"]).sum() >= 5
    # the same through the host entry point, from numpy arrays and the host-side plan's info (uint32 fields 32 bytes apart)
    hrow, hinfo = m.plan_routes(starts, route_cap=24, host=True)
    assert hinfo["length"].strides == (32,) and np.array_equal(hrow, to_np(prow))
    hgot = m.shortcut_routes((hrow, hinfo), path_cap=32)
    assert isinstance(hgot["status"], np.ndarray)
    for k in sr.INFO_FIELDS + ("waypoint_rows", "path_rows"):
        assert np.array_equal(to_np(got[k]).view(np.uint32), hgot[k].view(np.uint32)), k
    # the waypoints as a polyline: NaN behind the end, driven by the walks to the goal over the same slopes
    pts = m.route_waypoints(got["waypoint_rows"])
    assert pts.shape == (7, 24, 3) and pts.is_cuda
    wrows = to_np(got["waypoint_rows"])
    ref = np.full((7, 24, 3), np.nan, np.float32)
    for k in range(7):
        for i in range(int(want[0]["waypoints"][k])):
            ref[k, i] = s.point(int(wrows[k, i]), cells["mean"][wrows[k, i]][2])
    assert np.array_equal(to_np(pts).view(np.uint32), ref.view(np.uint32)) and np.array_equal(m.route_waypoints(wrows).view(np.uint32), ref.view(np.uint32))
    walk = m.walk_paths(pts, rows=32)
    assert (to_np(walk["status"]) == wr.DONE).all() and (to_np(walk["end_row"]) == row_of(cells, 6, 6)).all()
    assert np.array_equal(to_np(walk["rows"]), to_np(got["path_rows"])) and np.array_equal(to_np(walk["waypoints"]), want[0]["waypoints"].astype(np.int32))
    assert np.array_equal(to_np(walk["length"]).view(np.uint32), want[0]["cost_out"].view(np.uint32))
    # nothing to do
    for host in (False, True):
        none = m.shortcut_routes(np.zeros((0, 4), np.int32) if host else dev(np.zeros((0, 4)), np.int32), np.zeros(0, np.int32), host=host)
        assert len(none["status"]) == 0 and tuple(none["waypoint_rows"].shape) == (0, 4)


# ---- the handle's lifetime -------------------------------------------------------------------------------------------------------------

def test_first_consumer_call_a_larger_call_before_and_a_second_stream():
    import torch
    cloud = _gap()
    m = build(cloud, fr.P)                                  # a handle no consumer has touched: this call makes the column index
    cells = m.export()
    s = sr.Shortcutter(cells, cloud[0, :3], fr.GL, fr.ZL)
    r = route(cells, *GAP_ROUTE)
    rows, lengths = pack([r])
    want = check(m, s, rows, lengths, "first call", entries=(False,))
    big, big_len = pack([r[i % 7:] for i in range(600)], cap=40)
    check(m, s, big, big_len, "a larger call", caps=False)
    st = torch.cuda.Stream()
    for i in range(3):
        again = check(m, s, rows, lengths, ("after the larger call", i), stream=st if i else None)
        assert again[0].tobytes() == want[0].tobytes() and np.array_equal(again[1], want[1])
    got = m.shortcut_routes(dev(rows.view(np.int32), np.int32), dev(lengths.view(np.int32), np.int32), stream=st, window=5, waypoint_cap=4)
    st.synchronize()
    ref = s.shortcut(rows, lengths, window=5, waypoint_cap=4)
    assert np.array_equal(to_np(got["waypoint_rows"]).view(np.uint32), ref[1]) and to_np(got["links_tested"]).tolist() == ref[0]["links_tested"].tolist()


def test_after_an_update_a_crop_and_with_another_robot():
    from grid_ndt_amd import scenes
    from tests.test_shortcut_host import staircase
    cloud = scenes.bridge_ground()
    P = scenes.BRIDGE_PARAMS
    m = build(cloud, P, ATOMIC)                          # (updates need the additive strategy)
    rng = np.random.default_rng(12)
    other = dict(reachable_height=0.05, max_angle_deg=12.0)
    shorter = 0

    def fresh(what):
        nonlocal shorter
        cells = m.export()
        for robot in (None, other, None):
            s = sr.Shortcutter(cells, cloud[0, :3], P["grid_len"], P["z_len"], robot)
            assert s.w.f.angle_margin_deg > MARGIN, (what, robot)
            rows, lengths = pack([staircase(rng, s.w, int(rng.integers(5, 70))) for _ in range(6)])
            info, _, _, _ = check(m, s, rows, lengths, (what, robot), robot=robot, entries=(False,), caps=False)
            shorter += int((info["waypoints"] < info["length_in"]).sum())
        return cells

    before = fresh("before")
    x0, x1 = int(before["sx"].min()), int(before["sx"].max())
    m.change2DMap("slope", dev(cloud[1:4000, :3] + np.float32([0.0, 0.0, 0.3])))
    fresh("update")
    m.crop_box((x0 + (x1 - x0) // 4, x1 - (x1 - x0) // 4, -100000, 100000), "keep_inside")
    cropped = fresh("crop")
    assert cropped["num_nodes"] < before["num_nodes"] and shorter > 0
    # everything cropped away: every row is out of range
    m.crop_box((x1 + 50, x1 + 60, 1, 2), "keep_inside")
    assert m.sync()[0] == 0
    for host in (False, True):
        rc, info, wp, path, untouched = raw(m, np.uint32([[0, 1, 2]]), np.uint32([3]), path_cap=2, host=host)
        assert rc == 0 and info["status"][0] == sr.BAD_ROUTE and (wp == sr.NO_ROW).all() and (path == sr.NO_ROW).all() and untouched


# ---- refusals --------------------------------------------------------------------------------------------------------------------------

def test_refused_arguments():
    import torch
    import grid_ndt_amd as g
    from grid_ndt_amd._lib import ShortcutParams
    m, s, cells = drawn("gap", _gap)
    rows, lengths = pack([route(cells, *GAP_ROUTE)])
    for host in (False, True):
        assert raw(m, rows, lengths, host=host)[0] == 0
        assert raw(m, rows, lengths, window=257, host=host)[0] == ERR_INVALID and raw(m, rows, lengths, window=256, host=host)[0] == 0
        for checks in (2, 3, 0x80000000):
            assert raw(m, rows, lengths, checks=checks, host=host)[0] == ERR_INVALID, checks
        assert raw(m, rows, lengths, max_links=(1 << 24) + 1, host=host)[0] == ERR_INVALID and raw(m, rows, lengths, max_links=1 << 24, host=host)[0] == 0
        for k in range(4):
            assert raw(m, rows, lengths, reserved=tuple(int(j == k) for j in range(4)), host=host)[0] == ERR_INVALID, k
        for stride in (8, 32):
            assert raw(m, rows, lengths, stride=stride, host=host)[0] == 0
    prm = ShortcutParams()
    buf = torch.zeros(256, dtype=torch.int32, device="cuda")
    d_rows, d_len = dev(rows.view(np.int32), np.int32), dev(lengths.view(np.int32), np.int32)
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    call = m._L.gndt_shortcut_routes_device
    R, N, B = p(d_rows), p(d_len), C.byref(prm)
    info, wp, path = p(buf), p(buf, 64), p(buf, 256)
    ok = lambda *a: call(m._h, *a)
    assert ok(R, 1, 11, N, 4, None, B, None, wp, 11, None, 0, info, None) == 0
    assert ok(R, 1, 11, N, 4, None, None, None, wp, 11, None, 0, info, None) == ERR_INVALID                   # NULL params
    assert ok(R, 1, 11, N, 4, None, B, None, wp, 11, None, 0, None, None) == ERR_INVALID                      # NULL info
    assert ok(None, 1, 11, N, 4, None, B, None, wp, 11, None, 0, info, None) == ERR_INVALID                   # NULL routes
    assert ok(R, 1, 11, None, 4, None, B, None, wp, 11, None, 0, info, None) == ERR_INVALID                   # NULL lengths
    assert ok(R, 1 << 31, 11, N, 4, None, B, None, wp, 11, None, 0, info, None) == ERR_INVALID                # K = 2^31
    assert ok(R, 1, 0, N, 4, None, B, None, wp, 11, None, 0, info, None) == ERR_INVALID                       # route_cap 0
    for stride in (0, 2, 3, 6, 13):
        assert ok(R, 1, 11, N, stride, None, B, None, wp, 11, None, 0, info, None) == ERR_INVALID, stride     # the stride
    assert ok(R, 1, 11, N, 4, None, B, None, None, 11, None, 0, info, None) == ERR_INVALID                    # NULL waypoint_rows
    assert ok(R, 1, 11, N, 4, None, B, None, wp, 11, path, 0, info, None) == ERR_INVALID                      # path rows without a cap
    assert ok(R, 1, 11, N, 4, None, B, None, wp, 11, None, 4, info, None) == ERR_INVALID                      # a cap without path rows
    assert ok(R, 1, 11, N, 4, None, B, None, wp, 11, None, 0, p(buf, 8), None) == ERR_INVALID                 # info not aligned to 16
    assert ok(p(d_rows, 2), 1, 11, N, 4, None, B, None, wp, 11, None, 0, info, None) == ERR_INVALID           # routes not aligned
    assert ok(R, 1, 11, p(d_len, 1), 4, None, B, None, wp, 11, None, 0, info, None) == ERR_INVALID            # lengths not aligned
    assert ok(R, 1, 11, N, 4, None, B, p(buf, 65), wp, 11, None, 0, info, None) == ERR_INVALID                # hops not aligned
    assert ok(R, 1, 11, N, 4, None, B, None, p(buf, 66), 11, None, 0, info, None) == ERR_INVALID              # waypoint rows not aligned
    assert ok(R, 1, 11, N, 4, None, B, None, wp, 11, p(buf, 258), 4, info, None) == ERR_INVALID               # path rows not aligned
    torch.cuda.synchronize()
    buf.zero_()
    assert ok(R, 0, 11, N, 4, None, B, None, wp, 11, None, 0, info, None) == 0                                # nothing to do
    assert ok(None, 0, 0, None, 4, None, B, None, wp, 0, None, 0, info, None) == 0
    assert call(None, R, 1, 11, N, 4, None, B, None, wp, 11, None, 0, info, None) == ERR_INVALID
    assert m._L.gndt_shortcut_routes(None, None, 1, 11, None, 4, None, B, None, None, 11, None, 0, None) == ERR_INVALID
    torch.cuda.synchronize()
    assert not buf.any()                                                      # K = 0 wrote nothing
    # no finished build
    e = g.TwoDmap(0.5, 0.25)
    e.setCloudFirst((0.0, 0.0, 0.0))
    with pytest.raises(g.GndtError) as err:
        e.shortcut_routes(d_rows, d_len)
    assert err.value.code == ERR_INVALID
    with pytest.raises(ValueError):
        m.shortcut_routes(d_rows)                                             # rows without lengths
    # a capturing stream: refused, and the capture goes on
    st = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    x = torch.zeros(16, device="cuda")
    with g.graph_capture(graph, stream=st):
        rc = call(m._h, R, 1, 11, N, 4, None, B, None, wp, 11, None, 0, info, C.c_void_p(st.cuda_stream))
        x.add_(1.0)
    assert rc == ERR_INVALID
    graph.replay()
    torch.cuda.synchronize()
    assert float(x[0]) == 1.0
    check(m, s, rows, lengths, "after the refused capture")


# ---- the poisoned tier -----------------------------------------------------------------------------------------------------------------

# This file's hand-drawn tests on memory that does not start out as zeros (tests/test_gpu_poisoned.py describes the variant, the bytes and
# the rule): one child a byte, one at a time.  measured_s: the whole child (interpreter start to exit) on the MI355X under the regular
# library; limit_s: three times that, rounded up to 10 s.
POISON_IDS = ["test_open_floor_a_staircase_and_a_straight_run", "test_l_corridor_one_cell_wide_keeps_its_corner",
              "test_a_wall_with_a_gap_puts_the_waypoint_into_the_gap", "test_two_storeys_a_link_that_ends_on_the_other_storey_is_refused",
              "test_a_pillar_with_a_real_clearance_field", "test_a_low_ceiling_with_and_without_the_overhead_check",
              "test_group_and_window_edges_on_a_corridor[65]", "test_a_bend_leaves_the_far_group_empty_and_max_links_to_the_link",
              "test_wavefront_and_workgroup_edges_of_K[5]", "test_one_call_mixes_every_status",
              "test_routes_straight_out_of_a_device_side_plan_and_driven_by_the_walks",
              "test_first_consumer_call_a_larger_call_before_and_a_second_stream"]
HERE = "tests/test_gpu_shortcut.py::"
GROUP = dict(measured_s=4.31, limit_s=20, ids=[HERE + i for i in POISON_IDS])


def test_every_node_id_of_the_poison_group_is_collected():
    poison_tier.ids_collected(GROUP["ids"])


def test_the_poison_limit_is_three_times_the_measured_time():
    poison_tier.limit_follows_rule(GROUP["measured_s"], GROUP["limit_s"])


@poison_tier.refused_under_variant
@pytest.mark.parametrize("byte", poison_tier.BYTES, ids=poison_tier.BYTE_IDS)
def test_hand_drawn_maps_under_poison(byte):
    poison_tier.run_group("the hand-drawn shortcut maps", GROUP["ids"], GROUP["limit_s"], byte)
