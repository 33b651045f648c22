"""GPU tier: route planning (gndt_plan_routes_device / gndt_plan_routes, TwoDmap.plan_routes / findRoute).  On maps built and flooded on
the device — the flat floor, the drivable site under three robots / demands, the bridge with a goal on the deck and one under it —
every route equals the oracle's findRoute on the exported rows (at most 65 oracle calls a scene) and every byte of every query's info
and rows equals what the shared header gives on the host (tests/plan_shim.cpp) — equality, no tolerance.  Then the chunked launches,
the queue's spill tier, truncation, the edge inputs, repeat calls and streams, that nothing is modified, a new goal on the same map, the
refusals, and the C++ mirror's findRouteDevice."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from grid_ndt_amd import scenes
from tests import plan_ref as pr
from tests.gpu_kit import build, dev

pytestmark = pytest.mark.gpu

CAP = 256          # route_cap of the comparisons: above every route of these scenes (the longest is 174 slopes)
FIELDS = ("sx", "sy", "sz", "count", "first_idx", "mean", "cov", "rough", "normal", "flags")
_scenes = {}


def _flooded(m, cloud, P, goal, robot):
    """flood on the device, the oracle's flood of the exported rows beside it (bit-equal h, the same goal row)"""
    st = m.computeCost(goal, robot)
    pm = pr.PlanMap(m.export(), cloud[0], P, goal, robot)
    ce = m.cost_export()
    assert st["rc"] == pm.rc == 0
    assert np.array_equal(ce["h"].view(np.uint32), pm.h.view(np.uint32)) and np.array_equal(ce["state"], pm.state)
    return pm


def scene(name):
    """-> dict(m, pm, pts, kinds (None: every start is a slope), oracle (the queries compared with the oracle))"""
    if name in _scenes:
        return _scenes[name]
    if name == "floor":
        cloud, P = pr.floor_cloud(), pr.FLOOR_P
        m = build(cloud, P)
        pm = _flooded(m, cloud, P, pr.FLOOR_GOAL, pr.FLOOR_ROBOT)
        pts = pm.start_points(pm.slopes)
        s = dict(m=m, pm=pm, pts=pts, kinds=None, oracle=np.arange(0, len(pts), 25))
    elif name.startswith("site_"):
        demand, radius = pr.SITE_RUNS[name[5:]]
        cloud, P = scenes.drivable_site(), dict(scenes.COST_PARAMS, demand=demand)
        m = build(cloud, P)
        pm = _flooded(m, cloud, P, scenes.DRIVABLE_GOAL, dict(radius=radius))
        bare = pr.find_bare_point(pm, cloud, lambda p: m.query(p, "node"))
        pts, kinds = pr.site_starts(pm, bare_point=bare)
        s = dict(m=m, pm=pm, pts=pts, kinds=kinds, oracle=pr.oracle_sample(kinds))
    else:
        raise KeyError(name)
    _scenes[name] = s
    return s


_bridge = {}


def bridge(which):
    """One map, two goals: the flood is run again whenever the other goal is asked for (the tables of the first flood are kept)."""
    if "m" not in _bridge:
        _bridge["cloud"] = scenes.bridge_ground()
        _bridge["m"] = build(_bridge["cloud"], scenes.BRIDGE_PARAMS)
        _bridge["now"] = None
    m = _bridge["m"]
    if _bridge["now"] != which:
        pm = _flooded(m, _bridge["cloud"], scenes.BRIDGE_PARAMS, pr.BRIDGE_GOALS[which], None)
        _bridge["now"] = which
        if which not in _bridge:
            pts = pm.start_points(pr.bridge_start_rows(pm))
            _bridge[which] = dict(m=m, pm=pm, pts=pts, kinds=None, oracle=np.arange(len(pts)))
    return _bridge[which]


def host(rows, info):
    """(rows, info) of plan_routes as numpy: rows uint32, info in gndt_route_info's layout"""
    get = lambda v: v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)
    out = np.zeros(len(get(info["status"])), pr.INFO_DTYPE)
    for k in ("status", "length", "expansions", "queue_peak", "cost", "h_start"):
        out[k] = get(info[k])
    out["start_row"] = get(info["start_row"]).view(np.uint32)
    return np.ascontiguousarray(get(rows)).view(np.uint32), out


def shim_answers(s, cap=CAP, **kw):
    key = ("shim", cap, tuple(sorted(kw.items())))
    if key not in s:
        s[key] = s["pm"].shim_routes(s["pts"], route_cap=cap, **kw)
    return s[key]


def same(got, want, what):
    rows, info = got
    wrows, winfo = want[0], want[1]
    for k in pr.INFO_DTYPE.names:
        bad = np.flatnonzero(info[k].view(np.uint32) != winfo[k].view(np.uint32))
        assert len(bad) == 0, (what, k, bad[:5], info[k][bad[:5]], winfo[k][bad[:5]])
    assert np.array_equal(rows, wrows), what


def check_scene(s, name):
    m, pm, pts = s["m"], s["pm"], s["pts"]
    want = shim_answers(s)
    got = host(*m.plan_routes(dev(pts), route_cap=CAP))
    same(got, want, (name, "device"))
    rows, info = got
    assert info["length"].max() <= CAP
    for k in s["oracle"]:
        assert (pr.route_of(rows, info, k) or []) == pm.oracle_route(pts[k]), (name, int(k))
    return rows, info, want[2]


def test_floor_all_1600_starts_in_one_call():
    s = scene("floor")
    rows, info, re = check_scene(s, "floor")          # 1600 single-wave workgroups: more than the chip has CUs
    assert len(info) == 1600 and (info["status"] == pr.FOUND).all() and (info["start_row"] == s["pm"].slopes).all()
    assert re[:, 0].max() > 0 and info["queue_peak"].max() > 64


@pytest.mark.parametrize("run", sorted(pr.SITE_RUNS))
def test_site_routes(run):
    s = scene("site_" + run)
    rows, info, _ = check_scene(s, run)
    kinds, status = s["kinds"], info["status"]
    assert (status[np.isin(kinds, ("trav", "closed", "goal"))] == pr.FOUND).all()
    assert (status[kinds == "unreached"] == pr.NO_ROUTE).all()
    assert (status[np.isin(kinds, ("off", "nan", "bare"))] == pr.NO_START).all()
    assert (kinds == "trav").sum() == 24 and (kinds == "unreached").sum() == 24 and (kinds == "closed").sum() >= 1


@pytest.mark.parametrize("which", ["deck", "under", "deck"])       # the third run: back to the first goal, tables kept throughout
def test_bridge_routes_and_a_new_goal_on_the_same_map(which):
    s = bridge(which)
    rows, info, re = check_scene(s, which)
    assert (info["status"] == pr.FOUND).all() and info["length"].max() >= 20
    assert (rows[np.arange(len(rows)), info["length"] - 1] == s["pm"].goal_row).all()
    other = _bridge.get("under" if which == "deck" else "deck")
    if other is not None:
        assert other["pm"].goal_row != s["pm"].goal_row


def test_host_entry_point_and_find_route():
    s = scene("site_r025")
    m, pm, pts = s["m"], s["pm"], s["pts"]
    want = shim_answers(s)
    same(host(*m.plan_routes(pts, route_cap=CAP)), want, "gndt_plan_routes")
    same(host(*m.plan_routes(dev(pts), route_cap=CAP, host=True)), want, "host=True")
    k = int(np.flatnonzero(s["kinds"] == "trav")[3])
    assert m.findRoute(pts[k]) == pm.oracle_route(pts[k]) and len(pm.oracle_route(pts[k])) > 1
    assert m.findRoute(pts[np.flatnonzero(s["kinds"] == "unreached")[0]]) is None
    assert m.findRoute((np.nan, 0.0, 0.0)) is None


def test_chunked_launches_give_the_same_bytes():
    s = scene("floor")
    m, pm = s["m"], s["pm"]
    want = shim_answers(s)
    pts = s["pts"][::25]
    assert len(pts) == 64
    # a query's state: 16 bytes a row and 8 a queue entry beyond the LDS tier (include/gndt.h); room for 25 to 29 queries: 3 launches
    one = 16 * pm.n + 8 * pr.shim().planshim_queue_entries(len(pm.slopes))
    got = host(*m.plan_routes(dev(pts), route_cap=CAP, scratch_bytes=25 * one))
    same(got, (want[0][::25], want[1][::25]), "three launches")
    got = host(*m.plan_routes(dev(pts), route_cap=CAP, scratch_bytes=one))
    same(got, (want[0][::25], want[1][::25]), "one query a launch")
    import grid_ndt_amd as g
    with pytest.raises(g.GndtError) as e:
        m.plan_routes(dev(pts), route_cap=CAP, scratch_bytes=4096)
    assert e.value.code == 5       # GNDT_ERR_CAPACITY: one query does not fit
    same(host(*m.plan_routes(dev(pts), route_cap=CAP)), (want[0][::25], want[1][::25]), "after the refusal")


def test_capped_lds_tier_spills_and_gives_the_same_bytes():
    s = scene("floor")
    m = s["m"]
    want = shim_answers(s)
    assert want[1]["queue_peak"].max() > 64
    m.set_debug_option(m.DEBUG_PLAN_LDS_ENTRIES, 64)
    try:
        got = host(*m.plan_routes(dev(s["pts"]), route_cap=CAP))
    finally:
        m.set_debug_option(m.DEBUG_PLAN_LDS_ENTRIES, 1024)
    same(got, want, "64 entries in LDS")
    import grid_ndt_amd as g
    for bad in (0, 63, 100, 2048):
        with pytest.raises(g.GndtError):
            m.set_debug_option(m.DEBUG_PLAN_LDS_ENTRIES, bad)


def test_truncation_and_the_guard():
    s = scene("floor")
    m = s["m"]
    wrows, winfo, _ = shim_answers(s)
    pts = s["pts"][::25]
    lengths = winfo["length"][::25]
    cap = int(np.sort(lengths)[len(lengths) // 2])                 # half of the routes are longer than this
    assert (lengths > cap).any() and (lengths <= cap).any()
    rows, info = host(*m.plan_routes(dev(pts), route_cap=cap))
    same((rows, info), s["pm"].shim_routes(pts, route_cap=cap)[:2], "truncated")
    assert np.array_equal(info["length"], lengths) and np.array_equal(rows, wrows[::25, :cap])
    rows0, info0 = host(*m.plan_routes(dev(pts), route_cap=0))
    assert rows0.shape == (64, 0) and pr.info_bytes(info0) == pr.info_bytes(winfo[::25])
    few = int(np.median(winfo["expansions"][::25]))
    got = host(*m.plan_routes(dev(pts), route_cap=CAP, max_expansions=few))
    want = s["pm"].shim_routes(pts, route_cap=CAP, max_expansions=few)
    same(got, want, "guard")
    assert (got[1]["status"] == pr.LIMIT).any() and (got[1]["status"] == pr.FOUND).any()


def test_edge_inputs():
    s = scene("site_r025")
    m, pm, pts = s["m"], s["pm"], s["pts"]
    want = shim_answers(s)
    rows, info = m.plan_routes(dev(np.zeros((0, 3), np.float32)), route_cap=CAP)
    assert tuple(rows.shape) == (0, CAP) and len(info["status"]) == 0
    rows, info = m.plan_routes(np.zeros((0, 3), np.float32), route_cap=CAP)
    assert rows.shape == (0, CAP)
    pad = np.concatenate([pts, np.full((len(pts), 1), 7.0, np.float32)], 1)
    same(host(*m.plan_routes(dev(pad), route_cap=CAP)), want, "stride 16")
    same(host(*m.plan_routes(pad, route_cap=CAP)), want, "stride 16, host")
    # nearest_slope: the start is gndt_query's answer for the point, whatever its z
    lifted = pts.copy()
    lifted[:, 2] += np.float32(0.4)
    q = m.query(dev(lifted), "nearest_slope").cpu().numpy()
    got = host(*m.plan_routes(dev(lifted), start_mode="nearest_slope", route_cap=CAP))
    assert np.array_equal(got[1]["start_row"].view(np.int32), q) and (q >= 0).sum() > 40
    same(got, pm.shim_routes(lifted, mode=pr.NEAREST_SLOPE, route_cap=CAP)[:2], "nearest_slope")
    node = host(*m.plan_routes(dev(lifted), route_cap=CAP))
    qn = m.query(dev(lifted), "node").cpu().numpy()
    start = np.where((qn >= 0) & ((pm.flags[np.maximum(qn, 0)] & 2) != 0), qn, -1)
    assert np.array_equal(node[1]["start_row"].view(np.int32), start)


def test_repeat_calls_and_streams_give_identical_bytes():
    import torch
    s = scene("site_r06")
    m, pts = s["m"], dev(s["pts"])
    first = host(*m.plan_routes(pts, route_cap=CAP))
    same(host(*m.plan_routes(pts, route_cap=CAP)), first, "second call")
    torch.cuda.synchronize()
    outs = []
    for _ in range(2):
        st = torch.cuda.Stream()
        outs.append((st, m.plan_routes(pts, route_cap=CAP, stream=st)))
    for st, out in outs:
        st.synchronize()
        same(host(*out), first, "another stream")
    same(first, shim_answers(s), "the shim's")


def test_the_call_modifies_nothing():
    s = scene("site_true")
    m = s["m"]
    cells0, cost0 = m.export(), m.cost_export()
    m.plan_routes(dev(s["pts"]), route_cap=CAP)
    m.plan_routes(s["pts"], route_cap=8)
    cells1, cost1 = m.export(), m.cost_export()
    for k in FIELDS:
        assert np.array_equal(np.asarray(cells0[k]).view(np.uint8), np.asarray(cells1[k]).view(np.uint8)), k
    assert np.array_equal(cost0["h"].view(np.uint32), cost1["h"].view(np.uint32)) and np.array_equal(cost0["state"], cost1["state"])
    for k in ("rc", "levels", "traversable", "closed", "check_pushes"):
        assert cost0[k] == cost1[k]


def test_no_goal_gives_every_query_no_goal():
    cloud, P = pr.floor_cloud(8), pr.FLOOR_P
    m = build(cloud, P)
    assert m.computeCost((100.0, 100.0, 0.06), pr.FLOOR_ROBOT)["rc"] != 0
    pts = np.float32([[1.25, 1.25, 0.06], [np.nan, 0, 0], [2.25, 1.25, 0.06]])
    for starts in (dev(pts), pts):
        rows, info = host(*m.plan_routes(starts, route_cap=5))
        assert (info["status"] == pr.NO_GOAL).all() and (info["length"] == 0).all() and (rows == pr.NO_ROW).all()
        assert (info["start_row"] == pr.NO_ROW).all() and (info["cost"] == pr.FLT_MAX).all() and (info["h_start"] == pr.FLT_MAX).all()
        assert (info["expansions"] == 0).all() and (info["queue_peak"] == 0).all() and (info["reserved"] == 0).all()
    # a goal on the map afterwards: routes
    assert m.computeCost((1.25, 1.25, 0.06), pr.FLOOR_ROBOT)["rc"] == 0
    assert m.findRoute((3.25, 3.25, 0.06)) is not None


def test_refusals():
    import torch
    import grid_ndt_amd as g
    from grid_ndt_amd import _lib
    cloud, P = pr.floor_cloud(8), pr.FLOOR_P
    m = build(cloud, P)
    pts = dev(np.float32([[1.25, 1.25, 0.06], [2.25, 1.25, 0.06]]))

    def refused(call, code=1):
        with pytest.raises(g.GndtError) as e:
            call()
        assert e.value.code == code, e.value

    refused(lambda: m.plan_routes(pts, route_cap=8))                              # no cost map
    refused(lambda: m.plan_routes(pts.cpu().numpy(), route_cap=8))
    assert m.computeCost((1.25, 1.25, 0.06), pr.FLOOR_ROBOT)["rc"] == 0
    rows, info = host(*m.plan_routes(pts, route_cap=8))
    assert (info["status"] == pr.FOUND).all()
    # arguments
    L = m._L
    out_r, out_i = torch.zeros((2, 8), dtype=torch.int32, device="cuda"), torch.zeros((2, 8), dtype=torch.int32, device="cuda")
    raw = lambda prm, stride=12, r=out_r.data_ptr(), cap=8, i=out_i.data_ptr(), p=pts.data_ptr(): L.gndt_plan_routes_device(
        m._h, C.c_void_p(p), 2, stride, C.byref(prm) if prm is not None else None, C.c_void_p(r), cap, C.c_void_p(i), None)
    assert raw(_lib.PlanParams()) == 0
    for k in range(4):
        prm = _lib.PlanParams()
        prm.reserved[k] = 1
        assert raw(prm) == 1                                                     # reserved != 0
    assert raw(_lib.PlanParams(start_mode=2)) == 1 and raw(None) == 1 and raw(_lib.PlanParams(), stride=8) == 1
    assert raw(_lib.PlanParams(), r=0) == 1 and raw(_lib.PlanParams(), cap=0) == 1 and raw(_lib.PlanParams(), i=0) == 1
    assert raw(_lib.PlanParams(), p=0) == 1 and raw(_lib.PlanParams(), r=0, cap=0) == 0
    assert raw(_lib.PlanParams(), i=out_i.data_ptr() + 4) == 1                  # info_dev is written 16 bytes at a time
    torch.cuda.synchronize()
    # a capturing stream
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        p2 = dev(np.float32([[1.25, 1.25, 0.06], [2.25, 1.25, 0.06]]))
        stream.wait_stream(torch.cuda.default_stream())
        graph = torch.cuda.CUDAGraph()
        with pytest.raises(g.GndtError) as err:
            with g.graph_capture(graph, stream):
                m.plan_routes(p2, route_cap=8, stream=stream)
        assert err.value.code == 1
        del graph
        stream.synchronize()
        assert (host(*m.plan_routes(p2, route_cap=8, stream=stream))[1]["status"] == pr.FOUND).all()
        stream.synchronize()
    # a cost map made stale by an update
    m.change2DMap("slope", dev(cloud[1:40, :3] + np.float32([0.0, 0.0, 1.0])))
    m.sync()
    refused(lambda: m.plan_routes(pts, route_cap=8))
    assert m.computeCost((1.25, 1.25, 0.06), pr.FLOOR_ROBOT)["rc"] == 0
    assert (host(*m.plan_routes(pts, route_cap=8))[1]["status"] == pr.FOUND).all()


def test_cpp_find_route_device_equals_find_route(native_lib):
    from tests.test_compat_cpp import PLAN_CASES, _build_checker
    exe = _build_checker(native_lib, "plan_device_check")
    cloud, P = scenes.drivable_site(), scenes.COST_PARAMS
    with tempfile.NamedTemporaryFile(suffix=".f32") as f:
        np.ascontiguousarray(cloud, np.float32).tofile(f.name)
        for demand, start_xy, radius in PLAN_CASES:
            z = float(0.35 * np.sin(start_xy[0] / 7.0) + 0.25 * np.cos(start_xy[1] / 5.0))
            cmd = [exe, f.name, str(cloud.shape[0]), str(P["grid_len"]), str(P["z_len"]), str(P["slope_interval"]), demand]
            cmd += [repr(float(v)) for v in scenes.DRIVABLE_GOAL] + [repr(start_xy[0]), repr(start_xy[1]), repr(z), repr(radius)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            assert r.returncode == 0 and "findRouteDevice == findRoute OK" in r.stdout, r.stdout + r.stderr
