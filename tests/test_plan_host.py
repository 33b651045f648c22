"""CPU tier: route planning's shared header (grid_ndt_amd/csrc/gndt_plan.hpp), compiled with g++ into tests/_plan_shim.so and run query by
query as the kernel's wavefronts run it, against hand-derived corridors and, route for route, against the oracle's findRoute
(oracle.compute_cost(..., start=p)["path"]) on the flat floor, the drivable site and the bridge; the queue's spill and compaction under
the sanitizers in a stand-alone program; and the product entry points refuse to run without a GPU.  Routes are compared for equality:
there is no tolerance anywhere."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from grid_ndt_amd import scenes
from tests import plan_ref as pr
from tests.host_emulation import HostMap, shim_deps
from tests.test_planner_hand_routes import GL, IV, SCENES, ZL, _cells_to_cloud, _centre, _expected_keys

HERE = os.path.dirname(os.path.abspath(__file__))
_maps = {}


def cached(key, make):
    if key not in _maps:
        _maps[key] = make()
    return _maps[key]


def floor():
    return cached("floor", lambda: pr.host_map(pr.floor_cloud(), pr.FLOOR_P, pr.FLOOR_GOAL, pr.FLOOR_ROBOT))


def floor_answers():
    pm = floor()
    return cached("floor_answers", lambda: pm.shim_routes(pm.start_points(pm.slopes)))


def check_route(pm, route, start_row):
    """what holds for every route whatever the planner's order: from the start slope to the goal, slope by slope through adjacent cells"""
    assert route[0] == start_row and route[-1] == pm.goal_row and len(set(route)) == len(route)
    r = np.asarray(route)
    assert ((pm.flags[r] & 2) != 0).all()
    step = lambda a, b: (np.abs(a - b) == 1) | ((a * b == -1) & (np.abs(a - b) == 2))        # (there is no cell 0)
    dx, dy = step(pm.sx[r[1:]], pm.sx[r[:-1]]), step(pm.sy[r[1:]], pm.sy[r[:-1]])
    assert ((dx & (pm.sy[r[1:]] == pm.sy[r[:-1]])) | (dy & (pm.sx[r[1:]] == pm.sx[r[:-1]]))).all()


# ---- 1. hand-derived corridors ----

@pytest.mark.parametrize("name", sorted(SCENES))
def test_corridor_route_is_the_hand_derived_one(native_lib, name):
    sc = SCENES[name]
    start, goal = _centre(sc["route"][0]), _centre(sc["route"][-1])
    hm = HostMap(_cells_to_cloud(sc["cells"]), dict(grid_len=GL, z_len=ZL, slope_interval=IV, demand="slope"))
    pm = pr.PlanMap(hm.cells, hm.origin, hm.P, goal, dict(radius=0.2))
    rows, info, _ = pm.shim_routes(np.float32([start]))
    route = pr.route_of(rows, info, 0)
    assert route is not None, info
    keys = ["%s/%d" % (hm.cells["morton"][r], pm.sz[r]) for r in route]
    assert keys == _expected_keys(sc["route"]), (name, keys)
    assert route == pm.oracle_route(start)
    # g of the goal: one cell per step, and the flood's h at the start is the same walk the other way
    assert abs(float(info["cost"][0]) - GL * (len(route) - 1)) < 1e-3 * len(route)
    assert info["h_start"][0] == pm.h[route[0]] and info["start_row"][0] == route[0]
    assert info["expansions"][0] >= len(route) - 1 and info["queue_peak"][0] >= 1


# ---- 2. flat floor: staircase ties everywhere, the (f, insertion order) rule decides every route ----

def test_floor_every_slope_is_a_start_and_routes_equal_the_oracles():
    pm = floor()
    assert pm.n == len(pm.slopes) == pr.FLOOR_N ** 2 and pm.rc == 0
    rows, info, re = floor_answers()
    assert (info["status"] == pr.FOUND).all() and (info["start_row"] == pm.slopes).all()
    assert (info["h_start"] == pm.h[pm.slopes]).all()
    starts = pm.start_points(pm.slopes)
    checked = 0
    for k in range(0, len(starts), 7):               # 229 starts spread over the floor
        route = pr.route_of(rows, info, k)
        assert route == pm.oracle_route(starts[k]), k
        check_route(pm, route, int(pm.slopes[k]))
        checked += 1
    assert checked >= 200
    k = int(np.flatnonzero(pm.slopes == pm.goal_row)[0])       # the goal as its own start: one slope, nothing expanded
    assert pr.route_of(rows, info, k) == [pm.goal_row] and info["expansions"][k] == 0 and info["cost"][k] == 0
    # the quirk path: a stale second entry of a closed slope is popped and expanded again (GlobalPlan.h has no closed test at the pop)
    assert re[:, 0].max() > 0


def test_floor_small_first_tier_spills_and_changes_nothing():
    pm = floor()
    rows, info, re = floor_answers()
    assert info["queue_peak"].max() > 64
    rows64, info64, re64 = pm.shim_routes(pm.start_points(pm.slopes), lds_entries=64)
    assert np.array_equal(rows, rows64) and pr.info_bytes(info) == pr.info_bytes(info64) and np.array_equal(re, re64)


def test_floor_guard_truncation_and_start_modes():
    pm = floor()
    rows, info, _ = floor_answers()
    starts = pm.start_points(pm.slopes)
    far = int(np.argmax(info["expansions"]))
    n_exp, length = int(info["expansions"][far]), int(info["length"][far])
    # the guard: one expansion short of what the query needs ends it with LIMIT and no route; exactly enough finds it
    r1, i1, _ = pm.shim_routes(starts[far:far + 1], max_expansions=n_exp - 1)
    assert i1["status"][0] == pr.LIMIT and i1["length"][0] == 0 and i1["expansions"][0] == n_exp - 1 and (r1 == pr.NO_ROW).all()
    assert i1["cost"][0] == pr.FLT_MAX and i1["start_row"][0] == info["start_row"][far]
    r2, i2, _ = pm.shim_routes(starts[far:far + 1], max_expansions=n_exp)
    assert pr.info_bytes(i2) == pr.info_bytes(info[far:far + 1]) and np.array_equal(r2[0], rows[far])
    # a queue too small for the query's peak: LIMIT as well
    r3, i3, _ = pm.shim_routes(starts[far:far + 1], lds_entries=64, queue_entries=int(info["queue_peak"][far]) - 1)
    assert i3["status"][0] == pr.LIMIT and i3["length"][0] == 0
    # truncation: the first route_cap rows, the true length
    cap = length - 3
    r4, i4, _ = pm.shim_routes(starts[far:far + 1], route_cap=cap)
    assert i4["length"][0] == length and np.array_equal(r4[0], rows[far, :cap])
    r5, i5, _ = pm.shim_routes(starts[far:far + 1], route_cap=0)
    assert r5.shape == (1, 0) and pr.info_bytes(i5) == pr.info_bytes(info[far:far + 1])
    # NEAREST_SLOPE: z does not have to fall into the slope's level
    lifted = starts[::97].copy()
    lifted[:, 2] += 3.0
    _, i6, _ = pm.shim_routes(lifted)
    assert (i6["status"] == pr.NO_START).all() and (i6["start_row"] == pr.NO_ROW).all() and (i6["h_start"] == pr.FLT_MAX).all()
    r7, i7, _ = pm.shim_routes(lifted, mode=pr.NEAREST_SLOPE)
    assert pr.info_bytes(i7) == pr.info_bytes(info[::97]) and np.array_equal(r7, rows[::97])
    assert pr.shim().planshim_default_expansions(len(pm.slopes)) == 4 * len(pm.slopes) + 1024


# ---- 3. the drivable site, three robots / demands ----

def site(run):
    def make():
        demand, radius = pr.SITE_RUNS[run]
        hm = HostMap(scenes.drivable_site(), dict(scenes.COST_PARAMS, demand=demand))
        pm = pr.PlanMap(hm.cells, hm.origin, hm.P, scenes.DRIVABLE_GOAL, dict(radius=radius))
        return pm, hm
    return cached(("site", run), make)


@pytest.mark.parametrize("run", sorted(pr.SITE_RUNS))
def test_site_routes_equal_the_oracles(run):
    pm, hm = site(run)
    assert pm.rc == 0
    pts, kinds = pr.site_starts(pm, bare_point=pr.find_bare_point(pm, scenes.drivable_site(), lambda p: hm.query(p, pr.NODE)))
    for kind, least in (("trav", 24), ("closed", 1), ("unreached", 24), ("goal", 1), ("off", 1), ("nan", 1), ("bare", 1)):
        assert (kinds == kind).sum() >= least, kind
    rows, info, re = pm.shim_routes(pts)
    status = info["status"]
    # Re-expansions of closed slopes: on this map, with this goal, NO start has one in any of the three runs — every traversable
    # (11 633 / 11 628 / 11 979), closed (17 / 22 / 335) and unreached (2 769 / 2 769 / 3 194) slope was tried, the shim's counter
    # stayed 0.  The quirk is asserted where it happens: the floor (up to 17 in a query) and the bridge (up to 96).
    assert re[:, 0].max() == 0
    # the oracle finds routes from every traversable and closed start and from no unreached one
    assert (status[np.isin(kinds, ("trav", "closed", "goal"))] == pr.FOUND).all()
    assert (status[kinds == "unreached"] == pr.NO_ROUTE).all()
    assert (status[np.isin(kinds, ("off", "nan", "bare"))] == pr.NO_START).all()
    lengths = info["length"][np.isin(kinds, ("trav", "closed"))]
    assert lengths.min() >= 2 and lengths.max() >= 60
    for k in pr.oracle_sample(kinds):
        route = pr.route_of(rows, info, k)
        assert (route or []) == pm.oracle_route(pts[k]), (run, k, kinds[k])
    for k in np.flatnonzero(status == pr.FOUND):
        check_route(pm, pr.route_of(rows, info, k), int(info["start_row"][k]))
    assert (info["cost"][status != pr.FOUND] == pr.FLT_MAX).all()
    # nothing on this map comes near the guard
    assert info["expansions"].max() < 4 * len(pm.slopes) and (status != pr.LIMIT).all()


# ---- 4. the bridge: columns with two surfaces, a goal on the deck and one under it ----

def bridge(which):
    def make():
        hm = cached("bridge_rows", lambda: HostMap(scenes.bridge_ground(), scenes.BRIDGE_PARAMS))
        return pr.PlanMap(hm.cells, hm.origin, hm.P, pr.BRIDGE_GOALS[which])
    return cached(("bridge", which), make)


@pytest.mark.parametrize("which", sorted(pr.BRIDGE_GOALS))
def test_bridge_routes_pick_the_surface_in_ascending_level_order(which):
    pm = bridge(which)
    assert pm.rc == 0 and pm.state[pm.goal_row] == 1
    # the goals sit in one column, the deck's slope above the ground's
    other = bridge("under" if which == "deck" else "deck")
    assert pm.sx[pm.goal_row] == other.sx[other.goal_row] and pm.sy[pm.goal_row] == other.sy[other.goal_row]
    assert (pm.sz[pm.goal_row] > other.sz[other.goal_row]) == (which == "deck")
    pts = pm.start_points(pr.bridge_start_rows(pm))
    rows, info, re = pm.shim_routes(pts)
    assert (info["status"] == pr.FOUND).all() and info["length"].max() >= 20
    longest = 0
    for k in range(len(pts)):
        route = pr.route_of(rows, info, k)
        assert route == pm.oracle_route(pts[k]), (which, k)
        check_route(pm, route, int(info["start_row"][k]))
        longest = max(longest, len(route))
    assert longest >= 20
    assert re[:, 0].max() > 0           # stale entries of closed slopes are expanded again here too
    if which == "deck":                 # and f falls along an edge: an entry goes in below the popped key (plan_ref.bridge_start_rows)
        assert re[-1, 1] > 0


# ---- 5. the queue under the sanitizers, in a program of its own ----

def test_queue_spill_and_compaction_under_sanitizers():
    pm = floor()
    exe = os.path.join(HERE, "_plan_queue_main")
    src = os.path.join(HERE, "plan_queue_main.cpp")
    csrc = os.path.join(os.path.dirname(HERE), "grid_ndt_amd", "csrc")
    deps = shim_deps(src, os.path.join(HERE, "plan_shim.cpp"))
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                               "-I", csrc, "-I", HERE, "-o", exe, src])
    starts = pm.start_points(pm.slopes[::5])
    with tempfile.NamedTemporaryFile(suffix=".plan") as f:
        np.array([pm.n, pm.tsize, len(starts), pm.goal_row, 0, 0, 0, 0], np.uint64).tofile(f)
        np.float32(list(pm.origin) + [pm.P["grid_len"], pm.P["z_len"], pm.P["slope_interval"], 0, 0]).tofile(f)
        rb = pm.robot
        np.float32([rb["radius"], rb["reachable_height"], rb["max_rough"], rb["max_angle_deg"]]).tofile(f)
        for a in (pm.sx, pm.sy, pm.sz, pm.mean, pm.normal, pm.rough, pm.flags, pm.row_ncol, pm.ctab_key, pm.ctab_val, pm.h.view(np.uint32), starts):
            np.ascontiguousarray(a).tofile(f)
        f.flush()
        r = subprocess.run([exe, f.name], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.split("\n")
    assert lines[0].startswith("same %d peak " % len(starts)) and int(lines[0].split()[-1]) > 128, r.stdout
    assert lines[1].startswith("limit ") and int(lines[1].split()[1]) > 0, r.stdout


# ---- 6. no CPU path ----

def test_no_cpu_fallback_for_planning(native_lib):
    import torch
    from grid_ndt_amd import _lib
    L = _lib.lib()
    prm = _lib.PlanParams()
    assert L.gndt_plan_routes(None, None, 0, 12, prm, None, 0, None) == 1
    assert L.gndt_plan_routes_device(None, None, 0, 12, prm, None, 0, None, None) == 1
    if torch.cuda.is_available():
        return                                          # (the GPU tier takes it from here)
    import grid_ndt_amd as g
    m = g.TwoDmap(0.5, 0.5)
    m.setCloudFirst((0, 0, 0))
    for call in (lambda: m.plan_routes(np.ones((4, 3), np.float32), route_cap=8), lambda: m.findRoute((1.0, 1.0, 1.0))):
        with pytest.raises(g.GndtError) as e:
            call()
        assert e.value.code == 2   # GNDT_ERR_NO_DEVICE
