"""GPU tier: what the map's consumers share.  The flood, the point queries, the raster export, count-only clears, the clearance field
and the path walks read one column index of the map: whichever of them comes first builds it — in the consume-first order that is the
clearance field, or a walk — and the answers do not depend on the order, also after an update, a crop and a clear have moved the map
on.  The flood's column-range error (|s| > 32767) holds whoever built the index, and the field and the walks answer the same before
and after it.  And the codes each consumer entry point returns on a map whose build reported points outside the codec's key range."""
import ctypes as C

import numpy as np
import pytest

from grid_ndt_amd import scenes
from tests.gpu_kit import dev, handle, to_np

pytestmark = pytest.mark.gpu

ATOMIC, PARTITION = 1, 2
ERR_KEY_RANGE = 4


def _setup(cells):
    """a goal on a slope near the middle of the rows, a box around the map, a sensor above the goal and ray ends from the rows"""
    slopes = np.flatnonzero(cells["flags"] & 2)
    goal = tuple(float(v) for v in cells["mean"][slopes[len(slopes) // 2]])
    box = (int(cells["sx"].min()) - 2, int(cells["sx"].max()) + 2, int(cells["sy"].min()) - 2, int(cells["sy"].max()) + 2)
    sensor = np.array([goal[0], goal[1], goal[2] + 2.0], np.float32)
    ends = np.ascontiguousarray(cells["mean"][:: max(1, cells["num_nodes"] // 4000)], np.float32)
    return goal, box, sensor, ends


def _paths(cells, grid_len, seed=48, around=None):
    """48 paths of 5 waypoints over the map's slopes — around = (a point, a distance): over those that near to it in x and y —
    segments of up to two cells an axis (tests/test_walk_host.random_paths)"""
    from tests.test_walk_host import random_paths
    on = cells["mean"][(cells["flags"] & 2) != 0]
    if around is not None:
        on = on[(np.abs(on[:, :2] - np.float32(around[0][:2])) < around[1]).all(1)]
    return random_paths(np.random.default_rng(seed), 48, 5, on[:, :2].min(0), on[:, :2].max(0), float(on[:, 2].min()), float(on[:, 2].max()),
                        reach=2 * grid_len, on=on)


def _reach(m, paths, walk_first=False):
    """The clearance field and the path walks, device and host entry points: the field with the map's edge as a barrier, the walks with
    its hops.  Whichever comes first builds the column index when no one has: the field, or (walk_first) a walk without a field."""
    out = {}

    def bare():
        out.update({"wk0_" + k: to_np(v) for k, v in m.walk_paths(dev(paths), rows=4).items()})

    if walk_first:
        bare()
    cl = m.clearance(sources=("blocked", "open"))
    out.update({"cl_" + k: to_np(v) for k, v in cl.items()})
    out.update({"clh_" + k: v for k, v in m.clearance(sides=True, host=True).items()})
    out.update({"wk_" + k: to_np(v) for k, v in m.walk_paths(dev(paths), hops=cl["hops"], rows=4).items()})
    out.update({"wkh_" + k: v for k, v in m.walk_paths(paths, hops=out["cl_hops"], rows=4, host=True).items()})
    if not walk_first:
        bare()
    return out


def _consume(m, pts, box, sensor, ends, paths, walk_first=False):
    out = _reach(m, paths, walk_first)
    out["node"] = to_np(m.query(dev(pts)))
    out["nearest"] = m.query(pts, mode="nearest_slope")                       # (host entry point)
    r = m.raster(box, "lowest", layers=("row", "z", "nodes"))
    out.update({"r_" + k: to_np(r[k]) for k in ("row", "z", "nodes")})
    out["r_high"] = m.raster(box, "highest", layers=("row",), host=True)["row"]
    st, w = m.clear_rays(sensor, dev(ends), count_only=True, passes=True)
    out["clear"] = st
    out["passes"] = to_np(w)
    st_h, w_h = m.clear_rays(sensor, ends, count_only=True, passes=True)
    out["clear_h"] = st_h
    out["passes_h"] = w_h
    return out


def _flood(m, goal):
    out = {"stats": m.computeCost(goal)}
    c = m.cost_export()
    out["h"], out["state"] = c["h"], c["state"]
    return out


def _both_orders(m, pts, goal, box, sensor, ends, paths, flood_first, walk_first=False):
    if flood_first:
        f = _flood(m, goal)
        c = _consume(m, pts, box, sensor, ends, paths, walk_first)
    else:
        c = _consume(m, pts, box, sensor, ends, paths, walk_first)
        f = _flood(m, goal)
    c.update(f)
    rows, h, state = m.query(dev(pts), cost=True)                             # the gather reads index and cost map together
    c.update(g_rows=to_np(rows), g_h=to_np(h), g_state=to_np(state))
    c["r_cost"] = m.raster(box, "nearest_z", goal[2], layers=("row", "h", "state"), host=True)
    return c


def _assert_equal(a, b):
    assert a.keys() == b.keys()
    for k in a:
        x, y = a[k], b[k]
        if isinstance(x, dict):
            assert x.keys() == y.keys(), k
            for j in x:
                if isinstance(x[j], np.ndarray):
                    assert np.array_equal(x[j].view(np.uint32) if x[j].dtype == np.float32 else x[j],
                                          y[j].view(np.uint32) if y[j].dtype == np.float32 else y[j]), (k, j)
                else:
                    assert x[j] == y[j], (k, j)
        else:
            x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
            assert x.shape == y.shape, k
            if x.dtype == np.float32:
                x, y = x.view(np.uint32), y.view(np.uint32)
            assert np.array_equal(x, y), (k, np.flatnonzero(x.ravel() != y.ravel())[:8])


def _assert_not_vacuous(c, cells):
    assert (c["node"] >= 0).all() and (c["r_row"] >= 0).any() and (c["r_row"] < 0).any()
    assert c["clear"]["rays"] > 0 and (c["passes"] & 0x7FFFFFFF).max() > 0
    assert c["stats"]["traversable"] > 0 and (c["h"] < np.float32(3e38)).any()
    assert c["node"].max() < cells["num_nodes"]
    assert c["cl_counts"][0] > 0 and c["cl_counts"][1] > c["cl_counts"][0]
    assert np.array_equal(c["clh_sides"] != 0xFF, (cells["flags"] & 2) != 0)
    for k in ("wk_status", "wkh_status", "wk0_status"):
        assert (c[k] == 0).any() and (c[k] != 0).any(), k           # GNDT_WALK_DONE and something else


@pytest.mark.parametrize("name", ["bridge_ground", "campus_partition"])
def test_flood_and_consumers_in_either_order_answer_the_same(name):
    if name == "bridge_ground":
        cloud, P, strategy = scenes.bridge_ground(), scenes.BRIDGE_PARAMS, 0
    else:
        cloud, P, strategy = scenes.campus_frame(200_000), scenes.CAMPUS_PARAMS, PARTITION
    pts = np.ascontiguousarray(cloud[1::7])
    res = []
    # the flood first; the consumers first, where the clearance field is what builds the index; the same with a walk in front of it
    for flood_first, walk_first in ((True, False), (False, False), (False, True)):
        m = handle(P, strategy)
        m.setCloudFirst(cloud[0])
        m.create2DMap("slope", dev(cloud[1:]))
        cells = m.export()
        goal, box, sensor, ends = _setup(cells)
        c = _both_orders(m, pts, goal, box, sensor, ends, _paths(cells, P["grid_len"]), flood_first, walk_first)
        _assert_not_vacuous(c, cells)
        res.append(c)
    _assert_equal(res[0], res[1])
    _assert_equal(res[0], res[2])


def test_either_order_on_an_updated_map_after_update_crop_and_clear():
    """a map built by gndt_update* (the node table a clear needs): each step moves the map on, so the index is built again in between"""
    import grid_ndt_amd as g
    cloud, P = scenes.campus_frame(200_000), scenes.CAMPUS_PARAMS
    body = cloud[1:]
    half = len(body) // 2
    pts = np.ascontiguousarray(body[::7])
    handles = []
    for _ in range(2):
        m = handle(P, ATOMIC)
        m.setCloudFirst(cloud[0])
        m.change2DMap("slope", dev(body[:half]))
        handles.append(m)
    cells = handles[0].export()
    goal, box, sensor, ends = _setup(cells)
    paths = _paths(cells, P["grid_len"], around=(goal, 25.0))           # (inside the crop below)
    crop = g.crop_box_from_world(cloud[0], P["grid_len"], (goal[0] - 30.0, goal[1] - 30.0), (goal[0] + 30.0, goal[1] + 30.0))
    steps = [("update", lambda m: m.change2DMap("slope", dev(body[half:]))),
             ("crop", lambda m: m.crop_box(crop, "keep_inside")),
             ("clear", lambda m: m.clear_rays(sensor, dev(ends)))]
    nodes = []
    for step, change in [("built", None)] + steps:
        if change is not None:
            outs = [change(m) for m in handles]
            if step == "clear":
                assert outs[0] == outs[1] and outs[0]["cleared"] > 0, outs
        cells = [m.export() for m in handles]
        for k in ("sx", "sy", "sz", "count", "mean"):
            assert np.array_equal(cells[0][k], cells[1][k]), (step, k)
        nodes.append(cells[0]["num_nodes"])
        res = [_both_orders(m, pts, goal, box, sensor, ends, paths, flood_first) for m, flood_first in zip(handles, (True, False))]
        assert (res[0]["r_row"] >= 0).any() and res[0]["clear"]["rays"] > 0, step
        assert res[0]["cl_counts"][0] > 0 and (res[0]["wk_status"] == 0).any() and (res[0]["wk_status"] != 0).any(), step
        _assert_equal(res[0], res[1])
    assert nodes[1] > nodes[0] > 0 and nodes[2] < nodes[1] and nodes[3] < nodes[2], nodes


def _far_column_map():
    """a small map with one column beyond |sx| = 32767 (within the codec's 65535): grid_len 0.1, a point 3.3 km out"""
    P = dict(grid_len=0.1, z_len=0.05, slope_interval=0.08)
    rng = np.random.default_rng(0x5EED0C01)
    near = np.column_stack([rng.uniform(-3, 3, 4000), rng.uniform(-3, 3, 4000), rng.uniform(0, 0.02, 4000)]).astype(np.float32)
    far = np.float32([[3300.02, 0.03, 0.0]] * 4)
    cloud = np.vstack([np.zeros((1, 3), np.float32), near, far])
    m = handle(P, ATOMIC)
    m.setCloudFirst(cloud[0])
    m.create2DMap("slope", dev(cloud[1:]))
    cells = m.export()
    assert np.abs(cells["sx"]).max() > 32767 and np.abs(cells["sx"]).max() <= 65535
    return m, cloud, cells


def test_flood_reports_column_range_whoever_built_the_index():
    import grid_ndt_amd as g
    goal = (0.05, 0.05, 0.01)

    def flood_code(m):
        with pytest.raises(g.GndtError) as e:
            m.computeCost(goal)
        return e.value.code

    m, cloud, cells = _far_column_map()                 # on its own
    assert flood_code(m) == ERR_KEY_RANGE
    m, cloud, cells = _far_column_map()                 # after a query has built the index
    pts = dev(cloud[1:])
    before = to_np(m.query(pts))
    assert (before >= 0).all()
    assert flood_code(m) == ERR_KEY_RANGE
    assert np.array_equal(to_np(m.query(pts)), before)
    assert flood_code(m) == ERR_KEY_RANGE               # twice in a row
    assert flood_code(m) == ERR_KEY_RANGE
    assert np.array_equal(to_np(m.query(pts)), before)
    # after the clearance field has built the index, and after a walk has: the column is in the map for both, the flood's range is not theirs
    rng = np.random.default_rng(0x5EED0C03)
    paths = np.zeros((48, 5, 3), np.float32)
    paths[:, 0, :2] = rng.uniform(-3, 3, (48, 2))
    paths[:, 1:, :2] = paths[:, :1, :2] + np.cumsum(rng.uniform(-0.2, 0.2, (48, 4, 2)), axis=1)
    paths[:, :, 2] = 0.01
    paths[0, :, :2] = (3300.02, 0.03)                   # (stands on the far column and goes nowhere)
    for first in ("clearance", "walk"):
        m, cloud, cells = _far_column_map()
        far = np.flatnonzero(np.abs(cells["sx"]) > 32767)
        assert len(far) == 1 and cells["flags"][far[0]] & 2

        def reach():
            out = {}
            if first == "walk":
                out.update({"wk_" + k: to_np(v) for k, v in m.walk_paths(dev(paths), rows=4).items()})
            out.update({"cl_" + k: to_np(v) for k, v in m.clearance(sources=("blocked", "open"), sides=True).items()})
            if first != "walk":
                out.update({"wk_" + k: to_np(v) for k, v in m.walk_paths(dev(paths), rows=4).items()})
            out.update({"clh_" + k: v for k, v in m.clearance(sides=True, host=True).items()})
            out.update({"wkh_" + k: v for k, v in m.walk_paths(paths, rows=4, host=True).items()})
            return out

        before = reach()
        assert before["cl_sides"][far[0]] == 0xF0 and before["cl_hops"][far[0]] == 0 and before["cl_counts"][0] > 0
        assert before["wk_status"][0] == 0 and before["wk_start_row"][0] == far[0] and (before["wk_start_row"][1:] != far[0]).all()
        assert flood_code(m) == ERR_KEY_RANGE
        _assert_equal(before, reach())
        assert flood_code(m) == ERR_KEY_RANGE


def test_consumer_codes_on_a_map_built_with_points_beyond_the_key_range():
    """the build reports GNDT_ERR_KEY_RANGE (points beyond |nx| = 65535 are left out, test_gpu_parity); what each consumer entry
    point then returns, each on a fresh handle"""
    import grid_ndt_amd as g
    from grid_ndt_amd import _lib
    P = dict(grid_len=0.5, z_len=0.1, slope_interval=0.08)
    rng = np.random.default_rng(0x5EED0C02)
    near = np.column_stack([rng.uniform(-20, 20, 20000), rng.uniform(-20, 20, 20000), rng.uniform(0, 0.05, 20000)]).astype(np.float32)
    cloud = np.vstack([near, np.float32([[0.5 * 70000, 0, 0]] * 4)])
    pts = np.ascontiguousarray(near[::5])
    box = _lib.CropBox(-10, 10, -10, 10)
    L = _lib.lib()

    def make(strategy):
        m = handle(P, strategy)
        m.setCloudFirst((0, 0, 0))
        with pytest.raises(g.GndtError) as e:
            m.create2DMap("slope", dev(cloud))
            m.sync()
        assert e.value.code == ERR_KEY_RANGE
        return m

    def raster(m, host):
        w = C.c_uint32(); ht = C.c_uint32()
        assert L.gndt_raster_shape(C.byref(box), C.byref(w), C.byref(ht)) == 0
        if host:
            out = np.empty(w.value * ht.value, np.int32)
            lay = _lib.RasterLayers(C.c_void_p(out.ctypes.data), None, None, None, None, None)
            return L.gndt_raster(m._h, C.byref(box), 0, 0.0, C.byref(lay))
        import torch
        out = torch.empty(w.value * ht.value, dtype=torch.int32, device="cuda")
        lay = _lib.RasterLayers(C.c_void_p(out.data_ptr()), None, None, None, None, None)
        rc = L.gndt_raster_device(m._h, C.byref(box), 0, 0.0, C.byref(lay), None)
        torch.cuda.synchronize()
        return rc

    def query(m, host):
        if host:
            rows = np.empty(len(pts), np.int32)
            return L.gndt_query(m._h, C.c_void_p(pts.ctypes.data), len(pts), 12, 0, C.c_void_p(rows.ctypes.data), None, None)
        import torch
        t = dev(pts)
        rows = torch.empty(len(pts), dtype=torch.int32, device="cuda")
        rc = L.gndt_query_device(m._h, C.c_void_p(t.data_ptr()), len(pts), 12, 0, C.c_void_p(rows.data_ptr()), None, None, None)
        torch.cuda.synchronize()
        return rc

    def clear(m, host):
        o = (C.c_float * 3)(0.0, 0.0, 2.0)
        prm = _lib.ClearParams(0.0, 0.0, 1, 1)
        st = _lib.ClearStats()
        if host:
            return L.gndt_clear_rays(m._h, o, C.c_void_p(pts.ctypes.data), len(pts), 12, C.byref(prm), None, C.byref(st))
        t = dev(pts)
        rc = L.gndt_clear_rays_device(m._h, o, C.c_void_p(t.data_ptr()), len(pts), 12, C.byref(prm), None, C.byref(st), None)
        return rc

    def crop(m, host):
        if host:
            return L.gndt_crop(m._h, C.byref(box), 0)
        return L.gndt_crop_device(m._h, C.byref(box), 0, None)

    room = 1 << 16                                      # (more entries than the map has rows, should a call go through)

    def clearance(m, host):
        prm = _lib.ClearanceParams(1, 4)
        if host:
            hops, cnt = np.zeros(room, np.uint32), np.zeros(4, np.uint32)
            return L.gndt_clearance(m._h, None, C.byref(prm), C.c_void_p(hops.ctypes.data), None, None, C.c_void_p(cnt.ctypes.data))
        import torch
        hops, cnt = torch.zeros(room, dtype=torch.int32, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
        rc = L.gndt_clearance_device(m._h, None, C.byref(prm), C.c_void_p(hops.data_ptr()), None, None, C.c_void_p(cnt.data_ptr()), None)
        torch.cuda.synchronize()
        return rc

    def walk(m, host):
        prm = _lib.WalkParams()
        paths = np.ascontiguousarray(pts[:8].reshape(4, 2, 3))
        if host:
            info = np.zeros(4 * 12, np.uint32)
            return L.gndt_walk_paths(m._h, C.c_void_p(paths.ctypes.data), 4, 2, 12, None, C.byref(prm), None, None, 0, C.c_void_p(info.ctypes.data))
        import torch
        t = dev(paths)
        info = torch.zeros(4 * 12, dtype=torch.int32, device="cuda")
        rc = L.gndt_walk_paths_device(m._h, C.c_void_p(t.data_ptr()), 4, 2, 12, None, C.byref(prm), None, None, 0, C.c_void_p(info.data_ptr()), None)
        torch.cuda.synchronize()
        return rc

    # (the clearance field and the walks start as the queries do — query_sync — and nothing in include/gndt.h says otherwise: the query's code)
    calls = {"query_device": (query, False), "query": (query, True), "raster_device": (raster, False), "raster": (raster, True),
             "crop_device": (crop, False), "crop": (crop, True), "clear_rays_device": (clear, False), "clear_rays": (clear, True),
             "clearance_device": (clearance, False), "clearance": (clearance, True), "walk_paths_device": (walk, False),
             "walk_paths": (walk, True)}
    want = {"query_device": ERR_KEY_RANGE, "query": ERR_KEY_RANGE, "raster_device": ERR_KEY_RANGE, "raster": ERR_KEY_RANGE,
            "crop_device": 0, "crop": ERR_KEY_RANGE, "clear_rays_device": 0, "clear_rays": 0,
            "clearance_device": ERR_KEY_RANGE, "clearance": ERR_KEY_RANGE, "walk_paths_device": ERR_KEY_RANGE, "walk_paths": ERR_KEY_RANGE}
    for strategy in (ATOMIC, PARTITION):
        got = {}
        for name, (fn, host) in calls.items():
            got[name] = fn(make(strategy), host)
        assert got == want, (strategy, got)
