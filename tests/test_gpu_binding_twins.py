"""GPU tier: the two twins of every map consumer of the Python binding — torch CUDA input against host=True / numpy input — on one
small map and on an empty one, at K or N of 0, 1 and 3.  Both answers must have the same keys, the same bits, and the dtypes of
DTYPES, a literal table of what the binding returned before its two branches a method were folded into one body (device / host).
The map is a 16 x 16-column plane around the origin (so column indices of both signs) with a one-level step at x = 1 and a hole of
2 x 2 columns; the inputs are chosen so that every field of every record is non-zero somewhere and same-width neighbours differ
(FIELDS_SEEN lists what is asserted to be so): a swapped 16-bit half or a wrong 64-bit column of the device decode shows as a
difference from the host twin.  tests/test_binding_calls_host.py checks what the host twins hand to the C library."""
import numpy as np
import pytest
from tests.gpu_kit import dev as _dev

pytestmark = pytest.mark.gpu

P = dict(grid_len=0.5, z_len=0.25, slope_interval=0.08)
ORIGIN = (0.0, 0.0, -2.0)
ROBOT = {"radius": 0.25}
KS = (0, 1, 3)

I4, U4, F4, I8, U8, F8, U1, U2, B1 = "i4", "u4", "f4", "i8", "u8", "f8", "u1", "u2", "b1"
_ROUTE = {"rows": (I4, I4), "status": (I4, I4), "length": (I4, U4), "start_row": (I4, I4), "expansions": (I4, U4), "queue_peak": (I4, U4),
          "cost": (F4, F4), "h_start": (F4, F4)}
DTYPES = {      # key: (device, host)
    "query": {"0": (I4, I4), "1": (F4, F4), "2": (I4, I4)},
    "plan_routes": _ROUTE,
    "descend_routes": _ROUTE,
    "raster": {"row": (I4, I4), "z": (F4, F4), "rough": (F4, F4), "nodes": (I4, I4), "h": (F4, F4), "state": (I4, I4)},
    "frontiers": dict({k: (I4, I4) for k in ("label", "size", "best_row", "sx_min", "sx_max", "sy_min", "sy_max", "open_sides", "labels")},
                      best_h=(F4, F4), sum_px=(I8, I8), sum_py=(I8, I8), sum_pz=(I8, I8), counts=(I4, U4)),
    "clearance": {"hops": (I4, I4), "nearest": (I4, I4), "sides": (U1, U1), "counts": (I4, I4)},
    "obstacle_field": {"hops": (I4, I4), "obstacle": (I4, I4), "counts": (I4, I4)},
    "walk_paths": dict({k: (I4, I4) for k in ("status", "stop_side", "steps", "waypoints", "start_row", "end_row", "hops_min", "rows")},
                       length=(F4, F4), climb=(F4, F4), rough_max=(F4, F4)),
    "route_field": {"cost": (F4, F4), "next": (I4, I4), "counts": (I4, I4), "converged": (I4, I4)},
    "shortcut_routes": dict({k: (I4, I4) for k in ("status", "length_in", "waypoints", "path_slopes", "links_tested", "fallback_links",
                                                   "hops_min", "waypoint_rows", "path_rows")}, cost_in=(F4, F4), cost_out=(F4, F4)),
    "footprints": dict({k: (F4, F4) for k in ("z", "normal", "along", "across", "rms", "step_max", "bump_max", "headroom", "pitch", "roll")},
                       status=(I4, I4), flags=(I4, I4), centre_row=(I4, I4), cells=(I4, U2), support=(I4, U2), gaps=(I4, U2),
                       unknown=(I4, U2), ok=(B1, B1), rows=(I4, I4)),
    "clear_rays": {"passes": (I4, U4)},
    "cast_rays": {"row": (I4, I4), "range": (F4, F4), "d2": (F4, F4)},
    "view_gain": dict({k: (I4, U4) for k in ("rays", "skipped", "hits", "unknown", "known", "status")}, steps=(I8, U8), sum_ux=(I8, I8),
                      sum_uy=(I8, I8), row=(I4, I4), range=(F4, F4)),
    "score_poses": {"score": (F8, F8), "d2_sum": (F8, F8), "matched": (I8, I8), "terms": (I8, I8), "d2": (F4, F4), "row": (I4, I4)},
    "score_derivs": {"score": (F8, F8), "d2_sum": (F8, F8), "matched": (I8, I8), "terms": (I8, I8), "g": (F8, F8), "H": (F8, F8)},
    "segment_scan": dict({k: (I4, U4) for k in ("label", "cells", "off_surface", "unmapped", "counts")},
                         **{k: (I4, I4) for k in ("sx_min", "sx_max", "sy_min", "sy_max", "sz_min", "sz_max", "point_label")},
                         sum_x=(I8, I8), sum_y=(I8, I8), sum_z=(I8, I8), z_lo=(F4, F4), z_hi=(F4, F4), point_class=(U1, U1)),
}
# per method: the fields that must be non-zero somewhere at K or N = 3 on the map, and groups whose members must differ from each
# other.  Every field of every record is listed but those this level map keeps at zero whatever the pose: footprints' along, across,
# rms, step_max and bump_max (the supports of one level lie in one plane), walk_paths' climb (no walk changes height: the step is
# blocked), shortcut_routes' fallback_links (every link holds), view_gain's skipped and status (every ray and pose is valid) and
# segment_scan's off_surface (a metre over the ground no node counts).  Their columns are held apart by the random bytes of
# tests/test_abi_layout_host.py.
FIELDS_SEEN = {
    "plan_routes": (("status", "length", "start_row", "expansions", "queue_peak", "cost", "h_start"), []),
    "footprints": (("status", "flags", "centre_row", "cells", "support", "gaps", "unknown", "z", "normal", "headroom"),
                   [("cells", "support", "gaps", "unknown")]),
    "view_gain": (("rays", "hits", "unknown", "known", "steps", "sum_ux", "sum_uy"), [("sum_ux", "sum_uy"), ("unknown", "known")]),
    "frontiers": (("label", "size", "best_row", "best_h", "sx_min", "sx_max", "sy_min", "sy_max", "sum_px", "sum_py", "sum_pz", "open_sides"),
                  [("sum_px", "sum_py", "sum_pz"), ("sx_min", "sx_max", "sy_min", "sy_max")]),
    "segment_scan": (("label", "cells", "unmapped", "sx_min", "sx_max", "sy_min", "sy_max", "sz_min", "sz_max", "sum_x", "sum_y", "sum_z",
                      "z_lo", "z_hi"), [("sum_x", "sum_y", "sum_z"), ("z_lo", "z_hi")]),
    "walk_paths": (("status", "stop_side", "steps", "waypoints", "start_row", "end_row", "length", "rough_max", "hops_min"),
                   [("start_row", "end_row"), ("steps", "waypoints")]),
    "shortcut_routes": (("status", "length_in", "waypoints", "path_slopes", "links_tested", "cost_in", "cost_out", "hops_min"),
                        [("length_in", "waypoints")]),
}


def _cloud():
    per = 4
    a = -4.0 + (np.arange(16 * per) + 0.5) * (8.0 / (16 * per))
    X, Y = (v.ravel() for v in np.meshgrid(a, a, indexing="ij"))
    Z = np.where(X < 1.0, 0.05, 0.30)                                   # one level up from x = 1 on
    keep = ~((X > -2.0) & (X < -1.0) & (Y > 0.5) & (Y < 1.5))           # the hole
    return np.stack([X, Y, Z], 1)[keep].astype(np.float32)


def _new_map():
    import grid_ndt_amd as g
    m = g.TwoDmap(P["grid_len"], P["z_len"], strategy=1)
    m.setInterval(P["slope_interval"])
    m.setCloudFirst(ORIGIN)
    return m


@pytest.fixture(scope="module")
def plane(native_lib):
    m = _new_map()
    m.create2DMap("slope", _dev(_cloud()))
    assert 200 <= m.sync()[0] <= 300
    st = m.computeCost((-3.2, -3.3, 0.05), robot=ROBOT)
    assert st["rc"] == 0
    return m


@pytest.fixture(scope="module")
def empty(native_lib):
    m = _new_map()
    m.create2DMap("slope", np.zeros((0, 3), np.float32))
    assert m.sync()[0] == 0
    m.computeCost((-3.2, -3.3, 0.05), robot=ROBOT)       # (no goal in an empty map, but a cost map of the current grid)
    return m


def _flat(r):
    """a method's answer as one dict: a (rows, info) pair, a tuple or a (dict, stats) pair included"""
    if isinstance(r, dict):
        return dict(r)
    if isinstance(r, tuple) and len(r) == 2 and isinstance(r[1], dict) and not isinstance(r[0], dict):
        return dict(r[1], rows=r[0])
    if isinstance(r, tuple) and len(r) == 2 and isinstance(r[0], dict):
        out = dict(r[0])
        if isinstance(r[1], dict):
            out.update({"stats:" + k: v for k, v in r[1].items()})
        else:
            out["passes"] = r[1]
        return out
    return {str(i): v for i, v in enumerate(r)} if isinstance(r, tuple) else {"0": r}


def _agree(method, dev, host, cut=None):
    """same keys, DTYPES' dtypes, the same bits; cut: host lists are cut to the clusters found, device lists are not"""
    import torch
    dev, host = _flat(dev), _flat(host)
    assert set(dev) == set(host), (method, sorted(dev), sorted(host))
    for k in dev:
        d, h = dev[k], host[k]
        if not isinstance(d, torch.Tensor):
            assert not isinstance(h, np.ndarray) and (d == h or (d != d and h != h)), (method, k, d, h)
            continue
        assert d.is_cuda and isinstance(h, (np.ndarray, np.generic)), (method, k)
        d = d.cpu().numpy()
        h = np.asarray(h)
        assert (d.dtype.str[1:], h.dtype.str[1:]) == DTYPES[method][k], (method, k, d.dtype, h.dtype)
        if cut is not None and k != "counts" and d.shape != h.shape and d.ndim == 1 and k not in ("labels", "point_class", "point_label"):
            assert h.shape[0] == cut
            if k in ("size", "cells"):
                assert (d[cut:] == 0).all(), (method, k)
            d = d[:cut]
        assert d.shape == h.shape, (method, k, d.shape, h.shape)
        if d.dtype.itemsize == h.dtype.itemsize:
            same = np.ascontiguousarray(d).view(np.uint8).tobytes() == np.ascontiguousarray(h).view(np.uint8).tobytes()
        else:
            same = (d.astype(np.int64) == h.astype(np.int64)).all()
        assert same, (method, k, d, h)
    return host


def _seen(method, host):
    fields, groups = FIELDS_SEEN[method]
    print(method, {k: np.asarray(v).tolist() for k, v in host.items() if np.asarray(v).size <= 12})    # (the figures, before they are asserted)
    for k in fields:
        assert np.any(np.asarray(host[k]) != 0), (method, k, host[k])
    for grp in groups:
        for i, a in enumerate(grp):
            for b in grp[i + 1:]:
                assert np.any(np.asarray(host[a]).astype(np.float64) != np.asarray(host[b]).astype(np.float64)), (method, a, b, host[a])


def _refused(call):
    """The one place where the twins part, pinned as it is: at K = 0 a torch tensor without elements has a NULL data pointer, so a device
    twin that is asked for per-item rows (or, in descend_routes, hands over its empty info tensor) is refused by the library with
    GNDT_ERR_INVALID, where the host twin's empty numpy array still has an address and the call answers with nothing."""
    from grid_ndt_amd import GndtError
    with pytest.raises(GndtError) as e:
        call()
    assert e.value.code == 1


def _points(k):
    """on the plane: below the step, on it, at the hole's rim"""
    return np.array([[-3.2, 2.7, 0.05], [2.3, -1.2, 0.30], [-0.7, 0.8, 0.05]], np.float32)[:k]


@pytest.fixture(scope="module", params=("plane", "empty"))
def which(request):
    return request.param, request.getfixturevalue(request.param)


@pytest.mark.parametrize("k", KS)
def test_query_plan_descend_shortcut(which, k):
    name, m = which
    p = _points(k)
    _agree("query", m.query(_dev(p), "nearest_slope", cost=True), m.query(p, "nearest_slope", cost=True))
    dev = m.plan_routes(_dev(p), start_mode="nearest_slope", route_cap=64)
    host = m.plan_routes(p, start_mode="nearest_slope", route_cap=64, host=True)
    got = _agree("plan_routes", dev, host)
    # a search cut short knows the flood's h at its start and no cost: the one case in which the two differ
    cut = _agree("plan_routes", m.plan_routes(_dev(p), start_mode="nearest_slope", route_cap=64, max_expansions=3),
                 m.plan_routes(p, start_mode="nearest_slope", route_cap=64, max_expansions=3, host=True))
    if name == "plane" and k == 3:
        _seen("plan_routes", got)
        assert (cut["cost"] != cut["h_start"]).any()
    sh = m.shortcut_routes(host, robot=ROBOT, path_cap=16, host=True)
    if k:
        got = _agree("shortcut_routes", m.shortcut_routes(dev, robot=ROBOT, path_cap=16), sh)
    else:   # K = 0 with rows asked for: see _refused; without them the twins agree
        assert sh["path_rows"].shape == (0, 16) and sh["status"].shape == (0,)
        _refused(lambda: m.shortcut_routes(dev, robot=ROBOT, path_cap=16))
        _agree("shortcut_routes", m.shortcut_routes(dev, robot=ROBOT), m.shortcut_routes(host, robot=ROBOT, host=True))
    if name == "plane" and k == 3:
        _seen("shortcut_routes", got)
    rows = m.sync()[0]
    goals = np.array([3, rows - 5, 40], np.int32)[:k] if rows else np.zeros(0, np.int32)
    fd = m.route_field(_dev(goals, np.int32), robot=ROBOT)
    fh = m.route_field(goals, robot=ROBOT, host=True)
    _agree("route_field", fd, fh)
    dh = m.descend_routes(p, fh, route_cap=32, host=True)
    if k:
        _agree("descend_routes", m.descend_routes(_dev(p), fd, route_cap=32), dh)
    else:   # K = 0: the info tensor itself is empty, "null info"
        assert dh[0].shape == (0, 32) and dh[1]["status"].shape == (0,)
        _refused(lambda: m.descend_routes(_dev(p), fd, route_cap=32))


def test_raster_and_fields(which):
    name, m = which
    box = (-8, 8, -8, 8)
    layers = ("row", "z", "rough", "nodes", "h", "state")
    _agree("raster", m.raster(box, layers=layers), m.raster(box, layers=layers, host=True))
    cd = m.clearance(robot=ROBOT, sources=("blocked", "open"), sides=True)
    ch = m.clearance(robot=ROBOT, sources=("blocked", "open"), sides=True, host=True)
    _agree("clearance", cd, ch)
    for k in KS:
        boxes = np.array([[-3, -2, -3, -2, 9, 9], [4, 5, 1, 2, 10, 10], [-1, 1, 6, 7, 9, 9]], np.int32)[:k]
        _agree("obstacle_field", m.obstacle_field(_dev(boxes, np.int32), robot=ROBOT, base=cd), m.obstacle_field(boxes, robot=ROBOT, base=ch))
        paths = np.array([[[-3.2, -3.2, 0.05], [-0.3, -2.2, 0.05], [0.8, 3.1, 0.05]],
                          [[-3.0, 3.0, 0.05], [3.0, 3.0, 0.05], [np.nan, 0.0, 0.0]],
                          [[2.2, -2.2, 0.30], [3.3, 1.2, 0.30], [2.2, 3.3, 0.30]]], np.float32)[:k]
        wh = m.walk_paths(paths, robot=ROBOT, hops=ch, rows=8, host=True)
        if k:
            got = _agree("walk_paths", m.walk_paths(_dev(paths), robot=ROBOT, hops=cd, rows=8), wh)
        else:
            assert wh["rows"].shape == (0, 8) and wh["status"].shape == (0,)
            _refused(lambda: m.walk_paths(_dev(paths), robot=ROBOT, hops=cd, rows=8))
            _agree("walk_paths", m.walk_paths(_dev(paths), robot=ROBOT, hops=cd), m.walk_paths(paths, robot=ROBOT, hops=ch, host=True))
        if name == "plane" and k == 3:
            _seen("walk_paths", got)


@pytest.mark.parametrize("k", KS)
def test_footprints_and_views(which, k):
    name, m = which
    # over the step, whose upper side max_dz leaves without support (gaps); half over the map's edge and across the hole (unknown)
    poses = np.array([[0.8, 0.2, 0.05, 1.0, 0.2], [-3.6, -3.4, 0.05, -1.0, -0.5], [-1.5, 1.0, 0.05, 0.3, 1.0]], np.float32)[:k]
    kw = dict(robot=ROBOT, max_dz=0.1, height=1.0, min_cover=0.9, rows=6)
    fd = m.footprints(_dev(poses), 0.9, 0.6, **kw)
    fh = m.footprints(poses, 0.9, 0.6, host=True, **kw)
    got = _agree("footprints", fd, fh)
    if name == "plane" and k == 3:
        _seen("footprints", got)
    from grid_ndt_amd import rollouts
    dirs = rollouts.view_directions(1.2, 0.6, 6, 3)
    T = np.zeros((3, 3, 4))
    for i, (yaw, t) in enumerate(((np.pi * 0.9, (-2.6, -1.7, 0.45)), (np.pi * 1.2, (-3.1, 2.2, 0.5)), (0.3, (2.0, 2.0, 0.7)))):
        T[i] = [[np.cos(yaw), -np.sin(yaw), 0, t[0]], [np.sin(yaw), np.cos(yaw), 0, t[1]], [0, 0, 1, t[2]]]
    vd = m.view_gain(T[:k], dirs, 3.0, per_ray=True)
    vh = m.view_gain(T[:k], dirs, 3.0, per_ray=True, host=True)
    got = _agree("view_gain", vd, vh)
    if name == "plane" and k == 3:
        _seen("view_gain", got)
        assert (got["sum_ux"] < 0).any() and (got["sum_uy"] < 0).any()


@pytest.mark.parametrize("n", KS)
def test_rays_scores_and_segments(which, n):
    name, m = which
    ends = _points(n)
    o = (0.1, 0.2, 1.5)
    _agree("clear_rays", m.clear_rays(o, _dev(ends), count_only=True, passes=True), m.clear_rays(o, ends, count_only=True, passes=True))
    _agree("cast_rays", m.cast_rays(o, _dev(ends), stats=True), m.cast_rays(o, ends, stats=True))
    scan = _points(n) + np.float32(0.01)
    T = np.tile(np.eye(4)[None], (2, 1, 1))
    T[1, :3, 3] = (0.05, -0.02, 0.01)
    _agree("score_poses", m.score_poses(_dev(scan), T, neighbourhood=7, per_point=1), m.score_poses(scan, T, neighbourhood=7, per_point=1))
    _agree("score_derivs", m.score_derivs(_dev(scan), T, neighbourhood=7), m.score_derivs(scan, T, neighbourhood=7))
    # two points in one cell a metre over the plane and one over the step: clusters the map does not explain
    novel = np.array([[-2.3, 1.2, 1.1], [-2.2, 1.3, 1.15], [2.6, -3.1, 1.6]], np.float32)[:n]
    for cap in (None, 3):
        sd = m.segment_scan(_dev(novel), labels=True, max_clusters=cap)
        sh = m.segment_scan(novel, labels=True, max_clusters=cap)
        got = _agree("segment_scan", sd, sh, cut=min(int(sh["counts"][0]), cap) if cap else None)
        if name == "plane" and n == 3:
            _seen("segment_scan", got)


@pytest.mark.parametrize("cap", (None, 0, 1, 3))
def test_frontiers(which, cap):
    name, m = which
    fd = m.frontiers(candidates="slopes", labels=True, max_clusters=cap)
    fh = m.frontiers(candidates="slopes", labels=True, max_clusters=cap, host=True)
    got = _agree("frontiers", fd, fh, cut=min(int(fh["counts"][0]), cap) if cap is not None else None)
    if name == "plane" and cap is None:
        _seen("frontiers", got)
