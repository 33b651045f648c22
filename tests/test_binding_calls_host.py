"""What the Python binding hands to the C library, and what it hands back, on the host path of every map consumer.

`_lib.lib` is replaced by a fake whose every `gndt_*` attribute records its arguments and returns 0: integers and floats by value,
`byref(struct)` as the list of the struct's field values, pointers as NULL ("0") or non-NULL ("P").  The fake `gndt_sync` writes fixed counts, the fake
`gndt_raster_shape` a fixed shape, and the fake `gndt_frontiers` / `gndt_segment_scan` a cluster count of 2.  Each consumer method is
called through its host twin with K or N of 0, 1 and 3, on a map of 0 rows and one of 5, with every optional output on and off, every
string-or-int mode in both spellings, `robot` None and given, and `hops` / `base` / `field` None, numpy and dict.  The call list and
every returned object's keys, dtypes and shapes are compared, with no tolerance, with tests/golden/binding_calls.json (the distinct
entries once, and the entry of every case), which

    python tests/test_binding_calls_host.py --record tests/golden/binding_calls.json [--package-root DIR]

wrote once from the binding as it was before it was folded into one body per method (DIR: a checkout of that commit).  The device
twins need a GPU: tests/test_gpu_binding_twins.py.  No libgndt is loaded here."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "binding_calls.json")


def _enc_value(tp, v):
    if tp is C.c_void_p:
        return "P" if v else "0"
    if isinstance(v, C.Structure):
        return _enc_struct(v)
    if isinstance(v, C.Array):
        return [x for x in v]
    return v


def _enc_struct(s):
    return [_enc_value(tp, getattr(s, name)) for name, tp in s._fields_]


def _enc_arg(a):
    if a is None:
        return "0"
    if hasattr(a, "_obj"):                      # byref(x)
        o = a._obj
        return {"&": _enc_struct(o) if isinstance(o, C.Structure) else _enc_arg(o)}
    if isinstance(a, C.c_void_p):
        return "P" if a.value else "0"
    if isinstance(a, C.Array):
        return [x for x in a]
    if isinstance(a, C._SimpleCData):
        return a.value
    if isinstance(a, (bool, np.bool_)):
        return bool(a)
    if isinstance(a, (int, np.integer)):
        return int(a)
    if isinstance(a, (float, np.floating)):
        return repr(float(a))
    if isinstance(a, bytes):
        return a.decode()
    raise TypeError(f"argument of type {type(a)}")


def _enc_result(r):
    if isinstance(r, dict):
        return {str(k): _enc_result(v) for k, v in r.items()}
    if isinstance(r, (tuple, list)):
        return [_enc_result(v) for v in r]
    if isinstance(r, np.ndarray):
        return f"{r.dtype.str}{list(r.shape)}"
    if isinstance(r, np.generic):
        return f"{r.dtype.str}[]"
    if r is None or isinstance(r, (bool, int, str)):
        return r
    if isinstance(r, float):
        return repr(r)
    raise TypeError(f"result of type {type(r)}")


class FakeLib:
    """Every gndt_* symbol: records the call, returns 0."""

    def __init__(self):
        self.calls = []
        self.counts = (5, 4, 3)                 # rows, columns, slopes of gndt_sync

    def __getattr__(self, name):
        if not name.startswith("gndt_"):
            raise AttributeError(name)

        def call(*args):
            self.calls.append([name] + [_enc_arg(a) for a in args])
            if name == "gndt_create":
                args[1]._obj.value = 1
            elif name == "gndt_sync":
                for a, v in zip(args[1:], self.counts):
                    a._obj.value = v
            elif name == "gndt_raster_shape":
                args[1]._obj.value, args[2]._obj.value = 4, 3
            elif name in ("gndt_frontiers", "gndt_segment_scan"):
                C.c_uint32.from_address(args[-1].value).value = 2       # counts[0]: the clusters found
            elif name == "gndt_last_error":
                return None
            return 0
        return call


ROBOT = {"radius": 0.3, "max_angle_deg": 25.0}


def _pts(k, w=3):
    return (np.arange(k * w, dtype=np.float32).reshape(k, w) * 0.25 + 0.5)


def _cases(rows):
    """-> {method: [(label, callable(m))]}: `rows` is the map's row count (what the fake gndt_sync says)"""
    hops_np = np.arange(rows, dtype=np.int32)
    hops_u = hops_np.astype(np.uint32)
    field = {"cost": np.zeros(rows, np.float32), "next": np.full(rows, -1, np.int32)}
    out = {}

    def add(method, label, fn):
        out.setdefault(method, []).append((f"rows{rows}:{label}", fn))

    for k in (0, 1, 3):
        p3, p4 = _pts(k), _pts(k, 4)
        add("plan_routes", f"K{k}", lambda m, p=p3: m.plan_routes(p))
        add("plan_routes", f"K{k}:host", lambda m, p=p4: m.plan_routes(p, host=True, route_cap=7, max_expansions=9, scratch_bytes=4096))
        add("plan_routes", f"K{k}:cap0", lambda m, p=p3: m.plan_routes(p, route_cap=0))
        add("query", f"N{k}", lambda m, p=p3: m.query(p))
        add("query", f"N{k}:cost", lambda m, p=p4: m.query(p, cost=True))
        add("walk_paths", f"K{k}", lambda m, k=k: m.walk_paths(np.zeros((k, 4, 3), np.float32)))
        add("walk_paths", f"K{k}:rows", lambda m, k=k: m.walk_paths(np.zeros((k, 2, 4), np.float32), rows=6, host=True))
        add("descend_routes", f"K{k}", lambda m, p=p3: m.descend_routes(p, field))
        add("descend_routes", f"K{k}:cap", lambda m, p=p4: m.descend_routes(p, field, route_cap=5, max_steps=11, host=True))
        routes = np.full((k, 6), -1, np.int32)
        lengths = np.zeros(k, np.int32)
        add("shortcut_routes", f"K{k}", lambda m, r=routes, ln=lengths: m.shortcut_routes(r, ln))
        add("shortcut_routes", f"K{k}:tuple", lambda m, r=routes, ln=lengths: m.shortcut_routes((r, {"length": ln.astype(np.uint32)}), path_cap=4,
                                                                                                  waypoint_cap=3, host=True))
        add("shortcut_routes", f"K{k}:strided", lambda m, r=routes, k=k: m.shortcut_routes(r, np.zeros((k, 8), np.uint32)[:, 1], waypoint_cap=0))
        add("footprints", f"K{k}", lambda m, k=k: m.footprints(_pts(k, 5), 0.4, 0.3))
        add("footprints", f"K{k}:yaw", lambda m, k=k: m.footprints(_pts(k, 4), 0.4, 0.3, rows=5, host=True))
        add("clear_rays", f"N{k}", lambda m, p=p3: m.clear_rays((0.0, 1.0, 2.0), p))
        add("clear_rays", f"N{k}:passes", lambda m, p=p4: m.clear_rays((0.0, 1.0, 2.0, 9.0), p, passes=True))
        add("cast_rays", f"N{k}", lambda m, p=p3: m.cast_rays((0.0, 1.0, 2.0), p))
        add("cast_rays", f"N{k}:each", lambda m, p=p4, k=k: m.cast_rays(_pts(k, 3), p, stats=True))
        dirs = _pts(k, 3)
        add("view_gain", f"K{k}", lambda m, k=k: m.view_gain(np.tile(np.eye(4)[None], (k, 1, 1)), _pts(2, 3), 3.0, host=True))
        add("view_gain", f"N{k}", lambda m, d=dirs: m.view_gain(np.eye(4)[:3], d, 3.0, per_ray=True, host=True))
        add("view_gain", f"K{k}:flat", lambda m, k=k: m.view_gain(np.zeros((k, 12)), _pts(2, 4), 3.0, per_ray=True, host=True))
        poses = np.tile(np.eye(4)[None], (max(k, 1), 1, 1))
        add("score_poses", f"N{k}", lambda m, p=p3, T=poses: m.score_poses(p, T))
        add("score_poses", f"N{k}:per_point", lambda m, p=p4, T=poses: m.score_poses(p, T[:, :3], per_point=0))
        add("score_derivs", f"N{k}", lambda m, p=p3, T=poses: m.score_derivs(p, T))
        add("segment_scan", f"N{k}", lambda m, p=p3: m.segment_scan(p))
        add("segment_scan", f"N{k}:labels", lambda m, p=p4: m.segment_scan(p, pose=np.eye(4), labels=True, max_clusters=3))
        add("segment_scan", f"N{k}:cap1", lambda m, p=p3: m.segment_scan(p, max_clusters=1))
        add("segment_scan", f"N{k}:cap0", lambda m, p=p3: m.segment_scan(p, max_clusters=0, labels=True))
        boxes = np.arange(k * 6, dtype=np.int64).reshape(k, 6)
        add("obstacle_field", f"B{k}", lambda m, b=boxes: m.obstacle_field(b))
        add("obstacle_field", f"B{k}:host", lambda m, b=boxes: m.obstacle_field(b.astype(np.int32), obstacle=False, host=True))
        goals = np.arange(k, dtype=np.int32)
        add("route_field", f"G{k}", lambda m, g=goals: m.route_field(g, host=True))
        add("route_field", f"G{k}:points", lambda m, p=p3, k=k: m.route_field(p, goal_costs=np.zeros(k, np.float32), next=False, host=True))

    if rows == 0:
        return out
    # every option once, at K or N of 3 on the map of 5 rows
    p = _pts(3)
    for mode in ("node", 0, "nearest_slope", 1):
        add("plan_routes", f"mode={mode!r}", lambda m, v=mode: m.plan_routes(p, start_mode=v))
        add("query", f"mode={mode!r}", lambda m, v=mode: m.query(p, mode=v))
    box = (-3, 2, 1, 4)
    for mode in ("lowest", 0, "highest", 1, "nearest_z", 2):
        add("raster", f"mode={mode!r}", lambda m, v=mode: m.raster(box, mode=v, host=True))
    add("raster", "z_ref", lambda m: m.raster(box, mode="nearest_z", z_ref=1.5, host=True))
    add("raster", "no layers", lambda m: m.raster(box, layers=(), host=True))
    for name in ("row", "z", "rough", "nodes", "h", "state"):
        add("raster", f"layer {name}", lambda m, v=name: m.raster(box, layers=(v,), host=True))
    add("raster", "all layers", lambda m: m.raster(box, layers=("row", "z", "rough", "nodes", "h", "state"), host=True))
    for cand in ("reached", 0, "slopes", 1):
        add("frontiers", f"candidates={cand!r}", lambda m, v=cand: m.frontiers(candidates=v, host=True))
    for rule in ("column", 0, "level", 1):
        add("frontiers", f"open_rule={rule!r}", lambda m, v=rule: m.frontiers(open_rule=v, level_reach=2, min_open=2, link_dz=3, min_size=4, host=True))
    add("frontiers", "box", lambda m: m.frontiers(box=box, host=True))
    add("frontiers", "labels", lambda m: m.frontiers(labels=True, host=True))
    for cap in (0, 1, 3):
        add("frontiers", f"cap{cap}", lambda m, v=cap: m.frontiers(max_clusters=v, host=True))
        add("frontiers", f"cap{cap}:labels", lambda m, v=cap: m.frontiers(max_clusters=v, labels=True, box=box, host=True))
    for src in (("blocked",), "open", ("blocked", "open", "overhead"), 5):
        add("clearance", f"sources={src!r}", lambda m, v=src: m.clearance(sources=v, host=True))
    for hops, nearest, sides in ((True, True, False), (False, False, True), (True, False, True), (False, False, False), (True, True, True)):
        add("clearance", f"out={hops},{nearest},{sides}", lambda m, a=hops, b=nearest, c=sides: m.clearance(hops=a, nearest=b, sides=c, max_hops=7,
                                                                                                          host=True))
    add("clearance", "robot", lambda m: m.clearance(robot=ROBOT, host=True))
    boxes = np.arange(18, dtype=np.int32).reshape(3, 6)
    seg = {k: np.arange(3, dtype=np.int32) for k in ("label", "sx_min", "sx_max", "sy_min", "sy_max", "sz_min", "sz_max")}
    seg["counts"] = np.array([2, 0, 0, 0], np.uint32)
    add("obstacle_field", "robot", lambda m: m.obstacle_field(boxes, robot=ROBOT))
    add("obstacle_field", "robot radius only", lambda m: m.obstacle_field(boxes, robot={"radius": 0.6}, levels_below=1))
    add("obstacle_field", "levels", lambda m: m.obstacle_field(boxes, inflate=1, max_hops=5, levels_above=2, levels_below=3, max_columns=100))
    add("obstacle_field", "segment dict", lambda m: m.obstacle_field(seg))
    add("obstacle_field", "segment dict, host", lambda m: m.obstacle_field(seg, host=True, obstacle=False))
    add("obstacle_field", "base numpy", lambda m: m.obstacle_field(boxes, base=hops_np))
    add("obstacle_field", "base uint32", lambda m: m.obstacle_field(boxes, base=hops_u))
    add("obstacle_field", "base dict", lambda m: m.obstacle_field(boxes, base={"hops": hops_np}, host=True))
    paths = np.zeros((3, 4, 3), np.float32)
    for mode in ("nearest_slope", 1, "node", 2):
        add("walk_paths", f"mode={mode!r}", lambda m, v=mode: m.walk_paths(paths, start_mode=v))
        add("descend_routes", f"mode={mode!r}", lambda m, v=mode: m.descend_routes(p, field, start_mode=v))
    add("walk_paths", "robot", lambda m: m.walk_paths(paths, robot=ROBOT, overhead=True, max_steps=50))
    add("walk_paths", "hops numpy", lambda m: m.walk_paths(paths, hops=hops_np, min_hops=2))
    add("walk_paths", "hops uint32", lambda m: m.walk_paths(paths, hops=hops_u, min_hops=2))
    add("walk_paths", "hops dict", lambda m: m.walk_paths(paths, hops={"hops": hops_np}, min_hops=2, rows=3))
    goals = np.arange(3, dtype=np.int32)
    add("route_field", "robot", lambda m: m.route_field(goals, robot=ROBOT, overhead=True, max_cost=9.0, max_rounds=12, host=True))
    add("route_field", "goal_costs", lambda m: m.route_field(goals.astype(np.int64), goal_costs=np.ones(3), host=True))
    add("route_field", "hops numpy", lambda m: m.route_field(goals, hops=hops_np, min_hops=1, soft_hops=3, soft_weight=0.5, host=True))
    add("route_field", "hops dict", lambda m: m.route_field(goals, hops={"hops": hops_u}, min_hops=1, next=False, host=True))
    add("descend_routes", "field float64", lambda m: m.descend_routes(p, {"cost": field["cost"].astype(np.float64), "next": field["next"].astype(np.int64)}))
    routes, lengths = np.full((3, 6), -1, np.int32), np.zeros(3, np.int32)
    add("shortcut_routes", "robot", lambda m: m.shortcut_routes(routes, lengths, robot=ROBOT, window=16, overhead=True, max_links=40))
    add("shortcut_routes", "hops numpy", lambda m: m.shortcut_routes(routes, lengths, hops=hops_np, min_hops=2))
    add("shortcut_routes", "hops dict", lambda m: m.shortcut_routes(routes.astype(np.int64), lengths.astype(np.int64), hops={"hops": hops_u}, min_hops=2))
    poses = _pts(3, 5)
    for w in ("cell", 0, "count", 1):
        add("footprints", f"weight={w!r}", lambda m, v=w: m.footprints(poses, 0.4, 0.3, weight=v))
    add("footprints", "robot", lambda m: m.footprints(poses, 0.4, 0.3, robot=ROBOT, max_dz=0.2, height=1.5, min_cells=4, min_cover=0.5))
    add("clear_rays", "options", lambda m: m.clear_rays((0.0, 1.0, 2.0), p, max_range=5.0, end_margin=0.2, min_passes=2, count_only=True))
    for mode in ("voxel", 0, "ndt", 1):
        add("cast_rays", f"mode={mode!r}", lambda m, v=mode: m.cast_rays((0.0, 1.0, 2.0), p, mode=v, min_count=2, max_range=9.0, min_range=0.5,
                                                                        cov_rel=0.02, cov_floor=1e-5, max_d2=6.0))
    add("view_gain", "options", lambda m: m.view_gain(np.eye(4), p, 3.0, min_count=2, min_range=0.5, host=True))
    T = np.tile(np.eye(4)[None], (3, 1, 1))
    add("score_poses", "options", lambda m: m.score_poses(p, T, neighbourhood=7, min_count=4, cov_rel=0.02, cov_floor=1e-5, max_d2=6.0, per_point=2))
    add("score_derivs", "options", lambda m: m.score_derivs(p, T, neighbourhood=7, min_count=4, cov_rel=0.02, cov_floor=1e-5, max_d2=6.0))
    for cl in (None, 4, "off_surface", ("off_surface", "unmapped")):
        add("segment_scan", f"classes={cl!r}", lambda m, v=cl: m.segment_scan(p, classes=v, neighbourhood=1, novel_d2=9.0, min_points=2, connectivity=6,
                                                                            min_cluster_points=3, min_cluster_cells=2, min_count=4, cov_rel=0.02,
                                                                            cov_floor=1e-5))
    return out


METHODS = ("plan_routes", "query", "raster", "frontiers", "clearance", "obstacle_field", "walk_paths", "route_field", "descend_routes",
           "shortcut_routes", "footprints", "clear_rays", "cast_rays", "view_gain", "score_poses", "score_derivs", "segment_scan")


def run_method(method):
    """-> {case label: {"calls": [...], "result": ...}} of one consumer method under the fake library"""
    from grid_ndt_amd import _lib, map2d
    real = _lib.lib
    got = {}
    try:
        for rows in (0, 5):
            fake = FakeLib()
            fake.counts = (rows, min(rows, 4), min(rows, 3))
            _lib.lib = lambda fake=fake: fake
            for label, fn in _cases(rows).get(method, ()):
                m = map2d.TwoDmap(0.5, 0.25)
                m.setCloudFirst((1.0, 2.0, 3.0))
                fake.calls.clear()
                result = fn(m)
                got[label] = {"calls": [c for c in fake.calls if c[0] not in ("gndt_create", "gndt_set_origin")], "result": _enc_result(result)}
                m._h = None                     # (nothing to destroy)
    finally:
        _lib.lib = real
    return json.loads(json.dumps(got))


def test_every_consumer_has_cases():
    assert set(_cases(5)) == set(METHODS)


@pytest.mark.parametrize("method", METHODS)
def test_host_calls_match_golden(method):
    with open(GOLDEN) as f:
        golden = json.load(f)
    want = {label: golden["entries"][i] for label, i in golden["cases"][method].items()}
    got = run_method(method)
    assert sorted(got) == sorted(want)
    for label in want:
        assert got[label]["calls"] == want[label]["calls"], f"{method} {label}: the C calls differ"
        assert got[label]["result"] == want[label]["result"], f"{method} {label}: the returned object differs"


@pytest.mark.parametrize("dtype", (np.int64, np.int32, np.uint32))
def test_hops_of_any_integer_width_reach_the_library_as_one_int32_a_row(dtype):
    """walk_paths, shortcut_routes and obstacle_field hand `hops` / `base` over as n 4-byte words: -1 stays CLEARANCE_BEYOND, 8-byte
    integers are converted by value (they were once reinterpreted, two words an entry)"""
    from grid_ndt_amd import _lib, map2d
    seen = {}

    class Reading(FakeLib):
        def __getattr__(self, name):
            call = FakeLib.__getattr__(self, name)
            at = {"gndt_walk_paths": 7, "gndt_shortcut_routes": 8, "gndt_obstacle_field": 6, "gndt_route_field": 6}.get(name)

            def reading(*args):
                if at is not None:
                    seen[name] = list((C.c_int32 * 5).from_address(args[at].value))
                return call(*args)
            return reading

    real, fake = _lib.lib, Reading()
    hops = np.array([-1, 0, 3, 70000, 2], dtype=np.int64).astype(dtype)
    try:
        _lib.lib = lambda: fake
        m = map2d.TwoDmap(0.5, 0.25)
        m.setCloudFirst((1.0, 2.0, 3.0))
        m.walk_paths(np.zeros((1, 2, 3), np.float32), hops=hops)
        m.shortcut_routes(np.full((1, 4), -1, np.int32), np.zeros(1, np.int32), hops=hops)
        m.obstacle_field(np.zeros((1, 6), np.int32), base=hops)
        m.route_field(np.zeros(1, np.int32), hops=hops, host=True)
        m._h = None
    finally:
        _lib.lib = real
    assert seen == {k: [-1, 0, 3, 70000, 2] for k in ("gndt_walk_paths", "gndt_shortcut_routes", "gndt_obstacle_field", "gndt_route_field")}


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", required=True)
    ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    a = ap.parse_args()
    sys.path.insert(0, a.package_root)
    entries, cases = [], {}                     # (many cases make the same calls: each distinct entry is stored once)
    for method in METHODS:
        for label, entry in run_method(method).items():
            if entry not in entries:
                entries.append(entry)
            cases.setdefault(method, {})[label] = entries.index(entry)
    with open(a.record, "w") as f:           # (one entry, and one method's cases, a line: a change shows as lines in a diff)
        enc = lambda v: json.dumps(v, separators=(",", ":"), sort_keys=True)
        f.write('{"cases":{\n' + ",\n".join(f"{enc(m)}:{enc(cases[m])}" for m in sorted(cases)) + '\n},\n"entries":[\n')
        f.write(",\n".join(enc(e) for e in entries) + "\n]}\n")
