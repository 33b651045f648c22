"""GPU tier: a large problem, then a small one, on ONE handle.  Every consumer of the map keeps scratch of its own on the handle and keeps
it when the next call needs less, so a small call after a large one finds the large call's leftovers there — where a fresh handle in a
fresh process finds zeroed pages.  For each consumer the handle answers a large problem (the 40 000-point box, a batch of more than
one workgroup plus a partial one, five poses), is rebuilt from every eighth point and cropped to one quadrant, and answers a small one
(37 points / rays / starts, one pose, another goal and robot).  The small answer must be, byte for byte, the answer of the same call on
a fresh handle that holds the same map, and must pass the consumer's restatement by the gate of that consumer's own test file.

"The same map" on a fresh handle: the sums of a build are fp64 atomics that arrive in any order, so two builds of one cloud differ in
the last bits of a few moments (tests/test_gpu_reproducible.py).  The fresh handle therefore receives the used handle's own
statistics (stats_export / stats_merge, the twins of tests/test_gpu_crop.py and tests/test_gpu_clear.py) and finalises them: the same
rows to the bit, in buffers that never held anything else.  Each test asserts that first.  Coarsen and merge add fp64 sums by atomics
themselves: their keys, counts, first-seen indices and tallies are compared exactly across the two handles, their sums by the
restatement's derived bound on either handle.

The clearance field and the path walks take lattice maps instead of the box (121 x 121 cells with two walls, then 41 x 25 with one,
cropped by a column line on either side; tests/clearance_ref.LATTICES), on which a field is tens of hops deep and walks are long;
their small answers equal the restatements exactly, and one test runs both consumers in turn on one used handle.

Every test asserts that it is not vacuous: the small call has matches / hits / routes / clusters, and fewer than the large one."""
import numpy as np
import pytest

from grid_ndt_amd import scenes
from oracle import oracle
from tests import cast_ref as cf
from tests import clear_ref as cr
from tests import clearance_ref as clr
from tests import coarsen_ref as cor
from tests import frontier_ref as fr
from tests import plan_ref as pr
from tests import query_ref as qr
from tests import raster_ref as rr
from tests import score_derivs_ref as dr
from tests import score_maps_ref as mr
from tests import score_ref as sr
from tests import walk_ref as wr
from tests.gpu_kit import dev as _dev

pytestmark = pytest.mark.gpu

ATOMIC = 1
BOX = dict(grid_len=0.5, z_len=0.5, slope_interval=0.08, demand="slope")
GL, ZL = BOX["grid_len"], BOX["z_len"]
FIELDS = ("sx", "sy", "sz", "count", "first_idx", "mean", "cov", "rough", "normal", "flags")
QUADRANT = (1, 4096, 1, 4096)          # the columns on the positive side of the origin on both axes
LARGE, SMALL = 4096 + 37, 37           # batch sizes: sixteen workgroups of 256 and a partial one; less than a wave, no power of two
MAP_LAYERS = ("row", "z", "rough", "nodes")
CAP = 256
# The box is no terrain: its slopes are scattered, and a robot has to be told to climb.  Under LARGE_ROBOT the flood of the large map
# from LARGE_GOAL_ROW reaches 387 of 455 slopes, under SMALL_ROBOT that of the small map from SMALL_GOAL_ROW 11 of 82 (the oracle's
# flood on the oracle's maps; the tests assert the floors below on the device's).
LARGE_ROBOT = dict(radius=0.1, reachable_height=0.6, max_rough=100.0, max_angle_deg=60.0)
SMALL_ROBOT = dict(radius=0.1, reachable_height=1.0, max_rough=100.0, max_angle_deg=89.0)
LARGE_GOAL_ROW, SMALL_GOAL_ROW = 3021, 721
_cache = {}


def _cloud():
    if "cloud" not in _cache:
        _cache["cloud"] = scenes.uniform_box(40_001, half_xy=6.0, half_z=1.0)
    return _cache["cloud"]


def _origin():
    return _cloud()[0]


def _body():
    return _cloud()[1:]


def _small_body():
    return np.ascontiguousarray(_body()[::8])


def _np(v):
    if isinstance(v, dict):
        return {k: _np(x) for k, x in v.items()}
    if isinstance(v, (tuple, list)):
        return type(v)(_np(x) for x in v)
    return v.cpu().numpy() if hasattr(v, "cpu") else v


def _handle(P=BOX, origin=None):
    import grid_ndt_amd as g
    m = g.TwoDmap(P["grid_len"], P["z_len"], strategy=ATOMIC)
    m.setInterval(P["slope_interval"])
    m.setCloudFirst(_origin() if origin is None else origin)
    return m


def _map_of(body, P=BOX):
    m = _handle(P)
    m.create2DMap("slope", _dev(body))
    m.sync()
    return m


def _large():
    """a handle that holds the large map"""
    return _map_of(_body())


def _same_bytes(a, b, what=""):
    """two answers (arrays, scalars, dicts, tuples of them), byte for byte"""
    a, b = _np(a), _np(b)
    if isinstance(a, dict):
        assert a.keys() == b.keys(), (what, sorted(a), sorted(b))
        for k in a:
            _same_bytes(a[k], b[k], (what, k))
    elif isinstance(a, (tuple, list)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _same_bytes(x, y, (what, i))
    elif isinstance(a, np.ndarray):
        x, y = np.ascontiguousarray(a), np.ascontiguousarray(b)
        assert x.shape == y.shape and x.dtype == y.dtype, (what, x.shape, y.shape, x.dtype, y.dtype)
        assert x.tobytes() == y.tobytes(), (what, np.flatnonzero(x.reshape(-1).view(np.uint8) != y.reshape(-1).view(np.uint8))[:8])
    else:
        assert a == b or (a != a and b != b), (what, a, b)


def _same_map(a, b, what):
    ea, eb = a.export(), b.export()
    for k in ("num_nodes", "num_columns", "num_slopes"):
        assert ea[k] == eb[k], (what, k, ea[k], eb[k])
    _same_bytes({k: ea[k] for k in FIELDS}, {k: eb[k] for k in FIELDS}, what)
    return ea


def _shrink_to(a, small, crop, P=BOX, origin=None):
    """The used handle `a` is rebuilt from the points `small` and cropped to the box `crop` -> (a fresh handle holding the same map —
    given `a`'s own statistics — and that map's export)."""
    a.create2DMap("slope", _dev(small))
    st = {k: v.clone() for k, v in a.stats_export().items()}
    b = _handle(P, origin)
    b.reset("slope")
    b.stats_merge(st["key"], st["sums"], st["count"], st["first_idx"])
    b.accumulate("slope", _dev(np.zeros((0, 3), np.float32)), first_idx_base=len(small))     # (the stream position of `a`)
    b.finalize()
    _same_map(a, b, "rebuilt")
    for m in (a, b):
        m.crop_box(crop, "keep_inside")
    return b, _same_map(a, b, "cropped")


def _shrink(a, n_large):
    """The used handle `a` is rebuilt from every eighth point and cropped to one quadrant -> (a fresh handle holding the same map, that
    map's export).  n_large: the node count `a` held before."""
    b, cells = _shrink_to(a, _small_body(), QUADRANT)
    assert 100 < cells["num_nodes"] < n_large // 2 and (cells["sx"] >= 1).all() and (cells["sy"] >= 1).all()
    assert ((cells["flags"] & 1) != 0).sum() > 50 and ((cells["flags"] & 2) != 0).sum() > 20
    return b, cells


def _points(n, seed, lo=(-6.5, -6.5, -1.2), hi=(6.5, 6.5, 1.2)):
    """n points of the box and a little beyond, a few of them not finite"""
    p = np.random.default_rng(seed).uniform(lo, hi, size=(n, 3)).astype(np.float32)
    p[5::97, 1] = np.nan
    return p


def _quadrant_points(n, seed):
    o = _origin()
    return _points(n, seed, lo=(o[0] - 0.7, o[1] - 0.7, -1.2), hi=(6.3, 6.3, 1.2))


def _yaw(deg, t=(0.0, 0.0, 0.0)):
    a = np.radians(deg)
    return np.array([[np.cos(a), -np.sin(a), 0, t[0]], [np.sin(a), np.cos(a), 0, t[1]], [0, 0, 1, t[2]]], np.float64)


POSES5 = np.stack([_yaw(0), _yaw(0, (0.3 * GL, 0, 0)), _yaw(0, (0, 0, 0.3 * ZL)), _yaw(2.0), _yaw(0, (5000.0, 0, 0))])
POSE1 = _yaw(1.0, (0.1 * GL, -0.05 * GL, 0.02 * ZL))[None]


# ---- query -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ilp", [1, 4])
def test_query(ilp):
    import grid_ndt_amd as g
    g.TwoDmap.set_debug_option(g.TwoDmap.DEBUG_QUERY_ILP, ilp)
    try:
        a = _large()
        big = _dev(_points(LARGE, 1))
        a.computeCost(tuple(a.export()["mean"][LARGE_GOAL_ROW]), LARGE_ROBOT)
        hits_large = {mode: int((_np(a.query(big, mode, cost=True)[0]) >= 0).sum()) for mode in ("node", "nearest_slope")}
        b, cells = _shrink(a, a.sync()[0])
        pts = _quadrant_points(SMALL, 2)
        t = _dev(pts)
        for mode, ref in (("node", qr.node_rows), ("nearest_slope", qr.nearest_slope_rows)):
            got = _np(a.query(t, mode))
            _same_bytes(got, b.query(t, mode), ("query", mode))
            _same_bytes(a.query(pts, mode), b.query(pts, mode), ("query, host", mode))
            want = ref(cells, pts, _origin(), GL, ZL)
            assert np.array_equal(got.astype(np.int64), want), (mode, np.flatnonzero(got != want)[:8])
            assert 0 < int((got >= 0).sum()) < hits_large[mode] and (got < 0).any()
        # the cost gather: a new goal and robot on the small map
        for m in (a, b):
            assert m.computeCost(tuple(cells["mean"][SMALL_GOAL_ROW]), SMALL_ROBOT)["rc"] == 0
        ga, gb = a.query(t, "nearest_slope", cost=True), b.query(t, "nearest_slope", cost=True)
        _same_bytes(ga, gb, "query with cost")
        rows, h, state = _np(ga)
        ce = a.cost_export()
        hit = rows >= 0
        assert np.array_equal(h[hit].view(np.uint32), ce["h"][rows[hit]].view(np.uint32)) and (state[hit] == ce["state"][rows[hit]]).all()
        assert (h[~hit] == qr.FLT_MAX).all() and (state[~hit] == 0).all()
    finally:
        g.TwoDmap.set_debug_option(g.TwoDmap.DEBUG_QUERY_ILP, 1)


# ---- raster ----------------------------------------------------------------------------------------------------------------------------

def _box_of(cells):
    return int(cells["sx"].min()), int(cells["sx"].max()), int(cells["sy"].min()), int(cells["sy"].max())


def test_raster():
    a = _large()
    big = a.export()
    x0, x1, y0, y1 = _box_of(big)
    filled_large = 0
    for mode, z in (("lowest", None), ("highest", None), ("nearest_z", 0.1)):
        for host in (False, True):
            r = a.raster((x0 - 3, x1 + 3, y0 - 3, y1 + 3), mode, z, layers=MAP_LAYERS, host=host)
        filled_large = int((_np(r["row"]) >= 0).sum())
    b, cells = _shrink(a, big["num_nodes"])
    sx0, sx1, sy0, sy1 = _box_of(cells)
    box = (sx0, sx1 - 2, sy0 - 1, sy1)              # an edge inside the map, one outside
    for mode, z in (("lowest", None), ("highest", None), ("nearest_z", 0.1)):
        for host in (False, True):
            got = _np(a.raster(box, mode, z, layers=MAP_LAYERS, host=host))
            _same_bytes(got, b.raster(box, mode, z, layers=MAP_LAYERS, host=host), ("raster", mode, host))
            want = rr.raster(cells, box, mode, 0.0 if z is None else z)
            for k in MAP_LAYERS:
                assert rr.same(got[k], want[k]), (mode, host, k)
            assert 0 < int((got["row"] >= 0).sum()) < filled_large and (got["row"] < 0).any()


# ---- clear: counting and clearing ------------------------------------------------------------------------------------------------------

def _sensor():
    return (_origin() + np.float32([0.2, 0.1, 0.05])).astype(np.float32)


def test_clear():
    a = _large()
    n_large = a.sync()[0]
    ends_large = np.ascontiguousarray(_body()[3::9][:LARGE])
    assert len(ends_large) == LARGE
    st_count, _ = a.clear_rays(_sensor(), _dev(ends_large), count_only=True, passes=True)
    st_large = a.clear_rays(_sensor(), _dev(ends_large))
    assert st_count["cleared"] == 0 and st_large["cleared"] > 0
    b, cells = _shrink(a, n_large)
    q = _small_body()
    q = q[(q[:, 0] > _origin()[0] + 1.0) & (q[:, 1] > _origin()[1] + 1.0)]
    ends = np.ascontiguousarray(q[::7][:SMALL])
    ends[11] = np.nan
    assert len(ends) == SMALL
    for mr_, em in ((0.0, 0.0), (4.0, 0.3)):
        want, rays, skipped = cr.passes(cells, _origin(), GL, ZL, _sensor(), ends, mr_, em)
        ga = a.clear_rays(_sensor(), _dev(ends), max_range=mr_, end_margin=em, count_only=True, passes=True)
        gb = b.clear_rays(_sensor(), _dev(ends), max_range=mr_, end_margin=em, count_only=True, passes=True)
        _same_bytes(ga, gb, ("count only", mr_, em))
        _same_bytes(a.clear_rays(_sensor(), ends, max_range=mr_, end_margin=em, count_only=True, passes=True),
                    b.clear_rays(_sensor(), ends, max_range=mr_, end_margin=em, count_only=True, passes=True), ("count only, host", mr_, em))
        st, words = ga[0], _np(ga[1]).view(np.uint32)
        assert (st["rays"], st["skipped"], st["cleared"]) == (rays, skipped, 0) and skipped == 1
        assert st["protected_rows"] == int(((want & cr.PROTECTED) != 0).sum()) > 0
        assert np.array_equal(words, want), np.flatnonzero(words != want)[:8]
    _same_map(a, b, "after counting")
    # the clear itself
    want, rays, skipped = cr.passes(cells, _origin(), GL, ZL, _sensor(), ends)
    drop = cr.cleared_rows(want, 1)
    ga, gb = a.clear_rays(_sensor(), _dev(ends), passes=True), b.clear_rays(_sensor(), _dev(ends), passes=True)
    _same_bytes(ga, gb, "clear")
    assert ga[0]["cleared"] == int(drop.sum()) and ga[0]["rays"] == rays
    assert 0 < ga[0]["cleared"] < st_large["cleared"]
    after = _same_map(a, b, "after the clear")
    keys = lambda c: qr.pack(c["sx"], c["sy"], c["sz"])
    assert after["num_nodes"] == cells["num_nodes"] - int(drop.sum())
    assert np.array_equal(np.sort(keys(after)), np.sort(keys(cells)[~drop]))    # the survivors


# ---- cast ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["voxel", "ndt"])
def test_cast(mode):
    a = _large()
    sensor = _sensor() + np.float32([0.0, 0.0, 2.5])                           # above the box, looking down and across
    rng = np.random.default_rng(5)
    ends_large = _points(LARGE, 6)
    origins_large = (sensor[None, :] + rng.uniform(-0.3, 0.3, size=(LARGE, 3))).astype(np.float32)
    _, st1 = a.cast_rays(sensor, _dev(ends_large), mode=mode, stats=True)
    _, st2 = a.cast_rays(_dev(origins_large), _dev(ends_large), mode=mode, stats=True)
    assert st1["hits"] > 0 and st2["hits"] > 0
    b, cells = _shrink(a, a.sync()[0])
    ends = _quadrant_points(SMALL, 7)
    ends[::3, 2] = -1.5                                                         # through the whole box
    origins = (sensor[None, :] + rng.uniform(-0.3, 0.3, size=(SMALL, 3))).astype(np.float32)
    for o, what in ((sensor, "one origin"), (origins, "an origin a ray")):
        od = o if o.ndim == 1 else _dev(o)
        ga, sa = a.cast_rays(od, _dev(ends), mode=mode, stats=True)
        gb, sb = b.cast_rays(od, _dev(ends), mode=mode, stats=True)
        _same_bytes((ga, sa), (gb, sb), ("cast", mode, what))
        _same_bytes(a.cast_rays(o, ends, mode=mode), b.cast_rays(o, ends, mode=mode), ("cast, host", mode, what))
        want = cf.cast(cells, _origin(), GL, ZL, o, ends, mode=cf.VOXEL if mode == "voxel" else cf.NDT)
        cf.assert_same(_np(ga), want, (mode, what))
        assert sa["hits"] == int((want["row"] != cf.NO_ROW).sum()) and 0 < sa["hits"] < min(st1["hits"], st2["hits"])
        assert sa["hits"] < sa["rays"] - sa["skipped"]


# ---- score, score derivatives ----------------------------------------------------------------------------------------------------------

def _scans():
    """(the large scan: LARGE points of the cloud; the small one: SMALL points of the quadrant's part of the small cloud)"""
    q = _small_body()
    q = q[(q[:, 0] > _origin()[0]) & (q[:, 1] > _origin()[1])]
    return np.ascontiguousarray(_body()[1::9][:LARGE]), np.ascontiguousarray(q[::5][:SMALL])


def test_score():
    a = _large()
    scan_large, scan = _scans()
    assert len(scan_large) == LARGE and len(scan) == SMALL
    large = {nbh: _np(a.score_poses(_dev(scan_large), POSES5, neighbourhood=nbh, per_point=3)) for nbh in (1, 7)}
    b, cells = _shrink(a, a.sync()[0])
    t = _dev(scan)
    for nbh in (1, 7):
        ga, gb = a.score_poses(t, POSE1, neighbourhood=nbh, per_point=0), b.score_poses(t, POSE1, neighbourhood=nbh, per_point=0)
        _same_bytes(ga, gb, ("score", nbh))
        _same_bytes(a.score_poses(scan, POSE1, neighbourhood=nbh, per_point=0), b.score_poses(scan, POSE1, neighbourhood=nbh, per_point=0),
                    ("score, host", nbh))
        want = sr.score(cells, _origin(), GL, ZL, scan, POSE1, nbh, 0)
        got = _np(ga)
        sr.assert_pose_sums(got, want, what=("reuse", nbh))
        sr.assert_per_point(got["d2"], got["row"], want["poses_out"][0], what=("reuse", nbh))
        assert 0 < int(got["matched"][0]) < int(large[nbh]["matched"][0]) and int(got["matched"][0]) < SMALL


def test_score_derivs():
    a = _large()
    scan_large, scan = _scans()
    large = {nbh: _np(a.score_derivs(_dev(scan_large), POSES5, neighbourhood=nbh)) for nbh in (1, 7)}
    b, cells = _shrink(a, a.sync()[0])
    t = _dev(scan)
    for nbh in (1, 7):
        ga, gb = a.score_derivs(t, POSE1, neighbourhood=nbh), b.score_derivs(t, POSE1, neighbourhood=nbh)
        _same_bytes(ga, gb, ("derivs", nbh))
        _same_bytes(a.score_derivs(scan, POSE1, neighbourhood=nbh), b.score_derivs(scan, POSE1, neighbourhood=nbh), ("derivs, host", nbh))
        want = dr.derivs(cells, _origin(), GL, ZL, scan, POSE1, nbh)
        got = _np(ga)
        dr.assert_derivs(got, want, what=("reuse", nbh))
        assert np.abs(got["H"][0]).max() > 0 and 0 < int(got["matched"][0]) < int(large[nbh]["matched"][0])


# ---- map-to-map score and derivatives --------------------------------------------------------------------------------------------------

def test_score_maps():
    a = _large()
    src_large = _map_of(_body()[1::2])
    large = {}
    for nbh in (1, 7):
        large[nbh] = _np(a.score_map(src_large, POSES5, neighbourhood=nbh, per_node=3))
        a.score_map_derivs(src_large, POSES5, neighbourhood=nbh)
    b, cells = _shrink(a, a.sync()[0])
    # the source of the small call: the other points of the quadrant, thinned as the map was
    q = _body()[4::8]
    src = _map_of(q[(q[:, 0] > _origin()[0]) & (q[:, 1] > _origin()[1])])
    src_cells = src.export()
    assert 0 < src_cells["num_nodes"] < src_large.sync()[0] // 2
    for nbh in (1, 7):
        ga, gb = a.score_map_derivs(src, POSE1, neighbourhood=nbh), b.score_map_derivs(src, POSE1, neighbourhood=nbh)
        _same_bytes(ga, gb, ("maps, derivs", nbh))
        pa, pb = a.score_map(src, POSE1, neighbourhood=nbh, per_node=0), b.score_map(src, POSE1, neighbourhood=nbh, per_node=0)
        _same_bytes(pa, pb, ("maps, score", nbh))
        want = mr.derivs(cells, _origin(), GL, ZL, src_cells, POSE1, nbh)
        mr.assert_derivs(_np(ga), want, what=("reuse", nbh))
        plain = _np(pa)
        mr.assert_pose_sums(plain, want, what=("reuse", nbh))
        mr.assert_per_node(plain["d2"], plain["row"], want["poses_out"][0], what=("reuse", nbh))
        assert 0 < int(plain["matched"][0]) < int(large[nbh]["matched"][0])
    # the used handle as the source of a fresh destination: the scratch of that side
    d1, d2 = _map_of(_small_body()), _map_of(_small_body())
    _same_bytes(d1.score_map(a, POSE1, per_node=0)["row"], d1.score_map(b, POSE1, per_node=0)["row"], "the used handle as the source")
    want = mr.score(d2.export(), _origin(), GL, ZL, cells, POSE1, 1, 0)
    got = _np(d2.score_map(a, POSE1, per_node=0))
    mr.assert_pose_sums(got, want, what="source")
    mr.assert_per_node(got["d2"], got["row"], want["poses_out"][0], what="source")


# ---- the cost flood, plan, frontiers: the second call also changes goal and robot ------------------------------------------------------

def _flood(m, cells, goal_row, robot):
    """the device's flood from the slope `goal_row`, checked against the oracle's flood of the same rows (tests/test_gpu_cost.py's gate)"""
    assert cells["flags"][goal_row] & 2
    goal = tuple(float(v) for v in cells["mean"][goal_row])
    st = m.computeCost(goal, robot=robot)
    got = m.cost_export()
    ref = oracle.compute_cost(cells, _origin(), GL, ZL, BOX["slope_interval"], goal, demand="slope", robot=robot)
    assert st["rc"] == ref["rc"] == 0
    assert ref["angle_margin_deg"] > 1e-3, "scene puts an angle within 1e-3 deg of the gate: pick another goal"
    np.testing.assert_array_equal(got["h"], ref["h"])
    np.testing.assert_array_equal(got["state"], ref["state"])
    assert (st["traversable"], st["closed"], st["check_pushes"], st["ring"]) == (ref["traversable"], ref["closed"], ref["check_pushes"], ref["ring"])
    return goal, st, got


@pytest.mark.parametrize("one_workgroup", [1, 0])
def test_cost_flood(one_workgroup):
    import grid_ndt_amd as g
    g.TwoDmap.set_debug_option(g.TwoDmap.DEBUG_COST_ONE_WORKGROUP, one_workgroup)
    try:
        a = _large()
        big = a.export()
        _, st_large, _ = _flood(a, big, LARGE_GOAL_ROW, LARGE_ROBOT)
        _flood(a, big, int(np.flatnonzero(big["flags"] & 2)[7]), SMALL_ROBOT)      # (a second goal and robot on the large map)
        assert st_large["traversable"] > 300
        b, cells = _shrink(a, big["num_nodes"])
        goal, st, got = _flood(a, cells, SMALL_GOAL_ROW, SMALL_ROBOT)
        stb = b.computeCost(goal, robot=SMALL_ROBOT)
        _same_bytes((st, got), (stb, b.cost_export()), "flood")
        assert 1 < st["traversable"] < st_large["traversable"]
    finally:
        g.TwoDmap.set_debug_option(g.TwoDmap.DEBUG_COST_ONE_WORKGROUP, 1)


def _plan_host(rows, info):
    """(rows, info) of plan_routes as numpy: rows uint32, info in gndt_route_info's layout (tests/test_gpu_plan.py's host())"""
    rows, info = _np(rows), _np(info)
    out = np.zeros(len(info["status"]), pr.INFO_DTYPE)
    for k in ("status", "length", "expansions", "queue_peak", "cost", "h_start"):
        out[k] = info[k]
    out["start_row"] = info["start_row"].view(np.uint32)
    return np.ascontiguousarray(rows).view(np.uint32), out


def test_plan():
    a = _large()
    big = a.export()
    goal, _, _ = _flood(a, big, LARGE_GOAL_ROW, LARGE_ROBOT)
    pm = pr.PlanMap(big, _origin(), BOX, goal, LARGE_ROBOT)
    starts_large = np.resize(pm.start_points(pm.slopes), (LARGE, 3)).astype(np.float32)
    _, info_large = _plan_host(*a.plan_routes(_dev(starts_large), route_cap=CAP))
    found_large = int((info_large["status"] == 0).sum())
    b, cells = _shrink(a, big["num_nodes"])
    goal, _, _ = _flood(a, cells, SMALL_GOAL_ROW, SMALL_ROBOT)
    assert b.computeCost(goal, robot=SMALL_ROBOT)["rc"] == 0
    pm = pr.PlanMap(cells, _origin(), BOX, goal, SMALL_ROBOT)
    starts = np.resize(pm.start_points(pm.slopes), (SMALL, 3)).astype(np.float32)
    starts[3] = np.nan
    starts[4] = (1e4, 1e4, 0.0)
    for mode in ("node", "nearest_slope"):
        ga, gb = a.plan_routes(_dev(starts), mode, route_cap=CAP), b.plan_routes(_dev(starts), mode, route_cap=CAP)
        _same_bytes(ga, gb, ("plan", mode))
        _same_bytes(a.plan_routes(starts, mode, route_cap=CAP), b.plan_routes(starts, mode, route_cap=CAP), ("plan, host", mode))
        rows, info = _plan_host(*ga)
        want = pm.shim_routes(starts, mode=pr.NODE if mode == "node" else pr.NEAREST_SLOPE, route_cap=CAP)
        for k in pr.INFO_DTYPE.names:
            bad = np.flatnonzero(info[k].view(np.uint32) != want[1][k].view(np.uint32))
            assert len(bad) == 0, (mode, k, bad[:5], info[k][bad[:5]], want[1][k][bad[:5]])
        assert np.array_equal(rows, want[0]), mode
        found = int((info["status"] == 0).sum())
        assert 0 < found < min(found_large, SMALL) and info["length"][info["status"] == 0].max() > 1
        if mode == "node":
            for k in np.flatnonzero(info["status"] == 0)[:5]:
                assert pr.route_of(rows, info, k) == pm.oracle_route(starts[k]), int(k)


@pytest.mark.parametrize("candidates", ["reached", "slopes"])
def test_frontiers(candidates):
    from tests.test_gpu_frontiers import cfg, check, raw
    cand = fr.REACHED if candidates == "reached" else fr.SLOPES
    a = _large()
    big = a.export()
    _flood(a, big, LARGE_GOAL_ROW, LARGE_ROBOT)
    large = {}
    for rule in (fr.OPEN_COLUMN, fr.OPEN_LEVEL):
        rc, got = raw(a, cfg(cand, rule))
        assert rc == 0
        large[rule] = got["counts"]
    b, cells = _shrink(a, big["num_nodes"])
    goal, _, cost = _flood(a, cells, SMALL_GOAL_ROW, SMALL_ROBOT)
    assert b.computeCost(goal, robot=SMALL_ROBOT)["rc"] == 0
    ref_map = fr.Map(cells)
    for rule in (fr.OPEN_COLUMN, fr.OPEN_LEVEL):
        c = cfg(cand, rule)
        got, _ = check(a, ref_map, c, cost, what=("reuse", candidates, rule))
        rc, other = raw(b, c)
        assert rc == 0
        _same_bytes({k: got[k] for k in ("label", "counts", "buf")}, {k: other[k] for k in ("label", "counts", "buf")}, ("frontiers", candidates, rule))
        _same_bytes(raw(a, c, host=True)[1]["buf"], raw(b, c, host=True)[1]["buf"], ("frontiers, host", candidates, rule))
        assert 0 < int(got["counts"][0]) and 0 < int(got["counts"][1]) < int(large[rule][1])
        # a list of two entries: cut, and nothing written behind it
        check(a, ref_map, c, cost, cap=2, what=("reuse, short list", candidates, rule))


# ---- crop ------------------------------------------------------------------------------------------------------------------------------

def test_crop():
    from tests.test_gpu_crop import _assert_same, _filtered
    a = _large()
    big = a.export()
    x0, x1, y0, y1 = _box_of(big)
    a.crop_box((x0 + 1, x1, y0, y1 - 1), "keep_inside")                # the large crop: nearly everything stays
    _assert_same(a.export(), _filtered(big, (x0 + 1, x1, y0, y1 - 1), "keep_inside"))
    dropped_large = big["num_nodes"] - a.sync()[0]
    small = _small_body()
    a.create2DMap("slope", _dev(small))
    mine = a.export()
    b, cells = _shrink(a, big["num_nodes"])                            # (rebuilds and crops both; compares them)
    # the same build's rows, filtered: _shrink rebuilt `a` once more, from the same points, so keys, counts and labels are `mine`'s
    want = _filtered(mine, QUADRANT, "keep_inside")
    for k in ("num_nodes", "num_columns", "num_slopes"):
        assert cells[k] == want[k], k
    for k in ("sx", "sy", "sz", "count", "first_idx", "flags"):
        assert np.array_equal(cells[k], want[k]), k
    # a second, smaller crop on both, against the filter of the handle's own rows
    sx0, sx1, sy0, sy1 = _box_of(cells)
    inner = (sx0 + 2, sx1 - 1, sy0 + 1, sy1 - 3)
    for m in (a, b):
        m.crop_box(inner, "drop_inside")
    after = _same_map(a, b, "second crop")
    _assert_same(after, _filtered(cells, inner, "drop_inside"))
    assert 0 < cells["num_nodes"] - after["num_nodes"] and 0 < after["num_nodes"] and dropped_large > 0


# ---- coarsen, merge --------------------------------------------------------------------------------------------------------------------

def _stats(m):
    import torch
    st = m.stats_export()
    torch.cuda.synchronize()
    st = {k: v.cpu().numpy().copy() for k, v in st.items()}
    order = np.argsort(st["key"].astype(np.uint64))
    return {"key": st["key"].astype(np.uint64)[order], "count": st["count"].astype(np.int64)[order] & 0xFFFFFFFF,
            "first_idx": st["first_idx"].astype(np.int64)[order] & 0xFFFFFFFF, "sums": st["sums"][order]}


def _exact(a, b, what):
    for k in ("key", "count", "first_idx"):
        assert np.array_equal(a[k], b[k]), (what, k)


def test_coarsen():
    a = _large()
    n_large = a.sync()[0]
    into_a = a.coarsen(2, 2)                                            # the large problem: the used source, a used destination
    parents_large = into_a.sync()[0]
    a.coarsen(2, 2, into=into_a)                                        # (and once more into the map it made)
    b, cells = _shrink(a, n_large)
    for fxy, fz in ((2, 2), (4, 1)):
        src = _stats(a)
        _exact(src, _stats(b), "sources")
        ca = a.coarsen(fxy, fz, into=into_a if (fxy, fz) == (2, 2) else None)
        cb = b.coarsen(fxy, fz)
        got, other = _stats(ca), _stats(cb)
        _exact(got, other, ("coarsen", fxy, fz))
        ea, eb = ca.export(), cb.export()
        for k in ("num_nodes", "num_columns", "num_slopes"):
            assert ea[k] == eb[k], k
        for k in ("sx", "sy", "sz", "count", "first_idx"):
            assert np.array_equal(ea[k], eb[k]), k
        want = cor.coarsen(src["key"], src["count"], src["first_idx"], src["sums"], fxy, fz, _origin(), GL, ZL)
        assert np.array_equal(got["key"], want["key"]) and np.array_equal(got["count"], want["count"].astype(np.int64))
        assert np.array_equal(got["first_idx"], want["first_idx"].astype(np.int64))
        for st in (got, other):
            assert (np.abs(st["sums"] - want["sums"]) <= want["tol"]).all()
        assert ea["num_nodes"] == len(want["key"]) and 0 < ea["num_nodes"] < min(parents_large, cells["num_nodes"])


def test_merge():
    from tests import merge_ref
    from tests.test_merge_host import rigid
    pose_large, pose = rigid(17.0, 4.0, (0.731, -0.419, 0.057)), rigid(-9.0, 2.0, (0.21, 0.33, -0.04))
    geo = (_origin()[:3], GL, ZL)
    a = _large()
    n_large = a.sync()[0]
    st_large = a.merge_from(_map_of(_body()[1::2]), pose=pose_large)
    assert st_large["merged_nodes"] > 1000 and a.sync()[0] > n_large
    b, cells = _shrink(a, n_large)
    q = _body()[4::8]
    src = _map_of(q[(q[:, 0] > _origin()[0]) & (q[:, 1] > _origin()[1])])
    s = _stats(src)
    prior = _stats(a)
    _exact(prior, _stats(b), "destinations")
    sta, stb = a.merge_from(src, pose=pose, min_count=2), b.merge_from(src, pose=pose, min_count=2)
    assert sta == stb, (sta, stb)
    got, other = _stats(a), _stats(b)
    _exact(got, other, "merge")
    want = merge_ref.merge(s, pose, geo, geo, prior=prior, min_count=2, base=len(_small_body()))
    assert sta == want["stats"], (sta, want["stats"])
    assert np.array_equal(got["key"], want["key"]) and np.array_equal(got["count"], want["count"].astype(np.int64))
    assert np.array_equal(got["first_idx"], want["first_idx"].astype(np.int64))
    for st in (got, other):
        assert (np.abs(st["sums"] - want["sums"]) <= want["tol"]).all()
    assert 0 < sta["merged_nodes"] < st_large["merged_nodes"] and sta["below_min_count"] > 0 and sta["new_nodes"] > 0
    ea, eb = a.export(), b.export()
    assert ea["num_nodes"] == eb["num_nodes"] == a.sync()[0] == len(want["key"])
    for k in ("sx", "sy", "sz", "count", "first_idx"):
        assert np.array_equal(ea[k], eb[k]), k


# ---- the clearance field, path walks -------------------------------------------------------------------------------------------------
# The box is useless here: its field is at most 2 hops deep on the large map and 1 on the small one, and no walk on it takes more than
# 10 steps.  Lattices instead (tests/clearance_ref.LATTICES; the CPU tier asserts their premises on the oracle's builds): the large map
# 121 x 121 cells with two walls — 14 641 rows, more than k_clearance_wg holds, so the large call takes a launch a hop whatever the
# option says — the small one 41 x 25 with one wall, cropped by a column line on either side of x: 975 rows.  The pointers into
# h->clearance.scratch and h->walk.scratch (gndt_api_clearance.hip, gndt_api_walk.hip: steps | keys | flags | tall) are computed from
# n, so on the used handle every region of the small call lies on another region's bytes of the large one.

LAT = fr.P
LAT_CROP = (2, 40, -4096, 4096)
OTHER_ROBOT = dict(reachable_height=0.05)


def _lattice_body(name):
    if ("lattice", name) not in _cache:
        cloud = clr.lattice(name, LAT)
        assert cloud[0].tobytes() == fr.ORIGIN.tobytes()
        _cache[("lattice", name)] = cloud[1:]
    return _cache[("lattice", name)]


def _lattice_large():
    """-> (a handle that holds the large lattice, its export, its restatement)"""
    a = _handle(LAT, fr.ORIGIN)
    a.create2DMap("slope", _dev(_lattice_body(14641)))
    a.sync()
    cells = a.export()
    f = clr.Field(cells)
    assert cells["num_nodes"] == 14641 > 9216 and ((cells["flags"] & 2) != 0).all() and f.angle_margin_deg > 1e-3
    return a, cells, f


def _lattice_small(a):
    b, cells = _shrink_to(a, _lattice_body("41x25"), LAT_CROP, LAT, fr.ORIGIN)
    assert cells["num_nodes"] == 39 * 25 and ((cells["flags"] & 2) != 0).all() and cells["sx"].min() == 2 and cells["sx"].max() == 40
    return b, cells


def _lattice_paths(cells, K, seed, reach):
    from tests.test_walk_host import random_paths
    on = cells["mean"][(cells["flags"] & 2) != 0]
    return random_paths(np.random.default_rng(seed), K, 6, on[:, :2].min(0), on[:, :2].max(0), 0.0, 0.1, reach=reach, on=on)


def _field(got):
    return {k: got[k] for k in ("hops", "nearest", "sides", "counts")}


@pytest.mark.parametrize("one_workgroup", [1, 0])
def test_clearance(one_workgroup):
    """gndt_api_clearance.hip `key[1] = key[0] + n; flags = ...(key[1] + n); tall = ...(flags + kFlagWords)` and `if (!wg)
    hipMemsetAsync(flags, 0, (max_hops + 1) * 4)`: after the large call the small call's keys lie on old steps, its flags on old keys,
    its tall bytes on old keys; the one-workgroup kernel (option 1: 975 rows fit) clears no flag word at all."""
    import tests.test_gpu_clearance as tgc
    with tgc.one_workgroup(bool(one_workgroup)):
        a, big, fl = _lattice_large()
        for host in (False, True):
            large = tgc.check(a, fl, clr.BLOCKED, 64, host=host, what=("large", host))
            tgc.check(a, fl, clr.BLOCKED | clr.OPEN | clr.OVERHEAD, 7, host=host, what=("large, 7 hops", host))
        assert tuple(large["counts"]) == (412, 14596, 64, 0)
        b, cells = _lattice_small(a)
        fs = clr.Field(cells)
        assert fs.angle_margin_deg > 1e-3 and cells["num_nodes"] < big["num_nodes"] // 8
        for max_hops in (3, 64):
            got = tgc.check(a, fs, clr.BLOCKED, max_hops, what=("small", max_hops))
            for host in (False, True):
                (ra, ga), (rb, gb) = tgc.raw(a, clr.BLOCKED, max_hops, host=host), tgc.raw(b, clr.BLOCKED, max_hops, host=host)
                assert ra == rb == 0 and tgc.untouched(ga) and tgc.untouched(gb)
                _same_bytes(_field(ga), _field(gb), ("clearance", max_hops, host))
                _same_bytes(_field(ga), _field(got), ("clearance, the restatement's", max_hops, host))
            assert 0 < got["counts"][1] < large["counts"][1] and got["counts"][0] > 0
            assert (got["hops"] == clr.BEYOND).any() if max_hops == 3 else got["counts"][2] >= 10


@pytest.mark.parametrize("table", [1, 0])
def test_walk(table):
    """gndt_api_walk.hip `key0 = ...(step + 4 * n); flag = ...(key0 + n); tall = ...(flag + 2)` in h->walk.scratch, which only the
    table variant touches (option 1), and stage_pieces' staging area, which both host entry points share: a large batch with the
    large map's field, then 37 paths with the small map's.  (With min_hops = 2 no walk is ever BLOCKED — a slope beside a blocked side
    has hops 0 and ends the walk one step earlier — so the large batch is also walked without a limit.)"""
    import tests.test_gpu_walk as tgw
    with tgw.step_table(bool(table)):
        a, big, fl = _lattice_large()
        field = a.clearance(max_hops=64)
        paths_large = _lattice_paths(big, LARGE, 11, 3.0)
        dev = _np(a.walk_paths(_dev(paths_large), hops=field, min_hops=2, rows=4))
        _same_bytes(dev, a.walk_paths(paths_large, hops=field, min_hops=2, rows=4, host=True), "large, host")
        assert {wr.DONE, wr.TOO_CLOSE, wr.LEFT_MAP} <= set(dev["status"].tolist())
        free = _np(a.walk_paths(_dev(paths_large), hops=field, rows=4))
        assert {wr.DONE, wr.BLOCKED} <= set(free["status"].tolist()) and free["steps"].max() > 10
        b, cells = _lattice_small(a)
        fa, fb = _np(a.clearance()), _np(b.clearance())
        _same_bytes(fa, fb, "the small field")
        hops = fa["hops"].view(np.uint32)
        assert np.array_equal(hops, clr.Field(cells).clearance(clr.BLOCKED, 32)["hops"])
        paths = _lattice_paths(cells, SMALL, 12, 1.5)
        for robot in (None, OTHER_ROBOT):
            w = wr.Walker(cells, fr.ORIGIN, fr.GL, fr.ZL, robot)
            assert w.f.angle_margin_deg > 1e-3
            want_info, want_rows, _ = w.walk(paths, hops=hops, min_hops=2, row_cap=6)
            for host in (False, True):
                ra = tgw.raw(a, paths, robot=robot, hops=hops, min_hops=2, row_cap=6, host=host)
                rb = tgw.raw(b, paths, robot=robot, hops=hops, min_hops=2, row_cap=6, host=host)
                assert ra[0] == rb[0] == 0 and ra[3] and rb[3], (robot, host)
                assert ra[1].tobytes() == rb[1].tobytes() and ra[2].tobytes() == rb[2].tobytes(), (robot, host)
                wr.same(ra[1], ra[2], want_info, want_rows, ("reuse", robot, host))
            seen = set(want_info["status"].tolist())
            assert len(seen) >= 3 and {wr.DONE, wr.TOO_CLOSE} <= seen and want_info["steps"].max() > 3, seen


def test_clearance_then_walk_share_nothing():
    """gndt_handle.hpp's h->clearance.scratch and h->walk.scratch are two areas: a walk through the table (k_clearance_steps into the
    walk's own steps, keys and flag) between two clearance calls changes nothing for them, and a clearance call between two walks
    nothing for those — on a handle on which both have held the large map's tables."""
    import tests.test_gpu_clearance as tgc
    import tests.test_gpu_walk as tgw
    a, big, fl = _lattice_large()
    large = tgc.check(a, fl, clr.BLOCKED, 64, what="large")
    with tgw.step_table(True):
        info = _np(a.walk_paths(_dev(_lattice_paths(big, LARGE, 11, 3.0)), hops=large["hops"].view(np.int32), rows=4))
    assert {wr.DONE, wr.BLOCKED} <= set(info["status"].tolist())
    b, cells = _lattice_small(a)
    fs = clr.Field(cells)
    w = wr.Walker(cells, fr.ORIGIN, fr.GL, fr.ZL, field=fs)
    assert fs.angle_margin_deg > 1e-3
    paths = _lattice_paths(cells, SMALL, 12, 1.5)

    def walk(table, hops, min_hops):
        want_info, want_rows, _ = w.walk(paths, hops=hops, min_hops=min_hops, row_cap=6)
        with tgw.step_table(table):
            rc, got_info, got_rows, untouched = tgw.raw(a, paths, hops=hops, min_hops=min_hops, row_cap=6)
        assert rc == 0 and untouched
        wr.same(got_info, got_rows, want_info, want_rows, ("share nothing", table))
        assert {wr.DONE, wr.TOO_CLOSE} <= set(want_info["status"].tolist())

    first = tgc.check(a, fs, clr.BLOCKED, 64, what="first")
    walk(True, first["hops"], 2)
    second = tgc.check(a, fs, clr.BLOCKED | clr.OPEN, 5, what="second")
    rc, other = tgc.raw(b, clr.BLOCKED | clr.OPEN, 5)
    assert rc == 0
    _same_bytes(_field(second), _field(other), "the second field")
    assert (second["hops"] == clr.BEYOND).any() and second["counts"][0] > first["counts"][0]
    walk(False, second["hops"], 1)
    _same_bytes(_field(tgc.check(a, fs, clr.BLOCKED, 64, what="again")), _field(first), "the first field again")


# ---- surface patches ---------------------------------------------------------------------------------------------------------------
# gndt_api_patch.hip carves moments | parent | size_at | tile_cnt | slack out of h->patch by n, tiles and patch_cap: after 134 400 rows
# and a list of 2 100 patches every region of the small call (280 rows, 70 patches) lies on the large call's moments.

def test_patches():
    from tests import edge_shapes as es
    from tests import patch_ref as pt
    from tests.test_gpu_patches import check
    H, lines = es.TRIP_STRIPES
    a = _handle(LAT, fr.ORIGIN)
    a.create2DMap("slope", _dev(es.cells_points(*es.stripes_cells(H, lines))[1:]))
    a.sync()
    R = pt.rule()
    big = a.export()
    assert big["num_nodes"] == H * lines > es.PATCH_TRIP
    ref = pt.patches_fast(big, R)
    for host in (False, True):
        large, _ = check(a, None, R, ref=ref, cap=lines, host=host, planes="all", what=("large", host))
    assert int(large["counts"][0]) == lines
    h, k = 4, es.STRIPES[4]
    b, cells = _shrink_to(a, es.cells_points(*es.stripes_cells(h, k))[1:], QUADRANT, LAT, fr.ORIGIN)
    assert cells["num_nodes"] == h * k < big["num_nodes"] // 8
    ref = pt.patches_fast(cells, R)
    for host in (False, True):
        for kw in (dict(), dict(cap=es.EDGES["kPatchSlots"] + 1), dict(min_size=h + 1)):
            got, r = check(a, None, R, ref=ref, host=host, planes="all", what=("small", host, kw), **kw)
            other, _ = check(b, None, R, ref=ref, host=host, planes="all", what=("small, fresh handle", host, kw), **kw)
            assert got["label"].tobytes() == other["label"].tobytes() and got["counts"].tobytes() == other["counts"].tobytes()
            for f in pt.INTEGER_FIELDS + ("kind", "reserved"):
                assert got["patches"][f].tobytes() == other["patches"][f].tobytes(), (host, kw, f)
            if not kw:
                assert 0 < int(got["counts"][0]) == k < int(large["counts"][0]) and r["compared"] == k
