"""GPU tier: scan scoring on the device-resident grid (gndt_score_poses_device / gndt_score_poses, TwoDmap.score_poses) against the
numpy restatement of the definition (tests/score_ref.py) on the exported cells: every accumulate strategy, both neighbourhoods, a
batch of poses with the per-point outputs; the identity is the peak of the score and matches most of the scan; results are the same
bits from run to run, in a batch or one pose at a time, at either stride, on any stream; the score follows the map through updates,
removals, crops and clears; the entry points' error codes; and the map is left as it was.

Tolerances (derived, not tuned): rows, matched and terms exact; d2, score and d2_sum to rtol
1e-9 (fp64 arithmetic on bit-identical inputs, condition number of A at most 301); the per-point d2 is fp32: the reference rounded to
fp32, within 1 ulp of fp32."""
import ctypes as C
import math

import numpy as np
import pytest

from grid_ndt_amd import scenes
from tests import query_ref as qr
from tests import score_ref as sr
from tests.gpu_kit import dev, handle, to_np

pytestmark = pytest.mark.gpu

ATOMIC, PARTITION, TILE, AUTO = 1, 2, 5, 0
ERR_INVALID = 1
TERRAIN = scenes.TERRAIN_PARAMS
FACE = dict(grid_len=0.5, z_len=0.25, slope_interval=0.08, demand="slope")
BOX = dict(grid_len=0.5, z_len=0.5, slope_interval=0.08, demand="slope")


def _scene(name):
    return {"bridge_ground": lambda: (scenes.bridge_ground(), scenes.BRIDGE_PARAMS),
            "uniform_box": lambda: (scenes.uniform_box(40_001, half_xy=6.0, half_z=1.0), BOX),
            "terrain": lambda: (scenes.terrain_cloud(300_000), TERRAIN),
            "campus": lambda: (scenes.campus_frame(60_000), scenes.CAMPUS_PARAMS),
            "face_lattice": lambda: (qr.face_lattice(grid_len=FACE["grid_len"], z_len=FACE["z_len"]), FACE)}[name]()


def _built(name, strategy=AUTO):
    cloud, P = _scene(name)
    m = handle(P, strategy)
    m.setCloudFirst(cloud[0])
    m.create2DMap("slope", dev(cloud[1:]))
    return cloud, P, m


def yaw(deg, t=(0.0, 0.0, 0.0)):
    a = math.radians(deg)
    return np.array([[math.cos(a), -math.sin(a), 0, t[0]], [math.sin(a), math.cos(a), 0, t[1]], [0, 0, 1, t[2]]], np.float64)


def six_poses(P):
    """identity; +0.3 cell in x; +0.3 level in z; yaw 2 degrees; a translation that leaves the map entirely; a pose with a NaN"""
    bad = yaw(0)
    bad[2, 0] = np.nan
    return np.stack([yaw(0), yaw(0, (0.3 * P["grid_len"], 0, 0)), yaw(0, (0, 0, 0.3 * P["z_len"])), yaw(2.0), yaw(0, (5000.0, 0, 0)), bad])


def _ref(m, cloud, P, scan, poses, nbh, per_point=None, **kw):
    return sr.score(m.export(), cloud[0], P["grid_len"], P["z_len"], scan, poses, nbh, per_point, **kw)


def _bits(out):
    """the four sums of a result as integers"""
    o = to_np(out)
    return (o["score"].astype(np.float64).view(np.uint64).tolist(), o["d2_sum"].astype(np.float64).view(np.uint64).tolist(),
            o["matched"].tolist(), o["terms"].tolist())


# ---- 1. against the restatement ----

@pytest.mark.parametrize("strategy", [ATOMIC, PARTITION, TILE, AUTO])
@pytest.mark.parametrize("name", ["bridge_ground", "uniform_box", "terrain", "face_lattice"])
def test_scores_equal_the_restatement(name, strategy):
    cloud, P, m = _built(name, strategy)
    scan = np.ascontiguousarray(cloud[1:][::5])
    t = dev(scan)
    poses = six_poses(P)
    for nbh in (1, 7):
        want = _ref(m, cloud, P, scan, poses, nbh)
        assert want["terms"][0] > 100 and (want["terms"][:4] > 0).all()
        for k in (0, 3):
            got = to_np(m.score_poses(t, poses, neighbourhood=nbh, per_point=k))
            sr.assert_pose_sums(got, want, what=(name, strategy, nbh))
            sr.assert_per_point(got["d2"], got["row"], want["poses_out"][k], what=(name, strategy, nbh, k))
            # off the map, and the pose with a NaN: all four sums exactly 0
            for j in (4, 5):
                assert got["score"][j] == 0.0 and got["d2_sum"][j] == 0.0 and got["matched"][j] == 0 and got["terms"][j] == 0
        if nbh == 7:
            assert want["terms"][0] > want["matched"][0]           # (neighbours did contribute)


# ---- 2. and 3. the identity is the peak, and it is not an empty match ----

@pytest.mark.parametrize("name", ["bridge_ground", "uniform_box", "terrain", "campus"])
def test_identity_is_the_peak_and_matches_the_scan(name):
    cloud, P, m = _built(name)
    scan = np.ascontiguousarray(cloud[1:][::7][:20000])
    g, z = P["grid_len"], P["z_len"]
    poses = [yaw(0)] + [yaw(0, (f * g, 0, 0)) for f in (0.1, 0.3, 0.5, 1.0)] + [yaw(0, (0, 0, f * z)) for f in (0.1, 0.3, 0.5, 1.0)] + [yaw(2.0)]
    got = to_np(m.score_poses(dev(scan), np.stack(poses)))
    print(name, "score", got["score"].tolist(), "matched / n", got["matched"][0] / len(scan))
    assert (got["score"][0] > got["score"][1:]).all(), got["score"]
    if name != "campus":                                          # (campus: mostly single-point nodes, 0.11 by the definition)
        assert got["matched"][0] / len(scan) >= 0.80, got["matched"][0] / len(scan)
    sr.assert_pose_sums(got, _ref(m, cloud, P, scan, np.stack(poses), 1))


# ---- 4. bits ----

def test_results_are_the_same_bits_every_way():
    import torch
    cloud, P, m = _built("terrain")
    scan = np.ascontiguousarray(cloud[1:][::3])
    t3, t4 = dev(scan[:, :3]), dev(scenes.with_stride4(scan[:, :3]))
    poses = six_poses(P)
    for nbh in (1, 7):
        first = m.score_poses(t3, poses, neighbourhood=nbh, per_point=3)
        b0, d0, r0 = _bits(first), to_np(first)["d2"].view(np.uint32), to_np(first)["row"]
        assert b0[3][0] > 1000
        for _ in range(4):                                         # five calls in all
            again = m.score_poses(t3, poses, neighbourhood=nbh, per_point=3)
            assert _bits(again) == b0
            assert np.array_equal(to_np(again)["d2"].view(np.uint32), d0) and np.array_equal(to_np(again)["row"], r0)
        # a batch of 6 = six single-pose calls
        for k in range(6):
            one = _bits(m.score_poses(t3, poses[k], neighbourhood=nbh))
            assert [v[0] for v in one] == [v[k] for v in b0], (nbh, k)
        # stride 12 = stride 16
        assert _bits(m.score_poses(t4, poses, neighbourhood=nbh)) == b0
        # another stream = the handle's
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        other = m.score_poses(t3, poses, neighbourhood=nbh, stream=s)
        s.synchronize()
        assert _bits(other) == b0
        # pose T on cloud P = the identity on fl32(T P)
        moved = sr.transform(poses[3], scan)
        assert [v[0] for v in _bits(m.score_poses(dev(moved), yaw(0), neighbourhood=nbh))] == [v[3] for v in b0]


def test_a_batch_launched_in_groups_of_poses_has_the_single_calls_bits():
    """3 M points are 11 719 tiles, 281 KB of partial sums a pose: 240 poses exceed what one launch's scratch takes (64 MiB, 238
    poses), so the batch goes in two groups — pose k's record and the per-point outputs of a pose of the second group are what a
    single-pose call gives"""
    cloud = scenes.uniform_box(3_000_001)
    m = handle(BOX, max_nodes_hint=1 << 20)
    m.setCloudFirst(cloud[0])
    t = dev(cloud[1:])
    m.create2DMap("slope", t)
    rng = np.random.default_rng(9)
    poses = np.stack([yaw(float(a), (float(x), float(y), 0.0)) for a, x, y in zip(rng.uniform(-1, 1, 240), rng.uniform(-.2, .2, 240), rng.uniform(-.2, .2, 240))])
    batch = m.score_poses(t, poses, per_point=239)
    bb = _bits(batch)
    assert min(bb[3]) > 1_000_000
    for k in (0, 1, 237, 238, 239):
        one = m.score_poses(t, poses[k], per_point=0)
        assert [v[0] for v in _bits(one)] == [v[k] for v in bb], k
    assert np.array_equal(to_np(one)["d2"].view(np.uint32), to_np(batch)["d2"].view(np.uint32)) and np.array_equal(to_np(one)["row"], to_np(batch)["row"])


# ---- 5. the score follows the map ----

def test_score_follows_the_map():
    import grid_ndt_amd as g
    cloud, P = scenes.campus_frame(200_000), scenes.CAMPUS_PARAMS
    body = cloud[1:]
    half = len(body) // 2
    scan = np.ascontiguousarray(body[::7])
    t = dev(scan)
    poses = six_poses(P)[:4]
    m = handle(P, ATOMIC)
    m.setCloudFirst(cloud[0])
    m.change2DMap("slope", dev(body[:half]))

    def check(step):
        for nbh in (1, 7):
            got = to_np(m.score_poses(t, poses, neighbourhood=nbh, per_point=0))
            want = _ref(m, cloud, P, scan, poses, nbh, per_point=0)
            sr.assert_pose_sums(got, want, what=(step, nbh))
            sr.assert_per_point(got["d2"], got["row"], want, what=(step, nbh))
        return int(got["terms"][0])

    terms = [check("built")]
    m.change2DMap("slope", dev(body[half:]))
    terms.append(check("update"))
    m.del2DMap("slope", dev(body[:half // 2]))
    terms.append(check("remove"))
    cells = m.export()
    mid = cells["mean"][cells["num_nodes"] // 2]
    box = g.crop_box_from_world(cloud[0], P["grid_len"], (mid[0] - 30.0, mid[1] - 30.0), (mid[0] + 30.0, mid[1] + 30.0))
    m.crop_box(box, "keep_inside")
    terms.append(check("crop"))
    ends = np.ascontiguousarray(cells["mean"][:: max(1, cells["num_nodes"] // 4000)], np.float32)
    st = m.clear_rays((float(mid[0]), float(mid[1]), float(mid[2]) + 2.0), dev(ends))
    assert st["cleared"] > 0
    terms.append(check("clear"))
    m.set_deferred_emit(True)
    m.change2DMap("slope", dev(body[:half // 2]))
    terms.append(check("deferred"))
    assert terms[1] > terms[0] > 0 and terms[3] < terms[2] and terms[5] > terms[4] > 0, terms


def test_score_and_flood_do_not_depend_on_who_built_the_index():
    cloud, P = scenes.bridge_ground(), scenes.BRIDGE_PARAMS
    scan = np.ascontiguousarray(cloud[1::7])
    poses = six_poses(P)[:4]
    goal = (9.5, 3.0, 1.0)
    res = []
    for score_first in (True, False):
        m = handle(P)
        m.setCloudFirst(cloud[0])
        m.create2DMap("slope", dev(cloud[1:]))
        t = dev(scan)
        before = _bits(m.score_poses(t, poses, neighbourhood=7)) if score_first else None
        st = m.computeCost(goal, robot={"radius": 0.25})
        c = m.cost_export()
        after = _bits(m.score_poses(t, poses, neighbourhood=7))
        if score_first:
            assert before == after                                 # the same bits before and after computeCost
        res.append((after, st, c["h"].view(np.uint32), c["state"]))
    assert res[0][0] == res[1][0] and res[0][1] == res[1][1]
    assert np.array_equal(res[0][2], res[1][2]) and np.array_equal(res[0][3], res[1][3])
    assert res[0][1]["traversable"] > 0 and res[0][0][3][0] > 1000


# ---- 6. the host entry point, empty inputs, the error codes, capture ----

def _raw(m, pts, poses, K, prm, out=True, d2=False, row=False, host=False, stride=12, n=None, stream=None):
    """the C entry point itself -> rc"""
    import torch
    from grid_ndt_amd._lib import ScoreParams
    n = len(pts) if n is None and pts is not None else (n or 0)
    p = ScoreParams(*prm) if prm is not None else None
    if host:
        rec = np.zeros((max(K, 1), 4), np.int64)
        a, b = np.zeros(max(n, 1), np.float32), np.zeros(max(n, 1), np.uint32)
        ptr = lambda x: C.c_void_p(x.ctypes.data)
        return m._L.gndt_score_poses(m._h, ptr(pts) if pts is not None else None, n, stride, ptr(poses) if poses is not None else None, K,
                                     C.byref(p) if prm is not None else None, ptr(rec) if out else None, ptr(a) if d2 else None,
                                     ptr(b) if row else None)
    rec = torch.zeros((max(K, 1), 4), dtype=torch.int64, device="cuda")
    a = torch.zeros(max(n, 1), dtype=torch.float32, device="cuda")
    b = torch.zeros(max(n, 1), dtype=torch.int32, device="cuda")
    tp = dev(pts) if pts is not None else None
    tq = torch.from_numpy(poses).cuda() if poses is not None else None
    ptr = lambda x: C.c_void_p(x.data_ptr())
    rc = m._L.gndt_score_poses_device(m._h, ptr(tp) if tp is not None else None, n, stride, ptr(tq) if tq is not None else None, K,
                                      C.byref(p) if prm is not None else None, ptr(rec) if out else None, ptr(a) if d2 else None,
                                      ptr(b) if row else None, stream)
    torch.cuda.synchronize()
    return rc


def test_host_entry_point_empty_inputs_and_errors():
    import torch
    import grid_ndt_amd as g
    cloud, P, m = _built("terrain", ATOMIC)
    scan = np.ascontiguousarray(cloud[1:][::4])
    poses = six_poses(P)
    for nbh in (1, 7):
        on_dev = m.score_poses(dev(scan), poses, neighbourhood=nbh, per_point=3, max_d2=9.0)
        host = m.score_poses(scan, poses, neighbourhood=nbh, per_point=3, max_d2=9.0)
        assert _bits(on_dev) == _bits(host) and _bits(host)[3][0] > 1000
        assert np.array_equal(to_np(on_dev)["d2"].view(np.uint32), host["d2"].view(np.uint32)) and np.array_equal(to_np(on_dev)["row"], host["row"])
    # n == 0 with K > 0: K zeroed records; K == 0: nothing
    for pts in (dev(np.zeros((0, 3), np.float32)), np.zeros((0, 3), np.float32)):
        out = to_np(m.score_poses(pts, poses))
        assert len(out["score"]) == 6 and not out["score"].any() and not out["d2_sum"].any() and not out["matched"].any() and not out["terms"].any()
        out = to_np(m.score_poses(pts, poses, per_point=1))
        assert out["d2"].shape == (0,) and out["row"].shape == (0,)
    T = np.ascontiguousarray(poses.reshape(6, 12))
    ok = (1, 0, 0.0, 0.0, 0.0, 0)
    for host in (False, True):
        assert _raw(m, scan, T, 0, ok, host=host) == 0
        assert _raw(m, scan, None, 0, ok, out=False, host=host) == 0
        assert _raw(m, scan, T, 6, ok, host=host) == 0
        assert _raw(m, scan, T, 6, ok, d2=True, row=True, host=host) == 0
        # the refusals
        assert _raw(m, None, T, 6, ok, n=5, host=host) == ERR_INVALID                     # null points with n > 0
        assert _raw(m, scan, None, 6, ok, host=host) == ERR_INVALID                       # null poses
        assert _raw(m, scan, T, 6, ok, out=False, host=host) == ERR_INVALID               # null out
        assert _raw(m, scan, T, 6, None, host=host) == ERR_INVALID                        # null params
        assert _raw(m, scan, T, 6, ok, stride=8, host=host) == ERR_INVALID
        assert _raw(m, scan, T, 6, ok, stride=20, host=host) == ERR_INVALID
        for nbh in (0, 2, 6, 27, -1):
            assert _raw(m, scan, T, 6, (nbh, 0, 0.0, 0.0, 0.0, 0), host=host) == ERR_INVALID
        assert _raw(m, scan, T, 6, (1, 0, 0.0, 0.0, 0.0, 6), d2=True, host=host) == ERR_INVALID      # point_pose >= K
        assert _raw(m, scan, T, 6, (1, 0, 0.0, 0.0, 0.0, 6), row=True, host=host) == ERR_INVALID
        assert _raw(m, scan, T, 6, (1, 0, 0.0, 0.0, 0.0, 6), host=host) == 0                         # (not asked for: not looked at)
        for mc in (1, 2, -3):
            assert _raw(m, scan, T, 6, (1, mc, 0.0, 0.0, 0.0, 0), host=host) == ERR_INVALID
        assert _raw(m, scan, T, 6, (1, 3, 0.0, 0.0, 0.0, 0), host=host) == 0
        for bad in (-1.0, float("nan"), float("inf")):
            for slot in (2, 3, 4):
                prm = [1, 0, 0.0, 0.0, 0.0, 0]
                prm[slot] = bad
                assert _raw(m, scan, T, 6, tuple(prm), host=host) == ERR_INVALID, (bad, slot)
    big = np.ascontiguousarray(np.tile(T[:1], (65536, 1)))
    assert _raw(m, scan[:64], big, 65536, ok) == ERR_INVALID                              # K above the grid's y limit
    assert _raw(m, scan[:64], big, 65535, ok) == 0
    assert m._L.gndt_score_poses_device(None, None, 0, 12, None, 0, None, None, None, None, None) == ERR_INVALID
    assert m._L.gndt_score_poses(None, None, 0, 12, None, 0, None, None, None, None) == ERR_INVALID
    # min_count below the handle's min_points
    cloud5, P5 = _scene("uniform_box")
    m5 = handle(P5, ATOMIC, min_points=5)
    m5.setCloudFirst(cloud5[0])
    m5.create2DMap("slope", dev(cloud5[1:]))
    s5 = np.ascontiguousarray(cloud5[1::3])
    assert _raw(m5, s5, T, 6, (1, 4, 0.0, 0.0, 0.0, 0)) == ERR_INVALID
    assert _raw(m5, s5, T, 6, (1, 5, 0.0, 0.0, 0.0, 0)) == 0
    got = to_np(m5.score_poses(dev(s5), poses, neighbourhood=7))
    sr.assert_pose_sums(got, sr.score(m5.export(), cloud5[0], P5["grid_len"], P5["z_len"], s5, poses, 7, min_points=5))
    # no finished build
    e = handle(TERRAIN)
    e.setCloudFirst((0.0, 0.0, 0.0))
    with pytest.raises(g.GndtError) as err:
        e.score_poses(dev(scan), poses)
    assert err.value.code == ERR_INVALID
    # a capturing stream: refused, and the capture goes on
    from grid_ndt_amd._lib import ScoreParams
    want = _bits(m.score_poses(dev(scan), poses))
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    x = torch.zeros(16, device="cuda")
    tp, tq = dev(scan), torch.from_numpy(T).cuda()
    rec = torch.zeros((6, 4), dtype=torch.int64, device="cuda")
    prm = ScoreParams(*ok)
    torch.cuda.synchronize()
    with g.graph_capture(graph, stream=s):
        rc = m._L.gndt_score_poses_device(m._h, C.c_void_p(tp.data_ptr()), len(scan), 12, C.c_void_p(tq.data_ptr()), 6, C.byref(prm),
                                          C.c_void_p(rec.data_ptr()), None, None, C.c_void_p(s.cuda_stream))
        x.add_(1.0)
    assert rc == ERR_INVALID
    graph.replay()
    torch.cuda.synchronize()
    assert float(x[0]) == 1.0
    assert _bits(m.score_poses(dev(scan), poses)) == want


# ---- 7. the map is untouched ----

@pytest.mark.parametrize("strategy", [ATOMIC, PARTITION])
def test_the_map_is_untouched(strategy):
    cloud, P, m = _built("terrain", strategy)
    before = m.export()
    counts = m.sync()
    scan = np.ascontiguousarray(cloud[1:][::3])
    for nbh in (1, 7):
        m.score_poses(dev(scan), six_poses(P), neighbourhood=nbh, per_point=2)
        m.score_poses(scan, six_poses(P), neighbourhood=nbh, per_point=2)
    after = m.export()
    assert m.sync() == counts
    assert before.keys() == after.keys()
    for k in before:
        a, b = np.asarray(before[k]), np.asarray(after[k])
        assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b), k
