"""GPU tier: view gain (gndt_view_gain_device / gndt_view_gain, TwoDmap.view_gain / frontier_views, rollouts.view_directions).  Records
equal, field for field, the restatement with sets (tests/view_ref.py) on maps of three build paths, through both entry points, at both
strides, for batches of 1, 3 and 65 poses and fans around a wave, a workgroup and beyond; the hand-derived case of
tests/test_view_host.py; windows of one word, at the 64 KiB edge of ungranted LDS and at the largest reach, one beyond refused; the
record as a set (permuted and repeated fans, repeated poses); a workgroup's LDS after a call that filled it, and more poses than
workgroups; the per-ray outputs against cast_rays; repeat calls, streams, the untouched map, the empty batch, every invalid argument,
capture; frontier_views on the drivable site, and a map with one open and one walled side.

The restatement walks every ray of a scene once (65 poses x 1000 directions); every smaller batch or other fan is made from that
trace (view_ref.gain)."""
import ctypes as C

import numpy as np
import pytest

from grid_ndt_amd import rollouts, scenes
from grid_ndt_amd.map2d import _stream_ptr
from tests import cast_ref as cf
from tests import view_ref as vr
from tests.test_view_host import HAND_DIRS, HAND_OPEN, HAND_POSE, HAND_WALL, UNIT, hand_cloud, pose, rec
from tests.gpu_kit import build, dev

pytestmark = pytest.mark.gpu

ATOMIC, PARTITION, TILE = 1, 2, 5
FIELDS = ("sx", "sy", "sz", "count", "first_idx", "mean", "cov", "rough", "normal", "flags")
# reach = ceil(max_range / grid_len) + 1; the launch's LDS is 8 * ceil((2 reach + 1)^2 / 32) + 1024 bytes: 65 288 at reach 253 (the
# last that fits the 65 536 a launch gets without a grant), 65 800 at 254, 163 840 at 403 (all of a CU's LDS), 164 648 at 404
REACH_DEFAULT, REACH_MAX = 253, 403


def host(out):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in out.items()}


def records(out):
    """a view_gain dict (torch or numpy) -> a structured array of view_ref.INFO_DTYPE"""
    out = host(out)
    r = np.zeros(len(out["rays"]), vr.INFO_DTYPE)
    for k in vr.FIELDS:
        r[k] = out[k].astype(r[k].dtype)
    return r


def fan(n, seed):
    """n directions: towards the ground and the horizon, every fourth skyward, a few NaN"""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d[:, 2] = -np.abs(d[:, 2]) * 0.3 - 0.05
    d[::4, 2] = np.abs(d[::4, 2]) + 0.5
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = d.astype(np.float32)
    d[7::97] = np.nan
    return d


_scenes = {}
K_MAX, N_MAX = 65, 1000


def scene(name):
    """tests/test_gpu_cast.py's three recipes, built again: the 300 k-point terrain under ATOMIC and PARTITION, the depth frame under TILE
    -> dict(m, P, origin, cells, poses [65, 12], dirs [1000, 3], R, trace).  Pose 1 stands wholly outside the map, pose 2 has a NaN
    translation, the others stand 1.5 m over points of the cloud (so also at the map's edges) with yaws and small tilts of their own."""
    if name not in _scenes:
        if name in ("atomic", "partition"):
            cloud, P, strategy, R = scenes.terrain_cloud(300_000), scenes.TERRAIN_PARAMS, {"atomic": ATOMIC, "partition": PARTITION}[name], 4.0
            pts = cloud[150_000::10]
        else:
            cloud, P, strategy, R = scenes.depth_frame(), scenes.DEPTH_PARAMS, TILE, 9.0
            pts = cloud[1::8]
        m = build(cloud, P, strategy)
        if name == "tile":
            assert m.STRATEGY_NAMES[m.last_strategy()] == "tile"
        rng = np.random.default_rng(41)
        at = pts[rng.choice(len(pts), K_MAX, replace=False), :3].astype(np.float64) + np.array([0, 0, 1.5])
        poses = []
        for k in range(K_MAX):
            T = pose(at[k], rng.uniform(0, 2 * np.pi)).reshape(3, 4)
            a = rng.uniform(-0.3, 0.3)
            ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
            T[:, :3] = T[:, :3] @ ry
            poses.append(T.reshape(12))
        poses = np.stack(poses)
        poses[1, [3, 7]] = pts[:, :2].max(0) + 100.0
        poses[2, 3] = np.nan
        dirs = fan(N_MAX, 43)
        cells = m.export()
        tr = vr.trace(cells, cloud[0], P["grid_len"], P["z_len"], poses, dirs, R)
        _scenes[name] = dict(m=m, P=P, origin=cloud[0], cells=cells, poses=poses, dirs=dirs, R=R, trace=tr)
    return _scenes[name]


def hand_map(wall):
    key = ("hand", wall)
    if key not in _scenes:
        cloud = hand_cloud(wall)
        m = build(cloud, UNIT, ATOMIC)
        _scenes[key] = dict(m=m, cells=m.export(), origin=cloud[0])
    return _scenes[key]


def hand_ref(s, poses, dirs, R, **kw):
    return vr.trace(s["cells"], s["origin"], 1.0, 1.0, poses, dirs, R, **kw)


def pad4(a):
    return np.concatenate([a, np.full((len(a), 1), 7.0, np.float32)], 1)


@pytest.mark.parametrize("wall", [False, True])
def test_the_hand_case_through_both_entry_points(wall):
    """tests/test_view_host.py derives the two records by hand"""
    s = hand_map(wall)
    want = HAND_WALL if wall else HAND_OPEN
    on_dev = s["m"].view_gain(HAND_POSE, HAND_DIRS, 10.0, per_ray=True)
    hst = s["m"].view_gain(HAND_POSE, HAND_DIRS, 10.0, per_ray=True, host=True)
    for out in (host(on_dev), hst):
        assert rec(records(out)[0]) == want
        assert out["range"].shape == (1, 4) and (out["range"][0, 0] == 1.5 if wall else np.isinf(out["range"][0, 0]))
        assert (out["row"][0, 1:] == -1).all() and np.isinf(out["range"][0, 1:]).all()
    assert rec(vr.gain(hand_ref(s, HAND_POSE, HAND_DIRS, 10.0))[0]) == want


@pytest.mark.parametrize("name", ["atomic", "partition", "tile"])
def test_both_entry_points_equal_the_restatement(name):
    s = scene(name)
    m, tr, poses, dirs, R = s["m"], s["trace"], s["poses"], s["dirs"], s["R"]
    st = tr["status"]
    assert (st == cf.HIT).sum() > 1000 and (st == cf.MISS).sum() > 1000 and (st[0] == cf.SKIPPED).sum() >= 10     # the mix, per pose too
    full = vr.gain(tr)
    assert full["known"][1] == 0 and full["unknown"][1] > 20 and full["status"].tolist() == [0, 0, 1] + [0] * (K_MAX - 3)
    # (a pose 1.5 m over a point of the cloud can stand inside an occupied voxel: every ray then stops in the first column, known = 1)
    assert (full["known"][3:] >= 1).all() and np.median(full["known"][3:]) > 20 and (full["known"][3:] == 1).sum() < K_MAX // 2
    assert (full["unknown"][3:] > 0).sum() > K_MAX // 2 and (full["hits"][3:] > 0).all()
    d_pose = dev(poses, np.float64)
    for N in (1, 63, 64, 65, 255, 256, 257, 1000):
        want = vr.gain(tr, dirs=np.arange(N))
        for d in (dirs[:N], pad4(dirs[:N])):
            d_dirs = dev(d)
            for K in (1, 3, 65):
                vr.assert_same(records(m.view_gain(d_pose[:K], d_dirs, R)), want[:K], (name, "device", K, N, d.shape[1]))
            vr.assert_same(records(m.view_gain(poses[:3], d, R, host=True)), want[:3], (name, "host", N, d.shape[1]))
    vr.assert_same(records(m.view_gain(poses, dirs, R, host=True)), full, (name, "host", K_MAX, N_MAX))


def test_the_cast_parameters_equal_the_restatement():
    s = scene("atomic")
    poses, dirs = s["poses"][:5], s["dirs"][:257]
    base = vr.gain(s["trace"], poses=np.arange(5), dirs=np.arange(257))
    for kw in (dict(min_count=6), dict(min_range=1.5), dict(min_count=4, min_range=0.8)):
        want = vr.gain(vr.trace(s["cells"], s["origin"], s["P"]["grid_len"], s["P"]["z_len"], poses, dirs, s["R"], **kw))
        assert not np.array_equal(want["steps"], base["steps"]), kw                  # the parameter matters on these rays
        vr.assert_same(records(s["m"].view_gain(poses, dirs, s["R"], **kw)), want, kw)
        vr.assert_same(records(s["m"].view_gain(poses, dirs, s["R"], host=True, **kw)), want, (kw, "host"))


# the windows: one word (reach 2: 25 bits), a few words, either side of the ungranted 64 KiB, and the largest; the bitmap's size
# depends on max_range / grid_len alone, so the unit lattice with 16 rays a pose keeps the restatement small
EDGE_RANGES = [(0.8, 2), (1.0, 2), (2.0, 3), (10.0, 11), (REACH_DEFAULT - 1.0, REACH_DEFAULT), (REACH_DEFAULT + 0.0, REACH_DEFAULT + 1),
               (REACH_MAX - 1.5, REACH_MAX), (REACH_MAX - 1.0, REACH_MAX)]


@pytest.mark.parametrize("R,reach", EDGE_RANGES)
def test_window_edges(R, reach):
    s = hand_map(True)
    assert int(np.ceil(np.float32(R) / np.float32(1.0))) + 1 == reach
    a = np.arange(16) * (2 * np.pi / 16) + 0.05
    dirs = np.stack([np.cos(a), np.sin(a), np.zeros(16)], 1).astype(np.float32)
    dirs[:4] = HAND_DIRS                                                  # (rays along the axes reach the window's last column)
    poses = np.stack([HAND_POSE, pose((0.5, 8.5, 1.5), 0.7), pose((-3.2, 4.1, 1.5), 2.0)])
    want = vr.gain(hand_ref(s, poses, dirs, R))
    if R >= 10:
        # the axis rays end ceil(R) or ceil(R) + 1 cells from the origin's: within reach, and the first uses all of it but one
        assert want["unknown"][0] > 4 * (R - 6) and want["hits"][0] >= 1
    vr.assert_same(records(s["m"].view_gain(poses, dirs, R)), want, ("device", R))
    vr.assert_same(records(s["m"].view_gain(poses, dirs, R, host=True)), want, ("host", R))


def test_one_past_the_largest_window_is_refused():
    import grid_ndt_amd as g
    s = hand_map(True)
    for host_path in (False, True):
        with pytest.raises(g.GndtError) as err:
            s["m"].view_gain(HAND_POSE, HAND_DIRS, REACH_MAX + 0.0, host=host_path)
        assert err.value.code == 1 and f"is {REACH_MAX} " in str(err.value) and "gndt_coarsen_device" in str(err.value)
    vr.assert_same(records(s["m"].view_gain(HAND_POSE, HAND_DIRS, 10.0)), vr.gain(hand_ref(s, HAND_POSE, HAND_DIRS, 10.0)), "after the refusal")


def test_the_record_is_a_set_and_does_not_depend_on_the_block_size():
    import grid_ndt_amd as g
    s = scene("atomic")
    m, tr, R = s["m"], s["trace"], s["R"]
    K, N = 5, 257
    poses, dirs = s["poses"][:K], s["dirs"][:N]
    base = vr.gain(tr, poses=np.arange(K), dirs=np.arange(N))
    perm = np.random.default_rng(5).permutation(N)
    vr.assert_same(records(m.view_gain(poses, dirs[perm], R)), base, "permuted")
    three = records(m.view_gain(poses, np.concatenate([dirs, dirs, dirs]), R))
    vr.assert_same(three, vr.gain(tr, poses=np.arange(K), dirs=np.tile(np.arange(N), 3)), "three times")
    for k in vr.FIELDS:
        f = 3 if k in ("rays", "skipped", "hits", "steps") else 1
        assert np.array_equal(three[k].astype(np.int64), f * base[k].astype(np.int64)), k
    pick = np.array([4, 0, 4, 3, 0, 4])
    vr.assert_same(records(m.view_gain(poses[pick], dirs, R)), base[pick], "repeated poses")
    T = g.TwoDmap
    try:
        for threads in (64, 128, 256, 512):
            T.set_debug_option(T.DEBUG_VIEW_THREADS, threads)
            vr.assert_same(records(m.view_gain(s["poses"][:9], s["dirs"], R)), vr.gain(tr, poses=np.arange(9)), threads)
        for bad in (0, 32, 96, 2048, 256.5):
            with pytest.raises(g.GndtError):
                T.set_debug_option(T.DEBUG_VIEW_THREADS, bad)
    finally:
        T.set_debug_option(T.DEBUG_VIEW_THREADS, 1024)


def test_lds_left_by_a_full_window_and_more_poses_than_workgroups():
    """At the largest window a launch has one workgroup per CU, at most 256 of them.  First 256 poses whose dense fans mark most of
    their windows; then, on the same stream, 256 poses inside the occupied voxel, whose rays all stop in the first column: a bitmap
    that kept a bit of the first call would count that column as seen before and report known = 0.  Then 300 poses in one launch:
    workgroups that take a second pose clear between the two."""
    s = hand_map(True)
    m, R = s["m"], REACH_MAX - 1.0
    W = 2 * REACH_MAX + 1
    a = np.arange(2048) * (2 * np.pi / 2048)
    dense = np.stack([np.cos(a), np.sin(a), np.zeros(2048)], 1).astype(np.float32)
    far = pose((4.5, 40.5, 2.5))                                         # (off the floor and a level above the wall's node: nothing stops a ray)
    filled = host(m.view_gain(np.tile(far, (256, 1)), dense, R))
    assert ((filled["unknown"] + filled["known"]) > 0.5 * np.pi / 4 * W * W).all() and (filled["hits"] == 0).all()
    inside = pose((6.5, 4.5, 1.5))
    want = vr.gain(hand_ref(s, inside, HAND_DIRS, R))
    assert rec(want[0]) == dict(rays=4, skipped=0, hits=4, unknown=0, known=1, status=0, steps=4, sum_ux=0, sum_uy=0)
    got = records(m.view_gain(np.tile(inside, (256, 1)), HAND_DIRS, R))
    vr.assert_same(got, np.repeat(want, 256), "after the full windows")
    kinds = np.stack([HAND_POSE, inside, far, pose((0.5, 0.5, 1.5), 1.0), pose((np.nan, 0, 0))])
    pick = np.random.default_rng(9).integers(0, len(kinds), 300)
    want = vr.gain(hand_ref(s, kinds, dense[::256], R))
    assert len({tuple(rec(w).values()) for w in want}) == len(kinds)
    vr.assert_same(records(m.view_gain(kinds[pick], dense[::256], R)), want[pick], "300 poses")


def _raw(m, poses, K, dirs, n, stride, prm, info, row, rng, device=True):
    p = lambda t: C.c_void_p(0 if t is None else (t.data_ptr() if hasattr(t, "data_ptr") else t.ctypes.data))
    args = [m._h, p(poses), K, p(dirs), n, stride, C.byref(prm) if prm is not None else None, p(info), p(row), p(rng)]
    return m._L.gndt_view_gain_device(*args, _stream_ptr(None)) if device else m._L.gndt_view_gain(*args)


def test_per_ray_outputs_are_the_casts_bit_for_bit():
    import torch
    from grid_ndt_amd._lib import ViewParams
    s = scene("partition")
    m, R = s["m"], s["R"]
    K, N = 5, 257
    poses, dirs = s["poses"][:K], s["dirs"][:N]
    o32, e32 = vr.ends(poses, dirs, R)                                    # the header's fp64 expression, in numpy
    cast = host(m.cast_rays(dev(np.repeat(o32, N, axis=0)), dev(e32.reshape(K * N, 3)), mode="voxel", max_range=R))
    assert (cast["row"] >= 0).sum() > 100 and np.isinf(cast["range"]).sum() > 100 and np.isnan(cast["range"]).sum() > 5 * 2
    want = vr.gain(s["trace"], poses=np.arange(K), dirs=np.arange(N))
    for out in (host(m.view_gain(poses, dirs, R, per_ray=True)), m.view_gain(poses, dirs, R, per_ray=True, host=True)):
        assert np.array_equal(out["row"].reshape(-1), cast["row"])
        assert np.array_equal(out["range"].reshape(-1).view(np.uint32), cast["range"].view(np.uint32))
        vr.assert_same(records(out), want)
    # every combination of NULL row / range: what is given is written, the records are the same
    prm = ViewParams(R, 0.0, 0)
    for device in (True, False):
        mk = (lambda a, dt: dev(a, dt)) if device else (lambda a, dt: np.ascontiguousarray(a, dt))
        dp, dd = mk(poses, np.float64), mk(dirs, np.float32)
        for want_row in (False, True):
            for want_rng in (False, True):
                info = mk(np.full((K, 12), -7, np.int32), np.int32)
                row = mk(np.full(K * N, -7, np.int32), np.int32) if want_row else None
                rng = mk(np.full(K * N, -7.0, np.float32), np.float32) if want_rng else None
                assert _raw(m, dp, K, dd, N, 12, prm, info, row, rng, device) == 0
                if device:
                    torch.cuda.synchronize()
                h = lambda t: t.cpu().numpy() if device else t
                vr.assert_same(h(info).reshape(-1).view(vr.INFO_DTYPE), want, (device, want_row, want_rng))
                if want_row:
                    assert np.array_equal(h(row), cast["row"])
                if want_rng:
                    assert np.array_equal(h(rng).view(np.uint32), cast["range"].view(np.uint32))


def test_the_map_is_untouched_and_the_bytes_repeat():
    import torch
    s = scene("atomic")
    m, R = s["m"], s["R"]
    p, d = dev(s["poses"][:9], np.float64), dev(s["dirs"][:257])
    a = host(m.view_gain(p, d, R, per_ray=True))
    b = host(m.view_gain(p, d, R, per_ray=True))
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    c = m.view_gain(p, d, R, per_ray=True, stream=st)
    e = m.view_gain(s["poses"][:9], s["dirs"][:257], R, per_ray=True, stream=st.cuda_stream)     # a raw hipStream_t, uploads on it
    st.synchronize()
    c, e = host(c), host(e)
    torch.cuda.current_stream().wait_stream(st)
    for other in (b, c, e):
        for k in a:
            assert a[k].tobytes() == other[k].tobytes(), k
    after = m.export()
    for k in ("num_nodes", "num_columns", "num_slopes"):
        assert after[k] == s["cells"][k]
    for k in FIELDS:
        x, y = np.ascontiguousarray(after[k]), np.ascontiguousarray(s["cells"][k])
        assert x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32)), k


def test_invalid_arguments_leave_the_outputs_untouched():
    import torch
    import grid_ndt_amd as g
    from grid_ndt_amd._lib import ViewParams
    s = scene("atomic")
    m, R = s["m"], s["R"]
    K, N = 3, 64
    ok = lambda **kw: ViewParams(**{**dict(max_range=R, min_range=0.0, min_count=0), **kw})
    nan, inf = float("nan"), float("inf")
    bad_params = [ok(max_range=v) for v in (0.0, -1.0, nan, inf)] + [ok(min_range=v) for v in (-1.0, nan, inf)] + [ok(min_count=-1)]
    bad_params += [ok(reserved=(C.c_uint32 * 5)(*[int(i == j) for i in range(5)])) for j in range(5)]
    bad_params += [ok(max_range=(REACH_MAX + 1) * s["P"]["grid_len"])]                  # a window beyond the LDS
    for device in (True, False):
        mk = (lambda a, dt=np.float32: dev(a, dt)) if device else (lambda a, dt=np.float32: np.ascontiguousarray(a, dt))
        p, d = mk(s["poses"][:K], np.float64), mk(s["dirs"][:N])
        outs = [mk(np.full((K, 12), -7, np.int32), np.int32), mk(np.full(K * N, -7, np.int32), np.int32), mk(np.full(K * N, -7.0))]
        assert _raw(m, p, K, d, N, 12, ok(), *outs, device=device) == 0              # the arguments the bad ones differ from are good
        for t in outs:
            t[:] = -7
        calls = [(p, K, d, N, 12, q, *outs) for q in bad_params]
        calls += [(p, K, d, N, 12, None, *outs), (None, K, d, N, 12, ok(), *outs), (p, K, None, N, 12, ok(), *outs),
                  (p, K, d, N, 12, ok(), None, outs[1], outs[2]), (p, 1 << 31, d, N, 12, ok(), *outs), (p, K, d, 1 << 31, 12, ok(), *outs),
                  (p, K, d, N, 0, ok(), *outs), (p, K, d, N, 8, ok(), *outs), (p, K, d, N, 20, ok(), *outs)]
        if device:
            off = lambda t, b: C.c_void_p(t.data_ptr() + b)
            raw = lambda *a: m._L.gndt_view_gain_device(m._h, *a, _stream_ptr(None))
            q, ptr = C.byref(ok()), lambda t: C.c_void_p(t.data_ptr())
            assert raw(off(p, 4), K, ptr(d), N, 12, q, ptr(outs[0]), None, None) == 1
            assert raw(ptr(p), K, ptr(d), N, 12, q, off(outs[0], 4), None, None) == 1
            assert raw(ptr(p), K, off(d, 2), N, 12, q, ptr(outs[0]), None, None) == 1
            assert raw(ptr(p), K, ptr(d), N, 12, q, ptr(outs[0]), off(outs[1], 2), None) == 1
        for c in calls:
            assert _raw(m, *c, device=device) == 1, c
        if device:
            torch.cuda.synchronize()
        for t in outs:
            assert bool((t == -7).all())
    assert m._L.gndt_view_gain_device(None, None, 0, None, 0, 12, None, None, None, None, None) == 1
    assert m._L.gndt_view_gain(None, None, 0, None, 0, 12, None, None, None, None) == 1
    # a handle without a finished build
    P = s["P"]
    h = g.TwoDmap(P["grid_len"], P["z_len"], strategy=ATOMIC)
    h.setInterval(P["slope_interval"])
    h.setCloudFirst(s["origin"])
    for host_path in (False, True):
        with pytest.raises(g.GndtError) as err:
            h.view_gain(s["poses"][:K], s["dirs"][:N], R, host=host_path)
        assert err.value.code == 1
    for bad in (np.zeros((4, 2), np.float32), np.zeros(3, np.float32)):
        with pytest.raises(ValueError):
            m.view_gain(s["poses"][:K], bad, R)


def test_capture_is_refused_and_the_empty_batches():
    import torch
    import grid_ndt_amd as g
    from grid_ndt_amd._lib import ViewParams
    s = scene("atomic")
    m, R = s["m"], s["R"]
    # K == 0 or N == 0: GNDT_OK, nothing written
    p, d = dev(s["poses"][:3], np.float64), dev(s["dirs"][:64])
    outs = [dev(np.full((3, 12), -7, np.int32), np.int32), dev(np.full(192, -7, np.int32), np.int32), dev(np.full(192, -7.0))]
    hp, hd = s["poses"][:3].copy(), s["dirs"][:64].copy()
    houts = [np.full((3, 12), -7, np.int32), np.full(192, -7, np.int32), np.full(192, -7.0, np.float32)]
    for K, N in ((0, 64), (3, 0), (0, 0)):
        assert _raw(m, p, K, d, N, 12, ViewParams(R, 0.0, 0), *outs) == 0
        assert _raw(m, None, K, None, N, 12, ViewParams(R, 0.0, 0), None, None, None) == 0
        assert _raw(m, hp, K, hd, N, 12, ViewParams(R, 0.0, 0), *houts, device=False) == 0
    torch.cuda.synchronize()
    assert all(bool((t == -7).all()) for t in outs) and all((t == -7).all() for t in houts)
    out = host(m.view_gain(np.zeros((0, 12)), s["dirs"][:64], R, per_ray=True))
    assert all(len(out[k]) == 0 for k in vr.FIELDS) and out["row"].shape == (0, 64)
    out = m.view_gain(s["poses"][:3], np.zeros((0, 3), np.float32), R, per_ray=True, host=True)
    assert all((out[k] == 0).all() and len(out[k]) == 3 for k in vr.FIELDS) and out["range"].shape == (3, 0)
    # a stream under capture
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        stream.wait_stream(torch.cuda.default_stream())
        graph = torch.cuda.CUDAGraph()
        with pytest.raises(g.GndtError) as err:
            with g.graph_capture(graph, stream):
                m.view_gain(p, d, R, stream=stream)
        assert err.value.code == 1
        del graph
        stream.synchronize()
        got = m.view_gain(p, d, R, stream=stream)
        stream.synchronize()
        vr.assert_same(records(got), vr.gain(s["trace"], poses=np.arange(3), dirs=np.arange(64)), "after the refused capture")


def test_frontier_views_on_the_drivable_site():
    cloud, P = scenes.drivable_site(), scenes.COST_PARAMS
    m = build(cloud, P)
    assert m.computeCost(scenes.DRIVABLE_GOAL, dict(radius=0.25))["rc"] == 0
    fr = m.frontiers(max_clusters=None)
    found = int(fr["counts"][0])
    assert found > 4
    fr = m.frontiers(max_clusters=found + 2)                               # (room to spare: two entries of size 0)
    yaws = 4
    poses = m.frontier_views(fr, yaws=yaws, height=1.0)
    assert tuple(poses.shape) == ((found + 2) * yaws, 12)
    dirs = rollouts.view_directions(np.deg2rad(90.0), np.deg2rad(20.0), 16, 3)
    assert dirs.shape == (48, 3) and dirs.dtype == np.float32 and np.allclose(np.linalg.norm(dirs, axis=1), 1.0, atol=1e-6)
    out = m.view_gain(poses, dirs, 12.0)
    got = records(out)
    assert (got["status"][:found * yaws] == 0).all() and (got["status"][found * yaws:] == 1).all() and (got["skipped"][found * yaws:] == 48).all()
    hp = poses.cpu().numpy()
    hfr = m.frontiers(max_clusters=found + 2, host=True)
    assert np.array_equal(m.frontier_views(hfr, yaws=yaws, height=1.0), hp[:found * yaws])
    want = vr.gain(vr.trace(m.export(), cloud[0], P["grid_len"], P["z_len"], hp, dirs, 12.0))
    vr.assert_same(got, want, "site")
    # the exploration step's score: unknown per pose, by cluster and yaw
    score = got["unknown"].reshape(found + 2, yaws)
    assert (score[found:] == 0).all() and score[:found].max() > score[:found].min()


def test_the_open_side_shows_more_unknown_than_the_walled_side():
    """A floor of 21 x 21 columns (cells 0 .. 20, level 1) with a wall of nodes at sensor height (level 2) in every cell of x = 20.
    Sensors at x = 10.5, z = 1.5 (level 2), y in 7.5 .. 13.5, with a horizontal fan of +-30 degrees and 30 m of range.  Looking east,
    every ray meets the wall: at x = 20 it is at most 9.5 tan 30 = 5.5 m to the side of the sensor, so inside y in [2, 19], and it
    stops there having crossed floor columns only: unknown = 0.  Looking west, nothing stands at level 2: every ray leaves the floor at
    x = 0 after at most 10.5 / cos 30 = 12.2 m and crosses columns that are not in the map for the rest of its 30 m: unknown > 0."""
    g21 = np.arange(21, dtype=np.float32) + np.float32(0.5)
    floor = np.stack([np.repeat(g21, 21), np.tile(g21, 21), np.full(441, 0.5, np.float32)], 1)
    wall = np.stack([np.full(21, 20.5, np.float32), g21, np.full(21, 1.5, np.float32)], 1)
    cloud = np.concatenate([np.zeros((1, 3), np.float32), floor, wall])
    m = build(cloud, UNIT, ATOMIC)
    cells = m.export()
    assert cells["num_nodes"] == 441 + 21
    dirs = rollouts.view_directions(np.deg2rad(60.0), 0.0, 33, 1)
    ys = np.arange(7.5, 14.0, 1.0)
    east = np.stack([pose((10.5, y, 1.5), 0.0) for y in ys])
    west = np.stack([pose((10.5, y, 1.5), np.pi) for y in ys])
    want = vr.gain(vr.trace(cells, cloud[0], 1.0, 1.0, np.concatenate([east, west]), dirs, 30.0))
    we, ww = want[:len(ys)], want[len(ys):]
    assert (we["unknown"] == 0).all() and (we["hits"] == 33).all() and (ww["hits"] == 0).all() and ww["unknown"].min() > we["unknown"].max()
    got = records(m.view_gain(np.concatenate([east, west]), dirs, 30.0))
    vr.assert_same(got, want, "open and walled")
    assert got["unknown"][len(ys):].min() > got["unknown"][:len(ys)].max()
