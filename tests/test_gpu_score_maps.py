"""GPU tier: map-to-map scoring on two device-resident maps (gndt_score_maps_device / gndt_score_maps_derivs_device,
TwoDmap.score_map / score_map_derivs / register_map / stitch(method="d2d")) against the numpy restatement of the definition
(tests/score_maps_ref.py) on the exported cells: every accumulate strategy for both maps, a source at the destination's lengths and
one at half of them with another origin, both neighbourhoods, a batch of poses with the per-node outputs; results are the same bits
from run to run, in a batch or one pose at a time, on any stream, and the derivatives' four sums are the score's; the entry points'
error codes; both maps are left as they were; and the registration driven on the device, step by step against the restatement.

Tolerances (derived in tests/score_maps_ref.py, not tuned): rows, matched and terms exact; score and d2_sum at score_ref.RTOL; g and H
entry-wise within RTOL_D x the sum of the absolute values of the entry's per-pair contributions; the per-node d2 is fp32: the
reference rounded to fp32, within 1 ulp of fp32.  Of the refusals, "handles on different devices" needs two devices and is not run
here.  The recovery cases and their endings are tests/test_score_maps_host.py's."""
import ctypes as C

import numpy as np
import pytest

from grid_ndt_amd import scenes
from tests import score_derivs_ref as dr
from tests import score_maps_ref as mr
from tests import score_ref as sr
from tests.gpu_kit import dev, handle, to_np
from tests.test_gpu_score import ATOMIC, AUTO, BOX, ERR_INVALID, PARTITION, TILE, _built, _scene, six_poses, yaw
from tests.test_gpu_score import _bits as _score_bits

pytestmark = pytest.mark.gpu


def _map_of(cloud, P, strategy=AUTO, scale=1.0, **kw):
    """the map of cloud[1:] at `scale` times P's lengths, its origin cloud[0]"""
    m = handle(dict(P, grid_len=float(np.float32(P["grid_len"]) * np.float32(scale)), z_len=float(np.float32(P["z_len"]) * np.float32(scale))),
                strategy, **kw)
    m.setCloudFirst(cloud[0])
    m.create2DMap("slope", dev(cloud[1:]))
    return m


def _second(cloud, shift=(0.0, 0.0, 0.0)):
    """every second point behind an origin row moved by `shift`"""
    return np.concatenate([cloud[:1] + np.asarray(shift, np.float32), cloud[1:][::2]]).astype(np.float32)


def _ref(dst, cloud, P, src, poses, nbh, derivs=True, **kw):
    fn = mr.derivs if derivs else mr.score
    return fn(dst.export(), cloud[0], P["grid_len"], P["z_len"], src.export(), poses, nbh, **kw)


def _bits(out):
    """every value of a result as integers: the four sums, then g and H where there are any"""
    o = to_np(out)
    b = list(_score_bits(out))
    for k in ("g", "H"):
        if k in o:
            b.append(np.ascontiguousarray(o[k], np.float64).view(np.uint64).reshape(len(o[k]), -1).tolist())
    return b


def _pose(bits, k):
    return [v[k] for v in bits]


# ---- 1. against the restatement ----

@pytest.mark.parametrize("source", ["same", "half"])
@pytest.mark.parametrize("strategy", [ATOMIC, PARTITION, TILE, AUTO])
@pytest.mark.parametrize("name", ["bridge_ground", "uniform_box", "terrain", "face_lattice"])
def test_maps_equal_the_restatement(name, strategy, source):
    cloud, P, dst = _built(name, strategy)
    if source == "same":
        src = _map_of(_second(cloud), P, strategy)
    else:
        src = _map_of(_second(cloud, (0.13 * P["grid_len"], -0.07 * P["grid_len"], 0.05 * P["z_len"])), P, strategy, scale=0.5)
    poses = six_poses(P)
    for nbh in (1, 7):
        want = _ref(dst, cloud, P, src, poses, nbh)
        # (every second point of face_lattice leaves at most 2 points in a half-length cell: no source row counts, and the answer is 0)
        empty = (name, source) == ("face_lattice", "half")
        assert (len(want["source"].idx) == 0 and not want["terms"].any()) if empty else (want["terms"][0] > 100 and (want["terms"][:4] > 0).all())
        got = to_np(dst.score_map_derivs(src, poses, neighbourhood=nbh))
        mr.assert_derivs(got, want, what=(name, strategy, source, nbh))
        assert np.array_equal(got["H"], got["H"].transpose(0, 2, 1))
        for k in (0, 3):
            plain = to_np(dst.score_map(src, poses, neighbourhood=nbh, per_node=k))
            mr.assert_pose_sums(plain, want, what=(name, strategy, source, nbh))
            mr.assert_per_node(plain["d2"], plain["row"], want["poses_out"][k], what=(name, strategy, source, nbh, k))
        # off the map, and the pose with a NaN: exactly 0
        for j in (4, 5):
            assert got["score"][j] == 0.0 and got["d2_sum"][j] == 0.0 and got["matched"][j] == 0 and got["terms"][j] == 0
            assert not got["g"][j].any() and not got["H"][j].any()
            assert plain["score"][j] == 0.0 and plain["d2_sum"][j] == 0.0 and plain["matched"][j] == 0 and plain["terms"][j] == 0
        if nbh == 7 and not empty:
            assert want["terms"][0] > want["matched"][0]           # (neighbours did contribute)


# ---- 2. bits ----

def test_results_are_the_same_bits_every_way():
    import torch
    cloud, P, dst = _built("terrain")
    src = _map_of(_second(cloud), P)
    poses = six_poses(P)
    for nbh in (1, 7):
        first = dst.score_map_derivs(src, poses, neighbourhood=nbh)
        b0 = _bits(first)
        assert b0[3][0] > 1000
        plain = dst.score_map(src, poses, neighbourhood=nbh, per_node=3)
        p0, d0, r0 = _bits(plain), to_np(plain)["d2"].view(np.uint32), to_np(plain)["row"]
        assert p0 == b0[:4]                                        # the derivatives' first four fields are the score's bits
        for _ in range(2):                                         # three calls in all
            assert _bits(dst.score_map_derivs(src, poses, neighbourhood=nbh)) == b0
            again = dst.score_map(src, poses, neighbourhood=nbh, per_node=3)
            assert _bits(again) == p0
            assert np.array_equal(to_np(again)["d2"].view(np.uint32), d0) and np.array_equal(to_np(again)["row"], r0)
        for k in range(6):                                         # a batch of 6 = six single-pose calls
            assert _pose(_bits(dst.score_map_derivs(src, poses[k], neighbourhood=nbh)), 0) == _pose(b0, k), (nbh, k)
            assert _pose(_bits(dst.score_map(src, poses[k], neighbourhood=nbh)), 0) == _pose(p0, k), (nbh, k)
        s = torch.cuda.Stream()                                    # another stream = the handle's
        torch.cuda.synchronize()
        o1, o2 = dst.score_map_derivs(src, poses, neighbourhood=nbh, stream=s), dst.score_map(src, poses, neighbourhood=nbh, stream=s)
        s.synchronize()
        assert _bits(o1) == b0 and _bits(o2) == p0
    # the map against itself
    for nbh in (1, 7):
        want = _ref(dst, cloud, P, dst, poses, nbh)
        got = dst.score_map_derivs(dst, poses, neighbourhood=nbh)
        mr.assert_derivs(to_np(got), want, what=("self", nbh))
        assert _bits(dst.score_map(dst, poses, neighbourhood=nbh)) == _bits(got)[:4]
    own = to_np(dst.score_map(dst, yaw(0), per_node=0))
    counted = ~np.isnan(own["d2"])
    assert counted.sum() > 1000 and int(own["terms"][0]) == int(own["matched"][0])


def test_a_source_of_one_partial_tile_and_one_with_rows_without_statistics():
    cloud, P = scenes.drivable_site(100_000), scenes.COST_PARAMS
    dst = _map_of(np.concatenate([cloud[:1], cloud[1::2]]), P)
    poses = six_poses(P)
    # the few hundred points of a 6 m x 5 m patch: fewer than 256 rows
    pts = cloud[2::2]
    few = _map_of(np.concatenate([cloud[:1], pts[(np.abs(pts[:, 0]) < 3.0) & (np.abs(pts[:, 1]) < 2.5)]]), P)
    rows = few.sync()[0]
    assert 0 < rows < 256
    # every other point: not a multiple of 256 rows, and the thinned corner's rows without statistics among the counted ones
    half = _map_of(np.concatenate([cloud[:1], cloud[2::2]]), P)
    cells = half.export()
    has = (np.asarray(cells["flags"]) & 1) != 0
    assert half.sync()[0] % 256 != 0 and 0 < (~has).sum() < len(has) and (~has)[:np.flatnonzero(has)[-1]].any()
    for src, floor in ((few, 30), (half, 1000)):
        for nbh in (1, 7):
            want = _ref(dst, cloud, P, src, poses, nbh)
            assert want["terms"][0] > floor
            got = dst.score_map_derivs(src, poses, neighbourhood=nbh)
            mr.assert_derivs(to_np(got), want, what=("rows", floor, nbh))
            plain = dst.score_map(src, poses, neighbourhood=nbh, per_node=1)
            assert _bits(plain) == _bits(got)[:4]
            mr.assert_per_node(to_np(plain)["d2"], to_np(plain)["row"], want["poses_out"][1], what=("rows", floor, nbh))


def test_a_batch_launched_in_groups_of_poses_has_the_single_calls_bits():
    """a 3 M-point box is some 640 000 rows, 2 500 tiles: 600 KB of the derivatives' partial sums a pose and 60 KB of the score's, so
    one launch's scratch (64 MiB) takes some 110 poses of the one and 1 100 of the other — two poses more than that go in two groups,
    and pose k's record is what a single-pose call gives"""
    cloud = scenes.uniform_box(3_000_001)
    dst = handle(BOX, max_nodes_hint=1 << 20)
    dst.setCloudFirst(cloud[0])
    dst.create2DMap("slope", dev(cloud[1:]))
    src = handle(BOX, max_nodes_hint=1 << 20)
    src.setCloudFirst(cloud[0])
    src.create2DMap("slope", dev(cloud[1:][::2]))
    tiles = (src.sync()[0] + 255) // 256
    waves = (29 * 16 + 2 * 16) * 8
    for width, per_tile, call in ((31, 240, dst.score_map_derivs), (4, 24, dst.score_map)):
        chunk = (64 << 20) // (tiles * per_tile + (waves if width == 31 else 0))
        K = chunk + 2
        assert 2 < K <= 65535
        rng = np.random.default_rng(9)
        poses = np.stack([yaw(float(a), (float(x), float(y), 0.0)) for a, x, y in zip(rng.uniform(-1, 1, K), rng.uniform(-.2, .2, K), rng.uniform(-.2, .2, K))])
        bb = _bits(call(src, poses))
        assert min(bb[3]) > 100_000
        for k in (0, chunk - 1, chunk, K - 1):
            assert _pose(_bits(call(src, poses[k])), 0) == _pose(bb, k), (width, k)
    batch = dst.score_map(src, poses, per_node=K - 1)              # the per-node outputs of a pose of the second group
    one = dst.score_map(src, poses[K - 1], per_node=0)
    assert np.array_equal(to_np(one)["d2"].view(np.uint32), to_np(batch)["d2"].view(np.uint32)) and np.array_equal(to_np(one)["row"], to_np(batch)["row"])


# ---- 3. errors and capture ----

def _raw(dst, src, poses, K, prm, out=True, d2=False, row=False, derivs=False, stream=None):
    """the C entry points themselves -> rc"""
    import torch
    from grid_ndt_amd._lib import ScoreParams
    p = ScoreParams(*prm) if prm is not None else None
    n = max(src.sync()[0], 1) if src is not None and src._h is not None else 1
    rec = torch.zeros((max(K, 1), 31), dtype=torch.int64, device="cuda")
    a = torch.zeros(n, dtype=torch.float32, device="cuda")
    b = torch.zeros(n, dtype=torch.int32, device="cuda")
    tq = torch.from_numpy(poses).cuda() if poses is not None else None
    ptr = lambda x: C.c_void_p(x.data_ptr())
    hd, hs = (dst._h if dst is not None else None), (src._h if src is not None else None)
    if derivs:
        rc = dst_lib(dst, src).gndt_score_maps_derivs_device(hd, hs, ptr(tq) if tq is not None else None, K, C.byref(p) if p is not None else None,
                                                             ptr(rec) if out else None, stream)
    else:
        rc = dst_lib(dst, src).gndt_score_maps_device(hd, hs, ptr(tq) if tq is not None else None, K, C.byref(p) if p is not None else None,
                                                      ptr(rec) if out else None, ptr(a) if d2 else None, ptr(b) if row else None, stream)
    torch.cuda.synchronize()
    return rc


def dst_lib(dst, src):
    return (dst if dst is not None else src)._L


def test_empty_inputs_and_errors():
    import torch
    import grid_ndt_amd as g
    cloud, P, dst = _built("uniform_box", ATOMIC)
    src = _map_of(_second(cloud), P, ATOMIC)
    poses = six_poses(P)
    T = np.ascontiguousarray(poses.reshape(6, 12))
    ok = (1, 0, 0.0, 0.0, 0.0, 0)
    for derivs in (False, True):
        assert _raw(dst, src, T, 0, ok, derivs=derivs) == 0
        assert _raw(dst, src, None, 0, ok, out=False, derivs=derivs) == 0
        assert _raw(dst, src, T, 6, ok, derivs=derivs) == 0
        # the refusals
        assert _raw(None, src, T, 6, ok, derivs=derivs) == ERR_INVALID                    # a null handle
        assert _raw(dst, None, T, 6, ok, derivs=derivs) == ERR_INVALID
        assert _raw(dst, src, T, 6, None, derivs=derivs) == ERR_INVALID                   # null params
        assert _raw(dst, src, T, 6, ok, out=False, derivs=derivs) == ERR_INVALID          # null out
        assert _raw(dst, src, None, 6, ok, derivs=derivs) == ERR_INVALID                  # null poses
        for nbh in (0, 2, 6, 27, -1):
            assert _raw(dst, src, T, 6, (nbh, 0, 0.0, 0.0, 0.0, 0), derivs=derivs) == ERR_INVALID
        for mc in (1, 2, -3):
            assert _raw(dst, src, T, 6, (1, mc, 0.0, 0.0, 0.0, 0), derivs=derivs) == ERR_INVALID
        assert _raw(dst, src, T, 6, (1, 3, 0.0, 0.0, 0.0, 0), derivs=derivs) == 0
        for bad in (-1.0, float("nan"), float("inf")):
            for slot in (2, 3, 4):
                prm = [1, 0, 0.0, 0.0, 0.0, 0]
                prm[slot] = bad
                assert _raw(dst, src, T, 6, tuple(prm), derivs=derivs) == ERR_INVALID, (bad, slot)
        big = np.ascontiguousarray(np.tile(T[:1], (65536, 1)))
        assert _raw(dst, src, big, 65536, ok, derivs=derivs) == ERR_INVALID               # K above the grid's y limit
    assert _raw(dst, src, T, 6, ok, d2=True, row=True) == 0
    assert _raw(dst, src, T, 6, (1, 0, 0.0, 0.0, 0.0, 6), d2=True) == ERR_INVALID         # node_pose >= K
    assert _raw(dst, src, T, 6, (1, 0, 0.0, 0.0, 0.0, 6), row=True) == ERR_INVALID
    assert _raw(dst, src, T, 6, (1, 0, 0.0, 0.0, 0.0, 6)) == 0                            # (not asked for: not looked at)
    assert _raw(dst, src, T, 6, (1, 0, 0.0, 0.0, 0.0, 6), derivs=True) == 0
    # min_count below either handle's min_points
    m5 = _map_of(_second(cloud), P, ATOMIC, min_points=5)
    for a, b in ((dst, m5), (m5, dst)):
        assert _raw(a, b, T, 6, (1, 4, 0.0, 0.0, 0.0, 0)) == ERR_INVALID
        assert _raw(a, b, T, 6, (1, 5, 0.0, 0.0, 0.0, 0)) == 0
    got = to_np(dst.score_map_derivs(m5, poses, neighbourhood=7))
    mr.assert_derivs(got, _ref(dst, cloud, P, m5, poses, 7, src_min_points=5), what="min_points 5")
    # no source rows: K zeroed records
    empty = _map_of(_second(cloud), P, ATOMIC)
    empty.crop_box((30000, 30010, 30000, 30010), "keep_inside")
    assert empty.sync()[0] == 0
    for out in (to_np(dst.score_map(empty, poses, per_node=1)), to_np(dst.score_map_derivs(empty, poses))):
        assert len(out["score"]) == 6 and not any(np.asarray(out[k]).any() for k in out if k not in ("d2", "row"))
    assert out["H"].shape == (6, 6, 6)
    # no finished build in either handle
    e = handle(P)
    e.setCloudFirst((0.0, 0.0, 0.0))
    e._ensure("slope")
    for a, b in ((dst, e), (e, dst)):
        for call in (a.score_map, a.score_map_derivs):
            with pytest.raises(g.GndtError) as err:
                call(b, poses)
            assert err.value.code == ERR_INVALID
    # a capturing stream: refused, and the capture goes on
    from grid_ndt_amd._lib import ScoreParams
    want = _bits(dst.score_map_derivs(src, poses))
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    x = torch.zeros(16, device="cuda")
    tq = torch.from_numpy(T).cuda()
    rec = torch.zeros((6, 31), dtype=torch.int64, device="cuda")
    prm = ScoreParams(*ok)
    torch.cuda.synchronize()
    with g.graph_capture(graph, stream=s):
        rc1 = dst._L.gndt_score_maps_device(dst._h, src._h, C.c_void_p(tq.data_ptr()), 6, C.byref(prm), C.c_void_p(rec.data_ptr()), None, None,
                                            C.c_void_p(s.cuda_stream))
        rc2 = dst._L.gndt_score_maps_derivs_device(dst._h, src._h, C.c_void_p(tq.data_ptr()), 6, C.byref(prm), C.c_void_p(rec.data_ptr()),
                                                   C.c_void_p(s.cuda_stream))
        x.add_(1.0)
    assert rc1 == ERR_INVALID and rc2 == ERR_INVALID
    graph.replay()
    torch.cuda.synchronize()
    assert float(x[0]) == 1.0
    assert _bits(dst.score_map_derivs(src, poses)) == want


# ---- 4. the maps are untouched ----

def _same_export(before, after):
    assert before.keys() == after.keys()
    for k in before:
        a, b = np.asarray(before[k]), np.asarray(after[k])
        assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b), k


@pytest.mark.parametrize("strategy", [ATOMIC, PARTITION])
def test_the_maps_are_untouched(strategy):
    cloud, P, dst = _built("terrain", strategy)
    src = _map_of(_second(cloud), P, strategy)
    scan = dev(cloud[1:][::3])
    before = (dst.export(), src.export(), dst.sync(), src.sync(), _score_bits(dst.score_poses(scan, six_poses(P), neighbourhood=7)))
    for nbh in (1, 7):
        dst.score_map(src, six_poses(P), neighbourhood=nbh, per_node=2)
        dst.score_map_derivs(src, six_poses(P), neighbourhood=nbh)
    assert (dst.sync(), src.sync()) == before[2:4]
    _same_export(before[0], dst.export())
    _same_export(before[1], src.export())
    assert _score_bits(dst.score_poses(scan, six_poses(P), neighbourhood=7)) == before[4]


# ---- 5. registration on the device ----

def _recovery_maps(scene, frame):
    from tests.test_score_derivs_host import RECOVERY_SCENES
    from tests.test_score_maps_host import TRUTH, split_cloud
    cloud, P = RECOVERY_SCENES[scene]()
    dst = _map_of(split_cloud(cloud, 1), P, ATOMIC)
    src = _map_of(split_cloud(cloud, 2, None if frame == "same" else TRUTH[frame]), P, ATOMIC)
    return cloud, P, dst, src, TRUTH[frame]


def _recovery_cases():
    from tests.test_score_maps_host import RECOVERY_CASES
    return RECOVERY_CASES


@pytest.mark.parametrize("nbh", [1, 7])
@pytest.mark.parametrize("scene,frame,start", _recovery_cases())
def test_register_map_on_the_device_step_by_step(scene, frame, start, nbh):
    from tests.test_score_derivs_host import check_steps, starts
    from tests.test_score_maps_host import RECOVERY, assert_recovered, compose
    cloud, P, dst, src, truth = _recovery_maps(scene, frame)
    ref_eval, ref_score = mr.callables(dst.export(), cloud[0], P["grid_len"], P["z_len"], src.export(), nbh)
    T0 = compose(starts(P)[start], truth)
    r = dst.register_map(src, T0, neighbourhood=nbh)
    print(scene, frame, nbh, start, "device:", r["reason"], r["iterations"], "documented:", RECOVERY[(scene, frame, nbh, start)])
    check_steps(r, T0, ref_eval, ref_score, 0.5 * P["grid_len"], what=("device", scene, frame, nbh, start))
    assert_recovered(r["T"], T0, truth, what=("device", scene, frame, nbh, start))


def test_stitch_d2d_registers_then_merges_and_means_is_unchanged():
    from tests.test_score_derivs_host import starts
    from tests.test_score_maps_host import assert_recovered, compose
    cloud, P, a, src, truth = _recovery_maps("drivable_site", "moved")
    T0 = compose(starts(P)["A"], truth)
    before = src.export()
    res, st = a.stitch(src, T0, method="d2d")
    assert_recovered(res["T"], T0, truth, what="stitch d2d")
    b = _recovery_maps("drivable_site", "moved")[2]
    assert st == b.merge_from(src, pose=res["T"]) and st["merged_nodes"] == before["num_nodes"]
    ea, eb = a.export(), b.export()                                # (the merge's floating-point adds have no fixed order: the exact fields)
    for k in ("sx", "sy", "sz", "count", "first_idx", "flags"):
        assert np.array_equal(np.asarray(ea[k]), np.asarray(eb[k])), k
    _same_export(before, src.export())
    # method="means" is the default, and what stitch did before: the same poses in history
    c, d = _recovery_maps("drivable_site", "moved")[2], _recovery_maps("drivable_site", "moved")[2]
    r1, s1 = c.stitch(src, T0)
    r2, s2 = d.stitch(src, T0, method="means")
    assert s1 == s2 and r1["reason"] == r2["reason"] and len(r1["history"]) == len(r2["history"])
    for h1, h2 in zip(r1["history"], r2["history"]):
        assert np.array_equal(np.asarray(h1["T"]).view(np.uint64), np.asarray(h2["T"]).view(np.uint64))
    cells = src.export()
    ref = _recovery_maps("drivable_site", "moved")[2].register(dev(cells["mean"][(cells["flags"] & 1) != 0]), T0)
    assert np.array_equal(np.asarray(r1["T"]).view(np.uint64), np.asarray(ref["T"]).view(np.uint64)) and r1["iterations"] == ref["iterations"]
    with pytest.raises(ValueError):
        c.stitch(src, T0, method="points")


def test_register_map_with_a_one_level_pyramid_recovers_start_b():
    """the moved frame's start B at neighbourhood 7 through one coarser destination level: the restatement's run ends 7.8 mm and
    0.5 mrad off with the source scored as it is at both levels, 5.4 mm and 0.2 mrad off with the source's own coarse map at the
    coarse level"""
    from tests.test_score_derivs_host import starts
    from tests.test_score_maps_host import assert_recovered, compose
    cloud, P, dst, src, truth = _recovery_maps("drivable_site", "moved")
    T0 = compose(starts(P)["B"], truth)
    pyr = dst.pyramid(1)
    r = dst.register_map(src, T0, pyramid=pyr)
    assert len(r["levels"]) == 2
    assert_recovered(r["T"], T0, truth, what="pyramid, the source as it is")
    r2 = dst.register_map(src, T0, pyramid=pyr, other_pyramid=src.pyramid(1))
    assert len(r2["levels"]) == 2
    assert_recovered(r2["T"], T0, truth, what="pyramid, the source's own coarse map")
    with pytest.raises(ValueError):
        dst.register_map(src, T0, pyramid=pyr, other_pyramid=[])
