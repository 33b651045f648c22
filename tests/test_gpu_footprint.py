"""GPU tier: footprint poses (gndt_footprint_poses_device / gndt_footprint_poses, TwoDmap.footprints / footprints_along).  Every map is
built on the device; the device must equal the shim (tests/footprint_shim.cpp: the kernel's own per-pose code lane after lane, on the
handle's own export) bit for bit — every word of every info record and every row — through both entry points, into outputs
over-allocated with a sentinel tail that must stay untouched.  Box sizes n = 1, 3, 4 (the first with a second position a lane) and 15
(961 of the table's 1024 words), n = 16 refused; the wavefront, workgroup and grid-stride edges of K; both strides; the row caps around
`support`; a mixed batch against its poses alone, permuted, and run twice; the handle's lives; every refused argument; and a poisoned
tier of this file's own.  No tolerance anywhere."""
import ctypes as C
import numpy as np
import pytest

from tests import footprint_cases as fc
from tests import footprint_ref as fr
from tests import poison_tier
from tests.gpu_kit import Padded, PaddedCall, build, dev, robot_arg, to_np

pytestmark = pytest.mark.gpu

ERR_INVALID = 1
ATOMIC = 1
SENTINEL = 0xDEADBEEF
PAD = 3                      # sentinel entries behind the outputs
WAVES = 4                    # kFootWaves: wavefronts (poses) a workgroup
MAX_BLOCKS = 1024            # kFootMaxBlocks: one trip of the grid-stride loop holds WAVES * MAX_BLOCKS poses
P = fc.PLANE_P
_scenes = {}


def raw(m, poses, hl, hw, robot=None, max_dz=0.0, height=0.0, min_cells=0, min_cover=0.0, weight=0, row_cap=0, stride=20, stream=None, host=False,
        reserved=(0,) * 5):
    """The C entry points; info K + PAD records and K * row_cap + PAD row words of sentinel -> (rc, info [K], rows, untouched: the
    tails still hold the sentinel)"""
    from grid_ndt_amd._lib import FootprintParams
    K = len(poses)
    prm = FootprintParams(hl, hw, max_dz, height, min_cells, min_cover, weight, (C.c_uint32 * 5)(*reserved))
    info, rows = Padded(K, words=16, back=PAD, fill=SENTINEL), Padded(K * row_cap, back=PAD, fill=SENTINEL)
    rc = PaddedCall(host, stream, wait_for_current=True)(m._L.gndt_footprint_poses, m._L.gndt_footprint_poses_device, m._h,
                                                         fc.strided(poses, stride) if K else None, K, stride, robot_arg(robot, fr.ROBOT), C.byref(prm),
                                                         rows if row_cap else None, row_cap, info)
    return rc, info.body.view(fr.INFO_DTYPE), rows.body.reshape(K, row_cap), info.untouched() and rows.untouched()


def check(m, t, poses, hl, hw, what="", entries=(False, True), stream=None, row_cap=8, **kw):
    """both entry points against the shim on the rows t -> the shim's (info, rows)"""
    want = fc.run(t, poses, hl, hw, row_cap=row_cap, **kw)
    for host in entries:
        tag = (what, "host" if host else "device")
        rc, info, rows, untouched = raw(m, poses, hl, hw, row_cap=row_cap, host=host, stream=None if host else stream, **kw)
        assert rc == 0, (tag, m._L.gndt_last_error(m._h))
        fr.same_bits(info, rows, *want, tag)
        assert untouched, tag
    return want


def drawn(name, make=None, P=P):
    """a map built from a cloud -> (m, the rows of its export for the shim, the cloud)"""
    if name not in _scenes:
        cloud = make()
        m = build(cloud, P)
        _scenes[name] = (m, fc.map_rows(m.export(), cloud[0, :3], P), cloud)
    return _scenes[name]


def _plane():
    return drawn("plane", lambda: fc.plane_cloud(0.2, -0.1, noise=0.01))


def _poses(t, K, seed=3):
    rng = np.random.default_rng(seed)
    return fc.random_poses(rng, K, (-3.5, -3.5), (3.5, 3.5), -1.0, 1.0, on=t.mean[(t.flags & 2) != 0])


# ---- shapes and batches -----------------------------------------------------------------------------------------------------------------

# half extents on 0.5 m cells -> n = ceil(sqrt(hl^2 + hw^2) / 0.5)
BOXES = {1: (0.3, 0.2), 3: (1.2, 0.6), 4: (1.7, 0.9), 15: (7.0, 2.6)}


@pytest.mark.parametrize("n", sorted(BOXES))
def test_every_box_size_both_weights_and_a_band(n):
    m, t, _ = _plane()
    hl, hw = BOXES[n]
    assert fr.box_n(hl, hw, 0.5) == n
    poses = np.concatenate([_poses(t, 9, seed=n), fc.mixed_batch(t, np.random.default_rng(n))])
    got, _ = check(m, t, poses, hl, hw, n, min_cells=1)
    assert (got["status"] == fr.OK).sum() >= 9 and got["cells"].max() > {1: 1, 3: 9, 4: 20, 15: 200}[n]
    check(m, t, poses, hl, hw, (n, "count"), weight=fr.COUNT, max_dz=0.4, height=1.0, min_cover=0.7, row_cap=3, stride=32)


def test_a_box_of_n_16_is_refused():
    m, t, _ = _plane()
    poses = _poses(t, 2)
    for host in (False, True):
        assert raw(m, poses, 7.9, 0.5, host=host)[0] == ERR_INVALID                # sqrt(7.9^2 + 0.5^2) / 0.5 = 15.83 -> 16
        assert raw(m, poses, 7.4, 0.5, host=host)[0] == 0                          # 14.83 -> 15


@pytest.mark.parametrize("K", [1, 3, 4, 5])
def test_wavefront_and_workgroup_edges_of_K(K):
    m, t, _ = _plane()
    check(m, t, _poses(t, K, seed=K), 1.2, 0.6, K, stride=20 if K % 2 else 32)


def test_more_poses_than_one_trip_of_the_grid_stride_loop():
    m, t, _ = _plane()
    few = np.concatenate([_poses(t, 5), fc.mixed_batch(t, np.random.default_rng(2))])
    K = WAVES * MAX_BLOCKS + 1
    poses = few[np.arange(K) % len(few)]
    want, wrows = fc.run(t, few, 1.2, 0.6, row_cap=4)
    rc, info, rows, untouched = raw(m, poses, 1.2, 0.6, row_cap=4)
    assert rc == 0 and untouched
    fr.same_bits(info, rows, want[np.arange(K) % len(few)], wrows[np.arange(K) % len(few)], "tiled")


def test_row_caps_around_support():
    m, t, _ = _plane()
    poses = _poses(t, 6)
    full, frows = fc.run(t, poses, 1.2, 0.6, row_cap=64)
    s = int(full["support"][0])
    assert 3 < s < 64 and (frows[0, :s] != fr.NO_ROW).all() and (frows[0, s:] == fr.NO_ROW).all()
    for cap in (0, 1, s - 1, s):
        got, rows = check(m, t, poses, 1.2, 0.6, ("cap", cap), row_cap=cap)
        assert np.array_equal(rows, frows[:, :cap])
        fr.same_bits(got, None, full, None, ("cap", cap))


def test_a_mixed_batch_alone_permuted_and_twice():
    m, t, _ = _plane()
    rng = np.random.default_rng(9)
    poses = np.concatenate([fc.mixed_batch(t, rng), _poses(t, 6, seed=4)])
    far = poses[:1].copy()
    far[0, :3] = [3.9, 3.9, 0.4]                                               # the map's corner: sparse under min_cells
    poses = np.concatenate([poses, far])
    kw = dict(min_cells=8, height=1.0, min_cover=0.9)
    want, wrows = check(m, t, poses, 1.2, 0.6, "mixed", **kw)
    assert set(want["status"].tolist()) == {fr.OK, fr.BAD_POSE, fr.NO_GROUND, fr.SPARSE}, want["status"]
    for k in range(len(poses)):
        rc, info, rows, untouched = raw(m, poses[k:k + 1], 1.2, 0.6, row_cap=8, **kw)
        assert rc == 0 and untouched
        fr.same_bits(info, rows, want[k:k + 1], wrows[k:k + 1], ("alone", k))
    perm = rng.permutation(len(poses))
    rc, info, rows, untouched = raw(m, poses[perm], 1.2, 0.6, row_cap=8, **kw)
    assert rc == 0 and untouched
    fr.same_bits(info, rows, want[perm], wrows[perm], "permuted")
    again = raw(m, poses, 1.2, 0.6, row_cap=8, **kw)
    fr.same_bits(again[1], again[2], want, wrows, "twice")


def test_the_python_wrapper_yaw_poses_and_paths():
    import torch
    m, t, _ = _plane()
    poses = _poses(t, 7)
    want, wrows = fc.run(t, poses, 1.2, 0.6, row_cap=5, height=1.0)
    for host in (False, True):
        got = m.footprints(poses if host else dev(poses), 1.2, 0.6, height=1.0, rows=5, host=host)
        for k in ("status", "flags", "centre_row", "cells", "support", "gaps", "unknown"):
            assert np.array_equal(to_np(got[k]).astype(np.int64) & 0xFFFFFFFF, want[k].astype(np.int64)), (host, k)
        for k in ("z", "normal", "along", "across", "rms", "step_max", "bump_max", "headroom"):
            assert np.array_equal(to_np(got[k]).view(np.uint32), want[k].view(np.uint32)), (host, k)
        assert np.array_equal(to_np(got["rows"]).view(np.uint32), wrows)
        # (the arctangent is the wrapper's, numpy's on the host and torch's on the device: theirs differ in the last place of fp32)
        assert np.abs(to_np(got["pitch"]) - np.arctan(want["along"])).max() <= (0 if host else 1e-6)
        assert np.abs(to_np(got["roll"]) - np.arctan(want["across"])).max() <= (0 if host else 1e-6)
        assert np.array_equal(to_np(got["ok"]), (want["status"] == 0) & (want["flags"] == 0))
    yaw = np.arctan2(poses[:, 4].astype(np.float64), poses[:, 3].astype(np.float64)).astype(np.float32)
    by_yaw = m.footprints(np.concatenate([poses[:, :3], yaw[:, None]], 1), 1.2, 0.6)
    assert np.array_equal(by_yaw["cells"], want["cells"]) and np.abs(by_yaw["along"] - want["along"]).max() < 1e-5
    # two paths, the second ending early: every finite waypoint is evaluated with the heading to the next
    from grid_ndt_amd import rollouts
    paths = np.zeros((2, 4, 3), np.float32)
    paths[0, :, 0], paths[0, :, 1] = [-2.0, -1.0, 0.2, 1.5], [0.3, 0.5, 0.4, 0.1]
    paths[1, :, 0], paths[1, :, 1] = [1.0, 1.2, np.nan, 0.0], [-2.0, -1.0, 0.0, 0.0]
    along = m.footprints_along(dev(paths), 0.6, 0.4)
    flat, _ = fc.run(t, rollouts.headings(paths).reshape(8, 5), 0.6, 0.4)
    assert tuple(along["status"].shape) == (2, 4) and np.array_equal(to_np(along["status"]).ravel(), flat["status"])
    assert np.array_equal(to_np(along["z"]).view(np.uint32).ravel(), flat["z"].view(np.uint32))
    assert to_np(along["status"])[1].tolist() == [0, 0, 1, 1] and to_np(along["stands"]).tolist() == [True, True]
    assert m.footprints_along(paths, 0.6, 0.4, host=True)["stands"].tolist() == [True, True]
    for rows in (0, 3):                                      # no poses, with and without rows asked for, through both entry points
        for empty in (torch.zeros((0, 5), device="cuda"), np.zeros((0, 5), np.float32)):
            none = m.footprints(empty, 0.6, 0.4, rows=rows)
            assert len(none["status"]) == 0 and len(none["ok"]) == 0
            assert "rows" not in none if rows == 0 else tuple(none["rows"].shape) == (0, 3)


# ---- the handle's lives -----------------------------------------------------------------------------------------------------------------

def test_first_builder_of_the_column_index_a_large_host_call_then_a_small_one():
    import torch
    cloud = fc.kerb_cloud(0.2)
    m = build(cloud, P)                                     # a handle no consumer has touched: this call makes the column index
    t = fc.map_rows(m.export(), cloud[0, :3], P)
    poses = fc.headed([[0.1, 0.7, 0.1], [-0.2, -1.3, 0.3], [2.3, 2.1, 0.2]], [0.0, 2.0, -1.0])          # two across the kerb, one beside it
    want = check(m, t, poses, 1.2, 0.6, "first call", entries=(False,))
    assert (want[0]["flags"] & fr.STEP).any()
    big = poses[np.arange(4096) % 3]
    rc, info, rows, untouched = raw(m, big, 1.2, 0.6, row_cap=8, host=True)      # the host call's scratch grows ...
    assert rc == 0 and untouched
    fr.same_bits(info, rows, want[0][np.arange(4096) % 3], want[1][np.arange(4096) % 3], "4096")
    st = torch.cuda.Stream()
    for i in range(2):                                       # ... and is used again by a call of 3
        again = check(m, t, poses, 1.2, 0.6, ("after the larger call", i), stream=st if i else None)
        fr.same_bits(*again, *want, i)


def test_after_an_update_a_crop_a_clear_and_a_flood():
    import torch
    from grid_ndt_amd import scenes
    cloud = scenes.bridge_ground()
    BP = scenes.BRIDGE_PARAMS
    m = build(cloud, BP, ATOMIC)                            # (updates need the additive strategy)
    rng = np.random.default_rng(12)
    ok = 0

    def fresh(what):
        nonlocal ok
        t = fc.map_rows(m.export(), cloud[0, :3], BP)
        slopes = t.mean[(t.flags & 2) != 0]
        poses = fc.random_poses(rng, 12, slopes[:, :2].min(0), slopes[:, :2].max(0), 0.8, 3.2, on=slopes)
        for robot, kw in ((None, dict(max_dz=0.5, height=1.9)), (dict(reachable_height=0.05, max_angle_deg=12.0), dict(weight=fr.COUNT))):
            got, _ = check(m, t, poses, 0.3, 0.2, (what, robot), robot=robot, entries=(False,), **kw)
            ok += int((got["status"] == fr.OK).sum())
        return t

    before = fresh("before")
    x0, x1 = int(before.sx.min()), int(before.sx.max())
    m.change2DMap("slope", dev(cloud[1:4000, :3] + np.float32([0.0, 0.0, 0.3])))
    fresh("update")
    m.crop_box((x0 + (x1 - x0) // 4, x1 - (x1 - x0) // 4, -100000, 100000), "keep_inside")
    cropped = fresh("crop")
    assert cropped.n < before.n and ok > 40
    ends = cropped.mean[(cropped.flags & 2) != 0][::7].astype(np.float32) + np.float32([0, 0, -0.4])
    m.clear_rays((8.0, 3.0, 6.0), dev(ends))
    cleared = fresh("clear")
    assert cleared.n < cropped.n
    # a flood in between: the call only reads, h and state are what they were
    m.computeCost((9.5, 3.0, 1.0), robot={"radius": 0.25})
    h0 = m.cost_export()
    fresh("flood")
    h1 = m.cost_export()
    assert h0["h"].tobytes() == h1["h"].tobytes() and h0["state"].tobytes() == h1["state"].tobytes()
    # everything cropped away: no ground anywhere
    m.crop_box((x1 + 50, x1 + 60, 1, 2), "keep_inside")
    assert m.sync()[0] == 0
    for host in (False, True):
        rc, info, rows, untouched = raw(m, fc.headed([[8.0, 3.0, 1.0]], [0.0]), 0.3, 0.2, row_cap=2, host=host)
        assert rc == 0 and info["status"][0] == fr.NO_GROUND and (rows == fr.NO_ROW).all() and untouched


# ---- refusals --------------------------------------------------------------------------------------------------------------------------

def test_refused_arguments():
    import torch
    import grid_ndt_amd as g
    from grid_ndt_amd._lib import FootprintParams
    m, t, _ = _plane()
    poses = _poses(t, 2)
    nan, inf = float("nan"), float("inf")
    for host in (False, True):
        assert raw(m, poses, 1.2, 0.6, host=host)[0] == 0
        for hl, hw in ((0.0, 0.6), (1.2, 0.0), (-1.2, 0.6), (1.2, -0.6), (nan, 0.6), (1.2, nan), (inf, 0.6), (1.2, inf)):
            assert raw(m, poses, hl, hw, host=host)[0] == ERR_INVALID, (hl, hw)
        for weight in (2, 3, 0x80000000):
            assert raw(m, poses, 1.2, 0.6, weight=weight, host=host)[0] == ERR_INVALID, weight
        for k in range(5):
            assert raw(m, poses, 1.2, 0.6, reserved=tuple(int(j == k) for j in range(5)), host=host)[0] == ERR_INVALID, k
        for bad in (dict(max_dz=-0.1), dict(height=nan), dict(min_cover=-1.0)):
            assert raw(m, poses, 1.2, 0.6, host=host, **bad)[0] == ERR_INVALID, bad
        for stride in (24, 32, 64):
            assert raw(m, poses, 1.2, 0.6, stride=stride, host=host)[0] == 0
    prm = FootprintParams(1.2, 0.6)
    buf = torch.zeros(256, dtype=torch.int32, device="cuda")
    d_poses = dev(fc.strided(poses, 32))
    p = lambda x, off=0: C.c_void_p(x.data_ptr() + off)
    call = m._L.gndt_footprint_poses_device
    X, B = p(d_poses), C.byref(prm)
    info, rows = p(buf), p(buf, 256)
    ok = lambda *a: call(m._h, *a)
    assert ok(X, 2, 32, None, B, None, 0, info, None) == 0
    assert ok(X, 2, 32, None, None, None, 0, info, None) == ERR_INVALID                  # NULL params
    assert ok(X, 2, 32, None, B, None, 0, None, None) == ERR_INVALID                     # NULL info
    assert ok(None, 2, 32, None, B, None, 0, info, None) == ERR_INVALID                  # NULL poses
    assert ok(X, 1 << 21, 32, None, B, None, 0, info, None) == ERR_INVALID               # K * 1024 = 2^31
    for stride in (0, 4, 16, 18, 21, 22, 23, 30):
        assert ok(X, 2, stride, None, B, None, 0, info, None) == ERR_INVALID, stride     # the stride
    assert ok(X, 2, 32, None, B, rows, 0, info, None) == ERR_INVALID                     # rows without a cap
    assert ok(X, 2, 32, None, B, None, 4, info, None) == ERR_INVALID                     # a cap without rows
    assert ok(X, 2, 32, None, B, None, 0, p(buf, 8), None) == ERR_INVALID                # info not aligned to 16
    assert ok(p(d_poses, 2), 1, 32, None, B, None, 0, info, None) == ERR_INVALID         # poses not aligned
    assert ok(X, 2, 32, None, B, p(buf, 258), 4, info, None) == ERR_INVALID              # rows not aligned
    torch.cuda.synchronize()
    buf.zero_()
    assert ok(X, 0, 32, None, B, None, 0, info, None) == 0                               # nothing to do
    assert ok(None, 0, 20, None, B, None, 0, info, None) == 0
    assert call(None, X, 2, 32, None, B, None, 0, info, None) == ERR_INVALID
    assert m._L.gndt_footprint_poses(None, None, 1, 20, None, B, None, 0, None) == ERR_INVALID
    torch.cuda.synchronize()
    assert not buf.any()                                                                 # K = 0 wrote nothing
    # no finished build
    e = g.TwoDmap(0.5, 0.25)
    e.setCloudFirst((0.0, 0.0, 0.0))
    with pytest.raises(g.GndtError) as err:
        e.footprints(dev(poses), 1.2, 0.6)
    assert err.value.code == ERR_INVALID
    with pytest.raises(ValueError):
        m.footprints(dev(poses[:, :3]), 1.2, 0.6)                                       # neither a vector nor a yaw
    # a capturing stream: refused, and the capture goes on
    st = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    x = torch.zeros(16, device="cuda")
    with g.graph_capture(graph, stream=st):
        rc = call(m._h, X, 2, 32, None, B, None, 0, info, C.c_void_p(st.cuda_stream))
        x.add_(1.0)
    assert rc == ERR_INVALID
    graph.replay()
    torch.cuda.synchronize()
    assert float(x[0]) == 1.0
    check(m, t, poses, 1.2, 0.6, "after the refused capture")


# ---- the poisoned tier -----------------------------------------------------------------------------------------------------------------

# This file's tests on memory that does not start out as zeros (tests/test_gpu_poisoned.py describes the variant, the bytes and the
# rule): one child a byte, one at a time.  measured_s: the whole child (interpreter start to exit) on the MI355X under the regular
# library; limit_s: three times that, rounded up to 10 s.
POISON_IDS = ["test_every_box_size_both_weights_and_a_band[1]", "test_every_box_size_both_weights_and_a_band[4]",
              "test_every_box_size_both_weights_and_a_band[15]", "test_wavefront_and_workgroup_edges_of_K[5]",
              "test_row_caps_around_support", "test_a_mixed_batch_alone_permuted_and_twice",
              "test_first_builder_of_the_column_index_a_large_host_call_then_a_small_one", "test_after_an_update_a_crop_a_clear_and_a_flood"]
HERE = "tests/test_gpu_footprint.py::"
GROUP = dict(measured_s=4.47, limit_s=20, ids=[HERE + i for i in POISON_IDS])


def test_every_node_id_of_the_poison_group_is_collected():
    poison_tier.ids_collected(GROUP["ids"])


def test_the_poison_limit_is_three_times_the_measured_time():
    poison_tier.limit_follows_rule(GROUP["measured_s"], GROUP["limit_s"])


@poison_tier.refused_under_variant
@pytest.mark.parametrize("byte", poison_tier.BYTES, ids=poison_tier.BYTE_IDS)
def test_footprints_under_poison(byte):
    poison_tier.run_group("the footprints", GROUP["ids"], GROUP["limit_s"], byte)
