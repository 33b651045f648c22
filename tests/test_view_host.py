"""CPU tier: view gain's per-ray code and marking (grid_ndt_amd/csrc/gndt_view.hpp on gndt_cast.hpp's walk), compiled with g++ into
tests/_view_shim.so, against a hand-derived case on the unit lattice and, field for field, against the restatement of the definition
with sets (tests/view_ref.py) on a map the oracle builds; the set semantics; the window's sizes; and the product entry points refuse to
run without a GPU."""
import ctypes as C

import numpy as np
import pytest

from grid_ndt_amd import scenes
from tests import cast_ref as cf
from tests import view_ref as vr
from tests.host_emulation import MAP, HostMap, load_shim

_shim = None


def shim():
    global _shim
    if _shim is None:
        vp, f, u32, d = C.c_void_p, C.c_float, C.c_uint32, C.c_double
        _shim = load_shim("view_shim.cpp", "_view_shim.so", {
            "viewshim_window": ([f, f, vp], None),
            "viewshim_gain": ([vp, u32, vp, u32, u32, MAP, u32, f, d, vp, vp, vp], C.c_int),
        })
    return _shim


def window(max_range, grid_len):
    """-> reach, words of a bitmap, LDS bytes of the launch, the largest reach without a grant, the largest with one"""
    out = np.zeros(5, np.uint64)
    shim().viewshim_window(max_range, grid_len, out.ctypes.data)
    return tuple(int(v) for v in out)


def host_gain(m, poses, dirs, max_range, min_count=0, min_range=0.0, per_ray=True):
    """view_one over every ray of every pose on a HostMap, as k_view_gain's threads run it -> (records, row [K, N], range [K, N])"""
    T = vr.as_poses(poses)
    d = np.ascontiguousarray(dirs, np.float32)
    K, n = len(T), len(d)
    info = np.frombuffer(b"\xa5" * (48 * max(K, 1)), vr.INFO_DTYPE).copy()       # (every field is written by the record)
    row = np.full((K, n), 0xDEADBEEF, np.uint32)
    rng = np.full((K, n), -1.0, np.float32)
    rc = shim().viewshim_gain(T.ctypes.data, K, d.ctypes.data, d.shape[1], n, m.shim_map(), min_count if min_count else 1,
                              max_range, float(np.float32(min_range)), info.ctypes.data, row.ctypes.data if per_ray else None,
                              rng.ctypes.data if per_ray else None)
    assert rc == 0
    return info[:K], row.view(np.int32).astype(np.int64), rng


def ref_trace(m, poses, dirs, max_range, **kw):
    return vr.trace(m.cells, m.origin, m.P["grid_len"], m.P["z_len"], poses, dirs, max_range, **kw)


def pose(t, yaw=0.0):
    c, s = np.cos(yaw), np.sin(yaw)
    return np.array([c, -s, 0, t[0], s, c, 0, t[1], 0, 0, 1, t[2]], np.float64)


def rec(r):
    return {k: int(r[k]) for k in vr.FIELDS}


# ---- 1. the hand case on the unit lattice (map origin 0, grid_len = z_len = 1) ----
#
# A floor of 81 columns, cells c(sx), c(sy) in [0, 8], one node each at level 1 (z in (0, 1]).  The sensor stands at (4.5, 4.5, 1.5), in
# cell (4, 4) at level 2, with the identity rotation; max_range 10, so reach = ceil(10 / 1) + 1 = 11 and W = 23.  Four rays along +x, -x,
# +y, -y at z = 1.5: level 2 all the way, so no floor node (level 1) stops them.
#   +x ends at x = 14.5, cell 14: cells 4 .. 14 are 11 columns, 4 .. 8 in the map (5 known), 9 .. 14 not (6 unknown, sum of cells 69).
#   -x ends at x = -5.5, cell -6: cells 4 .. -6 are 11 columns, 4 .. 0 known (5), -1 .. -6 unknown (6, sum -21).
#   +y and -y the same with x and y swapped; the unknown columns of a ray along x all have the other coordinate's cell 4 (6 * 4 = 24).
# rays 4, hits 0, steps 44; known 4 * 5 - 3 = 17 (the origin's column is every ray's first); unknown 24;
# sum_ux = 69 - 21 + 24 + 24 = 96 = sum_uy.
# One more node at cell (6, 4), level 2 (z in (1, 2]): the +x ray enters that voxel at x = 6, range 1.5, and stops, having seen cells
# 4, 5, 6 (3 known).  hits 1, steps 44 - 11 + 3 = 36, known 17 - 2 = 15 (cells 7 and 8 of the row are not seen), unknown 24 - 6 = 18,
# sum_ux = 96 - 69 = 27, sum_uy = 96 - 24 = 72.

UNIT = dict(grid_len=1.0, z_len=1.0, slope_interval=0.08)
HAND_POSE = pose((4.5, 4.5, 1.5))
HAND_DIRS = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0]], np.float32)
HAND_OPEN = dict(rays=4, skipped=0, hits=0, unknown=24, known=17, status=0, steps=44, sum_ux=96, sum_uy=96)
HAND_WALL = dict(rays=4, skipped=0, hits=1, unknown=18, known=15, status=0, steps=36, sum_ux=27, sum_uy=72)


def hand_cloud(wall):
    """the origin row, the 81 floor points and, with `wall`, the point in cell (6, 4) at level 2"""
    g = np.arange(9, dtype=np.float32) + np.float32(0.5)
    floor = np.stack([np.repeat(g, 9), np.tile(g, 9), np.full(81, 0.5, np.float32)], 1)
    extra = [np.array([[6.5, 4.5, 1.5]], np.float32)] if wall else []
    return np.concatenate([np.zeros((1, 3), np.float32), floor] + extra).astype(np.float32)


@pytest.mark.parametrize("wall", [False, True])
def test_the_hand_case(wall):
    m = HostMap(hand_cloud(wall), UNIT)
    assert m.n == 81 + wall and window(10.0, 1.0)[:2] == (11, (23 * 23 + 31) // 32)
    info, row, rng = host_gain(m, HAND_POSE, HAND_DIRS, 10.0)
    assert rec(info[0]) == (HAND_WALL if wall else HAND_OPEN)
    tr = ref_trace(m, HAND_POSE, HAND_DIRS, 10.0)
    assert rec(vr.gain(tr)[0]) == rec(info[0])
    if wall:
        assert rng[0, 0] == 1.5 and (m.sx[row[0, 0]], m.sy[row[0, 0]], m.sz[row[0, 0]]) == (7, 5, 2)
        assert (row[0, 1:] == cf.NO_ROW).all() and np.isinf(rng[0, 1:]).all()
    else:
        assert (row[0] == cf.NO_ROW).all() and np.isinf(rng[0]).all()
    # every visit of the +x ray, as the restatement saw it
    a, b = tr["start"][0], tr["start"][1]
    assert list(zip(tr["sx"][a:b].tolist(), tr["sy"][a:b].tolist())) == [(c + 1, 5) for c in range(4, 7 if wall else 15)]


def test_a_pose_without_a_key_or_off_the_map():
    m = HostMap(hand_cloud(False), UNIT)
    poses = np.stack([pose((np.nan, 4.5, 1.5)), pose((4.5, 1e9, 1.5)), pose((40.5, 40.5, 1.5)), HAND_POSE])
    info, row, rng = host_gain(m, poses, HAND_DIRS, 10.0)
    for k in (0, 1):
        assert rec(info[k]) == dict(rays=0, skipped=4, hits=0, unknown=0, known=0, status=1, steps=0, sum_ux=0, sum_uy=0)
        assert (row[k] == cf.NO_ROW).all() and np.isnan(rng[k]).all()
    # wholly outside the map: 4 * 11 - 3 distinct columns, all unknown
    assert rec(info[2]) == dict(rays=4, skipped=0, hits=0, unknown=41, known=0, status=0, steps=44, sum_ux=41 * 40, sum_uy=41 * 40)
    assert rec(info[3]) == HAND_OPEN
    vr.assert_same(info, vr.gain(ref_trace(m, poses, HAND_DIRS, 10.0)))


# ---- 2. the terrain map of tests/test_cast_host.py: a fan of 257 rays from 7 poses ----

_scene = None


def terrain():
    """-> HostMap, poses [7, 12] (four yaws at the scan's sensor, one tilted, one far outside the map, one with a NaN translation),
    directions [257, 3] (a fan towards the ground and the horizon, every fourth ray skyward, a few NaN), the trace"""
    global _scene
    if _scene is None:
        P = scenes.TERRAIN_PARAMS
        frames = scenes.terrain_frames(2, points_per_frame=16_384)
        px, py = scenes._pose_xy(np.int64(1), 200.0, 14.0)
        s = (px, py, float(np.median(frames[16_384:, 2])) + 1.8)
        m = HostMap(frames, P)
        rng = np.random.default_rng(31)
        d = rng.normal(size=(257, 3))
        d[:, 2] = -np.abs(d[:, 2]) * 0.3 - 0.05
        d[::4, 2] = np.abs(d[::4, 2]) + 0.5
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        d = d.astype(np.float32)
        d[5::61] = np.nan
        ry = np.array([[np.cos(0.2), 0, np.sin(0.2)], [0, 1, 0], [-np.sin(0.2), 0, np.cos(0.2)]])
        tilt = np.concatenate([pose(s, 0.4).reshape(3, 4)[:, :3] @ ry, np.array(s, np.float64)[:, None]], 1).reshape(12)
        poses = np.stack([pose(s, y) for y in (0.0, 1.3, 2.9, 4.4)] + [tilt, pose((s[0] + 500.0, s[1], s[2])), pose((s[0], np.nan, s[2]))])
        _scene = (m, poses, d, ref_trace(m, poses, d, 6.0))
    return _scene


def test_records_and_rays_equal_the_restatement_on_an_oracle_map():
    m, poses, d, tr = terrain()
    assert m.n == 3002
    want = vr.gain(tr)
    st = tr["status"]
    assert (st[:5] == cf.HIT).sum() > 100 and (st[:5] == cf.MISS).sum() > 100 and (st[:5] == cf.SKIPPED).sum() >= 5 * 4
    assert (want["unknown"][:5] > 50).all() and (want["known"][:5] > 50).all() and want["known"][5] == 0 and want["unknown"][5] > 50
    assert want["status"].tolist() == [0, 0, 0, 0, 0, 0, 1]
    info, row, rng = host_gain(m, poses, d, 6.0)
    vr.assert_same(info, want)
    assert np.array_equal(row, tr["row"]) and np.array_equal(rng.view(np.uint32), tr["range"].view(np.uint32))
    # stride 16, no per-ray outputs
    d4 = np.concatenate([d, np.full((len(d), 1), 7.0, np.float32)], 1)
    vr.assert_same(host_gain(m, poses, d4, 6.0, per_ray=False)[0], want, "stride 16")
    # the parameters of the cast: nodes of fewer points and nearer ones do not stop a ray
    for kw in (dict(min_count=5), dict(min_range=2.5), dict(min_count=3, min_range=1.0)):
        t2 = ref_trace(m, poses, d, 6.0, **kw)
        w2 = vr.gain(t2)
        assert not np.array_equal(w2["steps"], want["steps"]), kw
        vr.assert_same(host_gain(m, poses, d, 6.0, **kw)[0], w2, kw)
    # another range: another window
    t3 = ref_trace(m, poses[:3], d[:65], 2.3)
    vr.assert_same(host_gain(m, poses[:3], d[:65], 2.3)[0], vr.gain(t3), "2.3 m")


def test_the_record_is_a_set_of_columns():
    m, poses, d, tr = terrain()
    base = vr.gain(tr)
    perm = np.random.default_rng(5).permutation(len(d))
    info, _, _ = host_gain(m, poses, d[perm], 6.0)
    vr.assert_same(info, base, "permuted")
    vr.assert_same(vr.gain(tr, dirs=perm), base, "permuted, restated")
    info3, _, _ = host_gain(m, poses, np.concatenate([d, d, d]), 6.0)
    vr.assert_same(info3, vr.gain(tr, dirs=np.tile(np.arange(len(d)), 3)), "three times")
    for k in vr.FIELDS:
        f = 3 if k in ("rays", "skipped", "hits", "steps") else 1
        assert np.array_equal(info3[k].astype(np.int64), f * base[k].astype(np.int64)), k
    # a pose given twice
    twice, _, _ = host_gain(m, poses[[1, 0, 1]], d, 6.0)
    assert twice[0] == twice[2] and twice[0] == base[1] and twice[1] == base[0]


def test_the_window_sizes():
    # reach = ceil(max_range / grid_len) + 1; two bitmaps of (2 reach + 1)^2 bits and a tail of 1024 bytes in 64 KiB / 160 KiB of LDS
    assert window(10.0, 1.0)[0] == 11 and window(0.5, 1.0)[0] == 2 and window(30.0, 0.2)[0] == 151 and window(1.0, 1.0)[0] == 2
    for mr, g in ((10.0, 1.0), (30.0, 0.2), (7.3, 0.25)):
        reach, words, lds, small, large = window(mr, g)
        W = 2 * reach + 1
        assert words == -(-W * W // 32) and lds == 8 * words + 1024
    small, large = window(1.0, 1.0)[3:]
    fits = lambda r, room: 8 * -(-(2 * r + 1) ** 2 // 32) + 1024 <= room
    assert fits(small, 64 << 10) and not fits(small + 1, 64 << 10) and fits(large, 160 << 10) and not fits(large + 1, 160 << 10)
    assert (small, large) == (253, 403)


# ---- 3. no CPU path ----

def test_no_cpu_fallback_for_view_gain(native_lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import grid_ndt_amd as g
    m = g.TwoDmap(0.5, 0.5)
    m.setCloudFirst((0, 0, 0))
    with pytest.raises(g.GndtError) as e:
        m.view_gain(HAND_POSE, HAND_DIRS, 10.0, host=True)
    assert e.value.code == 2   # GNDT_ERR_NO_DEVICE
    from grid_ndt_amd import _lib
    L = _lib.lib()
    assert L.gndt_view_gain(None, None, 0, None, 0, 12, None, None, None, None) == 1
    assert L.gndt_view_gain_device(None, None, 0, None, 0, 12, None, None, None, None, None) == 1
