"""CPU tier: ray casting's per-ray code (grid_ndt_amd/csrc/gndt_cast.hpp on gndt_ray.hpp's walk and gndt_score.hpp's cofactors), compiled
with g++ into tests/_cast_shim.so, against hand-derived answers on the unit lattice and, bit for bit, against the numpy restatement of
the definition (tests/cast_ref.py) on maps the oracle builds; and the product entry points refuse to run without a GPU."""
import ctypes as C
import math

import numpy as np
import pytest

from grid_ndt_amd import scenes
from tests import cast_ref as cf
from tests.host_emulation import MAP, HostMap, load_shim

VOXEL, NDT = cf.VOXEL, cf.NDT
_shim = None


def shim():
    global _shim
    if _shim is None:
        vp, f, i32, u32, u64, d = C.c_void_p, C.c_float, C.c_int32, C.c_uint32, C.c_uint64, C.c_double
        _shim = load_shim("cast_shim.cpp", "_cast_shim.so", {
            "castshim_walk": ([vp, f, f, vp, vp, f, vp, vp, i32], C.c_int),
            "castshim_cast": ([C.c_int, vp, u32, vp, u32, u64, MAP, u32, f, d, d, d, d] + [vp] * 4, C.c_int),
        })
    return _shim


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def host_cast(m, origins, ends, mode=VOXEL, **kw):
    """cast_one over every ray on a HostMap, as k_cast's lanes run it -> dict(row int64, range, d2 float32, stats)"""
    prm = cf.params(mode=mode, **kw)
    o, e = _f32(origins), _f32(ends)
    n = len(e)
    so = 0 if o.ndim == 1 else o.shape[1]
    row = np.full(max(n, 1), 0xDEADBEEF, np.uint32)
    rng = np.full(max(n, 1), -1.0, np.float32)
    d2 = np.full(max(n, 1), -1.0, np.float32)
    stats = np.zeros(3, np.uint64)
    rc = shim().castshim_cast(mode, o.ctypes.data, so, e.ctypes.data, e.shape[1], n, m.shim_map(), prm["min_count"], prm["max_range"],
                              prm["min_range"], prm["cov_rel"], prm["cov_floor"], prm["max_d2"], row.ctypes.data, rng.ctypes.data,
                              d2.ctypes.data, stats.ctypes.data)
    assert rc == 0
    return dict(row=row[:n].view(np.int32).astype(np.int64), range=rng[:n], d2=d2[:n],
                stats={"rays": int(stats[0]), "skipped": int(stats[1]), "hits": int(stats[2])})


def ref_cast(m, origins, ends, mode=VOXEL, **kw):
    return cf.cast(m.cells, m.origin, m.P["grid_len"], m.P["z_len"], origins, ends, mode=mode, **kw)


def both(m, origins, ends, mode=VOXEL, **kw):
    """the shim's answer, checked bit for bit against the restatement's"""
    got, want = host_cast(m, origins, ends, mode, **kw), ref_cast(m, origins, ends, mode, **kw)
    cf.assert_same(got, want, (mode, kw))
    assert got["stats"] == want["stats"]
    return got


def shim_walk(m, o, p, max_range=0.0):
    """-> [(sx, sy, lev_in, lev_out, t_in, t_out), ...] or None for a skipped ray"""
    mo, oo, pp = _f32(m.origin), _f32(o), _f32(p)
    cap = 1 << 12
    cols, ts = np.zeros((cap, 4), np.int32), np.zeros((cap, 2), np.float64)
    k = shim().castshim_walk(mo.ctypes.data, m.P["grid_len"], m.P["z_len"], oo.ctypes.data, pp.ctypes.data, max_range, cols.ctypes.data,
                             ts.ctypes.data, cap)
    if k < 0:
        return None
    assert k <= cap
    return [tuple(int(v) for v in cols[i]) + tuple(float(v) for v in ts[i]) for i in range(k)]


def ref_walk(m, o, p, max_range=0.0):
    r = cf.cast(m.cells, m.origin, m.P["grid_len"], m.P["z_len"], o, _f32(p)[None, :], max_range=max_range)
    if r["status"][0] == cf.SKIPPED:
        return None
    s = r["steps"]
    return [tuple(int(s[k][i]) for k in ("sx", "sy", "lev_in", "lev_out")) + (float(s["t_in"][i]), float(s["t_out"][i]))
            for i in range(len(s["sx"]))]


# ---- 1. hand-derived cases on the unit lattice (origin 0, lengths 1): the rows come from a tiny cloud through the oracle ----

UNIT = dict(grid_len=1.0, z_len=1.0, slope_interval=0.08)
O = (0.5, 0.5, 0.5)


def tiny(*nodes, seed=3):
    """a map of a few nodes: (centre, points, half spread) each -> (HostMap, {voxel key: row})"""
    rng = np.random.default_rng(seed)
    pts = [np.zeros((1, 3), np.float32)]
    for c, k, h in nodes:
        pts.append((np.asarray(c)[None, :] + rng.uniform(-h, h, size=(k, 3))).astype(np.float32))
    m = HostMap(np.concatenate(pts), UNIT)
    return m, {(int(a), int(b), int(c)): i for i, (a, b, c) in enumerate(zip(m.sx, m.sy, m.sz))}


def one(m, o, p, mode=VOXEL, **kw):
    r = both(m, o, _f32(p)[None, :], mode, **kw)
    return int(r["row"][0]), float(r["range"][0]), float(r["d2"][0])


def test_axis_parallel_ray_hits_where_it_enters_the_voxel():
    m, rows = tiny(((2.5, 0.5, 0.5), 4, 0.2))
    assert set(rows) == {(3, 1, 1)}
    assert one(m, O, (3.5, 0.5, 0.5)) == (rows[3, 1, 1], 1.5, 0.0)
    w = shim_walk(m, O, (3.5, 0.5, 0.5))
    assert w == ref_walk(m, O, (3.5, 0.5, 0.5))
    assert [c[:4] for c in w] == [(1, 1, 1, 1), (2, 1, 1, 1), (3, 1, 1, 1), (4, 1, 1, 1)]
    assert w[2][4:] == (0.5, 2.5 / 3.0) and w[0][4] == 0.0 and w[3][5] == 1.0
    # max_range one column short of the node: a miss; just into its column: the same hit
    assert one(m, O, (3.5, 0.5, 0.5), max_range=1.4) == (cf.NO_ROW, math.inf, math.inf)
    assert one(m, O, (3.5, 0.5, 0.5), max_range=1.6) == (rows[3, 1, 1], 1.5, 0.0)
    assert shim_walk(m, O, (3.5, 0.5, 0.5), 1.4)[-1][:2] == (2, 1)


def test_climbing_ray_takes_its_range_from_the_z_plane():
    # d = (2, 0, 3): x = 1 at t = 0.25 (z 1.25, level 2), x = 2 at t = 0.75 (z 2.75, level 3); the node sits one level above column 2's entry
    m, rows = tiny(((1.5, 0.5, 2.5), 4, 0.2))
    assert set(rows) == {(2, 1, 3)}
    row, rng, d2 = one(m, O, (2.5, 0.5, 3.5))
    assert row == rows[2, 1, 3] and d2 == 0.0
    assert rng == float(np.float32(0.5 * math.sqrt(13.0)))          # z = 2 at t = 0.5, inside [0.25, 0.75]
    w = shim_walk(m, O, (2.5, 0.5, 3.5))
    assert [c[:4] for c in w] == [(1, 1, 1, 2), (2, 1, 2, 3), (3, 1, 3, 4)] and w[1][4:] == (0.25, 0.75)
    # a node at the entry level of its column is hit at the column's t_in
    m, rows = tiny(((1.5, 0.5, 1.5), 4, 0.2))
    assert one(m, O, (2.5, 0.5, 3.5))[:2] == (rows[2, 1, 2], float(np.float32(0.25 * math.sqrt(13.0))))


def test_vertical_rays_across_level_0():
    m, rows = tiny(((0.5, 0.5, 1.5), 4, 0.2), ((0.5, 0.5, -0.5), 4, 0.2))
    assert set(rows) == {(1, 1, 2), (1, 1, -1)}
    lo, hi = (0.5, 0.5, -1.5), (0.5, 0.5, 2.5)
    assert [c[:4] for c in shim_walk(m, lo, hi)] == [(1, 1, -2, 3)]
    assert one(m, lo, hi) == (rows[1, 1, -1], 0.5, 0.0)             # up: enters level -1 through the plane -1
    assert one(m, hi, lo) == (rows[1, 1, 2], 0.5, 0.0)              # down: enters level 2 through the plane 2
    assert one(m, lo, hi, min_range=1.0) == (rows[1, 1, 2], 2.5, 0.0)       # ... the next level in visit order: plane 1
    assert one(m, hi, lo, min_range=1.0) == (rows[1, 1, -1], 2.5, 0.0)      # ... plane 0


def test_ray_across_x0():
    m, rows = tiny(((-1.5, 0.5, 0.5), 4, 0.2))
    assert set(rows) == {(-2, 1, 1)}
    assert one(m, O, (-1.5, 0.5, 0.5)) == (rows[-2, 1, 1], 1.5, 0.0)
    assert [c[:2] for c in shim_walk(m, O, (-1.5, 0.5, 0.5))] == [(1, 1), (-1, 1), (-2, 1)]


def test_zero_length_ray_inside_an_occupied_voxel():
    m, rows = tiny(((0.5, 0.5, 0.5), 4, 0.2))
    for mode in (VOXEL, NDT):
        row, rng, _ = one(m, O, O, mode)
        assert (row, rng) == (rows[1, 1, 1], 0.0)
        assert one(m, O, O, mode, min_range=0.1) == (cf.NO_ROW, math.inf, math.inf)


def test_a_nearer_node_below_min_count_is_passed_over():
    m, rows = tiny(((1.5, 0.5, 0.5), 1, 0.2), ((2.5, 0.5, 0.5), 4, 0.2))
    assert one(m, O, (3.5, 0.5, 0.5)) == (rows[2, 1, 1], 0.5, 0.0)
    assert one(m, O, (3.5, 0.5, 0.5), min_count=2) == (rows[3, 1, 1], 1.5, 0.0)
    assert one(m, O, (3.5, 0.5, 0.5), NDT)[0] == rows[3, 1, 1]       # one point: no statistics


def test_ndt_range_lies_inside_the_voxel_segment():
    m, rows = tiny(((2.8, 0.5, 0.5), 12, 0.05))                     # the mean sits off-centre, near x = 2.8
    row, rng, d2 = one(m, O, (3.5, 0.5, 0.5), NDT)
    assert row == rows[3, 1, 1]
    assert 1.5 < rng < 2.5 and abs(rng - 2.3) < 0.05
    # the ray runs through the box the points were drawn from: the mean lies within h = 0.05 of it in y and in z, a uniform box has
    # sigma = h / sqrt(3) per axis, so d2 is at most about 3 + 3; 9 is the 3-sigma gate
    assert 0.0 <= d2 < 9.0
    assert one(m, O, (3.5, 0.5, 0.5), VOXEL) == (row, 1.5, 0.0)


def test_ndt_max_d2_turns_a_grazing_ray_into_a_miss_or_the_next_node():
    # a tight cluster in a corner of voxel (3, 1, 1); the ray crosses the voxel along y = 0.1, 0.8 away from it
    m, rows = tiny(((2.5, 0.9, 0.5), 12, 0.02))
    o, p = (0.5, 0.1, 0.5), (4.5, 0.1, 0.5)
    row, rng, d2 = one(m, o, p, NDT)
    assert row == rows[3, 1, 1] and d2 > 100.0 and 1.5 <= rng <= 2.5
    assert one(m, o, p, NDT, max_d2=9.0) == (cf.NO_ROW, math.inf, math.inf)
    m, rows = tiny(((2.5, 0.9, 0.5), 12, 0.02), ((3.5, 0.1, 0.5), 12, 0.05))
    assert one(m, o, p, NDT)[0] == rows[3, 1, 1]
    row, rng, d2 = one(m, o, p, NDT, max_d2=9.0)
    assert row == rows[4, 1, 1] and d2 < 9.0 and 2.5 <= rng <= 3.5


def test_skipped_rays():
    m, _ = tiny(((2.5, 0.5, 0.5), 4, 0.2))
    good = (3.5, 0.5, 0.5)
    for bad in ((np.nan, 0.5, 0.5), (0.5, np.inf, 0.5), (0.5, 0.5, -np.inf), (1e6, 0.5, 0.5)):
        for o, p in ((O, bad), (bad, good)):
            assert shim_walk(m, o, p) is None and ref_walk(m, o, p) is None
            for mode in (VOXEL, NDT):
                r = both(m, o, _f32(p)[None, :], mode)
                assert r["row"][0] == cf.NO_ROW and np.isnan(r["range"][0]) and np.isnan(r["d2"][0])
                assert r["stats"] == {"rays": 0, "skipped": 1, "hits": 0}
    # per-ray origins, a bad one among good ones
    o = np.tile(_f32(O), (3, 1))
    o[1, 0] = np.nan
    r = both(m, o, np.tile(_f32(good), (3, 1)))
    assert r["stats"] == {"rays": 2, "skipped": 1, "hits": 2} and r["row"][1] == cf.NO_ROW


# ---- 2. the terrain map (two frames of 16 384 points): 1 024 rays past the scan's end points, a quarter lifted into the sky ----

_scene = None


def _terrain():
    """tests/test_clear_host.py's terrain map, re-stated: two frames of 16 384 points, the second frame's sensor 1.8 m over its median z"""
    P = scenes.TERRAIN_PARAMS
    frames = scenes.terrain_frames(2, points_per_frame=16_384)
    px, py = scenes._pose_xy(np.int64(1), 200.0, 14.0)
    f1 = frames[16_384:]
    sensor = (px, py, float(np.median(f1[:, 2])) + 1.8)
    return HostMap(frames, P), sensor, f1


def terrain_rays():
    global _scene
    if _scene is None:
        m, sensor, f1 = _terrain()
        s = _f32(sensor)
        p = f1[::16][:1024, :3]
        ends = (s[None, :] + np.float32(1.5) * (p - s[None, :])).astype(np.float32)
        ends[::4, 2] = s[2] + np.abs(ends[::4, 2] - s[2]) + np.float32(5.0)
        jitter = np.random.default_rng(17).uniform(-0.3, 0.3, size=ends.shape).astype(np.float32)
        _scene = (m, s, ends, (s[None, :] + jitter).astype(np.float32))
    return _scene


# (the rays that hit do so 1.9 m to 3.4 m from the sensor: ranges that cut through the middle of them)
CASES = [dict(), dict(max_range=2.5), dict(min_range=2.6), dict(min_count=5), dict(max_range=3.0, min_range=2.2, min_count=4)]
NDT_CASES = [dict(max_d2=4.0), dict(cov_rel=0.05, cov_floor=1e-4, max_d2=1.5)]


@pytest.mark.parametrize("mode", [VOXEL, NDT])
def test_shared_origin_equals_the_restatement_bit_for_bit(mode):
    m, s, ends, _ = terrain_rays()
    assert m.n == 3002
    for kw in CASES + (NDT_CASES if mode == NDT else []):
        r = both(m, s, ends, mode, **kw)
        hit = r["row"] != cf.NO_ROW
        assert hit.any() and (~hit).any(), kw                       # both branches are exercised
        assert (hit == np.isfinite(r["range"])).all() and (r["d2"][hit] >= 0).all()
    r = both(m, s, ends, mode)
    hit = r["row"] != cf.NO_ROW
    assert not hit[::4].any()                                       # the lifted quarter sees the sky
    if mode == VOXEL:
        assert 0.70 < hit.mean() < 0.80 and (r["d2"][hit] == 0).all()
    else:
        assert 0.67 < hit.mean() < 0.77
        assert (np.asarray(m.cells["count"])[r["row"][hit]] >= 3).all()
    # stride 16, and a batch with skipped rays in it
    e4 = np.concatenate([ends, np.ones((len(ends), 1), np.float32)], 1)
    cf.assert_same(host_cast(m, s, e4, mode), r)
    bad = ends.copy()
    bad[::37] = np.nan
    rb = both(m, s, bad, mode)
    assert rb["stats"]["skipped"] == len(bad[::37]) and np.isnan(rb["range"][::37]).all()


@pytest.mark.parametrize("mode", [VOXEL, NDT])
def test_per_ray_origins_equal_the_restatement_bit_for_bit(mode):
    m, s, ends, origins = terrain_rays()
    for kw in CASES[:3] + (NDT_CASES[:1] if mode == NDT else []):
        r = both(m, origins, ends, mode, **kw)
        hit = r["row"] != cf.NO_ROW
        assert hit.any() and (~hit).any(), kw
    o4 = np.concatenate([origins, np.zeros((len(origins), 1), np.float32)], 1)
    cf.assert_same(host_cast(m, o4, ends, mode), ref_cast(m, origins, ends, mode))
    # rays back towards the sensor from their ends: other octants, other entry sides
    both(m, ends, origins, mode)


def test_voxel_hits_are_voxels_the_clearing_walk_visits():
    """independent of cast_ref: every hit row is one the count-only clearing walk of the same rays passes (tests/clear_ref.py)"""
    from tests import clear_ref as cr
    m, s, ends, _ = terrain_rays()
    r = host_cast(m, s, ends, VOXEL)
    words, _, _ = cr.passes(m.cells, m.origin, m.P["grid_len"], m.P["z_len"], s, ends)
    hit = r["row"][r["row"] != cf.NO_ROW]
    assert ((words[hit] & 0x7FFFFFFF) > 0).all()
    L = np.linalg.norm(ends.astype(np.float64) - s.astype(np.float64), axis=1)
    ok = r["row"] != cf.NO_ROW
    assert (r["range"][ok].astype(np.float64) <= L[ok] * (1 + 1e-6)).all()


# ---- 3. no CPU path ----

def test_no_cpu_fallback_for_casts(native_lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import grid_ndt_amd as g
    m = g.TwoDmap(0.5, 0.5)
    m.setCloudFirst((0, 0, 0))
    ends = np.ones((4, 3), np.float32)
    for kw in ({}, {"mode": "ndt"}, {"stats": True}):
        with pytest.raises(g.GndtError) as e:
            m.cast_rays((0, 0, 1), ends, **kw)
        assert e.value.code == 2   # GNDT_ERR_NO_DEVICE
    from grid_ndt_amd import _lib
    L = _lib.lib()
    assert L.gndt_cast_rays(None, None, 0, None, 0, 12, None, None, None) == 1
    assert L.gndt_cast_rays_device(None, None, 0, None, 0, 12, None, None, None, None) == 1
