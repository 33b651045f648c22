"""CPU tier: scan scoring's per-element code (grid_ndt_amd/csrc/gndt_score.hpp: score_transform, score_node, score_point, and the
kernels' fixed summation tree restated in tests/score_shim.cpp), compiled with g++ into tests/_score_shim.so, against the numpy
restatement of the definition (tests/score_ref.py) on maps the oracle builds; and the product entry points refuse to run without a
GPU.

Tolerances (derived, not tuned): q, keys, rows, matched and terms are exact; d2, score and
d2_sum agree to rtol 1e-9 (fp64 arithmetic on bit-identical inputs, condition number of A at most 301: a few tens of ulps x 301 is about
1e-12; sums of non-negative terms add at most n 2^-53); the per-point d2 is fp32: the reference rounded to fp32, within 1 ulp of fp32."""
import ctypes as C
import math

import numpy as np
import pytest

from grid_ndt_amd import scenes
from tests import query_ref as qr
from tests import score_ref as sr
from tests.host_emulation import MAP, HostMap, load_shim

_shim = None


def shim():
    global _shim
    if _shim is None:
        vp, f, u32, u64, d = C.c_void_p, C.c_float, C.c_uint32, C.c_uint64, C.c_double
        _shim = load_shim("score_shim.cpp", "_score_shim.so", {
            "sshim_transform": ([vp, vp, u32, u64, vp], None),
            "sshim_score": ([C.c_int, vp, u32, u64, vp, u32, MAP, u32, d, d, d, u32] + [vp] * 5, C.c_int),
        })
    return _shim


def _face_scene():
    P = dict(grid_len=0.5, z_len=0.25, slope_interval=0.08)
    return qr.face_lattice(grid_len=P["grid_len"], z_len=P["z_len"]), P


SCENES = {
    "bridge_ground": lambda: (scenes.bridge_ground(), scenes.BRIDGE_PARAMS),
    "uniform_box": lambda: (scenes.uniform_box(40_001, half_xy=6.0, half_z=1.0), dict(grid_len=0.5, z_len=0.5, slope_interval=0.08)),
    "face_lattice": _face_scene,
}
_maps = {}


def _map(name):
    if name not in _maps:
        cloud, P = SCENES[name]()
        _maps[name] = (cloud, HostMap(cloud, P))
    return _maps[name]


def host_score(m, pts, poses, nbh=1, per_point=None, **params):
    """score_point over every (point, pose) pair on a HostMap, summed in the kernels' tree -> the dict TwoDmap.score_poses returns,
    with per_point=k also pt_terms / pt_d2_sum (a point's own sums)"""
    prm = sr.defaults(**params)
    pts = np.ascontiguousarray(pts, np.float32)
    T = np.ascontiguousarray(sr.as_poses(poses)).reshape(-1, 12)
    K, n = T.shape[0], pts.shape[0]
    rec = np.zeros((K, 4), np.int64)
    d2 = np.full(n, -1.0, np.float32)
    row = np.full(n, 0xDEADBEEF, np.uint32)
    pt_terms = np.zeros(n, np.uint32)
    pt_d2 = np.zeros(n, np.float64)
    want = per_point is not None
    p = lambda a: C.c_void_p(a.ctypes.data if want else 0)
    rc = shim().sshim_score(nbh, pts.ctypes.data, pts.shape[1], n, T.ctypes.data, K, m.shim_map(), prm["min_count"], prm["cov_rel"],
                            prm["cov_floor"], prm["max_d2"], per_point if want else 0xFFFFFFFF, rec.ctypes.data, p(d2), p(row),
                            p(pt_terms), p(pt_d2))
    assert rc == 0
    fl = rec.view(np.float64)
    out = {"score": fl[:, 0].copy(), "d2_sum": fl[:, 1].copy(), "matched": rec[:, 2].copy(), "terms": rec[:, 3].copy()}
    if want:
        out.update(d2=d2, row=row.view(np.int32).astype(np.int64), pt_terms=pt_terms, pt_d2_sum=pt_d2)
    return out


def ref_score(m, pts, poses, nbh=1, per_point=None, **params):
    return sr.score(m.cells, m.origin, m.P["grid_len"], m.P["z_len"], pts, poses, nbh, per_point, **params)


def yaw(deg, t=(0.0, 0.0, 0.0)):
    a = math.radians(deg)
    return np.array([[math.cos(a), -math.sin(a), 0, t[0]], [math.sin(a), math.cos(a), 0, t[1]], [0, 0, 1, t[2]]], np.float64)


def five_poses(P):
    """identity; +0.3 cell in x; +0.3 level in z; yaw 2 degrees; a matrix that is no rotation (scale and shear)"""
    odd = np.array([[1.01, 0.02, 0.0, 0.05], [-0.03, 0.98, 0.01, -0.02], [0.0, 0.01, 1.02, 0.01]], np.float64)
    return np.stack([yaw(0), yaw(0, (0.3 * P["grid_len"], 0, 0)), yaw(0, (0, 0, 0.3 * P["z_len"])), yaw(2.0), odd])


# ---- 1. the transform ----

def test_transform_equals_numpy_bit_for_bit():
    rng = np.random.default_rng(5)
    pts = rng.uniform(-300, 300, size=(20_000, 4)).astype(np.float32)
    poses = [yaw(0), yaw(37.0, (1e4, -1e4, 12.5)), yaw(-121.0, (0.1, 0.2, -0.3)),
             rng.normal(size=(3, 4)), rng.normal(size=(3, 4)) * np.array([1, 1, 1, 1e4])]         # the last two: R is no rotation
    qa, qb = rng.normal(size=4), rng.normal(size=4)                                                # a random rotation (quaternion)
    w, x, y, z = qa / np.linalg.norm(qa)
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    poses.append(np.concatenate([R, 100 * qb[:3, None]], 1))
    for T in poses:
        T = np.ascontiguousarray(T, np.float64)
        got = np.zeros((len(pts), 3), np.float32)
        shim().sshim_transform(T.ctypes.data, pts.ctypes.data, pts.shape[1], len(pts), got.ctypes.data)
        want = sr.transform(T, pts)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---- 2. identity, DIRECT1: the row of every point is the NODE query's, where that node has enough points ----

@pytest.mark.parametrize("name", sorted(SCENES))
def test_identity_rows_are_the_node_querys(name):
    cloud, m = _map(name)
    body = cloud[1:, :3]
    lo, hi = body.min(0), body.max(0)
    rnd = np.random.default_rng(3).uniform(lo - 1.0, hi + 1.0, size=(20_000, 3)).astype(np.float32)
    odd = qr.odd_points(m.origin, m.P["grid_len"], m.P["z_len"], (float(lo.min()), float(hi.max())))
    pts = np.concatenate([body, rnd, odd]).astype(np.float32)
    node = qr.node_rows(m.cells, pts, m.origin, m.P["grid_len"], m.P["z_len"])
    count = np.asarray(m.cells["count"]).astype(np.int64)
    for min_count in (0, 5):
        mc = sr.defaults(min_count=min_count)["min_count"]
        want = np.where((node >= 0) & (count[np.maximum(node, 0)] >= mc), node, sr.NO_ROW)
        got = host_score(m, pts, yaw(0), 1, per_point=0, min_count=min_count)
        assert np.array_equal(got["row"], want), np.flatnonzero(got["row"] != want)[:10]
        assert int(got["matched"][0]) == int(got["terms"][0]) == int((want >= 0).sum())
        assert np.array_equal(np.isinf(got["d2"]), want < 0)
    assert (want >= 0).sum() > 100          # (the case is not empty)


# ---- 3. d2, sums, matched, terms against the restatement ----

@pytest.mark.parametrize("nbh", [1, 7])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_scores_equal_the_restatement(name, nbh):
    cloud, m = _map(name)
    scan = np.ascontiguousarray(cloud[1:][::3])
    poses = five_poses(m.P)
    want = ref_score(m, scan, poses, nbh)
    assert want["terms"][0] > 100 and (want["terms"] > 0).all()
    for k in (0, 3, 4):
        got = host_score(m, scan, poses, nbh, per_point=k)
        sr.assert_pose_sums(got, want, what=(name, nbh))
        sr.assert_per_point(got["d2"], got["row"], want["poses_out"][k], what=(name, nbh, k))
        # every point's own sums: its terms exactly, their d2 at rtol
        wp = want["poses_out"][k]
        valid = wp["all_rows"] != sr.NO_ROW
        assert np.array_equal(got["pt_terms"], valid.sum(1))
        wsum = np.where(valid, wp["all_d2"], 0.0).sum(1)
        assert np.all(np.abs(got["pt_d2_sum"] - wsum) <= sr.RTOL * np.abs(wsum))


# ---- 4. DIRECT7 across index 0 on every axis: the candidates are the seven keys, found by brute force ----

def _scalar_key(p, o, length, limit):
    """one axis of the codec in Python floats of float32 values: ceil(|p - o| / len), 0 -> 1, the sign of p - o"""
    c = math.ceil(float(np.float32(abs(np.float32(np.float32(p) - np.float32(o)))) / np.float32(length)))
    n = max(int(c), 1)
    assert n <= limit
    return n if np.float32(p) > np.float32(o) else -n


def test_direct7_candidates_across_the_origin_by_brute_force():
    P = dict(grid_len=0.5, z_len=0.25, slope_interval=0.08)
    rng = np.random.default_rng(17)
    o = np.array([0.2, -0.1, 0.05], np.float32)
    body = (o + rng.uniform(-1, 1, size=(6000, 3)) * np.array([2.2, 2.2, 1.1])).astype(np.float32)     # +-4.4 cells around the origin
    cloud = np.concatenate([o[None], body]).astype(np.float32)
    m = HostMap(cloud, P)
    cells = m.cells
    node_of = {(int(x), int(y), int(z)): r for r, (x, y, z) in enumerate(zip(cells["sx"], cells["sy"], cells["sz"]))}
    assert {np.sign(k[a]) for k in node_of for a in range(3)} == {-1, 1}
    scan = (o + rng.uniform(-1, 1, size=(1500, 3)) * np.array([2.6, 2.6, 1.3])).astype(np.float32)
    prm = sr.defaults()
    nodes = sr.Nodes(cells)

    def step(v, d):
        return v + d if v + d != 0 else v + 2 * d

    cand = np.full((len(scan), 7), sr.NO_ROW, np.int64)
    for i, p in enumerate(scan):
        sx = _scalar_key(p[0], o[0], P["grid_len"], qr.MAX_XY)
        sy = _scalar_key(p[1], o[1], P["grid_len"], qr.MAX_XY)
        sz = _scalar_key(p[2], o[2], P["z_len"], qr.MAX_Z)
        seven = [(sx, sy, sz), (step(sx, -1), sy, sz), (step(sx, 1), sy, sz), (sx, step(sy, -1), sz), (sx, step(sy, 1), sz),
                 (sx, sy, step(sz, 1)), (sx, sy, step(sz, -1))]
        assert all(0 not in k for k in seven) and len(set(seven)) == 7
        for j, k in enumerate(seven):
            # brute force: every row of the map compared with the key
            hit = np.flatnonzero((cells["sx"] == k[0]) & (cells["sy"] == k[1]) & (cells["sz"] == k[2]))
            assert hit.size <= 1
            if hit.size and cells["count"][hit[0]] >= prm["min_count"]:
                cand[i, j] = hit[0]
    crossing = sum(1 for i in range(len(scan)) if (cand[i] >= 0).sum() >= 2)
    assert crossing > 500
    got = host_score(m, scan, yaw(0), 7, per_point=0)
    assert np.array_equal(got["pt_terms"], (cand >= 0).sum(1))
    d2 = np.stack([sr.d2_of(nodes, cand[:, j], scan, prm)[0] for j in range(7)], 1)
    wsum = np.where(cand >= 0, d2, 0.0).sum(1)
    assert np.all(np.abs(got["pt_d2_sum"] - wsum) <= sr.RTOL * np.abs(wsum))
    # the nearest candidate is one of the seven, and the restatement agrees with the brute force as well
    best = np.where((cand >= 0).any(1), cand[np.arange(len(scan)), np.argmin(d2, 1)], sr.NO_ROW)
    assert np.array_equal(got["row"], best)
    want = ref_score(m, scan, yaw(0), 7, per_point=0)
    assert np.array_equal(np.sort(want["poses_out"][0]["all_rows"], 1), np.sort(cand, 1))
    sr.assert_pose_sums(got, want)


# ---- 5. a rank-1 node, the max_d2 gate, NaN points and poses ----

def test_rank1_node_gate_and_nan():
    P = dict(grid_len=0.5, z_len=0.5, slope_interval=0.08)
    o = np.zeros(3, np.float32)
    line = np.array([[0.1, 0.1, 0.1], [0.2, 0.2, 0.2], [0.3, 0.3, 0.3]], np.float32)               # one cell, collinear: rank-1 scatter
    blob = (np.array([0.75, 0.25, 0.25]) + np.random.default_rng(2).normal(scale=0.05, size=(50, 3))).astype(np.float32)
    m = HostMap(np.concatenate([o[None], line, blob]).astype(np.float32), P)
    r1 = [r for r in range(m.n) if m.cells["count"][r] == 3]
    assert len(r1) == 1 and np.linalg.matrix_rank(np.array([[m.cells["cov"][r1[0]][k] for k in row] for row in ((0, 1, 2), (1, 3, 4), (2, 4, 5))]), tol=1e-9) == 1
    scan = np.array([[0.2, 0.2, 0.2], [0.15, 0.3, 0.1], [0.4, 0.05, 0.45], [0.75, 0.25, 0.25], [0.9, 0.4, 0.1],
                     [np.nan, 0.2, 0.2], [0.2, np.inf, 0.2], [30.0, 30.0, 30.0]], np.float32)
    bad = yaw(0)
    bad[1, 2] = np.nan
    poses = np.stack([yaw(0), bad])
    got = host_score(m, scan, poses, 1, per_point=0)
    want = ref_score(m, scan, poses, 1, per_point=0)
    sr.assert_pose_sums(got, want)
    sr.assert_per_point(got["d2"], got["row"], want)
    assert np.array_equal(got["row"][:3], [r1[0]] * 3) and np.isfinite(got["d2"][:5]).all() and (got["d2"][:5] >= 0).all()
    assert got["d2"][0] < 1e-6 and got["d2"][2] > 10.0         # on the line's mean; off the line (only eps wide there)
    assert (got["row"][5:] == sr.NO_ROW).all() and np.isinf(got["d2"][5:]).all()
    assert int(got["matched"][0]) == 5
    # the pose with a NaN: nothing, and no error
    assert got["score"][1] == 0.0 and got["d2_sum"][1] == 0.0 and got["matched"][1] == 0 and got["terms"][1] == 0
    # the gate: what lies beyond max_d2 does not count (the case keeps clear of the gate itself)
    gate = 4.0
    assert sr.gate_margin(want["poses_out"], gate) > 1e-6
    g2 = host_score(m, scan, poses, 1, per_point=0, max_d2=gate)
    w2 = ref_score(m, scan, poses, 1, per_point=0, max_d2=gate)
    sr.assert_pose_sums(g2, w2)
    sr.assert_per_point(g2["d2"], g2["row"], w2)
    kept = want["d2"] <= gate
    assert 0 < kept.sum() < 5 and int(g2["terms"][0]) == int(kept.sum()) and np.array_equal(g2["row"] >= 0, kept)
    assert float(g2["d2"][np.isfinite(g2["d2"])].max()) <= gate


def test_pose_arguments_of_the_python_method():
    """TwoDmap.score_poses takes [K, 3, 4], [K, 4, 4] (last row dropped) or one matrix, any float dtype -> contiguous float64 [K, 12]"""
    import grid_ndt_amd as g
    T = np.random.default_rng(1).normal(size=(5, 3, 4))
    want = T.reshape(5, 12)
    T44 = np.concatenate([T, np.tile([[[0, 0, 0, 1.0]]], (5, 1, 1))], 1)
    for arg in (T, T44, T44[:, ::1].copy(order="F")):
        got = g.TwoDmap._as_poses(arg)
        assert got.dtype == np.float64 and got.flags.c_contiguous and np.array_equal(got, want)
    assert np.array_equal(g.TwoDmap._as_poses(T[2]), want[2:3]) and np.array_equal(g.TwoDmap._as_poses(T44[2]), want[2:3])
    f32 = g.TwoDmap._as_poses(T.astype(np.float32))
    assert f32.dtype == np.float64 and np.array_equal(f32, T.astype(np.float32).astype(np.float64).reshape(5, 12))
    for bad in (np.zeros((5, 4, 3)), np.zeros((5, 12)), np.zeros(12), np.zeros((2, 5, 3, 4))):
        with pytest.raises(ValueError):
            g.TwoDmap._as_poses(bad)


# ---- 6. no CPU path ----

def test_no_cpu_fallback_for_scores(native_lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import grid_ndt_amd as g
    m = g.TwoDmap(0.5, 0.5)
    m.setCloudFirst((0, 0, 0))
    with pytest.raises(g.GndtError) as e:
        m.score_poses(np.ones((4, 3), np.float32), np.eye(4))
    assert e.value.code == 2   # GNDT_ERR_NO_DEVICE
    # both entry points, called directly: a null handle is invalid
    L = native_lib
    assert L.gndt_score_poses(None, None, 0, 12, None, 0, None, None, None, None) == 1
    assert L.gndt_score_poses_device(None, None, 0, 12, None, 0, None, None, None, None, None) == 1
