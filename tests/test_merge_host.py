"""CPU tier: the map merge's per-node code (grid_ndt_amd/csrc/gndt_merge.hpp, compiled with g++ into tests/_merge_shim.so) against the
numpy restatement (tests/merge_ref.py), bit for bit; the merged map against a build of the moved points, on the host emulation of the
pipeline; and the entry point refuses null handles.

Tolerances (derived in tests/merge_ref.py, not tuned): destination keys and the shim's nine sums bit for bit the restatement's; at map
level keys, counts, first-seen indices, the node order and the flags exact, a destination sum within j u x the sum of the absolute
values of its j addends plus the per-addend bounds of the steps, of the two accumulations and, where the moved cloud was rounded to
float32, of that rounding.  The map-level equalities hold when every source node's points key into the destination cell its mean keys
into; each test asserts that first (measured: 0 of 3 051 and 0 of 18 642 nodes violate it, in all three cases)."""
import ctypes as C

import numpy as np
import pytest

from tests import coarsen_ref as cr
from tests import host_emulation as he
from tests import merge_ref as mr
from tests.host_emulation import load_shim
from tests.test_coarsen_host import SETTINGS, fine_stats

_shim = None


def shim():
    global _shim
    if _shim is None:
        vp, f, u64 = C.c_void_p, C.c_float, C.c_uint64
        _shim = load_shim("merge_shim.cpp", "_merge_shim.so", {
            "mshim_merge": ([vp, vp, vp, u64, vp, vp, f, f, vp, f, f, vp, vp, vp], None),
        })
    return _shim


def shim_merge(keys, count, sums, pose, src_geo, dst_geo):
    keys = np.ascontiguousarray(keys, np.uint64)
    count = np.ascontiguousarray(count, np.uint32)
    sums = np.ascontiguousarray(sums, np.float64)
    T = np.ascontiguousarray(np.asarray(pose, np.float64).reshape(-1, 4)[:3])
    so, do = np.float32(src_geo[0]), np.float32(dst_geo[0])
    dkey = np.zeros(keys.size, np.uint64)
    ok = np.zeros(keys.size, np.uint8)
    out = np.zeros((keys.size, 9))
    shim().mshim_merge(keys.ctypes.data, count.ctypes.data, sums.ctypes.data, keys.size, T.ctypes.data, so.ctypes.data, src_geo[1],
                       src_geo[2], do.ctypes.data, dst_geo[1], dst_geo[2], dkey.ctypes.data, ok.ctypes.data, out.ctypes.data)
    return dkey, ok != 0, out


def rigid(yaw_deg, pitch_deg, t):
    y, p = np.radians(yaw_deg), np.radians(pitch_deg)
    Rz = np.array([[np.cos(y), -np.sin(y), 0], [np.sin(y), np.cos(y), 0], [0, 0, 1]])
    Ry = np.array([[np.cos(p), 0, np.sin(p)], [0, 1, 0], [-np.sin(p), 0, np.cos(p)]])
    return np.concatenate([Rz @ Ry, np.asarray(t, np.float64)[:, None]], 1)


def geo(setting):
    gl, zl, origin = SETTINGS[setting]
    return (np.float32(origin), gl, zl)


def random_nodes(rng, n):
    sx = rng.integers(1, 3000, n) * rng.choice([-1, 1], n)
    sy = rng.integers(1, 3000, n) * rng.choice([-1, 1], n)
    sz = rng.integers(1, 400, n) * rng.choice([-1, 1], n)
    # the keys at +-1 and at the range's ends
    sx[:8] = [1, -1, 65535, -65535, 1, -1, 1, -1]
    sy[:8] = [1, -1, 1, -1, 65535, -65535, -1, 1]
    sz[:8] = [1, -1, 1, -1, 1, -1, (1 << 21) - 1, -((1 << 21) - 1)]
    keys = cr.pack(sx, sy, sz)
    count = rng.integers(1, 100000, n).astype(np.uint32)
    count[8:16] = [1, 2, 3, 1 << 31, 0xFFFFFFFF, 1, 2, 3]
    count[:5] = [1, 2, 3, 1 << 31, 0xFFFFFFFF]
    sums = rng.normal(size=(n, 9)) * 10.0 ** rng.integers(-12, 3, size=(n, 1))
    sums[16:24] = 0.0                                              # zero sums: the mean is the centre, S = 0
    sums[5:7] = 0.0
    return keys, count, sums


def check_bits(keys, count, sums, pose, src_geo, dst_geo):
    dkey, ok, out = shim_merge(keys, count, sums, pose, src_geo, dst_geo)
    wkey, wok, wout = mr.merge_nodes(keys, count, sums, pose, src_geo, dst_geo)
    assert np.array_equal(ok, wok)
    assert np.array_equal(dkey[ok], wkey[ok])
    assert np.array_equal(out[ok].view(np.uint64), wout[ok].view(np.uint64))
    return dkey, ok, out


# ---- 1. the per-node arithmetic: the shim's bits are the restatement's ----

@pytest.mark.parametrize("setting", range(len(SETTINGS)))
def test_merge_node_equals_the_restatement_bit_for_bit(setting):
    rng = np.random.default_rng(700 + setting)
    keys, count, sums = random_nodes(rng, 50000)
    src_geo, dst_geo = geo(setting), geo((setting + 2) % len(SETTINGS))
    poses = {"identity": np.eye(4)[:3], "rigid": rigid(17.0, 4.0, (0.37, -1.21, 0.113)),
             "flip": np.concatenate([np.diag([-1.0, -1.0, 1.0]), np.zeros((3, 1))], 1),
             "not a rotation": np.concatenate([rng.normal(size=(3, 3)), rng.normal(size=(3, 1))], 1)}
    for name, pose in poses.items():
        dkey, ok, out = check_bits(keys, count, sums, pose, src_geo, dst_geo)
        print("setting", setting, name, "nodes with a key:", int(ok.sum()), "of", ok.size)
        assert ok.sum() > 0.5 * ok.size
        # the same geometry on both sides, under the identity: every key is its own
        if name == "identity":
            skey, sok, _ = check_bits(keys, count, sums, pose, src_geo, src_geo)
            small = np.abs(sums[:, :3] / count[:, None]).max(1) < 0.4 * min(src_geo[1], src_geo[2])      # the mean inside the cell
            small[:8] = False                      # (at the range's ends float32 resolves less than a cell's tenth)
            assert sok[small].all() and np.array_equal(skey[small], keys[small])


def test_a_mean_sent_out_of_range_or_to_nan_has_no_key():
    rng = np.random.default_rng(9)
    keys, count, sums = random_nodes(rng, 2000)
    g = geo(0)
    far = np.concatenate([np.eye(3), [[1e6], [0.0], [0.0]]], 1)                  # 2 000 000 cells off: beyond |sx| <= 65535
    beyond_fp32 = np.concatenate([np.eye(3), [[0.0], [1e39], [0.0]]], 1)         # finite in fp64, inf in fp32
    with_inf = np.concatenate([np.diag([np.inf, 1.0, 1.0]), np.zeros((3, 1))], 1)
    with_nan = np.concatenate([np.diag([1.0, 1.0, np.nan]), np.zeros((3, 1))], 1)
    high = np.concatenate([np.eye(3), [[0.0], [0.0], [0.2 * (1 << 21) + 100.0]]], 1)       # beyond |sz| < 2^21 at z_len 0.1, from the lowest level too
    for pose in (far, beyond_fp32, with_inf, with_nan, high):
        dkey, ok, out = check_bits(keys, count, sums, pose, g, g)
        assert not ok.any()


# ---- 2. map level: the merged statistics finalise to the map of a build of the moved points ----

def lattice_pose(o, grid_len, z_len):
    """90 degrees about z, t = o - R o + (3 grid_len, -2 grid_len, 1 z_len): cells go to cells"""
    R = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    o = np.float32(o).astype(np.float64)
    t = o - R @ o + np.array([3.0 * np.float32(grid_len), -2.0 * np.float32(grid_len), 1.0 * np.float32(z_len)], np.float64)
    return np.concatenate([R, t[:, None]], 1)


def moved_cloud(cloud, pose):
    """fl32(T p) for every point but point 0, which stays the origin"""
    T = np.asarray(pose, np.float64)
    q = cloud.copy()
    q[1:, :3] = (cloud[1:, :3].astype(np.float64) @ T[:, :3].T + T[:, 3]).astype(np.float32)
    return q


CASES = {"identity": (1, 1, False), "identity 2x": (2, 2, False), "identity 4x": (4, 4, False), "lattice": (1, 1, True)}


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("name", ["campus_frame", "uniform_box"])
def test_merged_statistics_finalise_to_the_build_of_the_moved_points(name, case):
    cloud, P, (uk, count, first, sums, cen), ab = fine_stats(name)
    fxy, fz, moved = CASES[case]
    o = cloud[0, :3]
    gl, zl = P["grid_len"], P["z_len"]
    GL, ZL = float(cr.coarse_len(gl, fxy)), float(cr.coarse_len(zl, fz))
    src_geo, dst_geo = (o, gl, zl), (o, GL, ZL)
    pose = lattice_pose(o, gl, zl) if moved else np.eye(4)[:3]
    q = moved_cloud(cloud, pose) if moved else cloud
    # the condition: every source node's points key into the one destination cell its mean keys into
    pkey, pok, _ = mr.point_keys(np.ascontiguousarray(cloud[1:, :3]), o, gl, zl)
    inv = np.searchsorted(uk, pkey)
    assert pok.all() and np.array_equal(uk[inv], pkey)
    qkey, qok, _ = mr.point_keys(np.ascontiguousarray(q[1:, :3]), o, GL, ZL)
    dkey, ok, _ = mr.merge_nodes(uk, count, sums, pose, src_geo, dst_geo)
    assert ok.all() and qok.all()
    violating = np.unique(inv[qkey != dkey[inv]]).size
    print(name, case, "nodes violating the condition:", violating, "of", uk.size)
    assert violating == 0
    src = {"key": uk, "count": count, "first_idx": first, "sums": sums}
    got = mr.merge(src, pose, src_geo, dst_geo, abs_sums=ab)
    assert got["stats"] == {"source_nodes": uk.size, "below_min_count": 0, "skipped": 0, "merged_nodes": uk.size,
                            "merged_points": len(cloud) - 1, "new_nodes": got["key"].size}
    wk, wcount, wfirst, wsums, wcen = he.accumulate(q[1:], o, GL, ZL)
    assert np.array_equal(got["key"], wk) and np.array_equal(got["count"], wcount) and np.array_equal(got["first_idx"], wfirst)
    if not moved:
        par = cr.coarsen(uk, count, first, sums, fxy, fz, o, gl, zl)
        assert np.array_equal(got["key"], par["key"]) and np.array_equal(got["count"], par["count"])
        assert np.array_equal(got["first_idx"], par["first_idx"]) and np.array_equal(got["addends"], par["children"])
        if (fxy, fz) == (1, 1):
            assert np.array_equal(got["key"], uk)
    tol = got["tol"].copy()
    if moved:
        np.add.at(tol, np.searchsorted(wk, qkey), mr.moved_cloud_bound(q[1:, :3], wcen[np.searchsorted(wk, qkey)]))
    err = np.abs(got["sums"] - wsums)
    print(name, case, "nodes", wk.size, "worst error / bound", float((err / np.maximum(tol, 1e-300)).max()))
    assert (err <= tol).all()
    a = he.finalize(got["key"], got["count"], got["first_idx"], got["sums"], wcen, P["slope_interval"])
    b = he.finalize(wk, wcount, wfirst, wsums, wcen, P["slope_interval"])
    for k in ("sx", "sy", "sz", "count", "first_idx", "flags"):
        assert np.array_equal(a[k], b[k]), k
    assert (a["num_nodes"], a["num_columns"], a["num_slopes"]) == (b["num_nodes"], b["num_columns"], b["num_slopes"])


def test_min_count_and_a_prior_map():
    """step 8 of the restatement on a hand-made case: counts add, first indices take the minimum with base + first, small nodes stay"""
    g = (np.float32([0, 0, 0]), 0.5, 0.5)
    src = {"key": cr.pack([1, 2, 3], [1, 1, 1], [1, 1, 1]), "count": np.uint32([1, 2, 5]), "first_idx": np.uint32([0, 1, 3]),
           "sums": np.zeros((3, 9))}
    prior = {"key": cr.pack([3, 9], [1, 9], [1, 9]), "count": np.uint32([4, 7]), "first_idx": np.uint32([2, 0]), "sums": np.zeros((2, 9))}
    got = mr.merge(src, None, g, g, prior=prior, min_count=3, base=11)
    assert got["stats"] == {"source_nodes": 3, "below_min_count": 2, "skipped": 0, "merged_nodes": 1, "merged_points": 5, "new_nodes": 0}
    assert np.array_equal(got["key"], np.sort(prior["key"])) and sorted(got["count"].tolist()) == [7, 9]
    assert got["first_idx"][np.flatnonzero(got["count"] == 9)[0]] == 2 and got["addends"].tolist().count(2) == 1


# ---- 3. no CPU path ----

def test_merge_refuses_null_handles(native_lib):
    assert native_lib.gndt_merge_map_device(None, None, None, None, None, None) == 1      # GNDT_ERR_INVALID
