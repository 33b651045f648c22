"""CPU tier: the fixtures of the blocked-bucket shape tests (tests/blocked_scenes.py) hold.  For every scene the oracle's map gives,
through the numpy restatement of the layout rule (blocked_scenes.plan), exactly the block shape the scene is there for — one per shape
of k_bucket_blocked — and the oracle's own map passes the parity gates on its own: a "perfect build" (the oracle's fp64 truth rounded to
float32) meets parity.compare's strict gates with no node on a widened covariance allowance and none below the input resolution, so the
GPU tier (tests/test_gpu_blocked_shapes.py) needs none of compare's escape hatches."""
import numpy as np
import pytest

from tests import blocked_scenes as bs
from tests import parity


def _check_fixture(ref, P, n, want):
    """`want`: the scene's table row.  -> the layout."""
    lay = bs.plan(ref, n)
    (x0, y0, z0), (X, Y, Z) = bs.extent(ref)
    assert lay["state"] == 1, lay
    assert Z == want["levels"]
    assert (1 << lay["shx"], 1 << lay["shy"], 1 << lay["shz"]) == want["block"], lay
    assert (lay["nx"], lay["ny"]) == want["blocks"] and lay["buckets"] == lay["nx"] * lay["ny"], lay
    assert z0 - lay["z0"] == want["zpad"] == ((1 << lay["shz"]) - Z) // 2
    assert (x0 - lay["x0"], y0 - lay["y0"]) == (1 << lay["shx"], 1 << lay["shy"])      # one block of margin
    assert int(ref["num_nodes"]) == want["nodes"]
    return lay


def _fits(ref, lay):
    """Every node of the map lies in a block of the layout (a blocked build of its cloud meets no record outside the box)."""
    (x0, y0, z0), (X, Y, Z) = bs.extent(ref)
    return (lay["x0"] <= x0 and x0 + X <= lay["x0"] + (lay["nx"] << lay["shx"]) and lay["y0"] <= y0 and
            y0 + Y <= lay["y0"] + (lay["ny"] << lay["shy"]) and lay["z0"] <= z0 and z0 + Z <= lay["z0"] + (1 << lay["shz"]))


def _check_reference_alone(ref, demand, min_points):
    out = bs.perfect_build(ref)
    rep = parity.compare(out, ref, demand, min_points=min_points)
    assert rep["ok"], rep["fail"]
    assert rep["cov_nodes_over_1e-5_vs_fp32"] == 0 and rep["cov_nodes_below_input_resolution"] == 0, rep
    return rep


@pytest.mark.parametrize("name", list(bs.SCENES))
def test_scene_gives_its_block_shape_and_the_reference_alone_passes_the_gates(name):
    want = bs.SCENES[name]
    cloud = bs.cloud(name)
    assert cloud.shape == (bs.POINTS + 1, 3) and cloud.dtype == np.float32
    assert np.array_equal(cloud[0], np.float32(want["origin"]))
    P = bs.params(name)
    ref = parity.ref_from_cloud(cloud, P, mode=2)
    _check_fixture(ref, P, bs.POINTS, want)
    flags = ref["flags"].astype(np.int64)
    assert int(np.count_nonzero((flags & 1) == 0)) == want["below_min"]
    if name == "levels_4_at_interval":       # the label threshold is decided both ways
        assert int(np.count_nonzero(flags & 2)) == bs.AT_INTERVAL["slopes"] and int(np.count_nonzero(flags & 4)) == bs.AT_INTERVAL["down"]
    _check_reference_alone(ref, "slope", 3)
    # another cloud of the scene (the GPU tier's fourth build) keeps inside the first one's box and its block of margin
    other = parity.ref_from_cloud(bs.cloud(name, bs.SEED + 1), P, mode=2)
    assert _fits(other, bs.plan(ref, bs.POINTS))


def test_box_is_the_stated_function_of_seed_and_index():
    lo, hi = (10.0, -98.0, 0.0), (98.0, -10.0, 0.24)
    pts = bs.box(bs.SEED, lo, hi, n=1000)
    assert pts.shape == (1000, 3) and pts.dtype == np.float32
    from grid_ndt_amd import scenes
    for i in (0, 1, 7, 999):
        for a in range(3):
            u = float(scenes.u01(np.uint64(3 * i + a), bs.SEED))
            assert pts[i, a] == np.float32(lo[a] + u * (hi[a] - lo[a]))
    assert np.array_equal(pts, bs.box(bs.SEED, lo, hi, n=2000)[:1000])      # a pure function of (seed, index)
    assert not np.array_equal(pts, bs.box(bs.SEED + 1, lo, hi, n=1000))


def test_min_points_5_variant_of_the_interval_scene():
    name = "levels_4_at_interval"
    P = bs.params(name, min_points=5)
    ref = parity.ref_from_cloud(bs.cloud(name), P, mode=2)
    _check_fixture(ref, P, bs.POINTS, bs.SCENES[name])
    assert int(np.count_nonzero((ref["flags"].astype(np.int64) & 1) == 0)) == bs.AT_INTERVAL["below_min_5"]
    _check_reference_alone(ref, "slope", 5)


def test_folded_interval_scene_has_half_the_nodes_in_the_same_blocks():
    name = "levels_4_at_interval"
    P = bs.params(name)
    cloud = bs.cloud(name)
    fold = bs.folded(cloud)
    assert np.array_equal(fold[:, :2], cloud[:, :2]) and np.array_equal(fold[0], cloud[0])
    ref = parity.ref_from_cloud(fold, P, mode=2)
    assert int(ref["num_nodes"]) == bs.FOLDED_NODES and sorted(set(ref["sz"].tolist())) == [-2, 2]
    lay = bs.plan(ref, bs.POINTS)
    assert (1 << lay["shx"], 1 << lay["shy"], 1 << lay["shz"]) == bs.SCENES[name]["block"]
    assert _fits(parity.ref_from_cloud(cloud, P, mode=2), lay)      # the unfolded cloud fits the folded one's box
