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
    # no label decision inside the oracle's own fp32 error: a build without any error of its own gives the oracle's labels
    assert np.array_equal(bs.labels_of_perfect_build(ref, bs.INTERVAL, demand, min_points), ref["flags"].astype(np.int64))
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


# ---- the small scenes, the fuzzed boxes and the layout's lifetime (tests/test_gpu_blocked_small.py) -------------------------------------

@pytest.mark.parametrize("name", list(bs.SMALL_SCENES))
def test_small_scene_gives_its_table_row_and_the_reference_alone_passes_the_gates(name):
    want = bs.SMALL_SCENES[name]
    twin = bs.SCENES[name]
    assert (want["grid_len"], want["z_len"], want["origin"]) == (twin["grid_len"], twin["z_len"], twin["origin"])
    cloud = bs.small_cloud(name)
    assert cloud.shape == (bs.SMALL_POINTS + 1, 3) and cloud.dtype == np.float32 and np.array_equal(cloud[0], np.float32(want["origin"]))
    assert np.array_equal(cloud[1:], bs.box(bs.SEED, want["lo"], want["hi"], bs.SMALL_POINTS))
    for a in (0, 1):      # cut around the large box's centre
        assert abs((want["lo"][a] + want["hi"][a]) - (twin["lo"][a] + twin["hi"][a])) < 1e-9
    P = bs.small_params(name)
    ref = parity.ref_from_cloud(cloud, P, mode=2)
    lay = bs.plan(ref, bs.SMALL_POINTS)
    assert lay == want["layout"], (lay, want["layout"])
    assert (lay["nx"], lay["ny"], lay["buckets"]) == (10, 10, 100)                       # 8 x 8 blocks and the margin
    assert (1 << lay["shx"], 1 << lay["shy"], 1 << lay["shz"]) == twin["block"]           # the large twin's block shape
    assert bs.extent(ref)[1] == want["box"] and int(ref["num_nodes"]) == want["nodes"]
    assert want["box"][0] == 8 << lay["shx"] and want["box"][1] == 8 << lay["shy"] and want["box"][2] == twin["levels"]
    _check_reference_alone(ref, "slope", 3)
    other = parity.ref_from_cloud(bs.small_cloud(name, bs.SEED + 1), P, mode=2)          # (the GPU tier's fourth build)
    assert _fits(other, lay) and bs.fits(other, lay)
    _check_reference_alone(other, "slope", 3)
    assert bs.SMALL_FLOOR <= bs.SMALL_POINTS < bs.POINTS // 8 + 1


def _fuzz_ref(seed):
    b = bs.fuzz_box(seed)
    return b, parity.ref_from_cloud(bs.fuzz_cloud(seed), bs.fuzz_params(b), mode=2)


@pytest.mark.parametrize("seed", bs.FUZZ_SEEDS + (bs.FUZZ_SEED_SEPARATE_PASSES,))
def test_fuzzed_box_is_planned_blocked_and_the_reference_alone_passes_the_gates(seed):
    b, ref = _fuzz_ref(seed)
    assert b == bs.fuzz_box(seed)                                  # a pure function of the seed
    X, Y, Z = b["box"]
    lay = bs.plan(ref, b["n"])
    assert lay["state"] == 1, (b, lay)
    assert bs.extent(ref) == (b["corner"], b["box"])               # the map occupies exactly the box that was drawn
    assert 1 <= Z <= 32 and (1 << lay["shz"]) >= Z > (1 << lay["shz"]) // 2
    assert X % (1 << lay["shx"]) and Y % (1 << lay["shy"])         # no multiple of the block
    per_block = b["n"] // ((lay["nx"] - 2) * (lay["ny"] - 2))
    assert 1700 <= per_block <= 4500, per_block
    assert all(abs(c) + e <= bs.FUZZ_FAR for c, e in zip(b["corner"][:2], (X, Y)))
    o = np.float64(b["origin"])
    assert not np.any(np.float64(np.float32(b["origin"])) != o) and not np.any(o / b["grid_len"] == np.round(o / b["grid_len"]))
    if seed == bs.FUZZ_SEED_SEPARATE_PASSES:
        assert 16_384 < (b["n"] + 31) // 32 + 1 and b["n"] < 600_000      # more bitmap words than Tuning::place_emit_words
    else:
        assert b["n"] < 200_000 and (b["n"] + 31) // 32 + 1 <= 16_384
    rep = parity.compare(bs.perfect_build(ref), ref, b["demand"], min_points=b["min_points"])
    assert rep["ok"], rep["fail"]
    assert np.array_equal(bs.labels_of_perfect_build(ref, bs.INTERVAL, b["demand"], b["min_points"]), ref["flags"].astype(np.int64))


def test_the_fuzz_seeds_in_use_cover_what_the_generator_is_there_for():
    boxes = [bs.fuzz_box(s) for s in bs.FUZZ_SEEDS]
    assert len(bs.FUZZ_SEEDS) == len(set(bs.FUZZ_SEEDS)) == 16
    assert {(b["grid_len"], b["z_len"]) for b in boxes} == set(bs.FUZZ_CELLS)
    levels = {b["box"][2] for b in boxes}
    assert {1, 2, 4, 8, 16, 32} <= levels and levels & {3, 7, 15, 31} and levels & {5, 9, 17}
    assert {b["min_points"] for b in boxes} == {1, 3, 5} and {b["demand"] for b in boxes} == {"slope", "true"}
    assert any(all(c + e <= 0 for c, e in zip(b["corner"], b["box"])) for b in boxes)                   # all-negative
    assert any(c + e == 0 for b in boxes for c, e in zip(b["corner"], b["box"]))                        # ends on index -1
    assert any(c == 0 for b in boxes for c in b["corner"])                                              # starts on index 1
    assert any(c > 1000 for b in boxes for c in b["corner"][:2]) and any(c < -1000 for b in boxes for c in b["corner"][:2])
    # the generator itself reaches tens of thousands of columns (such boxes fail the gates on the oracle alone: blocked_scenes.FUZZ_SEEDS)
    assert max(abs(c) for s in range(100, 260) for c in bs.random_box(s)["corner"][:2]) > 20_000


def test_layout_memory_on_the_oracles_maps_follows_the_scripted_lifetime():
    """The restatement of the three host rules, driven by the script the GPU tier drives the handle with: hashed, blocked; a miss, one
    re-run and "no"; a new decision outside the window; blocked; reset by the origin; decided anew."""
    P = bs.small_params(bs.LIFETIME_SCENE)
    mem = bs.LayoutMemory(floor=bs.SMALL_FLOOR)
    script = bs.lifetime_script()
    assert [s[0][0] for s in script] == list("11234577")
    a_lay = bs.SMALL_SCENES[bs.LIFETIME_SCENE]["layout"]
    seen = []
    for what, cloud, new_origin, strategy, reruns, state, _ in script:
        if new_origin:
            mem.set_origin(changed=True)
            assert mem.block_layout() == {"state": 0}
        n = cloud.shape[0] - 1
        ref = parity.ref_from_cloud(cloud, P, mode=2)
        before = mem.retries
        got = mem.build(ref, n)
        assert (got, mem.retries - before, mem.state) == (strategy, reruns, state), (what, got, mem.retries - before, mem.state)
        seen.append((n, mem.block_layout()))
        _check_reference_alone(ref, "slope", 3)
    n, n15 = bs.SMALL_POINTS, bs.SMALL_POINTS + bs.SMALL_POINTS // 2
    assert [s[0] for s in seen] == [n, n, n, n, n15, n15, n15, n15]
    assert not (n15 <= n + n // 4)                                          # 1.5 n lies outside n's window
    assert seen[0][1] == seen[1][1] == a_lay
    assert seen[2][1] == seen[3][1] == {"state": -1}
    shifted_lay = dict(a_lay, x0=a_lay["x0"] + 3 * (1 << a_lay["shx"]))
    assert seen[4][1] == seen[5][1] == shifted_lay                          # the same blocks, three further along x
    assert seen[6][1] == seen[7][1] and seen[6][1]["state"] == 1 and seen[6][1] != shifted_lay      # other keys under the other origin
    # with the floor at its default none of these clouds is ever blocked
    mem = bs.LayoutMemory()
    for what, cloud, new_origin, *_ in script[:2]:
        assert mem.build(parity.ref_from_cloud(cloud, P, mode=2), cloud.shape[0] - 1) == bs.HASHED


def test_folded_small_interval_scene_has_half_the_nodes_in_the_same_blocks():
    name = "levels_4_at_interval"
    P = bs.small_params(name)
    cloud = bs.small_cloud(name)
    ref = parity.ref_from_cloud(bs.folded(cloud), P, mode=2)
    assert int(ref["num_nodes"]) == bs.SMALL_FOLDED_NODES and sorted(set(ref["sz"].tolist())) == [-2, 2]
    lay = bs.plan(ref, bs.SMALL_POINTS)
    assert lay == bs.SMALL_SCENES[name]["layout"]
    assert _fits(parity.ref_from_cloud(cloud, P, mode=2), lay)      # the unfolded cloud fits the folded one's box
    _check_reference_alone(ref, "slope", 3)
    # rows for a hint of SMALL_FOLDED_NODES nodes (hint + hint / 8, partition_begin) hold the folded map and not the unfolded one
    assert bs.SMALL_FOLDED_NODES < bs.SMALL_FOLDED_NODES + bs.SMALL_FOLDED_NODES // 8 < bs.SMALL_SCENES[name]["nodes"]
