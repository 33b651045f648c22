"""GPU tier: k_bucket_blocked (gndt_blocked.hpp) reached with small clouds.  The host takes blocked buckets from 2^20 points on, a
tuning choice (Tuning::blocked_min_points) and no limit of the kernel; with the floor lowered to 65 536 points
(GNDT_DEBUG_BLOCKED_MIN_POINTS, blocked_scenes.blocked_floor) and strategy PARTITION_TWO_LEVEL a box of 131 072 points in 8 x 8 blocks
takes them, and the kernel can be held to what the 1.1 M-point scenes of tests/test_gpu_blocked_shapes.py cannot pay for: every block
shape again at an eighth of the points, sixteen fuzzed boxes (extents that are no multiple of the block, corners on either side of
the skipped index 0 and thousands of columns out, odd level padding, origins off the lattice), the lifetime of the layout the handle
remembers (the size window, a "no" and a new decision, the reset on another origin) and a small blocked build in the buffers a
1.1 M-point one left behind.  tests/test_gpu_poisoned.py runs a group of these on memory that does not start out as zeros.

Every test asserts through last_strategy() == 7 and block_layout() that it reached the blocked kernel, and holds every map to the
oracle's by parity.compare's gates, unchanged (tests/test_blocked_scenes_host.py: the oracle alone passes the strict gates on every
cloud used here).

What the small builds do NOT cover: a cloud of 131 072 points has 4 097 bitmap words, so behind the bucket kernel it is ordered and
emitted by k_place_emit_rows (words <= Tuning::place_emit_words = 16 384, launch_order_and_emit); a production-size blocked build takes
the separate ordering passes and k_emit_rows.  Both read the staging rows k_bucket_blocked writes and both must give the oracle's map.
The 1.1 M-point tests remain the cover of the production combination; one fuzzed box here (blocked_scenes.FUZZ_SEED_SEPARATE_PASSES:
555 022 points, 17 346 words) reaches the separate passes at moderate size."""
import ctypes as C

import numpy as np
import pytest

from tests import blocked_scenes as bs
from tests import parity
from tests.gpu_kit import dev, handle

pytestmark = pytest.mark.gpu

EXACT_FIELDS = ("sx", "sy", "sz", "count", "first_idx", "flags")


def _set_origin(m, origin):
    """gndt_set_origin on the LIVE handle (TwoDmap.setCloudFirst makes a new one, which remembers nothing)"""
    o = (C.c_float * 3)(*[float(v) for v in origin])
    m._check(m._L.gndt_set_origin(m._h, o))
    m.cloudFirst = tuple(float(v) for v in origin)


def _is_the_oracles_map(m, ref, P, what):
    out = m.export()
    rep = parity.compare(out, ref, P["demand"], min_points=P["min_points"])
    assert rep["ok"], (what, m.STRATEGY_NAMES[m.last_strategy()], rep["fail"])
    return out


def _blocked_and_not_rerun(m, retries, what):
    assert m.last_strategy() == bs.BLOCKED and m.retry_count() == retries, (what, m.STRATEGY_NAMES[m.last_strategy()], m.retry_count(), retries)


def test_with_the_default_floor_a_small_scene_is_never_blocked():
    """Nobody who does not ask gets another build: the handle decides "yes" for the small box, and the floor holds."""
    import grid_ndt_amd as g
    name = "flat_1"
    P = bs.small_params(name)
    cloud = bs.small_cloud(name)
    ref = parity.ref_from_cloud(cloud, P, mode=2)
    m = handle(P, bs.TWO_LEVEL, min_points=P["min_points"])
    m.setCloudFirst(cloud[0])
    t = dev(cloud[1:], copy=True)
    for k in range(3):
        m.create2DMap("slope", t)
        _is_the_oracles_map(m, ref, P, ("default floor, build", k))
        assert m.last_strategy() == bs.HASHED, (k, m.STRATEGY_NAMES[m.last_strategy()])
    assert m.block_layout() == bs.SMALL_SCENES[name]["layout"]
    with bs.blocked_floor():                                     # ... and the same handle takes them once asked
        m.create2DMap("slope", t)
        _is_the_oracles_map(m, ref, P, "lowered floor")
        assert m.last_strategy() == bs.BLOCKED
    with pytest.raises(g.GndtError):
        with bs.blocked_floor(bs.SMALL_FLOOR - 1):
            pass
    m.create2DMap("slope", t)                                    # the default is back, whatever happened in the blocks
    m.sync()
    assert m.last_strategy() == bs.HASHED


@pytest.mark.parametrize("demand", ["slope", "true"])
@pytest.mark.parametrize("name", list(bs.SMALL_SCENES))
def test_every_block_shape_small(name, demand):
    """_shape_and_parity of tests/test_gpu_blocked_shapes.py at an eighth of the points: three builds and one of the sibling cloud, every
    map the oracle's, the layout after the first build the plan's, builds 2 - 4 blocked and not re-run."""
    P = bs.small_params(name, demand)
    cloud = bs.small_cloud(name)
    ref = parity.ref_from_cloud(cloud, P, mode=2)
    want = bs.plan(ref, bs.SMALL_POINTS)
    assert want == bs.SMALL_SCENES[name]["layout"]               # (the fixture: also CPU tier)
    with bs.blocked_floor():
        m = handle(P, bs.TWO_LEVEL, min_points=P["min_points"])
        m.setCloudFirst(cloud[0])
        t = dev(cloud[1:], copy=True)
        retries = None
        for k in range(3):
            m.create2DMap(demand, t)
            _is_the_oracles_map(m, ref, P, (name, "build", k))
            if k == 0:
                got, retries = m.block_layout(), m.retry_count()
                print(f"[blocked small] {name} {demand}: {got}, first build {m.STRATEGY_NAMES[m.last_strategy()]}, re-runs {retries}")
                assert got == want, (got, want)
                assert m.last_strategy() == bs.HASHED
            else:
                _blocked_and_not_rerun(m, retries, (name, k))
        other = bs.small_cloud(name, bs.SEED + 1)
        m.create2DMap(demand, dev(other[1:], copy=True))
        _is_the_oracles_map(m, parity.ref_from_cloud(other, P, mode=2), P, (name, "other cloud"))
        _blocked_and_not_rerun(m, retries, (name, "other cloud"))
        assert m.block_layout() == want


@pytest.mark.parametrize("seed", bs.FUZZ_SEEDS + (bs.FUZZ_SEED_SEPARATE_PASSES,))
def test_fuzzed_boxes(seed):
    """Two builds of a random_box: the layout the plan's, the second build blocked and not re-run, both maps the oracle's."""
    b = bs.fuzz_box(seed)
    P = bs.fuzz_params(b)
    cloud = bs.fuzz_cloud(seed)
    ref = parity.ref_from_cloud(cloud, P, mode=2)
    want = bs.plan(ref, b["n"])
    assert want["state"] == 1
    with bs.blocked_floor():
        m = handle(P, bs.TWO_LEVEL, min_points=P["min_points"])
        m.setCloudFirst(cloud[0])
        t = dev(cloud[1:], copy=True)
        m.create2DMap(b["demand"], t)
        _is_the_oracles_map(m, ref, P, (seed, "first build"))
        got, retries = m.block_layout(), m.retry_count()
        print(f"[blocked small] seed {seed}: {b['box']} cells at {b['corner']}, {b['n']} points, min_points {b['min_points']}, {b['demand']}: {got}")
        assert got == want, (got, want)
        m.create2DMap(b["demand"], t)
        _is_the_oracles_map(m, ref, P, (seed, "second build"))
        _blocked_and_not_rerun(m, retries, seed)


def test_staging_rows_run_out_inside_a_small_blocked_build():
    """test_staging_rows_run_out_inside_a_blocked_build of tests/test_gpu_blocked_shapes.py, small: a handle told to expect 16 383 nodes
    sizes its staging rows for them (hint + hint / 8); the folded cloud fits, and the unfolded cloud of the same box and size, with twice
    the nodes, runs out of rows inside the blocked bucket kernel (sbase + M > stage_cap): the build is run again with more."""
    import grid_ndt_amd as g
    name = "levels_4_at_interval"
    P = bs.small_params(name)
    b = bs.small_cloud(name)
    a = bs.folded(b)
    ref_a = parity.ref_from_cloud(a, P, mode=2)
    assert int(ref_a["num_nodes"]) == bs.SMALL_FOLDED_NODES
    with bs.blocked_floor():
        m = g.TwoDmap(P["grid_len"], P["z_len"], strategy=bs.TWO_LEVEL, min_points=P["min_points"], max_nodes_hint=bs.SMALL_FOLDED_NODES)
        m.setInterval(P["slope_interval"])
        m.setCloudFirst(a[0])
        ta = dev(a[1:], copy=True)
        for k in range(2):
            m.create2DMap("slope", ta)
            _is_the_oracles_map(m, ref_a, P, ("folded cloud, build", k))
        assert m.last_strategy() == bs.BLOCKED and m.block_layout() == bs.SMALL_SCENES[name]["layout"]
        before = m.retry_count()
        m.create2DMap("slope", dev(b[1:], copy=True))
        _is_the_oracles_map(m, parity.ref_from_cloud(b, P, mode=2), P, "unfolded cloud")
        print(f"[blocked small] staging rows: re-runs {before} -> {m.retry_count()}, the build ended as {m.STRATEGY_NAMES[m.last_strategy()]}")
        assert m.retry_count() > before and m.last_strategy() == bs.BLOCKED      # (more rows is not a "no": the re-run is blocked again)


def test_layout_lifetime_on_one_handle():
    """blocked_scenes.lifetime_script on ONE handle against blocked_scenes.LayoutMemory: decided per size window, "no" after a miss (one
    re-run, hashed) until the size leaves the window, decided anew there, reset by another origin.  A re-run for ROOM is not the
    layout's: where a cloud is the first of its size on the handle the count may rise by more than the restatement's."""
    P = bs.small_params(bs.LIFETIME_SCENE)
    mem = bs.LayoutMemory(floor=bs.SMALL_FLOOR)
    seen = []
    with bs.blocked_floor():
        m = handle(P, bs.TWO_LEVEL, min_points=P["min_points"])
        m.setCloudFirst(bs.small_cloud(bs.LIFETIME_SCENE)[0])
        m._ensure("slope")                                       # (the handle itself: made by the first call that needs it)
        assert m.block_layout()["state"] == 0
        for what, cloud, new_origin, strategy, reruns, state, sized in bs.lifetime_script():
            if new_origin:
                m.sync()
                _set_origin(m, cloud[0])
                mem.set_origin()
                assert m.block_layout()["state"] == 0 == mem.state                       # step 6
            ref = parity.ref_from_cloud(cloud, P, mode=2)
            n = cloud.shape[0] - 1
            before, model_before = m.retry_count(), mem.retries
            m.create2DMap("slope", dev(cloud[1:], copy=True))
            _is_the_oracles_map(m, ref, P, what)
            model_strategy = mem.build(ref, n)
            assert (model_strategy, mem.retries - model_before, mem.state) == (strategy, reruns, state), what      # (the script: also CPU tier)
            delta = m.retry_count() - before
            got = m.block_layout()
            print(f"[blocked small] lifetime {what}: {m.STRATEGY_NAMES[m.last_strategy()]}, re-runs +{delta}, layout {got}")
            assert m.last_strategy() == model_strategy, (what, m.STRATEGY_NAMES[m.last_strategy()])
            assert delta == reruns if sized else delta >= reruns, (what, delta, reruns)
            want = mem.block_layout()
            assert (got == want) if want["state"] == 1 else (got["state"] == want["state"]), (what, got, want)
            seen.append(m.last_strategy())
    assert seen.count(bs.BLOCKED) == 3 and m.retry_count() >= 1


# large scene -> small scene of the same cells.  The handle's cells are fixed when it is made, so a pair shares them: flat_1 (blocks of
# 32 x 16 x 1) then levels_2 (16 x 16 x 2) under one origin — the small cloud falls out of the large one's size window; levels_16_off_origin
# (8 x 4 x 16) then levels_6_padded (8 x 8 x 8, level padding) under ANOTHER origin — the reset; and levels_32_moved_origin large then small
LARGE_THEN_SMALL = (("flat_1", "levels_2"), ("levels_16_off_origin", "levels_6_padded"), ("levels_32_moved_origin", "levels_32_moved_origin"))


@pytest.mark.parametrize("large,small", LARGE_THEN_SMALL, ids=[f"{a}-then-{b}" for a, b in LARGE_THEN_SMALL])
def test_large_then_small_on_one_handle(large, small):
    """The handle builds a 1.1 M-point scene twice (blocked: its parity is tests/test_gpu_blocked_shapes.py's business), then a small
    scene twice.  A handle's buffers only grow, so every buffer of the small blocked build — records of both levels, cursors, ranges,
    staging rows, order arrays, result rows — lies inside what the large one left behind.  The small map is the oracle's, and its keys,
    counts, first-seen indices and flags are, byte for byte, those of the same two builds on a fresh handle (moments go through the
    gates only: two builds of one cloud may differ in their last bits, tests/test_gpu_reproducible.py)."""
    P = bs.small_params(small)
    assert P == bs.params(large)                                 # one handle: the same cells
    big, cloud = bs.cloud(large), bs.small_cloud(small)
    ref = parity.ref_from_cloud(cloud, P, mode=2)
    want = bs.SMALL_SCENES[small]["layout"]
    with bs.blocked_floor():
        used = handle(P, bs.TWO_LEVEL, min_points=P["min_points"])
        used.setCloudFirst(big[0])
        tb = dev(big[1:], copy=True)
        for _ in range(2):
            used.create2DMap("slope", tb)
            used.sync()
        assert used.last_strategy() == bs.BLOCKED
        large_layout, large_nodes = used.block_layout(), int(used.export()["num_nodes"])
        del tb
        _set_origin(used, cloud[0])
        assert used.block_layout()["state"] == (1 if np.array_equal(big[0], cloud[0]) else 0)
        fresh = handle(P, bs.TWO_LEVEL, min_points=P["min_points"])
        fresh.setCloudFirst(cloud[0])
        t = dev(cloud[1:], copy=True)
        outs = []
        for m in (used, fresh):
            m.create2DMap("slope", t)
            _is_the_oracles_map(m, ref, P, (small, "first small build", m is used))
            assert m.last_strategy() == bs.HASHED and m.block_layout() == want
            retries = m.retry_count()
            m.create2DMap("slope", t)
            outs.append(_is_the_oracles_map(m, ref, P, (small, "second small build", m is used)))
            _blocked_and_not_rerun(m, retries, (small, m is used))      # not vacuous: both end blocked
    a, b = outs
    for k in EXACT_FIELDS:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k
    assert int(a["num_nodes"]) == bs.SMALL_SCENES[small]["nodes"] and int(a["num_nodes"]) * 3 < large_nodes == bs.SCENES[large]["nodes"]
    assert want != large_layout and want["buckets"] < large_layout["buckets"] and bs.SMALL_POINTS * 8 < bs.POINTS
