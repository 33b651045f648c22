"""GPU tier: the blocked bucket kernel's column table and the per-column ordering pass (gndt_blocked.hpp col_tab, gndt_partition.hpp
k_order_dest_table).

A blocked build that orders and emits in two kernels writes one record per column of every block and no ord_cf / ord_idx; the pass runs
over those records.  A 131 072-point box takes that tail only when asked (GNDT_DEBUG_PLACE_EMIT_WORDS = 0: never the one-kernel tail of
small clouds), so every small test here sets it, lowers the floor under blocked buckets (blocked_scenes.blocked_floor) and asks for
strategy PARTITION_TWO_LEVEL — and asserts last_strategy() == 7 and the layout, so that a fallback to hashed buckets fails.  Every map
is held to the oracle's by parity.compare's strict gates, unchanged, for both demands.  Two GPU builds are compared in their exact
fields only (keys, counts, first-seen indices, flags, in row order): the moments of two builds of one cloud may differ in their last
bits (tests/test_gpu_reproducible.py).

What can go wrong and where it is looked for:
  * the table's stride (2^(shx + shy) records per block) and the column prefix across waves: every block shape;
  * who writes a column's record: blocks built voxel by voxel to hold exactly 512 nodes (every column at its full height), one node
    (every record but one empty), and one column with nodes at levels 2 and 5 but none at level 0 (its record is written by a thread
    that holds no node) — the counts are checked on the oracle's map in the set-up; margin blocks (no nodes at all) surround every box;
  * records of an earlier build: a second cloud of the same layout without a third of the first one's columns, and the build after a
    cloud that left the box or ran the staging rows out (both early ways out of the kernel);
  * a record or an order word nobody wrote: a group of these tests once more on the poisoned variant of the library, both fill bytes;
  * the production combination: a 1.1 M-point box that takes 8 x 8 x 8 blocks with no debug option set."""
import contextlib
import functools

import numpy as np
import pytest

from tests import blocked_scenes as bs
from tests import parity
from tests import poison_tier
from tests.gpu_kit import dev, handle

pytestmark = pytest.mark.gpu

EXACT_FIELDS = ("sx", "sy", "sz", "count", "first_idx", "flags")
PLACE_EMIT_WORDS_DEFAULT = 16_384      # Tuning::place_emit_words
POINTS_PER_VOXEL = 4                   # of a voxel that an edit fills (min_points is 3)


@contextlib.contextmanager
def two_kernel_tail(column_dest=1):
    """GNDT_DEBUG_PLACE_EMIT_WORDS = 0 and GNDT_DEBUG_COLUMN_DEST for a block, under the lowered floor; the defaults come back"""
    import grid_ndt_amd as g
    T = g.TwoDmap
    with bs.blocked_floor():
        T.set_debug_option(T.DEBUG_PLACE_EMIT_WORDS, 0)
        T.set_debug_option(T.DEBUG_COLUMN_DEST, column_dest)
        try:
            yield
        finally:
            T.set_debug_option(T.DEBUG_PLACE_EMIT_WORDS, PLACE_EMIT_WORDS_DEFAULT)
            T.set_debug_option(T.DEBUG_COLUMN_DEST, 1)


def _is_the_oracles_map(m, ref, P, what):
    out = m.export()
    rep = parity.compare(out, ref, P["demand"], min_points=P["min_points"])
    assert rep["ok"], (what, m.STRATEGY_NAMES[m.last_strategy()], rep["fail"])
    return out


def _blocked(m, retries, what):
    assert m.last_strategy() == bs.BLOCKED and m.retry_count() == retries, (what, m.STRATEGY_NAMES[m.last_strategy()], m.retry_count(), retries)


def _decided_then_blocked(cloud, ref, P, want, what, builds=2):
    """A fresh handle: the first build hashed, its map decides the layout `want`; every later build blocked and not re-run; every map
    the oracle's.  -> the handle, the last export."""
    m = handle(P, bs.TWO_LEVEL, min_points=P["min_points"])
    m.setCloudFirst(cloud[0])
    t = dev(cloud[1:], copy=True)
    out = retries = None
    for k in range(builds):
        m.create2DMap(P["demand"], t)
        out = _is_the_oracles_map(m, ref, P, (what, "build", k))
        if k == 0:
            retries = m.retry_count()
            assert m.last_strategy() == bs.HASHED and m.block_layout() == want, (what, m.STRATEGY_NAMES[m.last_strategy()], m.block_layout(), want)
        else:
            _blocked(m, retries, (what, k))
    return m, out


# ---- every shape ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("demand", ["slope", "true"])
@pytest.mark.parametrize("name", list(bs.SMALL_SCENES))
def test_every_block_shape_through_the_column_pass(name, demand):
    """512, 256, 128, 64, 32 and 16 columns per block: the table's stride and, from 128 columns on, the column prefix across waves."""
    P = bs.small_params(name, demand)
    cloud = bs.small_cloud(name)
    ref = parity.ref_from_cloud(cloud, P, mode=2)
    with two_kernel_tail():
        m, _ = _decided_then_blocked(cloud, ref, P, bs.SMALL_SCENES[name]["layout"], name, builds=3)
        other = bs.small_cloud(name, bs.SEED + 1)
        retries = m.retry_count()
        m.create2DMap(demand, dev(other[1:], copy=True))
        _is_the_oracles_map(m, parity.ref_from_cloud(other, P, mode=2), P, (name, "other cloud"))
        _blocked(m, retries, (name, "other cloud"))


# ---- blocks built voxel by voxel ----------------------------------------------------------------------------------------------------------

def _slot(lay, lx, ly, lz):
    return (lz << (lay["shx"] + lay["shy"])) | (ly << lay["shx"]) | lx


def _edits(name):
    """block (bx, by) of the small scene's layout (1 .. 8: inside the margin) -> the slots of the block that get points"""
    lay = bs.SMALL_SCENES[name]["layout"]
    edits = {(2, 2): list(range(512)), (2, 6): [_slot(lay, 2, 5, (1 << lay["shz"]) // 2)]}
    if lay["shz"] >= 3:
        edits[(6, 2)] = [_slot(lay, 1, 6, 2), _slot(lay, 1, 6, 5)]      # one column, nothing at level 0
    return edits


@functools.lru_cache(maxsize=2)
def edited_cloud(name):
    """The small scene with the blocks of _edits emptied and filled again voxel by voxel: POINTS_PER_VOXEL points within 0.3 cells of the
    centre of every chosen voxel; the other points that lay in those blocks are drawn again in the rest of the box, so the cloud keeps
    its size; the points are shuffled (no locality, first-seen indices of the new nodes anywhere).  Cell c (contiguous index) of an axis
    is origin + [c, c + 1) * cell on either side of the origin (blocked_scenes.contiguous)."""
    s = bs.SMALL_SCENES[name]
    lay, base = s["layout"], bs.small_cloud(name)
    o, pts = np.float64(base[0]), np.array(base[1:], np.float64)
    cell = np.float64([s["grid_len"], s["grid_len"], s["z_len"]])
    ext = (1 << lay["shx"], 1 << lay["shy"], 1 << lay["shz"])
    r = np.random.default_rng(0xED17)
    boxes = {}
    for (bx, by) in _edits(name):
        c0 = np.float64([lay["x0"] + bx * ext[0], lay["y0"] + by * ext[1]])
        boxes[(bx, by)] = (o[:2] + c0 * cell[:2] - 1e-3, o[:2] + (c0 + ext[:2]) * cell[:2] + 1e-3)      # (a little more: float32 points on the faces go too)

    def in_an_edited_block(p):
        hit = np.zeros(p.shape[0], bool)
        for lo, hi in boxes.values():
            hit |= ((p[:, :2] > lo) & (p[:, :2] < hi)).all(1)
        return hit

    gone = in_an_edited_block(pts)
    new = []
    for (bx, by), slots in _edits(name).items():
        sl = np.int64(slots)
        c = np.stack([lay["x0"] + bx * ext[0] + (sl & (ext[0] - 1)), lay["y0"] + by * ext[1] + ((sl >> lay["shx"]) & (ext[1] - 1)),
                      lay["z0"] + (sl >> (lay["shx"] + lay["shy"]))], 1).astype(np.float64)
        c = np.repeat(c, POINTS_PER_VOXEL, 0)
        new.append(o + (c + 0.5 + r.uniform(-0.3, 0.3, c.shape)) * cell)
    rest = int(gone.sum()) - sum(a.shape[0] for a in new)
    assert rest > 0
    lo, hi = np.float64(s["lo"]), np.float64(s["hi"])
    again = lo + r.random((rest, 3)) * (hi - lo)
    for _ in range(64):
        bad = in_an_edited_block(again)
        if not bad.any():
            break
        again[bad] = lo + r.random((int(bad.sum()), 3)) * (hi - lo)
    assert not in_an_edited_block(again).any()
    allp = np.concatenate([pts[~gone]] + new + [again], 0)
    assert allp.shape[0] == bs.SMALL_POINTS
    allp = allp[r.permutation(allp.shape[0])]
    c = np.concatenate([base[:1], allp.astype(np.float32)], 0)
    c.setflags(write=False)
    return c


def nodes_per_block(ref, lay):
    """-> {(bx, by): [(contiguous level, count), ...]} of an oracle map under a layout"""
    cx, cy, cz = (bs.contiguous(ref[k]) for k in ("sx", "sy", "sz"))
    bx, by = (cx - lay["x0"]) >> lay["shx"], (cy - lay["y0"]) >> lay["shy"]
    out = {}
    for b, z in zip(zip(bx.tolist(), by.tolist()), cz.tolist()):
        out.setdefault(b, []).append(z)
    return out


@functools.lru_cache(maxsize=4)
def edited_ref(name, demand):
    """The oracle's map of edited_cloud and the layout it decides; the intended node counts hold on that map (asserted, nothing skipped)."""
    P = bs.small_params(name, demand)
    cloud = edited_cloud(name)
    ref = parity.ref_from_cloud(cloud, P, mode=2)
    want = bs.plan(ref, bs.SMALL_POINTS)
    lay = bs.SMALL_SCENES[name]["layout"]
    assert want == lay, (want, lay)
    per = nodes_per_block(ref, lay)
    for b, slots in _edits(name).items():
        assert len(per.get(b, [])) == len(slots), (name, b, len(per.get(b, [])), len(slots))
    if (6, 2) in _edits(name):
        assert sorted(z - lay["z0"] for z in per[(6, 2)]) == [2, 5]
    counts = sorted(len(v) for v in per.values())
    assert counts[-1] == 512 and counts[0] == 1
    assert len(per) <= 64 and lay["buckets"] == 100          # (the 36 margin blocks hold nothing)
    # (the labels the oracle gives are those of a build without error: no node of the fixture sits on the threshold)
    assert np.array_equal(bs.labels_of_perfect_build(ref, bs.INTERVAL, demand, P["min_points"]), ref["flags"].astype(np.int64))
    return ref, want


@pytest.mark.parametrize("demand", ["slope", "true"])
@pytest.mark.parametrize("name", ["flat_1", "levels_6_padded"])
def test_blocks_of_512_nodes_and_of_one(name, demand):
    """32 x 16 x 1 and 8 x 8 x 8 blocks: a full block, a block of one node, (8 x 8 x 8) a block whose only column has no node at level 0."""
    P = bs.small_params(name, demand)
    ref, want = edited_ref(name, demand)
    with two_kernel_tail():
        _decided_then_blocked(edited_cloud(name), ref, P, want, (name, "edited"), builds=3)


# ---- records of an earlier build ----------------------------------------------------------------------------------------------------------

def without_a_third_of_the_columns(cloud, grid_len):
    """Every point of a column with (cx + cy) % 3 == 0 moved one cell along x: those columns are gone, the cloud keeps its size."""
    out = cloud.copy()
    c = np.floor((out[1:, :2].astype(np.float64) - np.float64(out[0, :2])) / grid_len).astype(np.int64)
    move = (c[:, 0] + c[:, 1]) % 3 == 0
    out[1:, 0][move] += np.float32(grid_len)
    return out


@pytest.mark.parametrize("demand", ["slope", "true"])
def test_a_table_that_holds_another_clouds_columns(demand):
    """Cloud A twice, then on the same handle cloud B of the same layout without a third of A's columns: the table still holds A's
    record for each of them until B's build writes nodes = 0 there."""
    name = "levels_4_at_interval"
    P = bs.small_params(name, demand)
    a = bs.small_cloud(name)
    b = without_a_third_of_the_columns(a, P["grid_len"])
    ref_a, ref_b = parity.ref_from_cloud(a, P, mode=2), parity.ref_from_cloud(b, P, mode=2)
    assert int(ref_b["num_columns"]) * 10 <= int(ref_a["num_columns"]) * 7 and bs.fits(ref_b, bs.SMALL_SCENES[name]["layout"])
    with two_kernel_tail():
        m, _ = _decided_then_blocked(a, ref_a, P, bs.SMALL_SCENES[name]["layout"], "A")
        retries = m.retry_count()
        for cloud, ref, what in ((b, ref_b, "B"), (a, ref_a, "A again")):
            m.create2DMap(demand, dev(cloud[1:], copy=True))
            _is_the_oracles_map(m, ref, P, what)
            _blocked(m, retries, what)


def test_the_build_after_a_cloud_that_left_the_box():
    """A few hundred points of the cloud three blocks out: their buckets leave the kernel early (blk_miss), the build is re-run hashed;
    the original cloud on the same handle gives the oracle's map again."""
    name = "levels_6_padded"
    P = bs.small_params(name)
    lay = bs.SMALL_SCENES[name]["layout"]
    a = bs.small_cloud(name)
    out = a.copy()
    out[1:301, 0] += np.float32(11 * (1 << lay["shx"]) * P["grid_len"])      # (beyond the box and its block of margin)
    ref_a, ref_out = parity.ref_from_cloud(a, P, mode=2), parity.ref_from_cloud(out, P, mode=2)
    assert not bs.fits(ref_out, lay)
    with two_kernel_tail():
        m, _ = _decided_then_blocked(a, ref_a, P, lay, "A")
        before = m.retry_count()
        m.create2DMap("slope", dev(out[1:], copy=True))
        _is_the_oracles_map(m, ref_out, P, "the cloud that leaves the box")
        assert m.last_strategy() == bs.HASHED and m.retry_count() > before and m.block_layout()["state"] == -1
        for k in range(2):
            m.create2DMap("slope", dev(a[1:], copy=True))
            _is_the_oracles_map(m, ref_a, P, ("A after the miss", k))


def test_the_build_after_the_staging_rows_ran_out():
    """test_staging_rows_run_out_inside_a_small_blocked_build (tests/test_gpu_blocked_small.py) with the column pass behind it: the
    buckets that find no rows leave early and write empty records; the re-run and the next build of the first cloud are blocked and
    give the oracle's maps."""
    name = "levels_4_at_interval"
    P = bs.small_params(name)
    b = bs.small_cloud(name)
    a = bs.folded(b)
    ref_a, ref_b = parity.ref_from_cloud(a, P, mode=2), parity.ref_from_cloud(b, P, mode=2)
    assert int(ref_a["num_nodes"]) == bs.SMALL_FOLDED_NODES
    with two_kernel_tail():
        m = handle(P, bs.TWO_LEVEL, min_points=P["min_points"], max_nodes_hint=bs.SMALL_FOLDED_NODES)
        m.setCloudFirst(a[0])
        ta = dev(a[1:], copy=True)
        for k in range(2):
            m.create2DMap("slope", ta)
            _is_the_oracles_map(m, ref_a, P, ("folded cloud, build", k))
        assert m.last_strategy() == bs.BLOCKED and m.block_layout() == bs.SMALL_SCENES[name]["layout"]
        before = m.retry_count()
        m.create2DMap("slope", dev(b[1:], copy=True))
        _is_the_oracles_map(m, ref_b, P, "unfolded cloud")
        assert m.retry_count() > before and m.last_strategy() == bs.BLOCKED
        after = m.retry_count()
        m.create2DMap("slope", ta)
        _is_the_oracles_map(m, ref_a, P, "folded cloud again")
        _blocked(m, after, "folded cloud again")


# ---- both passes ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["flat_1", "levels_6_padded"])
def test_the_column_pass_and_the_node_pass_agree(name):
    """GNDT_DEBUG_COLUMN_DEST 1 and 0 on the edited cloud: keys, counts, first-seen indices and flags byte for byte, row by row."""
    P = bs.small_params(name)
    ref, want = edited_ref(name, "slope")
    outs = []
    for column_dest in (1, 0):
        with two_kernel_tail(column_dest):
            outs.append(_decided_then_blocked(edited_cloud(name), ref, P, want, (name, "column_dest", column_dest))[1])
    a, b = outs
    assert int(a["num_nodes"]) == int(b["num_nodes"]) == int(ref["num_nodes"])
    for k in EXACT_FIELDS:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k


# ---- poison -----------------------------------------------------------------------------------------------------------------------------

HERE = "tests/test_gpu_blocked_columns.py::"
POISON_IDS = [HERE + "test_every_block_shape_through_the_column_pass[flat_1-slope]",
              HERE + "test_every_block_shape_through_the_column_pass[levels_32_moved_origin-true]",
              HERE + "test_blocks_of_512_nodes_and_of_one[levels_6_padded-slope]",
              HERE + "test_a_table_that_holds_another_clouds_columns[slope]",
              HERE + "test_the_build_after_a_cloud_that_left_the_box",
              HERE + "test_the_build_after_the_staging_rows_ran_out",
              HERE + "test_the_column_pass_and_the_node_pass_agree[flat_1]"]
# measured_s: the whole child (interpreter start to exit) on the MI355X under the regular library; limit_s: three times that, rounded
# up to 10 s (poison_malloc adds a fill and a device synchronisation to every allocation).
GROUP = dict(measured_s=4.88, limit_s=20, ids=POISON_IDS)


def test_every_node_id_of_the_poison_group_is_collected():
    poison_tier.ids_collected(GROUP["ids"])


def test_the_poison_limit_is_three_times_the_measured_time():
    poison_tier.limit_follows_rule(GROUP["measured_s"], GROUP["limit_s"])


@poison_tier.refused_under_variant
@pytest.mark.parametrize("byte", poison_tier.BYTES, ids=poison_tier.BYTE_IDS)
def test_under_poison(byte):
    """POISON_IDS in one child process on the -DGNDT_POISON variant (tests/poisoned_child.py, as tests/test_gpu_poisoned.py runs its
    groups): a column record or an ord_* word that nobody wrote reads as the fill byte there, not as a fresh process's zero."""
    poison_tier.run_group("the column table", GROUP["ids"], GROUP["limit_s"], byte)


# ---- production -------------------------------------------------------------------------------------------------------------------------

def test_a_production_size_box_with_no_option_set():
    """1.1 M points, 8 x 8 x 8 blocks, strategy AUTO, every option at its default: the column pass is what such a build runs."""
    name = "levels_6_padded"
    P = bs.params(name)
    cloud = bs.cloud(name)
    ref = parity.ref_from_cloud(cloud, P, mode=2)
    want = bs.plan(ref, bs.POINTS)
    assert (1 << want["shx"], 1 << want["shy"], 1 << want["shz"]) == (8, 8, 8)
    m = handle(P, min_points=P["min_points"])
    m.setCloudFirst(cloud[0])
    t = dev(cloud[1:], copy=True)
    for k in range(3):
        m.create2DMap("slope", t)
        _is_the_oracles_map(m, ref, P, (name, "build", k))
        if k == 0:
            assert m.block_layout() == want
        else:
            assert m.last_strategy() == bs.BLOCKED and m.retry_count() == 0, (k, m.STRATEGY_NAMES[m.last_strategy()], m.retry_count())
