"""CPU tier of the count-edge shapes (tests/edge_shapes.py, used by tests/test_gpu_count_edges.py): the constants the shapes derive from
are the headers' and the launches', the lattice generator is frontier_ref.cells_cloud bit for bit, the cyclic batches' multiplicities
add up, and — on the restatements alone, over the oracle's map — the items of a batch's second grid-stride trip hold every kind of
answer the GPU tier then compares.

A failure of the first two tests means: a constant or a launch was retuned; derive tests/edge_shapes.py's counts from it again."""
import os
import re

import numpy as np
import pytest

from tests import cast_ref as cf
from tests import clear_ref as cr
from tests import clearance_ref as clr
from tests import edge_shapes as es
from tests import frontier_ref as fr
from tests import parity
from tests import query_ref as qr

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "grid_ndt_amd", "csrc")


def _text(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _const(text, name):
    """the initialiser of `constexpr <type> name = ...;` evaluated over the constants of EDGES (kCropT * kCropV)"""
    m = re.search(r"constexpr\s+\w+\s+" + name + r"\s*=\s*([^;]+);", text)
    assert m, name
    return int(eval(re.sub(r"(?<=\d)u\b", "", m.group(1)), {"__builtins__": {}}, dict(es.EDGES)))


def test_the_headers_constants_are_the_tables():
    crop, score, derivs, handle, kernels = (_text(n) for n in ("gndt_crop.hpp", "gndt_score.hpp", "gndt_score_derivs.hpp",
                                                                 "gndt_handle.hpp", "gndt_kernels.hpp"))
    E = es.EDGES
    for name in ("kCropT", "kCropV", "kCropTile", "kCropScanT"):
        assert _const(crop, name) == E[name], name
    for name in ("kScoreTile", "kScoreReduceBlock"):
        assert _const(score, name) == E[name], name
    # the reduce loops' strides, and the unrolled loads they stand for
    m = re.search(r"t0 < tiles; t0 \+= (\d+)u \* kScoreReduceBlock\)", score)
    assert m and int(m.group(1)) == E["score_reduce_unroll"]
    assert re.search(r"for \(uint32_t j = 0; j < %du; \+\+j\)" % E["score_reduce_unroll"], score)
    m = re.search(r"t0 < tiles; t0 \+= (\d+)u \* kScoreReduceBlock\)", derivs)
    assert m and int(m.group(1)) == E["derivs_reduce_unroll"]
    # the one-workgroup scans walk their tiles in chunks of kCropScanT
    assert "base < tiles; base += kCropScanT" in crop and "base < tiles; base += kCropScanT" in _text("gndt_frontier.hpp")
    # grid_for's defaults
    m = re.search(r"inline int grid_for\(uint64_t work, int block = kBlock, int max_blocks = ([^)]+)\)", handle)
    assert m and eval(m.group(1), {"__builtins__": {}}) == E["grid_max_blocks"]
    assert _const(kernels, "kBlock") == E["grid_block"]
    assert E["grid_block"] * E["grid_max_blocks"] == E["grid_cap"] == es.CAP


def _grid_for_calls(text):
    """the argument lists of every grid_for( call of a file, parentheses balanced"""
    out = []
    for m in re.finditer(r"grid_for\(", text):
        depth, j = 1, m.end()
        while depth:
            depth += {"(": 1, ")": -1}.get(text[j], 0)
            j += 1
        out.append(text[m.end():j - 1])
    return out


def test_the_launches_still_cap_at_the_tables_count():
    explicit = ("gndt_api_cast.hip", "gndt_api_clear.hip", "gndt_api_raster.hip", "gndt_api_query.hip", "gndt_api_frontier.hip")
    for name in explicit:
        calls = _grid_for_calls(_text(name))
        assert calls, name
        for c in calls:
            assert re.fullmatch(r".+, 256, 2048", c), (name, c)
    for name in ("gndt_api_coarsen.hip", "gndt_api_merge.hip", "gndt_api_crop.hip"):
        calls = _grid_for_calls(_text(name))
        assert calls, name
        for c in calls:
            assert "," not in c, (name, c)                              # grid_for's defaults
    merges = re.findall(r"hipLaunchKernelGGL\(k_stats_merge, dim3\(grid_for\(([^()]*(?:\([^()]*\))?[^()]*)\)\)", _text("gndt_api_table.hip"))
    assert len(merges) >= 2 and all("," not in c for c in merges), merges
    # the query's loop strides by the grid times ILP, the launch covers ceil(n / ILP) threads
    assert "i0 += gsz * ILP" in _text("gndt_query.hpp") and "grid_for((n + ILP - 1) / ILP, 256, 2048)" in _text("gndt_api_query.hip")


def test_the_patch_reductions_constants_and_launch_are_the_tables():
    E = es.EDGES
    patch = _text("gndt_patch.hpp")
    for name in ("kPatchSlots", "kPatchWaveMin"):
        assert _const(patch, name) == E[name], name
    # the one launch of fewer workgroups carries both reductions; every other row pass of the call is the frontiers' launch
    calls = _grid_for_calls(_text("gndt_api_patch.hip"))
    few = [c for c in calls if re.fullmatch(r"n, 256, \d+", c) and not c.endswith(", 2048")]
    assert few == ["n, %d, %d" % (E["grid_block"], E["patch_reduce_blocks"])], calls
    assert "n, 256, 2048" in calls
    assert E["patch_reduce_cap"] == E["grid_block"] * E["patch_reduce_blocks"] == es.PATCH_TRIP
    assert E["kPatchSlots"] & (E["kPatchSlots"] - 1) == 0


@pytest.mark.parametrize("H,lines", [(3, 70), (4, 70), (5, 70), (16, 20), (64, 30), (96, 5)])
def test_premise_stripes_are_a_patch_a_line_all_well_posed(H, lines):
    """on the oracle's map, by the restatement alone: row r is cell r, line i is the patch of the rows i H .. i H + H - 1 under every
    connectivity, every patch well posed, horizontal and of slopes only"""
    from tests import patch_ref as pr
    ix, iy = es.stripes_cells(H, lines)
    cells = parity.ref_from_cloud(es.cells_points(ix, iy), es.P)
    n = H * lines
    assert cells["num_nodes"] == n and np.array_equal(cells["sx"][:n], ix + 1) and np.array_equal(cells["sy"][:n], iy + 1)
    m = pr.Map(cells)
    for conn in (1, 3):
        R = pr.rule(pr.NODES, conn)
        ref = m.patches(R)
        recs, counts = pr.listed(ref)
        assert tuple(counts) == (lines, n, lines, 0)
        assert np.array_equal(ref["label"], np.arange(n) // H * H) and (recs["nodes"] == H).all()
        assert np.array_equal(recs["label"], np.arange(lines) * H) and (recs["kind"] == pr.HORIZONTAL | pr.SLOPES_ONLY).all()
        assert all(pr.well_posed(m, R, ref, rec)[0] for rec in recs)


def test_premise_floors_are_two_patches_labelled_0_and_a():
    from tests import patch_ref as pr
    for a, n in ((300, 700), (256, 257), (1, 600)):
        ix, iy = es.floors_cells(a, n)
        assert len(ix) == n and iy.max() < es.FLOOR_LINE and ix[a] - ix[a - 1] == 3 and iy[a] == 0
        cells = parity.ref_from_cloud(es.cells_points(ix, iy), es.P)
        assert cells["num_nodes"] == n and np.array_equal(cells["sx"][:n], ix + 1) and np.array_equal(cells["sy"][:n], iy + 1)
        ref = pr.Map(cells).patches(pr.rule())
        assert ref["patches"]["label"].tolist() == [0, a] and ref["patches"]["nodes"].tolist() == [a, n - a]
        assert np.array_equal(ref["label"], np.where(np.arange(n) < a, 0, a))
    w, p, k = es.wave_groups(np.arange(700) >= 300)
    assert (w[:6].tolist(), p[:6].tolist(), k[:6].tolist()) == ([0, 1, 2, 3, 4, 4], [0, 0, 0, 0, 0, 1], [64, 64, 64, 64, 44, 20]) and k.sum() == 700


def test_lattice_points_is_cells_cloud_bit_for_bit():
    W, H = 25, 41
    holes = [(3, 7), (3, 8), (11, 0), (24, 40), (0, 0), (12, 20)]
    cells = [(ix, iy) for ix in range(W) for iy in range(H) if (ix, iy) not in set(holes)]
    want = fr.cells_cloud(cells)
    got = es.lattice_points(W, H, holes)
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape == (1 + 9 * (W * H - len(holes)), 3)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # without holes: clearance_ref.lattice_cloud's floor
    assert np.array_equal(es.lattice_points(7, 5).view(np.uint32), clr.lattice_cloud(7, 5).view(np.uint32))
    # the pitch holes stay off the border and are distinct
    ph = es.pitch_holes(1024, 1024)
    assert len(set(ph)) == len(ph) > 500 and all(0 < ix < 1023 and 0 < iy < 1023 for ix, iy in ph)


def test_cyclic_batches_and_their_multiplicities():
    base = np.arange(es.BASE) * 3 + 1
    counts = set(es.CAST_COUNTS + es.QUERY_COUNTS + es.SCORE_COUNTS + (es.QUERY_ILP4_COUNT, 0, es.BASE - 1, es.BASE, es.BASE + 1))
    for n in sorted(counts):
        mult = es.multiplicity(n)
        assert mult.sum() == n and mult.min() >= n // es.BASE and mult.max() <= n // es.BASE + 1
        if n <= es.CAP + 65:
            b = es.cyclic(base, n)
            assert len(b) == n and np.array_equal(np.bincount((b - 1) // 3, minlength=es.BASE), mult)
            assert n == 0 or (b[0] == 1 and b[-1] == base[(n - 1) % es.BASE])
    # the second trip holds other items than the first at every lane: item CAP + l is not item l
    lanes = np.arange(es.BASE)
    assert ((es.CAP + lanes) % es.BASE != lanes % es.BASE).all()
    assert es.tail_items(es.CAP + 65).tolist() == [(es.CAP + k) % es.BASE for k in range(65)] and es.tail_items(es.CAP).size == 0
    assert es.CAP % es.BASE == 384 and (4 * es.CAP) % es.BASE == 1536


@pytest.fixture(scope="module")
def small():
    """the oracle's map of the small lattice"""
    cells = parity.ref_from_cloud(es.small_cloud(), es.P)
    W, H, _ = clr.LATTICES[es.SMALL]
    assert cells["num_nodes"] == W * H and ((cells["flags"] & 2) != 0).all()
    return cells


def test_premise_cast_second_trip_holds_a_hit_a_miss_and_a_skipped_ray(small):
    sensor, origins, ends = es.cast_base()
    for mode in (cf.VOXEL, cf.NDT):
        for o in (sensor, origins):
            want = cf.cast(small, es.ORIGIN, es.P["grid_len"], es.P["z_len"], o, ends, mode=mode)
            st = want["status"]
            assert (st == cf.HIT).sum() > 1000 and (st == cf.MISS).sum() > 500 and (st == cf.SKIPPED).sum() > 100
            assert st[es.tail_items(es.CAP + 1)].tolist() == [cf.HIT]                  # n = 524 289: its one item of the second trip
            tail = st[es.tail_items(es.CAP + 65)]
            assert {cf.HIT, cf.MISS, cf.SKIPPED} <= set(tail.tolist())
            assert len(set(st[:1].tolist()) | set(st[:65].tolist())) == 3               # and the wave-sized batches see all three


def test_premise_query_second_trip_holds_a_matched_and_an_unmatched_point(small):
    pts = es.query_base()
    args = (small, pts, es.ORIGIN, es.P["grid_len"], es.P["z_len"])
    for rows in (qr.node_rows(*args), qr.nearest_slope_rows(*args)):
        assert rows[es.tail_items(es.CAP + 1)].tolist()[0] >= 0
        assert rows[es.tail_items(es.QUERY_ILP4_COUNT, first=4 * es.CAP)].tolist()[0] >= 0
        for ilp in (1, 4):                     # a thread's ILP items lie one grid apart: the last of them at ILP 4 are items >= 3 CAP
            tail = rows[np.arange(ilp * es.CAP - 64, ilp * es.CAP + 1) % es.BASE]
            assert (tail >= 0).any() and (tail == qr.NO_ROW).any()
    assert (qr.node_rows(*args) != qr.nearest_slope_rows(*args)).any()


def test_premise_clear_second_trip_protects_and_passes_rows(small):
    sensor, pts = es.clear_base()
    tail = pts[es.tail_items(es.CAP + 65)]
    words, rays, skipped = cr.passes(small, es.ORIGIN, es.P["grid_len"], es.P["z_len"], sensor, tail)
    assert rays > 50 and skipped > 0
    assert ((words & cr.PROTECTED) != 0).sum() > 10 and ((words & ~cr.PROTECTED) > 0).sum() > 50
    one, rays1, _ = cr.passes(small, es.ORIGIN, es.P["grid_len"], es.P["z_len"], sensor, pts[es.tail_items(es.CAP + 1)])
    assert rays1 == 1 and ((one & cr.PROTECTED) != 0).sum() == 1 and ((one & ~cr.PROTECTED) > 0).sum() > 1
    # the cyclic sum equals the restatement of the batch written out, where that is small enough to write out
    for n in (1, 65, 2 * es.BASE + 17):
        want = cr.passes(small, es.ORIGIN, es.P["grid_len"], es.P["z_len"], sensor, es.cyclic(pts, n))
        got = es.clear_words(small, sensor, pts, n)
        assert np.array_equal(got[0], want[0]) and got[1:] == want[1:], n
    # a clear with min_passes = 3 at n = 524 289 drops rows, keeps rows, and spares protected rows with as many passes
    words, _, _ = es.clear_words(small, sensor, pts, es.CAP + 1)
    drop = cr.cleared_rows(words, 3)
    assert 0 < drop.sum() < len(words) and (((words & cr.PROTECTED) != 0) & ((words & ~cr.PROTECTED) >= 3)).any()
