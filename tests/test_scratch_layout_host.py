"""CPU tier: the scratch layouts of the map's consumers (grid_ndt_amd/csrc/gndt_scratch.hpp's Carver and the layout structs next to
the kernels), instantiated by tests/scratch_layout_shim.cpp over a fake base.  Each layout is restated here from its piece list as plain
running sums, without the carver and without rounding anything up: the layouts run from the widest alignment to the narrowest, so a
carver that pads anywhere, a piece that is carved but not counted and a pair that stops being adjacent all show as a differing offset.
The totals are also the byte counts the entry points summed by hand before the carver, so an allocation is the size it always was."""
import ctypes as C

import numpy as np
import pytest

from tests import host_emulation as he

CLEARANCE, ROUTE, WALK, OBSTACLE, FRONTIER, SEGMENT, MARKS = range(7)
NS = (0, 1, 3, 255, 256, 257, 9216, 9217, 20448, 20449)     # the one-workgroup limits of clearance and route field; odd counts
BOXES = (0, 1, 3)
CLR_FLAG_WORDS, ROUTE_FLAG_WORDS = 1024 + 8, 4096 + 8
TILE = 1024                                                  # rows of a tile of the ordered compaction (kCropTile)

_lib = None


def shim():
    global _lib
    if _lib is None:
        vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
        _lib = he.load_shim("scratch_layout_shim.cpp", "_scratch_layout_shim.so", {
            "slshim_seg_slots": ([u64], u64),
            "slshim_flag_words": ([C.c_int], u32),
            "slshim_layout": ([C.c_int, u64, u64, u64, C.c_int, vp, vp, vp, vp], C.c_int),
        })
    return _lib


def tiles_of(n):
    return (n + TILE - 1) // TILE


def slots_of(n):
    """gndt_segment_scan's cell table: the smallest power of two >= max(2 n, 1024)"""
    s = 1024
    while s < 2 * n:
        s *= 2
    return s


def pieces_of(which, n, a=0, b=0):
    """(the pieces as (name, element size, element alignment, count) in layout order, the members as (name, piece, byte offset into
    it) in declaration order, the hand-summed byte count of the entry point before the carver)"""
    if which == CLEARANCE:
        p = [("step", 8, 4, 4 * n), ("key0", 8, 8, n), ("key1", 8, 8, n), ("flags", 4, 4, CLR_FLAG_WORDS), ("tall", 1, 1, n)]
        return p, None, n * 49 + CLR_FLAG_WORDS * 4
    if which == ROUTE:
        p = [("first", 8, 4, 4 * n), ("rest", 8, 4, 4 * n), ("key", 8, 8, n), ("flags", 4, 4, ROUTE_FLAG_WORDS), ("w", 4, 4, n), ("more", 1, 1, n)]
        return p, None, n * 77 + ROUTE_FLAG_WORDS * 4
    if which == WALK:
        p = [("step", 8, 4, 4 * n), ("key0", 8, 8, n), ("flag", 4, 4, 2), ("tall", 1, 1, n)]
        return p, None, n * 41 + 8
    if which == OBSTACLE:
        p = [("header", 8, 8, 8), ("W", 8, 8, a), ("key0", 8, 8, n), ("key1", 8, 8, n), ("step", 8, 4, 4 * n), ("flags", 4, 4, CLR_FLAG_WORDS),
             ("covers", 4, 4, a), ("list", 4, 4, n), ("tall", 1, 1, n)]
        return p, None, 64 + a * 12 + n * 53 + CLR_FLAG_WORDS * 4
    if which == FRONTIER:
        p = [("parent", 4, 4, n), ("size_at", 4, 4, n), ("tile_cnt", 4, 4, 3 * a), ("open", 1, 1, n), ("slack", 1, 1, 16)]
        return p, None, n * 9 + a * 12 + 16
    if which == SEGMENT:                                 # a = slots, b = tiles; the two pairs are one piece each
        p = [("key|first", 8, 8, a + a // 2), ("count", 4, 4, a), ("slot_root", 4, 4, n), ("parent", 4, 4, n), ("cells_at|points_at", 4, 4, 2 * n),
             ("tile_cnt", 4, 4, 4 * b), ("cls_of", 1, 1, n), ("slack", 1, 1, 16)]
        m = [("key", 0, 0), ("first", 0, 8 * a), ("count", 1, 0), ("slot_root", 2, 0), ("parent", 3, 0), ("cells_at", 4, 0), ("points_at", 4, 4 * n),
             ("tile_cnt", 5, 0), ("cls_of", 6, 0), ("slack", 7, 0)]
        return p, m, a * 16 + n * 17 + b * 16 + 16
    assert which == MARKS
    return [("cover", 8, 8, n), ("cstamp", 4, 4, n), ("slot", 4, 4, n)], None, n * 16


def carved(which, n, a=0, b=0, sizing=False):
    pieces = np.zeros((16, 4), np.uint64)
    members = np.full(16, 0xDEAD, np.uint64)
    counts = np.zeros(2, np.uint32)
    total = C.c_uint64(0)
    rc = shim().slshim_layout(which, n, a, b, int(sizing), pieces.ctypes.data, members.ctypes.data, counts.ctypes.data, C.addressof(total))
    assert rc == 0
    return [tuple(int(v) for v in row) for row in pieces[:counts[0]]], [int(v) for v in members[:counts[1]]], int(total.value)


def check(which, n, a=0, b=0):
    want, members, by_hand = pieces_of(which, n, a, b)
    got, got_members, total = carved(which, n, a, b)
    # the restatement: every piece starts where the one before ends
    offsets, at = [], 0
    for _, elem, _, count in want:
        offsets.append(at)
        at += elem * count
    assert [g[0] for g in got] == offsets, (which, n, a, b)
    assert [g[1:] for g in got] == [w[1:] for w in want], (which, n, a, b)
    assert total == at == by_hand, (which, n, a, b)
    # aligned, disjoint, and the last piece ends at the total
    for (off, elem, align, count), w in zip(got, want):
        assert off % align == 0, (which, n, a, b, w[0])
    spans = sorted((off, off + elem * count) for off, elem, _, count in got)
    assert all(lo2 >= hi1 for (_, hi1), (lo2, _) in zip(spans, spans[1:])), (which, n, a, b)
    assert spans[-1][1] == total
    # the layout's pointers are its pieces (and, in a pair, the second array starts where the first ends)
    members = members or [(name, k, 0) for k, (name, *_) in enumerate(want)]
    assert got_members == [offsets[k] + inside for _, k, inside in members], (which, n, a, b)
    # over a null base the layout only sizes: the same total, every pointer null
    _, null_members, null_total = carved(which, n, a, b, sizing=True)
    assert null_total == total and not any(null_members)
    return dict(zip((w[0] for w in want), offsets)), total


def test_the_shim_has_the_kernels_constants():
    L = shim()
    assert L.slshim_flag_words(0) == CLR_FLAG_WORDS and L.slshim_flag_words(1) == ROUTE_FLAG_WORDS
    for n in NS + (511, 512, 513, 1 << 20):
        assert L.slshim_seg_slots(n) == slots_of(n)


@pytest.mark.parametrize("which", [CLEARANCE, ROUTE, WALK], ids=["clearance", "route_field", "walk"])
def test_row_layouts(which):
    for n in NS:
        check(which, n)


def test_obstacle_layout():
    for n in NS:
        for boxes in BOXES:
            check(OBSTACLE, n, boxes)
        check(MARKS, n + n // 4)                         # obstacle_marks' growth rule
    # the worked case: 5 rows, 3 boxes
    at, total = check(OBSTACLE, 5, 3)
    assert at == {"header": 0, "W": 64, "key0": 88, "key1": 128, "step": 168, "flags": 328, "covers": 4456, "list": 4468, "tall": 4488}
    assert total == 4493


def test_frontier_layout():
    for n in NS:
        check(FRONTIER, n, tiles_of(n))


def test_segment_layout_and_its_two_memset_pairs():
    for n in NS:
        slots, tiles = slots_of(n), tiles_of(n)
        at, _ = check(SEGMENT, n, slots, tiles)
        _, members, _ = carved(SEGMENT, n, slots, tiles)
        key, first, count, _, _, cells_at, points_at, tile_cnt = members[:8]
        # one memset of 12 B a slot clears key | first and ends where count starts; one of 8 B a point clears cells_at | points_at
        assert first == key + 8 * slots and count == key + 12 * slots
        assert points_at == cells_at + 4 * n and tile_cnt == cells_at + 8 * n
