"""GPU tier: the surface patches' reductions where their order-dependent device logic runs (gndt_patch.hpp: k_patch_reduce's wave
carry over the trips of its loop, k_patch_moments<true>'s eight tagged LDS slots and their fallback to memory, the kPatchWaveMin edge,
k_patch_moments<false>), on lattices drawn for it (tests/edge_shapes.py: stripes — every second line of cells empty, so a line of H
cells is a patch of H consecutive rows — and two floors of lines of 256 cells).  Every count derives from edge_shapes.EDGES, which
tests/test_edge_shapes_host.py reads back from the header and the launch.

Every case goes through check and raw of tests/test_gpu_patches.py — labels, counts and every integer field for equality, tails and
front untouched, planes under PLANE_ABS / VAR_REL where well posed ("all") or centroid and normal on the thin floors ("thin") —
through both entry points and under GNDT_DEBUG_PATCH_LDS 1 and 0.  The restatement of the large maps is patch_ref.patches_fast, which
tests/test_patch_fast_ref_host.py holds equal to Map.patches to the bit; the header's row code passed it on the oracle's maps of
these very scenes there.  Every case asserts from the row numbers alone (carry_events, slot_events: which rows meet in which wave,
workgroup and trip of a launch of 512 workgroups) that the path it exists for is taken.

  A  stripes in one and two workgroups, H = 3, 4, 5, 16, 96: below, at and across kPatchWaveMin; 16 patches a wave on 8 slots
  B  two floors over three trips, 266 305 rows: the carry joins, is flushed by the other floor, meets 3 rows of its own patch
  C  stripes of 64 over the trip edge, 134 400 rows: a second trip that brings another patch to every wave and to every slot

Measured on the MI355X (pytest --durations=0):
  A  5 cases  0.01 to 0.02 s each, 24 calls a case (the first case of a process 1.6 s: it loads the library)
  B  2 cases  0.35 s and 0.29 s: the map of 2.4 M points built and exported, one patches_fast, 16 calls
  C  1 case   0.10 s
Plane deviations against the restatement over this tier, the million-row cases of tests/test_gpu_count_edges.py and the reuse case
of tests/test_gpu_scratch_reuse.py (pytest -s prints every scene's): test_gpu_patches.PLANES_MEASURED_EDGES."""
import collections

import numpy as np
import pytest

from tests import edge_shapes as es
from tests import frontier_ref as fr
from tests import patch_ref as pr
from tests.gpu_kit import build, debug_option
from tests.test_gpu_patches import PAD, check, drawn

pytestmark = pytest.mark.gpu

SLOTS, WAVE_MIN = es.EDGES["kPatchSlots"], es.EDGES["kPatchWaveMin"]
TRIP, BLOCK, WAVE = es.PATCH_TRIP, es.EDGES["grid_block"], 64
LDS = "DEBUG_PATCH_LDS"
_worst = dict(centroid=0.0, normal=0.0, var_rel=0.0)


def carry_events(patch_of_row):
    """What k_patch_reduce's waves do with the rows of a map, from the row numbers alone: patch_of_row [n] is the list place of each
    row's patch (-1: none).  Wave w of the rows is slot w % 2048 of the launch in trip w // 2048; a slot takes its groups in row order.
    -> Counter: "alone" (fewer than kPatchWaveMin rows: their own atomics), "alone, beside its carry" (the same while the carry holds
    that very patch), "first" (a combined sum into an empty carry), "join" (into the carry of its own patch), "flush" (another
    patch's carry goes to memory)"""
    w, p, k = es.wave_groups(patch_of_row)
    slots = TRIP // WAVE
    carry, ev = {}, collections.Counter()
    for i in np.lexsort((np.arange(len(w)), w // slots, w % slots)).tolist():
        slot, patch = int(w[i] % slots), int(p[i])
        if patch < 0:
            continue
        if k[i] < WAVE_MIN:
            ev["alone, beside its carry" if carry.get(slot) == patch else "alone"] += 1
        elif carry.get(slot) == patch:
            ev["join"] += 1
        else:
            ev["flush" if slot in carry else "first"] += 1
            carry[slot] = patch
    return ev


def slot_events(patch_of_row):
    """The same for k_patch_moments<true>: workgroup b of the launch holds the rows [256 (b + 512 t), + 256) over its trips t; a
    combined group claims slot place % kPatchSlots or finds it claimed.  The waves of a workgroup are taken in row order here; on the
    device any of them may come first, which changes WHICH patch owns a slot but not how many patches a workgroup turns away — the
    callers assert only that.  -> Counter: "alone", "lds" (claimed, or its own patch's),
    "lds, later trip" (its own patch's slot from an earlier trip), "fallback" (another patch's: to memory), "fallback, later trip",
    "workgroups with a fallback" """
    w, p, k = es.wave_groups(patch_of_row)
    blocks, per = TRIP // BLOCK, BLOCK // WAVE
    tags, ev, fell = {}, collections.Counter(), set()
    for i in np.lexsort((np.arange(len(w)), w // (blocks * per))).tolist():         # trip after trip (a workgroup's waves: any order)
        b, trip, patch = int(w[i] // per % blocks), int(w[i] // (blocks * per)), int(p[i])
        if patch < 0:
            continue
        if k[i] < WAVE_MIN:
            ev["alone"] += 1
            continue
        tag = tags.setdefault((b, patch % SLOTS), (patch, trip))
        if tag[0] == patch:
            ev["lds, later trip" if tag[1] < trip else "lds"] += 1
        else:
            ev["fallback, later trip" if tag[1] < trip else "fallback"] += 1
            fell.add(b)
    ev["workgroups with a fallback"] = len(fell)
    return ev


def both_entries_both_stages(m, ref_map, R, ref, planes, what, **kw):
    """one check through the device and the host entry point, with the moment pass's LDS stage and without -> [(got, ref)] of the four"""
    out = []
    for lds in (1, 0):
        with debug_option(LDS, lds, 1):
            for host in (False, True):
                got, r = check(m, ref_map, R, host=host, planes=planes, ref=ref, what=(what, "lds", lds, "host", host), **kw)
                for key, v in zip(("centroid", "normal", "var_rel"), r.get("deviation", (0.0, 0.0, 0.0))[:2 if planes == "thin" else 3]):
                    _worst[key] = max(_worst[key], v)
                out.append((got, r))
    return out


def large_map(ix, iy):
    """the device's map of the cells (ix, iy), row r cell r -> (m, the export's Rows)"""
    m = build(es.cells_points(ix, iy), fr.P)
    cells = m.export()
    n = len(ix)
    assert cells["num_nodes"] == n and np.array_equal(cells["sx"][:n], ix + 1) and np.array_equal(cells["sy"][:n], iy + 1)
    assert (np.asarray(cells["sz"][:n]) == 1).all()
    return m, pr.Rows(cells)


# ---- A: stripes in one and two workgroups ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H", sorted(es.STRIPES))
def test_stripes_below_at_and_across_the_wave_minimum_on_eight_slots(H):
    lines = es.STRIPES[H]
    n = H * lines
    ix, iy = es.stripes_cells(H, lines)
    m, ref_map, cells = drawn(("stripes", H), lambda: es.cells_points(ix, iy), fr.P)
    assert ref_map.n == n and np.array_equal(ref_map.sx, ix + 1) and np.array_equal(ref_map.sy, iy + 1)           # row r is cell r
    assert n <= 2 * BLOCK and (n > BLOCK) == (H != 3)
    place = np.arange(n) // H
    w, p, k = es.wave_groups(place)
    pairs = {(int(k[i]), int(k[i + 1])) for i in range(len(k) - 1) if p[i] == p[i + 1]}           # a patch split over two waves
    carry, slots = carry_events(place), slot_events(place)
    in_workgroup = np.bincount(np.arange(lines) * H // BLOCK)             # patches a workgroup, where none lies across two (H = 4, 16)
    no_slot = int(np.maximum(in_workgroup - SLOTS, 0).sum())
    if H == 3:
        assert (k < WAVE_MIN).all() and set(carry) == {"alone"} and slots["alone"] == len(k)
    elif H == 4:
        assert (k == WAVE_MIN).all() and lines > SLOTS and WAVE // H > SLOTS
        first_wave = [int(v) for v in p[w == 0]]
        assert first_wave == list(range(2 * SLOTS))                      # one wave: places 0..7 claim the slots, 8..15 find them claimed
        assert BLOCK % H == 0 and slots["fallback"] == no_slot >= WAVE // H - SLOTS and slots["lds"] == lines - no_slot and carry["flush"] > 0
    elif H == 5:
        assert {(4, 1), (3, 2), (2, 3), (1, 4)} <= pairs
        across = [int(w[i + 1]) for i in range(len(k) - 1) if p[i] == p[i + 1] and (k[i], k[i + 1]) == (1, 4)]
        assert BLOCK // WAVE in across                                   # 1 + 4 over the workgroup boundary at row 256
        assert carry["alone"] > 0 and carry["flush"] > 0 and slots["fallback"] > 0
    elif H == 16:
        assert (k == 16).all() and lines > SLOTS and BLOCK % H == 0 and in_workgroup[0] == 2 * SLOTS             # places p and p + 8
        assert slots["fallback"] == no_slot == SLOTS and slots["lds"] == lines - no_slot
    elif H == 96:
        per_patch = np.bincount(p)
        assert (per_patch >= 2).all() and (k >= WAVE_MIN).all() and slots["lds"] > lines and slots["fallback"] == 0       # waves share a slot
    R = pr.rule()
    ref, loop = pr.patches_fast(cells, R), ref_map.patches(R)
    assert np.array_equal(ref["label"], loop["label"]) and ref["patches"].tobytes() == loop["patches"].tobytes()
    for got, r in both_entries_both_stages(m, ref_map, R, ref, "all", ("stripes", H)):
        rec = got["patches"]
        assert tuple(got["counts"]) == (lines, n, lines, 0) and r["compared"] == lines == len(rec)
        assert np.array_equal(got["label"], place * H) and np.array_equal(rec["label"], np.arange(lines) * H)
        assert (rec["nodes"] == H).all() and (rec["points"] == 9 * H).all() and (rec["kind"] == pr.HORIZONTAL | pr.SLOPES_ONLY).all()
    # a cut list: the rows of the patches behind it have no place, between rows and beside waves that have one
    for cap in (1, SLOTS, SLOTS + 1, lines - 1):
        cut = np.where(place < cap, place, -1)
        assert (cut >= 0).any() and (cut < 0).any() == (cap < lines)      # (the five lines of H = 96 fit a list of 8 or 9 whole)
        for got, r in both_entries_both_stages(m, ref_map, R, ref, "all", ("stripes", H, "cap", cap), cap=cap):
            assert int(got["counts"][0]) == lines and len(got["patches"]) == min(cap, lines) == r["compared"]
    # nothing listed: the labels and the counts of rows and patches stay, the list is not touched
    for got, r in both_entries_both_stages(m, ref_map, R, ref, "all", ("stripes", H, "min_size"), min_size=H + 1):
        assert tuple(got["counts"]) == (0, n, lines, 0) and len(got["patches"]) == 0 and np.array_equal(got["label"], place * H)
    print("worst plane deviations so far:", _worst)


# ---- B: two floors over three trips ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("a", es.FLOORS_A, ids=["30_rows_into_the_wave", "3_rows_into_the_wave"])
def test_two_floors_over_three_trips_of_the_reductions(a):
    n, into = es.FLOORS_N, a % WAVE
    assert n > 2 * TRIP and TRIP < a < 2 * TRIP and into in (30, 3) and (n - 1) % WAVE == 0
    ix, iy = es.floors_cells(a, n)
    floor = (np.arange(n) >= a).astype(np.int64)
    ev = carry_events(floor)
    # trip 2: the waves below a join floor 0's carry; the wave across a flushes it for floor 1 (or meets 3 rows of floor 0 beside
    # the carry that holds floor 0, and then flushes); the waves above flush; trip 3 joins again, and ends on one row
    # (the waves below a in trip 2 and the wave behind the one across a in trip 3 join; the last row's wave carries floor 1 by then)
    joins = (a - TRIP) // WAVE + (1 if into >= WAVE_MIN else 0) + 1              # whole waves below a, the wave across a, one of trip 3
    assert ev["first"] == TRIP // WAVE and ev["join"] == joins and ev["flush"] == TRIP // WAVE, ev
    assert ev["alone, beside its carry"] == (1 if into >= WAVE_MIN else 2) and ev["alone"] == 0, ev
    last_wave = es.wave_groups(floor)
    assert int(last_wave[2][-1]) == 1 and int(last_wave[0][-1]) // (TRIP // WAVE) == 2               # one row, in trip 3
    sl = slot_events(floor)
    assert sl["lds, later trip"] > 0 and sl["fallback"] + sl["fallback, later trip"] == 0            # places 0 and 1: a slot each
    m, rows = large_map(ix, iy)
    R = pr.rule()
    ref = pr.patches_fast(rows, R)
    want = ref["patches"]
    assert want["label"].tolist() == [0, a] and want["nodes"].tolist() == [a, n - a] and want["points"].tolist() == [9 * a, 9 * (n - a)]
    for f, sel in ((0, floor == 0), (1, floor == 1)):
        assert (int(want["sum_px"][f]), int(want["sum_py"][f]), int(want["sum_pz"][f])) == (int(ix[sel].sum()), int(iy[sel].sum()), 0)
        assert (int(want["sx_min"][f]), int(want["sx_max"][f])) == (int(ix[sel].min()) + 1, int(ix[sel].max()) + 1)
    for got, r in both_entries_both_stages(m, None, R, ref, "thin", ("floors", a), cap=2 + PAD):
        assert tuple(got["counts"]) == (2, n, 2, 0) and pr.same_integers(got["patches"], want)
    for got, r in both_entries_both_stages(m, None, R, ref, "thin", ("floors", a, "cap 1"), cap=1):
        assert int(got["counts"][0]) == 2 and got["patches"]["label"].tolist() == [0]
    # min_size: a + 1 lists neither floor (the first has a rows), n - a + 1 the first alone — the second's rows have no place then
    for got, r in both_entries_both_stages(m, None, R, ref, "thin", ("floors", a, "min_size a + 1"), min_size=a + 1, cap=2 + PAD):
        assert tuple(got["counts"]) == (0, n, 2, 0) and len(got["patches"]) == 0
    assert n - a < a and carry_events(np.where(floor == 0, 0, -1))["flush"] == 0
    for got, r in both_entries_both_stages(m, None, R, ref, "thin", ("floors", a, "min_size n - a + 1"), min_size=n - a + 1, cap=2 + PAD):
        assert tuple(got["counts"]) == (1, n, 2, 0) and got["patches"]["nodes"].tolist() == [a]
    print("worst plane deviations so far:", _worst)


# ---- C: stripes over the trip edge -------------------------------------------------------------------------------------------------

def test_stripes_of_a_wave_over_the_trip_edge():
    H, lines = es.TRIP_STRIPES
    n = H * lines
    behind = n - TRIP
    assert H == WAVE and TRIP < n < 2 * TRIP and behind % BLOCK == 0
    place = np.arange(n) // H
    ev, sl = carry_events(place), slot_events(place)
    # every wave of the second trip brings another patch than its first: it flushes, never joins; and finds its slot another patch's
    assert ev["flush"] == behind // WAVE and ev["join"] == 0 and ev["first"] == TRIP // WAVE
    assert sl["fallback, later trip"] == behind // WAVE and sl["workgroups with a fallback"] == behind // BLOCK and sl["lds"] == TRIP // WAVE
    m, rows = large_map(*es.stripes_cells(H, lines))
    R = pr.rule()
    ref = pr.patches_fast(rows, R)
    assert len(ref["patches"]) == lines and np.array_equal(ref["patches"]["label"], np.arange(lines) * H)
    for got, r in both_entries_both_stages(m, None, R, ref, "all", "trip stripes", cap=lines + PAD):
        assert tuple(got["counts"]) == (lines, n, lines, 0) and r["compared"] == lines == len(got["patches"])
    for got, r in both_entries_both_stages(m, None, R, ref, "all", "trip stripes, cap", cap=lines - 1):
        assert int(got["counts"][0]) == lines and r["compared"] == lines - 1 == len(got["patches"])
    print("worst plane deviations so far:", _worst)
