"""GPU tier: path walks (gndt_walk_paths_device / gndt_walk_paths, TwoDmap.walk_paths).  Every map is built on the device; every field
of every path and every row is compared for equality with the restatement (tests/walk_ref.py) on the handle's own export, through
both kernel variants (the step found with the gates, the step read from the per-call table) and both entry points, into outputs
over-allocated with a sentinel tail that must stay untouched.  Hand-drawn maps whose answer is known beforehand — a corridor between
plateaus, a pit column taller than the step mask, two storeys with an exact tie, a low ceiling — then wave and workgroup edges of K,
terminators, strides, row caps, the codec's edge, the step guard, a real clearance field, crop / update / another robot, a second
stream, the Python interface and every refused argument; more paths than one trip of the kernel's grid-stride loop, and the table
choice left at its default on both sides of its threshold and at it.  No tolerance anywhere: the one step that is not IEEE arithmetic is the
gates' acosf, and every compared scene keeps its angle decisions more than 1e-3 degrees from the threshold."""
import ctypes as C

import numpy as np
import pytest

from grid_ndt_amd import scenes
from tests import clearance_ref as cr
from tests import frontier_ref as fr
from tests import walk_ref as wr
from tests.gpu_kit import Padded, PaddedCall, build, debug_option, dev, robot_arg, to_np

pytestmark = pytest.mark.gpu

ERR_INVALID = 1
ATOMIC = 1
SENTINEL = 0x5A5A5A5A
PAD = 3                      # sentinel entries behind the outputs
MARGIN = 1e-3
START = {"nearest_slope": 1, "node": 2}
_scenes = {}


def step_table(on):
    """gndt_debug_set_option(GNDT_DEBUG_WALK_STEP_TABLE, .) for a block; the default comes back whatever happens in it"""
    return debug_option("DEBUG_WALK_STEP_TABLE", 1 if on else 0, 2)


def raw(m, paths, robot=None, start_mode="nearest_slope", overhead=False, hops=None, min_hops=0, max_steps=0, row_cap=0, stream=None, host=False,
        reserved=(0,) * 4, checks=None, mode=None):
    """The C entry points, info K + PAD entries and rows K * row_cap + PAD words of sentinel -> (rc, info [K], rows [K, row_cap],
    untouched: the tails still hold the sentinel)"""
    from grid_ndt_amd._lib import WalkParams
    paths = np.ascontiguousarray(paths, np.float32)
    K, T, sf = paths.shape
    prm = WalkParams(START[start_mode] if mode is None else mode, (1 if overhead else 0) if checks is None else checks, min_hops, max_steps,
                     (C.c_uint32 * 4)(*reserved))
    info, rows = Padded(K, words=12, back=PAD, fill=SENTINEL), Padded(K * row_cap, back=PAD, fill=SENTINEL)
    hp = None if hops is None else np.ascontiguousarray(hops).view(np.uint32)
    rc = PaddedCall(host, stream, wait_for_current=True)(m._L.gndt_walk_paths, m._L.gndt_walk_paths_device, m._h, paths, K, T, 4 * sf,
                                                         robot_arg(robot, cr.ROBOT), C.byref(prm), hp, rows if row_cap else None, row_cap, info)
    return rc, info.body.view(wr.INFO_DTYPE), rows.body.reshape(K, row_cap), info.untouched() and rows.untouched()


def check(m, w, paths, what="", entries=(False, True), stream=None, **kw):
    """both variants through the given entry points against the restatement -> (the restatement's info, rows, walked)"""
    ref_kw = {k: v for k, v in kw.items() if k != "robot"}
    want_info, want_rows, walked = w.walk(paths, **ref_kw)
    for table in (False, True):
        with step_table(table):
            for host in entries:
                rc, info, rows, untouched = raw(m, paths, host=host, stream=None if host else stream, **kw)
                tag = (what, "table" if table else "inline", "host" if host else "device")
                assert rc == 0, (tag, m._L.gndt_last_error(m._h))
                wr.same(info, rows, want_info, want_rows, tag)
                assert untouched, tag
    return want_info, want_rows, walked


def drawn(name, make, P=fr.P, robot=None):
    """a map drawn from a cloud -> (m, restatement, export)"""
    key = (name, tuple(sorted((robot or {}).items())))
    if key not in _scenes:
        base = [v for k, v in _scenes.items() if k[0] == name]
        if base:
            m, _, cells, cloud = base[0]
        else:
            cloud = make()
            m = build(cloud, P)
            cells = m.export()
        w = wr.Walker(cells, cloud[0, :3], P["grid_len"], P["z_len"], robot)
        assert w.f.angle_margin_deg > MARGIN, (name, w.f.angle_margin_deg)
        _scenes[key] = (m, w, cells, cloud)
    return _scenes[key][:3]


def flat_cloud(cells):
    """nine points a cell at one exact z, the origin (0, 0, 0) first: cell (ix, iy) is column (ix + 1, iy + 1) for ix, iy >= 0, its mean
    the cell's centre and z to the bit, the lattice corners binary fractions"""
    pts = [[0.0, 0.0, 0.0]]
    for ix, iy, z in cells:
        for a in (0.125, 0.25, 0.375):
            for b in (0.125, 0.25, 0.375):
                pts.append([ix * 0.5 + a, iy * 0.5 + b, z])
    return np.ascontiguousarray(np.float32(pts))


def row_of(cells, sx, sy, nth=0):
    return int(np.flatnonzero((cells["sx"] == sx) & (cells["sy"] == sy))[nth])


def path(*xy, z=0.06):
    return np.float32([[[x, y, z] for x, y in xy]])


# ---- maps whose answer is known beforehand -------------------------------------------------------------------------------------------

def test_corridor_along_across_and_out_of_the_end():
    m, w, cells = drawn("corridor", cr.corridor_cloud, cr.CORRIDOR_P)
    assert cells["num_nodes"] == 156
    # cell ix covers x in 0.01 + [ix, ix + 1) / 2: the corridor's floor is ix = 0 .. 6 (columns 1 .. 7), iy = 0 .. 11 (columns 1 .. 12)
    paths = np.concatenate([path((1.76, 0.3), (1.76, 5.7), (1.76, 5.7)),          # along the corridor
                            path((1.76, 2.76), (4.26, 2.76), (4.3, 2.76)),        # into the plateau's step on the right
                            path((1.76, 5.3), (1.76, 7.0), (1.76, 7.2)),          # out of the corridor's end
                            path((0.3, 2.76), (-1.3, 2.76), (0.3, 2.76))])        # across index 0 of x: the step on the left
    info, rows, walked = check(m, w, paths, "corridor", row_cap=12)
    assert info["status"].tolist() == [wr.DONE, wr.BLOCKED, wr.LEFT_MAP, wr.BLOCKED]
    assert info["stop_side"].tolist() == [wr.NO_SIDE, 2, 1, 3] and info["steps"].tolist() == [11, 3, 1, 0]
    assert info["waypoints"].tolist() == [3, 1, 1, 1]
    assert [int(cells["sy"][r]) for r in walked[0]] == list(range(1, 13)) and {int(cells["sx"][r]) for r in walked[0]} == {4}
    assert [int(cells["sx"][r]) for r in walked[1]] == [4, 5, 6, 7] and int(cells["sx"][info["end_row"][3]]) == 1
    assert info["length"][0] > 5.4 and info["length"][0] < 5.6 and info["climb"][0] < 0.11
    # the rows a caller keeps: none, one, all of them, fewer
    for cap in (0, 1, 12, 5):
        got, rws, _ = check(m, w, paths[:1], ("cap", cap), row_cap=cap)
        assert got["steps"][0] + 1 == 12 and rws.shape == (1, cap)
        assert rws[0].tolist() == walked[0][:cap]
    # the guard: the walk needs 11 steps
    got, _, _ = check(m, w, paths[:1], "11 steps", max_steps=11)
    assert got["status"][0] == wr.DONE and got["steps"][0] == 11
    got, rws, _ = check(m, w, paths[:1], "10 steps", max_steps=10, row_cap=12)
    assert got["status"][0] == wr.LIMIT and got["steps"][0] == 10 and got["waypoints"][0] == 1 and rws[0, 11] == wr.NO_ROW


def test_a_step_through_a_pit_column_taller_than_the_step_mask():
    """pit_cloud: cells ix = 0 .. 7 at iy = 0, cell 3's column 37 rows of which the floor's slope is the last (beyond bit 31 of a step
    mask: the table variant has to walk the column's rest with the gates), cell 7 a metre higher"""
    m, w, cells = drawn("pit", cr.pit_cloud)
    col = np.flatnonzero((cells["sx"] == 4) & (cells["sy"] == 1))
    slopes = np.flatnonzero((cells["flags"] & 2) != 0)
    assert len(col) == 37 and [int(r - col[0]) for r in slopes if r in col] == [36]
    paths = np.concatenate([path((0.25, 0.25), (3.25, 0.25)), path((3.25, 0.25), (0.25, 0.25)), path((2.75, 0.25), (3.8, 0.25)),
                            path((1.75, 0.25), (1.8, 0.3))])
    info, rows, walked = check(m, w, paths, "pit", row_cap=8)
    assert info["status"].tolist() == [wr.DONE, wr.DONE, wr.BLOCKED, wr.DONE] and info["steps"].tolist() == [6, 6, 1, 0]
    assert [int(cells["sx"][r]) for r in walked[0]] == [1, 2, 3, 4, 5, 6, 7] and walked[0][3] == col[36] and walked[1] == walked[0][::-1]
    assert info["stop_side"][2] == 2 and info["start_row"][3] == col[36]


def _tie(first):
    z = (0.5, 1.5) if first == "low" else (1.5, 0.5)
    return lambda: flat_cloud([(0, 0, 1.0), (1, 0, z[0]), (1, 0, z[1]), (2, 0, 1.5), (0, 1, 1.0), (1, 1, 1.0), (2, 1, 1.0)])


@pytest.mark.parametrize("first", ["low", "high"])
def test_two_storeys_least_dz_and_a_tie_to_the_smaller_row(first):
    """Column (2, 1) holds a slope half a metre under and one half a metre over the start's 1.0 m, both means exact: with a reach of
    0.6 m both are steps and |dz| ties to the bit, so the smaller row is taken — the lower storey when it was seen first (from there
    the 1.5 m of column (3, 1) is out of reach), the upper one otherwise.  From (2, 2) at 1.0 m the step into (2, 1) is the same tie;
    from a start at 1.4 m ... there is none: NEAREST_SLOPE only picks the start."""
    robot = dict(reachable_height=0.6)
    m, w, cells = drawn("tie_" + first, _tie(first), robot=robot)
    lo, hi = (row_of(cells, 2, 1, 0), row_of(cells, 2, 1, 1)) if first == "low" else (row_of(cells, 2, 1, 1), row_of(cells, 2, 1, 0))
    assert cells["mean"][lo][2] == np.float32(0.5) and cells["mean"][hi][2] == np.float32(1.5) and cells["mean"][row_of(cells, 1, 1)][2] == np.float32(1.0)
    paths = np.concatenate([path((0.25, 0.25), (1.25, 0.25), z=1.0), path((0.75, 0.75), (0.75, 0.25), z=1.0),
                            path((1.25, 0.25), (0.3, 0.25), z=1.5), path((1.25, 0.75), (1.25, 0.25), z=1.0)])
    info, rows, walked = check(m, w, paths, "tie", robot=robot, row_cap=3)
    taken = min(lo, hi)
    assert walked[0][1] == taken and walked[1][1] == taken
    assert info["status"][0] == (wr.BLOCKED if first == "low" else wr.DONE) and info["steps"][0] == (1 if first == "low" else 2)
    assert walked[2][:2] == [row_of(cells, 3, 1), hi] and info["status"][2] == wr.DONE        # 1.5 -> 1.5 (0 < 1.0), then down 0.5
    assert info["climb"][2] == np.float32(0.5) and info["status"][3] == wr.DONE and info["climb"][3] == np.float32(0.5)
    # the default robot (reach 0.15) has no step into column (2, 1) at all
    m2, w2, _ = drawn("tie_" + first, _tie(first))
    got, _, _ = check(m2, w2, paths[:2], "tie, default robot")
    assert got["status"].tolist() == [wr.BLOCKED, wr.BLOCKED] and got["stop_side"].tolist() == [2, 0]


def _ceiling():
    floor = [(ix, iy, 0.26) for ix in range(-4, 4) for iy in range(-3, 3)]
    lid = [(ix, iy, 0.56) for ix in range(-4, -1) for iy in range(-3, 3)]           # 0.3 m above the floor's first three lines
    return fr.cells_cloud(floor + lid, 5)


def test_a_low_ceiling_stops_the_walk_only_when_asked():
    m, w, cells = drawn("ceiling", _ceiling)
    paths = np.concatenate([path((1.25, 0.25), (-1.75, 0.25), z=0.26), path((-1.25, 0.25), (1.25, 0.25), z=0.26)])
    info, _, walked = check(m, w, paths, "ceiling, check off")
    assert info["status"].tolist() == [wr.DONE, wr.DONE] and info["steps"].tolist() == [6, 5]
    info, _, walked = check(m, w, paths, "ceiling, check on", overhead=True)
    assert info["status"].tolist() == [wr.OVERHEAD, wr.OVERHEAD] and info["steps"].tolist() == [4, 0]
    assert int(cells["sx"][info["end_row"][0]]) == -2 and info["end_row"][1] == info["start_row"][1]
    slim = dict(radius=0.1)                                                           # 0.3 m is not within 0.2 m
    ms, ws, _ = drawn("ceiling", _ceiling, robot=slim)
    info, _, _ = check(ms, ws, paths, "ceiling, slim", overhead=True, robot=slim)
    assert info["status"].tolist() == [wr.DONE, wr.DONE]


def _ground():
    return flat_cloud([(ix, iy, 0.125) for ix in range(-6, 6) for iy in range(-6, 6)])


def test_lattice_corners_zero_length_segments_and_the_codecs_edge():
    m, w, cells = drawn("ground", _ground)
    z = 0.125
    paths = np.concatenate([path((0.25, 0.25), (0.75, 0.75), (0.75, 0.75), z=z),              # through the corner (0.5, 0.5): x first
                            path((-0.25, -0.25), (0.25, 0.25), (-0.75, 0.25), z=z),           # through the origin: index 0 of both axes
                            path((0.25, 0.25), (0.25, 0.25), (0.3, 0.3), z=z),                # a segment of no length, two points a column
                            path((0.25, 0.25), (0.75, 0.25), (1e9, 0.25), z=z),               # a waypoint the codec cannot key
                            path((0.25, 0.25), (0.75, 0.25), (2000.0, 0.25), z=z),            # keyed, far outside the map
                            path((-0.25, 0.75), (0.25, -0.75), (0.25, 0.25), z=z)])
    info, rows, walked = check(m, w, paths, "corners", row_cap=6)
    col = lambda r: (int(cells["sx"][r]), int(cells["sy"][r]))
    assert [col(r) for r in walked[0]] == [(1, 1), (2, 1), (2, 2)] and info["waypoints"][0] == 3
    assert [col(r) for r in walked[1]] == [(-1, -1), (1, -1), (1, 1), (-1, 1), (-2, 1)]
    assert info["steps"][2] == 0 and info["status"][2] == wr.DONE and info["waypoints"][2] == 3 and info["length"][2] == 0
    assert info["status"][3] == wr.LEFT_MAP and info["stop_side"][3] == wr.NO_SIDE and info["steps"][3] == 1 and info["waypoints"][3] == 2
    assert info["status"][4] == wr.LEFT_MAP and info["stop_side"][4] == 2 and col(info["end_row"][4]) == (6, 1)
    assert info["status"][5] == wr.DONE


@pytest.mark.parametrize("K,T,sf", [(1, 33, 3), (63, 2, 4), (64, 1, 3), (65, 33, 4), (257, 2, 3), (257, 1, 4)])
def test_wave_and_workgroup_edges_of_K_terminators_and_strides(K, T, sf):
    from tests.test_walk_host import random_paths
    m, w, cells = drawn("ground", _ground)
    rng = np.random.default_rng(K * 100 + T)
    paths = random_paths(rng, K, T, (-3.0, -3.0), (3.0, 3.0), 0.1, 0.2, reach=0.45, sf=sf)
    paths[0, 0, :2] = 0.25                                   # (a call of one path has a start)
    if T > 2 and K > 4:
        paths[4, 1, 0] = np.nan                              # a terminator at j = 1
        paths[3, T // 2, 1] = np.inf                         # and one mid-path
    hops = rng.integers(0, 9, cells["num_nodes"]).astype(np.uint32)
    info, _, _ = check(m, w, paths, (K, T, sf), row_cap=4, hops=hops, min_hops=1 if K == 65 else 0, entries=(False,) if K == 257 else (False, True))
    assert (info["status"] == wr.DONE).any() or K == 1
    assert info["status"][0] != wr.NO_START
    if T > 2 and K > 4:
        assert info["waypoints"][4] <= 1 and info["waypoints"][3] <= T // 2


def test_more_paths_than_one_trip_of_the_grid_stride_loop():
    """k_walk_paths `for (p = blockIdx.x * blockDim.x + threadIdx.x; p < K; p += gsz)` with at most 8192 workgroups of 64 lanes: 65
    paths more than one trip holds, so one wavefront and one lane of a second come round again.  The batch repeats 4099 distinct
    paths (a prime: no repeat shares its lane with its original), the restatement walks those once and is tiled the same way."""
    from tests.test_walk_host import random_paths
    m, w, cells = drawn("ground", _ground)
    D, K = 4099, 8192 * 64 + 65
    assert K > 8192 * 64
    base = random_paths(np.random.default_rng(4099), D, 2, (-3.0, -3.0), (3.0, 3.0), 0.1, 0.2, reach=0.9)
    assert len(np.unique(base.reshape(D, -1).view(np.uint32), axis=0)) == D
    paths = np.resize(base, (K, 2, 3))
    assert paths[D].tobytes() == base[0].tobytes() and paths[K - 1].tobytes() == base[(K - 1) % D].tobytes()
    info_d, rows_d, _ = w.walk(base, row_cap=1)
    tile = np.arange(K) % D
    want_info, want_rows = info_d[tile], rows_d[tile]
    assert {wr.DONE, wr.LEFT_MAP} <= set(info_d["status"].tolist()) and info_d["steps"].max() >= 2
    for table in (False, True):
        with step_table(table):
            rc, info, rows, untouched = raw(m, paths, row_cap=1)
        assert rc == 0 and untouched, table
        assert info[:K - D].tobytes() == info[D:].tobytes() and rows[:K - D].tobytes() == rows[D:].tobytes(), table
        wr.same(info, rows, want_info, want_rows, ("grid stride", table))


def _three_ways(m, w, paths, what, **kw):
    """one call with the table option at its default, against the restatement; the same call forced to either variant: the same bytes"""
    want_info, want_rows, _ = w.walk(paths, **kw)
    rc, info, rows, untouched = raw(m, paths, **kw)
    assert rc == 0 and untouched, (what, m._L.gndt_last_error(m._h))
    wr.same(info, rows, want_info, want_rows, (what, "default"))
    for table in (False, True):
        with step_table(table):
            rc, i2, r2, untouched = raw(m, paths, **kw)
        assert rc == 0 and untouched and i2.tobytes() == info.tobytes() and r2.tobytes() == rows.tobytes(), (what, table)
    return want_info


def _lattice_paths(cells, K, seed, reach):
    from tests.test_walk_host import random_paths
    on = cells["mean"][(cells["flags"] & 2) != 0]
    return random_paths(np.random.default_rng(seed), K, 2, on[:, :2].min(0), on[:, :2].max(0), 0.0, 0.1, reach=reach, on=on)


def test_the_default_table_choice_on_both_sides_of_its_threshold():
    """gndt_api_walk.hip `table = ... mode == 2 && n <= kWalkTableRowsPerWaypoint * T`, with the option left at its default of 2: on
    9217 rows T = 2 walks inline (n > 4096) and T = 6 through the table (n <= 12288).  The T = 6 paths are the T = 2 ones with the
    last waypoint repeated.  Every other comparing test forces the option."""
    m, w, cells = drawn("lattice 9217", lambda: cr.lattice(9217, fr.P))
    n = int(cells["num_nodes"])
    assert n == 9217 and 2048 * 2 < n <= 2048 * 6
    p2 = _lattice_paths(cells, 96, 17, 2.5)
    p6 = np.ascontiguousarray(np.concatenate([p2, np.repeat(p2[:, 1:], 4, axis=1)], axis=1))
    assert p6.shape == (96, 6, 3)
    i2 = _three_ways(m, w, p2, "T = 2: inline", row_cap=4)
    i6 = _three_ways(m, w, p6, "T = 6: the table", row_cap=4)
    assert {wr.DONE, wr.LEFT_MAP} <= set(i2["status"].tolist()) and i2["steps"].max() >= 4
    for k in ("status", "steps", "end_row", "length"):
        assert np.array_equal(i2[k], i6[k]), k              # (padding changes `waypoints` alone)


def test_the_default_table_choice_at_its_threshold_to_the_row():
    """gndt_api_walk.hip `n <= kWalkTableRowsPerWaypoint * T` at equality: 2048 rows and T = 1 take the table by the `=`, and so do the
    2047 rows left when one column is dropped; both against the restatement and the forced variants.  Under the poisoned variant of
    the library (tests/test_gpu_poisoned.py), which counts what it allocates, the default call at equality is also seen to make the
    table: the walk's scratch of 41 bytes a row and 8 is the one allocation between an inline call and it."""
    import grid_ndt_amd as g
    from grid_ndt_amd import _lib
    m = build(cr.lattice(2048, fr.P), fr.P)
    for left in (2048, 2047):
        cells = m.export()
        n = int(cells["num_nodes"])
        assert n == left and ((cells["flags"] & 2) != 0).all() and (n == 2048 * 1 if left == 2048 else n < 2048 * 1)
        w = wr.Walker(cells, fr.ORIGIN, fr.P["grid_len"], fr.P["z_len"])
        assert w.f.angle_margin_deg > MARGIN
        paths = np.ascontiguousarray(_lattice_paths(cells, 96, left, 1.0)[:, :1])
        if _lib.VARIANT == "poison" and left == 2048:
            with step_table(False):
                assert raw(m, paths)[0] == 0                # (the column index is made here)
            before = g.TwoDmap.poisoned_bytes()[0]
            assert raw(m, paths)[0] == 0
            assert g.TwoDmap.poisoned_bytes()[0] - before == n * 41 + 8
        info = _three_ways(m, w, paths, ("T = 1", left), row_cap=2)
        assert {wr.DONE, wr.NO_START} <= set(info["status"].tolist()) and (info["steps"] == 0).all()
        if left == 2048:
            m.crop_box((5, 5, 7, 7), "drop_inside")


def test_hops_and_min_hops_against_a_real_clearance_field():
    m, w, cells = drawn("corridor", cr.corridor_cloud, cr.CORRIDOR_P)
    cl = m.clearance(host=True)
    hops = cl["hops"].view(np.uint32)
    assert np.array_equal(hops, w.f.clearance(cr.BLOCKED, 32)["hops"])
    paths = np.concatenate([path((1.76, 0.3), (1.76, 5.7)), path((1.76, 2.76), (0.3, 2.76)), path((0.3, 0.3), (0.3, 1.3))])
    info, _, _ = check(m, w, paths, "hops only", hops=hops)
    assert info["status"].tolist() == [wr.DONE] * 3 and info["hops_min"].tolist() == [3, 0, 0]
    info, _, _ = check(m, w, paths, "min_hops 2", hops=hops, min_hops=2)
    assert info["status"].tolist() == [wr.DONE, wr.TOO_CLOSE, wr.TOO_CLOSE] and info["steps"].tolist() == [11, 2, 0]
    assert info["hops_min"].tolist() == [3, 1, 0]
    info, _, _ = check(m, w, paths, "no field")
    assert (info["hops_min"] == wr.BEYOND).all()
    # the Python interface takes what clearance() returned, on the device and on the host
    for host in (False, True):
        field = m.clearance(host=host)
        got = m.walk_paths(paths if host else dev(paths), hops=field, min_hops=2, rows=3, host=host)
        assert to_np(got["status"]).tolist() == [wr.DONE, wr.TOO_CLOSE, wr.TOO_CLOSE] and to_np(got["hops_min"]).tolist() == [3, 1, 0]


def test_after_an_update_a_crop_and_with_another_robot():
    """what a table of another map or another robot would answer differently shows here: every call makes its own"""
    from tests.test_walk_host import random_paths
    cloud = scenes.bridge_ground()
    P = scenes.BRIDGE_PARAMS
    m = build(cloud, P, ATOMIC)                          # (updates need the additive strategy)
    rng = np.random.default_rng(9)
    other = dict(reachable_height=0.05, max_angle_deg=12.0)
    seen = set()

    def fresh(what):
        cells = m.export()
        on = cells["mean"][(cells["flags"] & 2) != 0]
        paths = random_paths(rng, 48, 5, on[:, :2].min(0), on[:, :2].max(0), float(on[:, 2].min()), float(on[:, 2].max()), reach=0.6, on=on)
        for robot in (None, other, None):
            w = wr.Walker(cells, cloud[0, :3], P["grid_len"], P["z_len"], robot)
            assert w.f.angle_margin_deg > MARGIN, (what, robot)
            info, _, _ = check(m, w, paths, (what, robot), robot=robot, row_cap=6, entries=(False,))
            seen.update(info["status"].tolist())
        return cells

    before = fresh("before")
    x0, x1 = int(before["sx"].min()), int(before["sx"].max())
    m.change2DMap("slope", dev(cloud[1:4000, :3] + np.float32([0.0, 0.0, 0.3])))
    fresh("update")
    m.crop_box((x0 + (x1 - x0) // 4, x1 - (x1 - x0) // 4, -100000, 100000), "keep_inside")
    cropped = fresh("crop")
    assert cropped["num_nodes"] < before["num_nodes"] and {wr.DONE, wr.BLOCKED, wr.LEFT_MAP} <= seen
    # everything cropped away: no path has a start, through either variant
    m.crop_box((x1 + 50, x1 + 60, 1, 2), "keep_inside")
    assert m.sync()[0] == 0
    for table in (False, True):
        with step_table(table):
            for host in (False, True):
                rc, info, rows, untouched = raw(m, path((0.1, 0.1), (0.5, 0.5)), row_cap=2, host=host)
                assert rc == 0 and info["status"][0] == wr.NO_START and info["waypoints"][0] == 0 and (rows == wr.NO_ROW).all() and untouched


def test_a_second_stream_repeat_calls_and_the_python_interface():
    import torch
    from grid_ndt_amd import rollouts
    from tests.test_walk_host import random_paths
    m, w, cells = drawn("ground", _ground)
    rng = np.random.default_rng(3)
    paths = random_paths(rng, 96, 6, (-3.0, -3.0), (3.0, 3.0), 0.1, 0.2, reach=0.7)
    s = torch.cuda.Stream()
    want, want_rows, _ = check(m, w, paths, "second stream", stream=s, row_cap=5, entries=(False,))
    check(m, w, paths[:, :, [0, 1, 2, 2]], "stride 16", row_cap=5)
    for kw in (dict(), dict(host=True), dict(stream=s)):
        got = m.walk_paths(paths if kw.get("host") else dev(paths), rows=5, **kw)
        if "stream" in kw:
            s.synchronize()
        assert isinstance(got["status"], np.ndarray) == bool(kw.get("host"))
        for k in wr.INFO_FIELDS:
            assert to_np(got[k]).view(np.uint32).tobytes() == want[k].view(np.uint32).tobytes(), (k, kw)
        assert np.array_equal(to_np(got["rows"]).view(np.uint32), want_rows)
    got = m.walk_paths(dev(paths), start_mode="node", overhead=True, max_steps=3, robot=dict(radius=0.2))
    ref, _, _ = w.walk(paths, start_mode="node", overhead=True, max_steps=3)
    assert np.array_equal(to_np(got["status"]), ref["status"]) and "rows" not in got
    # flood -> arcs -> walk_paths -> choose
    assert m.computeCost((2.25, 2.25, 0.125))["rc"] == 0
    h = torch.from_numpy(m.cost_export()["h"]).cuda()
    arcs = rollouts.arcs(torch.tensor([0.25, 0.25, 0.125, 0.6], device="cuda"), 1.0, np.linspace(-1.5, 1.5, 13), 0.2, 12)
    info = m.walk_paths(arcs)
    best = rollouts.choose(info, h[info["end_row"].long().clamp(min=0)])
    ref, _, _ = w.walk(arcs.cpu().numpy())
    done = np.flatnonzero(ref["status"] == wr.DONE)
    assert best in done and m.cost_export()["h"][ref["end_row"][best]] == m.cost_export()["h"][ref["end_row"][done]].min()
    # nothing to do
    for host in (False, True):
        empty = m.walk_paths(np.zeros((0, 4, 3), np.float32) if host else dev(np.zeros((0, 4, 3))), host=host)
        assert len(empty["status"]) == 0


# ---- refusals ----------------------------------------------------------------------------------------------------------------------

def test_refused_arguments():
    import torch
    import grid_ndt_amd as g
    from grid_ndt_amd._lib import WalkParams
    m, w, cells = drawn("ground", _ground)
    p1 = path((0.25, 0.25), (0.75, 0.25), z=0.125)
    for host in (False, True):
        assert raw(m, p1, host=host)[0] == 0
        for mode in (3, -1, 7):
            assert raw(m, p1, mode=mode, host=host)[0] == ERR_INVALID, mode
        rc, info, _, _ = raw(m, p1, mode=0, host=host)                        # 0 = the default: nearest slope
        assert rc == 0 and info["status"][0] == wr.DONE
        for checks in (2, 3, 0x80000000):
            assert raw(m, p1, checks=checks, host=host)[0] == ERR_INVALID, checks
        assert raw(m, p1, max_steps=(1 << 20) + 1, host=host)[0] == ERR_INVALID and raw(m, p1, max_steps=1 << 20, host=host)[0] == 0
        for k in range(4):
            assert raw(m, p1, reserved=tuple(int(j == k) for j in range(4)), host=host)[0] == ERR_INVALID, k
    prm = WalkParams()
    buf = torch.zeros(256, dtype=torch.int32, device="cuda")
    pts = dev(p1)
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    call = m._L.gndt_walk_paths_device
    ok = lambda *a: call(m._h, *a)
    assert ok(p(pts), 1, 2, 12, None, C.byref(prm), None, None, 0, p(buf), None) == 0
    assert ok(p(pts), 1, 2, 8, None, C.byref(prm), None, None, 0, p(buf), None) == ERR_INVALID                 # stride
    assert ok(p(pts), 1, 2, 12, None, None, None, None, 0, p(buf), None) == ERR_INVALID                        # NULL params
    assert ok(p(pts), 1, 2, 12, None, C.byref(prm), None, None, 0, None, None) == ERR_INVALID                  # NULL info
    assert ok(None, 1, 2, 12, None, C.byref(prm), None, None, 0, p(buf), None) == ERR_INVALID                  # NULL paths
    assert ok(p(pts), 1, 2, 12, None, C.byref(prm), None, None, 0, p(buf, 8), None) == ERR_INVALID             # info not aligned to 16
    assert ok(p(pts), 1, 2, 12, None, C.byref(prm), None, p(buf, 64), 0, p(buf), None) == ERR_INVALID          # rows without a cap
    assert ok(p(pts), 1, 2, 12, None, C.byref(prm), None, None, 4, p(buf), None) == ERR_INVALID                # a cap without rows
    assert ok(p(pts), 1, 2, 12, None, C.byref(prm), None, p(buf, 66), 4, p(buf), None) == ERR_INVALID          # rows not aligned
    assert ok(p(pts, 2), 1, 1, 12, None, C.byref(prm), None, None, 0, p(buf), None) == ERR_INVALID             # paths not aligned
    assert ok(p(pts), 1, 2, 12, None, C.byref(prm), p(buf, 65), None, 0, p(buf), None) == ERR_INVALID          # hops not aligned
    assert ok(p(pts), 1 << 16, 1 << 15, 12, None, C.byref(prm), None, None, 0, p(buf), None) == ERR_INVALID    # K T = 2^31
    assert ok(p(pts), 0, 2, 12, None, C.byref(prm), None, None, 0, p(buf), None) == 0                          # nothing to do
    assert ok(p(pts), 1, 0, 12, None, C.byref(prm), None, None, 0, p(buf), None) == 0
    assert call(None, p(pts), 1, 2, 12, None, C.byref(prm), None, None, 0, p(buf), None) == ERR_INVALID
    assert m._L.gndt_walk_paths(None, None, 1, 2, 12, None, C.byref(prm), None, None, 0, None) == ERR_INVALID
    torch.cuda.synchronize()
    assert not buf[12:].any()                                                 # K = 0 and T = 0 wrote nothing, one path wrote 48 bytes
    with pytest.raises(g.GndtError):
        g.TwoDmap.set_debug_option(g.TwoDmap.DEBUG_WALK_STEP_TABLE, 3)
    # no finished build
    e = g.TwoDmap(0.5, 0.25)
    e.setCloudFirst((0.0, 0.0, 0.0))
    with pytest.raises(g.GndtError) as err:
        e.walk_paths(pts)
    assert err.value.code == ERR_INVALID
    # a capturing stream: refused, and the capture goes on
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    x = torch.zeros(16, device="cuda")
    with g.graph_capture(graph, stream=s):
        rc = call(m._h, p(pts), 1, 2, 12, None, C.byref(prm), None, None, 0, p(buf), C.c_void_p(s.cuda_stream))
        x.add_(1.0)
    assert rc == ERR_INVALID
    graph.replay()
    torch.cuda.synchronize()
    assert float(x[0]) == 1.0
    check(m, w, p1, "after the refused capture")
