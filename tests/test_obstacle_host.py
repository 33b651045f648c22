"""CPU tier: the obstacle field's per-element code (grid_ndt_amd/csrc/gndt_obstacle.hpp: windows, the bisection over their prefix sums,
the stamped marks, the steps in worklist places, the rounds over compact keys, the finish), compiled with g++ into
tests/_obstacle_shim.so and run one element after another, against the restatement from the rows (tests/obstacle_ref.py: rows x boxes by
brute force, a breadth-first search) — hops, obstacle and counts for equality, with no tolerance: on the corridor, on the pit with its
37-row column, on tables whose step graph is directed, on the bridge with a box on the deck and one under it, and on 200 random tables
with 1 to 40 random boxes; marking front to back and back to front; call after call on the same stamped marks and on marks full of
garbage; and the product entry points refuse to run without a GPU."""
import ctypes as C

import numpy as np
import pytest

from tests import clearance_ref as cr
from tests import obstacle_ref as ob
from tests.host_emulation import MAP, HostMap, load_shim
from tests.test_clearance_host import FUZZ_ROBOT, MARGIN, Table, random_table

_shim = None


def shim():
    global _shim
    if _shim is None:
        vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
        _shim = load_shim("obstacle_shim.cpp", "_obstacle_shim.so", {
            "obshim_field": ([C.c_int, vp, vp, u32, u64, C.c_int64, vp, u64, MAP, u32] + [vp] * 8, C.c_int),
        })
    return _shim


class Marks:
    """the stamped words of a handle: "never" when made (garbage: any words whose stamps lie below the next call's), a stamp a call"""

    def __init__(self, n, garbage=None):
        room = max(n, 1)
        self.cstamp = np.zeros(room, np.uint32)
        self.slot = np.full(room, 0xA5A5A5A5, np.uint32)
        self.cover = np.full(room, 0xFFFFFFFFFFFFFFFF, np.uint64)
        self.stamp = 0
        if garbage is not None:                          # what earlier calls on other maps may have left: stamps up to 1000
            self.cstamp[:] = garbage.integers(0, 1001, room)
            self.cover[:] = ((0xFFFFFFFF - garbage.integers(0, 1001, room).astype(np.uint64)) << np.uint64(32)) | garbage.integers(0, 50, room).astype(np.uint64)
            self.stamp = 1000


def run(t, boxes, robot=None, inflate=0, max_hops=8, levels_above=0, levels_below=0, max_columns=0, base=None, n_boxes_dev=None, stride=24,
        order=0, marks=None, want=("hops", "obstacle"), in_place=False):
    """the shim's passes on t (a Table or a HostMap) -> dict(hops, obstacle, counts, info)"""
    rb = dict(cr.ROBOT)
    rb.update(robot or {})
    r4 = np.array([rb["radius"], rb["reachable_height"], rb["max_rough"], rb["max_angle_deg"]], np.float32)
    n = t.n
    boxes = np.ascontiguousarray(boxes, np.int32).reshape(-1, 6)
    recs = np.full((max(len(boxes), 1), stride // 4), 0x5A5A5A5A, np.int32)
    off = (stride - 24) // 8                             # the six words somewhere inside a wider record
    recs[:len(boxes), off:off + 6] = boxes
    marks = marks or Marks(n)
    marks.stamp += 1
    hops = np.full(max(n, 1), 0xDEADBEEF, np.uint32)
    obstacle = np.full(max(n, 1), 0xDEADBEEF, np.uint32)
    bs = None if base is None else np.ascontiguousarray(base, np.uint32)
    if in_place:
        hops[:n] = bs
        bs = hops
    counts = np.full(8, 0xDEADBEEF, np.uint32)
    info = np.zeros(8, np.uint32)
    prm = np.array([inflate, max_hops or 8, levels_above, levels_below], np.uint32)
    p = lambda a: None if a is None else a.ctypes.data
    rc = shim().obshim_field(order, p(r4), recs.ctypes.data + 4 * off, len(boxes), stride, -1 if n_boxes_dev is None else n_boxes_dev, p(prm),
                             max_columns or 1 << 24, t.shim_map(), marks.stamp, p(marks.cstamp), p(marks.slot), p(marks.cover), p(bs),
                             p(hops) if "hops" in want else None, p(obstacle) if "obstacle" in want else None, p(counts), p(info))
    assert rc == 0
    return dict(hops=hops[:n], obstacle=obstacle[:n], counts=counts, info=info)


def same(got, want, what, keys=("counts", "hops", "obstacle")):
    for k in keys:
        assert np.array_equal(got[k], want[k]), (what, k, np.flatnonzero(got[k] != want[k])[:8], got[k][:8], want[k][:8])


def not_vacuous(want, what):
    """covered > 0, some finite hops > 0, some BEYOND"""
    h = want["own_hops"]
    assert want["counts"][0] > 0 and ((h > 0) & (h != ob.BEYOND)).any() and (h == ob.BEYOND).any(), (what, want["counts"])


def check(t, f, boxes, what, robot=None, **kw):
    want = ob.field(f, t.cells, boxes, **kw)
    for order in (0, 1):
        same(run(t, boxes, robot, order=order, **kw), want, (what, order))
    return want


_maps = {}


def _map(name):
    from tests import frontier_ref as fr
    from grid_ndt_amd import scenes
    if name not in _maps:
        cloud, P = {"corridor": lambda: (cr.corridor_cloud(), cr.CORRIDOR_P), "pit": lambda: (cr.pit_cloud(), fr.P),
                    "bridge_ground": lambda: (scenes.bridge_ground(), scenes.BRIDGE_PARAMS)}[name]()
        m = HostMap(cloud, P, seed=13)
        _maps[name] = (m, cr.Field(m.cells))
    return _maps[name]


def test_corridor_boxes_inflation_hops_and_owner():
    t, f = _map("corridor")
    assert f.angle_margin_deg > MARGIN and t.n == 156
    z = int(t.sz[(t.sx == 4) & (t.sy == 6)][0])                # the corridor floor's level
    one = [[4, 4, 6, 6, z, z]]
    w = check(t, f, one, "one cell", max_hops=3)
    not_vacuous(w, "one cell")
    assert w["counts"][5] == 49 and w["counts"][1] == 1 + 4 + 8 + 12                  # the window's 7 x 7 columns, the diamond of 3 hops
    assert w["counts"][0] == 1 and w["counts"][2] == 3 and w["counts"][3] == 1 and w["counts"][4] == 1 and w["counts"][6] == 0
    for inflate in (0, 1, 3):
        w = check(t, f, one, ("inflate", inflate), inflate=inflate, max_hops=2)
        assert int(w["covered"].sum()) == int((f.slope & (np.abs(ob.lin(t.sx) - 3) <= inflate) & (np.abs(ob.lin(t.sy) - 5) <= inflate) & (t.sz == z)).sum())
    # two overlapping boxes: the owner is the smaller index; a void box between them; a box off the map; one on another level
    many = [[3, 5, 5, 7, z, z], [4, 6, 6, 8, z, z], [5, 4, 1, 1, z, z], [300, 310, 1, 4, z, z], [1, 2, 1, 2, z + 9, z + 9]]
    w = check(t, f, many, "overlap", max_hops=4)
    not_vacuous(w, "overlap")
    assert (w["obstacle"][w["covered"]] <= 1).all() and (w["obstacle"][(t.sx == 5) & (t.sy == 7)] == 0).all() and w["counts"][4] == 2
    assert (w["obstacle"][(t.sx == 6) & (t.sy == 8)] == 1).all()
    # the count on the device cuts the list, or leaves it
    for nd in (0, 1, 2, 5, 9):
        same(run(t, many, max_hops=4, n_boxes_dev=nd, stride=72), ob.field(f, t.cells, many, max_hops=4, n_boxes_dev=nd), ("n_boxes_dev", nd))
    # the body's levels decide by one level
    up = [[4, 4, 6, 6, z + 2, z + 3]]
    assert check(t, f, up, "above 1", levels_above=1)["counts"][0] == 0 and check(t, f, up, "above 2", levels_above=2)["counts"][0] == 1
    unlin = lambda v: v + 1 if v >= 0 else v              # (there is no level 0)
    down = [[4, 4, 6, 6, unlin(int(ob.lin(z)) - 3), unlin(int(ob.lin(z)) - 2)]]
    assert check(t, f, down, "below 1", levels_below=1)["counts"][0] == 0 and check(t, f, down, "below 2", levels_below=2)["counts"][0] == 1
    # across the walls nothing steps: the plateaus stay beyond however many hops
    w = check(t, f, one, "deep", max_hops=64)
    assert (w["own_hops"][ob.lin(t.sx) < 0] == ob.BEYOND).all() and (w["own_hops"][(ob.lin(t.sx) >= 0) & (ob.lin(t.sx) < 7)] != ob.BEYOND).all()


def test_budget_admits_a_prefix_and_counts_the_rest():
    t, f = _map("corridor")
    z = int(t.sz[(t.sx == 4) & (t.sy == 6)][0])
    boxes = [[2, 2, 3, 3, z, z], [9, 8, 1, 1, z, z], [5, 6, 8, 8, z, z], [1, 1, 1, 1, z, z], [7, 7, 10, 10, z, z]]
    void, admitted, dropped, w, W = ob.budget(ob.resolve(boxes), 1, 2)
    assert list(w) == [49, 0, 56, 49, 49] and list(W) == [49, 49, 105, 154, 203]
    for cols, n_adm in ((203, 4), (202, 3), (154, 3), (153, 2), (105, 2), (104, 1), (49, 1), (48, 0), (1, 0)):
        want = check(t, f, boxes, ("budget", cols), inflate=1, max_hops=2, max_columns=cols)
        assert int(want["admitted"].sum()) == n_adm and want["counts"][6] == 4 - n_adm, (cols, want["counts"])
        assert not want["admitted"][np.flatnonzero(want["dropped"]).min():].any() if want["dropped"].any() else True
        assert (want["counts"][0] > 0) == (n_adm > 0)
    # a box whose window holds no index that exists is admitted and covers nothing; a zone far larger than the map costs its window
    far = [[70000, 70010, 1, 2, z, z], [1, 1, 1, 1, z, z]]
    want = check(t, f, far, "off the codec's range", max_hops=2)
    assert list(want["w"]) == [0, 25] and want["counts"][4] == 1 and want["counts"][6] == 0
    want = check(t, f, [[-65535, 65535, -65535, 65535, z, z], [1, 1, 1, 1, z, z]], "the whole plane", max_hops=2)
    assert want["counts"][6] == 2 and want["counts"][0] == 0 and want["counts"][5] == 0


def test_pit_a_box_on_the_37_row_column_and_steps_through_it():
    t, f = _map("pit")
    c = int(np.flatnonzero(t.row_ncol == 37)[0])
    floor = c + 36
    assert (t.flags[c:floor] & 2 == 0).all() and t.flags[floor] & 2 and t.sx[c] == 4 and t.sy[c] == 1
    z = int(t.sz[floor])
    # on the column itself: of its 37 rows only the floor is covered, and the pit's nodes under it are rows in the worklist, not slopes in reach
    w = check(t, f, [[4, 4, 1, 1, z, z]], "on the pit", max_hops=2)
    not_vacuous(w, "on the pit")
    assert w["counts"][0] == 1 and w["covered"][floor] and w["counts"][5] == 5
    got = run(t, [[4, 4, 1, 1, z, z]], max_hops=2)
    assert got["info"][0] == 4 + 37 and (got["hops"][c:floor] == ob.BEYOND).all()
    # a box of every level of the pit covers the floor only through the body's levels below
    unlin = lambda v: v + 1 if v >= 0 else v              # (there is no level 0)
    under = [[4, 4, 1, 1, unlin(int(ob.lin(z)) - 30), unlin(int(ob.lin(z)) - 1)]]
    assert check(t, f, under, "in the pit", levels_below=0)["counts"][0] == 0
    assert check(t, f, under, "in the pit", levels_below=1)["counts"][0] == 1
    # beside it: the walk from cell 2 to cell 6 steps onto row 36 of the tall column, behind its neighbours' step masks
    w = check(t, f, [[7, 7, 1, 1, z, z]], "through the pit", max_hops=8)
    by_x = [int(w["own_hops"][(t.sx == x) & ((t.flags & 2) != 0)][0]) for x in range(1, 9)]
    assert by_x == [6, 5, 4, 3, 2, 1, 0, ob.BEYOND]        # (cell 7 stands a metre higher: no step leads off it)


def test_bridge_a_box_on_the_deck_leaves_the_ground_under_it_and_the_reverse():
    t, f = _map("bridge_ground")
    assert f.angle_margin_deg > MARGIN
    slope = (t.flags & 2) != 0
    cols = {}
    for r in np.flatnonzero(slope):
        cols.setdefault((int(t.sx[r]), int(t.sy[r])), []).append(int(r))
    two = {k: v for k, v in cols.items() if len(v) == 2 and abs(int(ob.lin(t.sz[v[0]])) - int(ob.lin(t.sz[v[1]]))) >= 3}
    assert len(two) > 4
    (x, y), rows = sorted(two.items())[len(two) // 2]
    ground, deck = sorted(rows, key=lambda r: int(t.sz[r]))
    for name, row, other in (("on the deck", deck, ground), ("under the deck", ground, deck)):
        z = int(t.sz[row])
        w = check(t, f, [[x, x, y, y, z, z]], name, levels_above=1, levels_below=0, max_hops=4)
        not_vacuous(w, name)
        assert w["covered"][row] and not w["covered"][other] and w["counts"][0] == 1
        assert w["own_hops"][row] == 0 and w["own_hops"][other] != 0
        assert w["in_reach"][other]                         # z plays no part in reach
    # both at once, the deck's box first: each storey names its own box
    zg, zd = int(t.sz[ground]), int(t.sz[deck])
    w = check(t, f, [[x, x, y, y, zd, zd], [x, x, y, y, zg, zg]], "both", levels_above=1, max_hops=4)
    assert w["obstacle"][deck] == 0 and w["obstacle"][ground] == 1
    base = f.clearance(cr.BLOCKED, 32)["hops"]
    same(run(t, [[x, x, y, y, zd, zd]], levels_above=1, max_hops=4, base=base), ob.field(f, t.cells, [[x, x, y, y, zd, zd]], levels_above=1, max_hops=4, base=base), "base")


def test_a_rough_cell_lets_walks_out_and_none_in():
    """Six cells in a line, x = 1 .. 6 at y = 1, level and smooth but cell 4, whose roughness is over the robot's limit.  The roughness
    gate looks at the destination only: the step 4 -> 3 and 4 -> 5 exist, 3 -> 4 and 5 -> 4 do not.  A walk to a box therefore crosses
    cell 4 only by starting on it, and the cells behind it stay BEYOND; a gate that looked at the source would give 6 5 4 ... instead."""
    n = 6
    rough = np.array([0.1, 0.1, 0.1, 2.0, 0.1, 0.1])
    t = Table(np.arange(1, n + 1), np.ones(n, int), np.ones(n, int), np.full(n, 3), np.ones(n, int),
              np.stack([np.arange(1, n + 1) * 0.5, np.full(n, 0.5), np.full(n, 0.05)], 1), np.tile(np.float32([0, 0, 1]), (n, 1)), rough)
    f = cr.Field(t.cells, FUZZ_ROBOT)
    edges = set(zip(f.edge_from.tolist(), f.edge_to.tolist()))
    assert (3, 2) in edges and (3, 4) in edges and (2, 3) not in edges and (4, 3) not in edges and (1, 2) in edges and (2, 1) in edges
    B = ob.BEYOND
    for box, hops in (([6, 6, 1, 1, 1, 1], [B, B, B, 2, 1, 0]), ([1, 1, 1, 1, 1, 1], [0, 1, 2, 3, B, B]), ([4, 4, 1, 1, 1, 1], [B, B, B, 0, B, B]),
                      ([3, 3, 1, 1, 1, 1], [2, 1, 0, 1, B, B])):
        want = check(t, f, [box], ("one way", box), robot=FUZZ_ROBOT, max_hops=8)
        assert want["own_hops"].tolist() == hops, (box, want["own_hops"])
        not_vacuous(want, box) if box[0] != 4 else None


def random_boxes(rng, side=18):
    """1 to 40 boxes over and around an 18 x 18 table: most a few cells wide, some void, some off the map, many overlapping"""
    out = []
    for _ in range(int(rng.integers(1, 41))):
        x0, y0 = (int(v) for v in rng.integers(-side // 2 - 3, side // 2 + 4, 2))
        x1, y1 = x0 + int(rng.integers(0, 4)), y0 + int(rng.integers(0, 4))
        z0 = int(rng.integers(-3, 4))
        z1 = z0 + int(rng.integers(0, 3))
        kind = rng.random()
        if kind < 0.08:
            x0, x1 = x1 + 1, x0 - 1                        # void on x (min > max even where x0 == x1)
        elif kind < 0.12:
            z0, z1 = z1 + 1, z0
        elif kind < 0.15:
            x0, x1 = x0 + 40, x1 + 40                      # off the map
        out.append([x0, x1, y0, y1, z0, z1])
    return out


def test_fuzz_200_random_tables_with_random_boxes():
    rng = np.random.default_rng(20241020)
    skipped = covered = far = beyond = dropped = voids = directed = 0
    tables = 200
    for k in range(tables):
        t = random_table(rng)
        f = cr.Field(t.cells, FUZZ_ROBOT)
        if f.angle_margin_deg <= MARGIN:
            skipped += 1
            continue
        boxes = random_boxes(rng)
        kw = dict(inflate=int(rng.integers(0, 3)), max_hops=int(rng.choice([1, 2, 3, 8])), levels_above=int(rng.integers(0, 3)),
                  levels_below=int(rng.integers(0, 2)))
        if rng.random() < 0.25:
            W = ob.budget(ob.resolve(boxes), kw["inflate"], kw["max_hops"])[4]
            kw["max_columns"] = max(int(W[int(rng.integers(0, len(W)))]) - int(rng.integers(0, 2)), 1)
        if rng.random() < 0.3:
            kw["base"] = f.clearance(cr.BLOCKED, 32)["hops"]
        if rng.random() < 0.2:
            kw["n_boxes_dev"] = int(rng.integers(0, len(boxes) + 3))
        want = ob.field(f, t.cells, boxes, **kw)
        marks = Marks(t.n, garbage=rng) if k % 3 == 0 else None
        got = run(t, boxes, FUZZ_ROBOT, order=k & 1, stride=(24, 72, 40)[k % 3], marks=marks, in_place=("base" in kw and k % 2 == 0), **kw)
        same(got, want, (k, kw))
        if marks is not None:                              # the next call on the same marks: other boxes, the same words
            boxes2 = random_boxes(rng)
            same(run(t, boxes2, FUZZ_ROBOT, marks=marks, max_hops=3), ob.field(f, t.cells, boxes2, max_hops=3), (k, "second call"))
        # the owner from one forward search per row: no layers, no rounds
        full = ob.field(f, t.cells, boxes, **{**kw, "max_hops": 1024, "base": None, "max_columns": 0}) if k % 10 == 0 else None
        if full is not None:
            first = np.where(full["covered"], full["obstacle"].astype(np.int64), -1)
            by_search = ob.owner_by_search(f, first)
            assert np.array_equal(np.where(by_search < 0, ob.NO_ROW, by_search).astype(np.uint32), full["obstacle"]), k
        h = want["own_hops"]
        edges = set(zip(f.edge_from.tolist(), f.edge_to.tolist()))
        covered += int(want["counts"][0])
        far += int(((h > 0) & (h != ob.BEYOND)).any())
        beyond += int((h[f.slope] == ob.BEYOND).any())
        dropped += int(want["counts"][6])
        voids += int((~want["admitted"] & ~want["dropped"]).sum())
        directed += int(any((b, a) not in edges for a, b in edges))
    assert skipped <= tables * 5 // 100, skipped
    print("fuzz:", dict(skipped=skipped, covered=covered, far=far, beyond=beyond, dropped=dropped, voids=voids, directed=directed))
    assert covered > tables and far > tables // 2 and beyond > tables // 2 and dropped > 20 and voids > 50 and directed > tables // 2


def test_null_outputs_and_the_marks_of_an_earlier_larger_call():
    t, f = _map("corridor")
    z = int(t.sz[(t.sx == 4) & (t.sy == 6)][0])
    marks = Marks(t.n)
    big = [[-3, 10, 1, 12, z, z + 4]]
    w = ob.field(f, t.cells, big, max_hops=2, levels_above=4)
    assert w["counts"][0] > 100
    same(run(t, big, max_hops=2, levels_above=4, marks=marks), w, "large")
    small = [[4, 4, 6, 6, z, z]]
    for wanted in (("hops",), ("obstacle",), ("hops", "obstacle")):
        got = run(t, small, max_hops=2, marks=marks, want=wanted)
        same(got, ob.field(f, t.cells, small, max_hops=2), ("small", wanted), ("counts",) + wanted)
        for k in {"hops", "obstacle"} - set(wanted):
            assert (got[k] == 0xDEADBEEF).all()
    # no boxes, and no rows in reach
    got = run(t, np.zeros((0, 6), np.int32), max_hops=2, marks=marks)
    assert tuple(got["counts"]) == (0, 0, 0, 0, 0, 0, 0, 0) and (got["hops"] == ob.BEYOND).all() and (got["obstacle"] == ob.NO_ROW).all()
    same(got, ob.field(f, t.cells, np.zeros((0, 6)), max_hops=2), "B = 0")


def test_no_cpu_fallback_for_the_obstacle_field(native_lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import grid_ndt_amd as g
    m = g.TwoDmap(0.5, 0.5)
    m.setCloudFirst((0, 0, 0))
    with pytest.raises(g.GndtError) as e:
        m.obstacle_field(np.array([[1, 1, 1, 1, 1, 1]], np.int32))
    assert e.value.code == 2   # GNDT_ERR_NO_DEVICE


def test_index_boxes_is_trans_morton_xyz_on_both_corners(native_lib):
    import grid_ndt_amd as g
    m = g.TwoDmap(0.5, 0.25)
    m.setCloudFirst((0.3, -0.2, 1.0))
    lo = np.float32([[0.3, -0.2, 1.0], [-0.7, -1.2, 0.5], [0.8, 0.3, 1.25], [-2.01, 0.29, 0.99], [0.0, 0.0, 0.0], [np.nan, 0, 0], [0, 0, 0]])
    hi = np.float32([[0.79, 0.29, 1.24], [0.31, -0.19, 1.01], [0.8, 0.3, 1.25], [3.3, 2.3, 2.0], [1e9, 0.0, 0.0], [1, 1, 1], [1, np.inf, 1]])
    got = m.index_boxes(lo, hi)
    assert got.dtype == np.int32 and got.shape == (7, 6)
    signed = lambda k: (k[2] if k[1][0] in "AB" else -k[2], k[3] if k[1][0] in "AC" else -k[3], k[4])
    for b in range(4):
        a = g.trans_morton_xyz(m.cloudFirst, m.gridLen, m.zLen, lo[b])
        c = g.trans_morton_xyz(m.cloudFirst, m.gridLen, m.zLen, hi[b])
        assert a[0] == 0 and c[0] == 0
        (ax, ay, az), (cx, cy, cz) = signed(a), signed(c)
        assert tuple(got[b]) == (ax, cx, ay, cy, az, cz), (b, got[b], a, c)
        assert a[1] == m.transMortonXYZ(lo[b])[0] and az == m.transMortonXYZ(lo[b])[1]
    # a cell of index s > 0 holds (s - 1) len < d <= s len, and d = 0 lies on the negative side: the origin itself, a box across the
    # seam on all three axes (no index 0), a point on three upper cell borders, corners on borders of both signs
    assert tuple(got[0]) == (-1, 1, -1, 1, -1, 1) and tuple(got[1]) == (-2, 1, -2, 1, -2, 1) and 0 not in got[:4]
    assert tuple(got[2]) == (1, 1, 1, 1, 1, 1) and tuple(got[3]) == (-5, 6, 1, 5, -1, 4)
    for b in (4, 5, 6):
        assert tuple(got[b]) == (1, 0, 1, 0, 1, 0), got[b]
