"""CPU tier: the clearance field's per-row code (grid_ndt_amd/csrc/gndt_clearance.hpp: the sides and steps of a slope, the rounds over
packed keys, the finish), compiled with g++ into tests/_clearance_shim.so and run one row after another, against the restatement from
the rows (tests/clearance_ref.py: a column dict, the gates in numpy, a breadth-first search) on maps the oracle builds, on 240 random
cell tables and on a column taller than the step mask — hops, nearest, sides and counts for equality; the field's properties on every
map; the in-place serial relaxation against the Jacobi rounds, byte for byte; and the product entry points refuse to run without a GPU."""
import ctypes as C

import numpy as np
import pytest

from tests import clearance_ref as cr
from tests.host_emulation import MAP, HostMap, MapRows, load_shim
from tests.test_raster_host import SCENES

MASKS = (1, 2, 3, 4, 5, 6, 7)
MARGIN = 1e-3            # degrees: tests/test_gpu_cost.py's rule for a decision that acosf's last bit could turn
_shim = None


def shim():
    global _shim
    if _shim is None:
        vp, u32 = C.c_void_p, C.c_uint32
        _shim = load_shim("clearance_shim.cpp", "_clearance_shim.so", {
            "clshim_step_rows": ([], u32),
            "clshim_clearance": ([C.c_int, vp, u32, u32, MAP] + [vp] * 5, C.c_int),
        })
    return _shim


class Table(MapRows):
    """The fields the clearance field reads, as arrays, with the column index the library would build"""

    def __init__(self, sx, sy, sz, flags, row_ncol, mean, normal, rough):
        super().__init__(dict(sx=sx, sy=sy, sz=sz, flags=flags, mean=mean, normal=normal, rough=rough), row_ncol)
        self.cells = dict(num_nodes=self.n, sx=self.sx, sy=self.sy, sz=self.sz, flags=self.flags, mean=self.mean, normal=self.normal,
                          rough=self.rough)


def run(t, robot, mask, max_hops, mode=0):
    """the shim's passes on t (a Table, or a HostMap: the same rows and index) -> dict(hops, nearest, sides, counts, worked)"""
    rb = dict(cr.ROBOT)
    rb.update(robot or {})
    r4 = np.array([rb["radius"], rb["reachable_height"], rb["max_rough"], rb["max_angle_deg"]], np.float32)
    n = t.n
    hops = np.full(max(n, 1), 0xDEADBEEF, np.uint32)
    near = np.full(max(n, 1), 0xDEADBEEF, np.uint32)
    sides = np.full(max(n, 1), 0xEE, np.uint8)
    counts = np.full(4, 0xDEADBEEF, np.uint32)
    info = np.zeros(1, np.uint32)
    p = lambda a: a.ctypes.data
    rc = shim().clshim_clearance(mode, p(r4), mask, max_hops, t.shim_map(), p(hops), p(near), p(sides), p(counts), p(info))
    assert rc == 0
    return dict(hops=hops[:n], nearest=near[:n], sides=sides[:n], counts=counts, worked=int(info[0]))


def same(got, want, what):
    for k in ("counts", "sides", "hops", "nearest"):
        assert np.array_equal(got[k], want[k]), (what, k, np.flatnonzero(got[k] != want[k])[:8], got[k][:8], want[k][:8])


def properties(f, ans, mask, max_hops, what):
    """what holds on every map: one step changes hops by at most one, hops is 0 exactly on the sources, nearest is a source and its
    own nearest, a lower limit only cuts"""
    hops, near = ans["hops"].astype(np.int64), ans["nearest"].astype(np.int64)
    fin = ans["hops"] != cr.BEYOND
    q, p = f.edge_from, f.edge_to
    along = fin[p] & (hops[p] < max_hops)
    assert (fin[q[along]] & (hops[q[along]] <= hops[p[along]] + 1)).all(), what
    assert np.array_equal(fin & (hops == 0), f.sources(mask)), what
    assert (near[~fin] == cr.NO_ROW).all() and f.sources(mask)[near[fin]].all(), what
    assert np.array_equal(near[near[fin]], near[fin]) and (hops[near[fin]] == 0).all(), what
    full = f.clearance(mask, 1024)
    cut = full["hops"].astype(np.int64) > max_hops
    assert np.array_equal(ans["hops"], np.where(cut, cr.BEYOND, full["hops"])), what
    assert np.array_equal(ans["nearest"], np.where(cut, cr.NO_ROW, full["nearest"])), what


_maps = {}


def _map(name):
    if name not in _maps:
        cloud, P = SCENES[name]()
        m = HostMap(cloud, P, seed=13)
        _maps[name] = (m, cr.Field(m.cells))
    return _maps[name]


@pytest.mark.parametrize("name", sorted(SCENES))
def test_oracle_scenes_under_every_source_mask(name):
    t, f = _map(name)
    assert f.angle_margin_deg > MARGIN, f.angle_margin_deg
    some = 0
    for mask in MASKS:
        for max_hops in (1, 2, 32):
            want = f.clearance(mask, max_hops)
            got = run(t, None, mask, max_hops)
            same(got, want, (name, mask, max_hops))
            properties(f, got, mask, max_hops, (name, mask, max_hops))
            some += int(want["counts"][0])
        # thread order cannot matter: relaxing one array in place, in row order, then clamping, gives the rounds' bytes
        serial = run(t, None, mask, 2, mode=1)
        same(serial, f.clearance(mask, 2), (name, mask, "in place"))
    assert some > 0


def random_unit(rng, count, tilt_lo, tilt_hi):
    """unit vectors tilted from the vertical by an angle (degrees) drawn from [tilt_lo, tilt_hi], towards a random side"""
    tilt, az = np.radians(rng.uniform(tilt_lo, tilt_hi, count)), rng.uniform(0.0, 2.0 * np.pi, count)
    return np.stack([np.sin(tilt) * np.cos(az), np.sin(tilt) * np.sin(az), np.cos(tilt)], 1)


def random_table(rng, side=18):
    """Random occupancy, one to three levels a column, random unit normals — ten gentle and four steep ones a table, so that the
    angle gate decides on both sides of its threshold, on few enough distinct angles that one within MARGIN of it is rare — mean z
    spread over the level (the reach decides), roughness on both sides of the limit (the graph is directed), most rows slopes.  The
    gates fail rarely enough for slopes to lie several steps from a barrier."""
    fill = rng.uniform(0.6, 0.95)
    cols = [(ix, iy) for ix in range(-side // 2, side // 2) for iy in range(-side // 2, side // 2) if rng.random() < fill]
    cols = [cols[i] for i in rng.permutation(len(cols))]
    pal = np.concatenate([random_unit(rng, 10, 0.0, 12.0), random_unit(rng, 4, 20.0, 50.0)])
    pool = np.array([-2, -1, 1, 2, 3])
    sx, sy, sz, ncol = [], [], [], []
    for ix, iy in cols:
        zs = rng.choice(pool, size=rng.choice([1, 1, 1, 1, 1, 1, 2, 2, 3]), replace=False)
        if rng.random() < 0.92 and 1 not in zs:           # most columns share a ground level
            zs[rng.integers(0, len(zs))] = 1
        for j, z in enumerate(zs):
            sx.append(ix + 1 if ix >= 0 else ix); sy.append(iy + 1 if iy >= 0 else iy); sz.append(int(z))
            ncol.append(len(zs) if j == 0 else 0)
    n = len(sx)
    sz = np.array(sz)
    lin = np.where(sz > 0, sz - 1, sz)
    mean = np.stack([np.array(sx) * 0.5, np.array(sy) * 0.5, lin * 0.25 + rng.uniform(0.0, 0.18, n)], 1)
    normal = pal[np.where(rng.random(n) < 0.05, rng.integers(10, 14, n), rng.integers(0, 10, n))]
    rough = np.where(rng.random(n) < 0.04, rng.uniform(1.0, 1.3, n), rng.uniform(0.0, 1.0, n))
    flags = np.where(rng.random(n) < 0.96, 3, 1)
    return Table(sx, sy, sz, flags, ncol, mean, normal, rough)


FUZZ_ROBOT = dict(radius=0.25, reachable_height=0.15, max_rough=1.0, max_angle_deg=30.0)


def test_fuzz_240_random_cell_tables():
    rng = np.random.default_rng(20240917)
    skipped = sources = directed = far = 0
    tables = 240
    for k in range(tables):
        t = random_table(rng)
        assert 100 <= t.n <= 800
        f = cr.Field(t.cells, FUZZ_ROBOT)
        if f.angle_margin_deg <= MARGIN:
            skipped += 1
            continue
        mask = int(rng.integers(1, 8))
        max_hops = int(rng.choice([1, 2, 3, 32]))
        want = f.clearance(mask, max_hops)
        got = run(t, FUZZ_ROBOT, mask, max_hops)
        same(got, want, (k, mask, max_hops))
        properties(f, got, mask, max_hops, (k, mask, max_hops))
        same(run(t, FUZZ_ROBOT, mask, max_hops, mode=1), want, (k, mask, max_hops, "in place"))
        # nearest from one forward search per row: no layers, no rounds
        full = f.clearance(mask, 1024)
        by_search = f.nearest_by_search(mask)
        assert np.array_equal(np.where(by_search < 0, cr.NO_ROW, by_search).astype(np.uint32), full["nearest"]), k
        # the restatement alone: the fuzz cannot pass on empty or trivial answers
        edges = set(zip(f.edge_from.tolist(), f.edge_to.tolist()))
        sources += int(want["counts"][0])
        directed += sum((b, a) not in edges for a, b in edges)
        far += int(full["counts"][2] >= 2)
    assert skipped <= tables * 5 // 100, skipped
    print("fuzz:", dict(skipped=skipped, sources=sources, one_way_steps=directed, tables_with_hops_2=far))
    assert sources > tables and directed > tables and far > tables // 2, (sources, directed, far)


def tall_corridor():
    """Columns x = 1 .. 6 at y = 1, one slope each at z = 0.05 but the last, which stands a metre higher: under BLOCKED the sources are
    columns 5 and 6.  Column 3 has 40 nodes, and its only slope is node 35: beyond the step mask of its neighbours."""
    sx, sy, sz, flags, ncol, mean, rough = [], [], [], [], [], [], []
    for x in range(1, 7):
        nodes = 40 if x == 3 else 1
        for j in range(nodes):
            sx.append(x); sy.append(1); sz.append(j + 1); ncol.append(nodes if j == 0 else 0)
            is_slope = nodes == 1 or j == 35
            flags.append(3 if is_slope else 1)
            mean.append([x * 0.5, 0.5, (1.05 if x == 6 else 0.05) if is_slope else 0.25 * j])
            rough.append(0.01)
    normal = np.tile(np.float32([0, 0, 1]), (len(sx), 1))
    return Table(sx, sy, sz, flags, ncol, mean, normal, rough)


def test_a_step_through_a_column_taller_than_the_step_mask():
    t = tall_corridor()
    c = int(np.flatnonzero(t.row_ncol == 40)[0])
    slope = int(np.flatnonzero((t.flags & 2) != 0)[2])
    assert t.row_ncol[c] > shim().clshim_step_rows() and slope - c == 35 >= shim().clshim_step_rows()
    f = cr.Field(t.cells)
    by_x = lambda a: [int(v) for v in a[(t.flags & 2) != 0]]
    for mode in (0, 1):
        got = run(t, None, cr.BLOCKED, 32, mode)
        same(got, f.clearance(cr.BLOCKED, 32), ("tall", mode))
        assert by_x(got["hops"]) == [4, 3, 2, 1, 0, 0] and tuple(got["counts"]) == (2, 6, 4, 0)
        assert by_x(got["nearest"])[:5] == [slope + 6] * 5          # column 5's row: 1 + 1 + 40 + 1 rows in front of it
    got = run(t, None, cr.BLOCKED, 2)
    assert by_x(got["hops"]) == [cr.BEYOND, cr.BEYOND, 2, 1, 0, 0]
    # with the map's edge as a barrier every slope is a source
    got = run(t, None, cr.BLOCKED | cr.OPEN, 32)
    assert by_x(got["hops"]) == [0] * 6 and (got["sides"][(t.flags & 2) == 0] == 0xFF).all()


def test_converged_rounds_do_no_work():
    """behind the last round that changed anything, and the one that found that out, every launch returns at once"""
    t = tall_corridor()
    assert run(t, None, cr.BLOCKED, 32)["worked"] == 5
    assert run(t, None, cr.BLOCKED, 1024)["worked"] == 5
    assert run(t, None, cr.BLOCKED, 3)["worked"] == 3


LDS_ROWS = 9216              # kClrLdsRows
_lattices = {}


def lattice_field(name):
    """a lattice of clearance_ref.LATTICES through the oracle -> (cells, restatement)"""
    from oracle import oracle
    from tests import frontier_ref as fr
    if name not in _lattices:
        cells = oracle.build_grid(cr.lattice(name, fr.P), fr.GL, fr.ZL, fr.IV, "slope", mode=oracle.MODE_INT_OPENMP)
        _lattices[name] = (cells, cr.Field(cells))
    return _lattices[name]


def lattice_premises(name, cells, f):
    """What the GPU tests on the lattice `name` take for granted, asserted on any build of it (the oracle's here, the device's there):
    the exact row count, every row a slope, the angle margin, and per lattice that the answers it is there for are not vacuous."""
    W, H, _ = cr.LATTICES[name]
    n = int(cells["num_nodes"])
    assert n == W * H and (n == name or isinstance(name, str)) and ((np.asarray(cells["flags"][:n]) & 2) != 0).all(), (name, n)
    assert f.angle_margin_deg > MARGIN, (name, f.angle_margin_deg)
    deep = f.clearance(cr.BLOCKED, 64)
    hops = deep["hops"]
    assert deep["counts"][0] > 0 and (hops == 0).any(), name
    if name in (1023, 1024, 1025, 9216, 9217):
        # k_clearance_wg's slot edges and its limit: rows far from the wall, the map's edge a barrier of its own, one hop alone
        assert ((hops > 32) & (hops != cr.BEYOND)).any(), name
        for mask in (cr.BLOCKED, cr.BLOCKED | cr.OPEN):
            assert f.clearance(mask, 64)["counts"][2] >= 6 and f.clearance(mask, 1)["counts"][2] == 1, (name, mask)
        assert (n <= LDS_ROWS) == (name != 9217) and (n == LDS_ROWS) == (name == 9216)
        assert (name < 9216) or (hops == cr.BEYOND).any()
    if name == 1025:
        depth = int(f.clearance(cr.BLOCKED, 1024)["counts"][2])
        assert 3 < depth and (depth + 3) | 1 <= 1024 and (f.clearance(cr.BLOCKED, depth - 1)["hops"] == cr.BEYOND).any()
    if name == 2048:
        assert n == 2048                                   # kWalkTableRowsPerWaypoint x T at T = 1
    if name == 9217:
        assert 2048 * 2 < n <= 2048 * 6                    # the walk's default: inline at T = 2, the table at T = 6
    if name == 131769:
        # the second trip of the grid-stride loops: rows 131 072 .. n - 1 (k_clearance_finish; quads 524 288 .. of the steps and rounds)
        assert 4 * n > 2048 * 256 and n > 512 * 256
        tail = hops[512 * 256:]
        assert (tail == cr.BEYOND).any() and (tail != cr.BEYOND).any() and (hops[:512 * 256] == cr.BEYOND).any() and deep["counts"][2] == 64
    if name == 14641:
        assert n > LDS_ROWS and tuple(deep["counts"]) == (412, 14596, 64, 0)
        assert f.clearance(cr.BLOCKED | cr.OPEN | cr.OVERHEAD, 7)["counts"][2] == 7
    if name == "41x25":
        assert tuple(deep["counts"]) == (68, 1025, 22, 0) and (f.clearance(cr.BLOCKED, 3)["hops"] == cr.BEYOND).any()


@pytest.mark.parametrize("name", list(cr.LATTICES), ids=[str(k) for k in cr.LATTICES])
def test_lattices_have_exact_row_counts_and_the_premises_of_the_gpu_tests(name):
    """tests/clearance_ref.lattice_cloud through the oracle: W x H rows to the row, all slopes, 28.8 degrees from the angle gate, and
    the fields the kernel-edge, scratch-reuse and poisoned tests of the GPU tier expect of them — checked where no GPU exists"""
    cells, f = lattice_field(name)
    lattice_premises(name, cells, f)
    if name == 1024:                                       # the shim runs the kernels' per-row code on one of them
        t = Table(cells["sx"], cells["sy"], cells["sz"], cells["flags"], np.ones(f.n), cells["mean"], cells["normal"], cells["rough"])
        for mask, max_hops in ((cr.BLOCKED, 64), (cr.BLOCKED | cr.OPEN, 1)):
            same(run(t, None, mask, max_hops), f.clearance(mask, max_hops), (name, mask, max_hops))


def test_no_cpu_fallback_for_clearance(native_lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import grid_ndt_amd as g
    m = g.TwoDmap(0.5, 0.5)
    m.setCloudFirst((0, 0, 0))
    for host in (False, True):
        with pytest.raises(g.GndtError) as e:
            m.clearance(host=host)
        assert e.value.code == 2   # GNDT_ERR_NO_DEVICE
