"""CPU tier: frontier extraction's per-row code (grid_ndt_amd/csrc/gndt_frontier.hpp: the candidate and open-side tests, the union-find,
the record reduction), compiled with g++ into tests/_frontier_shim.so and run one row after another, against the restatement from the
rows (tests/frontier_ref.py: a column dict and a breadth-first search) on maps the oracle builds and on 200 random occupancy grids —
every label, every record field, every count, for equality; parent[x] <= x after every union; and the product entry points refuse to
run without a GPU."""
import ctypes as C

import numpy as np
import pytest

from tests import frontier_ref as fr
from tests.host_emulation import MAP, HostMap, MapRows, load_shim
from tests.test_raster_host import SCENES, _boxes

_shim = None


def shim():
    global _shim
    if _shim is None:
        vp, u32 = C.c_void_p, C.c_uint32
        _shim = load_shim("frontier_shim.cpp", "_frontier_shim.so", {
            "fshim_lin": ([C.c_int], C.c_int),
            "fshim_frontiers": ([vp, u32, vp, MAP, vp, vp, vp, u32, vp], C.c_int64),
        })
    return _shim


def run(m, cfg, box=None, min_size=1, order=None, cap=None):
    """the passes on map m (a HostMap or a Grid) -> dict(label, open, clusters [min(listed, cap)], counts), and the untouched tail;
    min_open and min_size 0 mean 1, which the entry point settles before the kernels see them"""
    n = m.n
    min_size = max(min_size, 1)
    rule = np.array([cfg["candidates"], cfg["open_rule"], cfg["level_reach"], max(cfg["min_open"], 1), cfg["link_dz"], int(box is not None)]
                    + list(box if box is not None else (0, 0, 0, 0)), np.int32)
    cap = n if cap is None else cap
    label = np.full(max(n, 1), 0xDEADBEEF, np.uint32)
    opens = np.full(max(n, 1), 0xEE, np.uint8)
    clusters = np.full(max(cap, 1) * 16, 0xA5A5A5A5, np.uint32).view(fr.RECORD)
    counts = np.full(4, 0xDEADBEEF, np.uint32)
    o = None if order is None else np.ascontiguousarray(order, np.uint32)
    rc = shim().fshim_frontiers(rule.ctypes.data, min_size, None if o is None else o.ctypes.data, m.shim_map(), label.ctypes.data,
                                opens.ctypes.data, clusters.ctypes.data, cap, counts.ctypes.data)
    assert rc == 0, f"parent[x] <= x failed at row {rc - 1}"
    k = min(int(counts[0]), cap)
    return dict(label=label[:n], open=opens[:n], clusters=clusters[:k], counts=counts, tail=clusters[k:])


def want(m, ref_map, cfg, box=None):
    return ref_map.frontiers(box=box, h_bits=m.h_bits, state=m.state, **cfg)


def check(m, ref_map, cfg, box=None, min_size=1, order=None, what=""):
    got = run(m, cfg, box, min_size, order)
    ref = want(m, ref_map, cfg, box)
    recs, counts = fr.listed(ref, min_size)
    assert np.array_equal(got["counts"], counts), (what, got["counts"], counts)
    assert np.array_equal(got["label"], ref["label"]), what
    front = ref["label"] != fr.NO_ROW
    assert np.array_equal(got["open"][front], ref["open"][front]) and (got["open"][~front] == 0xFF).all(), what
    assert fr.same_records(got["clusters"], recs), (what, fr.diff_records(got["clusters"], recs))
    return ref


def cfg(candidates=fr.SLOPES, open_rule=fr.OPEN_COLUMN, level_reach=1, min_open=1, link_dz=1):
    return dict(candidates=candidates, open_rule=open_rule, level_reach=level_reach, min_open=min_open, link_dz=link_dz)


# both candidate modes x (OPEN_COLUMN, OPEN_LEVEL at reach 0 / 1 / 3), then min_open 1..4 and link_dz 0 / 1 / 2 under each open rule
CONFIGS = [cfg(c, r, lr) for c in (fr.REACHED, fr.SLOPES) for r, lr in ((fr.OPEN_COLUMN, 1), (fr.OPEN_LEVEL, 0), (fr.OPEN_LEVEL, 1), (fr.OPEN_LEVEL, 3))]
CONFIGS += [cfg(c, r, 1, mo, dz) for c, r in ((fr.SLOPES, fr.OPEN_COLUMN), (fr.REACHED, fr.OPEN_LEVEL))
            for mo, dz in ((2, 1), (3, 1), (4, 1), (0, 1), (1, 0), (1, 2), (2, 0), (2, 2))]

_maps = {}


def _map(name):
    if name not in _maps:
        cloud, P = SCENES[name]()
        m = HostMap(cloud, P, seed=13)
        _maps[name] = (m, fr.Map(m.cells))
    return _maps[name]


def test_lin_closes_the_hole_at_zero():
    for s in (-65535, -3, -2, -1, 1, 2, 3, 65535):
        assert shim().fshim_lin(s) == fr.lin(s)
    assert [shim().fshim_lin(s) for s in (-2, -1, 1, 2)] == [-2, -1, 0, 1]


@pytest.mark.parametrize("name", sorted(SCENES))
def test_every_label_record_and_count_is_the_restatement(name):
    m, ref_map = _map(name)
    some = 0
    for c in CONFIGS:
        ref = check(m, ref_map, c, what=(name, c))
        some += len(ref["clusters"])
    assert some > 0
    # min_size leaves clusters out of the list, not out of the labels or of counts[2]
    for ms in (0, 2, 5, 1 << 30):
        check(m, ref_map, CONFIGS[4], min_size=ms, what=(name, "min_size", ms))


@pytest.mark.parametrize("name", sorted(SCENES))
def test_boxes_as_the_raster_takes_them(name):
    m, ref_map = _map(name)
    for box in _boxes(m):
        for c in (cfg(fr.SLOPES, fr.OPEN_COLUMN), cfg(fr.REACHED, fr.OPEN_LEVEL, 1), cfg(fr.SLOPES, fr.OPEN_LEVEL, 0, 2, 2)):
            check(m, ref_map, c, box=box, what=(name, box, c))


def test_any_link_order_gives_the_same_bytes():
    m, ref_map = _map("bridge_ground")         # the ground's rim and the deck's: two long rings
    c = cfg(fr.SLOPES, fr.OPEN_COLUMN)
    first = run(m, c)
    assert len(first["clusters"]) > 1 and first["clusters"]["size"].max() > 8
    rng = np.random.default_rng(5)
    for order in (np.arange(m.n)[::-1], rng.permutation(m.n), rng.permutation(m.n)):
        got = run(m, c, order=order)
        assert got["label"].tobytes() == first["label"].tobytes() and got["clusters"].tobytes() == first["clusters"].tobytes()
        assert np.array_equal(got["counts"], first["counts"])


def test_a_short_list_is_cut_and_the_rest_untouched():
    m, ref_map = _map("bridge_ground")
    c = cfg(fr.SLOPES, fr.OPEN_LEVEL, 0)
    full = run(m, c)
    n = int(full["counts"][0])
    assert n >= 3
    for cap in (0, 1, n - 1, n, n + 3):
        got = run(m, c, cap=cap)
        assert np.array_equal(got["counts"], full["counts"])
        assert got["clusters"].tobytes() == full["clusters"][:cap].tobytes()
        assert (got["tail"].view(np.uint32) == 0xA5A5A5A5).all()


class Grid(MapRows):
    """A random occupancy grid as rows: side x side columns across the origin in a shuffled order, one to `levels` nodes each at random
    levels on both sides of 0, most of them slopes; a random cost map.  No cloud, no build: the fields frontier extraction reads.
    Its index has 2048 slots whatever the grid: not the library's rule, which gives 1024 up to 512 of the at most 576 columns."""

    def __init__(self, rng, side=24, levels=3):
        fill = rng.uniform(0.3, 0.9)
        cols = [(ix, iy) for ix in range(-side // 2, side // 2) for iy in range(-side // 2, side // 2) if rng.random() < fill]
        cols = [cols[i] for i in rng.permutation(len(cols))]
        pool = np.array([-2, -1, 1, 2, 3])
        sx, sy, sz, ncol = [], [], [], []
        for ix, iy in cols:
            zs = rng.choice(pool, size=rng.integers(1, levels + 1), replace=False)
            for j, z in enumerate(zs):
                sx.append(ix + 1 if ix >= 0 else ix); sy.append(iy + 1 if iy >= 0 else iy); sz.append(int(z))
                ncol.append(len(zs) if j == 0 else 0)
        n = len(sx)
        flags = np.where(rng.random(n) < 0.85, 3, 1)
        super().__init__(dict(sx=sx, sy=sy, sz=sz, flags=flags), ncol, table=2048,
                         h_bits=rng.integers(0, 0x7F7FFFFF, size=n, dtype=np.uint32), state=rng.integers(0, 3, size=n, dtype=np.uint32))
        self.cells = dict(num_nodes=self.n, sx=self.sx, sy=self.sy, sz=self.sz, flags=self.flags)


def test_fuzz_200_random_occupancy_grids():
    rng = np.random.default_rng(20240607)
    for k in range(200):
        g = Grid(rng)
        ref_map = fr.Map(g.cells)
        base = cfg(fr.SLOPES, fr.OPEN_COLUMN)
        ref = check(g, ref_map, base, what=(k, "base"))
        # the restatement alone: the fuzz cannot pass on empty answers
        assert len(ref["clusters"]) and ref["clusters"]["size"].max() >= 2, k
        c = cfg(int(rng.integers(0, 2)), int(rng.integers(0, 2)), int(rng.choice([0, 1, 3])), int(rng.integers(0, 5)), int(rng.integers(0, 3)))
        box = None if rng.random() < 0.5 else tuple(int(v) for v in (rng.integers(-13, 0), rng.integers(1, 14), rng.integers(-13, 0), rng.integers(1, 14)))
        check(g, ref_map, c, box=box, min_size=int(rng.integers(0, 4)), order=rng.permutation(g.n), what=(k, c, box))


def test_no_cpu_fallback_for_frontiers(native_lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import grid_ndt_amd as g
    m = g.TwoDmap(0.5, 0.5)
    m.setCloudFirst((0, 0, 0))
    for host in (False, True):
        with pytest.raises(g.GndtError) as e:
            m.frontiers(candidates="slopes", host=host)
        assert e.value.code == 2   # GNDT_ERR_NO_DEVICE
