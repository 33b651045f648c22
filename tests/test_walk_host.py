"""CPU tier: the path walks' per-path code (grid_ndt_amd/csrc/gndt_walk.hpp: the start, the step through a side — found with the gates
or read from the steps table — the checks and the sums), compiled with g++ into tests/_walk_shim.so and run one path after another,
against the restatement (tests/walk_ref.py) on maps the oracle builds, on 200 random cell tables and on a column taller than the step
mask: every field of every path and every row for equality, both variants.  The walk's properties on every map; a path driven there
and back; rollouts.arcs against the closed form; and the product entry points refuse to run without a GPU."""
import ctypes as C

import numpy as np
import pytest

from tests import clearance_ref as cr
from tests import walk_ref as wr
from tests.host_emulation import MAP, HostMap, load_shim
from tests.test_clearance_host import FUZZ_ROBOT, MARGIN, Table, random_table, tall_corridor
from tests.test_raster_host import SCENES

_shim = None
MODES = {"node": 0, "nearest_slope": 1}          # kQueryNode / kQueryNearestSlope


def shim():
    global _shim
    if _shim is None:
        vp, u32 = C.c_void_p, C.c_uint32
        _shim = load_shim("walk_shim.cpp", "_walk_shim.so",
                          {"wshim_walk": ([C.c_int, vp, vp, MAP, vp, vp, u32, C.c_uint64, u32, vp, u32, vp], C.c_int)})
    return _shim


def run(t, origin, grid_len, z_len, paths, table, robot=None, start_mode="nearest_slope", overhead=False, hops=None, min_hops=0, max_steps=0,
        row_cap=0):
    """the shim's walks on Table t -> (info, rows)"""
    rb = dict(cr.ROBOT)
    rb.update(robot or {})
    r4 = np.array([rb["radius"], rb["reachable_height"], rb["max_rough"], rb["max_angle_deg"]], np.float32)
    rule = np.array([MODES[start_mode], 1 if overhead else 0, min_hops, max_steps or wr.DEFAULT_STEPS], np.uint32)
    paths = np.ascontiguousarray(paths, np.float32)
    K, T, sf = paths.shape
    info = np.zeros(max(K, 1), wr.INFO_DTYPE)
    info.view(np.uint32)[:] = 0xDEADBEEF
    rows = np.full((K, row_cap), 0xDEADBEEF, np.uint32)
    hp = None if hops is None else np.ascontiguousarray(hops, np.uint32)
    p = lambda a: a.ctypes.data if a is not None and a.size else None
    rc = shim().wshim_walk(int(table), p(r4), p(rule), t.shim_map(origin=origin, grid_len=grid_len, z_len=z_len), p(hp), p(paths), sf, K, T,
                           p(rows), row_cap, p(info))
    assert rc == 0
    return info[:K], rows


def lin(s):
    return np.where(np.asarray(s) > 0, np.asarray(s) - 1, np.asarray(s))


def random_paths(rng, K, T, lo, hi, z_lo, z_hi, reach=3.0, sf=3, on=None):
    """K polylines inside (and a little outside) the rectangle lo..hi: random first waypoints — every other one at one of the points
    `on` (slopes' means: a sparse map is rarely hit by chance) — steps of up to `reach`, z drawn once a path; every fifth path ends
    early at a NaN, one in sixteen runs to a point the codec cannot key"""
    paths = np.zeros((K, T, sf), np.float32)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    pad = 0.05 * (hi - lo)
    paths[:, 0, :2] = rng.uniform(lo - pad, hi + pad, (K, 2))
    if on is not None:
        paths[::2, 0, :2] = on[rng.integers(0, len(on), len(paths[::2])), :2]
    for j in range(1, T):
        paths[:, j, :2] = paths[:, j - 1, :2] + rng.uniform(-reach, reach, (K, 2))
    paths[:, :, 2] = rng.uniform(z_lo, z_hi, (K, 1))
    if sf == 4:
        paths[:, :, 3] = 7.0
    for p in range(K):
        if T > 1 and p % 5 == 4:
            j = int(rng.integers(1, T))
            paths[p, j, int(rng.integers(0, 2))] = np.nan
            paths[p, j + 1:, :2] = 1e30                      # (behind the terminator: never looked at)
        if T > 1 and p % 16 == 7:
            paths[p, int(rng.integers(1, T)), 0] = 1e9       # beyond +-65535 columns
    return paths


def node_starts(rng, paths, t, origin, grid_len, z_len):
    """three paths in four start at the centre of a random node's voxel (a slope's or not), the whole path at that z"""
    r = rng.integers(0, t.n, len(paths))
    centre = np.asarray(origin, np.float64) + (np.stack([lin(t.sx[r]), lin(t.sy[r]), lin(t.sz[r])], 1) + 0.5) * [grid_len, grid_len, z_len]
    some = rng.random(len(paths)) < 0.75
    paths[some, 0, :3] = centre[some]
    paths[:, :, 2] = paths[:, :1, 2]


def properties(w, paths, info, walked, what):
    """what holds on every map: a walk moves one 4-neighbour column at a time (no index 0), along steps of the clearance graph, and a
    DONE path takes the Manhattan column distance of its segments"""
    edges = set(zip(w.f.edge_from.tolist(), w.f.edge_to.tolist()))
    sx, sy = np.asarray(w.sx), np.asarray(w.sy)
    for p, stood in enumerate(walked):
        assert len(stood) == (int(info["steps"][p]) + 1 if info["status"][p] != wr.NO_START else 0), (what, p)
        for a, b in zip(stood[:-1], stood[1:]):
            assert (a, b) in edges, (what, p, a, b)
            assert (sx[b], sy[b]) in cr.sides_of(int(sx[a]), int(sy[a])), (what, p, a, b)
        if info["status"][p] == wr.DONE:
            pts = paths[p, :int(info["waypoints"][p]), :3].copy()
            pts[:, 2] = pts[0, 2]
            kx, ky, _, ok, _ = wr.qr.keys(pts, w.origin, w.grid_len, w.z_len)
            assert ok.all(), (what, p)
            assert int(info["steps"][p]) == int(np.abs(np.diff(lin(kx))).sum() + np.abs(np.diff(lin(ky))).sum()), (what, p)
            j = int(info["waypoints"][p])
            assert j == paths.shape[1] or not np.isfinite(paths[p, j, :2]).all(), (what, p)


def both(t, w, paths, what, **kw):
    """both variants against the restatement -> (info, walked)"""
    want_info, want_rows, walked = w.walk(paths, **kw)
    for table in (False, True):
        info, rows = run(t, w.origin, w.grid_len, w.z_len, paths, table, robot=w.robot, **kw)
        wr.same(info, rows, want_info, want_rows, (what, "table" if table else "inline"))
    properties(w, paths, want_info, walked, what)
    return want_info, walked


_maps = {}


def _map(name):
    if name not in _maps:
        cloud, P = SCENES[name]()
        m = HostMap(cloud, P, seed=13)
        _maps[name] = (m, m, wr.Walker(m.cells, m.origin, P["grid_len"], P["z_len"]))      # (map, the table the shim runs on, walker)
    return _maps[name]


@pytest.mark.parametrize("name", sorted(SCENES))
def test_oracle_scenes_both_variants_are_the_restatement(name):
    m, t, w = _map(name)
    assert w.f.angle_margin_deg > MARGIN, w.f.angle_margin_deg
    rng = np.random.default_rng(77)
    g = m.P["grid_len"]
    lo = m.origin[:2] + np.array([lin(m.sx.min()), lin(m.sy.min())]) * g
    hi = m.origin[:2] + np.array([lin(m.sx.max()) + 1, lin(m.sy.max()) + 1]) * g
    zs = m.mean[(m.flags & 2) != 0][:, 2]
    hops = rng.integers(0, 6, t.n).astype(np.uint32)
    seen = set()
    for K, T, sf, kw in ((40, 6, 3, dict(row_cap=12)), (24, 9, 4, dict(start_mode="node", row_cap=3)),
                         (32, 5, 3, dict(overhead=True, hops=hops, min_hops=1, row_cap=40)), (16, 4, 3, dict(max_steps=5, hops=hops)),
                         (8, 1, 4, dict(row_cap=2))):
        paths = random_paths(rng, K, T, lo, hi, float(zs.min()) - 0.2, float(zs.max()) + 0.2, reach=4 * g, sf=sf, on=m.mean[(m.flags & 2) != 0])
        if kw.get("start_mode") == "node":                  # most starts in a node of the map, or the node lookup finds nothing
            node_starts(rng, paths, t, m.origin, g, m.P["z_len"])
        info, _ = both(t, w, paths, (name, K, T, sf), **kw)
        seen |= set(info["status"].tolist())
    print(name, "statuses:", sorted(seen))
    assert wr.DONE in seen and len(seen) >= 3, seen


def test_fuzz_200_random_cell_tables():
    rng = np.random.default_rng(20241019)
    skipped, tables = 0, 200
    seen = {}
    multi = 0
    for k in range(tables):
        t = random_table(rng)
        w = wr.Walker(t.cells, (0.0, 0.0, 0.0), 0.5, 0.25, FUZZ_ROBOT)
        if w.f.angle_margin_deg <= MARGIN:
            skipped += 1
            continue
        hops = rng.integers(0, 5, t.n).astype(np.uint32)
        kw = [dict(row_cap=8), dict(hops=hops, min_hops=int(rng.integers(0, 3)), row_cap=30), dict(overhead=True, max_steps=int(rng.integers(1, 9))),
              dict(start_mode="node", row_cap=1)][k % 4]
        paths = random_paths(rng, 12, int(rng.integers(1, 7)), (-4.5, -4.5), (4.5, 4.5), 0.0, 0.6, reach=2.0, sf=3 + k % 2)
        if kw.get("start_mode") == "node":
            node_starts(rng, paths, t, (0.0, 0.0, 0.0), 0.5, 0.25)
        info, walked = both(t, w, paths, k, **kw)
        for s in info["status"].tolist():
            seen[s] = seen.get(s, 0) + 1
        multi += sum(len(w.steps.get((a, cr.sides_of(w.sx[a], w.sy[a]).index((w.sx[b], w.sy[b]))), ())) > 1
                     for st in walked for a, b in zip(st[:-1], st[1:]))
    print("fuzz:", dict(skipped=skipped, statuses=seen, steps_with_a_choice=multi))
    assert skipped <= tables * 5 // 100, skipped
    assert all(seen.get(s, 0) > 0 for s in range(7)), seen
    assert multi > 20, multi


def test_a_step_into_a_column_taller_than_the_step_mask():
    """tall_corridor: columns x = 1 .. 6 along y = 1, column 3 forty nodes tall with its only slope at node 35, column 6 a metre up"""
    t = tall_corridor()
    w = wr.Walker(t.cells, (0.0, 0.0, 0.0), 0.5, 0.25)
    slopes = np.flatnonzero((t.flags & 2) != 0)
    paths = np.float32([[[0.25, 0.25, 0.05], [2.75, 0.25, 0.05]], [[2.25, 0.25, 0.05], [0.25, 0.25, 0.05]], [[1.25, 0.25, 0.05], [1.25, 0.75, 0.05]]])
    info, walked = both(t, w, paths, "tall", row_cap=6)
    assert info["status"].tolist() == [wr.BLOCKED, wr.DONE, wr.LEFT_MAP] and info["stop_side"].tolist() == [2, wr.NO_SIDE, 1]
    assert walked[0] == slopes[:5].tolist() and walked[1] == slopes[:5][::-1].tolist() and walked[2] == [int(slopes[2])]
    assert slopes[2] - np.flatnonzero(t.row_ncol == 40)[0] == 35


def plateau(rng, side=12):
    """one level of side x side cells around the origin, every row a slope, means jittered inside their cells, level normals"""
    idx = [i for i in range(-side // 2, side // 2 + 1) if i != 0]
    sx, sy = np.meshgrid(idx, idx, indexing="ij")
    sx, sy = sx.ravel(), sy.ravel()
    n = sx.size
    mean = np.stack([(lin(sx) + rng.uniform(0.2, 0.8, n)) * 0.5, (lin(sy) + rng.uniform(0.2, 0.8, n)) * 0.5, rng.uniform(0.02, 0.08, n)], 1)
    return Table(sx, sy, np.ones(n), np.full(n, 3), np.ones(n), mean, np.tile(np.float32([0, 0, 1]), (n, 1)), np.full(n, 0.01))


def test_there_and_back_over_a_plateau():
    """A path and its reverse stand on the same slopes in opposite order (no segment here passes within 1e-3 of a lattice corner, where
    the tie rule could choose another column).  TravelCost is symmetric to the bit (the fp32 differences negate exactly), so both
    lengths sum the same fp64 terms in opposite order: the fp64 sums differ by rounding of the order of n 2^-53, and the one rounding
    to fp32 can then fall on either side of a tie — equal or 1 ulp apart, never more.  The same holds for climb."""
    rng = np.random.default_rng(5)
    t = plateau(rng)
    w = wr.Walker(t.cells, (0.0, 0.0, 0.0), 0.5, 0.25)
    K, T = 48, 5
    paths = np.zeros((K, T, 3), np.float32)
    paths[:, :, :2] = (rng.integers(-5, 5, (K, T, 2)) + rng.uniform(0.3, 0.7, (K, T, 2))) * 0.5
    paths[:, :, 2] = 0.05
    paths[:, :, 0] += np.float32(0.013) * np.arange(T)[None, :]          # (no segment through a corner: the slopes are irrational enough)
    fwd, walked_f = both(t, w, paths, "there", row_cap=40)
    back, walked_b = both(t, w, paths[:, ::-1].copy(), "back", row_cap=40)
    assert (fwd["status"] == wr.DONE).all() and (back["status"] == wr.DONE).all() and fwd["steps"].sum() > 300
    for p in range(K):
        assert walked_f[p] == walked_b[p][::-1], p
    for k in ("length", "climb"):
        ulps = np.abs(fwd[k].view(np.int32).astype(np.int64) - back[k].view(np.int32).astype(np.int64))
        assert ulps.max() <= 1, (k, ulps.max())
    assert np.array_equal(fwd["rough_max"], back["rough_max"]) and np.array_equal(fwd["steps"], back["steps"])


def test_arcs_are_the_closed_form():
    from grid_ndt_amd import rollouts
    pose = (1.5, -2.0, 0.3, 0.4)
    v, dt, T = 0.8, 0.25, 9
    omegas = np.array([-1.2, -0.3, 0.0, 0.5, 2.0])
    a = rollouts.arcs(pose, v, omegas, dt, T)
    assert a.shape == (5, T, 3) and a.dtype == np.float32 and (a[:, 0] == np.float32(pose[:3])).all() and (a[:, :, 2] == np.float32(0.3)).all()
    t = np.arange(T) * dt
    for i, om in enumerate(omegas):
        if om == 0.0:
            want = np.stack([pose[0] + v * t * np.cos(pose[3]), pose[1] + v * t * np.sin(pose[3])], 1)
        else:
            # a circle of radius v / |w| whose centre lies to the left (w > 0) of the pose: every waypoint is on it, chord by chord
            r = v / om
            centre = np.array([pose[0] - r * np.sin(pose[3]), pose[1] + r * np.cos(pose[3])])
            assert np.allclose(np.hypot(*(a[i, :, :2] - centre).T), abs(r), atol=1e-5)
            want = centre + r * np.stack([np.sin(pose[3] + om * t), -np.cos(pose[3] + om * t)], 1)
        assert np.allclose(a[i, :, :2], want, atol=1e-5), i
        chord = np.hypot(*np.diff(a[i, :, :2], axis=0).T)
        assert np.allclose(chord, chord[0], atol=1e-5) and chord[0] <= v * dt + 1e-6
    torch = pytest.importorskip("torch")
    b = rollouts.arcs(torch.tensor(pose, dtype=torch.float32), v, omegas, dt, T)
    assert isinstance(b, torch.Tensor) and b.dtype == torch.float32 and np.allclose(b.numpy(), a, atol=1e-5)
    info = dict(status=np.array([2, 0, 0, 0, 6]), length=np.float32([1, 3, 2, 2, 1]))
    assert rollouts.choose(info, np.float32([0, 5, 5, 5, 0])) == 2 and rollouts.choose(info, np.float32([0, 5, 5, 4, 0])) == 3
    assert rollouts.choose(dict(status=np.array([1, 2]), length=np.float32([0, 0])), np.float32([0, 0])) == -1


def test_no_cpu_fallback_for_walks(native_lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import grid_ndt_amd as g
    m = g.TwoDmap(0.5, 0.5)
    m.setCloudFirst((0, 0, 0))
    for host in (False, True):
        with pytest.raises(g.GndtError) as e:
            m.walk_paths(np.zeros((2, 3, 3), np.float32), host=host)
        assert e.value.code == 2   # GNDT_ERR_NO_DEVICE
