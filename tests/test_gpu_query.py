"""GPU tier: point queries against the device-resident grid (gndt_query_device / gndt_query, TwoDmap.query).  A NODE query of every
built point names the node the build put it in, on every path that writes rows (each accumulate strategy, the blocked buckets,
updates with and without deferred emit, removal); the column index follows the map from build to build; NEAREST_SLOPE is a brute
force over the exported rows; the cost gather is cost_export() indexed by the rows."""
import numpy as np
import pytest

from grid_ndt_amd import scenes
from tests import query_ref as qr
from tests.gpu_kit import dev, handle

pytestmark = pytest.mark.gpu

ATOMIC, PARTITION, EXACT, TWO_LEVEL, TILE, AUTO = 1, 2, 3, 4, 5, 0
TERRAIN = scenes.TERRAIN_PARAMS
FACE = dict(grid_len=0.5, z_len=0.25, slope_interval=0.08, demand="slope")


def _scene(name):
    return {"bridge_ground": lambda: (scenes.bridge_ground(), scenes.BRIDGE_PARAMS),
            "campus": lambda: (scenes.campus_frame(200_000), scenes.CAMPUS_PARAMS),
            "terrain": lambda: (scenes.terrain_cloud(300_000), TERRAIN),
            "face_lattice": lambda: (qr.face_lattice(grid_len=FACE["grid_len"], z_len=FACE["z_len"]), FACE)}[name]()


def _assert_rows_are_the_builds(m, pts, rows, origin, P, first=True):
    """every point found its node: counts per row, first points (fresh builds), the points' own keys"""
    cells = m.export()
    rows = rows.cpu().numpy().astype(np.int64) if hasattr(rows, "cpu") else np.asarray(rows, np.int64)
    n = cells["num_nodes"]
    assert rows.shape[0] == pts.shape[0] and (rows != qr.NO_ROW).all() and rows.max() < n
    assert (np.bincount(rows, minlength=n) == cells["count"]).all()
    if first:
        assert (rows[cells["first_idx"].astype(np.int64)] == np.arange(n)).all()
    sx, sy, sz, _, ok = qr.keys(pts, origin, P["grid_len"], P["z_len"])
    assert ok.all()
    assert (cells["sx"][rows] == sx).all() and (cells["sy"][rows] == sy).all() and (cells["sz"][rows] == sz).all()
    return cells


@pytest.mark.parametrize("strategy", [ATOMIC, PARTITION, EXACT, TWO_LEVEL, TILE, AUTO])
@pytest.mark.parametrize("name", ["bridge_ground", "campus", "terrain", "face_lattice"])
def test_node_query_of_every_built_point_is_its_node(name, strategy):
    cloud, P = _scene(name)
    m = handle(P, strategy)
    m.setCloudFirst(cloud[0])
    t = dev(cloud[1:])
    m.create2DMap("slope", t)
    rows = m.query(t)
    _assert_rows_are_the_builds(m, cloud[1:], rows, cloud[0], P)
    if strategy == PARTITION and name == "bridge_ground":
        assert m.last_strategy() == 6        # at most 512 buckets: the one-level partition
    # the host entry point answers the same
    assert (m.query(cloud[1:]) == rows.cpu().numpy()).all()


def test_node_query_after_blocked_buckets():
    """AUTO's second build of a dense uniform box takes the blocked buckets (divide-free keys with their border fallback):
    the query, keying with the IEEE divide, names the same nodes"""
    P = dict(grid_len=0.5, z_len=0.5, slope_interval=0.08)
    cloud = scenes.uniform_box(2_500_001, half_xy=50.0)
    m = handle(P)
    m.setCloudFirst(cloud[0])
    t = dev(cloud[1:])
    for _ in range(2):
        m.create2DMap("slope", t)
        m.sync()
    assert m.STRATEGY_NAMES[m.last_strategy()] == "partition_blocked"
    _assert_rows_are_the_builds(m, cloud[1:], m.query(t), cloud[0], P)


@pytest.mark.parametrize("deferred", [False, True])
def test_node_query_after_updates_and_removal(deferred):
    cloud, P = scenes.terrain_cloud(240_000), TERRAIN
    m = handle(P, ATOMIC)
    m.setCloudFirst(cloud[0])
    if deferred:
        m.set_deferred_emit(True)
    cuts = [1, 90_000, 170_000, cloud.shape[0]]
    for a, b in zip(cuts[:-1], cuts[1:]):
        m.change2DMap("slope", dev(cloud[a:b]))
        got = m.query(dev(cloud[1:b]))
        _assert_rows_are_the_builds(m, cloud[1:b], got, cloud[0], P, first=False)
    # the last batch leaves again: the rest still finds its nodes, and nothing names a row beyond the map
    m.del2DMap("slope", dev(cloud[170_000:]))
    _assert_rows_are_the_builds(m, cloud[1:170_000], m.query(dev(cloud[1:170_000])), cloud[0], P, first=False)


def test_index_follows_the_map_from_build_to_build():
    """build A, query, build B on the same handle, query: B's rows (a column index left from A would name A's)"""
    a, P = scenes.campus_frame(200_000), scenes.CAMPUS_PARAMS
    b = scenes.campus_frame(150_000, seed=0x5EED0777)
    b[1:, :2] += np.float32(3.7)                     # another map, same origin
    b[0] = a[0]
    for strategy in (AUTO, ATOMIC):
        m = handle(P, strategy)
        m.setCloudFirst(a[0])
        m.create2DMap("slope", dev(a[1:]))
        _assert_rows_are_the_builds(m, a[1:], m.query(dev(a[1:])), a[0], P)
        m.create2DMap("slope", dev(b[1:]))
        _assert_rows_are_the_builds(m, b[1:], m.query(dev(b[1:])), a[0], P)
    # ... and an update in place of B
    m = handle(P, ATOMIC)
    m.setCloudFirst(a[0])
    m.change2DMap("slope", dev(a[1:]))
    _assert_rows_are_the_builds(m, a[1:], m.query(dev(a[1:])), a[0], P, first=False)
    m.change2DMap("slope", dev(b[1:]))
    both = np.concatenate([a[1:], b[1:]])
    _assert_rows_are_the_builds(m, both, m.query(dev(both)), a[0], P, first=False)


@pytest.mark.parametrize("name", ["bridge_ground", "terrain", "face_lattice"])
def test_nearest_slope_matches_a_brute_force_over_the_rows(name):
    cloud, P = _scene(name)
    m = handle(P)
    m.setCloudFirst(cloud[0])
    m.create2DMap("slope", dev(cloud[1:]))
    cells = m.export()
    body = cloud[1:]
    lo, hi = body.min(0), body.max(0)
    rng = np.random.default_rng(4)
    pts = rng.uniform(lo - 0.5, hi + 0.5, size=(200_000, 3)).astype(np.float32)
    pts[:1000, 2] = rng.uniform(-1e4, 1e4, size=1000).astype(np.float32)            # z far from every slope
    pts = np.concatenate([pts, body[:50_000], qr.odd_points(cloud[0], P["grid_len"], P["z_len"], (float(lo.min()), float(hi.max())))])
    want = qr.nearest_slope_rows(cells, pts, cloud[0], P["grid_len"], P["z_len"])
    got = m.query(dev(pts), "nearest_slope").cpu().numpy()
    assert (got == want).all(), np.flatnonzero(got != want)[:10]
    assert (want >= 0).mean() > 0.1 and (want == qr.NO_ROW).any()
    assert (m.query(pts, "nearest_slope") == want).all()


def test_cost_gather_is_cost_export_at_the_rows():
    import grid_ndt_amd as g
    cloud, P = scenes.bridge_ground(), scenes.BRIDGE_PARAMS
    m = handle(P)
    m.setCloudFirst(cloud[0])
    t = dev(cloud[1:])
    m.create2DMap("slope", t)
    with pytest.raises(g.GndtError) as e:           # no cost map yet
        m.query(t, cost=True)
    assert e.value.code == 1
    m.computeCost((9.5, 3.0, 1.0), robot={"radius": 0.25})
    ce = m.cost_export()
    rng = np.random.default_rng(2)
    lo, hi = cloud[1:].min(0), cloud[1:].max(0)
    pts = np.concatenate([cloud[1:], rng.uniform(lo - 2, hi + 2, size=(50_000, 3)).astype(np.float32),
                          np.float32([[np.nan, 0, 0], [1e9, 1e9, 0]])])
    for mode in ("node", "nearest_slope"):
        rows, h, st = (x.cpu().numpy() for x in m.query(dev(pts), mode, cost=True))
        hit = rows >= 0
        assert hit.any() and (~hit).any()
        assert (h[hit].view(np.uint32) == ce["h"][rows[hit]].view(np.uint32)).all()
        assert (st[hit] == ce["state"][rows[hit]]).all()
        assert (h[~hit] == qr.FLT_MAX).all() and (st[~hit] == 0).all()
        hr, hh, hs = m.query(pts, mode, cost=True)          # host entry point: the same
        assert (hr == rows).all() and (hh.view(np.uint32) == h.view(np.uint32)).all() and (hs == st).all()
    assert (ce["h"][rows[rows >= 0]] < qr.FLT_MAX).any()
    m.create2DMap("slope", t)                        # a new build: its cost map does not exist yet
    with pytest.raises(g.GndtError) as e:
        m.query(t, cost=True)
    assert e.value.code == 1


def test_edge_cases():
    import torch
    import grid_ndt_amd as g
    cloud, P = scenes.campus_frame(100_000), scenes.CAMPUS_PARAMS
    m = handle(P)
    m.setCloudFirst(cloud[0])
    with pytest.raises(g.GndtError) as e:            # no build yet
        m.query(dev(cloud[1:10]))
    assert e.value.code == 1
    t = dev(cloud[1:])
    m.create2DMap("slope", t)
    assert m.query(t[:0]).shape == (0,) and m.query(cloud[1:1]).shape == (0,)      # n = 0
    t4 = torch.cat([t, torch.full((t.shape[0], 1), 5.0, device=t.device)], 1).contiguous()
    r3 = m.query(t)
    assert torch.equal(m.query(t4), r3)                                           # stride 16 = stride 12
    assert (m.query(cloud[1:]) == r3.cpu().numpy()).all()                           # host = device
    for bad in (2, -1):
        with pytest.raises(g.GndtError) as e:
            m.query(t, bad)
        assert e.value.code == 1
    # an empty map: every answer is "no row"
    e0 = handle(P)
    e0.setCloudFirst(cloud[0])
    e0.create2DMap("slope", np.zeros((0, 3), np.float32))
    assert e0.sync()[0] == 0
    for mode in ("node", "nearest_slope"):
        assert (e0.query(t, mode).cpu().numpy() == qr.NO_ROW).all()
        assert (e0.query(cloud[1:], mode) == qr.NO_ROW).all()


@pytest.mark.parametrize("hint", [1 << 20, 0])
def test_full_size_s2_query_of_its_ten_million_points(hint):
    """The bench workload (10 M uniform points, 0.5 m cells), built with and without max_nodes_hint, then all its points queried"""
    cloud = scenes.uniform_box(10_000_001)
    P = dict(grid_len=0.5, z_len=0.5, slope_interval=0.08)
    m = handle(P, max_nodes_hint=hint)
    m.setCloudFirst(cloud[0])
    t = dev(cloud[1:])
    m.create2DMap("slope", t)
    n = m.sync()[0]
    rows = m.query(t).cpu().numpy().astype(np.int64)
    assert (rows >= 0).all()
    cells = m.export()
    assert (np.bincount(rows, minlength=n) == cells["count"]).all()
    assert (rows[cells["first_idx"].astype(np.int64)] == np.arange(n)).all()
