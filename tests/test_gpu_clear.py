"""GPU tier: free-space clearing (gndt_clear_rays_device / gndt_clear_rays, TwoDmap.clear_rays).  Count-only passes and protection bits
equal the numpy restatement (tests/clear_ref.py) on every path that writes rows and leave the map untouched; a clear equals gndt_remove
of the dropped nodes' points and the oracle's map of the stream without them; a ghost obstacle seen in one frame is cleared by a later
frame while everything seen stays; min_passes, errors, lifetimes and a hot voxel hit by every ray of a frame."""
import numpy as np
import pytest

from grid_ndt_amd import scenes
from tests import clear_ref as cr
from tests import parity
from tests import query_ref as qr
from tests.gpu_kit import dev, handle

pytestmark = pytest.mark.gpu

ATOMIC, PARTITION, EXACT, TWO_LEVEL, TILE, AUTO = 1, 2, 3, 4, 5, 0
TERRAIN = scenes.TERRAIN_PARAMS
FIELDS = ("sx", "sy", "sz", "count", "first_idx", "mean", "cov", "rough", "normal", "flags")
MASK = np.uint32(0x7FFFFFFF)
DEBUG_CLEAR_EXTENT = 5


def _assert_same(got, want, fields=FIELDS):
    for k in ("num_nodes", "num_columns", "num_slopes"):
        assert got[k] == want[k], (k, got[k], want[k])
    for k in fields:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), k


def _keys(cells):
    return qr.pack(cells["sx"], cells["sy"], cells["sz"])


def _sensor(k, lift=4.0):
    px, py = scenes._pose_xy(np.int64(k), 200.0, 14.0)
    return np.array([px, py, scenes.heightfield(np.array([px]), np.array([py]), 0x5EED0003)[0] + lift], np.float32)


def _words(m, o, pts, **kw):
    st, w = m.clear_rays(o, dev(pts), count_only=True, passes=True, **kw)
    return st, w.cpu().numpy().view(np.uint32)


def _scene(name):
    """-> (make, P, sensor, end points): a function that builds the map of path `name` on a fresh handle"""
    if name in ("atomic", "partition", "two_level"):
        cloud = scenes.terrain_cloud(300_000)
        strategy = {"atomic": ATOMIC, "partition": PARTITION, "two_level": TWO_LEVEL}[name]
        P, sensor, pts = TERRAIN, _sensor(1, 1.8), cloud[150_000::10]
    elif name == "tile":
        cloud, P, strategy = scenes.depth_frame(), scenes.DEPTH_PARAMS, TILE
        c = cloud[1:]
        sensor = np.array([np.median(c[:, 0]), np.median(c[:, 1]), c[:, 2].max() + 1.0], np.float32)
        pts = c[::8]
    else:  # blocked buckets
        P = dict(grid_len=0.5, z_len=0.5, slope_interval=0.08)
        cloud, strategy = scenes.uniform_box(2_500_001, half_xy=50.0), AUTO
        sensor, pts = np.array([3.1, -2.2, 0.7], np.float32), cloud[1::250]
    t = dev(cloud[1:])

    def make():
        m = handle(P, strategy)
        m.setCloudFirst(cloud[0])
        for _ in range(2 if name == "blocked" else 1):
            m.create2DMap("slope", t)
            m.sync()
        if name == "blocked":
            assert m.STRATEGY_NAMES[m.last_strategy()] == "partition_blocked"
        if name == "tile":
            assert m.STRATEGY_NAMES[m.last_strategy()] == "tile"
        return m
    return make, P, cloud[0], sensor, np.ascontiguousarray(pts, np.float32)


@pytest.mark.parametrize("name", ["atomic", "partition", "two_level", "blocked", "tile"])
def test_count_only_is_the_restatement_and_changes_nothing(name):
    import grid_ndt_amd as g
    make, P, origin, sensor, pts = _scene(name)
    m = make()
    before = m.export()
    pts = pts.copy()
    pts[::101] = np.nan
    try:
        for ext in (1, 0):
            g.TwoDmap.set_debug_option(DEBUG_CLEAR_EXTENT, ext)
            for mr, em in ((0.0, 0.0), (15.0, 0.3)):
                want, rays, skipped = cr.passes(before, origin, P["grid_len"], P["z_len"], sensor, pts, mr, em)
                st, got = _words(m, sensor, pts, max_range=mr, end_margin=em)
                assert (st["rays"], st["skipped"], st["cleared"]) == (rays, skipped, 0)
                assert st["protected_rows"] == int(((want & cr.PROTECTED) != 0).sum()) > 0
                assert (want & MASK).max() > 0
                assert np.array_equal(got, want), (name, ext, mr, em, np.flatnonzero(got != want)[:8])
                st_h, got_h = m.clear_rays(sensor, pts, max_range=mr, end_margin=em, count_only=True, passes=True)   # host entry point
                assert st_h == st and np.array_equal(got_h, want)
    finally:
        g.TwoDmap.set_debug_option(DEBUG_CLEAR_EXTENT, 0)
    _assert_same(m.export(), before)


def _rescan(frame, seed=4):
    """the same pose scanned again: every point moved by a little noise"""
    return (frame + np.random.default_rng(seed).normal(0.0, 0.03, frame.shape)).astype(np.float32)


def _twins(P, origin, body):
    """two handles with the same fp64 sums (the statistics of one build merged into both), stream position = len(body)"""
    x = handle(P, ATOMIC)
    x.setCloudFirst(origin)
    x.change2DMap("slope", dev(body))
    st = {k: v.clone() for k, v in x.stats_export().items()}
    out = []
    for _ in range(2):
        m = handle(P, ATOMIC)
        m.setCloudFirst(origin)
        m.reset("slope")
        m.stats_merge(st["key"], st["sums"], st["count"], st["first_idx"])
        m.accumulate("slope", dev(np.zeros((0, 3), np.float32)), first_idx_base=len(body))
        m.finalize()
        out.append(m)
    return out


def test_clear_equals_remove_and_the_oracle():
    """A clears with the rays of the next frame, B removes every point of the nodes A dropped: the same map, and after the next frame
    again; it is the oracle's map of the stream without those points (first_idx through the original positions)"""
    P = TERRAIN
    ppf = 32_768
    fr = scenes.terrain_frames(3, points_per_frame=ppf)
    origin, body, nxt = fr[0], fr[1:2 * ppf], _rescan(fr[ppf:2 * ppf])
    sensor = _sensor(1, 1.8)
    a, b = _twins(P, origin, body)
    before = a.export()
    words, _, _ = cr.passes(before, origin, P["grid_len"], P["z_len"], sensor, nxt)
    drop = cr.cleared_rows(words, 1)
    assert 0 < drop.sum() < before["num_nodes"]
    st, got = a.clear_rays(sensor, dev(nxt), passes=True)
    got = got.cpu().numpy().view(np.uint32)
    assert st["cleared"] == int(drop.sum()) and st["rays"] == len(nxt)
    assert np.array_equal(got[~drop & ((words & cr.PROTECTED) == 0)], words[~drop & ((words & cr.PROTECTED) == 0)])
    sx, sy, sz, _, ok = qr.keys(body, origin, P["grid_len"], P["z_len"])
    assert ok.all()
    gone = np.isin(qr.pack(sx, sy, sz), _keys(before)[drop])
    b.del2DMap("slope", dev(body[gone]))
    ea, eb = a.export(), b.export()
    _assert_same(ea, eb)
    assert not np.isin(_keys(ea), _keys(before)[drop]).any()
    alive = ~gone
    ref = parity.ref_from_cloud(np.concatenate([origin[None], body[alive]]), P)
    ref["first_idx"] = np.flatnonzero(alive)[ref["first_idx"].astype(np.int64)].astype(ref["first_idx"].dtype)
    parity.assert_parity(ea, ref)
    for m in (a, b):
        m.change2DMap("slope", dev(nxt))
    ea, eb = a.export(), b.export()
    for k in ("num_nodes", "num_columns", "num_slopes"):
        assert ea[k] == eb[k]
    for k in ("sx", "sy", "sz", "count", "first_idx", "flags"):
        assert np.array_equal(ea[k], eb[k]), k


def _ghost_stream():
    """four full frames; frame 2 (pose 1) also holds an obstacle hanging in the rays of frame 4 (pose 3): points 35-60 % of the way
    along its rays in a narrow azimuth window 8-25 m out, at least 0.6 m above the ray's end, in voxels no frame point lies in"""
    ppf = scenes.FRAME_POINTS
    fr = scenes.terrain_frames(5, points_per_frame=ppf)
    s3 = _sensor(3)
    p = fr[3 * ppf:4 * ppf]
    d = p - s3
    hd, az = np.hypot(d[:, 0], d[:, 1]), np.arctan2(d[:, 1], d[:, 0])
    idx = np.flatnonzero((hd > 8) & (hd < 25) & (np.abs(az - 0.5) < 0.08))
    t = np.random.default_rng(3).uniform(0.35, 0.6, size=(len(idx), 4))
    obs = (s3[None, None, :] + t[:, :, None] * d[idx][:, None, :]).reshape(-1, 3).astype(np.float32)
    obs = obs[(obs[:, 2] - np.repeat(p[idx, 2], 4)) > 0.6]
    frames = [fr[1:ppf + 1], fr[ppf + 1:2 * ppf + 1], fr[2 * ppf + 1:3 * ppf], p]     # (frames 3 and 4 as the oracle sees them)
    # only voxels no frame point lies in: every node of the obstacle is the obstacle's alone
    P = TERRAIN
    sx, sy, sz, _, _ = qr.keys(obs, fr[0], P["grid_len"], P["z_len"])
    fx, fy, fz, _, _ = qr.keys(fr[1:4 * ppf], fr[0], P["grid_len"], P["z_len"])
    obs = obs[~np.isin(qr.pack(sx, sy, sz), qr.pack(fx, fy, fz))]
    return fr[0], frames, obs, s3


def test_ghost_obstacle_is_cleared():
    P = TERRAIN
    origin, frames, obs, s3 = _ghost_stream()
    assert len(obs) > 1000
    a, b = handle(P, ATOMIC), handle(P, ATOMIC)
    for m in (a, b):
        m.setCloudFirst(origin)
    for k, f in enumerate(frames[:3]):
        a.change2DMap("slope", dev(np.concatenate([f, obs]) if k == 1 else f))
        b.change2DMap("slope", dev(f))
        if k == 1:     # precondition: the obstacle put nodes (and with them rows and labels) that the obstacle-free stream does not have
            ghost_keys = np.setdiff1d(_keys(a.export()), _keys(b.export()))
            assert len(ghost_keys) > 100
    for m in (a, b):
        m.change2DMap("slope", dev(frames[3]))
    ea = a.export()
    ghost_keys = np.setdiff1d(_keys(ea), _keys(b.export()))       # (what later frames did not also put points into)
    assert len(ghost_keys) > 100
    seen = qr.node_rows(ea, frames[3], origin, P["grid_len"], P["z_len"])
    seen_keys = _keys(ea)[seen[seen >= 0]]
    sa = a.clear_rays(s3, dev(frames[3]))
    sb = b.clear_rays(s3, dev(frames[3]))
    assert sa["cleared"] == sb["cleared"] + len(ghost_keys)
    ea, eb = a.export(), b.export()
    assert not np.isin(ghost_keys, _keys(ea)).any()                # the obstacle is gone
    assert np.isin(seen_keys, _keys(ea)).all()                     # nothing that holds an end point of the clearing frame left
    # the same map as the handle that never saw the obstacle (point indices differ by the obstacle's points; fp64 sums by their order)
    _assert_same(ea, eb, ("sx", "sy", "sz", "count", "flags"))
    # ... and both are the oracle's map of their stream without every point of the nodes they cleared: the obstacle's among them
    for e, stream in ((eb, np.concatenate(frames)), (ea, np.concatenate([frames[0], frames[1], obs, frames[2], frames[3]]))):
        cleared = np.setdiff1d(_keys(parity.ref_from_cloud(np.concatenate([origin[None], stream]), P)), _keys(e))
        sx, sy, sz, _, _ = qr.keys(stream, origin, P["grid_len"], P["z_len"])
        alive = ~np.isin(qr.pack(sx, sy, sz), cleared)
        ref = parity.ref_from_cloud(np.concatenate([origin[None], stream[alive]]), P)
        ref["first_idx"] = np.flatnonzero(alive)[ref["first_idx"].astype(np.int64)].astype(ref["first_idx"].dtype)
        parity.assert_parity(e, ref)
    # the cost flood sees the same map on the obstacle's columns
    gsx, gsy, _ = (np.array(v) for v in zip(*[(int(k >> 43) - (1 << 20), int((k >> 22) & 0x1FFFFF) - (1 << 20), 0) for k in ghost_keys]))
    slopes = np.flatnonzero(eb["flags"] & 2)
    goal = tuple(float(v) for v in eb["mean"][slopes[np.argmin(np.hypot(eb["mean"][slopes, 0] - s3[0], eb["mean"][slopes, 1] - s3[1]))]])
    ca, cb = a.computeCost(goal), b.computeCost(goal)
    assert ca["rc"] == cb["rc"] == 0
    ha, hb = a.cost_export(), b.cost_export()
    cols = np.isin(qr.pack(ea["sx"], ea["sy"], 0), qr.pack(gsx, gsy, 0))
    assert cols.sum() > 0
    assert (ha["state"][cols] == hb["state"][cols]).all()
    assert np.allclose(ha["h"][cols], hb["h"][cols], rtol=1e-4)


def test_min_passes():
    P = TERRAIN
    fr = scenes.terrain_frames(3, points_per_frame=32_768)
    origin, body, nxt = fr[0], fr[1:65_537], _rescan(fr[32_769:65_537])
    sensor = _sensor(1, 1.8)
    for mp in (1, 3):
        m = handle(P, ATOMIC)
        m.setCloudFirst(origin)
        m.change2DMap("slope", dev(body))
        before = m.export()
        _, w = _words(m, sensor, nxt)
        st, got = m.clear_rays(sensor, nxt, min_passes=mp, passes=True)      # (host entry point)
        prot = (w & cr.PROTECTED) != 0
        assert ((got & cr.PROTECTED) != 0).tolist() == prot.tolist()
        assert ((got & MASK) <= mp).all()
        assert np.array_equal((got & MASK)[~prot], np.minimum(w & MASK, mp)[~prot]) and ((got & MASK)[prot] == 0).all()
        drop = cr.cleared_rows(w, mp)
        assert st["cleared"] == int(drop.sum()) > 0
        assert np.array_equal(np.sort(_keys(m.export())), np.sort(_keys(before)[~drop]))
        if mp > 1:
            assert ((w & MASK)[~drop & ~prot] < mp).all() and ((w & MASK)[~drop & ~prot] > 0).any()   # rows with fewer passes survive


def test_errors_and_lifetime():
    import torch
    import grid_ndt_amd as g
    P = TERRAIN
    fr = scenes.terrain_frames(3, points_per_frame=32_768)
    origin, f0, f1 = fr[0], fr[1:32_769], fr[32_769:65_537]
    sensor = _sensor(1, 1.8)
    # PARTITION-built: clearing refused, the map unchanged; count-only works
    p = handle(P, PARTITION)
    p.setCloudFirst(origin)
    p.create2DMap("slope", dev(f0))
    before = p.export()
    with pytest.raises(g.GndtError) as e:
        p.clear_rays(sensor, dev(f1))
    assert e.value.code == 1
    _assert_same(p.export(), before)
    assert p.clear_rays(sensor, dev(f1), count_only=True)["rays"] == len(f1)
    m = handle(P, ATOMIC, max_points_hint=200_000, max_nodes_hint=200_000)
    m.setCloudFirst(origin)
    m.change2DMap("slope", dev(f0))
    m.change2DMap("slope", dev(f1))
    f1 = _rescan(f1)
    before = m.export()
    for kw in ({"min_passes": 0}, {"max_range": -1.0}, {"end_margin": float("nan")}, {"max_range": float("inf")}):
        with pytest.raises(g.GndtError) as e:
            m.clear_rays(sensor, dev(f1), **kw)
        assert e.value.code == 1
    for o in ((float("nan"), 0, 0), (1e7, 0, 0)):
        with pytest.raises(g.GndtError) as e:
            m.clear_rays(o, dev(f1))
        assert e.value.code == 1
    st = m.clear_rays(sensor, dev(np.zeros((0, 3), np.float32)))
    assert st == {"rays": 0, "skipped": 0, "protected_rows": 0, "cleared": 0}
    _assert_same(m.export(), before)
    bad = f1.copy()
    bad[::7] = np.nan
    st = m.clear_rays(sensor, dev(bad), count_only=True)
    assert st["skipped"] == len(bad[::7]) and st["rays"] == len(bad) - len(bad[::7])
    # cost map stale after a clear; queries answer from the new map
    cells = m.export()
    slopes = np.flatnonzero(cells["flags"] & 2)
    m.computeCost(tuple(float(v) for v in cells["mean"][slopes[len(slopes) // 2]]))
    w, _, _ = cr.passes(cells, origin, P["grid_len"], P["z_len"], sensor, f1)
    drop = cr.cleared_rows(w, 1)
    assert m.clear_rays(sensor, dev(f1))["cleared"] == int(drop.sum()) > 0
    with pytest.raises(g.GndtError) as e:
        m.cost_export()
    assert e.value.code == 1
    seen = fr[1:65_537]
    sx, sy, sz, _, _ = qr.keys(seen, origin, P["grid_len"], P["z_len"])
    gone = np.isin(qr.pack(sx, sy, sz), _keys(cells)[drop])
    rows = m.query(dev(seen)).cpu().numpy().astype(np.int64)
    assert (rows[gone] == qr.NO_ROW).all() and (rows[~gone] >= 0).all()
    # capture refused; a graph recorded before a clear is reported stale
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        buf = dev(f1)
        s.wait_stream(torch.cuda.default_stream())
        graph = torch.cuda.CUDAGraph()
        with g.graph_capture(graph, s):
            m.change2DMap("slope", buf, s)
        gr2 = torch.cuda.CUDAGraph()
        with pytest.raises(g.GndtError) as e:
            with g.graph_capture(gr2, s):
                m.clear_rays(sensor, buf, stream=s)
        assert e.value.code == 1
        del gr2
        s.synchronize()
        m.clear_rays(sensor, buf, stream=s)
        graph.replay()
        s.synchronize()
        with pytest.raises(g.GndtError) as e:
            m.sync()
        assert e.value.code == 5 and "replay" in str(e.value)
    del graph


def test_hot_voxel_counts_every_ray():
    """131 072 rays from one origin ending in a 3 x 3-column cluster: count-only is exact (wave-aggregated adds), and the origin's row
    counts every ray"""
    P = TERRAIN
    cloud = scenes.terrain_cloud(120_000)
    sensor = np.array([cloud[5000, 0], cloud[5000, 1], cloud[5000, 2] + 1.3], np.float32)
    rng = np.random.default_rng(5)
    near = (sensor[None, :] + rng.uniform(-0.05, 0.05, size=(20, 3))).astype(np.float32)    # nodes at the sensor
    m = handle(P, ATOMIC)
    m.setCloudFirst(cloud[0])
    m.change2DMap("slope", dev(np.concatenate([cloud[1:], near])))
    cells = m.export()
    c = cloud[9000]
    ends = np.empty((scenes.FRAME_POINTS, 3), np.float32)
    ends[:, 0] = c[0] + rng.uniform(-0.29, 0.29, len(ends))
    ends[:, 1] = c[1] + rng.uniform(-0.29, 0.29, len(ends))
    ends[:, 2] = c[2] + rng.uniform(-0.3, 0.3, len(ends))
    want, rays, _ = cr.passes(cells, cloud[0], P["grid_len"], P["z_len"], sensor, ends)
    st, got = _words(m, sensor, ends)
    assert st["rays"] == rays == len(ends)
    assert np.array_equal(got, want)
    orow = qr.node_rows(cells, sensor[None, :], cloud[0], P["grid_len"], P["z_len"])[0]
    assert orow >= 0 and (got[orow] & MASK) == len(ends)
