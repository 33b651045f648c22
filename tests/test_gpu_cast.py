"""GPU tier: ray casting (gndt_cast_rays_device / gndt_cast_rays, TwoDmap.cast_rays / cast_scan).  Rows, range bits and d2 bits equal the
numpy restatement (tests/cast_ref.py) in both modes on maps of three build paths, through both entry points, at every stride and at
batch sizes around a wave; waves whose lanes leave the walk at different steps; cross-checks against the count-only clearing walk and
the NODE query, which share no code with the restatement; the map is left untouched; repeat calls and other streams give the same
bits; errors, capture and the empty batch.

The restatement is computed once per map, mode and kind of origin for about 2 000 rays; rays are independent, so every smaller batch
is a slice of it."""
import ctypes as C

import numpy as np
import pytest

from grid_ndt_amd import scenes
from grid_ndt_amd.map2d import _stream_ptr
from tests import cast_ref as cf
from tests import query_ref as qr
from tests.gpu_kit import dev

pytestmark = pytest.mark.gpu

ATOMIC, PARTITION, TILE = 1, 2, 5
VOXEL, NDT = cf.VOXEL, cf.NDT
MODE_NAMES = {VOXEL: "voxel", NDT: "ndt"}
FIELDS = ("sx", "sy", "sz", "count", "first_idx", "mean", "cov", "rough", "normal", "flags")
N = 2000


def _sensor(k, lift):
    px, py = scenes._pose_xy(np.int64(k), 200.0, 14.0)
    return np.array([px, py, scenes.heightfield(np.array([px]), np.array([py]), 0x5EED0003)[0] + lift], np.float32)


_scenes = {}


def scene(name):
    """test_gpu_clear.py's recipes: the 300 k-point terrain under ATOMIC and PARTITION, the depth frame under TILE -> dict(m, P, origin,
    sensor, pts (the scan's end points), ends (N rays past them, every fourth lifted into the sky, a few NaN), origins (per ray), cells)"""
    if name not in _scenes:
        import grid_ndt_amd as g
        if name in ("atomic", "partition"):
            cloud, P = scenes.terrain_cloud(300_000), scenes.TERRAIN_PARAMS
            strategy = {"atomic": ATOMIC, "partition": PARTITION}[name]
            sensor, pts = _sensor(1, 1.8), cloud[150_000::10]
        else:
            cloud, P, strategy = scenes.depth_frame(), scenes.DEPTH_PARAMS, TILE
            c = cloud[1:]
            sensor = np.array([np.median(c[:, 0]), np.median(c[:, 1]), c[:, 2].max() + 1.0], np.float32)
            pts = c[::8]
        m = g.TwoDmap(P["grid_len"], P["z_len"], strategy=strategy)
        m.setInterval(P["slope_interval"])
        m.setCloudFirst(cloud[0])
        m.create2DMap("slope", dev(cloud[1:]))
        m.sync()
        if name == "tile":
            assert m.STRATEGY_NAMES[m.last_strategy()] == "tile"
        pts = np.ascontiguousarray(pts[:, :3], np.float32)
        p = pts[np.linspace(0, len(pts) - 1, N).astype(np.int64)]
        ends = (sensor[None, :] + np.float32(1.5) * (p - sensor[None, :])).astype(np.float32)
        ends[::4, 2] = sensor[2] + np.abs(ends[::4, 2] - sensor[2]) + np.float32(5.0)
        ends[7::97] = np.nan
        ends[11::193, 1] = np.inf
        jitter = np.random.default_rng(23).uniform(-0.3, 0.3, size=ends.shape).astype(np.float32)
        _scenes[name] = dict(m=m, P=P, origin=cloud[0], sensor=sensor, pts=pts, ends=ends, origins=(sensor[None, :] + jitter).astype(np.float32),
                             cells=m.export(), refs={})
    return _scenes[name]


def ref(s, mode, per_ray=False, **kw):
    key = (mode, per_ray, tuple(sorted(kw.items())))
    if key not in s["refs"]:
        s["refs"][key] = cf.cast(s["cells"], s["origin"], s["P"]["grid_len"], s["P"]["z_len"], s["origins"] if per_ray else s["sensor"],
                                 s["ends"], mode=mode, **kw)
    return s["refs"][key]


def sliced(want, n):
    return {k: want[k][:n] for k in ("row", "range", "d2")}


def host(out):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in out.items()}


def pad4(a):
    return np.concatenate([a, np.full((len(a), 1), 7.0, np.float32)], 1)


@pytest.mark.parametrize("mode", [VOXEL, NDT])
@pytest.mark.parametrize("name", ["atomic", "partition", "tile"])
def test_both_entry_points_equal_the_restatement_bit_for_bit(name, mode):
    s = scene(name)
    m, mn = s["m"], MODE_NAMES[mode]
    want = ref(s, mode)
    hit = want["row"] != cf.NO_ROW
    assert hit.sum() > 100 and (want["status"] == cf.MISS).sum() > 100 and (want["status"] == cf.SKIPPED).sum() > 10
    ends = s["ends"]
    # shared origin (stride 0): device and host, end strides 12 and 16, the stats
    out, st = m.cast_rays(s["sensor"], dev(ends), mode=mn, stats=True)
    cf.assert_same(host(out), want, (name, mode, "device"))
    assert st == want["stats"]
    cf.assert_same(host(m.cast_rays(s["sensor"], dev(pad4(ends)), mode=mn)), want, "device, stride 16")
    out, st = m.cast_rays(s["sensor"], ends, mode=mn, stats=True)
    cf.assert_same(out, want, "host")
    assert st == want["stats"]
    cf.assert_same(m.cast_rays(s["sensor"], pad4(ends), mode=mn), want, "host, stride 16")
    # batches around a wave: every lane count of the last wave's tally, with the tally and without, device and host
    for n in (1, 63, 64, 65):
        out, st = m.cast_rays(s["sensor"], dev(ends[:n]), mode=mn, stats=True)
        cf.assert_same(host(out), sliced(want, n), n)
        assert st["rays"] + st["skipped"] == n and st["hits"] == int((want["row"][:n] != cf.NO_ROW).sum())
        cf.assert_same(host(m.cast_rays(s["sensor"], dev(ends[:n]), mode=mn)), sliced(want, n), (n, "no stats"))
        out, st_h = m.cast_rays(s["sensor"], ends[:n], mode=mn, stats=True)
        cf.assert_same(out, sliced(want, n), (n, "host"))
        assert st_h == st
    # per-ray origins: strides 12 and 16, device and host
    want = ref(s, mode, per_ray=True)
    assert (want["row"] != cf.NO_ROW).sum() > 100
    for o in (s["origins"], pad4(s["origins"])):
        cf.assert_same(host(m.cast_rays(dev(o), dev(ends), mode=mn)), want, ("device origins", o.shape))
        cf.assert_same(m.cast_rays(o, ends, mode=mn), want, ("host origins", o.shape))
    for n in (1, 63, 64, 65):
        cf.assert_same(host(m.cast_rays(dev(s["origins"][:n]), dev(ends[:n]), mode=mn)), sliced(want, n), (n, "device origins"))
        cf.assert_same(m.cast_rays(s["origins"][:n], ends[:n], mode=mn), sliced(want, n), (n, "host origins"))


@pytest.mark.parametrize("mode", [VOXEL, NDT])
def test_parameters_equal_the_restatement(mode):
    s = scene("atomic")
    L = np.linalg.norm(s["ends"][np.isfinite(s["ends"]).all(1)] - s["sensor"], axis=1)
    mid = float(np.median(L)) / 1.5 * 0.8
    cases = [dict(max_range=mid), dict(min_range=mid), dict(min_count=6), dict(max_range=1.2 * mid, min_range=0.7 * mid, min_count=4)]
    if mode == NDT:
        cases += [dict(max_d2=4.0), dict(cov_rel=0.05, cov_floor=1e-4, max_d2=1.5)]
    base = ref(s, mode)
    for kw in cases:
        want = ref(s, mode, **kw)
        assert not np.array_equal(want["row"], base["row"]), kw              # the parameter matters on these rays
        cf.assert_same(host(s["m"].cast_rays(s["sensor"], dev(s["ends"]), mode=MODE_NAMES[mode], **kw)), want, kw)


@pytest.mark.parametrize("mode", [VOXEL, NDT])
def test_lanes_that_leave_the_walk_at_different_steps(mode):
    s = scene("atomic")
    m, cells, P = s["m"], s["cells"], s["P"]
    good = s["ends"][np.isfinite(s["ends"]).all(1)]
    # a wave of 64 identical rays, between two waves of different ones
    ends = np.concatenate([good[:64], np.tile(good[5], (64, 1)), good[64:128]])
    want = cf.cast(cells, s["origin"], P["grid_len"], P["z_len"], s["sensor"], ends, mode=mode)
    cf.assert_same(host(m.cast_rays(s["sensor"], dev(ends), mode=MODE_NAMES[mode])), want, "identical")
    assert len(set(want["row"][64:128].tolist())) == 1
    # zero-length rays inside occupied voxels alternating with rays across the whole map
    lo, hi = s["pts"].min(0), s["pts"].max(0)
    far = np.array([hi[0], hi[1], lo[2]], np.float32)
    origins = np.empty((128, 3), np.float32)
    ends = np.empty((128, 3), np.float32)
    origins[0::2] = ends[0::2] = s["pts"][:64]
    origins[1::2] = np.array([lo[0], lo[1], hi[2] + 2.0], np.float32)
    ends[1::2] = far[None, :] + np.linspace(0, 1, 64, dtype=np.float32)[:, None] * np.array([0, -5.0, 0], np.float32)
    want = cf.cast(cells, s["origin"], P["grid_len"], P["z_len"], origins, ends, mode=mode)
    steps = np.bincount(want["steps"]["ray"], minlength=128)
    assert (steps[0::2] == 1).all() and (steps[1::2] > 100).all()
    if mode == VOXEL:                                                         # (a scan point's voxel holds a node: range 0)
        assert (want["row"][0::2] != cf.NO_ROW).all() and (want["range"][0::2] == 0).all()
    cf.assert_same(host(m.cast_rays(dev(origins), dev(ends), mode=MODE_NAMES[mode])), want, "alternating")


@pytest.mark.parametrize("name", ["atomic", "partition", "tile"])
def test_voxel_hits_against_the_clearing_walk_and_the_node_query(name):
    """independent of cast_ref: the scan's own end points, shared origin, min_count = 1"""
    import torch
    s = scene(name)
    m = s["m"]
    pts = dev(s["pts"][:4096])
    out = m.cast_rays(s["sensor"], pts, mode="voxel", min_count=1)
    row, rng = out["row"].cpu().numpy().astype(np.int64), out["range"].cpu().numpy()
    _, words = m.clear_rays(s["sensor"], pts, count_only=True, passes=True)
    words = words.cpu().numpy().view(np.uint32) & np.uint32(0x7FFFFFFF)
    hit = row >= 0
    assert hit.sum() > 1000 and (words[row[hit]] > 0).all()
    seen = m.query(pts).cpu().numpy() >= 0
    assert seen.sum() > 1000 and hit[seen].all()
    L = np.sqrt(((s["pts"][:4096].astype(np.float64) - s["sensor"].astype(np.float64)) ** 2).sum(1)).astype(np.float32)
    assert (rng[seen] <= np.nextafter(L[seen], np.float32(np.inf))).all()
    torch.cuda.synchronize()


def test_the_map_is_untouched_and_the_bits_repeat():
    import torch
    s = scene("atomic")
    m = s["m"]
    e = dev(s["ends"])
    o = dev(s["origins"])
    for mode in ("voxel", "ndt"):
        a = host(m.cast_rays(o, e, mode=mode))
        b = host(m.cast_rays(o, e, mode=mode))
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        c = m.cast_rays(o, e, mode=mode, stream=st)
        d = m.cast_rays(s["origins"], e, mode=mode, stream=st.cuda_stream)       # a raw hipStream_t, host origins uploaded on it
        st.synchronize()
        c, d = host(c), host(d)
        torch.cuda.current_stream().wait_stream(st)
        for other in (b, c, d):
            for k in ("row", "range", "d2"):
                assert np.array_equal(a[k].view(np.uint32), other[k].view(np.uint32)), (mode, k)
    after = m.export()
    for k in ("num_nodes", "num_columns", "num_slopes"):
        assert after[k] == s["cells"][k]
    for k in FIELDS:
        x, y = np.ascontiguousarray(after[k]), np.ascontiguousarray(s["cells"][k])
        assert x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32)), k


def test_cast_scan_is_cast_rays_of_the_documented_ends():
    s = scene("atomic")
    m = s["m"]
    a = np.deg2rad(25.0)
    T = np.array([[np.cos(a), -np.sin(a), 0, s["sensor"][0]], [np.sin(a), np.cos(a), 0, s["sensor"][1]], [0, 0, 1, s["sensor"][2]]], np.float64)
    rng = np.random.default_rng(9)
    d = rng.normal(size=(1500, 3))
    d[:, 2] = -np.abs(d[:, 2]) - 0.2                                         # towards the ground
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    R = 12.0
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    ends = np.stack([T[i, 3] + R * ((T[i, 0] * x + T[i, 1] * y) + T[i, 2] * z) for i in range(3)], 1).astype(np.float32)
    for mode in ("voxel", "ndt"):
        got = host(m.cast_scan(T, d, R, mode=mode))
        want = host(m.cast_rays(T[:, 3].astype(np.float32), dev(ends), mode=mode))
        assert (want["row"] >= 0).sum() > 500
        for k in ("row", "range", "d2"):
            assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), (mode, k)
        assert (got["range"][got["row"] >= 0] <= np.float32(R) * (1 + 1e-6)).all()


def _raw(m, o, so, e, n, se, prm, out, stats=None, device=True):
    p = lambda t: C.c_void_p(0 if t is None else (t.data_ptr() if hasattr(t, "data_ptr") else t.ctypes.data))
    args = [m._h, p(o), so, p(e), n, se, C.byref(prm) if prm is not None else None, C.byref(out) if out is not None else None,
            C.byref(stats) if stats is not None else None]
    # (torch's current stream: the outputs are filled and read on it)
    return m._L.gndt_cast_rays_device(*args, _stream_ptr(None)) if device else m._L.gndt_cast_rays(*args)


def test_invalid_arguments_leave_the_outputs_untouched():
    import torch
    import grid_ndt_amd as g
    from grid_ndt_amd._lib import CastOut, CastParams, CastStats
    s = scene("atomic")
    m = s["m"]
    n = 256
    ends = np.ascontiguousarray(s["ends"][:n])
    ok = lambda **kw: CastParams(**{**dict(mode=0, min_count=0, max_range=0, min_range=0, cov_rel=0, cov_floor=0, max_d2=0, reserved=0), **kw})
    nan, inf = float("nan"), float("inf")
    bad_params = [ok(mode=2), ok(mode=-1), ok(reserved=1), ok(min_count=-1), ok(mode=1, min_count=1), ok(mode=1, min_count=2)]
    bad_params += [ok(**{k: v}) for k in ("max_range", "min_range", "cov_rel", "cov_floor", "max_d2") for v in (-1.0, nan, inf)]
    for device in (True, False):
        mk = (lambda a, dt=np.float32: dev(a, dt)) if device else (lambda a, dt=np.float32: np.ascontiguousarray(a, dt))
        o, e = mk(s["sensor"]), mk(ends)
        outs = [mk(np.full(n, -7, np.int32), np.int32), mk(np.full(n, -7.0, np.float32)), mk(np.full(n, -7.0, np.float32))]
        ptr = lambda t: t.data_ptr() if device else t.ctypes.data
        out = CastOut(*[ptr(t) for t in outs])
        assert _raw(m, o, 0, e, n, 12, ok(), out, device=device) == 0               # the arguments the bad ones differ from are good
        for t in outs:
            t[:] = -7
        calls = [(o, 0, e, n, 12, p, out) for p in bad_params]
        calls += [(o, 0, e, n, 12, None, out), (o, 0, e, n, 12, ok(), None), (o, 0, e, n, 12, ok(), CastOut(None, None, None)),
                  (None, 0, e, n, 12, ok(), out), (o, 0, None, n, 12, ok(), out), (o, 0, e, 1 << 31, 12, ok(), out),
                  (o, 4, e, n, 12, ok(), out), (o, 8, e, n, 12, ok(), out), (o, 0, e, n, 0, ok(), out), (o, 0, e, n, 8, ok(), out),
                  (o, 0, e, n, 20, ok(), out)]
        for c in calls:
            st = CastStats(5, 5, 5)
            assert _raw(m, *c, stats=st, device=device) == 1, c
        if device:
            torch.cuda.synchronize()
        for t in outs:
            assert bool((t == -7).all())
    assert m._L.gndt_cast_rays_device(None, None, 0, None, 0, 12, None, None, None, None) == 1
    assert m._L.gndt_cast_rays(None, None, 0, None, 0, 12, None, None, None) == 1
    # NDT's min_count below the handle's min_points; a handle without a finished build
    P = s["P"]
    h5 = g.TwoDmap(P["grid_len"], P["z_len"], strategy=ATOMIC, min_points=5)
    h5.setInterval(P["slope_interval"])
    small = scenes.terrain_cloud(20_000)
    h5.setCloudFirst(small[0])
    with pytest.raises(g.GndtError) as err:
        h5.cast_rays(s["sensor"], dev(ends))
    assert err.value.code == 1                                                    # no finished build
    h5.create2DMap("slope", dev(small[1:]))
    for mc in (3, 4):
        with pytest.raises(g.GndtError) as err:
            h5.cast_rays(s["sensor"], dev(ends), mode="ndt", min_count=mc)
        assert err.value.code == 1
    h5.cast_rays(s["sensor"], dev(ends), mode="ndt", min_count=5)
    h5.cast_rays(s["sensor"], dev(ends), mode="voxel", min_count=1)
    with pytest.raises(ValueError):
        m.cast_rays(s["origins"][:5], dev(ends))


def test_capture_is_refused_and_the_empty_batch():
    import torch
    import grid_ndt_amd as g
    from grid_ndt_amd._lib import CastOut, CastParams, CastStats
    s = scene("atomic")
    m = s["m"]
    # n == 0: GNDT_OK, stats zeroed, nothing written
    outs = [dev(np.full(4, -7, np.int32), np.int32), dev(np.full(4, -7.0)), dev(np.full(4, -7.0))]
    st = CastStats(5, 5, 5)
    for device in (True, False):
        st = CastStats(5, 5, 5)
        assert _raw(m, None, 0, None, 0, 12, CastParams(), CastOut(*[t.data_ptr() for t in outs]), stats=st, device=device) == 0
        assert (st.rays, st.skipped, st.hits) == (0, 0, 0)
    torch.cuda.synchronize()
    assert all(bool((t == -7).all()) for t in outs)
    out, st = m.cast_rays(s["sensor"], dev(np.zeros((0, 3), np.float32)), stats=True)
    assert st == {"rays": 0, "skipped": 0, "hits": 0} and all(len(out[k]) == 0 for k in ("row", "range", "d2"))
    out = m.cast_rays(s["sensor"], np.zeros((0, 4), np.float32), mode="ndt")
    assert all(len(out[k]) == 0 for k in ("row", "range", "d2"))
    # a stream under capture
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        o, e = dev(s["sensor"]), dev(s["ends"][:256])
        stream.wait_stream(torch.cuda.default_stream())
        graph = torch.cuda.CUDAGraph()
        with pytest.raises(g.GndtError) as err:
            with g.graph_capture(graph, stream):
                m.cast_rays(o, e, stream=stream)
        assert err.value.code == 1
        del graph
        stream.synchronize()
        want = ref(s, VOXEL)
        cf.assert_same(host(m.cast_rays(o, e, stream=stream)), sliced(want, 256), "after the refused capture")
        stream.synchronize()
