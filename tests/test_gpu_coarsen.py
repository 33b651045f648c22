"""GPU tier: map pyramids (gndt_coarsen_device, TwoDmap.coarsen / pyramid / register(pyramid=...)).  The coarsened map against the
oracle's build of the same cloud at the multiplied lengths (tests/parity.py), for fine maps built by strategy ATOMIC, by TILE and from
three update frames; the smallest shapes that can go wrong; after remove, crop and clear, where the points are gone, against the numpy
restatement (tests/coarsen_ref.py) applied to the source's own statistics; continuation by updates; the source is untouched; a
destination that held a map is replaced; every refusal; coarse-to-fine registration on the device.

Tolerances: parity's own against the oracle; against the restatement keys, counts and first-seen indices exact and the nine sums
within coarsen_ref's derived bound; the registration's condition is the CPU tier's (tests/test_coarsen_host.py): at most twice the
error of the fine-only run from the documented start B."""
import ctypes as C

import numpy as np
import pytest

from grid_ndt_amd import scenes
from tests import coarsen_ref as cr
from tests import parity
from tests import query_ref as qr
from tests import raster_ref as rr
from tests import score_derivs_ref as dr
from tests import score_ref as sr
from tests.gpu_kit import dev, handle, to_np
from tests.test_gpu_score import ATOMIC, BOX, ERR_INVALID, PARTITION, TILE, six_poses, yaw

pytestmark = pytest.mark.gpu

FACTORS = [(2, 2), (4, 2), (2, 1), (1, 2), (8, 8), (1, 1)]
SCENES = {
    "campus_frame": lambda: (scenes.campus_frame(20_000), scenes.CAMPUS_PARAMS),
    "uniform_box": lambda: (scenes.uniform_box(40_001, half_xy=6.0, half_z=1.0), BOX),
}
_clouds, _refs = {}, {}


def _scene(name):
    if name not in _clouds:
        _clouds[name] = SCENES[name]()
    return _clouds[name]


def _coarse_params(P, fxy, fz):
    return dict(P, grid_len=float(cr.coarse_len(P["grid_len"], fxy)), z_len=float(cr.coarse_len(P["z_len"], fz)))


def _oracle(name, fxy, fz):
    """the oracle's map of a scene at the multiplied lengths, made once and shared"""
    if (name, fxy, fz) not in _refs:
        cloud, P = _scene(name)
        _refs[(name, fxy, fz)] = parity.ref_from_cloud(cloud, _coarse_params(P, fxy, fz))
    return _refs[(name, fxy, fz)]


def _fine(cloud, P, how=ATOMIC):
    m = handle(P, TILE if how == TILE else ATOMIC)
    m.setCloudFirst(cloud[0])
    body = cloud[1:]
    if how == "frames":
        a, b = len(body) // 3, 2 * len(body) // 3
        for part in (body[:a], body[a:b], body[b:]):
            m.change2DMap("slope", dev(part))
    else:
        m.create2DMap("slope", dev(body))
    return m


def _same_bits(a, b, keys=None):
    for k in (keys or a.keys()):
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape, k
        assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y), k


def _stats(m):
    """the handle's node statistics as numpy copies (the views are the handle's buffers)"""
    st = m.stats_export()
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().copy() for k, v in st.items()}


# ---- 1. parity with the oracle at the multiplied lengths ----

@pytest.mark.parametrize("how", [ATOMIC, TILE, "frames"])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_coarsened_map_is_the_oracles_map_at_the_multiplied_lengths(name, how):
    cloud, P = _scene(name)
    m = _fine(cloud, P, how)
    src = m.export()
    for fxy, fz in FACTORS:
        c = m.coarsen(fxy, fz)
        assert np.float32(c.gridLen) == cr.coarse_len(P["grid_len"], fxy) and np.float32(c.zLen) == cr.coarse_len(P["z_len"], fz)
        out = c.export()
        rep = parity.assert_parity(out, _oracle(name, fxy, fz))
        print(name, how, (fxy, fz), {k: rep[k] for k in ("num_nodes", "cov_err_truth", "mean_err")})
        if (fxy, fz) == (1, 1):
            _same_bits(out, src, ("sx", "sy", "sz", "count", "first_idx", "flags"))
        else:
            assert out["num_nodes"] < src["num_nodes"]
    _same_bits(m.export(), src)


# ---- 2. the smallest shapes that can go wrong ----

def _cells_cloud(cells, per=3, P=BOX, seed=3, origin=(0.125, -0.25, 0.0625)):
    """a cloud (point 0 = the origin) with `per` points inside each of the cells (sx, sy, sz), shuffled"""
    rng = np.random.default_rng(seed)
    o = np.float32(origin)
    cells = np.asarray(cells, np.float64)
    lens = np.array([P["grid_len"], P["grid_len"], P["z_len"]])
    centre = (np.abs(cells) - 0.5) * np.sign(cells) * lens
    pts = np.repeat(centre, per, 0) + rng.uniform(-0.4, 0.4, size=(len(cells) * per, 3)) * lens
    rng.shuffle(pts)
    return np.ascontiguousarray(np.concatenate([o[None], (o + pts).astype(np.float32)]), np.float32)


def _check_cells(cells, factors, per=3, parents=None):
    cloud = _cells_cloud(cells, per)
    m = _fine(cloud, BOX)
    fine = m.export()
    assert fine["num_nodes"] == len(cells)
    c = m.coarsen(*factors)
    out = c.export()
    parity.assert_parity(out, parity.ref_from_cloud(cloud, _coarse_params(BOX, *factors)))
    if parents is not None:
        assert sorted(zip(out["sx"].tolist(), out["sy"].tolist(), out["sz"].tolist())) == sorted(parents)
    return fine, out


def test_smallest_shapes():
    # one node
    _check_cells([(3, -2, 1)], (2, 2), parents=[(2, -1, 1)])
    # one column holding only levels -1 and +1: the parents stay -1 and +1
    _check_cells([(3, 3, -1), (3, 3, 1)], (2, 2), parents=[(2, 2, -1), (2, 2, 1)])
    _check_cells([(3, 3, -1), (3, 3, 1)], (1, 8), parents=[(3, 3, -1), (3, 3, 1)])
    # columns at sx = +-1 and sy = +-1
    _check_cells([(1, 1, 1), (-1, 1, 1), (1, -1, 1), (-1, -1, 1)], (4, 2), parents=[(1, 1, 1), (-1, 1, 1), (1, -1, 1), (-1, -1, 1)])
    # three points in three fine cells of one coarse cell: no fine node has statistics, the parent has
    fine, out = _check_cells([(1, 1, 1), (2, 1, 1), (1, 2, 2)], (2, 2), per=1, parents=[(1, 1, 1)])
    assert not (fine["flags"] & 1).any() and out["count"].tolist() == [3] and (out["flags"] & 1).all()
    # 64 fine nodes (one wave) in one parent; 65 and 257 nodes cross the wave's and the workgroup's edge
    wave = [(x, y, 1) for x in range(1, 9) for y in range(1, 9)]
    _, out = _check_cells(wave, (8, 8), parents=[(1, 1, 1)])
    assert out["count"].tolist() == [192]
    _check_cells(wave + [(9, 1, 1)], (8, 8), parents=[(1, 1, 1), (2, 1, 1)])
    block = [(x, y, 1) for x in range(1, 17) for y in range(1, 17)]
    _check_cells(block + [(17, 1, 1)], (8, 8), parents=[(1, 1, 1), (2, 1, 1), (1, 2, 1), (2, 2, 1), (3, 1, 1)])
    _check_cells(block + [(-1, 1, -1)], (2, 2))


def test_a_source_emptied_by_a_crop_gives_an_empty_destination():
    cloud, P = _scene("uniform_box")
    m = _fine(cloud, P)
    m.crop_box((30000, 30010, 30000, 30010), "keep_inside")
    assert m.sync()[0] == 0
    c = m.coarsen(2)
    assert c.sync() == (0, 0, 0) and c.export()["num_nodes"] == 0
    # ... and it goes on from there: a frame given to both is the coarse build of that frame at the stream's indices
    for x in (m, c):
        x.change2DMap("slope", dev(cloud[1:2001]))
    assert c.export()["num_nodes"] > 0 and np.array_equal(np.sort(_stats(c)["count"]), np.sort(_stats(m.coarsen(2))["count"]))


# ---- 3. maps whose points are gone: against the restatement on the source's own statistics ----

def _check_against_restatement(m, P, origin, fxy, fz):
    src = _stats(m)
    c = m.coarsen(fxy, fz)
    got = _stats(c)
    want = cr.coarsen(src["key"], src["count"], src["first_idx"], src["sums"], fxy, fz, origin, P["grid_len"], P["z_len"])
    order = np.argsort(got["key"].astype(np.uint64))
    assert np.array_equal(got["key"].astype(np.uint64)[order], want["key"])
    assert np.array_equal(got["count"].astype(np.int64)[order], want["count"].astype(np.int64))
    assert np.array_equal(got["first_idx"].astype(np.int64)[order] & 0xFFFFFFFF, want["first_idx"].astype(np.int64))
    err = np.abs(got["sums"][order] - want["sums"])
    print((fxy, fz), "parents", len(order), "worst error / bound", float((err / np.maximum(want["tol"], 1e-300)).max()))
    assert (err <= want["tol"]).all()
    # the rows are what the destination's own finalisation makes of these statistics: as many nodes, the same counts
    out = c.export()
    assert out["num_nodes"] == len(order) and np.array_equal(np.sort(out["count"].astype(np.int64)), np.sort(want["count"].astype(np.int64)))
    return c


def test_after_remove_crop_and_clear():
    cloud, P = _scene("uniform_box")
    origin, body = cloud[0], cloud[1:]
    m = _fine(cloud, P)
    n0 = m.sync()[0]
    m.del2DMap("slope", dev(body[5000:16000]))
    _check_against_restatement(m, P, origin, 2, 2)
    m.crop((-4.2, -3.1), (3.3, 5.0))
    n1 = m.sync()[0]
    assert 0 < n1 < n0
    _check_against_restatement(m, P, origin, 4, 2)
    sensor = origin + np.float32([0.2, 0.1, 0.05])
    st = m.clear_rays(sensor, dev(body[::50]))
    assert st["cleared"] > 0 and 0 < m.sync()[0] < n1
    _check_against_restatement(m, P, origin, 2, 1)
    _check_against_restatement(m, P, origin, 8, 8)


# ---- 4. continuation ----

def test_coarse_map_follows_the_stream():
    cloud, P = _scene("campus_frame")
    body = cloud[1:]
    a, b = len(body) // 3, 2 * len(body) // 3
    m = handle(P, ATOMIC)
    m.setCloudFirst(cloud[0])
    m.change2DMap("slope", dev(body[:a]))
    m.change2DMap("slope", dev(body[a:b]))
    c = m.coarsen(2, 2)
    assert c.cloudFirst == m.cloudFirst
    for x in (m, c):
        x.change2DMap("slope", dev(body[b:]))
    parity.assert_parity(c.export(), _oracle("campus_frame", 2, 2))
    parity.assert_parity(m.export(), parity.ref_from_cloud(cloud, P))


# ---- 5. the source is untouched ----

def test_the_source_is_untouched():
    cloud, P = scenes.drivable_site(60_000), scenes.COST_PARAMS
    m = _fine(cloud, P)
    before = m.export()
    counts = m.sync()
    slopes = np.flatnonzero(before["flags"] & 2)
    goal = tuple(float(v) for v in before["mean"][slopes[len(slopes) // 2]])
    m.computeCost(goal, robot={"radius": 0.25})
    cost = m.cost_export()
    pts = dev(cloud[1:][::7])
    rows = m.query(pts).cpu().numpy()
    c = m.coarsen(2)
    c2 = m.coarsen(4, 2, into=None)
    assert c.sync()[0] > c2.sync()[0] > 0
    after = m.export()
    assert m.sync() == counts
    _same_bits(after, before)
    again = m.cost_export()                                          # the cost map computed before the call still exports
    assert np.array_equal(again["h"].view(np.uint32), cost["h"].view(np.uint32)) and np.array_equal(again["state"], cost["state"])
    assert np.array_equal(m.query(pts).cpu().numpy(), rows)          # row numbers still name the same rows
    assert np.array_equal(rows.astype(np.int64), qr.node_rows(after, cloud[1:][::7], cloud[0], P["grid_len"], P["z_len"]))


# ---- 6. a destination that held a map is replaced ----

def test_a_destination_that_held_a_map_is_replaced():
    cloud, P = _scene("uniform_box")
    Pc = _coarse_params(P, 2, 2)
    other = scenes.terrain_cloud(30_000)
    dst = handle(Pc, ATOMIC)
    dst.setCloudFirst(other[0])
    dst.create2DMap("slope", dev(other[1:]))
    held = dst.export()
    goal = tuple(float(v) for v in held["mean"][np.flatnonzero(held["flags"] & 2)[0]])
    dst.computeCost(goal, robot={"radius": 0.25})
    m = _fine(cloud, P)
    assert m.coarsen(2, into=dst) is dst and dst.cloudFirst == m.cloudFirst
    cells = dst.export()
    parity.assert_parity(cells, _oracle("uniform_box", 2, 2))
    import grid_ndt_amd as g
    with pytest.raises(g.GndtError):
        dst.cost_export()                                            # the old map's cost map is gone with it
    pts = np.ascontiguousarray(cloud[1:][::9])
    got = dst.query(dev(pts)).cpu().numpy().astype(np.int64)
    want = qr.node_rows(cells, pts, cloud[0], Pc["grid_len"], Pc["z_len"])
    assert np.array_equal(got, want) and (want >= 0).all()
    box = (int(cells["sx"].min()), int(cells["sx"].max()), int(cells["sy"].min()), int(cells["sy"].max()))
    for mode in ("lowest", "highest"):
        r = dst.raster(box, mode, layers=("row", "z", "rough", "nodes"))
        w = rr.raster(cells, box, mode, 0.0)
        for k in ("row", "z", "rough", "nodes"):
            assert rr.same(to_np({"x": r[k]})["x"], w[k]), (mode, k)
    poses = six_poses(Pc)
    for nbh in (1, 7):
        sc = to_np(dst.score_poses(dev(pts), poses, neighbourhood=nbh))
        ws = sr.score(cells, cloud[0], Pc["grid_len"], Pc["z_len"], pts, poses, nbh)
        assert ws["terms"][0] > 100
        sr.assert_pose_sums(sc, ws, what=("coarsened", nbh))


# ---- 7. refusals ----

def test_refusals_leave_the_destination_as_it_was():
    import torch
    import grid_ndt_amd as g
    cloud, P = _scene("uniform_box")
    Pc = _coarse_params(P, 2, 2)
    m = _fine(cloud, P)
    dst = handle(Pc, ATOMIC)
    dst.setCloudFirst(cloud[0])
    dst.create2DMap("slope", dev(cloud[1:20001]))
    before = dst.export()
    L = m._L
    null = C.c_void_p(0)

    def refused(rc):
        assert rc == ERR_INVALID
        _same_bits(dst.export(), before)

    refused(L.gndt_coarsen_device(None, dst._h, 2, 2, null))                       # a null handle
    assert L.gndt_coarsen_device(m._h, None, 2, 2, null) == ERR_INVALID
    assert L.gndt_coarsen_device(None, None, 2, 2, null) == ERR_INVALID
    assert L.gndt_coarsen_device(dst._h, dst._h, 1, 1, null) == ERR_INVALID          # src == dst
    _same_bits(dst.export(), before)
    for f in ((0, 2), (2, 0), (3, 2), (2, 3), (6, 6), (2048, 2), (2, 2048), (0xFFFFFFFF, 2)):
        refused(L.gndt_coarsen_device(m._h, dst._h, f[0], f[1], null))              # not a power of two in 1 .. 1024
    for f in ((1, 1), (2, 1), (1, 2), (4, 2), (4, 4), (2, 4)):
        refused(L.gndt_coarsen_device(m._h, dst._h, f[0], f[1], null))              # lengths that are not factor x the source's
    with pytest.raises(g.GndtError) as e:
        m.coarsen(4, 2, into=dst)
    assert e.value.code == ERR_INVALID and "grid_len" in str(e.value)
    empty = handle(P, ATOMIC)                                                       # no finished build
    empty.setCloudFirst(cloud[0])
    empty.reset("slope")
    refused(L.gndt_coarsen_device(empty._h, dst._h, 2, 2, null))
    with pytest.raises(g.GndtError) as e:
        handle(P, ATOMIC).coarsen(2)
    assert e.value.code == ERR_INVALID
    part = handle(P, PARTITION)                                                     # a map that is not in the node table
    part.setCloudFirst(cloud[0])
    part.create2DMap("slope", dev(cloud[1:]))
    refused(L.gndt_coarsen_device(part._h, dst._h, 2, 2, null))
    assert "node table" in L.gndt_last_error(dst._h).decode()
    if torch.cuda.device_count() > 1:                                                # handles on different devices
        far = g.TwoDmap(Pc["grid_len"], Pc["z_len"], device=1, strategy=ATOMIC)
        far.setCloudFirst(cloud[0])
        far.reset("slope")
        assert L.gndt_coarsen_device(m._h, far._h, 2, 2, null) == ERR_INVALID
        torch.cuda.set_device(0)
    # a capturing stream: refused, and the capture goes on
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    x = torch.zeros(16, device="cuda")
    torch.cuda.synchronize()
    with g.graph_capture(graph, stream=s):
        rc = L.gndt_coarsen_device(m._h, dst._h, 2, 2, C.c_void_p(s.cuda_stream))
        x.add_(1.0)
    graph.replay()
    torch.cuda.synchronize()
    assert float(x[0]) == 1.0
    refused(rc)
    # and the same call outside the capture works
    assert L.gndt_coarsen_device(m._h, dst._h, 2, 2, null) == 0
    parity.assert_parity(dst.export(), _oracle("uniform_box", 2, 2))


# ---- 8. coarse to fine on the device ----

def test_register_with_a_pyramid_recovers_a_start_beyond_the_fine_basin():
    """drivable_site(100 000), COST_PARAMS, every fifth point, neighbourhood 7, start C = yaw 5 degrees, (2.0, 1.5) cells, -0.5 level
    (1.256 m, 87 mrad off): the fine map alone returns the start; with m.pyramid(2) the error is at most twice that of the device's
    fine-only run from start B (the CPU tier's condition and reference; both measured 0.9 mm / 0.029 mrad on the host)."""
    from tests.test_score_derivs_host import starts
    cloud, P = scenes.drivable_site(100_000), scenes.COST_PARAMS
    m = _fine(cloud, P)
    t = dev(cloud[1:][::5])
    g_, z_ = P["grid_len"], P["z_len"]
    C_start = yaw(5.0, (2.0 * g_, 1.5 * g_, -0.5 * z_))
    fine = m.register(t, C_start)
    assert np.array_equal(fine["T"], C_start[:3]) and "levels" not in fine
    ref = m.register(t, starts(P)["B"])
    tB, aB = dr.pose_error(ref["T"])
    pyr = m.pyramid(2)
    assert [p.gridLen for p in pyr] == [4 * g_, 2 * g_] and [p.zLen for p in pyr] == [4 * z_, 2 * z_]
    res = m.register(t, C_start, pyramid=pyr)
    tp, ap = dr.pose_error(res["T"])
    print("device, fine only from B: %.2f mm %.4f mrad (%s, %d); pyramid from C: %.2f mm %.4f mrad;" %
          (1e3 * tB, 1e3 * aB, ref["reason"], ref["iterations"], 1e3 * tp, 1e3 * ap),
          "levels:", [("%.2f mm" % (1e3 * dr.pose_error(r["T"])[0]), r["reason"], r["iterations"]) for r in res["levels"]])
    assert len(res["levels"]) == 3 and np.array_equal(res["levels"][-1]["T"], res["T"])
    assert tp <= 2.0 * tB and ap <= 2.0 * aB, (tp, ap, tB, aB)
