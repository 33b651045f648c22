"""GPU tier: map merge (gndt_merge_map_device, TwoDmap.merge_from / stitch).  Into an empty destination the merged map against the
oracle's build of the (moved) cloud (tests/parity.py), for sources built by strategy ATOMIC, by TILE and from three update frames; into a
populated destination against the oracle's map of the whole stream, and on from there by updates; under a general pose against the
numpy restatement (tests/merge_ref.py) applied to the two handles' own statistics; the smallest shapes that can go wrong; a destination
table that has to grow; the source is untouched; every refusal; stitch; a graph recorded before a merge is reported stale.

Tolerances: parity's own against the oracle; against the restatement keys, counts and first-seen indices exact and the nine sums within
merge_ref's derived bound (the order of the adds, plus the per-addend rounding of the steps); stitch's pose is register's to the bit."""
import ctypes as C

import numpy as np
import pytest

from grid_ndt_amd import scenes
from tests import merge_ref as mr
from tests import parity
from tests import query_ref as qr
from tests.test_gpu_coarsen import _cells_cloud, _coarse_params, _fine, _same_bits, _scene, _stats
from tests.gpu_kit import dev, handle
from tests.test_gpu_score import ATOMIC, BOX, ERR_INVALID, PARTITION, TILE
from tests.test_merge_host import lattice_pose, moved_cloud, rigid

pytestmark = pytest.mark.gpu

EXACT = ("sx", "sy", "sz", "count", "first_idx", "flags")
_refs = {}


def _oracle(tag, cloud, P):
    """the oracle's map of a cloud, made once and shared"""
    if tag not in _refs:
        _refs[tag] = parity.ref_from_cloud(cloud, P)
    return _refs[tag]


def _empty(P, origin):
    d = handle(P, ATOMIC)
    d.setCloudFirst(origin)
    return d


def _keys(cells):
    return sorted(zip(cells["sx"].tolist(), cells["sy"].tolist(), cells["sz"].tolist()))


# ---- 1. into an empty destination: parity with the oracle ----

@pytest.mark.parametrize("how", [ATOMIC, TILE, "frames"])
@pytest.mark.parametrize("name", ["campus_frame", "uniform_box"])
def test_merge_into_an_empty_map_is_the_oracles_map(name, how):
    cloud, P = _scene(name)
    src = _fine(cloud, P, how)
    before = src.export()
    n_pts = len(cloud) - 1
    # the identity at equal geometry: the source's map again
    d = _empty(P, cloud[0])
    st = d.merge_from(src)
    out = d.export()
    rep = parity.assert_parity(out, _oracle((name, 1), cloud, P))
    _same_bits(out, src.coarsen(1, 1).export(), EXACT)
    assert st == {"source_nodes": before["num_nodes"], "merged_nodes": before["num_nodes"], "merged_points": n_pts, "below_min_count": 0,
                  "skipped": 0, "new_nodes": before["num_nodes"]}
    print(name, how, "identity", {k: rep[k] for k in ("num_nodes", "cov_err_truth", "mean_err")})
    # the identity at twice the lengths: the coarsened map
    d2 = _empty(_coarse_params(P, 2, 2), cloud[0])
    st2 = d2.merge_from(src)
    _same_bits(d2.export(), src.coarsen(2, 2).export(), EXACT)
    assert st2["merged_points"] == n_pts and st2["new_nodes"] == d2.sync()[0] < before["num_nodes"]
    _same_bits(src.export(), before)


# The lattice pose moves cells to cells, so the merged map is the oracle's map of the moved cloud T p.  The oracle takes float32 points:
# on the scenes above fl32(T p) differs from T p by half an ulp of a coordinate, which is 1e-5 of a node's extent and more, beyond
# parity's covariance gates (measured: 2.9e-5 against the gate of 2e-6) although the merge never rounds a point.  So this case runs on
# clouds whose moved points ARE float32 numbers: coordinates on odd multiples of 2^-11 m about an origin on the 2^-10 m grid, at cell
# lengths that are powers of two (no point sits on a cell face before or after the move).  tests/test_merge_host.py checks the
# rounded clouds of the scenes above on the host, with the rounding's own bound.
LATTICE_SCENES = {
    "uniform_box": lambda: (scenes.uniform_box(40_001, half_xy=6.0, half_z=1.0), BOX),
    "drivable_site": lambda: (scenes.drivable_site(60_000), scenes.COST_PARAMS),
}
_lattice = {}


def _dyadic(cloud):
    c = cloud.astype(np.float64)
    c[1:, :3] = (np.floor(c[1:, :3] * 1024.0) + 0.5) / 1024.0
    c[0, :3] = np.round(c[0, :3] * 1024.0) / 1024.0
    out = c.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), c)
    return out


def _lattice_scene(name):
    if name not in _lattice:
        cloud, P = LATTICE_SCENES[name]()
        cloud = _dyadic(cloud)
        pose = lattice_pose(cloud[0, :3], P["grid_len"], P["z_len"])
        exact = cloud[1:, :3].astype(np.float64) @ pose[:, :3].T + pose[:, 3]
        q = moved_cloud(cloud, pose)
        assert np.array_equal(q[1:, :3].astype(np.float64), exact)         # the moved points are float32 numbers
        _lattice[name] = (cloud, P, pose, q)
    return _lattice[name]


@pytest.mark.parametrize("how", [ATOMIC, TILE, "frames"])
@pytest.mark.parametrize("name", sorted(LATTICE_SCENES))
def test_merge_under_the_lattice_pose_is_the_oracles_map_of_the_moved_cloud(name, how):
    cloud, P, pose, q = _lattice_scene(name)
    src = _fine(cloud, P, how)
    n = src.sync()[0]
    d = _empty(P, cloud[0])
    st = d.merge_from(src, pose=pose)
    rep = parity.assert_parity(d.export(), _oracle((name, "moved"), q, P))
    assert st == {"source_nodes": n, "merged_nodes": n, "merged_points": len(cloud) - 1, "below_min_count": 0, "skipped": 0, "new_nodes": n}
    print(name, how, "lattice", {k: rep[k] for k in ("num_nodes", "cov_err_truth", "mean_err")})


# ---- 2. into a populated destination, and on from there ----

def test_merge_into_a_populated_map_continues_the_stream():
    cloud, P = _scene("campus_frame")
    body = cloud[1:]
    a, b = len(body) // 3, 2 * len(body) // 3
    dst = _empty(P, cloud[0])
    dst.create2DMap("slope", dev(body[:a]))
    src = _empty(P, cloud[0])
    src.create2DMap("slope", dev(body[a:b]))
    n0 = dst.sync()[0]
    st = dst.merge_from(src)
    assert st["merged_points"] == b - a and st["new_nodes"] == dst.sync()[0] - n0
    parity.assert_parity(dst.export(), _oracle(("campus", b), cloud[:1 + b], P))
    dst.change2DMap("slope", dev(body[b:]))
    parity.assert_parity(dst.export(), _oracle(("campus_frame", 1), cloud, P))


# ---- 3. a general pose: against the restatement on the handles' own statistics ----

def _sorted_stats(st):
    order = np.argsort(st["key"].astype(np.uint64))
    return {"key": st["key"].astype(np.uint64)[order], "count": st["count"].astype(np.int64)[order] & 0xFFFFFFFF,
            "first_idx": st["first_idx"].astype(np.int64)[order] & 0xFFFFFFFF, "sums": st["sums"][order]}


def _check_against_restatement(dst, src, pose, src_geo, dst_geo, base, min_count=0):
    prior, s = _stats(dst), _stats(src)
    st = dst.merge_from(src, pose=pose, min_count=min_count)
    got = _sorted_stats(_stats(dst))
    want = mr.merge(s, pose, src_geo, dst_geo, prior=prior, min_count=min_count, base=base)
    assert st == want["stats"], (st, want["stats"])
    assert np.array_equal(got["key"], want["key"])
    assert np.array_equal(got["count"], want["count"].astype(np.int64))
    assert np.array_equal(got["first_idx"], want["first_idx"].astype(np.int64))
    err = np.abs(got["sums"] - want["sums"])
    print("nodes", len(got["key"]), "most addends", int(want["addends"].max()), "worst error / bound",
          float((err / np.maximum(want["tol"], 1e-300)).max()))
    assert (err <= want["tol"]).all()
    assert int(got["count"].sum()) == int((prior["count"].astype(np.int64) & 0xFFFFFFFF).sum()) + st["merged_points"]
    return st


def test_a_general_pose_against_the_restatement():
    cloud, P = _scene("uniform_box")
    src = _fine(cloud, P)
    Pd = dict(P, grid_len=0.3, z_len=0.2)
    o2 = cloud[0, :3] + np.float32([0.37, -0.21, 0.05])
    dst = _empty(Pd, o2)
    dst.create2DMap("slope", dev(cloud[1:10001]))
    pose = rigid(17.0, 4.0, (0.731, -0.419, 0.057))
    st = _check_against_restatement(dst, src, pose, (cloud[0, :3], P["grid_len"], P["z_len"]), (o2, Pd["grid_len"], Pd["z_len"]), base=10000)
    assert st["merged_nodes"] == src.sync()[0] and st["new_nodes"] > 0
    assert dst.export()["num_nodes"] == dst.sync()[0]
    # and once more, the other way round, with a threshold: the destination's smaller nodes stay behind
    st = _check_against_restatement(src, dst, np.linalg.inv(np.vstack([pose, [0, 0, 0, 1]]))[:3], (o2, Pd["grid_len"], Pd["z_len"]),
                                    (cloud[0, :3], P["grid_len"], P["z_len"]), base=len(cloud) - 1, min_count=3)
    assert st["below_min_count"] > 0 and st["merged_nodes"] > 0


# ---- 4. the smallest shapes that can go wrong ----

def _cells_map(cells, per=3, P=BOX):
    cloud = _cells_cloud(cells, per, P)
    m = _fine(cloud, P)
    assert m.sync()[0] == len(cells)
    return cloud, m


def test_smallest_shapes():
    # one node; a one-point node (S = 0)
    for per in (3, 1):
        cloud, m = _cells_map([(3, -2, 1)], per)
        d = _empty(BOX, cloud[0])
        st = d.merge_from(m)
        assert st["merged_nodes"] == 1 and st["merged_points"] == per and st["new_nodes"] == 1
        _same_bits(d.export(), m.export(), EXACT)
        parity.assert_parity(d.export(), parity.ref_from_cloud(cloud, BOX))
    # the columns at sx, sy = +-1 under a pose that flips the signs
    cells = [(1, 1, 1), (-1, 1, 1), (1, -1, 1), (-1, -1, 2), (2, -1, -1)]
    cloud, m = _cells_map(cells)
    o = cloud[0, :3].astype(np.float64)
    R = np.diag([-1.0, -1.0, 1.0])
    flip = np.concatenate([R, (o - R @ o)[:, None]], 1)
    d = _empty(BOX, cloud[0])
    d.merge_from(m, pose=flip)
    assert _keys(d.export()) == sorted((-x, -y, z) for x, y, z in cells)
    parity.assert_parity(d.export(), parity.ref_from_cloud(moved_cloud(cloud, flip), BOX))
    # 64, 65 and 257 source nodes in ONE destination node of 8x cells: the wave's and the workgroup's edges
    cube = [(x, y, z) for z in range(1, 9) for x in range(1, 9) for y in range(1, 9)]
    for n in (64, 65, 257):
        cloud, m = _cells_map(cube[:n])
        P8 = _coarse_params(BOX, 8, 8)
        d = _empty(P8, cloud[0])
        st = d.merge_from(m)
        out = d.export()
        assert st["merged_nodes"] == n and st["new_nodes"] == 1 and _keys(out) == [(1, 1, 1)] and out["count"].tolist() == [3 * n]
        parity.assert_parity(out, parity.ref_from_cloud(cloud, P8))
    # min_count 3 drops the one- and two-point nodes
    c1, c2, c3 = [(1, 1, 1), (2, 1, 1)], [(3, 1, 1), (4, 1, 1), (5, 1, 1)], [(6, 1, 1), (7, 2, 1)]
    parts = [_cells_cloud(c, per) for c, per in ((c1, 1), (c2, 2), (c3, 3))]
    cloud = np.concatenate([parts[0]] + [p[1:] for p in parts[1:]])
    m = _fine(cloud, BOX)
    d = _empty(BOX, cloud[0])
    st = d.merge_from(m, min_count=3)
    assert st == {"source_nodes": 7, "merged_nodes": 2, "merged_points": 6, "below_min_count": 5, "skipped": 0, "new_nodes": 2}
    assert _keys(d.export()) == sorted(c3)


def test_empty_sources_and_nodes_that_do_not_travel():
    cloud, P = _scene("uniform_box")
    body = cloud[1:]
    # a source with a finished build of zero nodes: nothing arrives, the stream position is the source's
    m = _fine(cloud, P)
    m.crop_box((30000, 30010, 30000, 30010), "keep_inside")
    assert m.sync()[0] == 0
    d = _empty(P, cloud[0])
    st = d.merge_from(m)
    assert st == {k: 0 for k in st} and d.sync() == (0, 0, 0)
    d.change2DMap("slope", dev(body[:500]))
    assert int(d.export()["first_idx"].min()) == len(body)
    # a translation of 10^6 m: every node is skipped, the map is the same bits, the stream position has advanced
    src = _fine(cloud, P)
    dst = _empty(P, cloud[0])
    dst.create2DMap("slope", dev(body[:20000]))
    before = dst.export()
    far = np.concatenate([np.eye(3), [[1e6], [0.0], [0.0]]], 1)
    st = dst.merge_from(src, pose=far)
    n = src.sync()[0]
    assert st == {"source_nodes": n, "merged_nodes": 0, "merged_points": 0, "below_min_count": 0, "skipped": n, "new_nodes": 0}
    _same_bits(dst.export(), before)
    lone = cloud[:1, :3] + np.float32([[41.3, 37.7, 9.1]])                     # a cell nothing has touched
    dst.change2DMap("slope", dev(lone))
    after = dst.export()
    new = np.flatnonzero(after["first_idx"] == 20000 + len(body))
    assert after["num_nodes"] == before["num_nodes"] + 1 and new.size == 1 and after["count"][new].tolist() == [1]


# ---- 5. growth ----

def test_a_small_destination_table_grows():
    """a table sized for 1 024 nodes (a first build of 800 points without a hint) receives the 18 642-node campus map"""
    cloud, P = _scene("campus_frame")
    body = cloud[1:]
    dst = _empty(P, cloud[0])
    dst.create2DMap("slope", dev(body[:800]))
    early = dst.export()
    assert early["num_nodes"] <= 1024
    src = _fine(cloud, P)
    st = dst.merge_from(src)
    out = dst.export()
    assert st["merged_nodes"] == src.sync()[0] > 18000 and out["num_nodes"] == early["num_nodes"] + st["new_nodes"]
    whole = np.concatenate([cloud[:801], body])
    parity.assert_parity(out, _oracle(("campus", "800 + all"), whole, P))
    where = {k: i for i, k in enumerate(zip(out["sx"].tolist(), out["sy"].tolist(), out["sz"].tolist()))}
    rows = np.array([where[k] for k in zip(early["sx"].tolist(), early["sy"].tolist(), early["sz"].tolist())])
    assert (out["count"][rows] >= early["count"]).all() and np.array_equal(out["first_idx"][rows], early["first_idx"])


# ---- 6. the source is untouched ----

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
    d = _empty(dict(P, grid_len=0.4, z_len=0.2), cloud[0])
    assert d.merge_from(m, pose=rigid(3.0, 1.0, (0.2, 0.1, 0.0)))["merged_nodes"] == counts[0]
    after = m.export()
    assert m.sync() == counts
    _same_bits(after, before)
    again = m.cost_export()
    assert np.array_equal(again["h"].view(np.uint32), cost["h"].view(np.uint32)) and np.array_equal(again["state"], cost["state"])
    assert np.array_equal(m.query(pts).cpu().numpy(), rows)
    assert np.array_equal(rows.astype(np.int64), qr.node_rows(after, cloud[1:][::7], cloud[0], P["grid_len"], P["z_len"]))


# ---- 7. refusals ----

def test_refusals_leave_the_destination_as_it_was():
    import torch
    import grid_ndt_amd as g
    from grid_ndt_amd._lib import MergeParams
    cloud, P = _scene("uniform_box")
    src = _fine(cloud, P)
    dst = _empty(P, cloud[0])
    dst.create2DMap("slope", dev(cloud[1:20001]))
    before = dst.export()
    L = src._L
    null = C.c_void_p(0)

    def call(d, s, pose=None, prm=None, stream=null):
        T = None if pose is None else np.ascontiguousarray(pose, np.float64)
        return L.gndt_merge_map_device(d, s, C.c_void_p(T.ctypes.data if T is not None else 0), C.byref(prm) if prm is not None else None,
                                       None, stream)

    def refused(rc, text=None):
        assert rc == ERR_INVALID
        if text:
            assert text in L.gndt_last_error(dst._h).decode() and text in L.gndt_last_error(src._h).decode()
        _same_bits(dst.export(), before)

    refused(call(dst._h, None))                                                     # a null handle
    assert call(None, src._h) == ERR_INVALID and call(None, None) == ERR_INVALID
    refused(call(dst._h, dst._h))                                                   # src == dst
    for bad in (np.nan, np.inf, -np.inf):                                           # a non-finite pose entry
        for at in ((0, 0), (1, 3), (2, 2)):
            T = np.eye(4)[:3].copy()
            T[at] = bad
            refused(call(dst._h, src._h, T), "non-finite")
    refused(call(dst._h, src._h, prm=MergeParams(0, 1)), "reserved")
    refused(call(dst._h, src._h, prm=MergeParams(-1, 0)), "min_count")
    with pytest.raises(g.GndtError) as e:
        dst.merge_from(src, min_count=-2)
    assert e.value.code == ERR_INVALID and "min_count" in str(e.value)
    empty = _empty(P, cloud[0])                                                     # no finished build in the source
    empty.reset("slope")
    refused(call(dst._h, empty._h))
    part = handle(P, PARTITION)                                                    # a source that is not in the node table
    part.setCloudFirst(cloud[0])
    part.create2DMap("slope", dev(cloud[1:]))
    refused(call(dst._h, part._h))
    assert "node table" in L.gndt_last_error(dst._h).decode()
    bare = handle(P, ATOMIC)                                                       # a destination without an origin
    bare._ensure("slope", need_origin=False)
    assert call(bare._h, src._h) == ERR_INVALID and "origin" in L.gndt_last_error(bare._h).decode()
    held = part.export()                                                            # a destination that holds a PARTITION-built map
    assert call(part._h, src._h) == ERR_INVALID and "gndt_reset" in L.gndt_last_error(part._h).decode()
    _same_bits(part.export(), held)
    full = _empty(P, cloud[0])                                                      # the two streams together exceed 2^32 - 2 points
    full.reset("slope")
    full.accumulate("slope", dev(cloud[1:101]), first_idx_base=0xFFFFFFFE - 100 - (len(cloud) - 1) + 1)
    held = _sorted_stats(_stats(full))
    assert call(full._h, src._h) == ERR_INVALID and "2^32" in L.gndt_last_error(full._h).decode()
    now = _sorted_stats(_stats(full))
    assert all(np.array_equal(held[k].view(np.uint64) if k == "sums" else held[k], now[k].view(np.uint64) if k == "sums" else now[k]) for k in held)
    if torch.cuda.device_count() > 1:                                               # handles on different devices
        far = g.TwoDmap(P["grid_len"], P["z_len"], device=1, strategy=ATOMIC)
        far.setCloudFirst(cloud[0])
        far.reset("slope")
        assert call(far._h, src._h) == ERR_INVALID
        torch.cuda.set_device(0)
    # a capturing stream: refused, and the capture goes on
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    x = torch.zeros(16, device="cuda")
    torch.cuda.synchronize()
    with g.graph_capture(graph, stream=s):
        rc = call(dst._h, src._h, stream=C.c_void_p(s.cuda_stream))
        x.add_(1.0)
    graph.replay()
    torch.cuda.synchronize()
    assert float(x[0]) == 1.0
    refused(rc, "hipGraph")
    # and the same call outside the capture works
    assert call(dst._h, src._h) == 0
    assert dst.export()["num_nodes"] == src.sync()[0]


# ---- 8. stitch ----

def test_stitch_registers_then_merges():
    """drivable_site(100 000), COST_PARAMS; the other map holds every second point; start B of the registration tests"""
    from tests.test_score_derivs_host import starts
    cloud, P = scenes.drivable_site(100_000), scenes.COST_PARAMS
    other = _empty(P, cloud[0])
    other.create2DMap("slope", dev(cloud[1:][::2]))
    cells = other.export()
    scan = dev(cells["mean"][(cells["flags"] & 1) != 0])
    T0 = starts(P)["B"]
    a, b = _fine(cloud, P), _fine(cloud, P)
    ref = a.register(scan, T0)
    res, st = a.stitch(other, T0)
    assert np.array_equal(np.asarray(res["T"]).view(np.uint64), np.asarray(ref["T"]).view(np.uint64))
    assert (res["reason"], res["iterations"]) == (ref["reason"], ref["iterations"])
    st_b = b.merge_from(other, pose=ref["T"])
    assert st == st_b and st["merged_nodes"] == cells["num_nodes"] and st["merged_points"] == len(cloud[1:][::2])
    _same_bits(a.export(), b.export(), EXACT)


# ---- 9. a graph recorded before a merge ----

def test_an_update_graph_recorded_before_a_merge_is_reported_stale():
    """as after a crop or a clear: the replay is an error at sync (GNDT_ERR_CAPACITY), never a silently wrong map"""
    import torch
    import grid_ndt_amd as g
    P = scenes.TERRAIN_PARAMS
    frames = scenes.terrain_frames(3, points_per_frame=32_768)
    origin, f0, f1 = frames[0], frames[1:32_769], frames[32_769:65_537]
    dst = handle(P, ATOMIC, max_points_hint=400_000, max_nodes_hint=400_000)
    dst.setCloudFirst(origin)
    dst.change2DMap("slope", dev(f0))
    src = _empty(P, origin)
    src.create2DMap("slope", dev(f1[:8000]))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        buf = dev(f1)
        s.wait_stream(torch.cuda.default_stream())
        graph = torch.cuda.CUDAGraph()
        with g.graph_capture(graph, s):
            dst.change2DMap("slope", buf, s)
        s.synchronize()
        n0 = dst.sync()[0]
        st = dst.merge_from(src, stream=s)
        assert st["merged_points"] == 8000 and dst.sync()[0] == n0 + st["new_nodes"]
        graph.replay()
        s.synchronize()
        with pytest.raises(g.GndtError) as e:
            dst.sync()
        assert e.value.code == 5 and "replay" in str(e.value)
    del graph
