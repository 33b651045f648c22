"""CPU tier: the point queries' per-point code (grid_ndt_amd/csrc/gndt_query.hpp: query_points at ILP 1, 2 and 4, and the ctab_find
probe behind it), compiled with g++ into tests/_consumer_shim.so, against plain numpy lookups of the rows (tests/query_ref.py) on maps the
oracle builds; and the product entry point refuses to run without a GPU."""

import numpy as np
import pytest

from grid_ndt_amd import scenes
from tests import query_ref as qr
from tests.host_emulation import HostMap, consumer_shim


def _face_scene():
    P = dict(grid_len=0.5, z_len=0.25, slope_interval=0.08)
    return qr.face_lattice(grid_len=P["grid_len"], z_len=P["z_len"]), P


SCENES = {
    "bridge_ground": lambda: (scenes.bridge_ground(), scenes.BRIDGE_PARAMS),
    "campus": lambda: (scenes.campus_frame(60_000), scenes.CAMPUS_PARAMS),
    "uniform_box": lambda: (scenes.uniform_box(40_001, half_xy=6.0, half_z=1.0), dict(grid_len=0.5, z_len=0.5, slope_interval=0.08)),
    "face_lattice": _face_scene,
}
_maps = {}


def _map(name, table="library"):
    if (name, table) not in _maps:
        cloud, P = SCENES[name]()
        _maps[(name, table)] = (cloud, HostMap(cloud, P, table))
    return _maps[(name, table)]


def _queries(cloud, m, seed=3):
    """the built points, then random points over (and beyond) the map's extent, then the odd ones"""
    body = cloud[1:, :3]
    lo, hi = body.min(0), body.max(0)
    rng = np.random.default_rng(seed)
    rnd = rng.uniform(lo - 1.0, hi + 1.0, size=(20_000, 3)).astype(np.float32)
    odd = qr.odd_points(m.origin, m.P["grid_len"], m.P["z_len"], (float(lo.min()), float(hi.max())))
    return np.concatenate([body, rnd, odd]).astype(np.float32)


@pytest.mark.parametrize("table", ["library", "full"])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_node_query_is_the_row_with_the_points_key(name, table):
    cloud, m = _map(name, table)
    pts = _queries(cloud, m)
    want = qr.node_rows(m.cells, pts, m.origin, m.P["grid_len"], m.P["z_len"])
    nb = cloud.shape[0] - 1
    # every built point finds its node: the rows' counts and first points are the build's
    assert (want[:nb] >= 0).all()
    assert (np.bincount(want[:nb], minlength=m.n) == m.cells["count"]).all()
    assert (want[np.asarray(m.cells["first_idx"], np.int64)] == np.arange(m.n)).all()
    for ilp, threads in ((1, 1), (2, 7), (4, 64), (1, 1000)):
        got = m.query(pts, 0, ilp, threads)
        assert (got == want).all(), (ilp, threads, np.flatnonzero(got != want)[:10])
    # the odd points: no key, no row (and no error)
    odd = pts[nb + 20_000:]
    sx, sy, sz, ok_xy, ok = qr.keys(odd, m.origin, m.P["grid_len"], m.P["z_len"])
    assert (~np.isfinite(odd).all(1)).sum() == 9 and not ok[~np.isfinite(odd).all(1)].any()
    assert (m.query(odd, 0)[~ok] == qr.NO_ROW).all()


@pytest.mark.parametrize("table", ["library", "full"])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_nearest_slope_query_matches_a_brute_force(name, table):
    cloud, m = _map(name, table)
    pts = _queries(cloud, m, seed=5)
    rng = np.random.default_rng(9)
    z = pts[:, 2].copy()
    fin = np.isfinite(pts).all(1)
    pts2 = pts.copy()
    pts2[fin, 2] = rng.uniform(z[fin].min() - 3, z[fin].max() + 3, size=int(fin.sum())).astype(np.float32)   # any z
    for q in (pts, pts2):
        want = qr.nearest_slope_rows(m.cells, q, m.origin, m.P["grid_len"], m.P["z_len"])
        for ilp, threads in ((1, 1), (2, 5), (4, 64)):
            got = m.query(q, 1, ilp, threads)
            assert (got == want).all(), (ilp, threads, np.flatnonzero(got != want)[:10])
        hit = want >= 0
        assert hit.any() and (m.flags[want[hit]] & 2).all()


def test_nearest_slope_tie_goes_to_the_smaller_level():
    """two slopes of one column at the same distance from the query's z: the smaller sz wins, whatever their order in the column"""
    cloud, m = _map("face_lattice")
    body = cloud[1:]
    sx, sy, _, _, _ = qr.keys(body, m.origin, m.P["grid_len"], m.P["z_len"])
    tried = 0
    for col in np.flatnonzero(m.row_ncol >= 2):
        rows = np.arange(col, col + m.row_ncol[col])
        rows = rows[(m.flags[rows] & 2) != 0]
        if rows.size < 2:
            continue
        lo, hi = sorted(rows[:2], key=lambda r: m.sz[r])
        z_lo, z_hi = m.mean[lo, 2], m.mean[hi, 2]
        k = np.flatnonzero((sx == m.sx[col]) & (sy == m.sy[col]))[0]
        saved = m.mean.copy()
        try:
            for first, second in ((lo, hi), (hi, lo)):      # the tie from either side: the query's z halfway, both means mirrored
                mid = np.float32(0.5) * (z_lo + z_hi)
                m.mean[second, 2] = np.float32(mid + (mid - m.mean[first, 2]))
                if np.abs(m.mean[second, 2] - mid) != np.abs(m.mean[first, 2] - mid):
                    continue
                p = np.array([[body[k, 0], body[k, 1], mid]], np.float32)
                for ilp in (1, 2, 4):
                    assert m.query(p, 1, ilp)[0] == lo
                assert qr.nearest_slope_rows(m.cells | {"mean": m.mean}, p, m.origin, m.P["grid_len"], m.P["z_len"])[0] == lo
                tried += 1
                m.mean[:] = saved
        finally:
            m.mean[:] = saved
    assert tried >= 4


def test_cost_gather_is_the_rows_cost_and_flt_max_without_a_row():
    cloud, m = _map("bridge_ground")
    pts = _queries(cloud, m)
    for mode in (0, 1):
        for ilp in (1, 2, 4):
            rows, h, st = m.query(pts, mode, ilp, threads=33, gather=True)
            hit = rows >= 0
            assert hit.any() and (~hit).any()
            assert (h[hit].view(np.uint32) == m.h_bits[rows[hit]]).all() and (st[hit] == m.state[rows[hit]]).all()
            assert (h[~hit] == qr.FLT_MAX).all() and (st[~hit] == 0).all()


def test_stride_16_points_give_the_same_rows():
    cloud, m = _map("campus")
    pts = _queries(cloud, m)
    p4 = np.concatenate([pts, np.full((pts.shape[0], 1), np.float32(7.0))], 1)
    for mode in (0, 1):
        assert (m.query(p4, mode, 2, 9) == m.query(pts, mode, 2, 9)).all()


def test_probe_walks_past_other_columns():
    """in a full table most columns do not sit in their first slot: ctab_find must still name every column's first row"""
    _, m = _map("campus", "full")
    first = np.flatnonzero(m.row_ncol)
    got = np.array([consumer_shim().qshim_ctab_find(m.ctab_key.ctypes.data, m.ctab_val.ctypes.data, m.tsize, int(m.sx[r]), int(m.sy[r])) for r in first])
    assert (got == first).all()


def test_no_cpu_fallback_for_queries(native_lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import grid_ndt_amd as g
    m = g.TwoDmap(0.5, 0.5)
    m.setCloudFirst((0, 0, 0))
    with pytest.raises(g.GndtError) as e:
        m.query(np.zeros((10, 3), np.float32))
    assert e.value.code == 2   # GNDT_ERR_NO_DEVICE
