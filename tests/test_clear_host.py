"""CPU tier: free-space clearing's code (grid_ndt_amd/csrc/gndt_ray.hpp: the walk of a ray and the count-only passes of the kernels,
with and without the extent skip), compiled with g++ into tests/_consumer_shim.so, against hand-derived walks and against the numpy
restatement of the definition (tests/clear_ref.py) on maps the oracle builds; and the product entry points refuse to run without a GPU."""

import numpy as np
import pytest

from grid_ndt_amd import scenes
from tests import clear_ref as cr
from tests.host_emulation import HostMap, consumer_shim


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def shim_walk(map_origin, grid_len, z_len, o, p, max_range=0.0, end_margin=0.0):
    """-> [(sx, sy, lo, hi), ...] or None for a skipped point"""
    mo, oo, pp = _f32(map_origin), _f32(o), _f32(p)
    cap = 1 << 16
    out = np.zeros((cap, 4), np.int32)
    k = consumer_shim().cshim_walk(mo.ctypes.data, grid_len, z_len, oo.ctypes.data, pp.ctypes.data, max_range, end_margin, out.ctypes.data, cap)
    if k < 0:
        return None
    assert k <= cap
    return [tuple(int(v) for v in r) for r in out[:k]]


def ref_walk(map_origin, grid_len, z_len, o, p, max_range=0.0, end_margin=0.0):
    ok, cols = cr.rays(map_origin, grid_len, z_len, o, _f32(p)[None, :], max_range, end_margin)
    if not ok[0]:
        return None
    return [tuple(int(cols[k][i]) for k in ("sx", "sy", "lo", "hi")) for i in range(cols["sx"].size)]


UNIT = ((0.0, 0.0, 0.0), 1.0, 1.0)
O = (0.5, 0.5, 0.5)
HAND = [
    ("axis_parallel", O, (3.5, 0.5, 0.5), 0, 0, [(1, 1, 1, 1), (2, 1, 1, 1), (3, 1, 1, 1), (4, 1, 1, 1)]),
    ("vertical", O, (0.5, 0.5, 3.5), 0, 0, [(1, 1, 1, 4)]),
    ("vertical_down", (0.5, 0.5, 2.5), (0.5, 0.5, -1.5), 0, 0, [(1, 1, -2, 3)]),
    ("zero_length", O, O, 0, 0, [(1, 1, 1, 1)]),
    ("corner_tie_x_first", O, (2.5, 2.5, 0.5), 0, 0, [(1, 1, 1, 1), (2, 1, 1, 1), (2, 2, 1, 1), (3, 2, 1, 1), (3, 3, 1, 1)]),
    ("across_x0", O, (-1.5, 0.5, 0.5), 0, 0, [(1, 1, 1, 1), (-1, 1, 1, 1), (-2, 1, 1, 1)]),
    ("all_quadrants", (-0.5, -0.5, 0.5), (1.5, 1.5, 0.5), 0, 0, [(-1, -1, 1, 1), (1, -1, 1, 1), (1, 1, 1, 1), (2, 1, 1, 1), (2, 2, 1, 1)]),
    ("quadrant_c", (0.5, -0.5, 0.5), (-1.5, 1.5, 0.5), 0, 0, [(1, -1, 1, 1), (-1, -1, 1, 1), (-1, 1, 1, 1), (-2, 1, 1, 1), (-2, 2, 1, 1)]),
    ("end_on_border_pos", O, (2.0, 0.5, 0.5), 0, 0, [(1, 1, 1, 1), (2, 1, 1, 1)]),
    ("end_on_border_neg", O, (-2.0, 0.5, 0.5), 0, 0, [(1, 1, 1, 1), (-1, 1, 1, 1), (-2, 1, 1, 1)]),
    ("climbing", O, (2.5, 0.5, 2.5), 0, 0, [(1, 1, 1, 1), (2, 1, 1, 2), (3, 1, 2, 3)]),
    ("max_range", O, (10.5, 0.5, 0.5), 2.0, 0, [(1, 1, 1, 1), (2, 1, 1, 1), (3, 1, 1, 1)]),
    ("end_margin", O, (10.5, 0.5, 0.5), 0, 3.0, [(s, 1, 1, 1) for s in range(1, 9)]),
    ("margin_longer_than_ray", O, (10.5, 0.5, 3.5), 0, 20.0, [(1, 1, 1, 1)]),
]


@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_hand_derived_walks(case):
    _, o, p, mr, em, want = case
    assert shim_walk(*UNIT, o, p, mr, em) == want
    assert ref_walk(*UNIT, o, p, mr, em) == want


def test_skipped_points():
    for p in ((np.nan, 0.5, 0.5), (0.5, np.inf, 0.5), (1e6, 0.5, 0.5)):
        assert shim_walk(*UNIT, O, p) is None and ref_walk(*UNIT, O, p) is None


def _terrain():
    P = scenes.TERRAIN_PARAMS
    frames = scenes.terrain_frames(2, points_per_frame=16_384)
    px, py = scenes._pose_xy(np.int64(1), 200.0, 14.0)
    f1 = frames[16_384:]
    sensor = (px, py, float(np.median(f1[:, 2])) + 1.8)
    return HostMap(frames, P), sensor, f1


def _drivable():
    P = scenes.COST_PARAMS
    cloud = scenes.drivable_site(60_000)
    sensor = (0.3, -0.2, float(np.max(cloud[:, 2])) + 1.5)
    return HostMap(cloud, P), sensor, cloud[1:]


@pytest.mark.parametrize("scene", ["terrain", "drivable"])
def test_random_rays_visit_the_restatements_voxels(scene):
    m, sensor, pts = {"terrain": _terrain, "drivable": _drivable}[scene]()
    rng = np.random.default_rng(7)
    sel = pts[rng.choice(len(pts), 300, replace=False)]
    # end points anywhere around the map as well (rays through empty space, across the origin's axes)
    lo, hi = pts[:, :3].min(0), pts[:, :3].max(0)
    extra = _f32(rng.uniform(lo, hi, size=(100, 3)))
    for p in np.concatenate([sel, extra]):
        for mr, em in ((0.0, 0.0), (7.5, 0.0), (0.0, 1.3), (4.0, 0.4)):
            assert shim_walk(m.origin, m.P["grid_len"], m.P["z_len"], sensor, p, mr, em) == \
                ref_walk(m.origin, m.P["grid_len"], m.P["z_len"], sensor, p, mr, em)


@pytest.mark.parametrize("scene", ["terrain", "drivable"])
def test_count_only_passes_equal_the_restatement(scene):
    m, sensor, pts = {"terrain": _terrain, "drivable": _drivable}[scene]()
    pts = _f32(pts[::4])
    pts[::97] = np.nan                                             # skipped, counted
    for mr, em in ((0.0, 0.0), (20.0, 0.0), (0.0, 0.5)):
        want, rays, skipped = cr.passes(m.cells, m.origin, m.P["grid_len"], m.P["z_len"], sensor, pts, mr, em)
        assert rays > 0 and skipped == len(pts[::97])
        assert (want & 0x7FFFFFFF).max() > 10 and ((want & cr.PROTECTED) != 0).sum() > 10
        for ext in (True, False):
            got, r2, s2 = m.passes(sensor, pts, mr, em, ext=ext)
            assert (r2, s2) == (rays, skipped)
            assert np.array_equal(got, want), (mr, em, ext, np.flatnonzero(got != want)[:10])


def test_no_cpu_fallback_for_clears(native_lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import grid_ndt_amd as g
    m = g.TwoDmap(0.5, 0.5)
    m.setCloudFirst((0, 0, 0))
    pts = np.ones((4, 3), np.float32)
    for kw in ({}, {"count_only": True}):
        with pytest.raises(g.GndtError) as e:
            m.clear_rays((0, 0, 1), pts, **kw)
        assert e.value.code == 2   # GNDT_ERR_NO_DEVICE
    # both entry points, called directly: a null handle is invalid
    from grid_ndt_amd import _lib
    L = _lib.lib()
    assert L.gndt_clear_rays(None, None, None, 0, 12, None, None, None) == 1
    assert L.gndt_clear_rays_device(None, None, None, 0, 12, None, None, None, None) == 1
