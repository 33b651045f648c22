"""CPU tier: the raster export's code (grid_ndt_amd/csrc/gndt_query.hpp: raster_index, raster_count and the kernel's per-pixel function
raster_pixel at every mode and gather mask), compiled with g++ into tests/_consumer_shim.so, against a numpy restatement from the rows
(tests/raster_ref.py) on maps the oracle builds; gndt_raster_shape against numpy enumeration; and the product entry points refuse to run
without a GPU."""
import ctypes as C

import numpy as np
import pytest

from grid_ndt_amd import scenes
from tests import query_ref as qr
from tests import raster_ref as rr
from tests.host_emulation import HostMap, consumer_shim

ERR_INVALID = 1

SCENES = {
    "bridge_ground": lambda: (scenes.bridge_ground(), scenes.BRIDGE_PARAMS),
    "campus": lambda: (scenes.campus_frame(60_000), scenes.CAMPUS_PARAMS),
    "site_two_storey": lambda: (scenes.site_two_storey(400_000), scenes.COST_PARAMS),
    "face_lattice": lambda: (qr.face_lattice(grid_len=0.5, z_len=0.25), dict(grid_len=0.5, z_len=0.25, slope_interval=0.08)),
}
_maps = {}


def _map(name):
    if name not in _maps:
        cloud, P = SCENES[name]()
        _maps[name] = HostMap(cloud, P, seed=13)
    return _maps[name]


def _boxes(m):
    """the map's box, a box crossing 0 on both axes, one larger than the map, one outside it, a one-pixel box, a strip touching 0"""
    x0, x1, y0, y1 = m.box()
    r = m.n // 3
    one = (int(m.sx[r]), int(m.sx[r]), int(m.sy[r]), int(m.sy[r]))
    return [(x0, x1, y0, y1), (-3, 4, -5, 2), (x0 - 7, x1 + 5, y0 - 3, y1 + 9), (x1 + 10, x1 + 20, y0, y1), one,
            (0, max(x1, 1), y0, 0), (x0, x1, -1, 1)]


# ---- geometry ----------------------------------------------------------------------------------------------------------------------

AXES = [(-3, 4), (0, 5), (-6, 0), (0, 1), (-1, 0), (1, 1), (-1, -1), (7, 7), (-7, -7), (-65535, -65530), (65530, 65535), (-2, 2),
        (5, 9), (-9, -5), (-65535, 65535), (3, 2), (0, 0)]


@pytest.mark.parametrize("lo,hi", AXES)
def test_axis_index_and_count_enumerate_the_non_zero_indices(lo, hi):
    want = rr.axis(lo, hi)
    L = consumer_shim()
    assert L.rshim_count(lo, hi) == want.size
    if want.size and want.size < 1000:
        got = [L.rshim_index(lo, i) for i in range(want.size)]
        assert got == want.tolist()
    elif want.size:
        for i in (0, 1, 65534, 65535, 65536, want.size - 1):
            assert L.rshim_index(lo, i) == want[i]


def _shape(L, box):
    from grid_ndt_amd._lib import CropBox
    w, h = C.c_uint32(0xDEAD), C.c_uint32(0xBEEF)
    rc = L.gndt_raster_shape(C.byref(CropBox(*box)), C.byref(w), C.byref(h))
    return rc, (w.value, h.value)


def test_raster_shape_is_the_non_zero_index_count(native_lib):
    for ax in AXES:
        for ay in AXES[:9]:
            box = (ax[0], ax[1], ay[0], ay[1])
            w, h = rr.axis(*ax).size, rr.axis(*ay).size
            rc, got = _shape(native_lib, box)
            if w and h:
                assert rc == 0 and got == (w, h), box
            else:
                assert rc == ERR_INVALID, box


def test_raster_shape_refuses_bad_boxes(native_lib):
    for box in [(0, 0, 1, 5), (1, 5, 0, 0), (3, 2, 1, 1), (1, 1, 3, 2), (-65536, 1, 1, 2), (1, 65536, 1, 2), (1, 2, -65536, 2),
                (1, 2, 1, 65536), (-65535, 65535, -65535, 65535), (-40000, 40000, -40000, 40000)]:
        assert _shape(native_lib, box)[0] == ERR_INVALID, box
    # 2^31 pixels is allowed, one row more is not
    assert _shape(native_lib, (1, 32768, -32768, 32768)) == (0, (32768, 65536))
    assert _shape(native_lib, (-32768, 32768, 1, 32768)) == (0, (65536, 32768))
    assert _shape(native_lib, (1, 32769, -32768, 32768))[0] == ERR_INVALID
    from grid_ndt_amd._lib import CropBox
    w = C.c_uint32()
    assert native_lib.gndt_raster_shape(None, C.byref(w), C.byref(w)) == ERR_INVALID
    assert native_lib.gndt_raster_shape(C.byref(CropBox(1, 2, 1, 2)), None, C.byref(w)) == ERR_INVALID


def test_python_raster_shape(native_lib):
    import grid_ndt_amd as g
    assert g.raster_shape((-3, 4, 0, 5)) == (7, 5)
    with pytest.raises(g.GndtError):
        g.raster_shape((0, 0, 1, 1))


# ---- the per-pixel function ---------------------------------------------------------------------------------------------------------

def _z_refs(m):
    z = m.mean[(m.flags & 2) != 0, 2]
    return [float(np.median(z)), float(z.min()) - 1.0, float(z.max()) + 0.3, float(np.percentile(z, 80))]


@pytest.mark.parametrize("name", sorted(SCENES))
def test_every_mode_and_gather_mask_is_the_restatement(name):
    m = _map(name)
    for box in _boxes(m):
        for mode in (rr.LOWEST, rr.HIGHEST, rr.NEAREST_Z):
            for z_ref in (_z_refs(m) if mode == rr.NEAREST_Z else [0.0]):
                want = m.want(box, mode, z_ref)
                for gather in (0, 1, 2, 3):       # the layers the library asks each instantiation for
                    layers = ("row", "nodes") + (("z", "rough") if gather & 1 else ()) + (("h", "state") if gather & 2 else ())
                    got = m.raster(box, mode, z_ref, gather, layers)
                    for k in layers:
                        assert rr.same(got[k], want[k]), (name, box, mode, gather, k)


def test_null_layers_are_not_written():
    m = _map("campus")
    box = m.box()
    want = m.want(box, rr.HIGHEST)
    for layers in (("row",), ("nodes",), ("z",), ("rough", "state"), ("h",), ("row", "h")):
        got = m.raster(box, rr.HIGHEST, 0.0, 3, layers)
        assert set(got) == set(layers)
        for k in layers:
            assert rr.same(got[k], want[k]), (layers, k)


def test_bridge_lowest_and_highest_differ_on_the_multi_slope_columns():
    m = _map("bridge_ground")
    box = m.box()
    lo, hi = m.raster(box, rr.LOWEST), m.raster(box, rr.HIGHEST)
    slopes = rr.raster(m.cells, box, rr.LOWEST)
    cols = np.flatnonzero(m.row_ncol)
    multi = np.zeros(lo["row"].shape, bool)
    xs, ys = rr.axis(box[0], box[1]), rr.axis(box[2], box[3])
    for c in cols:
        r = np.arange(c, c + m.row_ncol[c])
        if ((m.flags[r] & 2) != 0).sum() > 1:
            multi[np.searchsorted(ys, m.sy[c]), np.searchsorted(xs, m.sx[c])] = True
    assert multi.sum() > 1000 and slopes["row"].size >= 9600
    assert ((lo["row"] != hi["row"]) == multi).all()
    assert (m.sz[hi["row"][multi]] > m.sz[lo["row"][multi]]).all()
    # nearest_z at the deck's height (z = 3, scenes.bridge_ground) picks the deck wherever the deck is over the ground
    deck = multi & (np.abs(hi["z"] - np.float32(3.0)) < np.float32(0.05))
    assert deck.sum() > 1000
    near = m.raster(box, rr.NEAREST_Z, 3.0)
    # (the deck's points at z = 3 sit on a level border: at its edges the deck is two slopes, the highest a hair further from 3)
    assert (np.abs(near["z"][deck] - np.float32(3.0)) < np.float32(0.05)).all()
    assert (near["row"][deck] != lo["row"][deck]).mean() > 0.9
    assert (near["row"][deck] == hi["row"][deck]).mean() > 0.95


def test_nearest_z_is_the_query_rule_at_the_pixel_centres():
    """NEAREST_Z's rows are those query_ref.nearest_slope_rows gives points at the pixel centres with z = z_ref"""
    m = _map("face_lattice")
    box = (-6, 6, -6, 6)
    xs, ys = rr.axis(box[0], box[1]), rr.axis(box[2], box[3])
    g = np.float32(m.P["grid_len"])
    cx = (m.origin[0] + np.sign(xs) * (np.abs(xs) - np.float32(0.5)) * g).astype(np.float32)
    cy = (m.origin[1] + np.sign(ys) * (np.abs(ys) - np.float32(0.5)) * g).astype(np.float32)
    X, Y = np.meshgrid(cx, cy)
    for z_ref in _z_refs(m):
        pts = np.stack([X.ravel(), Y.ravel(), np.full(X.size, np.float32(z_ref))], 1).astype(np.float32)
        sx, sy, _, _, _ = qr.keys(pts, m.origin, m.P["grid_len"], m.P["z_len"])
        assert (sx.reshape(X.shape) == xs[None, :]).all() and (sy.reshape(X.shape) == ys[:, None]).all()
        want = qr.nearest_slope_rows(m.cells, pts, m.origin, m.P["grid_len"], m.P["z_len"])
        assert (m.raster(box, rr.NEAREST_Z, z_ref)["row"].ravel() == want).all()


def test_no_cpu_fallback_for_rasters(native_lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import grid_ndt_amd as g
    m = g.TwoDmap(0.5, 0.5)
    m.setCloudFirst((0, 0, 0))
    for host in (False, True):
        with pytest.raises(g.GndtError) as e:
            m.raster((-2, 2, -2, 2), host=host)
        assert e.value.code == 2   # GNDT_ERR_NO_DEVICE
