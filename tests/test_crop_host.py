"""CPU tier: gndt_crop_box_from_world (host helper of the region crop, include/gndt.h) keys the ends of a world rectangle as the codec
keys points (gndt_trans_morton_xyz, query_ref.keys), so that the box holds exactly the columns of the points inside the rectangle; bad
rectangles and null pointers are refused."""
import ctypes as C

import numpy as np
import pytest

from tests import query_ref as qr

ERR_INVALID = 1


def _box(L, origin, grid_len, lo, hi):
    from grid_ndt_amd._lib import CropBox
    b = CropBox()
    rc = L.gndt_crop_box_from_world((C.c_float * 3)(*origin), C.c_float(grid_len), (C.c_float * 2)(*lo), (C.c_float * 2)(*hi), C.byref(b))
    return rc, (b.sx_min, b.sx_max, b.sy_min, b.sy_max)


def _codec_xy(L, origin, grid_len, p):
    q, key = C.create_string_buffer(2), C.create_string_buffer(16)
    nx, ny, sz = C.c_int32(), C.c_int32(), C.c_int32()
    rc = L.gndt_trans_morton_xyz((C.c_float * 3)(*origin), C.c_float(grid_len), C.c_float(1.0), (C.c_float * 3)(p[0], p[1], 0.0), q,
                                 C.byref(nx), C.byref(ny), C.byref(sz), key)
    assert rc == 0
    letter = q.value.decode()
    sx = nx.value if letter in "AB" else -nx.value
    sy = ny.value if letter in "AC" else -ny.value
    return sx, sy


def _check_box_is_the_sampled_columns(L, origin, grid_len, lo, hi, samples):
    rc, box = _box(L, origin, grid_len, lo, hi)
    assert rc == 0
    lo32, hi32 = np.float32(lo), np.float32(hi)
    inside = samples[((samples >= lo32) & (samples <= hi32)).all(1)]
    sx, sy, _, _, ok = qr.keys(np.c_[inside, np.zeros(len(inside), np.float32)], origin, grid_len, 1.0)
    assert ok.all()
    # every sampled point inside the rectangle lies in the box, and the box's extreme columns are met by the rectangle's corners
    assert sx.min() >= box[0] and sx.max() <= box[1] and sy.min() >= box[2] and sy.max() <= box[3]
    corners = np.array([lo32, hi32], np.float32)
    csx, csy, _, _, _ = qr.keys(np.c_[corners, np.zeros(2, np.float32)], origin, grid_len, 1.0)
    assert (csx[0], csx[1], csy[0], csy[1]) == box
    # the codec's own keys of the corners (gndt_trans_morton_xyz) agree
    assert _codec_xy(L, origin, grid_len, lo32)[0] == box[0] and _codec_xy(L, origin, grid_len, hi32)[0] == box[1]
    assert _codec_xy(L, origin, grid_len, lo32)[1] == box[2] and _codec_xy(L, origin, grid_len, hi32)[1] == box[3]
    # every column of the box holds a sampled point: the box is exactly the columns of the points inside (dense samples)
    got = set(zip(sx.tolist(), sy.tolist()))
    want = {(x, y) for x in range(box[0], box[1] + 1) if x != 0 for y in range(box[2], box[3] + 1) if y != 0}
    assert got == want
    return box


@pytest.mark.parametrize("grid_len", [0.2, 0.5, 0.1])
@pytest.mark.parametrize("origin", [(0.0, 0.0, 0.0), (12.345, -7.5, 1.0), (-100.3, 55.55, -3.0)])
def test_box_from_world_is_the_columns_of_the_points_inside(native_lib, origin, grid_len):
    rng = np.random.default_rng(0x5EED0C0)
    o = np.float32(origin[:2])
    for k in range(24):
        c = o + rng.uniform(-6.0, 6.0, 2).astype(np.float32)
        half = rng.uniform(0.01, 2.5, 2).astype(np.float32)
        lo, hi = (c - half).astype(np.float32), (c + half).astype(np.float32)
        # dense samples of the rectangle (its ends included) plus a margin around it
        g = [np.concatenate([np.linspace(lo[a] - 1.0, hi[a] + 1.0, 401, dtype=np.float32), [lo[a], hi[a]]]) for a in range(2)]
        xx, yy = np.meshgrid(g[0], g[1])
        samples = np.c_[xx.ravel(), yy.ravel()].astype(np.float32)
        _check_box_is_the_sampled_columns(native_lib, origin, grid_len, lo.tolist(), hi.tolist(), samples)


@pytest.mark.parametrize("grid_len", [0.5, 0.25])
def test_box_from_world_is_exact_on_lattice_multiples_and_the_origin(native_lib, grid_len):
    """rectangle ends exactly on cell borders (o + k * len, representable) and on the origin, in all four quadrants"""
    origin = (2.0, -3.0, 0.0)
    o = np.float32(origin[:2])
    for kx0, kx1, ky0, ky1 in [(0, 2, 0, 3), (-3, 0, 0, 2), (0, 4, -2, 0), (-2, -1, -5, 0), (-1, 1, -1, 1), (3, 3, -4, -4), (0, 0, 0, 0)]:
        lo = (o + np.float32([kx0, ky0]) * np.float32(grid_len)).astype(np.float32)
        hi = (o + np.float32([kx1, ky1]) * np.float32(grid_len)).astype(np.float32)
        g = [np.concatenate([np.linspace(lo[a] - 2 * grid_len, hi[a] + 2 * grid_len, 257, dtype=np.float32), [lo[a], hi[a]],
                             [np.nextafter(lo[a], np.float32(np.inf)), np.nextafter(hi[a], np.float32(-np.inf))]]).astype(np.float32)
             for a in range(2)]
        xx, yy = np.meshgrid(g[0], g[1])
        samples = np.c_[xx.ravel(), yy.ravel()].astype(np.float32)
        box = _check_box_is_the_sampled_columns(native_lib, origin, grid_len, lo.tolist(), hi.tolist(), samples)
        # a point on a border belongs to the cell the codec gives it: o itself is column -1, o + k len column k (k != 0)
        def col(k):
            return k if k != 0 else -1
        assert box == (col(kx0), col(kx1), col(ky0), col(ky1))


def test_box_from_world_clamps_to_the_codec_range(native_lib):
    rc, box = _box(native_lib, (0.0, 0.0, 0.0), 0.1, (-1e7, -5.0), (1e7, 5.0))
    assert rc == 0 and box[0] == -65535 and box[1] == 65535 and box[2:] == (-50, 50)


def test_box_from_world_refuses_bad_input(native_lib):
    L = native_lib
    from grid_ndt_amd._lib import CropBox
    o, lo, hi = (C.c_float * 3)(0, 0, 0), (C.c_float * 2)(0, 0), (C.c_float * 2)(1, 1)
    b = CropBox()
    assert _box(L, (0, 0, 0), 0.5, (1.0, 0.0), (0.0, 1.0))[0] == ERR_INVALID      # inverted x
    assert _box(L, (0, 0, 0), 0.5, (0.0, 1.0), (1.0, 0.0))[0] == ERR_INVALID      # inverted y
    assert _box(L, (0, 0, 0), 0.0, (0.0, 0.0), (1.0, 1.0))[0] == ERR_INVALID      # grid_len
    assert _box(L, (0, 0, 0), 0.5, (float("nan"), 0.0), (1.0, 1.0))[0] == ERR_INVALID
    assert _box(L, (0, 0, 0), 0.5, (0.0, 0.0), (float("inf"), 1.0))[0] == ERR_INVALID
    assert L.gndt_crop_box_from_world(None, C.c_float(0.5), lo, hi, C.byref(b)) == ERR_INVALID
    assert L.gndt_crop_box_from_world(o, C.c_float(0.5), None, hi, C.byref(b)) == ERR_INVALID
    assert L.gndt_crop_box_from_world(o, C.c_float(0.5), lo, None, C.byref(b)) == ERR_INVALID
    assert L.gndt_crop_box_from_world(o, C.c_float(0.5), lo, hi, None) == ERR_INVALID
    # the crop entry points refuse a null handle
    assert L.gndt_crop(None, C.byref(b), 0) == ERR_INVALID
    assert L.gndt_crop_device(None, C.byref(b), 0, None) == ERR_INVALID


def test_python_helper(native_lib):
    import grid_ndt_amd as g
    assert g.crop_box_from_world((0, 0, 0), 0.5, (0.1, -0.1), (1.1, 0.4)) == (1, 3, -1, 1)
    with pytest.raises(g.GndtError):
        g.crop_box_from_world((0, 0, 0), 0.5, (1.0, 0.0), (0.0, 1.0))
