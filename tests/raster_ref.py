"""Plain numpy answers to the raster export of include/gndt.h (gndt_raster*), written from the definitions and the rows alone: the image
of a box (sx_min, sx_max, sy_min, sy_max) has one pixel per non-zero (sx, sy) of the box, row-major from the smallest; a pixel's slope
is, among its column's rows with the slope flag, the one with the least sz (lowest), the greatest sz (highest) or the least
|mean_z - z_ref| in fp32, a tie going to the smaller sz (nearest_z).  Shared by the CPU tier (tests/test_raster_host.py) and the GPU
tier (tests/test_gpu_raster.py).  Test infrastructure only."""
import numpy as np

NO_ROW = -1
QNAN_BITS = np.uint32(0x7FC00000)
FLT_MAX = np.float32(np.finfo(np.float32).max)
LOWEST, HIGHEST, NEAREST_Z = 0, 1, 2
MODES = {"lowest": LOWEST, "highest": HIGHEST, "nearest_z": NEAREST_Z}


def axis(lo, hi):
    """the non-zero integers of [lo, hi], ascending: an axis's pixels"""
    s = np.arange(int(lo), int(hi) + 1, dtype=np.int64)
    return s[s != 0]


def raster(cells, box, mode, z_ref=0.0, h_bits=None, state=None):
    """-> dict of (height, width) layers: row (int64, -1 for none), z / rough (float32, quiet NaN), nodes (int64), and with a cost map
    (h_bits: uint32 per row, state per row) h (float32, FLT_MAX) and state (int64, 0)"""
    mode = MODES[mode] if isinstance(mode, str) else int(mode)
    xs, ys = axis(box[0], box[1]), axis(box[2], box[3])
    W, H = xs.size, ys.size
    sx, sy = np.asarray(cells["sx"], np.int64), np.asarray(cells["sy"], np.int64)
    sz = np.asarray(cells["sz"], np.int64)
    flags = np.asarray(cells["flags"], np.uint32)
    mz = np.asarray(cells["mean"], np.float32).reshape(-1, 3)[:, 2]
    inside = (sx >= box[0]) & (sx <= box[1]) & (sy >= box[2]) & (sy <= box[3])
    rows = np.flatnonzero(inside)
    pix = np.searchsorted(ys, sy[rows]) * W + np.searchsorted(xs, sx[rows])
    nodes = np.bincount(pix, minlength=W * H).astype(np.int64)
    slope = rows[(flags[rows] & 2) != 0]
    spix = np.searchsorted(ys, sy[slope]) * W + np.searchsorted(xs, sx[slope])
    if mode == LOWEST:
        order = np.lexsort((sz[slope], spix))
    elif mode == HIGHEST:
        order = np.lexsort((-sz[slope], spix))
    else:
        d = np.abs(mz[slope] - np.float32(z_ref)).astype(np.float32)
        order = np.lexsort((sz[slope], d, spix))
    slope, spix = slope[order], spix[order]
    first = np.ones(spix.size, bool)
    first[1:] = spix[1:] != spix[:-1]
    row = np.full(W * H, NO_ROW, np.int64)
    row[spix[first]] = slope[first]
    hit = row >= 0
    out = {"row": row, "nodes": nodes}
    z = np.full(W * H, QNAN_BITS, np.uint32).view(np.float32)
    z[hit] = mz[row[hit]]
    rough = np.full(W * H, QNAN_BITS, np.uint32).view(np.float32)
    rough[hit] = np.asarray(cells["rough"], np.float32)[row[hit]]
    out.update(z=z, rough=rough)
    if h_bits is not None:
        h = np.full(W * H, FLT_MAX, np.float32)
        h[hit] = np.asarray(h_bits, np.uint32)[row[hit]].view(np.float32)
        st = np.zeros(W * H, np.int64)
        st[hit] = np.asarray(state)[row[hit]]
        out.update(h=h, state=st)
    return {k: v.reshape(H, W) for k, v in out.items()}


def same(got, want):
    """layer equality, bit for bit for floats (NaN included), by value for integers (-1 == 0xFFFFFFFF as int32)"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return False
    if want.dtype == np.float32:
        return bool(np.array_equal(np.ascontiguousarray(got, np.float32).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)))
    return bool(np.array_equal(got.astype(np.int64), want.astype(np.int64)))
