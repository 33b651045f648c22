"""Plain numpy answers to free-space clearing (include/gndt.h "free-space clearing", gndt_clear_rays*), written from the definition: a
ray from the sensor origin o to an end point p is cut at e = o + d * min(1, max_range / |d|, max(0, |d| - end_margin) / |d|) (fp64);
it walks from the codec's column of o to that of e in |dx| + |dy| unit lattice steps, each across the plane the segment meets first
(fp64 crossing parameter clamped to [0, 1], a tie stepping x), and in every column the levels between its entry and exit levels (the
codec's levels of o and e at the ends, the codec's rule in fp64 at the crossings).  A row is passed by a ray whose walk visits its
voxel; it is protected when the NODE lookup of an uncut end point names it.  Every ray is advanced in lock step, vectorised over rays.
Shared by the CPU tier (tests/test_clear_host.py) and the GPU tier (tests/test_gpu_clear.py).  Test infrastructure only."""
import numpy as np

from tests import query_ref as qr

PROTECTED = np.uint32(0x80000000)
MAX_Z = (1 << 21) - 1


def _lin(s):
    return np.where(s > 0, s - 1, s)


def _signed(l):
    return np.where(l >= 0, l + 1, l)


def _level(z, oz, z_len):
    """sign(z - oz) * max(1, ceil(|z - oz| / z_len)), fp64"""
    c = np.clip(np.ceil(np.abs(z - np.float64(np.float32(oz))) / np.float64(np.float32(z_len))), 1.0, float(MAX_Z)).astype(np.int64)
    return np.where(z > np.float64(np.float32(oz)), c, -c)


def rays(origin_map, grid_len, z_len, o, pts, max_range=0.0, end_margin=0.0):
    """-> (ok, columns): ok[i] = point i defines a ray; columns = dict of arrays ray, sx, sy, lo, hi — every (ray, column) of the walks,
    in walk order per ray"""
    pts = np.asarray(pts, np.float32)[:, :3]
    o32 = np.asarray(o, np.float32)[:3]
    _, _, _, _, ok = qr.keys(pts, origin_map, grid_len, z_len)
    idx = np.flatnonzero(ok)
    p = pts[idx].astype(np.float64)
    r = o32.astype(np.float64)
    d = p - r
    L = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    f = np.ones(len(idx))
    pos = L > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        if max_range > 0:
            f = np.where(pos, np.minimum(f, np.float64(np.float32(max_range)) / L), f)
        f = np.where(pos, np.minimum(f, np.maximum(0.0, L - np.float64(np.float32(end_margin))) / L), f)
    e = np.where((f < 1.0)[:, None], (r[None, :] + d * f[:, None]).astype(np.float32), pts[idx])
    osx, osy, osz, _, _ = qr.keys(o32[None, :], origin_map, grid_len, z_len)
    esx, esy, esz, _, _ = qr.keys(e, origin_map, grid_len, z_len)
    m = len(idx)
    lx, ly = np.full(m, _lin(osx)[0], np.int64), np.full(m, _lin(osy)[0], np.int64)
    lx1, ly1 = _lin(esx).astype(np.int64), _lin(esy).astype(np.int64)
    lev_in = np.full(m, int(osz[0]), np.int64)
    sz_end = esz.astype(np.int64)
    gx, gy = np.float64(np.float32(origin_map[0])), np.float64(np.float32(origin_map[1]))
    g = np.float64(np.float32(grid_len))
    live = np.arange(m)
    out = {k: [] for k in ("ray", "sx", "sy", "lo", "hi")}
    while live.size:
        a, b = lx[live], ly[live]
        a1, b1 = lx1[live], ly1[live]
        mx, my = a != a1, b != b1
        last = ~mx & ~my
        with np.errstate(divide="ignore", invalid="ignore"):
            kx = np.where(a1 > a, a + 1, a).astype(np.float64)
            ky = np.where(b1 > b, b + 1, b).astype(np.float64)
            dx, dy = d[live, 0], d[live, 1]
            tx = np.where(dx == 0, 1.0, np.clip((gx + kx * g - r[0]) / dx, 0.0, 1.0))
            ty = np.where(dy == 0, 1.0, np.clip((gy + ky * g - r[1]) / dy, 0.0, 1.0))
        tx = np.where(mx, tx, 2.0)
        ty = np.where(my, ty, 2.0)
        step_x = mx & (~my | (tx <= ty))
        t = np.where(step_x, tx, ty)
        lev_out = np.where(last, sz_end[live], _level(r[2] + t * d[live, 2], origin_map[2], z_len))
        out["ray"].append(idx[live])
        out["sx"].append(_signed(a))
        out["sy"].append(_signed(b))
        out["lo"].append(np.minimum(lev_in[live], lev_out))
        out["hi"].append(np.maximum(lev_in[live], lev_out))
        lx[live] = np.where(step_x & ~last, a + np.where(a1 > a, 1, -1), a)
        ly[live] = np.where(~step_x & ~last, b + np.where(b1 > b, 1, -1), b)
        lev_in[live] = lev_out
        live = live[~last]
    cols = {k: np.concatenate(v) if v else np.zeros(0, np.int64) for k, v in out.items()}
    return ok, cols


def voxels(cols):
    """-> ray, sx, sy, sz of every voxel the walks visit (levels lo..hi, 0 skipped)"""
    lo, hi = cols["lo"], cols["hi"]
    cnt = hi - lo + 1 - ((lo < 0) & (hi > 0))
    rep = np.repeat(np.arange(lo.size), cnt)
    start = np.concatenate([[0], np.cumsum(cnt)[:-1]]) if lo.size else np.zeros(0, np.int64)
    off = np.arange(rep.size) - start[rep]
    z = lo[rep] + off
    z = np.where((lo[rep] < 0) & (z >= 0), z + 1, z)
    return cols["ray"][rep], cols["sx"][rep], cols["sy"][rep], z


def passes(cells, origin_map, grid_len, z_len, o, pts, max_range=0.0, end_margin=0.0):
    """-> (words, rays, skipped): per row the pass count, | PROTECTED where an uncut end point's NODE lookup names it (uint32)"""
    ok, cols = rays(origin_map, grid_len, z_len, o, pts, max_range, end_margin)
    n = int(cells["num_nodes"]) if "num_nodes" in cells else len(cells["sx"])
    keys = qr.pack(cells["sx"], cells["sy"], cells["sz"])
    order = np.argsort(keys, kind="stable")
    ks = keys[order]
    _, sx, sy, sz = voxels(cols)
    vk = qr.pack(sx, sy, sz)
    pos = np.searchsorted(ks, vk)
    pos = np.minimum(pos, max(n - 1, 0))
    hit = (ks[pos] == vk) if n else np.zeros(vk.size, bool)
    words = np.bincount(order[pos[hit]], minlength=n).astype(np.uint32) if n else np.zeros(0, np.uint32)
    pts = np.asarray(pts, np.float32)
    rows = qr.node_rows(cells, pts[ok], origin_map, grid_len, z_len) if ok.any() else np.zeros(0, np.int64)
    rows = rows[rows >= 0]
    words[rows] |= PROTECTED
    return words, int(ok.sum()), int((~ok).sum())


def cleared_rows(words, min_passes):
    """rows a clear with min_passes drops"""
    return ((words & PROTECTED) == 0) & ((words & np.uint32(0x7FFFFFFF)) >= np.uint32(min_passes))
