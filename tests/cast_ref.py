"""Plain numpy answers to ray casting (include/gndt.h "ray casting", gndt_cast_rays*), written from the definition: every ray from its
own origin o to its end point p is cut at e = o + d * min(1, max_range / |d|) (fp64) and walks free-space clearing's columns (the
restatement of tests/clear_ref.py with one origin per ray, which also keeps the crossing parameter of every step); a column visit
carries [t_in, t_out]; inside a column the map's rows with a level in the visit's range are looked at from the entry level towards the
exit level (here: the rows sorted by packed key, a column's slice of them taken forwards or backwards); the first candidate that
counts is the ray's answer.  Every ray is advanced in lock step, vectorised over rays; all arithmetic is float64 in the definition's
bracketing, so the library's outputs are matched bit for bit.
Shared by the CPU tier (tests/test_cast_host.py) and the GPU tier (tests/test_gpu_cast.py).  Test infrastructure only."""
import numpy as np

from tests import query_ref as qr
from tests import score_ref as sr

VOXEL, NDT = 0, 1
NO_ROW = qr.NO_ROW
MAX_Z = (1 << 21) - 1
SKIPPED, MISS, HIT = 0, 1, 2
_NAN32 = np.array([0x7FC00000], np.uint32).view(np.float32)[0]


def _lin(s):
    return np.where(s > 0, s - 1, s)


def _signed(l):
    return np.where(l >= 0, l + 1, l)


def _level(z, oz, z_len):
    """sign(z - oz) * max(1, ceil(|z - oz| / z_len)), fp64"""
    c = np.clip(np.ceil(np.abs(z - oz) / z_len), 1.0, float(MAX_Z)).astype(np.int64)
    return np.where(z > oz, c, -c)


def _cross(o_axis, length, k, r, d):
    """the walk's crossing rule: ((o_axis + k * length) - r) / d clamped to [0, 1]; 1 where d == 0"""
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (o_axis + k.astype(np.float64) * length - r) / d
    return np.where(d == 0, 1.0, np.clip(t, 0.0, 1.0))


def params(mode=VOXEL, min_count=0, max_range=0.0, min_range=0.0, cov_rel=0.0, cov_floor=0.0, max_d2=0.0, min_points=3):
    """the parameters as the library resolves them (the floats are the struct's float32 values widened)"""
    prm = sr.defaults(min_count=min_count, cov_rel=cov_rel, cov_floor=cov_floor, max_d2=max_d2, min_points=min_points)
    if mode == VOXEL:
        prm["min_count"] = int(min_count) if min_count else 1
    prm.update(mode=mode, max_range=float(np.float32(max_range)), min_range=float(np.float32(min_range)))
    return prm


def _cofactors(nodes, rows, prm):
    """scoring's A = S / (count - 1) + eps I and its cofactors, in the definition's order"""
    c = nodes.count[rows]
    S = nodes.cov[rows]
    with np.errstate(all="ignore"):
        inv = 1.0 / (np.maximum(c, 2) - 1).astype(np.float64)
        cxx, cxy, cxz, cyy, cyz, czz = (S[:, k] * inv for k in range(6))
        eps = np.maximum(prm["cov_rel"] * (((cxx + cyy) + czz) / 3.0), prm["cov_floor"])
        a00, a11, a22, a01, a02, a12 = cxx + eps, cyy + eps, czz + eps, cxy, cxz, cyz
        return (a11 * a22 - a12 * a12, a02 * a12 - a01 * a22, a01 * a12 - a02 * a11,
                a00 * a22 - a02 * a02, a01 * a02 - a00 * a12, a00 * a11 - a01 * a01)


def _candidates(nodes, rows, sz, lev_in, up, t_in, t_hi, r, d, L, grid, prm):
    """the candidates rows[i] (level sz[i]) of rays with origin r[i], direction d[i] -> (counts, range float64, d2 float64)"""
    oz, z_len = grid
    if prm["mode"] == VOXEL:
        valid = nodes.count[rows] >= prm["min_count"]
        t_z = _cross(oz, z_len, np.where(up, _lin(sz), _lin(sz) + 1), r[:, 2], d[:, 2])
        t = np.where(sz == lev_in, t_in, t_z)
        d2 = np.zeros(len(rows))
    else:
        c00, c01, c02, c11, c12, c22 = _cofactors(nodes, rows, prm)
        m = nodes.mean[rows]
        with np.errstate(all="ignore"):
            wx = (c00 * d[:, 0] + c01 * d[:, 1]) + c02 * d[:, 2]
            wy = (c01 * d[:, 0] + c11 * d[:, 1]) + c12 * d[:, 2]
            wz = (c02 * d[:, 0] + c12 * d[:, 1]) + c22 * d[:, 2]
            gx, gy, gz = m[:, 0] - r[:, 0], m[:, 1] - r[:, 1], m[:, 2] - r[:, 2]
            t = ((gx * wx + gy * wy) + gz * wz) / ((d[:, 0] * wx + d[:, 1] * wy) + d[:, 2] * wz)
        t = np.where(L > 0, t, 0.0)
    with np.errstate(invalid="ignore"):
        t = np.where(t >= t_in, t, t_in)              # (a NaN takes t_in)
        t = np.where(t > t_hi, t_hi, t)
    if prm["mode"] == NDT:
        q = r + t[:, None] * d
        _, valid, d2 = sr.d2_of(nodes, rows, q, prm)      # (count >= min_count and the max_d2 gate; raw d2)
    rng = t * L
    return valid & ~(rng < prm["min_range"]), rng, d2


def cast(cells, origin_map, grid_len, z_len, origins, ends, mode=VOXEL, min_points=3, **kw):
    """-> dict: status (SKIPPED / MISS / HIT), row (int64, NO_ROW), range and d2 (float32, the library's bits), stats {rays, skipped,
    hits}, and steps: dict of arrays ray, sx, sy, lev_in, lev_out, t_in, t_out — every (ray, column) of the walks, in walk order per
    ray (the whole walk, also behind a hit).  origins: (3,) or (n, 3|4); ends: (n, 3|4)."""
    prm = params(mode=mode, min_points=min_points, **kw)
    nodes = sr.Nodes(cells)
    ends = np.asarray(ends, np.float32)[:, :3]
    n = len(ends)
    o32 = np.asarray(origins, np.float32)
    o32 = np.broadcast_to(o32[:3], (n, 3)) if o32.ndim == 1 else o32[:, :3]
    ok = qr.keys(o32, origin_map, grid_len, z_len)[4] & qr.keys(ends, origin_map, grid_len, z_len)[4] if n else np.zeros(0, bool)
    idx = np.flatnonzero(ok)
    m = len(idx)
    r = o32[idx].astype(np.float64)
    d = ends[idx].astype(np.float64) - r
    L = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    f = np.ones(m)
    if prm["max_range"] > 0:
        with np.errstate(divide="ignore", invalid="ignore"):
            f = np.where(L > 0, np.minimum(f, prm["max_range"] / L), f)
    e = np.where((f < 1.0)[:, None], (r + d * f[:, None]).astype(np.float32), ends[idx])
    osx, osy, osz, _, _ = qr.keys(o32[idx], origin_map, grid_len, z_len)
    esx, esy, esz, _, _ = qr.keys(e, origin_map, grid_len, z_len)
    lx, ly = _lin(osx).astype(np.int64), _lin(osy).astype(np.int64)
    lx1, ly1 = _lin(esx).astype(np.int64), _lin(esy).astype(np.int64)
    lev_in = osz.astype(np.int64)
    sz_end = esz.astype(np.int64)
    gx, gy, gz = (np.float64(np.float32(v)) for v in origin_map[:3])
    g, zl = np.float64(np.float32(grid_len)), np.float64(np.float32(z_len))
    t_in = np.zeros(m)
    hit_row = np.full(m, NO_ROW, np.int64)
    hit_range = np.full(m, np.inf)
    hit_d2 = np.full(m, np.inf)
    live = np.arange(m)
    steps = {k: [] for k in ("ray", "sx", "sy", "lev_in", "lev_out", "t_in", "t_out")}
    while live.size:
        a, b, a1, b1 = lx[live], ly[live], lx1[live], ly1[live]
        mx, my = a != a1, b != b1
        last = ~mx & ~my
        tx = np.where(mx, _cross(gx, g, np.where(a1 > a, a + 1, a), r[live, 0], d[live, 0]), 2.0)
        ty = np.where(my, _cross(gy, g, np.where(b1 > b, b + 1, b), r[live, 1], d[live, 1]), 2.0)
        step_x = mx & (~my | (tx <= ty))
        t = np.where(step_x, tx, ty)
        lev_out = np.where(last, sz_end[live], _level(r[live, 2] + t * d[live, 2], gz, zl))
        t_out = np.where(last, f[live], t)
        sx, sy, li, ti = _signed(a), _signed(b), lev_in[live], t_in[live]
        for k, v in zip(steps, (idx[live], sx, sy, li, lev_out, ti, t_out)):
            steps[k].append(v)
        # the column's rows with a level in the visit's range, for the rays that have no answer yet
        open_ = hit_row[live] == NO_ROW
        if nodes.n and open_.any():
            w = live[open_]
            lo, hi = np.minimum(li, lev_out)[open_], np.maximum(li, lev_out)[open_]
            up = (li <= lev_out)[open_]
            i0 = np.searchsorted(nodes.keys, qr.pack(sx[open_], sy[open_], lo), "left")
            i1 = np.searchsorted(nodes.keys, qr.pack(sx[open_], sy[open_], hi), "right")
            t_hi = np.maximum(ti, t_out)[open_]
            pend = np.flatnonzero(i1 > i0)
            j = 0
            while pend.size:
                pos = np.where(up[pend], i0[pend] + j, i1[pend] - 1 - j)
                rows = nodes.order[pos]
                lvl = (nodes.keys[pos] & 0x3FFFFF) - (1 << 21)
                ww = w[pend]
                counts, rng, d2 = _candidates(nodes, rows, lvl, li[open_][pend], up[pend], ti[open_][pend], t_hi[pend], r[ww], d[ww], L[ww],
                                              (gz, zl), prm)
                hit_row[ww[counts]], hit_range[ww[counts]], hit_d2[ww[counts]] = rows[counts], rng[counts], d2[counts]
                j += 1
                pend = pend[~counts & (i0[pend] + j < i1[pend])]
        lx[live] = np.where(step_x & ~last, a + np.where(a1 > a, 1, -1), a)
        ly[live] = np.where(~step_x & ~last, b + np.where(b1 > b, 1, -1), b)
        lev_in[live] = lev_out
        t_in[live] = t_out
        live = live[~last]
    status = np.full(n, SKIPPED, np.int64)
    status[idx] = np.where(hit_row != NO_ROW, HIT, MISS)
    row = np.full(n, NO_ROW, np.int64)
    rng32 = np.full(n, _NAN32, np.float32)
    d232 = np.full(n, _NAN32, np.float32)
    with np.errstate(over="ignore"):
        row[idx], rng32[idx], d232[idx] = hit_row, hit_range.astype(np.float32), hit_d2.astype(np.float32)
    cat = lambda v, dt: np.concatenate(v) if v else np.zeros(0, dt)
    return dict(status=status, row=row, range=rng32, d2=d232,
                stats={"rays": int(m), "skipped": int(n - m), "hits": int((hit_row != NO_ROW).sum())},
                steps={k: cat(v, np.float64 if k.startswith("t_") else np.int64) for k, v in steps.items()})


def assert_same(got, want, what=""):
    """row exactly, range and d2 bit for bit; got: dict with row (any integer dtype, NO_ROW as -1 or 0xFFFFFFFF), range, d2"""
    if got.get("row") is not None:
        g = np.asarray(got["row"]).astype(np.uint32).view(np.int32).astype(np.int64)
        assert np.array_equal(g, want["row"]), (what, "row", np.flatnonzero(g != want["row"])[:8])
    for k in ("range", "d2"):
        if got.get(k) is not None:
            g, w = np.ascontiguousarray(got[k], np.float32).view(np.uint32), np.ascontiguousarray(want[k], np.float32).view(np.uint32)
            assert np.array_equal(g, w), (what, k, np.flatnonzero(g != w)[:8])
