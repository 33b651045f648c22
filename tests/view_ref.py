"""Plain numpy answers to view gain (include/gndt.h "view gain", gndt_view_gain*), written from the header's text: ray (k, i) runs from
float32(t_k) to the end point the header's fp64 expression gives, is cut at max_range and is handed the columns of the clearing walk
(restated here on its own: the cells of the origin and of the cut point, |dx| + |dy| unit steps between them, each across the lattice
plane the segment meets first, a tie stepping x); the ray stops in the column of the cast's hit (tests/cast_ref.py answers which row a
ray hits; a walk passes a column once, so the hit's column is one step of it).  The columns handed out up to there are SEEN; the sets
are plain Python sets of (sx, sy), the map's columns another; unknown = seen - map, known = seen & map.

trace() walks every ray of a batch once; gain() makes the records of any choice of poses and directions from it (directions by
index, so a permuted or repeated fan costs no second walk).
Shared by the CPU tier (tests/test_view_host.py) and the GPU tier (tests/test_gpu_view.py).  Test infrastructure only."""
import numpy as np

from tests import cast_ref as cf
from tests import query_ref as qr

FIELDS = ("rays", "skipped", "hits", "unknown", "known", "status", "steps", "sum_ux", "sum_uy")
INFO_DTYPE = np.dtype([("rays", np.uint32), ("skipped", np.uint32), ("hits", np.uint32), ("unknown", np.uint32), ("known", np.uint32),
                       ("status", np.uint32), ("steps", np.uint64), ("sum_ux", np.int64), ("sum_uy", np.int64)])
assert INFO_DTYPE.itemsize == 48


def lin(s):
    """the contiguous cell index of a signed index (no 0): c(s) = s > 0 ? s - 1 : s"""
    s = np.asarray(s, np.int64)
    return np.where(s > 0, s - 1, s)


def signed(c):
    c = np.asarray(c, np.int64)
    return np.where(c >= 0, c + 1, c)


def as_poses(poses):
    return np.ascontiguousarray(poses, np.float64).reshape(-1, 12)


def ends(poses, dirs, max_range):
    """-> origins float32 [K, 3], ends float32 [K, N, 3]: e_a = float32(t_a + max_range * ((R_a0 x + R_a1 y) + R_a2 z)), fp64, max_range
    the struct's float widened"""
    T = as_poses(poses).reshape(-1, 3, 4)
    d = np.asarray(dirs, np.float32)[:, :3].astype(np.float64)
    x, y, z = d[None, :, 0], d[None, :, 1], d[None, :, 2]
    R = np.float64(np.float32(max_range))
    with np.errstate(all="ignore"):
        e = np.stack([T[:, a, 3, None] + R * ((T[:, a, 0, None] * x + T[:, a, 1, None] * y) + T[:, a, 2, None] * z) for a in range(3)], 2)
        return T[:, :, 3].astype(np.float32), e.astype(np.float32)


def _cross(o_axis, length, k, r, d):
    """where r + t d meets lattice plane k of an axis: ((o_axis + k * length) - r) / d clamped to [0, 1]"""
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (o_axis + k.astype(np.float64) * length - r) / d
    return np.where(d == 0, 1.0, np.clip(t, 0.0, 1.0))


def _walk(o32, e32, origin_map, grid_len, max_range, z_len):
    """the columns every ray is handed -> ok [n] (not skipped), and ray, sx, sy of every visit, in walk order per ray"""
    n = len(e32)
    ok = qr.keys(o32, origin_map, grid_len, z_len)[4] & qr.keys(e32, origin_map, grid_len, z_len)[4] if n else np.zeros(0, bool)
    idx = np.flatnonzero(ok)
    r = o32[idx].astype(np.float64)
    d = e32[idx].astype(np.float64) - r
    L = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    R = np.float64(np.float32(max_range))
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(L > 0, np.minimum(1.0, R / L), 1.0)
    cut = np.where((f < 1.0)[:, None], (r + d * f[:, None]).astype(np.float32), e32[idx])
    ko, kc = qr.keys(o32[idx], origin_map, grid_len, z_len), qr.keys(cut, origin_map, grid_len, z_len)
    cx, cy, cx1, cy1 = lin(ko[0]), lin(ko[1]), lin(kc[0]), lin(kc[1])
    gx, gy, g = np.float64(np.float32(origin_map[0])), np.float64(np.float32(origin_map[1])), np.float64(np.float32(grid_len))
    out = ([], [], [])
    live = np.arange(len(idx))
    while live.size:
        a, b, a1, b1 = cx[live], cy[live], cx1[live], cy1[live]
        for lst, v in zip(out, (idx[live], signed(a), signed(b))):
            lst.append(v)
        mx, my = a != a1, b != b1
        tx = np.where(mx, _cross(gx, g, np.where(a1 > a, a + 1, a), r[live, 0], d[live, 0]), 2.0)
        ty = np.where(my, _cross(gy, g, np.where(b1 > b, b + 1, b), r[live, 1], d[live, 1]), 2.0)
        step_x = mx & (~my | (tx <= ty))
        step_y = my & ~step_x
        cx[live] = a + np.where(step_x, np.where(a1 > a, 1, -1), 0)
        cy[live] = b + np.where(step_y, np.where(b1 > b, 1, -1), 0)
        live = live[mx | my]
    cat = lambda v: np.concatenate(v) if v else np.zeros(0, np.int64)
    ray, sx, sy = (cat(v) for v in out)
    order = np.argsort(ray, kind="stable")                  # (lock step appended step by step: stable keeps walk order per ray)
    return ok, ray[order], sx[order], sy[order]


def trace(cells, origin_map, grid_len, z_len, poses, dirs, max_range, min_count=0, min_range=0.0):
    """every ray of K poses x N directions walked once -> dict: K, N, pose_ok [K], status / row / range [K, N] (the cast's: cf.SKIPPED /
    MISS / HIT, NO_ROW, float32 bits), start [K * N + 1] and sx, sy: the visits of ray k * N + i are start[r] : start[r + 1], the columns
    it SEES in walk order (cut behind the hit's column); columns: the map's set of (sx, sy)"""
    T = as_poses(poses)
    K, N = len(T), len(dirs)
    o32, e32 = ends(T, dirs, max_range)
    of = np.repeat(o32, N, axis=0)
    ef = e32.reshape(K * N, 3)
    ok, ray, sx, sy = _walk(of, ef, origin_map, grid_len, max_range, z_len)
    c = cf.cast(cells, origin_map, grid_len, z_len, of, ef, mode=cf.VOXEL, min_count=min_count, max_range=max_range, min_range=min_range)
    assert np.array_equal(c["status"] != cf.SKIPPED, ok)
    # the hit's column is one visit of its ray: the visits behind it are not seen
    msx, msy = np.asarray(cells["sx"], np.int64), np.asarray(cells["sy"], np.int64)
    hit = c["status"] == cf.HIT
    hx, hy = np.zeros(K * N, np.int64), np.zeros(K * N, np.int64)
    hx[hit], hy[hit] = msx[c["row"][hit]], msy[c["row"][hit]]
    first = np.searchsorted(ray, np.arange(K * N + 1))
    pos = np.arange(len(ray)) - first[ray]
    at = hit[ray] & (sx == hx[ray]) & (sy == hy[ray])
    stop = np.full(K * N, np.iinfo(np.int64).max, np.int64)
    assert np.array_equal(np.bincount(ray[at], minlength=K * N) > 0, hit) and (np.bincount(ray[at], minlength=K * N) <= 1).all()
    stop[ray[at]] = pos[at]
    keep = pos <= stop[ray]
    ray, sx, sy = ray[keep], sx[keep], sy[keep]
    return dict(K=K, N=N, pose_ok=qr.keys(o32, origin_map, grid_len, z_len)[4] if K else np.zeros(0, bool),
                status=c["status"].reshape(K, N), row=c["row"].reshape(K, N), range=c["range"].reshape(K, N),
                start=np.searchsorted(ray, np.arange(K * N + 1)), sx=sx, sy=sy,
                columns=set(zip(msx.tolist(), msy.tolist())))


def gain(tr, poses=None, dirs=None):
    """the records (a structured array of INFO_DTYPE) of the poses `poses` (indices into the trace, default all) for the fan made of the
    trace's directions `dirs` (indices, default all; an index given m times is a direction given m times)"""
    K, N = tr["K"], tr["N"]
    poses = np.arange(K) if poses is None else np.asarray(poses, np.int64)
    mult = np.bincount(np.arange(N) if dirs is None else np.asarray(dirs, np.int64), minlength=N)
    used = np.flatnonzero(mult)
    out = np.zeros(len(poses), INFO_DTYPE)
    for j, k in enumerate(poses):
        st = tr["status"][k]
        rec = out[j]
        rec["rays"] = int((mult * (st != cf.SKIPPED)).sum())
        rec["skipped"] = int((mult * (st == cf.SKIPPED)).sum())
        rec["hits"] = int((mult * (st == cf.HIT)).sum())
        rec["status"] = 0 if tr["pose_ok"][k] else 1
        a, b = tr["start"][k * N + used], tr["start"][k * N + used + 1]
        rec["steps"] = int((mult[used] * (b - a)).sum())
        # the visits of the pose's rays that are in the fan; equal pairs are folded in numpy first (a fan passes the columns near the
        # sensor thousands of times), the set is made of what is left
        lo, hi = int(tr["start"][k * N]), int(tr["start"][(k + 1) * N])
        in_fan = np.repeat(mult > 0, np.diff(tr["start"][k * N:(k + 1) * N + 1]))
        pair = np.unique(((tr["sx"][lo:hi][in_fan] + (1 << 20)) << 32) | (tr["sy"][lo:hi][in_fan] + (1 << 20)))
        seen = set(zip(((pair >> 32) - (1 << 20)).tolist(), ((pair & 0xFFFFFFFF) - (1 << 20)).tolist()))
        unknown = seen - tr["columns"]
        rec["unknown"], rec["known"] = len(unknown), len(seen & tr["columns"])
        c = lambda v: v - 1 if v > 0 else v
        rec["sum_ux"] = sum(c(u[0]) for u in unknown)
        rec["sum_uy"] = sum(c(u[1]) for u in unknown)
    return out


def view_gain(cells, origin_map, grid_len, z_len, poses, dirs, max_range, min_count=0, min_range=0.0):
    """-> (records, trace) of the whole batch"""
    tr = trace(cells, origin_map, grid_len, z_len, poses, dirs, max_range, min_count, min_range)
    return gain(tr), tr


def assert_same(got, want, what=""):
    """two arrays of records, field for field"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for k in FIELDS:
        g, w = got[k].astype(np.int64), want[k].astype(np.int64)
        assert np.array_equal(g, w), (what, k, np.flatnonzero(g != w)[:8], g[g != w][:8], w[g != w][:8])
