"""Plain numpy answers to the point queries of include/gndt.h (gndt_query*), written from the definitions and nothing else: the key is
transMortonXYZ's arithmetic in fp32 (map2D.h:950-976: n = ceil(|p - o| / len), 0 -> 1, sign + iff p > o), a NODE answer is the row
with that key, a NEAREST_SLOPE answer the slope row of the column with the least |mean_z - z| (ties: smaller sz).  Shared by the CPU
tier (tests/test_query_host.py) and the GPU tier (tests/test_gpu_query.py).  Test infrastructure only."""
import numpy as np

NO_ROW = -1
MAX_XY, MAX_Z = 65535, (1 << 21) - 1
FLT_MAX = np.float32(np.finfo(np.float32).max)


def _axis(p, o, length, limit):
    p = np.asarray(p, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.ceil(np.abs(p - np.float32(o)) / np.float32(length))
    ok = c <= np.float32(limit)                       # (NaN compares False)
    n = np.where(ok, c, 0).astype(np.int64)
    n[n == 0] = 1
    return np.where(p > np.float32(o), n, -n), ok


def keys(pts, origin, grid_len, z_len):
    """-> sx, sy, sz, ok_xy, ok_node of every point ([N, 3|4] float32)"""
    pts = np.asarray(pts, np.float32)
    finite = np.isfinite(pts[:, :3]).all(1)
    sx, okx = _axis(pts[:, 0], origin[0], grid_len, MAX_XY)
    sy, oky = _axis(pts[:, 1], origin[1], grid_len, MAX_XY)
    sz, okz = _axis(pts[:, 2], origin[2], z_len, MAX_Z)
    ok_xy = finite & okx & oky
    return sx, sy, sz, ok_xy, ok_xy & okz


def pack(sx, sy, sz):
    sx, sy, sz = (np.asarray(a, np.int64) for a in (sx, sy, sz))
    return ((sx + (1 << 20)) << 43) | ((sy + (1 << 20)) << 22) | (sz + (1 << 21))


def row_ncol(cells):
    """per row: its column's node count on the column's first row, else 0 (a column's rows are adjacent)"""
    sx, sy = np.asarray(cells["sx"]), np.asarray(cells["sy"])
    n = sx.size
    out = np.zeros(n, np.uint32)
    if n == 0:
        return out
    start = np.ones(n, bool)
    start[1:] = (sx[1:] != sx[:-1]) | (sy[1:] != sy[:-1])
    first = np.flatnonzero(start)
    out[first] = np.diff(np.append(first, n)).astype(np.uint32)
    return out


def node_rows(cells, pts, origin, grid_len, z_len):
    sx, sy, sz, _, ok = keys(pts, origin, grid_len, z_len)
    mk = pack(cells["sx"], cells["sy"], cells["sz"])
    if mk.size == 0:
        return np.full(len(sx), NO_ROW, np.int64)
    order = np.argsort(mk, kind="stable")
    smk = mk[order]
    q = pack(sx, sy, sz)
    pos = np.minimum(np.searchsorted(smk, q), smk.size - 1)
    return np.where(ok & (smk[pos] == q), order[pos], NO_ROW).astype(np.int64)


def nearest_slope_rows(cells, pts, origin, grid_len, z_len):
    pts = np.asarray(pts, np.float32)
    sx, sy, _, ok, _ = keys(pts, origin, grid_len, z_len)
    slope = np.flatnonzero(np.asarray(cells["flags"]) & 2)
    out = np.full(pts.shape[0], NO_ROW, np.int64)
    if slope.size == 0:
        return out
    ck = pack(np.asarray(cells["sx"])[slope], np.asarray(cells["sy"])[slope], 0)
    order = np.argsort(ck, kind="stable")
    rows, ck = slope[order], ck[order]
    q = pack(sx, sy, 0)
    lo, hi = np.searchsorted(ck, q, "left"), np.searchsorted(ck, q, "right")
    mz = np.asarray(cells["mean"], np.float32)[:, 2]
    sz = np.asarray(cells["sz"])
    best_d = np.full(pts.shape[0], np.inf, np.float32)
    best_sz = np.zeros(pts.shape[0], np.int64)
    for k in range(int((hi - lo).max()) if q.size else 0):
        live = ok & (lo + k < hi)
        r = rows[np.minimum(lo + k, rows.size - 1)]
        with np.errstate(invalid="ignore", over="ignore"):
            d = np.abs(mz[r] - pts[:, 2])
        take = live & ((out == NO_ROW) | (d < best_d) | ((d == best_d) & (sz[r] < best_sz)))
        out[take], best_d[take], best_sz[take] = r[take], d[take], sz[r][take]
    return out


def face_lattice(origin=(0.35, -1.65, 0.2), grid_len=0.5, z_len=0.25, k=4, kz=3, repeat=3):
    """A cloud (point 0 = origin) whose points sit exactly on cell faces: origin + i * grid_len, j * z_len for i, j of both signs,
    including -1, 0 and +1 (there is no index 0: both sides of the origin's face key to +-1)."""
    o = np.asarray(origin, np.float32)
    i = np.arange(-k, k + 1, dtype=np.float32)
    j = np.arange(-kz, kz + 1, dtype=np.float32)
    X, Y, Z = np.meshgrid(o[0] + i * np.float32(grid_len), o[1] + i * np.float32(grid_len), o[2] + j * np.float32(z_len), indexing="ij")
    pts = np.stack([X.ravel(), Y.ravel(), Z.ravel()], 1).astype(np.float32)
    pts = np.repeat(pts, repeat, axis=0)
    return np.concatenate([o[None, :], pts]).astype(np.float32)


def odd_points(origin, grid_len, z_len, extent, seed=7):
    """Points without an answer or at the codec's edges: off the map, NaN, +-Inf in each coordinate, |nx| / |ny| beyond 65535, |nz|
    at and beyond 2^21 - 1"""
    o = np.asarray(origin, np.float32)
    rng = np.random.default_rng(seed)
    lo, hi = extent
    pts = [rng.uniform(lo - 5 * (hi - lo), hi + 5 * (hi - lo), size=(64, 3)).astype(np.float32)]
    bad = np.tile(o, (12, 1))
    for a in range(3):
        bad[4 * a, a], bad[4 * a + 1, a], bad[4 * a + 2, a], bad[4 * a + 3, a] = np.nan, np.inf, -np.inf, np.float32(1e38)
    pts.append(bad)
    g, z = np.float32(grid_len), np.float32(z_len)
    edge = []
    for s in (1, -1):
        edge.append([o[0] + s * 65535 * g, o[1], o[2]])           # largest index: keyed
        edge.append([o[0] + s * 65536.5 * g, o[1], o[2]])         # beyond: no key
        edge.append([o[0], o[1] + s * 65536.5 * g, o[2]])
        edge.append([o[0], o[1], o[2] + s * np.float32(2 ** 21 + 10) * z])   # |nz| beyond the range: NODE no, NEAREST_SLOPE yes
        edge.append([o[0], o[1], o[2] + s * np.float32(2 ** 20) * z])
    pts.append(np.asarray(edge, np.float32))
    return np.concatenate(pts).astype(np.float32)
