"""What the CPU tier (tests/test_footprint_host.py) and the GPU tier (tests/test_gpu_footprint.py) of the footprint poses share: the
shim's loader and runner (tests/footprint_shim.cpp: the kernel's per-pose code lane after lane), the hand-made clouds whose answer is
known beforehand, and pose batches.  Test infrastructure only."""
import ctypes as C

import numpy as np

from tests import footprint_ref as fr
from tests import query_ref as qr
from tests.host_emulation import MAP, MapRows, load_shim

SENTINEL = 0xDEADBEEF
_shim = None


def shim():
    global _shim
    if _shim is None:
        vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
        _shim = load_shim("footprint_shim.cpp", "_footprint_shim.so",
                          {"fshim_footprints": ([vp, vp, vp, vp, MAP, vp, u64, u64, vp, u32, vp], C.c_int)})
    return _shim


def strided(poses, stride):
    """[K, 5] float32 -> bytes with a pose's five floats every `stride` bytes, the gaps filled with a float that would be noticed"""
    poses = np.ascontiguousarray(poses, np.float32)
    buf = np.full((max(len(poses), 1), stride // 4), 7.0e8, np.float32)
    buf[:len(poses), :5] = poses[:, :5]
    return buf


def run(t, poses, half_length, half_width, robot=None, max_dz=0.0, height=0.0, min_cells=0, min_cover=0.0, weight=fr.CELL, row_cap=0, stride=20,
        **grid):
    """the shim's poses on the rows of t (a MapRows) -> (info, rows); grid: origin / grid_len / z_len of a map made without them"""
    rb = dict(fr.ROBOT)
    rb.update(robot or {})
    grid_len = grid.get("grid_len", t.P.get("grid_len"))
    r4 = np.array([rb["radius"], rb["reachable_height"], rb["max_rough"], rb["max_angle_deg"]], np.float32)
    rule = fr.rule(half_length, half_width, rb, min_cover)
    frule = np.array([max_dz, height], np.float32)
    urule = np.array([min_cells or 3, weight, fr.box_n(half_length, half_width, grid_len)], np.uint32)
    assert urule[2] <= fr.MAX_N
    K = len(poses)
    buf = strided(poses, stride)
    info = np.zeros(max(K, 1), fr.INFO_DTYPE)
    info.view(np.uint32)[:] = SENTINEL
    rows = np.full((K, row_cap), SENTINEL, np.uint32)
    p = lambda a: a.ctypes.data if a is not None and a.size else None
    rc = shim().fshim_footprints(p(r4), p(rule), p(frule), p(urule), t.shim_map(**grid), p(buf), K, stride, p(rows), row_cap, p(info))
    assert rc == 0
    return info[:K], rows


def map_rows(cells, origin, P):
    """the rows of an export (the library's, the oracle's) with the column index derived on the host"""
    return MapRows(cells, qr.row_ncol(cells), origin=origin, P=P)


# ---- clouds whose answer is known beforehand: [origin; points] float32, built with PLANE_P ----
PLANE_P = dict(grid_len=0.5, z_len=0.25, slope_interval=0.08, demand="slope")


def _grid_points(lo, hi, per_cell, g=0.5):
    n = int(round((hi - lo) / g)) * per_cell
    a = lo + (np.arange(n) + 0.5) * ((hi - lo) / n)
    X, Y = np.meshgrid(a, a, indexing="ij")
    return X.ravel(), Y.ravel()


def plane_cloud(a, b, noise=0.0, lo=-4.0, hi=4.0, per_cell=5, seed=3, origin=(0.013, -0.021, -2.0)):
    """a surface z = a x + b y sampled per_cell^2 times a column, with optional noise in z"""
    X, Y = _grid_points(lo, hi, per_cell)
    Z = a * X + b * Y
    if noise:
        Z = Z + np.random.default_rng(seed).normal(0.0, noise, Z.shape)
    return np.concatenate([np.array([origin]), np.stack([X, Y, Z], 1)]).astype(np.float32)


def kerb_cloud(k, lo=-4.0, hi=4.0, per_cell=5, origin=(0.0, 0.0, -2.0)):
    """flat ground at z = 0.05 for x < 0 and at 0.05 + k for x > 0"""
    X, Y = _grid_points(lo, hi, per_cell)
    Z = np.where(X < 0, 0.05, 0.05 + k)
    return np.concatenate([np.array([origin]), np.stack([X, Y, Z], 1)]).astype(np.float32)


def headed(xyz, yaw):
    """[K, 3] points and yaws -> [K, 5] poses (the vector's length varies with the pose)"""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    yaw = np.broadcast_to(np.asarray(yaw, np.float64), (len(xyz),))
    r = 0.5 + np.arange(len(xyz)) % 3
    return np.concatenate([xyz, (r * np.cos(yaw))[:, None], (r * np.sin(yaw))[:, None]], 1).astype(np.float32)


def random_poses(rng, K, lo, hi, z_lo, z_hi, on=None):
    """K poses over (and a little outside) the rectangle lo..hi, every other one at one of the points `on`, random headings"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    pad = 0.05 * (hi - lo)
    xyz = np.concatenate([rng.uniform(lo - pad, hi + pad, (K, 2)), rng.uniform(z_lo, z_hi, (K, 1))], 1)
    if on is not None and len(on):
        xyz[::2] = on[rng.integers(0, len(on), len(xyz[::2]))]
    return headed(xyz, rng.uniform(-np.pi, np.pi, K))


def mixed_batch(t, rng, n_ok=6):
    """poses of every status on the rows t: ok ones on slopes' means, a non-finite field, a zero heading, one far off the map"""
    slopes = np.flatnonzero(t.flags & 2)
    on = t.mean[slopes[rng.integers(0, len(slopes), n_ok)]].astype(np.float64)
    p = headed(on, rng.uniform(-np.pi, np.pi, n_ok))
    bad = p[:3].copy()
    bad[0, 1] = np.nan
    bad[1, 3:] = 0.0
    bad[2, 4] = np.inf
    far = p[:1].copy()
    far[0, :2] += 1000.0
    return np.concatenate([p[:2], bad[:1], p[2:4], far, bad[1:], p[4:]]).astype(np.float32)
