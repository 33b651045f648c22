"""Plain numpy restatement of map coarsening (include/gndt.h "map pyramids", grid_ndt_amd/csrc/gndt_coarsen.hpp), written from the
definition: the parent of a signed index, the parent of a packed key, a node's centre, and the shift of a node's additive statistics
from its own centre to its parent's in the evaluation order the header states (bit for bit: IEEE double operations, one at a time).
`coarsen` applies it to a list of node statistics and adds the siblings up.  Shared by the CPU tier (tests/test_coarsen_host.py) and
the GPU tier (tests/test_gpu_coarsen.py).  Test infrastructure only.

The tolerance of a parent's nine sums (derived, not tuned).  Two ways to a parent's statistics are compared: (A) the fine nodes'
sums, each shifted to the parent's centre, the siblings added up; (B) the points accumulated about the parent's centre directly.  In
real arithmetic they are equal (v' = v + d for every point).  In fp64, with u = 2^-53, m the parent's points, m_c those of child c, j
the number of children, and T the sum of the absolute values of everything that is added up on way (A) —
    T_a  = sum_c (sum_i |v_a| + m_c |d_a|),    T_ab = sum_c (sum_i |v_a v_b| + |d_a| sum_i |v_b| + |d_b| sum_i |v_a| + m_c |d_a d_b|)
(T of way (B) is no larger: |v'_a v'_b| <= the four absolute products it expands into) — to first order in u:
  (A) a child's fine sum is m_c - 1 additions of terms that carry up to 3 roundings (the two differences p - c, their product):
      (m_c + 2) u of its share of T; the products with d and n carry 2 to 4 roundings more (d = c - c', each product), within the same
      count since they multiply sums that were counted with m_c; the shift is 3 additions, the siblings are j - 1 additions (in any
      order: the device adds them with floating-point atomics), each at most u T.  Together at most (m + j + 4) u T.
  (B) m - 1 additions of terms with up to 3 roundings: (m + 2) u T.
So |A - B| <= (2 m + j + 6) u T.  The additions behind the two values number (m - j) + 3 j + (j - 1) and m - 1, that is 2 m + 3 j - 2;
the tests use K = 2 m + 3 j + 8, which covers both counts, times u T.  Where (A) on the device is compared with (A) here on the SAME
fine sums (the GPU tier, after remove / crop / clear) only the shift and the siblings' order differ; the same bound holds with room,
and T is then formed from the absolute values of the fine sums themselves (`abs_sums` left out)."""
import numpy as np

from tests.host_emulation import unpack

U = 2.0 ** -53


def pack(sx, sy, sz):
    sx, sy, sz = (np.asarray(v, np.int64) for v in (sx, sy, sz))
    return (((sx + (1 << 20)) << 43) | ((sy + (1 << 20)) << 22) | (sz + (1 << 21))).astype(np.uint64)


def parent_index(s, f):
    """sign(s) * ceil(|s| / f) in integers; there is no index 0"""
    s = np.asarray(s, np.int64)
    f = int(f)
    return np.where(s > 0, (s + f - 1) // f, -((-s + f - 1) // f))


def parent_keys(keys, fxy, fz):
    sx, sy, sz = unpack(np.asarray(keys, np.uint64))
    return pack(parent_index(sx, fxy), parent_index(sy, fxy), parent_index(sz, fz))


def coarse_len(length, f):
    """what the destination handle holds: the fp32 product, exact for a power of two"""
    return np.float32(np.float32(f) * np.float32(length))


def centre(s, o, length):
    """axis_centre: (double)o + (s -+ 1/2) * (double)len, o and len fp32"""
    s = np.asarray(s, np.int64)
    half = np.where(s > 0, s.astype(np.float64) - 0.5, s.astype(np.float64) + 0.5)
    return np.float64(np.float32(o)) + half * np.float64(np.float32(length))


def centres(keys, origin, grid_len, z_len):
    sx, sy, sz = unpack(np.asarray(keys, np.uint64))
    return np.stack([centre(sx, origin[0], grid_len), centre(sy, origin[1], grid_len), centre(sz, origin[2], z_len)], 1)


def delta(keys, fxy, fz, origin, grid_len, z_len):
    """[n, 3]: the child's centre minus its parent's, the parent's at the multiplied lengths"""
    c = centres(keys, origin, grid_len, z_len)
    cp = centres(parent_keys(keys, fxy, fz), origin, coarse_len(grid_len, fxy), coarse_len(z_len, fz))
    return c - cp


_PAIRS = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]


def shift(count, sums, d, absolute=False):
    """coarsen_sums for every node, in the header's order; absolute=True: the same chain of absolute values (`sums` then holds the sums
    of the absolute values of the fine terms)"""
    n = np.asarray(count).astype(np.float64)
    s = np.asarray(sums, np.float64)
    d = np.abs(d) if absolute else np.asarray(d, np.float64)
    nd = n[:, None] * d
    out = np.empty_like(s)
    for a in range(3):
        out[:, a] = s[:, a] + nd[:, a]
    for k, (a, b) in enumerate(_PAIRS, start=3):
        p1 = d[:, a] * s[:, b]
        p2 = d[:, b] * s[:, a]
        p3 = nd[:, a] * d[:, b]
        out[:, k] = ((s[:, k] + p1) + p2) + p3
    return out


def coarsen(key, count, first_idx, sums, fxy, fz, origin, grid_len, z_len, abs_sums=None):
    """node statistics (any order; nodes without points are skipped, as k_coarsen skips them) -> the parents' statistics sorted by key:
    dict(key, count, first_idx, sums, children, tol) with tol [n, 9] the bound of the module's docstring"""
    key = np.asarray(key).astype(np.uint64)
    count = np.asarray(count).astype(np.int64)
    live = count > 0
    key, count = key[live], count[live]
    first_idx = np.asarray(first_idx).astype(np.int64)[live] & 0xFFFFFFFF
    sums = np.asarray(sums, np.float64)[live]
    abs_sums = np.abs(sums) if abs_sums is None else np.asarray(abs_sums, np.float64)[live]
    d = delta(key, fxy, fz, origin, grid_len, z_len)
    q = shift(count, sums, d)
    t = shift(count, abs_sums, d, absolute=True)
    pk, inv = np.unique(parent_keys(key, fxy, fz), return_inverse=True)
    out_sums = np.zeros((pk.size, 9))
    out_abs = np.zeros((pk.size, 9))
    np.add.at(out_sums, inv, q)
    np.add.at(out_abs, inv, t)
    out_count = np.bincount(inv, weights=count, minlength=pk.size).astype(np.int64)
    children = np.bincount(inv, minlength=pk.size).astype(np.int64)
    out_first = np.full(pk.size, np.iinfo(np.int64).max, np.int64)
    np.minimum.at(out_first, inv, first_idx)
    K = 2 * out_count + 3 * children + 8
    return {"key": pk, "count": out_count.astype(np.uint32), "first_idx": out_first.astype(np.uint32), "sums": out_sums,
            "children": children, "tol": K[:, None] * U * out_abs}
