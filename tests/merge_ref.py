"""Plain numpy restatement of the map merge (include/gndt.h "map merge", grid_ndt_amd/csrc/gndt_merge.hpp), written from the definition:
steps 1 to 7 for every source node in the evaluation order the header states (bit for bit: IEEE double operations, one at a time; the
codec's key in IEEE float32 operations), and step 8 over a list of node statistics (`merge`).  Shared by the CPU tier
(tests/test_merge_host.py) and the GPU tier (tests/test_gpu_merge.py).  Test infrastructure only.

The tolerance of a destination sum (derived, not tuned), u = 2^-53.  A destination sum is the sum of j values: the node's prior value,
if it had one, and one addend per source node that lands in it.
  (a) The order of the adds is not fixed (floating-point atomics): j u times the sum of the absolute values of the j values.
  (b) Each addend carries the rounding of steps 1 to 7.  With A_i = sum_j |R_ij| |m_j| + |t_i| (the absolute chain of step 3),
      Sabs_ab = |s2_ab| + |s1_a mu_b|, Wabs_ib = sum_k |R_ik| Sabs_kb, S'abs_ij = sum_k Wabs_ik |R_jk|, to first order in u:
        mu: 1 rounding, m: 1 more                      -> m'_i within 6 u A_i (3 products, 3 sums, the error of m times |R|)
        u_a = m'_a - c'_a                              -> within 6 u A_a + u |u_a|;   nu_a = n u_a within n u (6 A_a + 2 |u_a|)
        S_ab: 2 roundings in the product, 1 in the sum -> within 3 u Sabs_ab;   W_ib within 6 u Wabs_ib;   S'_ij within 9 u S'abs_ij
        nu_i u_j                                       -> within n u (6 (|u_i| A_j + |u_j| A_i) + 4 |u_i u_j|)
      out[a]    within n u (6 A_a + 2 |u_a|)
      out[3+ij] within u (10 S'abs_ij + n (6 (|u_i| A_j + |u_j| A_i) + 5 |u_i u_j|))          (the last add: u |out|)
      The centres c and c' are data (axis_centre, the same bits on both ways).
  (c) Where the merged map is compared with a BUILD of the moved points (`abs_sums` given: the sums of the absolute values of the
      source's terms), the source's sums carry their own accumulation, (m_c + 2) u of their share of T, and the build of the m moved
      points (m + 2) u T, with T the absolute chain of the real-arithmetic identity v' = R v + d, d = R c + t - c':
        T_a  = sum_j |R_aj| abs_s1_j + n |d_a|
        T_ab = sum_jk |R_aj| |R_bk| abs_s2_jk + |d_a| sum_k |R_bk| abs_s1_k + |d_b| sum_j |R_aj| abs_s1_j + n |d_a d_b|
      together (2 m + 8) u T, as tests/coarsen_ref.py counts its own.
  (d) Where the moved points were rounded to float32 before that build (`moved_cloud_bound`), each coordinate moved by at most half an
      ulp, e_a = 2^-24 |q_a| (the format's precision): sum v'_a changes by at most sum e_a, sum v'_a v'_b by at most
      sum (|v'_a| e_b + |v'_b| e_a + e_a e_b)."""
import numpy as np

from tests.coarsen_ref import centre, pack
from tests.host_emulation import unpack

U = 2.0 ** -53
MAX_XY, MAX_Z = 65535, (1 << 21) - 1
_PAIRS = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
_SYM = np.array([[0, 1, 2], [1, 3, 4], [2, 4, 5]])


def axis_index(p, o, length, limit):
    """gndt_math.hpp axis_index in IEEE float32: ((int)ceil(|p - o| / len), 0 -> 1, signed by p > o) and whether it is in range"""
    p = np.asarray(p, np.float32)
    o, length = np.float32(o), np.float32(length)
    with np.errstate(all="ignore"):
        c = np.ceil(np.abs(p - o) / length)
        ok = c <= np.float32(limit)
        n = np.where(ok, c, np.float32(limit)).astype(np.int64)
    n[n == 0] = 1
    return np.where(p > o, n, -n), ok


def point_keys(pf, origin, grid_len, z_len):
    """[n, 3] float32 -> (packed keys, ok)"""
    sx, okx = axis_index(pf[:, 0], origin[0], grid_len, MAX_XY)
    sy, oky = axis_index(pf[:, 1], origin[1], grid_len, MAX_XY)
    sz, okz = axis_index(pf[:, 2], origin[2], z_len, MAX_Z)
    return pack(sx, sy, sz), okx & oky & okz, (sx, sy, sz)


def as_pose(pose):
    T = np.eye(4)[:3] if pose is None else np.asarray(pose, np.float64).reshape(-1, 4)[:3]
    return np.ascontiguousarray(T[:, :3]), np.ascontiguousarray(T[:, 3])


def merge_nodes(key, count, sums, pose, src_geo, dst_geo, bounds=False, abs_sums=None):
    """Steps 1 to 7 for every node.  src_geo / dst_geo: (origin[3], grid_len, z_len).  -> (destination keys, ok, out [n, 9]); with
    bounds also the per-addend bound (b) [n, 9] (and, with abs_sums, (c)'s T [n, 9]).  Rows with ok False hold no key."""
    R, t = as_pose(pose)
    key = np.asarray(key).astype(np.uint64)
    s = np.asarray(sums, np.float64)
    dn = np.asarray(count).astype(np.uint32).astype(np.float64)
    (so, sgl, szl), (do, dgl, dzl) = src_geo, dst_geo
    sx, sy, sz = unpack(key)
    c = np.stack([centre(sx, so[0], sgl), centre(sy, so[1], sgl), centre(sz, so[2], szl)], 1)
    with np.errstate(all="ignore"):
        mu = s[:, :3] / dn[:, None]
        m = c + mu
        S = np.empty((len(key), 3, 3))
        for k, (a, b) in enumerate(_PAIRS, start=3):
            p = s[:, a] * mu[:, b]
            S[:, a, b] = S[:, b, a] = s[:, k] - p
        mp = np.empty((len(key), 3))
        for i in range(3):
            p0, p1, p2 = R[i, 0] * m[:, 0], R[i, 1] * m[:, 1], R[i, 2] * m[:, 2]
            mp[:, i] = ((p0 + p1) + p2) + t[i]
        mf = mp.astype(np.float32)
        ok = np.isfinite(mf).all(1)
        dkey, in_range, (dx, dy, dz) = point_keys(mf, do, dgl, dzl)
        ok &= in_range
        W = np.empty((len(key), 3, 3))
        for i in range(3):
            for b in range(3):
                p0, p1, p2 = R[i, 0] * S[:, 0, b], R[i, 1] * S[:, 1, b], R[i, 2] * S[:, 2, b]
                W[:, i, b] = (p0 + p1) + p2
        cd = np.stack([centre(dx, do[0], dgl), centre(dy, do[1], dgl), centre(dz, do[2], dzl)], 1)
        u = mp - cd
        nu = dn[:, None] * u
        out = np.empty((len(key), 9))
        out[:, :3] = nu
        for k, (i, j) in enumerate(_PAIRS, start=3):
            p0, p1, p2 = W[:, i, 0] * R[j, 0], W[:, i, 1] * R[j, 1], W[:, i, 2] * R[j, 2]
            Sp = (p0 + p1) + p2
            q = nu[:, i] * u[:, j]
            out[:, k] = Sp + q
        if not bounds:
            return dkey, ok, out
        aR = np.abs(R)
        A = np.abs(m) @ aR.T + np.abs(t)
        Sabs = np.empty_like(S)
        for k, (a, b) in enumerate(_PAIRS, start=3):
            Sabs[:, a, b] = Sabs[:, b, a] = np.abs(s[:, k]) + np.abs(s[:, a] * mu[:, b])
        Spabs = np.einsum("ik,nkl,jl->nij", aR, Sabs, aR)
        au = np.abs(u)
        tol = np.empty_like(out)
        tol[:, :3] = dn[:, None] * U * (6 * A + 2 * au)
        for k, (i, j) in enumerate(_PAIRS, start=3):
            tol[:, k] = U * (10 * Spabs[:, i, j] + dn * (6 * (au[:, i] * A[:, j] + au[:, j] * A[:, i]) + 5 * au[:, i] * au[:, j]))
        T = None
        if abs_sums is not None:
            ab = np.asarray(abs_sums, np.float64)
            d = np.abs(c @ R.T + t - cd)
            r1 = ab[:, :3] @ aR.T                                # sum_j |R_aj| abs_s1_j
            s2 = ab[:, 3:][:, _SYM]                              # [n, 3, 3]
            r2 = np.einsum("ik,nkl,jl->nij", aR, s2, aR)
            T = np.empty_like(out)
            T[:, :3] = r1 + dn[:, None] * d
            for k, (a, b) in enumerate(_PAIRS, start=3):
                T[:, k] = r2[:, a, b] + d[:, a] * r1[:, b] + d[:, b] * r1[:, a] + dn * d[:, a] * d[:, b]
    return dkey, ok, out, tol, T


def merge(src, pose, src_geo, dst_geo, prior=None, min_count=0, base=0, abs_sums=None):
    """Step 8.  src / prior: dicts of key, count, first_idx, sums (any order; prior = what the destination holds, None = empty).
    -> dict(key sorted, count, first_idx, sums, tol [n, 9], addends [n], stats): tol = (a) + (b) (+ (c) with abs_sums)."""
    key = np.asarray(src["key"]).astype(np.uint64)
    count = np.asarray(src["count"]).astype(np.int64) & 0xFFFFFFFF
    first = np.asarray(src["first_idx"]).astype(np.int64) & 0xFFFFFFFF
    sums = np.asarray(src["sums"], np.float64)
    live = count > 0
    take = live & (count >= max(int(min_count), 1))
    dkey, ok, out, tol, T = merge_nodes(key, np.maximum(count, 1), sums, pose, src_geo, dst_geo, bounds=True,
                                         abs_sums=np.abs(sums) if abs_sums is None else abs_sums)
    go = take & ok
    stats = {"source_nodes": int(live.sum()), "below_min_count": int((live & ~take).sum()), "skipped": int((take & ~ok).sum()),
             "merged_nodes": int(go.sum()), "merged_points": int(count[go].sum())}
    pk = np.zeros(0, np.uint64) if prior is None else np.asarray(prior["key"]).astype(np.uint64)
    pcount = np.zeros(0, np.int64) if prior is None else np.asarray(prior["count"]).astype(np.int64) & 0xFFFFFFFF
    pfirst = np.zeros(0, np.int64) if prior is None else np.asarray(prior["first_idx"]).astype(np.int64) & 0xFFFFFFFF
    psums = np.zeros((0, 9)) if prior is None else np.asarray(prior["sums"], np.float64)
    plive = pcount > 0
    all_key = np.concatenate([pk[plive], dkey[go]])
    uk, inv = np.unique(all_key, return_inverse=True)
    vals = np.concatenate([psums[plive], out[go]])
    o_sums = np.zeros((uk.size, 9))
    o_abs = np.zeros((uk.size, 9))
    o_tol = np.zeros((uk.size, 9))
    np.add.at(o_sums, inv, vals)
    np.add.at(o_abs, inv, np.abs(vals))
    np.add.at(o_tol, inv, np.concatenate([np.zeros_like(psums[plive]), tol[go]]))
    j = np.bincount(inv, minlength=uk.size).astype(np.int64)
    o_tol += j[:, None] * U * o_abs
    o_count = np.bincount(inv, weights=np.concatenate([pcount[plive], count[go]]), minlength=uk.size).astype(np.int64)
    if abs_sums is not None:
        o_T = np.zeros((uk.size, 9))
        np.add.at(o_T, inv, np.concatenate([np.abs(psums[plive]), T[go]]))
        o_tol += (2 * o_count + 8)[:, None] * U * o_T
    o_first = np.full(uk.size, np.iinfo(np.int64).max, np.int64)
    np.minimum.at(o_first, inv, np.concatenate([pfirst[plive], int(base) + first[go]]))
    stats["new_nodes"] = int(uk.size - np.unique(pk[plive]).size)
    return {"key": uk, "count": o_count.astype(np.uint32), "first_idx": o_first.astype(np.uint32), "sums": o_sums, "tol": o_tol,
            "addends": j, "stats": stats}


def moved_cloud_bound(q, cen):
    """(d): q [n, 3] float32 points, cen [n, 3] their nodes' centres -> per point [n, 9] what half an ulp of float32 in every coordinate
    moves its nine terms by (to be summed over a node's points)"""
    q = np.asarray(q, np.float32).astype(np.float64)
    e = np.abs(q) * 2.0 ** -24
    v = np.abs(q - cen)
    out = np.empty((len(q), 9))
    out[:, :3] = e
    for k, (a, b) in enumerate(_PAIRS, start=3):
        out[:, k] = v[:, a] * e[:, b] + v[:, b] * e[:, a] + e[:, a] * e[:, b]
    return out
