"""Plain numpy answers to map-to-map scoring (include/gndt.h "map-to-map scoring", gndt_score_maps*), written from the definition and
nothing else.  Which source rows count, the transform of their means, the key and the candidates come from tests/score_ref.py and
tests/query_ref.py (scan scoring's steps 1 to 3); the rotated source covariance, P = Sigma + C_d, eps, the adjugate chain and d2 in
the order the definition states; a pair's 6 + 21 derivative values in the order grid_ndt_amd/csrc/gndt_score_maps.hpp states
(r_a, phi_a / 2, B r_a, the second-order part of two rotations); math.fsum over the pairs.  Next to every entry of g and H the
restatement returns the sum of the absolute values of the entry's per-pair contributions.

Also here: the frozen function itself (`frozen_score`: the candidate rows and every pair's eps fixed, q(xi) = Exp(w) q + v and
A(xi) = Exp(w) Sigma Exp(w)^T + C_d + eps I with full matrices and numpy's solver, none of the chain above) for central differences,
and `callables`, the restatement as the two functions grid_ndt_amd.registration.register drives.  Shared by the CPU tier
(tests/test_score_maps_host.py) and the GPU tier (tests/test_gpu_score_maps.py).  Test infrastructure only.

Tolerances (derived, not tuned).  matched and terms are exact: the lookup is integer work on the bit-identical fp32 q.  score and
d2_sum at score_ref.RTOL: P adds one rounding per entry to scan scoring's chain and A keeps the condition number <= 301 (eps is
taken of P's own trace), so score_ref's derivation holds as it stands.  g and H entry-wise within RTOL_D x the sum of the absolute
values of the entry's per-pair contributions: the code under test and this restatement run the same fp64 operations in the same
order on bit-identical inputs (the header fixes the order, products are not fused), so a pair's 27 values differ only through
e = exp(-d2 / 2), ONE factor common to all of them — whatever cancels inside a pair's value (the lever arm q against ub, Sigma ub
against q) cancels identically on both sides and the error of a contribution stays relative to the contribution itself: e's, which
is exp's last bits (2^-52) plus d2 / 2 times d2's relative error (1e-12 by score_ref.RTOL's derivation, from cond(A) <= 301; terms
with d2 > 80 are below 1e-17 of a counted term): 4e-11.  The order of the sums adds n 2^-53 of the absolute sum.  Below 1e-10, so
RTOL_D = 1e-9 stands as in score_derivs_ref, with the same factor of ten in hand and no further factor."""
import math

import numpy as np

from tests import query_ref as qr
from tests import score_derivs_ref as dr
from tests import score_ref as sr

NO_ROW = sr.NO_ROW
RTOL_D = dr.RTOL_D
TRI = dr.TRI
FLAG_HAS_STATS = 1


def defaults(dst_min_points=3, src_min_points=3, **params):
    """the parameters as the library resolves them: min_count 0 = max(both maps' min_points, 3)"""
    return sr.defaults(min_points=max(int(dst_min_points), int(src_min_points)), **params)


class Source:
    """the rows of the source map's export: which of them count, their float64 means and scatters"""

    def __init__(self, cells, prm):
        self.n = int(len(cells["sx"]))
        self.count = np.asarray(cells["count"]).astype(np.int64)[:self.n]
        self.mean = np.asarray(cells["mean"], np.float32).reshape(-1, 3)[:self.n]
        self.cov = np.asarray(cells["cov"], np.float32).astype(np.float64).reshape(-1, 6)[:self.n]
        flags = np.asarray(cells["flags"]).astype(np.int64)[:self.n]
        self.counted = ((flags & FLAG_HAS_STATS) != 0) & (self.count >= prm["min_count"])
        self.idx = np.flatnonzero(self.counted)


def sigma(T, count, cov):
    """Sigma = R C R^T [n, 6] (xx xy xz yy yz zz) of C = S / (c - 1), in the definition's bracketing"""
    T = np.asarray(T, np.float64)[:3]
    with np.errstate(all="ignore"):
        r = 1.0 / (count - 1).astype(np.float64)
        c00, c01, c02, c11, c12, c22 = (cov[:, k] * r for k in range(6))
        C = [[c00, c01, c02], [c01, c11, c12], [c02, c12, c22]]
        W = [[(T[i, 0] * C[0][b] + T[i, 1] * C[1][b]) + T[i, 2] * C[2][b] for b in range(3)] for i in range(3)]
        S = lambda i, j: (W[i][0] * T[j, 0] + W[i][1] * T[j, 1]) + W[i][2] * T[j, 2]
        return np.stack([S(0, 0), S(0, 1), S(0, 2), S(1, 1), S(1, 2), S(2, 2)], 1)


def _pair(nodes, rows, qd, Sg, prm):
    """the destination rows[i] (NO_ROW: none) against the moved source nodes (qd float64 [n, 3], Sg [n, 6]) -> counted (count >=
    min_count), d2, eps and the chain's values ub (3), B (6), det; garbage where not counted"""
    r = np.maximum(rows, 0)
    c = nodes.count[r]
    counted = (rows != NO_ROW) & (c >= prm["min_count"])
    S, m = nodes.cov[r], nodes.mean[r]
    with np.errstate(all="ignore"):
        inv = 1.0 / (np.maximum(c, 2) - 1).astype(np.float64)
        pxx, pxy, pxz, pyy, pyz, pzz = (Sg[:, k] + S[:, k] * inv for k in range(6))
        eps = np.maximum(prm["cov_rel"] * (((pxx + pyy) + pzz) / 3.0), prm["cov_floor"])
        a00, a11, a22, a01, a02, a12 = pxx + eps, pyy + eps, pzz + eps, pxy, pxz, pyz
        c00, c01, c02 = a11 * a22 - a12 * a12, a02 * a12 - a01 * a22, a01 * a12 - a02 * a11
        c11, c12, c22 = a00 * a22 - a02 * a02, a01 * a02 - a00 * a12, a00 * a11 - a01 * a01
        det = (a00 * c00 + a01 * c01) + a02 * c02
        dx, dy, dz = qd[:, 0] - m[:, 0], qd[:, 1] - m[:, 1], qd[:, 2] - m[:, 2]
        ux = (c00 * dx + c01 * dy) + c02 * dz
        uy = (c01 * dx + c11 * dy) + c12 * dz
        uz = (c02 * dx + c12 * dy) + c22 * dz
        d2 = ((dx * ux + dy * uy) + dz * uz) / det
        rd = 1.0 / det
        ub = [ux * rd, uy * rd, uz * rd]
        B = [c00 * rd, c01 * rd, c02 * rd, c11 * rd, c12 * rd, c22 * rd]
    return dict(counted=counted, d2=d2, eps=eps, ub=ub, B=B)


def _values(qd, Sg, p, e):
    """a pair's 27 values [n, 27] in the order gndt_score_maps.hpp states"""
    qx, qy, qz = qd[:, 0], qd[:, 1], qd[:, 2]
    s00, s01, s02, s11, s12, s22 = (Sg[:, k] for k in range(6))
    ux, uy, uz = p["ub"]
    b00, b01, b02, b11, b12, b22 = p["B"]
    with np.errstate(all="ignore"):
        zx = qx - ((s00 * ux + s01 * uy) + s02 * uz)
        zy = qy - ((s01 * ux + s11 * uy) + s12 * uz)
        zz = qz - ((s02 * ux + s12 * uy) + s22 * uz)
        t00, t01, t02 = s02 * uy - s01 * uz, s12 * uy - s11 * uz, s22 * uy - s12 * uz
        t10, t11, t12 = s00 * uz - s02 * ux, s01 * uz - s12 * ux, s02 * uz - s22 * ux
        t20, t21, t22 = s01 * ux - s00 * uy, s11 * ux - s01 * uy, s12 * ux - s02 * uy
        r0 = (t00, t01 - zz, t02 + zy)
        r1 = (t10 + zz, t11, t12 - zx)
        r2 = (t20 - zy, t21 + zx, t22)
        f = [ux, uy, uz,
             0.5 * ((ux * r0[0] + uy * (r0[1] - qz)) + uz * (r0[2] + qy)),
             0.5 * ((ux * (r1[0] + qz) + uy * r1[1]) + uz * (r1[2] - qx)),
             0.5 * ((ux * (r2[0] - qy) + uy * (r2[1] + qx)) + uz * r2[2])]
        Bv = lambda r: ((b00 * r[0] + b01 * r[1]) + b02 * r[2], (b01 * r[0] + b11 * r[1]) + b12 * r[2], (b02 * r[0] + b12 * r[1]) + b22 * r[2])
        v0, v1, v2 = Bv(r0), Bv(r1), Bv(r2)
        dot = lambda a, b: (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]
        uzs = (ux * zx + uy * zy) + uz * zz
        x00 = (ux * zx - uzs) - (uy * t02 - uz * t01)
        x01 = 0.5 * (ux * zy + uy * zx) - (uy * t12 - uz * t11)
        x02 = 0.5 * (ux * zz + uz * zx) - (uy * t22 - uz * t21)
        x11 = (uy * zy - uzs) - (uz * t10 - ux * t12)
        x12 = 0.5 * (uy * zz + uz * zy) - (uz * t20 - ux * t22)
        x22 = (uz * zz - uzs) - (ux * t21 - uy * t20)
        o = [-(e * f[a]) for a in range(6)]
        o += [e * (f[0] * f[0] - b00), e * (f[0] * f[1] - b01), e * (f[0] * f[2] - b02),
              e * (f[0] * f[3] - v0[0]), e * (f[0] * f[4] - v1[0]), e * (f[0] * f[5] - v2[0]),
              e * (f[1] * f[1] - b11), e * (f[1] * f[2] - b12),
              e * (f[1] * f[3] - v0[1]), e * (f[1] * f[4] - v1[1]), e * (f[1] * f[5] - v2[1]),
              e * (f[2] * f[2] - b22),
              e * (f[2] * f[3] - v0[2]), e * (f[2] * f[4] - v1[2]), e * (f[2] * f[5] - v2[2]),
              e * ((f[3] * f[3] - dot(r0, v0)) - x00), e * ((f[3] * f[4] - dot(r0, v1)) - x01), e * ((f[3] * f[5] - dot(r0, v2)) - x02),
              e * ((f[4] * f[4] - dot(r1, v1)) - x11), e * ((f[4] * f[5] - dot(r1, v2)) - x12),
              e * ((f[5] * f[5] - dot(r2, v2)) - x22)]
    return np.stack(o, 1)


def score_pose(nodes, origin, grid_len, z_len, src, T, nbh, prm, derivs=False):
    """one pose -> dict(score, d2_sum, matched, terms; per source row d2 [src.n] float64 (inf: no term, NaN: the row does not count)
    and row; for the counted rows (src.idx) q [m, 3] float32, Sg [m, 6], rows / all_d2 / raw_d2 / eps [m, nbh] (NO_ROW / inf: the
    candidate does not count); with derivs g, H, g_abs, H_abs and vals [m, nbh, 27])"""
    q = sr.transform(T, src.mean[src.idx])
    qd = q.astype(np.float64)
    Sg = sigma(T, src.count[src.idx], src.cov[src.idx])
    sx, sy, sz, _, ok = qr.keys(q, origin, grid_len, z_len)
    m = len(q)
    R = np.full((m, nbh), NO_ROW, np.int64)
    D = np.full((m, nbh), np.inf)
    raw = np.full((m, nbh), np.inf)
    E = np.zeros((m, nbh))
    V = np.zeros((m, nbh, 27))
    for j, (kx, ky, kz, kok) in enumerate(sr.candidate_keys(sx, sy, sz, ok, nbh)):
        rows = nodes.rows(kx, ky, kz, kok)
        if nodes.n == 0:
            continue
        p = _pair(nodes, rows, qd, Sg, prm)
        valid = p["counted"]
        raw[:, j] = np.where(valid, p["d2"], np.inf)
        if prm["max_d2"] > 0.0:
            valid = valid & ~(p["d2"] > prm["max_d2"])
        R[:, j] = np.where(valid, rows, NO_ROW)
        D[:, j] = np.where(valid, p["d2"], np.inf)
        E[:, j] = np.where(valid, p["eps"], 0.0)
        if derivs:
            with np.errstate(all="ignore"):
                e = np.exp(-0.5 * p["d2"])
            V[:, j] = np.where(valid[:, None], _values(qd, Sg, p, e), 0.0)
    valid = R != NO_ROW
    terms = D[valid]
    best = np.full(m, np.inf)
    brow = np.full(m, NO_ROW, np.int64)
    for j in range(nbh):
        take = valid[:, j] & ((D[:, j] < best) | ((D[:, j] == best) & (R[:, j] < brow)))
        best[take], brow[take] = D[take, j], R[take, j]
    d2 = np.full(src.n, np.nan)
    row = np.full(src.n, NO_ROW, np.int64)
    d2[src.idx], row[src.idx] = best, brow
    out = dict(score=math.fsum(np.exp(-0.5 * terms).tolist()), d2_sum=math.fsum(terms.tolist()), terms=int(valid.sum()),
               matched=int(valid.any(1).sum()), d2=d2, row=row, q=q, Sg=Sg, rows=R, all_d2=D, raw_d2=raw, eps=E)
    if derivs:
        flat = V[valid]                                                 # (the pairs: everything else is exactly 0)
        tot = np.array([math.fsum(flat[:, k].tolist()) for k in range(27)])
        tab = np.array([math.fsum(np.abs(flat[:, k]).tolist()) for k in range(27)])
        out.update(g=tot[:6], H=dr._full(tot[6:]), g_abs=tab[:6], H_abs=dr._full(tab[6:]), vals=V)
    return out


def _run(dst_cells, origin, grid_len, z_len, src_cells, poses, nbh, derivs, dst_min_points, src_min_points, params):
    prm = defaults(dst_min_points, src_min_points, **params)
    nodes = sr.Nodes(dst_cells)
    src = Source(src_cells, prm)
    per = [score_pose(nodes, origin, grid_len, z_len, src, T, nbh, prm, derivs) for T in sr.as_poses(poses)]
    names = ("score", "d2_sum", "matched", "terms") + (("g", "H", "g_abs", "H_abs") if derivs else ())
    out = {k: np.array([p[k] for p in per], np.int64 if k in ("matched", "terms") else np.float64) for k in names}
    out["poses_out"] = per
    out["nodes"], out["source"], out["prm"] = nodes, src, prm
    return out


def score(dst_cells, origin, grid_len, z_len, src_cells, poses, nbh=sr.DIRECT1, per_node=None, dst_min_points=3, src_min_points=3, **params):
    """every pose -> dict of length-K arrays score, d2_sum, matched, terms; with per_node=k also d2 (float64) and row of pose k"""
    out = _run(dst_cells, origin, grid_len, z_len, src_cells, poses, nbh, False, dst_min_points, src_min_points, params)
    if per_node is not None:
        out.update(d2=out["poses_out"][per_node]["d2"], row=out["poses_out"][per_node]["row"])
    return out


def derivs(dst_cells, origin, grid_len, z_len, src_cells, poses, nbh=sr.DIRECT1, dst_min_points=3, src_min_points=3, **params):
    """every pose -> score's arrays and g, g_abs [K, 6], H, H_abs [K, 6, 6]"""
    return _run(dst_cells, origin, grid_len, z_len, src_cells, poses, nbh, True, dst_min_points, src_min_points, params)


def _sym(v6):
    """[n, 6] -> [n, 3, 3]"""
    i = np.array([[0, 1, 2], [1, 3, 4], [2, 4, 5]])
    return v6[:, i]


def frozen_score(nodes, per, xi):
    """the frozen sum at the perturbation xi: the pairs of the per-pose dict `per` and their eps fixed, q(xi) = Exp(w) q + v and
    A(xi) = Exp(w) Sigma Exp(w)^T + C_d + eps I, float64, numpy's solver"""
    xi = np.asarray(xi, np.float64)
    Ex = dr.so3_exp(xi[3:])
    q = per["q"].astype(np.float64) @ Ex.T + xi[:3]
    Sg = Ex @ _sym(per["Sg"]) @ Ex.T
    terms = []
    for j in range(per["rows"].shape[1]):
        v = per["rows"][:, j] != NO_ROW
        if not v.any():
            continue
        r = per["rows"][v, j]
        Cd = _sym(nodes.cov[r] / (nodes.count[r] - 1).astype(np.float64)[:, None])
        A = Sg[v] + Cd + per["eps"][v, j][:, None, None] * np.eye(3)
        d = q[v] - nodes.mean[r]
        terms.append(np.exp(-0.5 * np.einsum("ni,ni->n", d, np.linalg.solve(A, d[:, :, None])[:, :, 0])))
    return math.fsum(np.concatenate(terms).tolist()) if terms else 0.0


def central_differences(nodes, per, h):
    """g [6] and H [6, 6] of frozen_score at xi = 0 by central differences of step h"""
    f = lambda *steps: frozen_score(nodes, per, sum((s * h * np.eye(6)[a] for a, s in steps), np.zeros(6)))
    f0 = f()
    g = np.zeros(6)
    H = np.zeros((6, 6))
    plus, minus = [f((a, 1)) for a in range(6)], [f((a, -1)) for a in range(6)]
    for a in range(6):
        g[a] = (plus[a] - minus[a]) / (2 * h)
        H[a, a] = ((plus[a] - f0) + (minus[a] - f0)) / (h * h)
        for b in range(a + 1, 6):
            H[a, b] = H[b, a] = ((f((a, 1), (b, 1)) - f((a, 1), (b, -1))) - (f((a, -1), (b, 1)) - f((a, -1), (b, -1)))) / (4 * h * h)
    return g, H


def eps_min(per):
    """the smallest eps among the pairs (the scale below which the score is not smooth in h)"""
    return float(per["eps"][per["rows"] != NO_ROW].min())


def callables(dst_cells, origin, grid_len, z_len, src_cells, nbh, dst_min_points=3, src_min_points=3, **params):
    """(evaluate, score) of the restatement, as grid_ndt_amd.registration.register takes them"""
    def evaluate(T):
        d = derivs(dst_cells, origin, grid_len, z_len, src_cells, T, nbh, dst_min_points, src_min_points, **params)
        return {k: d[k] for k in ("score", "d2_sum", "matched", "terms", "g", "H", "g_abs", "H_abs")}

    def score_(T):
        return score(dst_cells, origin, grid_len, z_len, src_cells, T, nbh, None, dst_min_points, src_min_points, **params)["score"]

    return evaluate, score_


assert_derivs = dr.assert_derivs
assert_pose_sums = sr.assert_pose_sums


def assert_per_node(got_d2, got_row, want, what=""):
    """the per-node outputs: rows exactly; d2 NaN exactly where the source row does not count, elsewhere as score_ref.assert_per_point
    compares it (the reference rounded to float32, within 1 ulp of float32, +inf where there is no term)"""
    g = np.asarray(got_d2, np.float32)
    nan = np.isnan(np.asarray(want["d2"], np.float64))
    assert np.array_equal(np.isnan(g), nan), what
    assert np.all(np.asarray(got_row).astype(np.int64)[nan] == NO_ROW), what
    keep = ~nan
    sr.assert_per_point(g[keep], np.asarray(got_row)[keep], dict(d2=np.asarray(want["d2"])[keep], row=np.asarray(want["row"])[keep]), what)
