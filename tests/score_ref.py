"""Plain numpy answers to scan scoring (include/gndt.h "scan scoring", gndt_score_poses*), written from the definition and nothing
else: the pose applied in float64 in the definition's bracketing and rounded once to float32, the key through tests/query_ref.py's
`keys`, the nodes looked up by their packed key, the face neighbours by the index rules that skip 0, every term's d2 by the adjugate
in the order the definition's header states, math.fsum for the sums.  Shared by the CPU tier (tests/test_score_host.py) and the GPU
tier (tests/test_gpu_score.py).  Test infrastructure only."""
import math

import numpy as np

from tests import query_ref as qr

NO_ROW = qr.NO_ROW
DIRECT1, DIRECT7 = 1, 7
RTOL = 1e-9            # d2, score, d2_sum: fp64 arithmetic on identical inputs, condition number <= 301


def defaults(min_count=0, cov_rel=0.0, cov_floor=0.0, max_d2=0.0, min_points=3):
    """the parameters as the library resolves them: 0 = default; the floats are the struct's float32 values widened"""
    return dict(min_count=int(min_count) if min_count else max(int(min_points), 3),
                cov_rel=float(np.float32(cov_rel)) if cov_rel else float(np.float32(0.01)),
                cov_floor=float(np.float32(cov_floor)) if cov_floor else float(np.float32(1e-6)),
                max_d2=float(np.float32(max_d2)))


def as_poses(poses):
    a = np.asarray(poses, np.float64)
    if a.ndim == 2:
        a = a[None]
    return np.ascontiguousarray(a[:, :3, :])


def transform(T, pts):
    """q = fl32(T p): float64, ((R_i0 x + R_i1 y) + R_i2 z) + t_i, one rounding per coordinate"""
    T = np.asarray(T, np.float64)[:3]
    p = np.asarray(pts, np.float32)[:, :3].astype(np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.stack([((T[i, 0] * x + T[i, 1] * y) + T[i, 2] * z) + T[i, 3] for i in range(3)], 1)
        return q.astype(np.float32)


def _step_skip0(v, d):
    r = v + d
    return np.where(r == 0, r + d, r)


def _above(z):
    return np.where(z == -1, 1, z + 1)


def _below(z):
    return np.where(z == 1, -1, z - 1)


def candidate_keys(sx, sy, sz, ok, nbh):
    """-> [(sx, sy, sz, ok)] of the 1 or 7 candidates, a neighbour index beyond the codec's range dropped"""
    out = [(sx, sy, sz, ok)]
    if nbh == DIRECT7:
        for d in (-1, 1):
            v = _step_skip0(sx, d)
            out.append((v, sy, sz, ok & (np.abs(v) <= qr.MAX_XY)))
        for d in (-1, 1):
            v = _step_skip0(sy, d)
            out.append((sx, v, sz, ok & (np.abs(v) <= qr.MAX_XY)))
        for v in (_above(sz), _below(sz)):
            out.append((sx, sy, v, ok & (np.abs(v) <= qr.MAX_Z)))
    return out


class Nodes:
    """the rows of an export by packed key"""

    def __init__(self, cells):
        self.n = int(len(cells["sx"]))
        mk = qr.pack(cells["sx"], cells["sy"], cells["sz"])
        self.order = np.argsort(mk, kind="stable")
        self.keys = mk[self.order]
        self.count = np.asarray(cells["count"]).astype(np.int64)
        self.mean = np.asarray(cells["mean"], np.float32).astype(np.float64).reshape(-1, 3)
        self.cov = np.asarray(cells["cov"], np.float32).astype(np.float64).reshape(-1, 6)

    def rows(self, sx, sy, sz, ok):
        if self.n == 0:
            return np.full(len(sx), NO_ROW, np.int64)
        q = qr.pack(sx, sy, sz)
        pos = np.minimum(np.searchsorted(self.keys, q), self.n - 1)
        return np.where(ok & (self.keys[pos] == q), self.order[pos], NO_ROW).astype(np.int64)


def d2_of(nodes, rows, q, prm):
    """d2 of q[i] against rows[i] (float64) and whether that candidate counts"""
    r = np.maximum(rows, 0)
    c = nodes.count[r] if nodes.n else np.zeros(len(rows), np.int64)
    valid = (rows != NO_ROW) & (c >= prm["min_count"])
    if nodes.n == 0:
        return np.full(len(rows), np.inf), valid, np.full(len(rows), np.inf)
    S = nodes.cov[r]
    m = nodes.mean[r]
    with np.errstate(all="ignore"):
        inv = 1.0 / (np.maximum(c, 2) - 1).astype(np.float64)
        cxx, cxy, cxz, cyy, cyz, czz = (S[:, k] * inv for k in range(6))
        eps = np.maximum(prm["cov_rel"] * (((cxx + cyy) + czz) / 3.0), prm["cov_floor"])
        a00, a11, a22, a01, a02, a12 = cxx + eps, cyy + eps, czz + eps, cxy, cxz, cyz
        c00, c01, c02 = a11 * a22 - a12 * a12, a02 * a12 - a01 * a22, a01 * a12 - a02 * a11
        c11, c12, c22 = a00 * a22 - a02 * a02, a01 * a02 - a00 * a12, a00 * a11 - a01 * a01
        det = (a00 * c00 + a01 * c01) + a02 * c02
        qd = q.astype(np.float64)
        dx, dy, dz = qd[:, 0] - m[:, 0], qd[:, 1] - m[:, 1], qd[:, 2] - m[:, 2]
        ux = (c00 * dx + c01 * dy) + c02 * dz
        uy = (c01 * dx + c11 * dy) + c12 * dz
        uz = (c02 * dx + c12 * dy) + c22 * dz
        d2 = ((dx * ux + dy * uy) + dz * uz) / det
    raw = np.where(valid, d2, np.inf)
    if prm["max_d2"] > 0.0:
        valid = valid & ~(d2 > prm["max_d2"])
    return np.where(valid, d2, np.inf), valid, raw


def score_pose(nodes, origin, grid_len, z_len, pts, T, nbh, prm):
    """one pose -> dict(score, d2_sum, matched, terms, d2 [n] float64 (inf: no term), row [n], q [n, 3], and per candidate
    all_d2 / all_rows [n, nbh] (inf / NO_ROW: does not count), raw_d2 (before the max_d2 gate))"""
    q = transform(T, pts)
    sx, sy, sz, _, ok = qr.keys(q, origin, grid_len, z_len)
    d2s, rws, raws = [], [], []
    for kx, ky, kz, kok in candidate_keys(sx, sy, sz, ok, nbh):
        rows = nodes.rows(kx, ky, kz, kok)
        d2, valid, raw = d2_of(nodes, rows, q, prm)
        d2s.append(d2)
        raws.append(raw)
        rws.append(np.where(valid, rows, NO_ROW))
    D, R = np.stack(d2s, 1), np.stack(rws, 1)
    valid = R != NO_ROW
    terms = D[valid]
    best = np.full(len(q), np.inf)
    brow = np.full(len(q), NO_ROW, np.int64)
    for j in range(D.shape[1]):
        take = valid[:, j] & ((D[:, j] < best) | ((D[:, j] == best) & (R[:, j] < brow)))
        best[take], brow[take] = D[take, j], R[take, j]
    return dict(score=math.fsum(np.exp(-0.5 * terms).tolist()), d2_sum=math.fsum(terms.tolist()), terms=int(valid.sum()),
                matched=int(valid.any(1).sum()), d2=best, row=brow, q=q, all_d2=D, all_rows=R, raw_d2=np.stack(raws, 1))


def score(cells, origin, grid_len, z_len, pts, poses, nbh=DIRECT1, per_point=None, min_points=3, **params):
    """every pose -> dict of length-K arrays score, d2_sum, matched, terms; with per_point=k also d2 (float64), row of pose k and
    `poses_out`, the per-pose dicts"""
    prm = defaults(min_points=min_points, **params)
    nodes = Nodes(cells)
    per = [score_pose(nodes, origin, grid_len, z_len, pts, T, nbh, prm) for T in as_poses(poses)]
    out = {"score": np.array([p["score"] for p in per], np.float64), "d2_sum": np.array([p["d2_sum"] for p in per], np.float64),
           "matched": np.array([p["matched"] for p in per], np.int64), "terms": np.array([p["terms"] for p in per], np.int64),
           "poses_out": per}
    if per_point is not None:
        out.update(d2=per[per_point]["d2"], row=per[per_point]["row"])
    return out


def gate_margin(per, max_d2):
    """the least relative distance of a candidate's d2 (counted or gated) from max_d2 over the per-pose dicts: a case whose reference
    sits within RTOL of the gate would make `terms` depend on the last bits, so a test checks its own cases with this"""
    raw = np.concatenate([p["raw_d2"].ravel() for p in per])
    raw = raw[np.isfinite(raw)]
    return float(np.min(np.abs(raw - max_d2)) / max_d2) if raw.size else np.inf


def assert_pose_sums(got, want, k=None, what=""):
    """score / d2_sum at RTOL, matched / terms exactly; got and want dicts of length-K arrays (k: one pose)"""
    sel = slice(None) if k is None else k
    for name in ("matched", "terms"):
        g, w = np.asarray(got[name])[sel], np.asarray(want[name])[sel]
        assert np.array_equal(g, w), (what, name, g, w)
    for name in ("score", "d2_sum"):
        g, w = np.asarray(got[name], np.float64)[sel], np.asarray(want[name], np.float64)[sel]
        assert np.all(np.abs(g - w) <= RTOL * np.abs(w)), (what, name, g, w)


def assert_per_point(got_d2, got_row, want, what=""):
    """the per-point outputs: rows exactly, d2 against the reference rounded to float32, within 1 ulp of float32"""
    got_row = np.asarray(got_row).astype(np.int64)
    assert np.array_equal(got_row, want["row"]), (what, np.flatnonzero(got_row != want["row"])[:10])
    g = np.asarray(got_d2, np.float32)
    with np.errstate(over="ignore"):
        w = np.asarray(want["d2"], np.float64).astype(np.float32)
    none = np.isinf(w)
    assert np.array_equal(np.isinf(g) & (g > 0), none), what
    ulp = np.spacing(np.abs(w[~none]))
    assert np.all(np.abs(g[~none].astype(np.float64) - w[~none].astype(np.float64)) <= ulp.astype(np.float64)), what
