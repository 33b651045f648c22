"""Plain numpy answers to the scan score derivatives (include/gndt.h "scan score derivatives", gndt_score_derivs*), written from the
definition and nothing else.  Steps 1 to 4 (transform, key, candidates, which of them count) come from tests/score_ref.py; a counted
candidate's ub = A^-1 d and B = A^-1 by the adjugate and one reciprocal of the determinant, the nine per-point sums w3 and M in the
candidates' order, their expansion into g (6) and H (21) in the order grid_ndt_amd/csrc/gndt_score_derivs.hpp states, math.fsum over
the points.  Next to every entry of g and H the restatement returns the sum of the absolute values of that entry's terms — the same
chain with every product and sum taken of absolute values, down to the cofactors — because g and H are sums of signed terms that
cancel (g vanishes at the optimum) and a tolerance relative to the entry itself would mean nothing there.

Also here: the frozen function itself (`frozen_score`: the rows fixed, q(xi) = Exp(w) q + v in float64) for central differences, and
`callables`, the restatement as the two functions grid_ndt_amd.registration.register drives.  Shared by the CPU tier
(tests/test_score_derivs_host.py) and the GPU tier (tests/test_gpu_score_derivs.py).  Test infrastructure only.

RTOL_D, the entry-wise tolerance of g and H relative to that sum of absolute values (derived, not tuned): the code under test and the
restatement run the same fp64 operations on bit-identical inputs and differ only in what a compiler or numpy may do to them (exp's
last bits, the summation order).  An elementary term is e times two or three factors out of ub, B and q.  q is exact.  ub and B carry
the relative error of 1 / det — det is a sum of three products whose cancellation the condition number of A bounds (at most 301, so
3 x 301 x 2^-53 = 1e-13) — and, measured against the absolute-value chain, a few roundings more.  e = exp(-d2 / 2) has the relative
error d2 / 2 times d2's (1e-12 by score_ref.RTOL's own derivation), and terms with d2 > 80 are below 1e-17 of a counted term: 4e-11.
Two factors of 1 / det, e, and n 2^-53 for the order of the sums: below 1e-10.  RTOL_D = 1e-9 is score_ref.RTOL, with the same
factor of ten in hand."""
import math

import numpy as np

from tests import score_ref as sr

NO_ROW = sr.NO_ROW
RTOL_D = 1e-9
TRI = [(a, b) for a in range(6) for b in range(a, 6)]          # the record's order of H's upper triangle


def so3_exp(w):
    """Rodrigues, float64"""
    w = np.asarray(w, np.float64)
    t = float(np.linalg.norm(w))
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if t < 1e-12:
        return np.eye(3) + K + 0.5 * (K @ K)
    return np.eye(3) + (math.sin(t) / t) * K + (2.0 * math.sin(0.5 * t) ** 2 / (t * t)) * (K @ K)


def _chain(nodes, rows, qd, prm):
    """the counted candidates rows[i] (NO_ROW: none) at the float64 points qd -> valid, d2, e, ub (3), B (6: xx xy xz yy yz zz) and
    the absolute-value twins uba, Ba; zeros where not valid"""
    valid = rows != NO_ROW
    r = np.maximum(rows, 0)
    c = nodes.count[r]
    S, m = nodes.cov[r], nodes.mean[r]
    with np.errstate(all="ignore"):
        inv = 1.0 / (np.maximum(c, 2) - 1).astype(np.float64)
        cxx, cxy, cxz, cyy, cyz, czz = (S[:, k] * inv for k in range(6))
        eps = np.maximum(prm["cov_rel"] * (((cxx + cyy) + czz) / 3.0), prm["cov_floor"])
        a00, a11, a22, a01, a02, a12 = cxx + eps, cyy + eps, czz + eps, cxy, cxz, cyz
        c00, c01, c02 = a11 * a22 - a12 * a12, a02 * a12 - a01 * a22, a01 * a12 - a02 * a11
        c11, c12, c22 = a00 * a22 - a02 * a02, a01 * a02 - a00 * a12, a00 * a11 - a01 * a01
        det = (a00 * c00 + a01 * c01) + a02 * c02
        dx, dy, dz = qd[:, 0] - m[:, 0], qd[:, 1] - m[:, 1], qd[:, 2] - m[:, 2]
        ux = (c00 * dx + c01 * dy) + c02 * dz
        uy = (c01 * dx + c11 * dy) + c12 * dz
        uz = (c02 * dx + c12 * dy) + c22 * dz
        d2 = ((dx * ux + dy * uy) + dz * uz) / det
        rd = 1.0 / det
        e = np.exp(-0.5 * d2)
        ub = [ux * rd, uy * rd, uz * rd]
        B = [c00 * rd, c01 * rd, c02 * rd, c11 * rd, c12 * rd, c22 * rd]
        # the twins: every difference a sum of absolute values
        A = np.abs
        k00, k01, k02 = A(a11 * a22) + A(a12 * a12), A(a02 * a12) + A(a01 * a22), A(a01 * a12) + A(a02 * a11)
        k11, k12, k22 = A(a00 * a22) + A(a02 * a02), A(a01 * a02) + A(a00 * a12), A(a00 * a11) + A(a01 * a01)
        ax, ay, az = A(dx), A(dy), A(dz)
        uba = [(k00 * ax + k01 * ay + k02 * az) * rd, (k01 * ax + k11 * ay + k12 * az) * rd, (k02 * ax + k12 * ay + k22 * az) * rd]
        Ba = [k * rd for k in (k00, k01, k02, k11, k12, k22)]
    z = lambda v: np.where(valid, v, 0.0)
    return dict(valid=valid, d2=z(d2), e=z(e), ub=[z(v) for v in ub], B=[z(v) for v in B], uba=[z(v) for v in uba], Ba=[z(v) for v in Ba])


_PAIRS = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]


def _expand(q, w, m, absolute=False):
    """the 27 per-point values [n, 27] from w3 (3 arrays) and M (6 arrays); absolute: the twin (every term's absolute value added)"""
    qx, qy, qz = q[:, 0], q[:, 1], q[:, 2]
    mxx, mxy, mxz, myy, myz, mzz = m
    sub = lambda a, b: a + b if absolute else a - b               # a - b, or |a| + |b| of the twin's non-negative inputs
    o = [(w[j] if absolute else -w[j]) for j in range(3)]
    cross = [sub(qy * w[2], qz * w[1]), sub(qz * w[0], qx * w[2]), sub(qx * w[1], qy * w[0])]
    o += [(c if absolute else -c) for c in cross]
    p00, p01, p02 = sub(mxz * qy, mxy * qz), sub(mxx * qz, mxz * qx), sub(mxy * qx, mxx * qy)
    p10, p11, p12 = sub(myz * qy, myy * qz), sub(mxy * qz, myz * qx), sub(myy * qx, mxy * qy)
    p20, p21, p22 = sub(mzz * qy, myz * qz), sub(mxz * qz, mzz * qx), sub(myz * qx, mxz * qy)
    wq = (w[0] * qx + w[1] * qy) + w[2] * qz
    half = lambda a, b: 0.5 * (a + b)
    o += [mxx, mxy, mxz, p00, p01, p02, myy, myz, p10, p11, p12, mzz, p20, p21, p22,
          sub(sub(qy * p20, qz * p10), sub(w[0] * qx, wq)),
          sub(sub(qy * p21, qz * p11), half(w[0] * qy, w[1] * qx)),
          sub(sub(qy * p22, qz * p12), half(w[0] * qz, w[2] * qx)),
          sub(sub(qz * p01, qx * p21), sub(w[1] * qy, wq)),
          sub(sub(qz * p02, qx * p22), half(w[1] * qz, w[2] * qy)),
          sub(sub(qx * p12, qy * p02), sub(w[2] * qz, wq))]
    return np.stack(o, 1)


def _full(h21):
    H = np.zeros((6, 6))
    for v, (a, b) in zip(h21, TRI):
        H[a, b] = H[b, a] = v
    return H


def derivs_pose(nodes, origin, grid_len, z_len, pts, T, nbh, prm):
    """one pose -> dict(score, d2_sum, matched, terms, g [6], H [6, 6], g_abs, H_abs, and for the frozen function rows [n, nbh]
    (NO_ROW: does not count) and q [n, 3] float64, the per-point values vals [n, 27] and their absolute-value twins vabs)"""
    per = sr.score_pose(nodes, origin, grid_len, z_len, pts, T, nbh, prm)
    R = per["all_rows"]
    n = len(R)
    qd = per["q"].astype(np.float64)
    w = [np.zeros(n) for _ in range(3)]
    m = [np.zeros(n) for _ in range(6)]
    wa = [np.zeros(n) for _ in range(3)]
    ma = [np.zeros(n) for _ in range(6)]
    if nodes.n:
        for j in range(R.shape[1]):                                # the candidates' order
            c = _chain(nodes, R[:, j], qd, prm)
            for i in range(3):
                w[i] = w[i] + c["e"] * c["ub"][i]
                wa[i] = wa[i] + c["e"] * c["uba"][i]
            for k, (a, b) in enumerate(_PAIRS):
                m[k] = m[k] + c["e"] * (c["ub"][a] * c["ub"][b] - c["B"][k])
                ma[k] = ma[k] + c["e"] * (c["uba"][a] * c["uba"][b] + c["Ba"][k])
    has = (R != NO_ROW).any(1)
    qs = np.where(has[:, None], qd, 0.0)                           # (a point without a counted candidate adds nothing: q may be NaN)
    with np.errstate(all="ignore"):
        vals = np.where(has[:, None], _expand(qs, w, m), 0.0)
        vabs = np.where(has[:, None], _expand(np.abs(qs), wa, ma, absolute=True), 0.0)
    tot = np.array([math.fsum(vals[:, j].tolist()) for j in range(27)])
    tab = np.array([math.fsum(vabs[:, j].tolist()) for j in range(27)])
    return dict(score=per["score"], d2_sum=per["d2_sum"], matched=per["matched"], terms=per["terms"], g=tot[:6], H=_full(tot[6:]),
                g_abs=tab[:6], H_abs=_full(tab[6:]), rows=R, q=qd, vals=vals, vabs=vabs, raw_d2=per["raw_d2"])


def derivs(cells, origin, grid_len, z_len, pts, poses, nbh=sr.DIRECT1, min_points=3, **params):
    """every pose -> dict of arrays score, d2_sum, matched, terms [K], g, g_abs [K, 6], H, H_abs [K, 6, 6] and `poses_out`"""
    prm = sr.defaults(min_points=min_points, **params)
    nodes = sr.Nodes(cells)
    per = [derivs_pose(nodes, origin, grid_len, z_len, pts, T, nbh, prm) for T in sr.as_poses(poses)]
    out = {k: np.array([p[k] for p in per], np.int64 if k in ("matched", "terms") else np.float64)
           for k in ("score", "d2_sum", "matched", "terms", "g", "H", "g_abs", "H_abs")}
    out["poses_out"] = per
    return out


def frozen_score(nodes, rows, q, xi, prm):
    """the frozen sum at the perturbation xi: the candidates `rows` of every point fixed, q(xi) = Exp(w) q + v in float64"""
    xi = np.asarray(xi, np.float64)
    qx = q @ so3_exp(xi[3:]).T + xi[:3]
    terms = []
    for j in range(rows.shape[1]):
        c = _chain(nodes, rows[:, j], qx, prm)
        terms.append(c["e"][c["valid"]])
    return math.fsum(np.concatenate(terms).tolist())


def central_differences(nodes, rows, q, prm, h):
    """g [6] and H [6, 6] of frozen_score at xi = 0 by central differences of step h"""
    f = lambda *steps: frozen_score(nodes, rows, q, sum((s * h * np.eye(6)[a] for a, s in steps), np.zeros(6)), prm)
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


def eps_min(nodes, rows, prm):
    """the smallest eps among the counted nodes `rows` (the scale below which the score is not smooth in h)"""
    r = np.unique(rows[rows != NO_ROW])
    inv = 1.0 / (nodes.count[r] - 1).astype(np.float64)
    tr = ((nodes.cov[r, 0] * inv + nodes.cov[r, 3] * inv) + nodes.cov[r, 5] * inv) / 3.0
    return float(np.maximum(prm["cov_rel"] * tr, prm["cov_floor"]).min())


def callables(cells, origin, grid_len, z_len, pts, nbh, min_points=3, **params):
    """(evaluate, score) of the restatement, as grid_ndt_amd.registration.register takes them"""
    def evaluate(T):
        d = derivs(cells, origin, grid_len, z_len, pts, T, nbh, min_points, **params)
        return {k: d[k] for k in ("score", "d2_sum", "matched", "terms", "g", "H", "g_abs", "H_abs")}

    def score(T):
        return sr.score(cells, origin, grid_len, z_len, pts, T, nbh, None, min_points, **params)["score"]

    return evaluate, score


def assert_derivs(got, want, k=None, what=""):
    """matched / terms exactly, score / d2_sum at score_ref.RTOL, g and H entry-wise within RTOL_D x the sum of the absolute values of
    the entry's terms; got and want dicts of length-K arrays (k: one pose)"""
    sr.assert_pose_sums(got, want, k, what)
    sel = slice(None) if k is None else k
    for name in ("g", "H"):
        g, w = np.asarray(got[name], np.float64)[sel], np.asarray(want[name], np.float64)[sel]
        bound = RTOL_D * np.asarray(want[name + "_abs"], np.float64)[sel]
        assert np.all(np.abs(g - w) <= bound), (what, name, float(np.max(np.abs(g - w) / np.maximum(bound, 1e-300))))


def pose_error(T, truth=None):
    """(translation error in m, rotation angle in rad) of pose T against `truth` (default: the identity)"""
    T = np.asarray(T, np.float64)[:3]
    G = np.eye(4)[:3] if truth is None else np.asarray(truth, np.float64)[:3]
    dR = T[:, :3] @ G[:, :3].T
    ang = math.acos(max(-1.0, min(1.0, (np.trace(dR) - 1.0) / 2.0)))
    return float(np.linalg.norm(T[:, 3] - dR @ G[:, 3])), ang
