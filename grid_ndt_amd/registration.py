"""Newton registration of a scan against an NDT grid, driven from the scan score's derivatives (include/gndt.h "scan score
derivatives").  Pure numpy and independent of TwoDmap: `register` takes two callables, so the same driver runs on the device
(TwoDmap.register binds score_derivs / score_poses), on a host build of the per-element code and on a numpy restatement.

The pose perturbation is the derivatives': xi = (v, w) acts on the left, T <- [Exp(w) R | Exp(w) t + v].

One iteration of one start (K starts run the same rule side by side, their calls batched):
  1. D = evaluate(T).  D.terms == 0: stop, "no_overlap".
  2. lam, V = eigh(-H); lam_i <- max(|lam_i|, 1e-6 max_j |lam_j|); delta = V diag(1 / lam) V^T g.  (Saddle-free Newton: an ascent
     direction whatever the signs of the eigenvalues.)
  3. delta is scaled by min(1, step_t / |delta_v|, step_r / |delta_w|).
  4. Line search in one batched score call: the poses retract(T, a delta), a = 1, 1/2, 1/4, 1/8; the a of the highest score wins
     (ties: the larger a).  That score not above D.score: stop, "no_ascent", T unchanged.  (The true score jumps where a point
     changes cell, which the frozen derivatives do not see: "no_ascent" close to the optimum is a normal ending.)
  5. T <- retract(T, a delta); a |delta_v| < tol_t and a |delta_w| < tol_r: stop, "converged"; after max_iterations: "iterations".
The score never decreases along the accepted poses."""
import numpy as np

STEPS = (1.0, 0.5, 0.25, 0.125)
_FIELDS = ("score", "d2_sum", "matched", "terms", "g", "H")


def so3_exp(w):
    """Exp([w]x), Rodrigues in float64: I + (sin t / t) K + (2 sin^2(t / 2) / t^2) K^2, t = |w|"""
    w = np.asarray(w, np.float64).reshape(3)
    t = float(np.sqrt(w @ w))
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if t < 1e-12:
        a, b = 1.0, 0.5
    else:
        a, b = np.sin(t) / t, 2.0 * np.sin(0.5 * t) ** 2 / (t * t)
    return np.eye(3) + a * K + b * (K @ K)


def retract(T, xi):
    """[Exp(w) R | Exp(w) t + v] of T = [R | t] (3 x 4, or 4 x 4 whose last row is dropped) and xi = (v, w)"""
    T = np.asarray(T, np.float64)[:3]
    xi = np.asarray(xi, np.float64).reshape(6)
    E = so3_exp(xi[3:])
    return np.concatenate([E @ T[:, :3], (E @ T[:, 3] + xi[:3])[:, None]], 1)


def newton_delta(g, H, step_t, step_r):
    """steps 2 and 3: the saddle-free Newton step of gradient g and Hessian H, inside the two step bounds"""
    g = np.asarray(g, np.float64).reshape(6)
    H = np.asarray(H, np.float64).reshape(6, 6)
    lam, V = np.linalg.eigh(-H)
    lam = np.abs(lam)
    top = float(lam.max())
    if top > 0.0:
        delta = V @ ((V.T @ g) / np.maximum(lam, 1e-6 * top))
    else:
        delta = g.copy()               # (no curvature at all: the gradient's direction, cut to the bounds below)
    nv, nw = float(np.linalg.norm(delta[:3])), float(np.linalg.norm(delta[3:]))
    scale = min(1.0, step_t / nv if nv > 0.0 else np.inf, step_r / nw if nw > 0.0 else np.inf)
    return delta * scale


def _host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def choose_step(scores):
    """step 4's choice among the four candidates' scores: the index of the highest, ties to the larger a (the lower index)"""
    return int(np.argmax(np.asarray(scores, np.float64)))


def register(evaluate, score, T0, step_t, step_r=0.05, tol_t=1e-4, tol_r=1e-5, max_iterations=30):
    """evaluate(T [K, 3, 4]) -> dict of score, d2_sum, matched, terms [K], g [K, 6], H [K, 6, 6]; score(T [K, 3, 4]) -> scores [K].
    T0: one start ([3, 4] / [4, 4]) -> dict(T, reason, iterations, history); K starts ([K, 3, 4] / [K, 4, 4]) -> a list of those.
    history: per iteration dict(T (the pose evaluated), derivs, delta, scores (the four candidates'), a (None: not accepted))."""
    T0 = np.asarray(T0, np.float64)
    single = T0.ndim == 2
    T = np.array((T0[None] if single else T0)[:, :3, :], np.float64)
    out = [dict(T=T[k].copy(), reason=None, iterations=0, history=[]) for k in range(len(T))]
    live = list(range(len(T)))
    while live:
        D = {k: _host(v) for k, v in evaluate(T[live]).items()}
        trial, cand = [], []
        for j, k in enumerate(live):
            d = {f: (D[f][j].copy() if np.ndim(D[f][j]) else D[f][j].item()) for f in _FIELDS}
            h = dict(T=T[k].copy(), derivs=d, delta=None, scores=None, a=None)
            out[k]["history"].append(h)
            out[k]["iterations"] += 1
            if int(d["terms"]) == 0:
                out[k]["reason"] = "no_overlap"
                continue
            h["delta"] = newton_delta(d["g"], d["H"], step_t, step_r)
            trial.append(k)
            cand.extend(retract(T[k], a * h["delta"]) for a in STEPS)
        if trial:
            S = np.asarray(_host(score(np.stack(cand))), np.float64).reshape(len(trial), len(STEPS))
        for j, k in enumerate(trial):
            h = out[k]["history"][-1]
            h["scores"] = S[j].copy()
            best = choose_step(S[j])
            if not S[j, best] > h["derivs"]["score"]:
                out[k]["reason"] = "no_ascent"
                continue
            a = STEPS[best]
            h["a"] = a
            T[k] = cand[len(STEPS) * j + best]
            out[k]["T"] = T[k].copy()
            if a * np.linalg.norm(h["delta"][:3]) < tol_t and a * np.linalg.norm(h["delta"][3:]) < tol_r:
                out[k]["reason"] = "converged"
            elif out[k]["iterations"] >= max_iterations:
                out[k]["reason"] = "iterations"
        live = [k for k in live if out[k]["reason"] is None]
    return out[0] if single else out


def register_pyramid(stages, T0, step_r=0.05, tol_t=1e-4, tol_r=1e-5, max_iterations=30):
    """Coarse-to-fine: `register` on every stage in turn, each start's pose chained from stage to stage.  stages: a list of
    (evaluate, score, step_t), coarsest map first (TwoDmap.register(pyramid=...) binds the maps of TwoDmap.pyramid and half of each
    level's own cell).  The score's basin is less than a cell of the map it is taken on, so a start several fine cells off is first
    brought within a fine cell on the coarse maps.  T0 as for `register`; K starts run side by side on every stage.  Returns the last
    stage's result(s) with one more entry, levels: every stage's result of that start, in the order of `stages`."""
    stages = list(stages)
    if not stages:
        raise ValueError("register_pyramid needs at least one stage")
    T0 = np.asarray(T0, np.float64)
    single = T0.ndim == 2
    T = np.array((T0[None] if single else T0)[:, :3, :], np.float64)
    levels = [[] for _ in range(len(T))]
    for evaluate, score, step_t in stages:
        res = register(evaluate, score, T, step_t=step_t, step_r=step_r, tol_t=tol_t, tol_r=tol_r, max_iterations=max_iterations)
        for k, r in enumerate(res):
            levels[k].append(r)
            T[k] = r["T"]
    out = [dict(lv[-1], levels=lv) for lv in levels]
    return out[0] if single else out
