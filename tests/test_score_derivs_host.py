"""CPU tier: the scan score derivatives' per-element code (grid_ndt_amd/csrc/gndt_score_derivs.hpp: the sink of score_point,
score_derivs_expand, and the kernels' fixed summation tree restated in tests/score_derivs_shim.cpp), compiled with g++ into
tests/_score_derivs_shim.so, against the numpy restatement of the definition (tests/score_derivs_ref.py) on maps the oracle builds;
the restatement itself against central differences of its own frozen function; grid_ndt_amd/registration.py on hand cases and, driven
on the shim, step by step against the restatement; and the product entry points refuse to run without a GPU.

Tolerances (derived, not tuned): matched and terms exact; score and d2_sum at score_ref.RTOL, and bit for bit what the existing score
shim gives; g and H entry-wise within score_derivs_ref.RTOL_D x the sum of the absolute values of the entry's terms (derived there).
Finite differences: the error of g and of H against central differences falls by at least 3x per halving of h (a second-order
scheme gives 4x; the margin is for the last halving meeting the rounding floor), from h <= sqrt(eps_min) / 10.

Recovery (measured with the numpy restatement driver, the reference, with every 5th point of the cloud the map was built from as the
scan; start A = 0.2, -0.15 cells, 0.1 level, yaw 1 degree; start B = 0.4, 0.3 cells, -0.2 level, yaw 2 degrees; on uniform_box(40 001),
0.5 m cells and levels, that is 0.135 m / 17.5 mrad and 0.269 m / 34.9 mrad off, on drivable_site(100 000), a surface 30 m across in
0.5 m cells and 0.25 m levels, 0.127 m and 0.255 m): RECOVERY below has every case's final error, iterations and ending.  The tests
assert that the final pose of the restatement's own run and of the run under test is less than half the start offset off, in
translation and in angle.  bridge_ground and terrain are not recovery cases (needle-thin nodes; a lever arm of 200 m): they stay
cases for the derivative values."""
import ctypes as C
import math

import numpy as np
import pytest

from grid_ndt_amd import registration as reg
from grid_ndt_amd import scenes
from tests import score_derivs_ref as dr
from tests import score_ref as sr
from tests.host_emulation import MAP, HostMap, load_shim
from tests.test_score_host import _map, five_poses, host_score, yaw

# the restatement driver's own endings: (neighbourhood, start) -> final error (m, rad), iterations, reason
RECOVERY = {
    ("uniform_box", 1, "A"): "0.4 mm, 0.14 mrad, 8 iterations, converged",
    ("uniform_box", 1, "B"): "0.4 mm, 0.12 mrad, 11 iterations, converged",
    ("uniform_box", 7, "A"): "9.1 mm, 2.3 mrad, 3 iterations, no_ascent",
    ("uniform_box", 7, "B"): "0.8 mm, 0.13 mrad, 7 iterations, converged",
    ("drivable_site", 1, "A"): "0.9 mm, 0.027 mrad, 10 iterations, converged",
    ("drivable_site", 1, "B"): "0.9 mm, 0.027 mrad, 11 iterations, converged",
    ("drivable_site", 7, "A"): "0.9 mm, 0.029 mrad, 10 iterations, no_ascent",
    ("drivable_site", 7, "B"): "0.9 mm, 0.029 mrad, 12 iterations, converged",
}
RECOVERY_SCENES = {
    "uniform_box": lambda: (scenes.uniform_box(40_001, half_xy=6.0, half_z=1.0), dict(grid_len=0.5, z_len=0.5, slope_interval=0.08)),
    "drivable_site": lambda: (scenes.drivable_site(100_000), scenes.COST_PARAMS),
}
_rmaps = {}


def recovery_map(name):
    """(cloud, HostMap) of a recovery scene"""
    if name not in _rmaps:
        cloud, P = RECOVERY_SCENES[name]()
        _rmaps[name] = (cloud, HostMap(cloud, P))
    return _rmaps[name]


_shim = None


def shim():
    global _shim
    if _shim is None:
        vp, u32, u64, d = C.c_void_p, C.c_uint32, C.c_uint64, C.c_double
        _shim = load_shim("score_derivs_shim.cpp", "_score_derivs_shim.so", {
            "dshim_score_derivs": ([C.c_int, vp, u32, u64, vp, u32, MAP, u32, d, d, d, vp, u32, vp], C.c_int),
        })
    return _shim


def host_derivs(m, pts, poses, nbh=1, per_point=None, **params):
    """score_derivs_point over every (point, pose) pair on a HostMap, summed in the kernels' tree -> the dict TwoDmap.score_derivs
    returns, with per_point=k also vals [n, 27] (the points' own values at pose k)"""
    prm = sr.defaults(**params)
    pts = np.ascontiguousarray(pts, np.float32)
    T = np.ascontiguousarray(sr.as_poses(poses)).reshape(-1, 12)
    K, n = T.shape[0], pts.shape[0]
    rec = np.zeros((K, 31), np.int64)
    vals = np.zeros((n, 27), np.float64)
    want = per_point is not None
    rc = shim().dshim_score_derivs(nbh, pts.ctypes.data, pts.shape[1], n, T.ctypes.data, K, m.shim_map(), prm["min_count"], prm["cov_rel"],
                                   prm["cov_floor"], prm["max_d2"], rec.ctypes.data, per_point if want else 0xFFFFFFFF,
                                   C.c_void_p(vals.ctypes.data if want else 0))
    assert rc == 0
    fl = rec.view(np.float64)
    H = np.zeros((K, 6, 6))
    for j, (a, b) in enumerate(dr.TRI):
        H[:, a, b] = H[:, b, a] = fl[:, 10 + j]
    out = {"score": fl[:, 0].copy(), "d2_sum": fl[:, 1].copy(), "matched": rec[:, 2].copy(), "terms": rec[:, 3].copy(),
           "g": fl[:, 4:10].copy(), "H": H}
    if want:
        out["vals"] = vals
    return out


def ref_derivs(m, pts, poses, nbh=1, **params):
    return dr.derivs(m.cells, m.origin, m.P["grid_len"], m.P["z_len"], pts, poses, nbh, **params)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---- 1. the formulas: the restatement against central differences of its own frozen function ----

@pytest.mark.parametrize("nbh", [1, 7])
def test_restatement_equals_central_differences_of_the_frozen_sum(nbh):
    cloud, m = _map("uniform_box")
    scan = np.ascontiguousarray(cloud[1:][::5])
    P = m.P
    T = yaw(1.0, (0.1 * P["grid_len"], -0.1 * P["grid_len"], 0.1 * P["z_len"]))       # 1 degree and a tenth of a cell off
    prm = sr.defaults()
    nodes = sr.Nodes(m.cells)
    d = dr.derivs_pose(nodes, m.origin, P["grid_len"], P["z_len"], scan, T, nbh, prm)
    assert d["terms"] > 1000
    em = dr.eps_min(nodes, d["rows"], prm)
    h0 = min(1e-3, math.sqrt(em) / 10.0)
    errs = []
    for h in (h0, h0 / 2, h0 / 4):
        g, H = dr.central_differences(nodes, d["rows"], d["q"], prm, h)
        errs.append((float(np.abs(g - d["g"]).max() / np.abs(d["g"]).max()), float(np.abs(H - d["H"]).max() / np.abs(d["H"]).max())))
    print("nbh", nbh, "eps_min", em, "h0", h0, "relative errors of (g, H) at h0, h0/2, h0/4:", errs)
    for a, b in zip(errs, errs[1:]):
        assert b[0] * 3.0 <= a[0] and b[1] * 3.0 <= a[1], errs
    assert errs[-1][0] < 1e-3 and errs[-1][1] < 1e-2, errs          # (second order with no constant part)


# ---- 2. the per-element code against the restatement, and the four sums against the score shim bit for bit ----

@pytest.mark.parametrize("nbh", [1, 7])
@pytest.mark.parametrize("name", ["bridge_ground", "face_lattice", "uniform_box"])
def test_derivs_equal_the_restatement(name, nbh):
    cloud, m = _map(name)
    scan = np.ascontiguousarray(cloud[1:][::3])
    poses = five_poses(m.P)
    want = ref_derivs(m, scan, poses, nbh)
    assert want["terms"][0] > 100 and (want["terms"] > 0).all()
    got = host_derivs(m, scan, poses, nbh, per_point=3)
    dr.assert_derivs(got, want, what=(name, nbh))
    assert np.abs(want["g"]).max() > 0 and (np.abs(want["H"]).max((1, 2)) > 0).all()
    assert np.array_equal(got["H"], got["H"].transpose(0, 2, 1))
    # every point's own 27 values
    wp = want["poses_out"][3]
    assert np.all(np.abs(got["vals"] - wp["vals"]) <= dr.RTOL_D * wp["vabs"])
    # the four sums: the score shim's bits
    plain = host_score(m, scan, poses, nbh)
    for k in ("score", "d2_sum"):
        assert np.array_equal(_bits(got[k]), _bits(plain[k])), k
    for k in ("matched", "terms"):
        assert np.array_equal(got[k], plain[k]), k


# ---- 3. nothing to match: exact zeros; the gate ----

def test_nan_pose_off_the_map_and_the_gate():
    cloud, m = _map("uniform_box")
    scan = np.ascontiguousarray(cloud[1:][::7])
    bad = yaw(0)
    bad[2, 0] = np.nan
    poses = np.stack([yaw(0.5), yaw(0, (5000.0, 0, 0)), bad])
    for nbh in (1, 7):
        got = host_derivs(m, scan, poses, nbh)
        for k in (1, 2):
            assert got["score"][k] == 0.0 and got["d2_sum"][k] == 0.0 and got["matched"][k] == 0 and got["terms"][k] == 0
            assert not got["g"][k].any() and not got["H"][k].any() and np.isfinite(got["H"][k]).all()
        assert got["terms"][0] > 100
        gate = 4.0
        want = ref_derivs(m, scan, poses, nbh, max_d2=gate)
        assert sr.gate_margin(want["poses_out"], gate) > 1e-6
        g2 = host_derivs(m, scan, poses, nbh, max_d2=gate)
        dr.assert_derivs(g2, want, what=("gate", nbh))
        assert 0 < g2["terms"][0] < got["terms"][0]
        plain = host_score(m, scan, poses, nbh, max_d2=gate)
        assert np.array_equal(_bits(g2["score"]), _bits(plain["score"])) and np.array_equal(g2["terms"], plain["terms"])


# ---- 4. registration.py on hand cases ----

def test_retract_on_hand_cases():
    T = np.array([[1.0, 0, 0, 1.0], [0, 1.0, 0, 2.0], [0, 0, 1.0, 3.0]])
    assert np.array_equal(reg.retract(T, np.zeros(6)), T)
    q = reg.retract(T, [0.5, 0, 0, 0, 0, math.pi / 2])                # 90 degrees about z on the left, then the translation
    want = np.array([[0.0, -1, 0, -2 + 0.5], [1, 0, 0, 1], [0, 0, 1, 3]])
    assert np.abs(q - want).max() < 1e-15
    for w in (1e-13, 1e-9, 1e-5):                                     # |w| -> 0: I + [w]x to first order, a rotation always
        R = reg.so3_exp([w, -2 * w, 0.5 * w])
        K = np.array([[0, -0.5 * w, -2 * w], [0.5 * w, 0, -w], [2 * w, w, 0]])
        assert np.abs(R - (np.eye(3) + K)).max() <= 4 * w * w and np.abs(R @ R.T - np.eye(3)).max() < 1e-15
    R = reg.so3_exp([0.3, -0.2, 0.9])
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-15 and abs(np.linalg.det(R) - 1) < 1e-15
    assert np.abs(reg.so3_exp([0.3, -0.2, 0.9]) @ reg.so3_exp([-0.3, 0.2, -0.9]) - np.eye(3)).max() < 1e-15
    assert np.abs(reg.retract(np.eye(4), [1, 2, 3, 0, 0, 0]) - np.eye(4)[:3] - np.array([[0, 0, 0, 1], [0, 0, 0, 2], [0, 0, 0, 3.0]])).max() == 0


def test_newton_delta_on_hand_cases():
    rng = np.random.default_rng(4)
    A = rng.normal(size=(6, 6))
    Hneg = -(A @ A.T + 0.5 * np.eye(6))                                # negative definite, condition far below 1e6
    g = rng.normal(size=6)
    d = reg.newton_delta(g, Hneg, 1e9, 1e9)
    assert np.abs(d - np.linalg.solve(-Hneg, g)).max() <= 1e-10 * np.abs(d).max()
    Q, _ = np.linalg.qr(rng.normal(size=(6, 6)))
    Hind = Q @ np.diag([-3.0, -2.0, -1.0, 0.5, 2.0, 0.0]) @ Q.T       # indefinite, and singular
    d = reg.newton_delta(g, Hind, 1e9, 1e9)
    assert g @ d > 0 and np.isfinite(d).all()
    for st, sr_ in ((0.01, 1e9), (1e9, 0.002), (0.01, 0.002)):
        for H in (Hneg, Hind):
            full, d = reg.newton_delta(g, H, 1e9, 1e9), reg.newton_delta(g, H, st, sr_)
            assert np.linalg.norm(d[:3]) <= st * (1 + 1e-12) and np.linalg.norm(d[3:]) <= sr_ * (1 + 1e-12)
            s = min(1.0, st / np.linalg.norm(full[:3]), sr_ / np.linalg.norm(full[3:]))
            assert np.abs(d - s * full).max() <= 1e-15 * np.abs(full).max() and s < 1
    assert np.array_equal(reg.newton_delta(g, Hneg, 1e9, 1e9), reg.newton_delta(g, Hneg, 1e12, 1e12))
    assert np.isfinite(reg.newton_delta(g, np.zeros((6, 6)), 0.1, 0.1)).all()
    assert reg.choose_step([1.0, 2.0, 2.0, 0.5]) == 1 and reg.choose_step([3.0, 3.0, 3.0, 3.0]) == 0


# ---- 5. the driver on the shim, step by step against the restatement ----

def starts(P):
    g, z = P["grid_len"], P["z_len"]
    return {"A": yaw(1.0, (0.2 * g, -0.15 * g, 0.1 * z)), "B": yaw(2.0, (0.4 * g, 0.3 * g, -0.2 * z))}


def check_steps(res, T0, ref_eval, ref_score, step_t, step_r=0.05, what=""):
    """one start's result, every recorded iteration against the rule and the restatement: the derivatives and the four candidates'
    scores are the restatement's AT the recorded pose, delta is newton_delta of the recorded g and H, a is the rule's choice among the
    recorded scores, the accepted scores never decrease, and the poses chain"""
    hist = res["history"]
    assert res["iterations"] == len(hist) >= 1 and res["reason"] in ("converged", "no_ascent", "iterations", "no_overlap")
    T = np.asarray(T0, np.float64)[:3]
    accepted = []
    for it, h in enumerate(hist):
        assert np.array_equal(h["T"], T), (what, it)
        want = ref_eval(h["T"][None])
        got = {k: np.asarray(h["derivs"][k])[None] for k in ("score", "d2_sum", "matched", "terms", "g", "H")}
        dr.assert_derivs(got, want, what=(what, it))
        assert np.array_equal(h["delta"], reg.newton_delta(h["derivs"]["g"], h["derivs"]["H"], step_t, step_r))
        cand = np.stack([reg.retract(h["T"], a * h["delta"]) for a in reg.STEPS])
        ws = ref_score(cand)
        assert np.all(np.abs(h["scores"] - ws) <= sr.RTOL * np.abs(ws)), (what, it)
        best = int(np.argmax(h["scores"]))
        if h["scores"][best] > h["derivs"]["score"]:
            assert h["a"] == reg.STEPS[best] and all(h["scores"][j] < h["scores"][best] for j in range(best))
            accepted.append(float(h["scores"][best]))
            T = cand[best]
        else:
            assert h["a"] is None and it == len(hist) - 1 and res["reason"] == "no_ascent"
    assert np.array_equal(res["T"], T)
    first = float(hist[0]["derivs"]["score"])
    assert all(b >= a for a, b in zip([first] + accepted, accepted)), (what, accepted)
    if res["reason"] == "converged":
        h = hist[-1]
        assert h["a"] * np.linalg.norm(h["delta"][:3]) < 1e-4 and h["a"] * np.linalg.norm(h["delta"][3:]) < 1e-5
    # the accepted scores rise from one iteration's evaluation to the next one's as well (the same bits: score_derivs = score_poses)
    for a, b in zip(hist, hist[1:]):
        assert b["derivs"]["score"] == a["scores"][reg.STEPS.index(a["a"])], what


def assert_recovered(T, T0, what=""):
    """the recovery condition (b): less than half the start offset off, in translation and in angle (the truth is the identity)"""
    t0, a0 = dr.pose_error(T0)
    t, a = dr.pose_error(T)
    print(what, "start %.4f m %.5f rad -> end %.5f m %.6f rad" % (t0, a0, t, a))
    assert t < 0.5 * t0 and a < 0.5 * a0, (what, t, a, t0, a0)


@pytest.mark.parametrize("nbh", [1, 7])
@pytest.mark.parametrize("scene", sorted(RECOVERY_SCENES))
def test_driver_on_the_shim_step_by_step(scene, nbh):
    cloud, m = recovery_map(scene)
    scan = np.ascontiguousarray(cloud[1:][::5])
    P = m.P
    ref_eval, ref_score = dr.callables(m.cells, m.origin, P["grid_len"], P["z_len"], scan, nbh)
    evaluate = lambda T: host_derivs(m, scan, T, nbh)
    score = lambda T: host_score(m, scan, T, nbh)["score"]
    step_t = 0.5 * P["grid_len"]
    S = starts(P)
    names = sorted(S)
    T0 = np.stack([S[k] for k in names])
    res = reg.register(evaluate, score, T0, step_t=step_t)             # the starts side by side, their calls batched
    ref = reg.register(ref_eval, ref_score, T0, step_t=step_t)         # the reference's own run
    for k, r, w in zip(names, res, ref):
        print(nbh, k, "shim:", r["reason"], r["iterations"], "restatement:", w["reason"], w["iterations"], "documented:", RECOVERY[(scene, nbh, k)])
        check_steps(r, S[k], ref_eval, ref_score, step_t, what=("shim", scene, nbh, k))
        assert_recovered(w["T"], S[k], what=("restatement", scene, nbh, k))
        assert_recovered(r["T"], S[k], what=("shim", scene, nbh, k))
    # one start alone goes the way it goes in the batch
    one = reg.register(evaluate, score, S["A"], step_t=step_t)
    assert one["reason"] == res[0]["reason"] and np.array_equal(one["T"], res[0]["T"]) and one["iterations"] == res[0]["iterations"]


def test_driver_stops_without_overlap_and_at_the_iteration_limit():
    cloud, m = _map("uniform_box")
    scan = np.ascontiguousarray(cloud[1:][::9])
    evaluate = lambda T: host_derivs(m, scan, T, 7)
    score = lambda T: host_score(m, scan, T, 7)["score"]
    far = reg.register(evaluate, score, yaw(0, (5000.0, 0, 0)), step_t=0.25)
    assert far["reason"] == "no_overlap" and far["iterations"] == 1 and far["history"][0]["delta"] is None
    assert np.array_equal(far["T"], yaw(0, (5000.0, 0, 0)))
    two = reg.register(evaluate, score, starts(m.P)["B"], step_t=0.25, max_iterations=2)
    assert two["reason"] == "iterations" and two["iterations"] == 2 and two["history"][1]["a"] is not None


# ---- 6. no CPU path ----

def test_no_cpu_fallback_for_score_derivs(native_lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import grid_ndt_amd as g
    m = g.TwoDmap(0.5, 0.5)
    m.setCloudFirst((0, 0, 0))
    with pytest.raises(g.GndtError) as e:
        m.score_derivs(np.ones((4, 3), np.float32), np.eye(4))
    assert e.value.code == 2   # GNDT_ERR_NO_DEVICE
    with pytest.raises(g.GndtError) as e:
        m.register(np.ones((4, 3), np.float32), np.eye(4))
    assert e.value.code == 2
    L = native_lib
    assert L.gndt_score_derivs(None, None, 0, 12, None, 0, None, None) == 1
    assert L.gndt_score_derivs_device(None, None, 0, 12, None, 0, None, None, None) == 1
