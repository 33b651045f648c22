"""CPU tier: map-to-map scoring's per-element code (grid_ndt_amd/csrc/gndt_score_maps.hpp: score_maps_sigma, score_maps_pair,
score_maps_derivs_add, score_maps_row on score_point's lookup, and the kernels' fixed summation tree restated in
tests/score_maps_shim.cpp), compiled with g++ into tests/_score_maps_shim.so, against the numpy restatement of the definition
(tests/score_maps_ref.py) on maps the oracle builds; the restatement itself against central differences of its own frozen function;
grid_ndt_amd/registration.py driven on the shim, step by step against the restatement; and the product entry points refuse to run
without a GPU.

Tolerances (derived in tests/score_maps_ref.py, not tuned): matched and terms exact; score and d2_sum at score_ref.RTOL; g and H
entry-wise within RTOL_D x the sum of the absolute values of the entry's per-pair contributions.  Finite differences: the error of g and
of H against central differences falls by at least 3x per halving of h (a second-order scheme gives 4x; the margin is for the last
halving meeting the rounding floor), at three steps from h0 = min(1e-3, sqrt(eps_min) / 10).

Recovery (measured with the numpy restatement driver, the reference): the destination is the map of the points [1::2] of the cloud,
the source the map of the points [2::2] — two samplings of one surface that share no point — once built in the destination's frame
(truth: the identity) and once from the points moved by the inverse of yaw 17 degrees, t = (3.3, -1.7, 0.4) (truth: that pose, and
no source cell aligned with a destination cell).  Starts A and B of tests/test_score_derivs_host.py composed on the truth.  RECOVERY
below has every case's final error, iterations and ending.  The tests assert that the final pose of the restatement's own run and of
the run under test is less than half the start offset off, in translation and in angle.  uniform_box start B is not a case (it
recovers with neither map-to-map nor means-as-points scoring).

The moved source is voxelised from the cloud's own origin row, as the destination is; only its points are moved.  Where a source
map's cells happen to fall matters to these starts: with the origin row taken through the inverse pose as well, the same ten runs end
6.2 - 28.2 mm off except neighbourhood 7, start B, whose first step, capped at step_t = 0.25 m, lands on a side maximum 433 mm off
(score 1280; the truth scores 4580) and stops; of 24 runs over six source origins three end that way.  A coarser
destination level in front (register_map(pyramid=...)) is the remedy, as for scans."""
import ctypes as C
import math

import numpy as np
import pytest

from grid_ndt_amd import registration as reg
from grid_ndt_amd import scenes
from tests import query_ref as qr
from tests import score_derivs_ref as dr
from tests import score_maps_ref as mr
from tests import score_ref as sr
from tests.host_emulation import MAP, HostMap, load_shim
from tests.test_score_derivs_host import RECOVERY_SCENES, check_steps, starts
from tests.test_score_host import SCENES, _map, five_poses, yaw

# the restatement driver's own endings: (scene, frame, neighbourhood, start) -> final error, iterations, reason
RECOVERY = {
    ("drivable_site", "same", 1, "A"): "3.4 mm, 0.013 mrad, 7 iterations, converged",
    ("drivable_site", "same", 7, "A"): "4.8 mm, 0.070 mrad, 8 iterations, converged",
    ("drivable_site", "same", 1, "B"): "3.4 mm, 0.013 mrad, 16 iterations, converged",
    ("drivable_site", "same", 7, "B"): "4.8 mm, 0.071 mrad, 9 iterations, converged",
    ("drivable_site", "moved", 1, "A"): "7.6 mm, 0.602 mrad, 16 iterations, no_ascent",
    ("drivable_site", "moved", 7, "A"): "8.1 mm, 0.638 mrad, 8 iterations, no_ascent",
    ("drivable_site", "moved", 1, "B"): "14.8 mm, 0.832 mrad, 22 iterations, no_ascent",
    ("drivable_site", "moved", 7, "B"): "6.8 mm, 0.120 mrad, 11 iterations, no_ascent",
    ("uniform_box", "same", 1, "A"): "2.6 mm, 0.537 mrad, 5 iterations, converged",
    ("uniform_box", "same", 7, "A"): "2.8 mm, 0.864 mrad, 5 iterations, converged",
}
TRUTH = {"same": yaw(0.0), "moved": yaw(17.0, (3.3, -1.7, 0.4))}
RECOVERY_CASES = [("drivable_site", "same", "A"), ("drivable_site", "same", "B"), ("drivable_site", "moved", "A"),
                  ("drivable_site", "moved", "B"), ("uniform_box", "same", "A")]

_shim = None


def shim():
    global _shim
    if _shim is None:
        vp, u32, u64, d = C.c_void_p, C.c_uint32, C.c_uint64, C.c_double
        _shim = load_shim("score_maps_shim.cpp", "_score_maps_shim.so", {
            "mshim_score_maps": ([C.c_int, C.c_int, MAP, vp, u32, MAP, u32, d, d, d, vp, u32, vp, vp, vp], C.c_int),
            "mshim_pair_zero_sigma": ([vp, vp, u64, MAP, u32, d, d, d, vp, vp, vp, vp], None),
        })
    return _shim


def split_cloud(cloud, first, move=None):
    """the cloud of the points [first::2] behind the origin row; move: the points taken through the inverse of that pose (the origin
    row stays, as in the setup the recovery cases were set with: the map's cells are laid out from the cloud's own first row)"""
    c = np.concatenate([cloud[:1], cloud[first::2]]).astype(np.float32)
    if move is not None:
        T = np.asarray(move, np.float64)
        c[1:, :3] = ((c[1:, :3].astype(np.float64) - T[:, 3]) @ T[:, :3]).astype(np.float32)
    return c


_halves = {}


def halves(name):
    """(destination, source) HostMaps of the points [1::2] and [2::2] of a scoring scene"""
    if name not in _halves:
        cloud, P = SCENES[name]()
        _halves[name] = (HostMap(split_cloud(cloud, 1), P), HostMap(split_cloud(cloud, 2), P))
    return _halves[name]


def host_maps(dm, sm, poses, nbh=1, derivs=True, per_node=None, **params):
    """score_maps_row over every (source row, pose) pair of two HostMaps, summed in the kernels' tree -> the dict
    TwoDmap.score_map_derivs returns (derivs=False: g and H zero), with per_node=k also d2, row and vals [rows, 27] of pose k"""
    prm = mr.defaults(**params)
    T = np.ascontiguousarray(sr.as_poses(poses)).reshape(-1, 12)
    K, n = T.shape[0], sm.n
    rec = np.zeros((K, 31), np.int64)
    d2 = np.full(n, -1.0, np.float32)
    row = np.full(n, 0xDEADBEEF, np.uint32)
    vals = np.zeros((n, 27), np.float64)
    want = per_node is not None
    p = lambda a: C.c_void_p(a.ctypes.data if want else 0)
    rc = shim().mshim_score_maps(nbh, int(derivs), sm.shim_map(), T.ctypes.data, K, dm.shim_map(), prm["min_count"], prm["cov_rel"],
                                 prm["cov_floor"], prm["max_d2"], rec.ctypes.data, per_node if want else 0xFFFFFFFF, p(d2), p(row), p(vals))
    assert rc == 0
    fl = rec.view(np.float64)
    H = np.zeros((K, 6, 6))
    for j, (a, b) in enumerate(dr.TRI):
        H[:, a, b] = H[:, b, a] = fl[:, 10 + j]
    out = {"score": fl[:, 0].copy(), "d2_sum": fl[:, 1].copy(), "matched": rec[:, 2].copy(), "terms": rec[:, 3].copy(),
           "g": fl[:, 4:10].copy(), "H": H}
    if want:
        out.update(d2=d2, row=row.view(np.int32).astype(np.int64), vals=vals)
    return out


def ref_maps(dm, sm, poses, nbh=1, per_node=None, derivs=True, **params):
    fn = mr.derivs if derivs else mr.score
    kw = dict(per_node=per_node) if not derivs else {}
    return fn(dm.cells, dm.origin, dm.P["grid_len"], dm.P["z_len"], sm.cells, poses, nbh, **kw, **params)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---- 1. the formulas: the restatement against central differences of its own frozen function ----

@pytest.mark.parametrize("nbh", [1, 7])
def test_restatement_equals_central_differences_of_the_frozen_sum(nbh):
    dm, sm = halves("uniform_box")
    P = dm.P
    T = yaw(1.0, (0.1 * P["grid_len"], -0.1 * P["grid_len"], 0.1 * P["z_len"]))       # 1 degree and a tenth of a cell off
    want = ref_maps(dm, sm, T, nbh)
    d = want["poses_out"][0]
    assert d["terms"] > 200
    em = mr.eps_min(d)
    h0 = min(1e-3, math.sqrt(em) / 10.0)
    errs = []
    for h in (h0, h0 / 2, h0 / 4):
        g, H = mr.central_differences(want["nodes"], d, h)
        errs.append((float(np.abs(g - d["g"]).max() / np.abs(d["g"]).max()), float(np.abs(H - d["H"]).max() / np.abs(d["H"]).max())))
    print("nbh", nbh, "eps_min", em, "h0", h0, "relative errors of (g, H) at h0, h0/2, h0/4:", errs)
    for a, b in zip(errs, errs[1:]):
        assert b[0] * 3.0 <= a[0] and b[1] * 3.0 <= a[1], errs
    assert errs[-1][0] < 1e-3 and errs[-1][1] < 1e-2, errs


# ---- 2. the per-pair code against the restatement ----

@pytest.mark.parametrize("nbh", [1, 7])
@pytest.mark.parametrize("name", ["bridge_ground", "face_lattice", "uniform_box"])
def test_maps_equal_the_restatement(name, nbh):
    dm, sm = halves(name)
    poses = five_poses(dm.P)
    want = ref_maps(dm, sm, poses, nbh)
    assert want["terms"][0] > 100 and (want["terms"] > 0).all()
    got = host_maps(dm, sm, poses, nbh, per_node=3)
    mr.assert_derivs(got, want, what=(name, nbh))
    assert np.abs(want["g"]).max() > 0 and (np.abs(want["H"]).max((1, 2)) > 0).all()
    assert np.array_equal(got["H"], got["H"].transpose(0, 2, 1))
    # every source row's own 27 values (the sum over its candidates), and its nearest destination row
    wp = want["poses_out"][3]
    src = want["source"]
    assert 0 < len(src.idx) < sm.n or name == "face_lattice"           # (rows without statistics sit among the counted ones)
    assert not got["vals"][~src.counted].any()
    assert np.all(np.abs(got["vals"][src.idx] - wp["vals"].sum(1)) <= mr.RTOL_D * np.abs(wp["vals"]).sum(1))
    mr.assert_per_node(got["d2"], got["row"], wp, what=(name, nbh))
    # the score-only kernel's record: the derivatives' first four fields to the bit, the same per-node outputs
    plain = host_maps(dm, sm, poses, nbh, derivs=False, per_node=3)
    for k in ("score", "d2_sum"):
        assert np.array_equal(_bits(got[k]), _bits(plain[k])), k
    for k in ("matched", "terms", "row"):
        assert np.array_equal(got[k], plain[k]), k
    assert np.array_equal(got["d2"].view(np.uint32), plain["d2"].view(np.uint32))
    assert not plain["g"].any() and not plain["H"].any()
    mr.assert_pose_sums(plain, ref_maps(dm, sm, poses, nbh, derivs=False), what=(name, nbh, "score"))


# ---- 3. Sigma = 0: scan scoring's bits ----

@pytest.mark.parametrize("name", ["bridge_ground", "uniform_box"])
def test_zero_sigma_pair_has_score_nodes_bits(name):
    cloud, m = _map(name)
    prm = sr.defaults()
    rng = np.random.default_rng(8)
    rows = rng.integers(0, m.n, size=5000).astype(np.uint32)
    q = (np.asarray(m.cells["mean"], np.float32)[rows] + rng.normal(scale=0.2, size=(len(rows), 3))).astype(np.float32)
    count = m.count
    for gate in (0.0, 4.0):
        pd, nd = np.zeros(len(rows)), np.zeros(len(rows))
        pk, nk = np.zeros(len(rows), np.uint8), np.zeros(len(rows), np.uint8)
        shim().mshim_pair_zero_sigma(q.ctypes.data, rows.ctypes.data, len(rows), m.shim_map(), prm["min_count"], prm["cov_rel"],
                                     prm["cov_floor"], gate, pd.ctypes.data, nd.ctypes.data, pk.ctypes.data, nk.ctypes.data)
        enough = count[rows] >= prm["min_count"]
        assert enough.sum() > 1000 and np.array_equal(pk, nk)
        assert np.array_equal(pd[enough].view(np.uint64), nd[enough].view(np.uint64))
        assert (pk != 0).sum() < enough.sum() if gate else np.array_equal(pk != 0, enough)


# ---- 4. a map against itself at the identity: exact ----

@pytest.mark.parametrize("name", ["uniform_box", "bridge_ground"])
def test_self_score_at_the_identity_is_exact(name):
    cloud, m = _map(name)
    prm = mr.defaults()
    src = mr.Source(m.cells, prm)
    # the premise: every counted row's fp32 mean keys into the row's own cell
    sx, sy, sz, _, ok = qr.keys(src.mean[src.idx], m.origin, m.P["grid_len"], m.P["z_len"])
    assert ok.all() and np.array_equal(sx, m.sx[src.idx]) and np.array_equal(sy, m.sy[src.idx]) and np.array_equal(sz, m.sz[src.idx])
    assert len(src.idx) > 100
    got = host_maps(m, m, yaw(0), 1, per_node=0)
    assert got["score"][0] == float(len(src.idx)) and int(got["terms"][0]) == int(got["matched"][0]) == len(src.idx)
    assert got["d2_sum"][0] == 0.0 and not got["g"][0].any()
    assert np.array_equal(got["row"][src.idx], src.idx) and not got["d2"][src.idx].any()
    assert np.isnan(got["d2"][~src.counted]).all() and (got["row"][~src.counted] == sr.NO_ROW).all()


# ---- 5. nothing to match: exact zeros; the gate ----

def test_nan_pose_off_the_map_and_the_gate():
    dm, sm = halves("uniform_box")
    bad = yaw(0)
    bad[2, 0] = np.nan
    poses = np.stack([yaw(0.5), yaw(0, (5000.0, 0, 0)), bad])
    for nbh in (1, 7):
        got = host_maps(dm, sm, poses, nbh)
        for k in (1, 2):
            assert got["score"][k] == 0.0 and got["d2_sum"][k] == 0.0 and got["matched"][k] == 0 and got["terms"][k] == 0
            assert not got["g"][k].any() and not got["H"][k].any() and np.isfinite(got["H"][k]).all()
        assert got["terms"][0] > 100
        gate = 4.0
        want = ref_maps(dm, sm, poses, nbh, max_d2=gate)
        assert sr.gate_margin(want["poses_out"], gate) > 1e-6
        g2 = host_maps(dm, sm, poses, nbh, max_d2=gate, per_node=0)
        mr.assert_derivs(g2, want, what=("gate", nbh))
        mr.assert_per_node(g2["d2"], g2["row"], want["poses_out"][0], what=("gate", nbh))
        assert 0 < g2["terms"][0] < got["terms"][0]
        assert float(g2["d2"][np.isfinite(g2["d2"])].max()) <= gate


# ---- 6. the driver on the shim, step by step against the restatement; recovery ----

_rmaps = {}


def recovery_maps(scene, frame):
    """(destination, source) HostMaps of a recovery case and the truth pose"""
    if (scene, frame) not in _rmaps:
        cloud, P = RECOVERY_SCENES[scene]()
        _rmaps[(scene, frame)] = (HostMap(split_cloud(cloud, 1), P),
                                  HostMap(split_cloud(cloud, 2, None if frame == "same" else TRUTH[frame]), P))
    return _rmaps[(scene, frame)] + (TRUTH[frame],)


def compose(S, G):
    """S after G, both [3, 4]"""
    return np.concatenate([S[:, :3] @ G[:, :3], (S[:, :3] @ G[:, 3] + S[:, 3])[:, None]], 1)


def assert_recovered(T, T0, truth, what=""):
    """the recovery condition: less than half the start offset off the truth, in translation and in angle"""
    t0, a0 = dr.pose_error(T0, truth)
    t, a = dr.pose_error(T, truth)
    print(what, "start %.4f m %.5f rad -> end %.5f m %.6f rad" % (t0, a0, t, a))
    assert t < 0.5 * t0 and a < 0.5 * a0, (what, t, a, t0, a0)
    return t, a


@pytest.mark.parametrize("nbh", [1, 7])
@pytest.mark.parametrize("scene,frame,start", RECOVERY_CASES)
def test_driver_on_the_shim_step_by_step(scene, frame, start, nbh):
    dm, sm, truth = recovery_maps(scene, frame)
    P = dm.P
    ref_eval, ref_score = mr.callables(dm.cells, dm.origin, P["grid_len"], P["z_len"], sm.cells, nbh)
    evaluate = lambda T: host_maps(dm, sm, T, nbh)
    score = lambda T: host_maps(dm, sm, T, nbh, derivs=False)["score"]
    step_t = 0.5 * P["grid_len"]
    T0 = compose(starts(P)[start], truth)
    r = reg.register(evaluate, score, T0, step_t=step_t)
    w = reg.register(ref_eval, ref_score, T0, step_t=step_t)           # the reference's own run
    what = (scene, frame, nbh, start)
    check_steps(r, T0, ref_eval, ref_score, step_t, what=("shim",) + what)
    t, a = dr.pose_error(w["T"], truth)
    print("measured: %r: \"%.1f mm, %.3f mrad, %d iterations, %s\"," % (what, 1e3 * t, 1e3 * a, w["iterations"], w["reason"]),
          "documented:", RECOVERY[what])
    assert_recovered(w["T"], T0, truth, what=("restatement",) + what)
    assert_recovered(r["T"], T0, truth, what=("shim",) + what)


# ---- 7. no CPU path ----

def test_no_cpu_fallback_for_score_maps(native_lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import grid_ndt_amd as g
    m = g.TwoDmap(0.5, 0.5)
    m.setCloudFirst((0, 0, 0))
    for call in (lambda: m.score_map(m, np.eye(4)), lambda: m.score_map_derivs(m, np.eye(4)), lambda: m.register_map(m, np.eye(4)),
                 lambda: m.stitch(m, np.eye(4), method="d2d")):
        with pytest.raises(g.GndtError) as e:
            call()
        assert e.value.code == 2   # GNDT_ERR_NO_DEVICE
    L = native_lib
    assert L.gndt_score_maps_device(None, None, None, 0, None, None, None, None, None) == 1
    assert L.gndt_score_maps_derivs_device(None, None, None, 0, None, None, None) == 1
