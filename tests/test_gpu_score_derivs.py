"""GPU tier: the scan score derivatives on the device-resident grid (gndt_score_derivs_device / gndt_score_derivs,
TwoDmap.score_derivs) against the numpy restatement of the definition (tests/score_derivs_ref.py) on the exported cells: every
accumulate strategy, both neighbourhoods, a batch of poses; score, d2_sum, matched and terms are score_poses' bits; all 31 fields are
the same bits from run to run, in a batch or one pose at a time, at either stride, on any stream and when a batch is launched in
groups of poses; the entry points' error codes; the map is left as it was; and TwoDmap.register on the device, every recorded step
against the rule and the restatement.

Tolerances (derived, not tuned) are the CPU tier's (tests/test_score_derivs_host.py): matched and terms exact, score and d2_sum at
score_ref.RTOL, g and H entry-wise within score_derivs_ref.RTOL_D x the sum of the absolute values of the entry's terms.

Recovery: the cases and the restatement driver's own endings are tests/test_score_derivs_host.py's (RECOVERY there: uniform_box and
drivable_site, every 5th point, starts A and B a quarter of a metre and up to 2 degrees off; the restatement ends within 9.1 mm /
2.3 mrad of the truth in every case); the device's final pose is held to the same condition, less than half the start offset off."""
import ctypes as C

import numpy as np
import pytest

from grid_ndt_amd import scenes
from tests import score_derivs_ref as dr
from tests import score_ref as sr
from tests.gpu_kit import dev, handle, to_np
from tests.test_gpu_score import ATOMIC, AUTO, BOX, ERR_INVALID, PARTITION, TERRAIN, TILE, _built, six_poses, yaw
from tests.test_gpu_score import _bits as _score_bits

pytestmark = pytest.mark.gpu


def _ref(m, cloud, P, scan, poses, nbh, **kw):
    return dr.derivs(m.export(), cloud[0], P["grid_len"], P["z_len"], scan, poses, nbh, **kw)


def _bits(out):
    """all 31 fields of a result as integers (H by its 21 upper-triangle values)"""
    o = to_np(out)
    f = lambda a: np.ascontiguousarray(a, np.float64).view(np.uint64).tolist()
    H = np.stack([o["H"][:, a, b] for a, b in dr.TRI], 1)
    assert np.array_equal(o["H"], np.transpose(o["H"], (0, 2, 1)))
    return (f(o["score"]), f(o["d2_sum"]), o["matched"].tolist(), o["terms"].tolist(), f(o["g"]), f(H))


def _pose(bits, k):
    return [v[k] for v in bits]


# ---- 1. against the restatement ----

@pytest.mark.parametrize("strategy", [ATOMIC, PARTITION, TILE, AUTO])
@pytest.mark.parametrize("name", ["bridge_ground", "uniform_box", "terrain", "face_lattice"])
def test_derivs_equal_the_restatement(name, strategy):
    cloud, P, m = _built(name, strategy)
    scan = np.ascontiguousarray(cloud[1:][::5])
    t = dev(scan)
    poses = six_poses(P)
    for nbh in (1, 7):
        want = _ref(m, cloud, P, scan, poses, nbh)
        assert want["terms"][0] > 100 and (want["terms"][:4] > 0).all()
        got = to_np(m.score_derivs(t, poses, neighbourhood=nbh))
        dr.assert_derivs(got, want, what=(name, strategy, nbh))
        assert got["g"].shape == (6, 6) and got["H"].shape == (6, 6, 6) and np.array_equal(got["H"], got["H"].transpose(0, 2, 1))
        assert (np.abs(got["H"][:4]).max((1, 2)) > 0).all()
        # off the map, and the pose with a NaN: every field exactly 0
        for j in (4, 5):
            assert got["score"][j] == 0.0 and got["d2_sum"][j] == 0.0 and got["matched"][j] == 0 and got["terms"][j] == 0
            assert not got["g"][j].any() and not got["H"][j].any() and np.isfinite(got["H"][j]).all()
        # the four sums: score_poses' bits
        assert _score_bits(got) == _score_bits(m.score_poses(t, poses, neighbourhood=nbh))


# ---- 2. bits ----

def test_results_are_the_same_bits_every_way():
    import torch
    cloud, P, m = _built("terrain")
    scan = np.ascontiguousarray(cloud[1:][::3])
    t3, t4 = dev(scan[:, :3]), dev(scenes.with_stride4(scan[:, :3]))
    poses = six_poses(P)
    for nbh in (1, 7):
        plain = _score_bits(m.score_poses(t3, poses, neighbourhood=nbh))
        b0 = _bits(m.score_derivs(t3, poses, neighbourhood=nbh))
        assert b0[3][0] > 1000 and list(b0[:4]) == list(plain)
        for _ in range(2):
            assert _bits(m.score_derivs(t3, poses, neighbourhood=nbh)) == b0
        for k in range(6):                                          # a batch of 6 = six single-pose calls
            assert _pose(_bits(m.score_derivs(t3, poses[k], neighbourhood=nbh)), 0) == _pose(b0, k), (nbh, k)
        assert _bits(m.score_derivs(t4, poses, neighbourhood=nbh)) == b0                    # stride 12 = stride 16
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        other = m.score_derivs(t3, poses, neighbourhood=nbh, stream=s)
        s.synchronize()
        assert _bits(other) == b0                                                            # another stream = the handle's
        assert _score_bits(m.score_poses(t3, poses, neighbourhood=nbh)) == plain             # score_poses keeps its bits afterwards
        moved = sr.transform(poses[3], scan)                                                 # pose T on cloud P = identity on fl32(T P)
        assert _pose(_bits(m.score_derivs(dev(moved), yaw(0), neighbourhood=nbh)), 0) == _pose(b0, 3)


def test_a_batch_launched_in_groups_of_poses_has_the_single_calls_bits():
    """3 M points are 11 719 tiles, 2.8 MB of partial sums a pose: 30 poses exceed what one launch's scratch takes (64 MiB, 23
    poses), so the batch goes in two groups — pose k's record is what a single-pose call gives"""
    cloud = scenes.uniform_box(3_000_001)
    m = handle(BOX, max_nodes_hint=1 << 20)
    m.setCloudFirst(cloud[0])
    t = dev(cloud[1:])
    m.create2DMap("slope", t)
    rng = np.random.default_rng(9)
    poses = np.stack([yaw(float(a), (float(x), float(y), 0.0)) for a, x, y in zip(rng.uniform(-1, 1, 30), rng.uniform(-.2, .2, 30), rng.uniform(-.2, .2, 30))])
    bb = _bits(m.score_derivs(t, poses))
    assert min(bb[3]) > 1_000_000
    assert list(bb[:4]) == list(_score_bits(m.score_poses(t, poses)))
    for k in (0, 1, 22, 23, 29):
        assert _pose(_bits(m.score_derivs(t, poses[k])), 0) == _pose(bb, k), k


# ---- 3. the host entry point, empty inputs, the error codes, capture ----

def _raw(m, pts, poses, K, prm, out=True, host=False, stride=12, n=None, stream=None):
    """the C entry point itself -> rc"""
    import torch
    from grid_ndt_amd._lib import ScoreParams
    n = len(pts) if n is None and pts is not None else (n or 0)
    p = ScoreParams(*prm) if prm is not None else None
    if host:
        rec = np.zeros((max(K, 1), 31), np.int64)
        ptr = lambda x: C.c_void_p(x.ctypes.data)
        return m._L.gndt_score_derivs(m._h, ptr(pts) if pts is not None else None, n, stride, ptr(poses) if poses is not None else None, K,
                                      C.byref(p) if prm is not None else None, ptr(rec) if out else None)
    rec = torch.zeros((max(K, 1), 31), dtype=torch.int64, device="cuda")
    tp = dev(pts) if pts is not None else None
    tq = torch.from_numpy(poses).cuda() if poses is not None else None
    ptr = lambda x: C.c_void_p(x.data_ptr())
    rc = m._L.gndt_score_derivs_device(m._h, ptr(tp) if tp is not None else None, n, stride, ptr(tq) if tq is not None else None, K,
                                       C.byref(p) if prm is not None else None, ptr(rec) if out else None, stream)
    torch.cuda.synchronize()
    return rc


def test_host_entry_point_empty_inputs_and_errors():
    import torch
    import grid_ndt_amd as g
    from grid_ndt_amd._lib import PoseDerivs, ScoreParams
    assert C.sizeof(PoseDerivs) == 248
    cloud, P, m = _built("terrain", ATOMIC)
    scan = np.ascontiguousarray(cloud[1:][::4])
    poses = six_poses(P)
    for nbh in (1, 7):
        on_dev = m.score_derivs(dev(scan), poses, neighbourhood=nbh, max_d2=9.0)
        host = m.score_derivs(scan, poses, neighbourhood=nbh, max_d2=9.0)
        assert isinstance(host["H"], np.ndarray) and _bits(on_dev) == _bits(host) and _bits(host)[3][0] > 1000
    # n == 0 with K > 0: K zeroed records; K == 0: nothing
    for pts in (dev(np.zeros((0, 3), np.float32)), np.zeros((0, 3), np.float32)):
        out = to_np(m.score_derivs(pts, poses))
        assert len(out["score"]) == 6 and out["H"].shape == (6, 6, 6)
        assert not any(np.asarray(out[k]).any() for k in ("score", "d2_sum", "matched", "terms", "g", "H"))
    T = np.ascontiguousarray(poses.reshape(6, 12))
    ok = (1, 0, 0.0, 0.0, 0.0, 0)
    for host in (False, True):
        assert _raw(m, scan, T, 0, ok, host=host) == 0
        assert _raw(m, scan, None, 0, ok, out=False, host=host) == 0
        assert _raw(m, scan, T, 6, ok, host=host) == 0
        assert _raw(m, scan, T, 6, (1, 0, 0.0, 0.0, 0.0, 99), host=host) == 0                # (point_pose is ignored)
        # the refusals
        assert _raw(m, None, T, 6, ok, n=5, host=host) == ERR_INVALID                        # null points with n > 0
        assert _raw(m, scan, None, 6, ok, host=host) == ERR_INVALID                          # null poses
        assert _raw(m, scan, T, 6, ok, out=False, host=host) == ERR_INVALID                  # null out
        assert _raw(m, scan, T, 6, None, host=host) == ERR_INVALID                           # null params
        assert _raw(m, scan, T, 6, ok, stride=8, host=host) == ERR_INVALID
        assert _raw(m, scan, T, 6, ok, stride=20, host=host) == ERR_INVALID
        for nbh in (0, 2, 6, 27, -1):
            assert _raw(m, scan, T, 6, (nbh, 0, 0.0, 0.0, 0.0, 0), host=host) == ERR_INVALID
        for mc in (1, 2, -3):
            assert _raw(m, scan, T, 6, (1, mc, 0.0, 0.0, 0.0, 0), host=host) == ERR_INVALID
        assert _raw(m, scan, T, 6, (1, 3, 0.0, 0.0, 0.0, 0), host=host) == 0
        for bad in (-1.0, float("nan"), float("inf")):
            for slot in (2, 3, 4):
                prm = [1, 0, 0.0, 0.0, 0.0, 0]
                prm[slot] = bad
                assert _raw(m, scan, T, 6, tuple(prm), host=host) == ERR_INVALID, (bad, slot)
    big = np.ascontiguousarray(np.tile(T[:1], (65536, 1)))
    assert _raw(m, scan[:64], big, 65536, ok) == ERR_INVALID                                 # K above the grid's y limit
    assert _raw(m, scan[:64], big, 65535, ok) == 0
    assert m._L.gndt_score_derivs_device(None, None, 0, 12, None, 0, None, None, None) == ERR_INVALID
    assert m._L.gndt_score_derivs(None, None, 0, 12, None, 0, None, None) == ERR_INVALID
    # no finished build
    e = handle(TERRAIN)
    e.setCloudFirst((0.0, 0.0, 0.0))
    with pytest.raises(g.GndtError) as err:
        e.score_derivs(dev(scan), poses)
    assert err.value.code == ERR_INVALID
    # a capturing stream: refused, and the capture goes on
    want = _bits(m.score_derivs(dev(scan), poses))
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    x = torch.zeros(16, device="cuda")
    tp, tq = dev(scan), torch.from_numpy(T).cuda()
    rec = torch.zeros((6, 31), dtype=torch.int64, device="cuda")
    prm = ScoreParams(*ok)
    torch.cuda.synchronize()
    with g.graph_capture(graph, stream=s):
        rc = m._L.gndt_score_derivs_device(m._h, C.c_void_p(tp.data_ptr()), len(scan), 12, C.c_void_p(tq.data_ptr()), 6, C.byref(prm),
                                           C.c_void_p(rec.data_ptr()), C.c_void_p(s.cuda_stream))
        x.add_(1.0)
    assert rc == ERR_INVALID
    graph.replay()
    torch.cuda.synchronize()
    assert float(x[0]) == 1.0
    assert _bits(m.score_derivs(dev(scan), poses)) == want


# ---- 4. the map is untouched ----

@pytest.mark.parametrize("strategy", [ATOMIC, PARTITION])
def test_the_map_is_untouched(strategy):
    cloud, P, m = _built("terrain", strategy)
    before = m.export()
    counts = m.sync()
    scan = np.ascontiguousarray(cloud[1:][::3])
    old = _score_bits(m.score_poses(dev(scan), six_poses(P), neighbourhood=7))
    for nbh in (1, 7):
        m.score_derivs(dev(scan), six_poses(P), neighbourhood=nbh)
        m.score_derivs(scan, six_poses(P), neighbourhood=nbh)
    assert _score_bits(m.score_poses(dev(scan), six_poses(P), neighbourhood=7)) == old
    after = m.export()
    assert m.sync() == counts
    assert before.keys() == after.keys()
    for k in before:
        a, b = np.asarray(before[k]), np.asarray(after[k])
        assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b), k


# ---- 5. TwoDmap.register on the device, step by step ----

@pytest.mark.parametrize("nbh", [1, 7])
@pytest.mark.parametrize("scene", ["drivable_site", "uniform_box"])
def test_register_on_the_device_step_by_step(scene, nbh):
    import torch
    from tests.test_score_derivs_host import RECOVERY_SCENES, assert_recovered, check_steps, starts
    cloud, P = RECOVERY_SCENES[scene]()
    m = handle(P)
    m.setCloudFirst(cloud[0])
    m.create2DMap("slope", dev(cloud[1:]))
    scan = np.ascontiguousarray(cloud[1:][::5])
    t = dev(scan)
    ref_eval, ref_score = dr.callables(m.export(), cloud[0], P["grid_len"], P["z_len"], scan, nbh)
    S = starts(P)
    names = sorted(S)
    T0 = np.stack([S[k] for k in names])
    res = m.register(t, T0, neighbourhood=nbh)                       # the starts side by side
    step_t = 0.5 * P["grid_len"]
    for k, r in zip(names, res):
        print(nbh, k, "device:", r["reason"], r["iterations"])
        check_steps(r, S[k], ref_eval, ref_score, step_t, what=("device", scene, nbh, k))
        assert_recovered(r["T"], S[k], what=("device", scene, nbh, k))
    # one start, on a stream of its own, from host points as well
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    one = m.register(t, S["B"], neighbourhood=nbh, stream=s)
    check_steps(one, S["B"], ref_eval, ref_score, step_t, what=("device, one start", nbh))
    assert_recovered(one["T"], S["B"], what=("device, one start", nbh))
    host = m.register(scan, S["B"], neighbourhood=nbh, max_iterations=2)
    assert host["iterations"] <= 2 and [h["a"] for h in host["history"]] == [h["a"] for h in one["history"][:len(host["history"])]]
