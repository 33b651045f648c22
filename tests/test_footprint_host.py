"""CPU tier: the footprint poses' per-pose code (grid_ndt_amd/csrc/gndt_footprint.hpp: the centre, the box, the supports, the folded
sums, the plane, the shape and the verdicts), compiled with g++ into tests/_footprint_shim.so and run one pose after another with the
wavefront's lanes in turn, against the restatement (tests/footprint_ref.py) on maps the oracle builds and on 200 random cell tables,
both weights, with and without a band.  Integers and rows for equality.  Floats within BOUND: the restatement sums sequentially in
plain fp64 and solves with LAPACK where the shim folds 64 partial sums and solves with min_eigenpair_sym3, so the two differ by
reordering and by the solver's last bits; the largest difference measured over these scenes is MEASURED, the bound 4 x that
(DESIGN.md 4.3o).  Then the properties of the answer on clouds whose answer is known beforehand, the per-pose code under the
sanitizers in a program of its own, rollouts.headings, and the product entry points refuse to run without a GPU."""
import os
import subprocess

import numpy as np
import pytest

from tests import footprint_cases as fc
from tests import footprint_ref as fr
from tests.host_emulation import HostMap, MapRows, shim_deps
from tests.test_clearance_host import random_table
from tests.test_raster_host import SCENES

HERE = os.path.dirname(os.path.abspath(__file__))
# The largest |shim - restatement| per field over the oracle scenes, the clouds of footprint_cases and the 200 random tables below, as
# this file measures and prints it (-s shows the figures).  The fp64 results differ around 1e-15 and every one of them rounded to
# the same float in these scenes, except where the value itself is far below 1: a normal component of 1e-8, the rms of a scatter that
# is flat to rounding (sqrt of a lambda that is cancellation noise), a bump of 1e-9, a slope of 1e-15 on a level floor.  A field that
# measured 0 is compared for equality.  Every bound is far below one unit in the last place of fp32 at the field's usual magnitude.
MEASURED = {"z": 0.0, "normal": 8.9e-16, "along": 1.2e-16, "across": 3.1e-17, "rms": 7.6e-11, "step_max": 0.0, "bump_max": 2.8e-17, "headroom": 0.0}
BOUND = {k: 4.0 * v for k, v in MEASURED.items()}
_seen = {k: 0.0 for k in MEASURED}
_maps = {}


def _map(name):
    if name not in _maps:
        cloud, P = SCENES[name]() if name in SCENES else CLOUDS[name]()
        _maps[name] = HostMap(cloud, P, seed=17)
    return _maps[name]


CLOUDS = {"tilted_noisy": lambda: (fc.plane_cloud(0.2, -0.1, noise=0.01), fc.PLANE_P),
          "tilted_exact": lambda: (fc.plane_cloud(0.25, 0.125), fc.PLANE_P),
          "kerb_low": lambda: (fc.kerb_cloud(0.1), fc.PLANE_P),
          "kerb_high": lambda: (fc.kerb_cloud(0.2), fc.PLANE_P)}


MAX_CLOSE = 0.05      # the share of a scene's poses that may leave the float comparison of z, normal, along and across
_close = {}           # scene -> [poses the restatement calls close, poses]


def both(t, f, poses, hl, hw, what, scene, max_close=MAX_CLOSE, tilt_undetermined=False, **kw):
    """the shim against the restatement, with the rows kept and cut -> (info, rows of the shim).  A pose whose two smallest
    eigenvalues the restatement finds closer than 1e-6 of the largest leaves the comparison of z, normal, along and across: at most
    max_close of this call's poses, and the callers check the same share over their scene as a whole."""
    grid = kw.pop("grid", {})
    want, wrows, close = f.footprints(poses, hl, hw, row_cap=32, **kw)
    got, grows = fc.run(t, poses, hl, hw, robot=f.robot, row_cap=32, **grid, **kw)
    n = _close.setdefault(scene, [0, 0])
    n[0], n[1] = n[0] + int(close.sum()), n[1] + len(poses)
    assert close.sum() <= max_close * len(poses), (what, int(close.sum()), len(poses))
    a, b = got, want
    if tilt_undetermined and close.any():
        # face_lattice alone: three collinear means without scatter leave the plane's direction undetermined, and the TILT bit, which is
        # read off the normal, with it.  On those poses flags may differ in TILT and in no other bit; every other integer stays.
        assert not ((got["flags"] ^ want["flags"])[close] & ~np.uint32(fr.TILT)).any(), what
        assert np.array_equal(got["flags"][~close], want["flags"][~close]), what
        a, b = got.copy(), want.copy()
        a["flags"][close] &= ~np.uint32(fr.TILT)
        b["flags"][close] &= ~np.uint32(fr.TILT)
    fr.same_ints(a, grows, b, wrows, what)
    diffs = fr.float_diffs(got, want, keep=~close)
    for k, v in diffs.items():
        _seen[k] = max(_seen[k], v)
        assert v <= BOUND[k], (what, k, v, BOUND[k])
    cut, crows = fc.run(t, poses, hl, hw, robot=f.robot, row_cap=2, stride=32, **grid, **kw)
    fr.same_bits(cut, crows, got, grows[:, :2], (what, "cut"))
    none, _ = fc.run(t, poses, hl, hw, robot=f.robot, **grid, **kw)
    fr.same_bits(none, None, got, None, (what, "no rows"))
    assert (got["cells"] == got["support"] + got["gaps"] + got["unknown"]).all(), what
    return got, grows


VARIANTS = (dict(), dict(weight=fr.COUNT), dict(max_dz=0.3, height=1.8, min_cover=0.8), dict(weight=fr.COUNT, max_dz=0.12, min_cells=5, height=0.6))


@pytest.mark.parametrize("name", sorted(SCENES) + ["tilted_noisy"])
def test_oracle_scenes_both_weights_with_and_without_a_band(name):
    m = _map(name)
    g = m.P["grid_len"]
    f = fr.Footprinter(m.cells, m.origin, g, m.P["z_len"])
    rng = np.random.default_rng(41)
    slopes = m.mean[(m.flags & 2) != 0]
    lo, hi = slopes[:, :2].min(0), slopes[:, :2].max(0)
    poses = np.concatenate([fc.random_poses(rng, 40, lo, hi, slopes[:, 2].min(), slopes[:, 2].max(), on=slopes), fc.mixed_batch(m, rng)])
    seen = {}
    for (hl, hw) in ((1.2 * g, 0.8 * g), (3.7 * g, 2.1 * g)):
        for kw in VARIANTS:
            got, _ = both(m, f, poses, hl, hw, (name, hl, hw, kw), name, max_close=0.0 if name in ("bridge_ground", "tilted_noisy") else MAX_CLOSE,
                          tilt_undetermined=name == "face_lattice", **kw)
            for st in got["status"].tolist():
                seen[st] = seen.get(st, 0) + 1
    print(name, dict(statuses=seen, seen=_seen, close=_close[name]))
    assert _close[name][0] <= MAX_CLOSE * _close[name][1], _close[name]
    assert seen.get(fr.OK, 0) > 0 and seen.get(fr.BAD_POSE, 0) > 0 and seen.get(fr.NO_GROUND, 0) > 0, seen


def cov_table(rng):
    """a random cell table (tests/test_clearance_host.random_table) whose rows are Gaussians: counts and scatters drawn here"""
    t = random_table(rng)
    n = t.n
    count = rng.integers(3, 200, n).astype(np.uint32)
    a = rng.normal(0.0, 1.0, (n, 3, 3)) * np.array([0.12, 0.12, 0.02])[None, :, None]
    s = np.einsum("nij,nkj->nik", a, a) * count[:, None, None]
    cov = np.stack([s[:, 0, 0], s[:, 0, 1], s[:, 0, 2], s[:, 1, 1], s[:, 1, 2], s[:, 2, 2]], 1).astype(np.float32)
    return MapRows(dict(t.cells, count=count, cov=cov), t.row_ncol)


FUZZ_GRID = dict(origin=(0.0, 0.0, 0.0), grid_len=0.5, z_len=0.25)


def test_fuzz_200_random_cell_tables():
    rng = np.random.default_rng(20251021)
    seen, flags = {}, 0
    for k in range(200):
        t = cov_table(rng)
        f = fr.Footprinter(t.cells, (0.0, 0.0, 0.0), 0.5, 0.25, robot=dict(reachable_height=0.12))
        slopes = t.mean[(t.flags & 2) != 0]
        poses = np.concatenate([fc.random_poses(rng, 8, (-4.5, -4.5), (4.5, 4.5), -0.6, 0.8, on=slopes), fc.mixed_batch(t, rng, 4)])
        hl, hw = [(0.3, 0.2), (1.0, 0.5), (0.8, 0.8), (2.0, 1.0)][k % 4]
        got, _ = both(t, f, poses, hl, hw, (k, hl, hw), "fuzz", grid=FUZZ_GRID, **VARIANTS[(k // 4) % 4])
        for st in got["status"].tolist():
            seen[st] = seen.get(st, 0) + 1
        flags |= int(np.bitwise_or.reduce(got["flags"]))
    print("fuzz:", dict(statuses=seen, flags=flags, seen=_seen, close=_close["fuzz"]))
    assert _close["fuzz"][0] <= MAX_CLOSE * _close["fuzz"][1], _close["fuzz"]
    assert all(seen.get(st, 0) > 0 for st in range(4)), seen
    assert flags == fr.TILT | fr.STEP | fr.COVER | fr.LOW, flags


# the exact plane: z = a x + b y sampled without noise.  along and across are the plane's directional slopes up to the fp32 rounding
# of the cloud and of the rows' means and scatters (measured 6.0e-8 at slopes of 0.25: one unit in
# the last place of fp32 at 0.5; 4 x that)
PLANE_MARGIN = 4 * 6.0e-8


def test_a_sampled_plane_returns_its_directional_slopes():
    a, b = 0.25, 0.125
    m = _map("tilted_exact")
    yaw = np.linspace(-np.pi, np.pi, 17)
    xyz = np.stack([np.linspace(-1.6, 1.7, 17), np.linspace(1.2, -1.9, 17), np.zeros(17)], 1)
    xyz[:, 2] = a * xyz[:, 0] + b * xyz[:, 1]
    poses = fc.headed(xyz, yaw)
    worst = 0.0
    for hl, hw, w in ((0.8, 0.6, fr.CELL), (2.0, 1.0, fr.COUNT)):
        got, _ = fc.run(m, poses, hl, hw, weight=w)
        assert (got["status"] == fr.OK).all() and ((got["flags"] & fr.TILT) == 0).all()    # (a column's levels are steps of their own)
        h = poses[:, 3:5].astype(np.float64)
        h /= np.linalg.norm(h, axis=1)[:, None]
        along, across = a * h[:, 0] + b * h[:, 1], b * h[:, 0] - a * h[:, 1]
        worst = max(worst, np.abs(got["along"] - along).max(), np.abs(got["across"] - across).max(),
                    np.abs(got["z"] - (a * poses[:, 0].astype(np.float64) + b * poses[:, 1])).max())
    print("plane: largest difference", worst)
    assert worst <= PLANE_MARGIN, worst


@pytest.mark.parametrize("name,k", [("kerb_low", 0.1), ("kerb_high", 0.2)])
def test_a_kerb_is_the_difference_of_the_two_supports_means(name, k):
    m = _map(name)
    left, right = [int(np.flatnonzero((m.sx == s) & (m.sy == 2) & ((m.flags & 2) != 0))[0]) for s in (-1, 1)]
    want = np.abs(np.float32(m.mean[right, 2] - m.mean[left, 2]))
    assert abs(float(want) - k) < 1e-6
    o = m.origin.astype(np.float64)
    poses = fc.headed([[o[0] + 0.1, o[1] + 0.75, 0.05], [o[0] - 0.2, o[1] + 0.75, 0.3]], [0.0, 2.0])
    got, rows = fc.run(m, poses, 0.6, 0.6, row_cap=16)
    assert (got["status"] == fr.OK).all()
    assert all(left in r and right in r for r in rows.tolist())
    assert (got["step_max"].view(np.uint32) == want.view(np.uint32)).all(), (got["step_max"], want)
    assert (((got["flags"] & fr.STEP) != 0) == (want > np.float32(0.15))).all()
    far, _ = fc.run(m, fc.headed([[o[0] + 2.6, o[1] + 0.75, 0.0]], [0.0]), 0.6, 0.6)
    assert far["step_max"][0] == 0 and far["flags"][0] == 0


def test_under_and_on_the_bridge_differ_by_the_poses_z_alone():
    m = _map("bridge_ground")
    at = [8.02, 3.03]
    poses = fc.headed([at + [1.0], at + [3.0]], [0.4, 0.4])
    for height, low in ((2.5, True), (1.5, False), (0.0, False)):
        got, _ = fc.run(m, poses, 0.3, 0.2, max_dz=0.5, height=height)
        assert (got["status"] == fr.OK).all() and got["centre_row"][0] != got["centre_row"][1]
        assert abs(got["z"][0] - 1.0) < 1e-3 and abs(got["z"][1] - 3.0) < 1e-3, got["z"]
        assert 1.9 < got["headroom"][0] < 2.1 and got["headroom"][1] == fr.FLT_MAX, got["headroom"]
        assert bool(got["flags"][0] & fr.LOW) == low and not got["flags"][1] & fr.LOW
        assert got["cells"][0] == got["cells"][1]


def test_the_headings_length_changes_no_bit_and_its_sign_only_the_slopes():
    m = _map("tilted_noisy")
    rng = np.random.default_rng(6)
    poses = fc.random_poses(rng, 48, (-3, -3), (3, 3), -1.0, 1.0, on=m.mean[(m.flags & 2) != 0])
    base, brows = fc.run(m, poses, 1.0, 0.5, row_cap=24, height=1.0, min_cover=0.9)
    assert (base["status"] == fr.OK).sum() > 40
    for scale in (2.0 ** -10, 2.0 ** 10):
        q = poses.copy()
        q[:, 3:5] *= np.float32(scale)
        got, rows = fc.run(m, q, 1.0, 0.5, row_cap=24, height=1.0, min_cover=0.9)
        fr.same_bits(got, rows, base, brows, scale)
    q = poses.copy()
    q[:, 3:5] = -q[:, 3:5]
    got, rows = fc.run(m, q, 1.0, 0.5, row_cap=24, height=1.0, min_cover=0.9)
    want = base.copy()
    want["along"], want["across"] = -base["along"], -base["across"]
    fr.same_bits(got, rows, want, brows, "negated")


def test_a_footprint_across_index_0_counts_the_cells_it_counts_elsewhere():
    m = _map("tilted_noisy")
    o = m.origin.astype(np.float64)
    for hl, hw, yaw in ((0.8, 0.45, 0.3), (1.9, 0.7, 2.2), (0.6, 0.35, -1.0)):
        at = [[o[0] + 0.1 + sx * 0.5, o[1] + 0.15 + sy * 0.5, 0.0] for sx, sy in ((0, 0), (-1, -1), (3, 2), (-4, 3))]
        got, _ = fc.run(m, fc.headed(at, yaw) * np.float32([1, 1, 1, 2, 2]), hl, hw, min_cells=1)
        assert (got["status"] == fr.OK).all() and (got["unknown"] == 0).all()
        assert (got["cells"] == got["cells"][0]).all() and got["cells"][0] > 1, got["cells"]


def _strip(sx_at):
    """a 3 x 3 block of single-slope columns at sx = sx_at .. sx_at + 2, sy = 1 .. 3 (origin 0, grid 0.5)"""
    sx, sy = np.meshgrid(np.arange(sx_at, sx_at + 3), np.arange(1, 4), indexing="ij")
    sx, sy = sx.ravel(), sy.ravel()
    n = len(sx)
    lin = lambda s: np.where(s > 0, s - 0.5, s + 0.5) * 0.5
    cells = dict(sx=sx, sy=sy, sz=np.ones(n, np.int32), flags=np.full(n, 3), mean=np.stack([lin(sx), lin(sy), np.full(n, 0.1)], 1),
                 normal=np.tile([0.0, 0.0, 1.0], (n, 1)), rough=np.full(n, 0.01), count=np.full(n, 9, np.uint32),
                 cov=np.tile(np.float32([0.2, 0, 0, 0.2, 0, 0.001]), (n, 1)))
    return MapRows(cells, np.ones(n, np.uint32))


def test_the_maps_edge_and_the_codecs_last_index_count_unknown():
    for sx_at in (5, 65533, -65535):
        t = _strip(sx_at)
        f = fr.Footprinter(t.cells, (0.0, 0.0, 0.0), 0.5, 0.25)
        xs = t.mean[[1, 7], 0].astype(np.float64)                 # the block's first and last column, the middle row
        poses = fc.headed([[xs[0], 0.75, 0.1], [xs[1], 0.75, 0.1]], [0.0, np.pi])
        got, _ = both(t, f, poses, 0.6, 0.3, sx_at, "strips", max_close=0.0, grid=FUZZ_GRID, min_cells=2)
        assert (got["status"] == fr.OK).all(), got["status"]
        assert (got["unknown"] > 0).all() and (got["cells"] == got["cells"][0]).all(), (sx_at, got["unknown"], got["cells"])
        assert (got["support"] + got["unknown"] == got["cells"]).all()


def test_the_per_pose_code_under_the_sanitizers():
    exe = os.path.join(HERE, "cpp", "footprint_check")
    src = os.path.join(HERE, "cpp", "footprint_check.cpp")
    csrc = os.path.join(os.path.dirname(HERE), "grid_ndt_amd", "csrc")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in shim_deps(src)):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-static-libasan", "-static-libubsan", "-I", csrc, "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    word = r.stdout.split()
    assert word[0] == "ok" and int(word[1]) > 3000 and int(word[2]) > 10000, r.stdout


def test_headings_point_at_the_next_waypoint_and_end_at_the_terminator():
    from grid_ndt_amd import rollouts
    p = np.zeros((3, 4, 3), np.float32)
    p[0, :, 0] = [0, 1, 3, 6]
    p[1, :, 1] = [0, 2, np.nan, 5]
    p[2, 1:, 0] = np.nan
    h = rollouts.headings(p)
    assert h.shape == (3, 4, 5) and h.dtype == np.float32
    assert np.array_equal(h[0, :, 3], [1, 2, 3, 3]) and not h[0, :, 4].any() and np.array_equal(h[0, :, :3], p[0])
    assert np.array_equal(h[1, :2, 3:], [[0, 2], [0, 2]]) and np.isnan(h[1, 2:]).all()
    assert np.array_equal(h[2, 0], [0, 0, 0, 1, 0]) and np.isnan(h[2, 1:]).all()
    import torch
    assert np.array_equal(rollouts.headings(torch.from_numpy(p)).numpy(), h, equal_nan=True)
    assert np.array_equal(rollouts.headings(np.concatenate([p, p[..., :1]], -1)), h, equal_nan=True)


def test_no_cpu_fallback_for_footprints(native_lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import grid_ndt_amd as g
    m = g.TwoDmap(0.5, 0.5)
    m.setCloudFirst((0, 0, 0))
    with pytest.raises(g.GndtError) as e:
        m.footprints(np.zeros((2, 5), np.float32), 0.3, 0.2, host=True)
    assert e.value.code == 2   # GNDT_ERR_NO_DEVICE
    with pytest.raises(g.GndtError) as e:
        m.footprints_along(np.zeros((2, 3, 3), np.float32), 0.3, 0.2, host=True)
    assert e.value.code == 2
