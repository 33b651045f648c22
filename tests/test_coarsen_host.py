"""CPU tier: map coarsening's per-node code (grid_ndt_amd/csrc/gndt_coarsen.hpp, compiled with g++ into tests/_coarsen_shim.so)
against the codec at the multiplied lengths and against the numpy restatement (tests/coarsen_ref.py); the coarsened map against a
build at the coarse lengths, on the host emulation of the pipeline; grid_ndt_amd.registration.register_pyramid on host builds of the
scan score's per-element code; and the entry point refuses a null handle.

Tolerances (derived in tests/coarsen_ref.py, not tuned): keys, counts, first-seen indices, the node order and the flags exact; the
shim's shifted sums bit for bit the restatement's; a parent's nine sums within (2 m + 3 j + 8) 2^-53 x the sum of the absolute values
of what is added up (m points, j children)."""
import ctypes as C
import itertools

import numpy as np
import pytest

from grid_ndt_amd import registration as reg
from grid_ndt_amd import scenes
from tests import coarsen_ref as cr
from tests import host_emulation as he
from tests import score_derivs_ref as dr
from tests.host_emulation import HostMap, load_shim
from tests.test_score_derivs_host import check_steps, host_derivs, recovery_map, starts
from tests.test_score_host import host_score, yaw

FACTORS = (1, 2, 4, 8, 1024)
_shim = None


def shim():
    global _shim
    if _shim is None:
        vp, f, u64 = C.c_void_p, C.c_float, C.c_uint64
        _shim = load_shim("coarsen_shim.cpp", "_coarsen_shim.so", {
            "cshim_parent_index": ([C.c_int, C.c_int], C.c_int),
            "cshim_parent_keys": ([vp, u64, C.c_int, C.c_int, vp], None),
            "cshim_coarsen": ([vp, vp, vp, u64, C.c_int, C.c_int, vp, f, f, f, f, vp, vp], None),
        })
    return _shim


def shim_parent_keys(keys, fxy, fz):
    keys = np.ascontiguousarray(keys, np.uint64)
    out = np.zeros_like(keys)
    shim().cshim_parent_keys(keys.ctypes.data, keys.size, fxy, fz, out.ctypes.data)
    return out


def point_keys(pts, o, gl, zl):
    """the codec's own keys (point_key through tests/host_math_shim.cpp) and their ok flags"""
    pts = np.ascontiguousarray(pts, np.float32)
    keys = np.zeros(pts.shape[0], np.uint64)
    ok = np.zeros(pts.shape[0], np.uint8)
    he.shim().shim_point_keys(C.c_void_p(pts.ctypes.data), C.c_uint64(pts.shape[0]), C.c_int(3), (C.c_float * 3)(*[float(v) for v in o]),
                              C.c_float(gl), C.c_float(zl), C.c_void_p(keys.ctypes.data), C.c_void_p(ok.ctypes.data))
    return keys, ok != 0


# ---- 1. the key identity: parent_key of a point's fine key is the point's key at the multiplied lengths ----

def lattice_adversarial(rng, o, gl, zl, n=12000):
    """tests/test_host_math.py's sets (points on cell boundaries, 1, 2, 3, 5 ulps either side of them, and anywhere), plus points whose
    offset from the origin is EXACTLY a whole number of cells in fp32, points on the origin's own planes, and the origin itself"""
    o = np.float32(o)
    k = rng.integers(1, 60000, size=(n, 3)).astype(np.float64)
    sign = rng.choice([-1.0, 1.0], size=k.shape)
    lens = np.array([gl, gl, zl], np.float64)
    base = (o.astype(np.float64) + sign * k * lens).astype(np.float32)
    pts = [base]
    for steps in (1, 2, 3, 5):
        pts.append(np.nextafter(base, np.float32(np.inf)) if steps == 1 else base + np.spacing(base) * steps)
        pts.append(np.nextafter(base, np.float32(-np.inf)) if steps == 1 else base - np.spacing(base) * steps)
    pts.append((o + (rng.random((n, 3)) * 2 - 1) * np.float32([3000, 3000, 50])).astype(np.float32))
    # exactly on planes: small whole numbers of cells, every multiple of the factors among them, added in fp32 as the codec subtracts
    m = rng.integers(-4100, 4101, size=(n, 3)).astype(np.float32)
    pts.append(o + m * np.float32([gl, gl, zl]))
    on = (o + (rng.random((n // 4, 3)) * 2 - 1) * np.float32([300, 300, 20])).astype(np.float32)
    for a in range(3):                                 # one coordinate equal to the origin's: on its plane
        q = on.copy()
        q[:, a] = o[a]
        pts.append(q)
    pts.append(np.tile(o, (3, 1)))
    pts.append(np.stack([np.nextafter(o, np.float32(np.inf)), np.nextafter(o, np.float32(-np.inf))]))
    return np.ascontiguousarray(np.concatenate(pts, 0), np.float32)


SETTINGS = ((0.5, 0.1, (0.0, 0.0, 0.0)), (0.2, 0.2, (1.37, -2.11, 0.3)), (0.1, 0.05, (-7.3, 4.4, 1.0)),
            (1.0 / 3.0, 0.07, (0.013, -0.021, 0.44)), (0.3, 0.3, (100.25, -200.5, 3.0)))


@pytest.mark.parametrize("setting", range(len(SETTINGS)))
def test_parent_key_is_the_point_key_at_the_multiplied_lengths(setting):
    gl, zl, origin = SETTINGS[setting]
    rng = np.random.default_rng(100 + setting)
    pts = lattice_adversarial(rng, origin, gl, zl)
    fine, ok = point_keys(pts, origin, gl, zl)
    assert ok.sum() > 0.9 * ok.size
    total = 0
    for fxy, fz in itertools.product(FACTORS, FACTORS):
        coarse, ok_c = point_keys(pts, origin, float(cr.coarse_len(gl, fxy)), float(cr.coarse_len(zl, fz)))
        assert ok_c[ok].all()
        got = shim_parent_keys(fine[ok], fxy, fz)
        bad = np.flatnonzero(got != coarse[ok])
        assert bad.size == 0, (fxy, fz, bad.size, pts[ok][bad[:3]], he.unpack(fine[ok][bad[:3]]))
        assert np.array_equal(cr.parent_keys(fine[ok], fxy, fz), got)
        total += int(ok.sum())
    print("setting", setting, "points x factor pairs checked:", total)


def test_parent_key_at_the_edges_of_the_key_range():
    """|s| = 1 and the largest indices of each axis, both signs: by integer arithmetic, and as points through the codec"""
    edge_xy = [1, -1, 2, -2, 3, -3, 1023, 1024, 1025, -1023, -1024, -1025, 65534, -65534, 65535, -65535]
    edge_z = [1, -1, 2, -2, 1024, -1025, (1 << 21) - 2, -((1 << 21) - 2), (1 << 21) - 1, -((1 << 21) - 1)]
    for s in edge_xy + edge_z:
        for f in FACTORS:
            want = (1 if s > 0 else -1) * (-(-abs(s) // f))
            assert shim().cshim_parent_index(s, f) == want and int(cr.parent_index(s, f)) == want and want != 0
    sx, sy, sz = (np.array(v) for v in zip(*itertools.product(edge_xy, edge_xy[::3], edge_z)))
    keys = cr.pack(sx, sy, sz)
    for fxy, fz in itertools.product(FACTORS, FACTORS):
        gx, gy, gz = he.unpack(shim_parent_keys(keys, fxy, fz))
        assert np.array_equal(gx, cr.parent_index(sx, fxy)) and np.array_equal(gy, cr.parent_index(sy, fxy))
        assert np.array_equal(gz, cr.parent_index(sz, fz))
    # the same cells as points: the centre of cell s, at lengths whose products are exact in fp32, origin 0
    gl = zl = 0.5
    half = lambda s: (abs(s) - 0.5) * (1 if s > 0 else -1)
    pts = np.float32([[half(x) * gl, half(y) * gl, half(z) * zl] for x, y, z in zip(sx, sy, sz)])
    fine, ok = point_keys(pts, (0, 0, 0), gl, zl)
    assert ok.all() and np.array_equal(fine, keys)
    for fxy, fz in itertools.product(FACTORS, FACTORS):
        coarse, ok_c = point_keys(pts, (0, 0, 0), gl * fxy, zl * fz)
        assert ok_c.all() and np.array_equal(shim_parent_keys(fine, fxy, fz), coarse)


# ---- 2. the moment shift: the shim's bits are the restatement's ----

def test_coarsen_sums_equal_the_restatement_bit_for_bit():
    rng = np.random.default_rng(5)
    n = 50000
    for (gl, zl, origin), (fxy, fz) in zip(SETTINGS, ((2, 2), (4, 2), (1, 8), (1024, 1), (8, 1024))):
        sx = rng.integers(1, 65536, n) * rng.choice([-1, 1], n)
        sy = rng.integers(1, 3000, n) * rng.choice([-1, 1], n)
        sz = rng.integers(1, 1 << 21, n) * rng.choice([-1, 1], n)
        sx[:4], sy[:4], sz[:4] = [1, -1, 65535, -65535], [1, -1, 1, -1], [1, -1, (1 << 21) - 1, -((1 << 21) - 1)]
        keys = cr.pack(sx, sy, sz)
        count = rng.integers(1, 100000, n).astype(np.uint32)
        count[:8] = [1, 2, 3, 1, 0xFFFFFFFF, 1 << 31, 7, 1]
        sums = rng.normal(size=(n, 9)) * 10.0 ** rng.integers(-12, 6, size=(n, 1))
        sums[:2] = 0.0
        o = np.float32(origin)
        d = np.zeros((n, 3))
        out = np.zeros((n, 9))
        shim().cshim_coarsen(keys.ctypes.data, count.ctypes.data, sums.ctypes.data, n, fxy, fz, o.ctypes.data, gl, zl,
                             float(cr.coarse_len(gl, fxy)), float(cr.coarse_len(zl, fz)), d.ctypes.data, out.ctypes.data)
        wd = cr.delta(keys, fxy, fz, o, gl, zl)
        assert np.array_equal(d.view(np.uint64), wd.view(np.uint64))
        want = cr.shift(count, sums, wd)
        assert np.array_equal(out.view(np.uint64), want.view(np.uint64)), (fxy, fz)
        # a child's centre lies within its parent: |delta| <= (f - 1) / 2 cells
        lim = np.array([(fxy - 1) * 0.5 * gl, (fxy - 1) * 0.5 * gl, (fz - 1) * 0.5 * zl]) * (1 + 1e-6) + 1e-9
        assert (np.abs(wd) <= lim).all()
        if fxy == 1:
            assert not d[:, :2].any()


# ---- 3. map level: the coarsened statistics finalise to the map of a build at the coarse lengths ----

MAP_SCENES = {
    "uniform_box": lambda: (scenes.uniform_box(40_001, half_xy=6.0, half_z=1.0), dict(grid_len=0.5, z_len=0.5, slope_interval=0.08)),
    "campus_frame": lambda: (scenes.campus_frame(20_000), scenes.CAMPUS_PARAMS),
}
_fine = {}


def fine_stats(name):
    """(cloud, P, accumulate's tuple at the fine lengths, the sums of the absolute values of its terms), made once"""
    if name not in _fine:
        cloud, P = MAP_SCENES[name]()
        body, o = cloud[1:], cloud[0, :3]
        t = he.accumulate(body, o, P["grid_len"], P["z_len"])
        keys, ok = point_keys(body[:, :3], o, P["grid_len"], P["z_len"])
        assert ok.all()
        uk, inv = np.unique(keys, return_inverse=True)
        assert np.array_equal(uk, t[0])
        v = np.abs(body[:, :3].astype(np.float64) - t[4][inv])
        q = np.stack([v[:, 0], v[:, 1], v[:, 2], v[:, 0] * v[:, 0], v[:, 0] * v[:, 1], v[:, 0] * v[:, 2], v[:, 1] * v[:, 1],
                      v[:, 1] * v[:, 2], v[:, 2] * v[:, 2]], 1)
        ab = np.zeros((uk.size, 9))
        np.add.at(ab, inv, q)
        _fine[name] = (cloud, P, t, ab)
    return _fine[name]


@pytest.mark.parametrize("factors", [(2, 2), (4, 2), (1, 2), (8, 8)])
@pytest.mark.parametrize("name", sorted(MAP_SCENES))
def test_coarsened_statistics_finalise_to_the_coarse_build(name, factors):
    cloud, P, (uk, count, first, sums, cen), ab = fine_stats(name)
    fxy, fz = factors
    o = cloud[0, :3]
    GL, ZL = float(cr.coarse_len(P["grid_len"], fxy)), float(cr.coarse_len(P["z_len"], fz))
    got = cr.coarsen(uk, count, first, sums, fxy, fz, o, P["grid_len"], P["z_len"], abs_sums=ab)
    wk, wcount, wfirst, wsums, wcen = he.accumulate(cloud[1:], o, GL, ZL)
    assert np.array_equal(got["key"], wk) and np.array_equal(got["count"], wcount) and np.array_equal(got["first_idx"], wfirst)
    assert got["children"].max() > 1 and got["children"].max() <= fxy * fxy * fz
    err = np.abs(got["sums"] - wsums)
    worst = float((err / np.maximum(got["tol"], 1e-300)).max())
    print(name, factors, "parents", wk.size, "worst error / bound", worst)
    assert (err <= got["tol"]).all()
    gcen = cr.centres(got["key"], o, GL, ZL)
    assert np.array_equal(gcen, wcen)
    a = he.finalize(got["key"], got["count"], got["first_idx"], got["sums"], gcen, P["slope_interval"])
    b = he.finalize(wk, wcount, wfirst, wsums, wcen, P["slope_interval"])
    for k in ("sx", "sy", "sz", "count", "first_idx", "flags"):
        assert np.array_equal(a[k], b[k]), k
    assert (a["num_nodes"], a["num_columns"], a["num_slopes"]) == (b["num_nodes"], b["num_columns"], b["num_slopes"])


# ---- 4. coarse to fine: register_pyramid on the shim ----

def test_register_pyramid_recovers_a_start_beyond_the_fine_basin():
    """drivable_site(100 000), COST_PARAMS, every fifth point as the scan, neighbourhood 7.  Start C = yaw 5 degrees, (2.0, 1.5) cells,
    -0.5 level: 1.256 m and 87 mrad off.  The fine map alone does not move (no_ascent at iteration 1).  Through host builds of the same
    cloud at 4x and 2x the lengths — by the key identity the coarsened maps — and then the fine map, the pose ends where the fine-only
    run from the documented start B (0.255 m off) ends, the reference here: measured 0.9 mm / 0.029 mrad for both (per level:
    3.4 mm, 1.5 mm, 0.9 mm).  Asserted: at most twice B's error in translation and in angle (a no_ascent and a converged ending stop
    up to one step apart)."""
    cloud, m1 = recovery_map("drivable_site")
    P = m1.P
    scan = np.ascontiguousarray(cloud[1:][::5])
    maps = []
    for f in (4, 2):
        maps.append(HostMap(cloud, dict(P, grid_len=float(cr.coarse_len(P["grid_len"], f)), z_len=float(cr.coarse_len(P["z_len"], f)))))
    maps.append(m1)
    g, z = P["grid_len"], P["z_len"]
    C_start = yaw(5.0, (2.0 * g, 1.5 * g, -0.5 * z))
    mk = lambda m: (lambda T: host_derivs(m, scan, T, 7), lambda T: host_score(m, scan, T, 7)["score"], 0.5 * m.P["grid_len"])
    stages = [mk(m) for m in maps]
    fine = reg.register(stages[-1][0], stages[-1][1], C_start, step_t=stages[-1][2])
    print("fine only from C:", fine["reason"], fine["iterations"])
    assert np.array_equal(fine["T"], C_start[:3])
    B = starts(P)["B"]
    ref = reg.register(stages[-1][0], stages[-1][1], B, step_t=stages[-1][2])
    tB, aB = dr.pose_error(ref["T"])
    res = reg.register_pyramid(stages, C_start)
    t, a = dr.pose_error(res["T"])
    print("reference (fine only from B): %.2f mm %.4f mrad, %s after %d" % (1e3 * tB, 1e3 * aB, ref["reason"], ref["iterations"]))
    print("pyramid from C:               %.2f mm %.4f mrad;" % (1e3 * t, 1e3 * a),
          "levels:", [("%.2f mm" % (1e3 * dr.pose_error(r["T"])[0]), r["reason"], r["iterations"]) for r in res["levels"]])
    assert len(res["levels"]) == 3 and res["levels"][-1]["history"] is res["history"] and res["reason"] == res["levels"][-1]["reason"]
    assert t <= 2.0 * tB and a <= 2.0 * aB, (t, a, tB, aB)
    T0 = C_start
    for m, lv, st in zip(maps, res["levels"], stages):
        ref_eval, ref_score = dr.callables(m.cells, m.origin, m.P["grid_len"], m.P["z_len"], scan, 7)
        check_steps(lv, T0, ref_eval, ref_score, st[2], what=("pyramid", m.P["grid_len"]))
        T0 = lv["T"]
    # K starts side by side chain their own poses; one start alone goes the way it goes in the batch
    two = reg.register_pyramid(stages, np.stack([C_start, B]))
    assert np.array_equal(two[0]["T"], res["T"]) and [r["iterations"] for r in two[0]["levels"]] == [r["iterations"] for r in res["levels"]]
    assert len(two[1]["levels"]) == 3 and dr.pose_error(two[1]["T"])[0] <= 2.0 * tB
    with pytest.raises(ValueError):
        reg.register_pyramid([], C_start)


# ---- 5. no CPU path ----

def test_coarsen_refuses_null_handles(native_lib):
    assert native_lib.gndt_coarsen_device(None, None, 2, 2, None) == 1      # GNDT_ERR_INVALID
