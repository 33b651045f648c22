"""The kernels' key, finalisation, cost and integer arithmetic (gndt_math.hpp, gndt_bucket3.hpp, gndt_cost.hpp, gndt_partition.hpp)
on adversarial inputs, on both builds: g++ for x86 (tests/host_math_shim.cpp) and hipcc for gfx950 (tests/device_math_shim.hip).
Each check runs on the host in the CPU tier; the device case also compares the device build with the host build.  Keys, the
finalisation's mean and scatter, cost_travel and the integer helpers must agree bit for bit; cost_angle (OCML's acosf against
glibc's) within a bound well under the 1e-3 degree exemption test_gpu_cost.py grants it."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests import host_emulation as he
from tests import parity

BACKENDS = ["host", pytest.param("device", marks=pytest.mark.gpu)]
CELLS = [(0.5, 0.1), (0.5, 0.5), (0.2, 0.2), (0.1, 0.05), (1.0 / 3.0, 0.07), (0.25, 0.5), (1.0, 0.1), (0.1, 0.1)]  # tools/fuzz_campaign.py
MAX_XY, MAX_Z = 65535, (1 << 21) - 1
ANGLE_BOUND_DEG = 1e-4     # device vs host cost_angle; test_gpu_cost.py exempts decisions within 1e-3 degrees of a gate


# ---- keys ----
def _axis_values(rng, o, length, limit, n):
    """fp32 coordinates along one axis: cell borders (random indices and 1, 65534 .. 65536, kMaxZ -+ 1) and 1 .. 3 ulps either side,
    interior points, p == o, -0.0, p - o subnormal, NaN, +-inf."""
    o = np.float32(o)
    k = np.concatenate([rng.integers(1, min(limit, 70000), n // 2), np.repeat([1, 2, 65534, 65535, 65536, limit - 1, limit, limit + 1],
                                                                              n // 64)]).astype(np.float64)
    sign = rng.choice([-1.0, 1.0], k.size)
    base = (np.float64(o) + sign * k * np.float64(np.float32(length))).astype(np.float32)
    v = [base]
    for st in (1, 2, 3):
        up, dn = base.copy(), base.copy()
        for _ in range(st):
            up, dn = np.nextafter(up, np.float32(np.inf)), np.nextafter(dn, np.float32(-np.inf))
        v += [up, dn]
    v.append((np.float64(o) + sign * (k - rng.random(k.size)) * length).astype(np.float32))
    tiny = [o, np.nextafter(o, np.float32(1)), np.nextafter(o, np.float32(-1)), np.float32(-0.0), np.float32(0.0),
            np.float32(1.4e-45), np.float32(-1.4e-45), np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf), np.float32(3.4e38)]
    v.append(np.repeat(np.float32(tiny), n // 64))
    return np.concatenate(v)


def _key_inputs(rng, gl, zl, origin, n=12000):
    cols = []
    for a, (length, limit) in enumerate(((gl, MAX_XY), (gl, MAX_XY), (zl, MAX_Z))):
        vals = _axis_values(rng, origin[a], length, limit, n)
        cols.append(rng.permutation(vals))
    m = min(c.size for c in cols)
    return np.ascontiguousarray(np.stack([c[:m] for c in cols], 1), np.float32)


def _numpy_key(pts, o, gl, zl):
    """The reference's (int)ceilf(fabsf(p - o) / len) per axis in numpy fp32 (map2D.h:965-970), its sign, and the key range."""
    o = np.float32(o)
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.ceil(np.abs(pts - o) / np.float32([gl, gl, zl]))
        ok = (q[:, 0] <= MAX_XY) & (q[:, 1] <= MAX_XY) & (q[:, 2] <= MAX_Z)
    qi = np.where(np.isfinite(q) & (q <= MAX_Z), q, 0).astype(np.int64)
    qi[qi == 0] = 1
    return np.where(pts > o, qi, -qi), ok


def _run_keys(backend, name, pts, o, gl, zl):
    keys = np.zeros(pts.shape[0], np.uint64)
    ok = np.zeros(pts.shape[0], np.uint8)
    he.call(backend, name, pts, C.c_uint64(pts.shape[0]), C.c_int(3), (C.c_float * 3)(*[float(v) for v in o]), C.c_float(gl),
            C.c_float(zl), keys, ok)
    return keys, ok


ORIGINS = [(0.0, 0.0, 0.0), (312.7, -845.3, 2.1), (-2999.9, 1500.25, -40.0), (1e-38, -1e-38, 0.0)]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("cells", CELLS, ids=[f"{g:.3g}x{z:.3g}" for g, z in CELLS])
def test_keys_and_record_offsets_on_borders_and_extremes(cells, backend):
    """point_key and point_key_fast against the numpy fp32 restatement for every cell pair of the fuzz campaign, origins up to
    3000 m, indices at the key-range limits and the special values.  On the device, both must equal the host build bit for bit,
    and so must the bucket kernels' key_offset sequence: s = point_key's index, v = (double)p - axis_centre(s, o, len) exactly
    ((s -+ 1/2) len is exact in fp64, so axis_index_offset's fma and the host's multiply-add round once, identically)."""
    gl, zl = cells
    rng = np.random.default_rng(int(gl * 1000) * 7 + int(zl * 1000))
    for origin in ORIGINS:
        o = np.float32(origin)
        pts = _key_inputs(rng, gl, zl, o)
        want, ok_ref = _numpy_key(pts, o, gl, zl)
        for name in ("point_keys", "point_keys_fast"):
            keys, ok = _run_keys(backend, name, pts, o, gl, zl)
            np.testing.assert_array_equal(ok != 0, ok_ref, err_msg=f"{name} ok, origin {origin}")
            got = np.stack(he.unpack(keys), 1)
            np.testing.assert_array_equal(got[ok_ref], want[ok_ref], err_msg=f"{name}, origin {origin}")
            if backend == "device":
                hk, hok = _run_keys("host", name, pts, o, gl, zl)
                np.testing.assert_array_equal(ok, hok)
                np.testing.assert_array_equal(keys[ok != 0], hk[ok != 0], err_msg=f"{name} device vs host, origin {origin}")
        assert ok_ref.sum() > 0.5 * pts.shape[0] and (~ok_ref).sum() > 100
        if backend != "device":
            continue
        n = pts.shape[0]
        s = np.zeros((n, 3), np.int32)
        v = np.zeros((n, 3), np.float64)
        ok = np.zeros(n, np.uint8)
        he.call("device", "key_offset", pts, C.c_uint64(n), C.c_int(3), (C.c_float * 3)(*[float(x) for x in o]), C.c_float(gl),
                C.c_float(zl), s, v, ok)
        np.testing.assert_array_equal(ok != 0, ok_ref, err_msg=f"key_offset ok, origin {origin}")
        np.testing.assert_array_equal(s[ok_ref], want[ok_ref], err_msg=f"key_offset s, origin {origin}")
        lens = np.float64(np.float32([gl, gl, zl]))
        half = np.where(s > 0, s - 0.5, s + 0.5)
        centre = np.float64(o) + half * lens                      # axis_centre (gndt_math.hpp), IEEE fp64, no contraction
        vref = pts.astype(np.float64) - centre
        bad = ok_ref[:, None] & (v.view(np.uint64) != vref.view(np.uint64))
        assert not bad.any(), (origin, pts[bad.any(1)][:5], v[bad.any(1)][:5], vref[bad.any(1)][:5])
        # axis_centre of those keys (shim_centres / dshim_centres): the numpy centre above, bit for bit, on both builds
        keys = np.ascontiguousarray(_run_keys("host", "point_keys", pts, o, gl, zl)[0][ok_ref])
        cen = [np.zeros((keys.size, 3)) for _ in range(2)]
        for b, c in zip(("device", "host"), cen):
            he.call(b, "centres", keys, C.c_uint64(keys.size), (C.c_float * 3)(*[float(x) for x in o]), C.c_float(gl), C.c_float(zl), c)
        np.testing.assert_array_equal(cen[0].view(np.uint64), cen[1].view(np.uint64))
        np.testing.assert_array_equal(cen[0].view(np.uint64), np.ascontiguousarray(centre[ok_ref]).view(np.uint64))


# ---- finalisation ----
def _exact_moments(p):
    """Exact centroid and scatter of fp32 points (n, 3), as Fractions, from integer sums of their dyadic values."""
    n = p.shape[0]
    X, K = [], []
    for col in p.T.astype(np.float64):
        m, e = np.frexp(col)
        mi, sh = (m * 2.0 ** 53).astype(np.int64), e.astype(np.int64) - 53
        k = int(-sh.min())
        X.append(np.array([int(a) << int(b + k) for a, b in zip(mi, sh)], dtype=object))
        K.append(k)
    s1 = [x.sum() for x in X]
    mean = [Fraction(s1[a], n << K[a]) for a in range(3)]
    S = [Fraction(n * (X[a] * X[b]).sum() - s1[a] * s1[b], n << (K[a] + K[b]))
         for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
    return mean, S


def _finalize(backend, count, sums, cen):
    n = count.size
    mean = np.zeros((n, 3), np.float32)
    cov = np.zeros((n, 6), np.float32)
    rough = np.zeros(n, np.float32)
    normal = np.zeros((n, 3), np.float32)
    he.call(backend, "finalize", np.ascontiguousarray(count, np.uint32), np.ascontiguousarray(sums), np.ascontiguousarray(cen),
            C.c_uint64(n), C.c_int(1), mean, cov, rough, normal)
    return mean, cov, rough, normal


def _nodes(kind, rng):
    """(points (n, 3) fp32, origin, grid_len, z_len) of one family of nodes."""
    if kind == "three_points":                       # 3 points in each of 20000 cells
        o = np.float32([-3.3, 7.1, 0.4])
        cell = rng.integers(-2000, 2000, (20000, 1, 3)).astype(np.float64)
        p = o + (cell + rng.random((20000, 3, 3))) * np.float64([0.2, 0.2, 0.1])
        return p.reshape(-1, 3).astype(np.float32), o, 0.2, 0.1
    if kind == "identical":                          # 20 nodes of 30000 identical points (the reference's padding)
        q = (rng.uniform(-50, 50, (20, 3))).astype(np.float32)
        return np.repeat(q, 30000, 0), np.float32([0.05, -0.05, 0.0]), 0.1, 0.05
    if kind == "zero_padding":                       # 20000 (0,0,0) and 200 real points in the node around 0, ~3 km from the origin
        o = np.float32([2999.13, -2999.41, 1.7])
        near = (rng.random((200, 3)) * 0.08).astype(np.float32)
        return np.concatenate([np.zeros((20000, 3), np.float32), near]), o, 0.1, 0.1
    if kind == "dense_far_cell":                     # 400000 points in one 0.05 m cell at |centre| ~ 3000 m
        c = np.float64([2999.975, -1500.025, 12.025])
        return (c + (rng.random((400000, 3)) - 0.5) * 0.0499).astype(np.float32), np.float32([0, 0, 0]), 0.05, 0.05
    if kind == "ulp_apart":                          # 3 .. 40 points one fp32 ulp apart, at magnitudes 0.7 .. 3e3
        pts = []
        for mag in (0.7, 13.0, 250.0, 2999.0):
            for m in (3, 5, 40):
                b = np.float32([mag, -mag * 0.9, mag * 0.3])
                for j in range(m):
                    pts.append(b.copy())
                    b = np.nextafter(b, np.float32(np.inf))
        return np.array(pts, np.float32), np.float32([0.013, -0.021, 0.002]), 0.5, 0.5
    raise KeyError(kind)


FAMILIES = ["three_points", "identical", "zero_padding", "dense_far_cell", "ulp_apart"]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("kind", FAMILIES)
def test_finalize_node_against_exact_moments(kind, backend):
    """finalize_node from sums built in fp64 on the host: the mean within 1 fp32 ulp of the exact centroid, the scatter within
    parity.TOL_COV_TRUTH of the exact one plus the rounding its fp64 sums allow (exactly zero where the points are identical: the
    noise floor), on a subsample of nodes.  On the device mean and cov must equal the host's bit for bit (IEEE fp64 without contraction on both), as must mean_z."""
    rng = np.random.default_rng(FAMILIES.index(kind) + 40)
    pts, o, gl, zl = _nodes(kind, rng)
    uk, count, first, sums, cen = he.accumulate(pts, o, gl, zl)
    mean, cov, rough, normal = _finalize(backend, count, sums, cen)
    assert np.isfinite(mean).all() and np.isfinite(cov).all() and np.isfinite(rough).all() and np.isfinite(normal).all()
    if backend == "device":
        hm, hc, hr, hn = _finalize("host", count, sums, cen)
        np.testing.assert_array_equal(mean.view(np.uint32), hm.view(np.uint32))
        np.testing.assert_array_equal(cov.view(np.uint32), hc.view(np.uint32))
        cz = np.ascontiguousarray(cen[:, 2])
        svz = np.ascontiguousarray(sums[:, 2])
        mz = [np.zeros(count.size, np.float32) for _ in range(2)]
        for b, out in zip(("device", "host"), mz):
            he.call(b, "mean_z_n", np.ascontiguousarray(count, np.uint32), svz, cz, C.c_uint64(count.size), out)
        np.testing.assert_array_equal(mz[0].view(np.uint32), mz[1].view(np.uint32))
        np.testing.assert_array_equal(mz[0], hm[:, 2])
    keys = _point_keys_of(pts, o, gl, zl)
    worst = worst_fp64 = 0.0
    for i in rng.choice(uk.size, min(uk.size, 40), replace=False):
        p = pts[keys == uk[i]]
        em, eS = _exact_moments(p)
        for a in range(3):
            ex = np.float32(float(em[a]))
            assert abs(Fraction(float(mean[i, a])) - em[a]) <= Fraction(float(np.spacing(np.abs(ex)))), (kind, i, a)
        emax = max(abs(x) for x in eS)
        if emax == 0:                                # identical points: the noise floor makes the scatter exactly zero (gndt_math.hpp)
            assert (cov[i] == 0).all() and rough[i] == np.float32(0.01) and tuple(normal[i]) == (0, 0, 1), (kind, i, cov[i])
        err = max(abs(Fraction(float(cov[i, k])) - eS[k]) for k in range(6))
        # TOL_COV_TRUTH of the largest entry, plus what the fp64 arithmetic of the sums can leave: node_moments subtracts
        # (Sum v_j)(Sum v_k) / n from Sum v_j v_k, sums of n terms with up to n 2^-53 relative rounding each, bounded by
        # max_k Sum v_k^2 (Cauchy-Schwarz), and zeroes a diagonal below 2 n 2^-53 Sum v_k^2 (its noise floor): 4 n 2^-53 in all
        fp64 = 4.0 * count[i] * 2.0 ** -53 * float(sums[i, [3, 6, 8]].max())
        assert err <= Fraction(parity.TOL_COV_TRUTH) * emax + Fraction(fp64), (kind, i, float(err), float(emax), fp64)
        worst = max(worst, float(err / emax) if emax else 0.0)
        worst_fp64 = max(worst_fp64, fp64 / float(emax) if emax else 0.0)
    print(f"finalize {kind} {backend}: max |d cov| / max |cov| {worst:.3e} (fp64 allowance up to {worst_fp64:.3e} of it)")


def _point_keys_of(pts, o, gl, zl):
    keys, ok = _run_keys("host", "point_keys", np.ascontiguousarray(pts, np.float32), o, gl, zl)
    assert ok.all()
    return keys


# ---- cost helpers ----
def _angle_pairs(rng):
    """Unit-normal pairs (fp32) at angles swept over 0 .. 180 degrees, dense near 0 (acos near 1) and within 0.01 degrees of the
    gates 15, 20, 30 and 45 (and of 180 minus them: the fold)."""
    deg = [np.linspace(0, 180, 200001), 10.0 ** -rng.uniform(0, 8, 100000), rng.uniform(0, 0.05, 100000)]
    for g in (15.0, 20.0, 30.0, 45.0):
        deg += [g + rng.uniform(-0.01, 0.01, 50000), 180 - g + rng.uniform(-0.01, 0.01, 20000)]
    deg = np.concatenate(deg)
    n1 = rng.normal(size=(deg.size, 3))
    n1 /= np.linalg.norm(n1, axis=1, keepdims=True)
    n1[: deg.size // 4] = [0, 0, 1]                  # (up, as most slopes are)
    axis = np.cross(n1, rng.normal(size=(deg.size, 3)))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    t = np.radians(deg)[:, None]
    n2 = n1 * np.cos(t) + np.cross(axis, n1) * np.sin(t)
    return np.ascontiguousarray(n1, np.float32), np.ascontiguousarray(n2, np.float32)


def _cost(backend, name, a, b):
    out = np.zeros(a.shape[0], np.float32)
    he.call(backend, name, a, b, C.c_uint64(a.shape[0]), out)
    return out


def _res(n1, n2):
    """cost_angle's fp32 cosine: fp32 dot as Eigen sums it, fp64 norms, the quotient rounded to fp32."""
    p = n1 * n2
    dot = p[:, 0] + (p[:, 1] + p[:, 2])
    a, b = n1.astype(np.float64) ** 2, n2.astype(np.float64) ** 2
    l1, l2 = np.sqrt((a[:, 0] + a[:, 1]) + a[:, 2]), np.sqrt((b[:, 0] + b[:, 1]) + b[:, 2])
    return (dot.astype(np.float64) / (l1 * l2)).astype(np.float32)


@pytest.mark.parametrize("backend", BACKENDS)
def test_cost_angle_and_travel(backend):
    """cost_angle against the degrees of an mpmath acos of its own fp32 cosine (both builds: within the fp32 rounding of the result
    plus a few ulps of acosf); cost_travel, IEEE throughout, on the host's value bit for bit.  On the device, |device - host| of
    cost_angle is gated at ANGLE_BOUND_DEG, a tenth of the 1e-3 degree exemption in test_gpu_cost.py, and reported."""
    import mpmath
    rng = np.random.default_rng(31)
    n1, n2 = _angle_pairs(rng)
    ang = _cost(backend, "cost_angle", n1, n2)
    res = _res(n1, n2)
    # a cosine that rounds beyond +-1 gives NaN, as acos does in the reference (map2D.h:477-482): the flood's gate then fails
    out = np.abs(res) > 1
    assert out.any() and np.isnan(ang[out]).all() and np.isfinite(ang[~out]).all()
    assert (ang[~out] >= 0).all() and (ang[~out] <= 90).all()
    sub = rng.choice(np.flatnonzero(~out), 20000, replace=False)
    with mpmath.workdps(30):
        exact = np.array([float(mpmath.acos(mpmath.mpf(float(r))) * 180 / mpmath.pi) for r in res[sub]])
    bound = 4 * np.spacing(np.float32(exact)).astype(np.float64)      # acosf within 2 ulp; * 180 and / pi each rounded to fp32
    exact = np.where(exact > 90, 180 - exact, exact)                   # (the fold: 180 - an, exact in fp32 for an > 90)
    err = np.abs(ang[sub].astype(np.float64) - exact)
    assert (err <= bound).all(), (err.max(), res[sub][np.argmax(err - bound)])
    print(f"cost_angle {backend}: max |angle - mpmath acos of the same fp32 cosine| {err.max():.3e} deg")
    if backend == "device":
        host = _cost("host", "cost_angle", n1, n2)
        np.testing.assert_array_equal(np.isnan(ang), np.isnan(host))
        d = np.abs(ang[~out].astype(np.float64) - host[~out])
        print(f"cost_angle device vs host: {int((d > 0).sum())} of {d.size} differ, max {d.max():.3e} deg "
              f"(host vs mpmath {np.abs(host[sub] - exact).max():.3e} deg)")
        assert d.max() <= ANGLE_BOUND_DEG, d.max()
    # cost_travel: mean pairs from 1e-30 to 1e4 m apart, and equal, subnormal and huge ones
    a = (rng.normal(size=(200000, 3)) * 10.0 ** rng.uniform(-3, 4, (200000, 1))).astype(np.float32)
    b = (a + rng.normal(size=a.shape) * 10.0 ** rng.uniform(-30, 4, (200000, 1))).astype(np.float32)
    b[:1000] = a[:1000]
    b[1000:2000] = np.nextafter(a[1000:2000], np.float32(np.inf))
    a[2000:3000] = rng.normal(size=(1000, 3)).astype(np.float32) * np.float32(1e-40)
    a[3000:4000] = rng.normal(size=(1000, 3)).astype(np.float32) * np.float32(1e37)
    b, a = np.ascontiguousarray(b), np.ascontiguousarray(a)
    tr = _cost(backend, "cost_travel", a, b)
    d = (a - b).astype(np.float64)
    with np.errstate(over="ignore"):
        want = np.sqrt((d[:, 0] ** 2 + d[:, 1] ** 2) + d[:, 2] ** 2).astype(np.float32)
    np.testing.assert_array_equal(tr, want)
    if backend == "device":
        np.testing.assert_array_equal(tr.view(np.uint32), _cost("host", "cost_travel", a, b).view(np.uint32))


# ---- integer helpers ----
def _mix64(x):
    x = x.astype(np.uint64)
    x ^= x >> np.uint64(33)
    x *= np.uint64(0xFF51AFD7ED558CCD)
    x ^= x >> np.uint64(33)
    x *= np.uint64(0xC4CEB9FE1A85EC53)
    x ^= x >> np.uint64(33)
    return x


def _ints(sx, sy, sz, blk, B, W):
    n = sx.size
    out = dict(pack=np.zeros(n, np.uint64), unpack=np.zeros((n, 3), np.int32), mix=np.zeros(n, np.uint64),
               chash=np.zeros(n, np.uint32), bucket=np.zeros(n, np.uint32), owner=np.zeros(n, np.uint32), contig=np.zeros((n, 2), np.int32))
    he.call("device", "ints", sx, sy, sz, C.c_uint64(n), (C.c_int32 * 7)(*blk), C.c_uint32(B), C.c_uint32(W), *out.values())
    return out


def _u32(x):
    return np.asarray(x, np.uint64) & np.uint64(0xFFFFFFFF)


def _column_hash(sx, sy):
    """gndt_partition.hpp column_hash, restated in numpy (uint32 arithmetic carried in uint64 and masked)."""
    a = _u32(sx.astype(np.int64) + 65536) & np.uint64(0x3FFFF)
    b = _u32(sy.astype(np.int64) + 65536) & np.uint64(0x3FFFF)
    h = _u32(a * np.uint64(0x9E3779) + b * np.uint64(0x85EBCB))
    h ^= h >> np.uint64(15)
    h = _u32((h & np.uint64(0xFFFFFF)) * np.uint64(0x1B3C6D))
    h ^= h >> np.uint64(13)
    return h


def _column_bucket(sx, sy, blk, B):
    """column_bucket: bucket_of(column_hash) without a block map, the clamped block index with one."""
    on, x0, y0, shx, shy, nx, ny = blk
    if not on:
        return ((_column_hash(sx, sy) >> np.uint64(8)) * np.uint64(B & 0xFFFFFF)) >> np.uint64(24)
    cx, cy = np.where(sx > 0, sx - 1, sx).astype(np.int64), np.where(sy > 0, sy - 1, sy).astype(np.int64)
    bx, by = np.clip((cx - x0) >> shx, 0, nx - 1), np.clip((cy - y0) >> shy, 0, ny - 1)
    return (bx * ny + by).astype(np.uint64)


@pytest.mark.gpu
def test_integer_helpers_on_the_device_match_their_restatements():
    """pack_key / unpack_key, mix64, column_hash, column_bucket (hashed and block map), owner_of and contiguous_index on the device
    against numpy restatements and, for owner_of, the host build in libgndt (gndt_owner_of_columns), over a grid of columns that
    includes +-1, +-65535 and the quadrant seams, for W = 1 .. 8."""
    from grid_ndt_amd import _lib
    edge = np.array([-65535, -65534, -32768, -1025, -1024, -513, -512, -2, -1, 1, 2, 512, 513, 1024, 1025, 32768, 65534, 65535])
    rng = np.random.default_rng(5)
    v = np.concatenate([edge, rng.integers(-65535, 65536, 200)])
    v = v[v != 0]
    sx, sy = [np.ascontiguousarray(a.reshape(-1), np.int32) for a in np.meshgrid(v, v, indexing="ij")]
    sz = np.ascontiguousarray(rng.choice([-MAX_Z, -(1 << 20), -2, -1, 1, 2, 7, 1 << 20, MAX_Z], sx.size), np.int32)
    pack = ((sx.astype(np.int64) + (1 << 20)).astype(np.uint64) << np.uint64(43)) | \
        ((sy.astype(np.int64) + (1 << 20)).astype(np.uint64) << np.uint64(22)) | (sz.astype(np.int64) + (1 << 21)).astype(np.uint64)
    chash = _column_hash(sx, sy).astype(np.uint32)
    contig = np.stack([np.where(sx > 0, sx - 1, sx), np.where(sy > 0, sy - 1, sy)], 1)
    blocks = [(0, 0, 0, 0, 0, 0, 0), (1, -40, -40, 5, 4, 3, 5), (1, -65535, -65535, 9, 0, 256, 1)]
    for W in range(1, 9):
        owner = np.zeros(sx.size, np.uint32)
        assert _lib.lib().gndt_owner_of_columns(sx.ctypes.data, sy.ctypes.data, sx.size, W, owner.ctypes.data) == 0
        for blk, B in zip(blocks, (7 if W % 2 else 32768, 15, 256)):
            d = _ints(sx, sy, sz, blk, B, W)
            np.testing.assert_array_equal(d["pack"], pack)
            np.testing.assert_array_equal(d["unpack"], np.stack([sx, sy, sz], 1))
            np.testing.assert_array_equal(d["mix"], _mix64(pack))
            np.testing.assert_array_equal(d["chash"], chash)
            np.testing.assert_array_equal(d["bucket"], _column_bucket(sx, sy, blk, B).astype(np.uint32), err_msg=f"blk={blk} B={B}")
            np.testing.assert_array_equal(d["owner"], owner, err_msg=f"W={W}")
            np.testing.assert_array_equal(d["contig"], contig)
            assert (d["bucket"] < B).all() and (d["owner"] < W).all()


# ---- CPU tier: the device shim still builds, with the library's flags ----
def test_device_shim_cross_compiles_with_the_library_flags(tmp_path, monkeypatch):
    """hipcc cross-compiles tests/device_math_shim.hip for gfx950, the shared object exports every dshim_ entry point, and its
    object embeds a gfx950 code object.  The compile takes its flags from grid_ndt_amd._lib.HIPCC_FLAGS at build time: a flag
    hipcc does not know, put into that list, makes it fail.  (No GPU needed: keeps the GPU tier's shim from rotting.)"""
    from grid_ndt_amd import _lib
    so = str(tmp_path / "dshim.so")
    he.build_device_shim(so, force=True)
    syms = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout.split()
    for name in he.DSHIM_ENTRIES:
        assert "dshim_" + name in syms, name
    with open(os.path.splitext(so)[0] + ".o", "rb") as f:
        assert b"amdgcn-amd-amdhsa--gfx950" in f.read()          # the embedded device code object's target
    monkeypatch.setattr(_lib, "HIPCC_FLAGS", _lib.HIPCC_FLAGS + ["--gndt-no-such-flag"])
    with pytest.raises(subprocess.CalledProcessError):
        he.build_device_shim(str(tmp_path / "probe.so"), force=True)
