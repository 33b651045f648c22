"""The fast minimum-eigenpair routine the kernels use (gndt_math.hpp: min_eigenpair_sym3) against numpy.linalg.eigh on scatter
matrices of every shape the path meets, and against mpmath at 50 digits on the hard families.  Every check runs on both builds of
the header: g++ for x86 (host_math_shim.cpp, CPU tier) and hipcc for gfx950 (device_math_shim.hip, GPU tier), where the fp32 start
value comes from OCML's sqrtf / acosf / cosf and the fp64 divide and sqrt are Newton expansions."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import host_emulation as he

BACKENDS = ["host", pytest.param("device", marks=pytest.mark.gpu)]


def _solve(S, backend="host"):
    S = np.ascontiguousarray(S, np.float64)
    n = S.shape[0]
    lam = np.zeros(n)
    vec = np.zeros((n, 3))
    he.call(backend, "min_eigen", S, C.c_uint64(n), lam, vec)
    return lam, vec


def _mats(S):
    return np.stack([np.stack([S[:, 0], S[:, 1], S[:, 2]], 1), np.stack([S[:, 1], S[:, 3], S[:, 4]], 1),
                     np.stack([S[:, 2], S[:, 4], S[:, 5]], 1)], 1)


def _scatter(points):
    d = points - points.mean(1, keepdims=True)
    M = np.einsum("nki,nkj->nij", d, d)
    return np.stack([M[:, 0, 0], M[:, 0, 1], M[:, 0, 2], M[:, 1, 1], M[:, 1, 2], M[:, 2, 2]], 1)


def _check(S, name, backend="host", truth=None):
    """The gates: lambda within 2e-6 trace, a unit vector, 1 - |cos| <= 1e-9 where the minimum is separated, residual <= 1e-5.
    truth = (w, V), ascending eigenvalues and their vectors (mpmath), instead of eigh; its trace is then not floored at 1e-300."""
    lam, vec = _solve(S, backend)
    w, V = np.linalg.eigh(_mats(S)) if truth is None else truth
    tr = np.maximum(w.sum(1), 1e-300 if truth is None else 1e-323)
    err = np.abs(lam - w[:, 0]) / tr
    assert np.all(np.isfinite(lam)) and np.all(np.isfinite(vec)), name
    assert err.max() <= 2e-6, (name, err.max(), S[err.argmax()])
    nrm = np.linalg.norm(vec, axis=1)
    assert np.allclose(nrm, 1.0, atol=1e-12), name
    sep = (w[:, 1] - w[:, 0]) > 1e-3 * w[:, 2]
    if sep.any():
        cosv = np.abs((vec[sep] * V[sep][:, :, 0]).sum(1))
        assert (1 - cosv).max() <= 1e-9, (name, (1 - cosv).max())
    # whatever the clustering, the vector must be a (near) eigenvector: |S v - lam v| small
    r = np.einsum("nij,nj->ni", _mats(S), vec) - lam[:, None] * vec
    scale = np.maximum(np.abs(S).max(1), 1e-300 if truth is None else 1e-323)
    assert (np.linalg.norm(r, axis=1) / scale).max() <= 1e-5, (name, (np.linalg.norm(r, axis=1) / scale).max())


@pytest.mark.parametrize("backend", BACKENDS)
def test_random_voxel_scatters(backend):
    rng = np.random.default_rng(0)
    for npts in (3, 4, 8, 16, 200):
        _check(_scatter(rng.uniform(-0.25, 0.25, (4000, npts, 3))), f"uniform{npts}", backend)


@pytest.mark.parametrize("backend", BACKENDS)
def test_flat_and_linear_cells(backend):
    rng = np.random.default_rng(1)
    p = rng.uniform(-0.25, 0.25, (4000, 30, 3))
    for thick in (1e-1, 1e-2, 1e-4, 1e-7, 0.0):
        q = p.copy()
        q[:, :, 2] *= thick                      # ground patches: lambda_min << lambda_max
        _check(_scatter(q), f"flat{thick}", backend)
        # tilted planes
        R = np.linalg.qr(rng.normal(size=(4000, 3, 3)))[0]
        _check(_scatter(np.einsum("nij,nkj->nki", R, q)), f"tilted{thick}", backend)
    line = p.copy()
    line[:, :, 1:] *= 1e-9                       # rank 1: two (near-)zero eigenvalues
    _check(_scatter(line), "line", backend)
    line[:, :, 1:] = 0
    _check(_scatter(line), "exact_line", backend)


@pytest.mark.parametrize("backend", BACKENDS)
def test_degenerate_and_scaled(backend):
    S = np.zeros((6, 6))
    S[1] = [2, 0, 0, 2, 0, 2]                    # isotropic
    S[2] = [3, 0, 0, 2, 0, 1]                    # diagonal
    S[3] = [1, 0, 0, 1, 0, 0]                    # plane z = const (bridge_ground's ground)
    S[4] = [0, 0, 0, 0, 0, 5]                    # vertical line
    S[5] = [1, 1, 1, 1, 1, 1]                    # rank one, oblique
    lam, vec = _solve(S, backend)
    assert lam[0] == 0 and tuple(vec[0]) == (0, 0, 1)      # identical points
    assert abs(lam[1] - 2) < 1e-5 and abs(lam[2] - 1) < 1e-12 and abs(abs(vec[2][2]) - 1) < 1e-12
    assert abs(lam[3]) < 1e-12 and abs(abs(vec[3][2]) - 1) < 1e-12
    assert abs(lam[4]) < 5e-12 and abs(vec[4][2]) < 1e-6
    assert abs(lam[5]) < 5e-12 and abs(vec[5].sum()) < 1e-5
    rng = np.random.default_rng(2)
    base = _scatter(rng.uniform(-1, 1, (2000, 10, 3)))
    for scale in (1e-18, 1e-6, 1e6, 1e18):
        _check(base * scale, f"scale{scale}", backend)


@pytest.mark.parametrize("backend", BACKENDS)
def test_matches_in_repo_jacobi(backend):
    rng = np.random.default_rng(3)
    S = _scatter(rng.uniform(-0.1, 0.1, (3000, 12, 3)) * np.array([1.0, 0.6, 0.05]))
    lam, _ = _solve(S, backend)
    ev = np.zeros((S.shape[0], 3))
    vv = np.zeros((S.shape[0], 9))
    he.call(backend, "jacobi", S, C.c_uint64(S.shape[0]), ev, vv)
    assert np.abs(lam - ev.min(1)).max() <= 1e-9 * np.abs(ev).max()


@pytest.mark.parametrize("backend", BACKENDS)
def test_oblique_lines_two_clustered_small_eigenvalues(backend):
    """Points of one scan line in a cell: rank-1 scatter in a general direction, the two small eigenvalues 1e-6 .. 1e-18 of the large
    one.  The fp32 start value is then up to ~1e-4 off (acos near 1) and used to land beyond the cubic's first critical point, where
    the Newton loop stopped at once and returned the start value (found by tools/fuzz_campaign.py: 3 nearly collinear points,
    lambda_min 2e-6 instead of 0 at trace 0.13).  The restart branch added for it is no longer reached by these inputs, nor by any
    other known one: the current estimate lands at least 9.59e-6 left of that critical point (the comment at the branch in
    gndt_math.hpp gives the reason).  The cases stay as a check of the result on the inputs that once failed, not of the branch."""
    rng = np.random.default_rng(4)
    for npts in (3, 5, 40):
        for thick in (1e-3, 1e-5, 1e-7, 1e-9, 0.0):
            p = rng.uniform(-0.25, 0.25, (6000, npts, 3))
            p[:, :, 1:] *= thick
            R = np.linalg.qr(rng.normal(size=(6000, 3, 3)))[0]
            _check(_scatter(np.einsum("nij,nkj->nki", R, p)), f"oblique_line{npts}_{thick}", backend)
    # the campaign's node itself
    S = np.array([[0.04515270355572436, 0.052456556703911396, -0.033486629652467556, 0.06094187334398763, -0.038903391133923534, 0.02483471148358755]])
    S = S * (1 + 1e-16 * rng.standard_normal((5000, 6)))
    lam, _ = _solve(S, backend)
    assert np.abs(lam).max() <= 2e-6 * 0.131, np.abs(lam).max()


# ---- hard families, gated against mpmath (mp.dps = 50) as well as eigh ----
def _rotated(rng, lams):
    """Scatters R diag(lams) R^T in random orientations (rows of lams: three eigenvalues)."""
    R = np.linalg.qr(rng.normal(size=(lams.shape[0], 3, 3)))[0]
    M = np.einsum("nij,nj,nkj->nik", R, lams, R)
    return np.stack([M[:, 0, 0], M[:, 0, 1], M[:, 0, 2], M[:, 1, 1], M[:, 1, 2], M[:, 2, 2]], 1)


def _clustered(rng, n=6000):
    """The two smallest eigenvalues 1e-3 .. 1e-12 of lambda_max apart, above zero or at it, in random orientations."""
    gap = 10.0 ** -rng.integers(3, 13, n).astype(np.float64)
    low = np.where(rng.random(n) < 0.5, 0.0, rng.uniform(1e-4, 0.3, n))
    return _rotated(rng, np.stack([low, low + gap, np.ones(n)], 1))


def _isotropy_switch(rng, n=6000):
    """c I + E with E traceless, |E| such that min_eigenpair_sym3's p2 lies within a factor 2 of its 1e-12 switch, either side
    (p2 ~ |E|_F^2 of the matrix scaled by max |S_ij|)."""
    D = rng.normal(size=(n, 3, 3))
    D = D + D.transpose(0, 2, 1)
    D -= np.eye(3) * (np.trace(D, axis1=1, axis2=2) / 3)[:, None, None]
    D /= np.linalg.norm(D, axis=(1, 2))[:, None, None]
    M = np.eye(3) + D * (1e-6 * np.sqrt(rng.uniform(0.5, 2.0, n)))[:, None, None]
    M *= rng.uniform(1e-3, 1e3, n)[:, None, None]
    return np.stack([M[:, 0, 0], M[:, 0, 1], M[:, 0, 2], M[:, 1, 1], M[:, 1, 2], M[:, 2, 2]], 1)


def _double_roots(rng, n=6000):
    """A double smallest root (r = +1, acos at 0) and a double largest root (r = -1, acos at pi), rotated and axis-aligned."""
    a = np.where(rng.random(n) < 0.3, 0.0, rng.uniform(0.0, 0.9, n))
    b = np.ones(n)
    lams = np.where((np.arange(n) % 2 == 0)[:, None], np.stack([a, a, b], 1), np.stack([a, b, b], 1))
    S = _rotated(rng, lams)
    k = n // 10                                      # exact diagonal ones, where the fp32 r sits exactly on the clamp
    S[:k] = 0.0
    S[:k, 0], S[:k, 3], S[:k, 5] = lams[:k, 0], lams[:k, 1], lams[:k, 2]
    return S


def _extreme_scale(rng, n=2000):
    """Entries around 1e-310 (fp64 subnormal: 1 / max |S_ij| overflows) and up to 1e30."""
    S = _scatter(rng.uniform(-1, 1, (n, 10, 3)))
    return S * np.where(np.arange(n) % 2 == 0, 10.0 ** rng.uniform(-312, -306, n), 10.0 ** rng.uniform(20, 30, n))[:, None]


def _oblique_lines(rng, n=6000):
    p = rng.uniform(-0.25, 0.25, (n, 5, 3))
    p[:, :, 1:] *= (10.0 ** -rng.integers(3, 10, n).astype(np.float64))[:, None, None]
    R = np.linalg.qr(rng.normal(size=(n, 3, 3)))[0]
    return _scatter(np.einsum("nij,nkj->nki", R, p))


HARD = {"clustered": _clustered, "isotropy_switch": _isotropy_switch, "double_roots": _double_roots, "extreme_scale": _extreme_scale,
        "oblique_lines": _oblique_lines}


@functools.lru_cache(maxsize=None)
def _family(name):
    return HARD[name](np.random.default_rng(sorted(HARD).index(name) + 100))


@functools.lru_cache(maxsize=None)
def _mp_truth(name, count=2000):
    """Ascending eigenvalues and their vectors of the family's first `count` matrices, by mpmath at 50 digits from the exact fp64
    entries (shared by both backends)."""
    import mpmath
    S = _family(name)[:count]
    w = np.zeros((count, 3))
    V = np.zeros((count, 3, 3))
    with mpmath.workdps(50):
        for i, s in enumerate(S):
            E, Q = mpmath.eigsy(mpmath.matrix([[s[0], s[1], s[2]], [s[1], s[3], s[4]], [s[2], s[4], s[5]]]))
            order = sorted(range(3), key=lambda k: E[k])
            w[i] = [float(E[k]) for k in order]
            V[i] = [[float(Q[r, k]) for k in order] for r in range(3)]
    return w, V


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("family", sorted(HARD))
def test_hard_families_against_mpmath_and_eigh(family, backend):
    S = _family(family)
    _check(S[:2000], f"{family}/mpmath", backend, truth=_mp_truth(family))
    if family != "extreme_scale":                    # (LAPACK's eigh is no truth for subnormal entries: that family is mpmath's alone)
        _check(S, f"{family}/eigh", backend)


def _rough_normal(S, backend):
    S = np.ascontiguousarray(S, np.float64)
    rough = np.zeros(S.shape[0], np.float32)
    normal = np.zeros((S.shape[0], 3), np.float32)
    he.call(backend, "rough_normal", S, C.c_uint64(S.shape[0]), rough, normal)
    return rough, normal


@pytest.mark.gpu
def test_rough_normal_device_against_host_report():
    """node_rough_normal on the device build against the host build, over every hard family and the scene-like bulk.  The two need
    not agree bit for bit (the fp32 start value differs by OCML's ulps, and so can the Newton iterate): reported, not gated; both
    sides are gated against the truth above."""
    rng = np.random.default_rng(9)
    sets = {name: _family(name) for name in HARD}
    sets["uniform"] = _scatter(rng.uniform(-0.25, 0.25, (20000, 12, 3)))
    flat = rng.uniform(-0.25, 0.25, (20000, 30, 3))
    flat[:, :, 2] *= 1e-3
    sets["flat"] = _scatter(flat)
    for name, S in sets.items():
        rd, nd = _rough_normal(S, "device")
        rh, nh = _rough_normal(S, "host")
        assert np.isfinite(rd).all() and np.isfinite(nd).all(), name
        rough_diff = rd.view(np.uint32) != rh.view(np.uint32)
        normal_diff = (nd.view(np.uint32) != nh.view(np.uint32)).any(1)
        tr = np.maximum(S[:, 0] + S[:, 3] + S[:, 5], 1e-323)
        print(f"rough_normal {name}: {S.shape[0]} nodes, rough differs bitwise on {int(rough_diff.sum())}, max |d rough| / trace "
              f"{(np.abs(rd.astype(np.float64) - rh) / tr).max():.3e}; normal differs on {int(normal_diff.sum())}, "
              f"max |d normal| {np.abs(nd.astype(np.float64) - nh).max():.3e}")
