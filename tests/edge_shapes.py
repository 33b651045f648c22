"""Shapes at the count edges of the consumer kernels: the constants the shapes derive from (EDGES; tests/test_edge_shapes_host.py reads
them out of the headers again, so that a retuned constant fails a test that says: derive the shapes anew), batches that repeat a short
base list (cyclic: the restatement runs on the base items only, counts and pass words are sums over the residues' multiplicities, in
exact integers), the base lists themselves, and a vectorised generator of frontier_ref.cells_cloud's lattices for a million cells.
Shared by the CPU tier (tests/test_edge_shapes_host.py) and the GPU tier (tests/test_gpu_count_edges.py).  Test infrastructure only."""
import math

import numpy as np

from tests import clear_ref as cr
from tests import clearance_ref as clr
from tests import frontier_ref as fr
from tests import query_ref as qr

# ---- the constants, and the counts derived from them ---------------------------------------------------------------------------------
EDGES = dict(
    grid_block=256, grid_max_blocks=2048,       # grid_for(n, 256, 2048) and grid_for's defaults (kBlock, 256 * 8)
    grid_cap=524_288,                           # threads of the largest launch: item grid_cap is the first of a loop's second trip
    kCropT=256, kCropV=4, kCropTile=1024,       # rows per thread and per workgroup of crop_keep_mask / k_crop_scatter / frontier_tally
    kCropScanT=1024,                            # tiles per chunk of the one-workgroup scans (k_crop_scan, k_frontier_scan)
    scan_carry_rows=1_048_576,                  # kCropScanT * kCropTile: the first row of the scans' second chunk
    kScoreTile=256, kScoreReduceBlock=1024,
    score_reduce_unroll=4, score_reduce_stride=4096,       # k_score_reduce: tiles t, t + 1024, t + 2048, t + 3072 a pass
    derivs_reduce_unroll=2, derivs_reduce_stride=2048,     # k_score_derivs_reduce
    score_reduce_points=1_048_576,              # score_reduce_stride * kScoreTile: point 1 048 576 opens tile 4096
    derivs_reduce_points=524_288,               # derivs_reduce_stride * kScoreTile: point 524 288 opens tile 2048
    patch_reduce_blocks=512,                    # grid_for(n, 256, 512): k_patch_reduce and k_patch_moments<true> (gndt_api_patch.hip)
    patch_reduce_cap=131_072,                   # row patch_reduce_cap is the first of their second trip
    kPatchSlots=8, kPatchWaveMin=4,             # k_patch_moments' tagged LDS slots; rows of a patch in a wave from which they are combined
)
assert EDGES["grid_cap"] == EDGES["grid_block"] * EDGES["grid_max_blocks"]
assert EDGES["kCropTile"] == EDGES["kCropT"] * EDGES["kCropV"] and EDGES["scan_carry_rows"] == EDGES["kCropScanT"] * EDGES["kCropTile"]
assert EDGES["score_reduce_stride"] == EDGES["score_reduce_unroll"] * EDGES["kScoreReduceBlock"]
assert EDGES["derivs_reduce_stride"] == EDGES["derivs_reduce_unroll"] * EDGES["kScoreReduceBlock"]
assert EDGES["score_reduce_points"] == EDGES["score_reduce_stride"] * EDGES["kScoreTile"]
assert EDGES["derivs_reduce_points"] == EDGES["derivs_reduce_stride"] * EDGES["kScoreTile"]
assert EDGES["patch_reduce_cap"] == EDGES["grid_block"] * EDGES["patch_reduce_blocks"]

CAP = EDGES["grid_cap"]
BASE = 4093            # prime: coprime to 64, 256 and 524 288, so a lane's item of the second trip is another one than of the first
assert all(BASE % p for p in range(2, int(math.isqrt(BASE)) + 1)) and math.gcd(BASE, CAP) == 1

WAVE_COUNTS = (1, 63, 64, 65)
CAST_COUNTS = WAVE_COUNTS + (CAP, CAP + 1, CAP + 65)
QUERY_COUNTS = (CAP, CAP + 1)
QUERY_ILP4_COUNT = 4 * CAP + 1
SCORE_COUNTS = (1, 255, 256, 257, 262_144, 262_145, EDGES["score_reduce_points"], EDGES["score_reduce_points"] + 1)
CROP_ROWS = {1: (1, 1), 2: (1, 2), 3: (1, 3), 4: (2, 2), 5: (1, 5), 1023: (31, 33), 1024: (32, 32), 1025: (25, 41), 1026: (27, 38),
             1_048_576: (1024, 1024), 1_048_577: (17, 61_681)}                  # rows -> (W, H) of the one-storey lattice
assert all(w * h == n for n, (w, h) in CROP_ROWS.items())


def cyclic(base, n):
    """item i is base[i % len(base)]"""
    base = np.asarray(base)
    return np.ascontiguousarray(base[np.arange(int(n), dtype=np.int64) % len(base)])


def multiplicity(n, m=BASE):
    """how often each of the m base items occurs among the first n items of a cyclic batch (int64 [m]; the sum is n)"""
    q, r = divmod(int(n), int(m))
    return q + (np.arange(m, dtype=np.int64) < r).astype(np.int64)


def tail_items(n, m=BASE, first=CAP):
    """the base indices of the items first .. n - 1 of a cyclic batch (those of the second grid-stride trip), in order"""
    return np.arange(first, max(int(n), first), dtype=np.int64) % m


# ---- lattices --------------------------------------------------------------------------------------------------------------------------
def lattice_cells(W, H, holes=(), count=None, tail=()):
    """-> (ix, iy) int64 arrays of the cells ix = 0 .. W-1 outer, iy = 0 .. H-1 inner, without the cells of `holes` ((ix, iy) pairs),
    cut to the first `count` of them, then the cells of `tail`"""
    k = np.arange(W * H, dtype=np.int64)
    holes = np.asarray(list(holes), np.int64).reshape(-1, 2)
    if len(holes):
        keep = np.ones(W * H, bool)
        keep[holes[:, 0] * H + holes[:, 1]] = False
        k = k[keep]
    if count is not None:
        assert count <= len(k)
        k = k[:count]
    ix, iy = np.divmod(k, H)
    tail = np.asarray(list(tail), np.int64).reshape(-1, 2)
    return np.concatenate([ix, tail[:, 0]]), np.concatenate([iy, tail[:, 1]])


def lattice_points(W, H, holes=(), count=None, tail=()):
    """The points frontier_ref.cells_cloud draws for lattice_cells(W, H, holes, count, tail): the origin point, then 3 x 3 points a cell
    with the same ripple, in the same order, from the same float64 expressions.  One storey, one node per column, every one a slope;
    rows follow first sight, so row r is cell r."""
    return cells_points(*lattice_cells(W, H, holes, count, tail))


def cells_points(ix, iy):
    """lattice_points for any list of cells (ix, iy), in their order"""
    k = ix
    ab = np.array([0.12, 0.25, 0.38])
    x = np.broadcast_to((ix * fr.GL)[:, None, None] + ab[None, :, None], (len(k), 3, 3))
    y = np.broadcast_to((iy * fr.GL)[:, None, None] + ab[None, None, :], (len(k), 3, 3))
    z = fr.Z_FLOOR + 0.002 * np.sin(7 * x) * np.cos(5 * y)
    pts = np.empty((1 + 9 * len(k), 3), np.float32)
    pts[0] = fr.ORIGIN
    pts[1:, 0], pts[1:, 1], pts[1:, 2] = x.reshape(-1), y.reshape(-1), z.reshape(-1)
    return pts


FLOOR_LINE = 256        # cells a line of floors_cells: a line is a workgroup's rows


def stripes_cells(H, lines):
    """-> (ix, iy) of the cells (2 i, j), i < lines outer, j < H inner: every second line of cells is empty, so line i is a patch of its
    own under every connectivity — H rows, the rows i H .. i H + H - 1, labelled i H"""
    i, j = np.divmod(np.arange(lines * H, dtype=np.int64), H)
    return 2 * i, j


def floors_cells(a, n):
    """-> (ix, iy) of two floors of lines of FLOOR_LINE cells: the first `a` cells line after line, two empty lines, then n - a cells
    line after line: two patches, the rows 0 .. a - 1 labelled 0 and the rows a .. n - 1 labelled a"""
    assert 0 < a < n
    k = np.arange(n, dtype=np.int64)
    second = k >= a
    k = np.where(second, k - a, k)
    first_lines = -(-a // FLOOR_LINE)
    return k // FLOOR_LINE + np.where(second, first_lines + 2, 0), k % FLOOR_LINE


# The surface patches' scenes (tests/test_gpu_patch_edges.py on the device, tests/test_patch_fast_ref_host.py on the oracle's maps)
PATCH_TRIP = EDGES["patch_reduce_cap"]
STRIPES = {3: 70, 4: 70, 5: 70, 16: 20, 96: 5}                     # H -> lines: 210 to 480 rows, one and two workgroups
FLOORS_N = 2 * PATCH_TRIP + 4096 + 65                              # three trips of the reductions, the last wave of one row
FLOORS_A = (PATCH_TRIP + 4096 + 30, PATCH_TRIP + 4096 + 3)         # the second floor's first row: 30 / 3 rows into a wave of trip 2
TRIP_STRIPES = (64, 2100)                                          # a wave a patch, 3 328 rows behind the first trip


def wave_groups(patch_of_row, wave=64):
    """the rows of one patch in one wave, for rows 0 .. n - 1 -> (wave, patch, rows) arrays, in row order"""
    p = np.asarray(patch_of_row, np.int64)
    w = np.arange(len(p), dtype=np.int64) // wave
    start = np.flatnonzero(np.r_[True, (p[1:] != p[:-1]) | (w[1:] != w[:-1])])
    return w[start], p[start], np.diff(np.r_[start, len(p)])


def pitch_holes(W, H, px=37, py=41):
    """holes at a fixed pitch, away from the border: every px-th by py-th cell"""
    return [(ix, iy) for ix in range(px // 2, W - 1, px) for iy in range(py // 2, H - 1, py) if ix > 0 and iy > 0]


def edge_lattice(n):
    """The lattice of exactly n rows for the row-count edges -> (points, cells (ix, iy)): CROP_ROWS[n]'s W x H floor with holes at a
    pitch of 37 x 41 cells (5 along an axis of at most 41 cells), so that frontier rows and small clusters lie in every tile, as many
    further cells of the next lines as the holes took, and the LAST row a cell on its own two columns away: a cluster of one whose
    root lies in the last tile, a kept or dropped row behind every other."""
    W, H = CROP_ROWS[n]
    if n < 1023:
        holes, lines = [], W
    else:
        holes = pitch_holes(W, H, 37 if W > 41 else 5, 41 if H > 41 else 5)
        lines = W + len(holes) // H + 1
    args = (lines, H, holes, n - 1, [(lines + 2, 0)])
    return lattice_points(*args), lattice_cells(*args)


def cell_centres(sx, sy):
    """the centre point of the lattice cells with signed indices (sx, sy) >= 1, at the floor's height"""
    sx, sy = np.asarray(sx, np.float64), np.asarray(sy, np.float64)
    return np.stack([(sx - 1) * fr.GL + 0.25, (sy - 1) * fr.GL + 0.25, np.full(sx.shape, fr.Z_FLOOR)], 1).astype(np.float32)


# ---- the small map and the base lists of its batches ----------------------------------------------------------------------------------
SMALL = "41x25"          # clearance_ref.LATTICES: 41 x 25 cells of 0.5 m from (0, 0), floor at level 1, a wall a metre higher on iy = 12
P = fr.P
ORIGIN = fr.ORIGIN


def small_cloud():
    return clr.lattice(SMALL)


def _floor_points():
    return small_cloud()[1:]


CAST_SENSOR = np.float32([10.2, 3.1, 2.5])


def cast_base():
    """-> (sensor, origins [BASE, 3], ends [BASE, 3]): rays from above the floor through it (hits), every eighth from item 1 lifted into
    the sky and every eighth from item 5 led away from the map (misses), items 2 mod 16 NaN and 3 mod 64 infinite (skipped).  Item 384
    = 524 288 mod BASE, the one item of the second trip at n = 524 289, is a ray through the floor."""
    rng = np.random.default_rng(41)
    i = np.arange(BASE)
    ends = np.stack([rng.uniform(0.3, 20.2, BASE), rng.uniform(0.3, 12.2, BASE), np.full(BASE, -0.5)], 1).astype(np.float32)
    sky = i % 8 == 1
    ends[sky, 2] = CAST_SENSOR[2] + np.float32(5.0)
    away = i % 8 == 5
    ends[away, 0] = rng.uniform(-30.0, -8.0, int(away.sum())).astype(np.float32)
    ends[away, 2] = np.float32(2.0)
    ends[i % 16 == 2] = np.nan
    ends[i % 64 == 3, 1] = np.inf
    origins = (CAST_SENSOR[None, :] + rng.uniform(-0.3, 0.3, (BASE, 3))).astype(np.float32)
    return CAST_SENSOR, origins, ends


CLEAR_SENSOR = np.float32([10.2, 3.1, 0.2])


def clear_base():
    """-> (sensor, end points [BASE, 3]): the sensor stands inside the floor's level, so that a ray to a floor point passes through
    every floor node on its way; three of four end points are points of the map's own cloud (their nodes are protected), every fourth
    hangs above the floor, items 2 mod 16 are NaN"""
    rng = np.random.default_rng(43)
    floor = _floor_points()
    i = np.arange(BASE)
    pts = floor[rng.integers(0, len(floor), BASE)].copy()
    up = i % 4 == 3
    pts[up, 2] += rng.uniform(0.5, 2.0, int(up.sum())).astype(np.float32)
    pts[i % 16 == 2] = np.nan
    return CLEAR_SENSOR, np.ascontiguousarray(pts, np.float32)


def query_base():
    """-> points [BASE, 3]: items 0 and 2 mod 4 are points of the map's own cloud (NODE and NEAREST_SLOPE name a row), 1 mod 4 lie off
    the map (no row either way), 3 mod 4 over a map column at another height (a row for NEAREST_SLOPE, mostly none for NODE), and
    items 5 mod 128 are NaN.  Items 384 (= 524 288 mod BASE) and 1536 (= 2 097 152 mod BASE) are map points."""
    rng = np.random.default_rng(47)
    floor = _floor_points()
    i = np.arange(BASE)
    pts = floor[rng.integers(0, len(floor), BASE)].copy()
    off = i % 4 == 1
    pts[off, 0] = rng.uniform(-9.0, -1.0, int(off.sum())).astype(np.float32)
    high = i % 4 == 3
    pts[high, 2] = rng.uniform(-3.0, 3.0, int(high.sum())).astype(np.float32)
    pts[i % 128 == 5] = np.nan
    return np.ascontiguousarray(pts, np.float32)


def scan_base():
    """-> points [BASE, 3]: points of the map's own cloud moved by a few centimetres (upwards: they stay in their node's level), every
    sixteenth from item 7 on far off the map"""
    rng = np.random.default_rng(53)
    floor = _floor_points()
    jitter = rng.normal(0.0, 0.02, (BASE, 3))
    jitter[:, 2] = np.abs(jitter[:, 2])
    pts = floor[rng.integers(0, len(floor), BASE)] + jitter.astype(np.float32)
    pts[np.arange(BASE) % 16 == 7, 0] += np.float32(500.0)
    return np.ascontiguousarray(pts, np.float32)


def scan_poses():
    """K = 3: the identity, a tenth of a cell along x, a yaw of one degree about the map's middle"""
    a = math.radians(1.0)
    c, s = math.cos(a), math.sin(a)
    cx, cy = 10.25, 6.25
    yaw = np.array([[c, -s, 0, cx - c * cx + s * cy], [s, c, 0, cy - s * cx - c * cy], [0, 0, 1, 0]], np.float64)
    eye = np.eye(4)[:3]
    shift = eye.copy()
    shift[0, 3] = 0.1 * fr.GL
    return np.stack([eye, shift, yaw])


# ---- expected answers of a cyclic batch from its base list's ---------------------------------------------------------------------------
def clear_words(cells, sensor, base_pts, n, max_range=0.0, end_margin=0.0):
    """-> (words uint32 [rows], rays, skipped) of the cyclic batch of n end points: every base ray's voxels weighted by its
    multiplicity, exact integers; a row is protected when a base end point that occurs names it"""
    mult = multiplicity(n, len(base_pts))
    ok, cols = cr.rays(ORIGIN, P["grid_len"], P["z_len"], sensor, base_pts, max_range, end_margin)
    rows_n = int(cells["num_nodes"])
    keys = qr.pack(cells["sx"], cells["sy"], cells["sz"])
    order = np.argsort(keys, kind="stable")
    ks = keys[order]
    ray, sx, sy, sz = cr.voxels(cols)
    vk = qr.pack(sx, sy, sz)
    pos = np.minimum(np.searchsorted(ks, vk), rows_n - 1)
    hit = ks[pos] == vk
    words = np.zeros(rows_n, np.int64)
    np.add.at(words, order[pos[hit]], mult[ray[hit]])
    assert words.max() < 1 << 31
    words = words.astype(np.uint32)
    used = ok & (mult > 0)
    prot = qr.node_rows(cells, np.asarray(base_pts, np.float32)[used], ORIGIN, P["grid_len"], P["z_len"])
    words[prot[prot >= 0]] |= cr.PROTECTED
    return words, int(mult[ok].sum()), int(mult[~ok].sum())


def weighted_score(per, mult):
    """the four sums of a cyclic scan from a base scan's per-pose answer (score_ref.score_pose): sum of multiplicity x term, the
    floats by math.fsum of the float64 products (a multiplicity below 2^53 / term count is exact as a float64), the counts exact"""
    D, R = per["all_d2"], per["all_rows"]
    valid = R != qr.NO_ROW
    w = np.broadcast_to(np.asarray(mult, np.int64)[:, None], D.shape)
    terms = D[valid]
    wf = w[valid].astype(np.float64)
    return dict(score=math.fsum((wf * np.exp(-0.5 * terms)).tolist()), d2_sum=math.fsum((wf * terms).tolist()),
                terms=int(w[valid].sum()), matched=int(np.asarray(mult, np.int64)[valid.any(1)].sum()))


def weighted_derivs(per, mult):
    """g, H and their absolute-value twins of a cyclic scan from score_derivs_ref.derivs_pose's per-point values of the base scan"""
    from tests import score_derivs_ref as dr
    wf = np.asarray(mult, np.float64)[:, None]
    tot = np.array([math.fsum(c.tolist()) for c in (wf * per["vals"]).T])
    tab = np.array([math.fsum(c.tolist()) for c in (wf * per["vabs"]).T])
    return dict(g=tot[:6], H=dr._full(tot[6:]), g_abs=tab[:6], H_abs=dr._full(tab[6:]))


def stack_poses(per_pose):
    """per-pose dicts of sums -> one dict of length-K arrays, as the assertions of score_ref / score_derivs_ref take them"""
    return {k: np.array([p[k] for p in per_pose], np.int64 if k in ("matched", "terms") else np.float64) for k in per_pose[0]}
