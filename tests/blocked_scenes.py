"""Scenes for BLOCKED buckets (gndt_blocked.hpp) and a numpy restatement of the rule that lays the blocks out (blocked_decide,
gndt_api_build.hip): one dense, evenly filled box per block shape of k_bucket_blocked — 512, 256, 128, 64, 32 and 16 columns per block
(shz = 0 .. 5) — among them boxes that do not straddle the origin, a moved origin, a box that leaves level padding in its blocks and a
scene whose adjacent-level means lie about one slope interval apart.  Shared by tests/test_blocked_scenes_host.py (the fixtures hold
on the CPU oracle) and tests/test_gpu_blocked_shapes.py (the device takes exactly these layouts and gives the oracle's maps)."""
import contextlib
import functools

import numpy as np

from grid_ndt_amd import scenes

SEED = 0x5EED0B10
POINTS = 1_100_000      # the smallest useful size: blocked buckets need 2^20 points and at least 64 blocks of 1 500 .. 5 000 points
INTERVAL = 0.08
K_MAX_FAN = 512         # (gndt_partition.hpp: up to 512 x 512 buckets)

LAYOUT_FIELDS = ("state", "x0", "y0", "z0", "shx", "shy", "shz", "nx", "ny", "buckets")


def _around(origin, ext):
    o, e = np.float64(origin), np.float64(ext)
    return tuple(o - e), tuple(o + e)


def _scene(cells, origin, lo, hi, levels, block, blocks, nodes, below_min, zpad=0):
    return dict(grid_len=cells[0], z_len=cells[1], origin=origin, lo=lo, hi=hi, levels=levels, block=block, blocks=blocks, nodes=nodes,
                below_min=below_min, zpad=zpad)


# name -> cells (xy, z), origin, box, and what the oracle's map of the seed-SEED cloud is: levels (Z), a block's columns along x, columns
# along y and levels, blocks along x and y (margin included), nodes, nodes below min_points = 3, level padding under the box
SCENES = {
    "flat_1": _scene((0.5, 0.5), (0.0, 0.0, 0.0), (-88.0, -88.0, 0.05), (88.0, 88.0, 0.45), 1, (32, 16, 1), (13, 24), 123_891, 854),
    "levels_2": _scene((0.5, 0.5), (0.0, 0.0, 0.0), (-64.0, -64.0, -0.45), (64.0, 64.0, 0.45), 2, (16, 16, 2), (18, 18), 131_035, 1_266),
    "levels_4_at_interval": _scene((0.5, 0.08), (0.0, 0.0, 0.0), (-44.0, -44.0, -0.16), (44.0, 44.0, 0.16), 4, (16, 8, 4), (13, 24),
                                   123_886, 877),
    "levels_3_positive": _scene((0.5, 0.08), (0.0, 0.0, 0.0), (10.0, -98.0, 0.0), (98.0, -10.0, 0.24), 3, (16, 8, 4), (14, 24), 92_927, 68),
    "levels_6_padded": _scene((0.5, 0.25), (-3.1, 4.7, -1.2), *_around((-3.1, 4.7, -1.2), (32.0, 32.0, 0.75)), 6, (8, 8, 8), (18, 18),
                              98_302, 96, zpad=1),
    "levels_16_off_origin": _scene((0.5, 0.25), (0.0, 0.0, 0.0), (10.0, -70.0, 1.0), (58.0, -22.0, 5.0), 16, (8, 4, 16), (15, 26),
                                   147_393, 2_970),
    "levels_32_moved_origin": _scene((0.25, 0.1), (37.3, -21.7, 2.9), *_around((37.3, -21.7, 2.9), (8.0, 8.0, 1.6)), 32, (4, 4, 32), (18, 18),
                                     131_049, 1_277),
}
# levels_4_at_interval: 84 680 slopes and 34 966 `down` labels (demand slope) — the threshold |dz| > interval falls on both sides —
# and 7 290 nodes without statistics at min_points = 5
AT_INTERVAL = dict(slopes=84_680, down=34_966, below_min_5=7_290)
FOLDED_NODES = 61_952      # (levels_4_at_interval with its inner two levels folded outward: 176 x 176 columns x levels -2 and 2)


def params(name, demand="slope", min_points=3):
    s = SCENES[name]
    return dict(grid_len=s["grid_len"], z_len=s["z_len"], slope_interval=INTERVAL, demand=demand, min_points=min_points)


def box(seed, lo, hi, n=POINTS):
    """n points: axis a of point i is lo[a] + u01(3 i + a, seed) * (hi[a] - lo[a]), rounded to float32."""
    i = np.arange(n, dtype=np.uint64) * np.uint64(3)
    out = np.empty((n, 3), np.float32)
    for a in range(3):
        out[:, a] = float(lo[a]) + scenes.u01(i + np.uint64(a), seed) * (float(hi[a]) - float(lo[a]))
    return out


@functools.lru_cache(maxsize=4)
def cloud(name, seed=SEED):
    """[origin] + box of the scene, read-only (shared between tests)."""
    s = SCENES[name]
    c = np.concatenate([np.float32([s["origin"]]), box(seed, s["lo"], s["hi"])], 0)
    c.setflags(write=False)
    return c


def folded(c):
    """levels_4_at_interval with the inner two levels folded outward: |z| < 0.08 -> z +- 0.08, clipped to +-0.16, an exact zero to 0.1.
    Only levels -2 and 2 are occupied: half the nodes of the unfolded cloud in the same box."""
    out = c.copy()
    z = out[1:, 2].astype(np.float64)
    inner = np.abs(z) < 0.08
    z = np.where(inner, np.where(z == 0.0, 0.1, z + np.copysign(0.08, z)), z)
    out[1:, 2] = np.clip(z, -0.16, 0.16)
    return out


def contiguous(s):
    """Signed indices skip 0; c = s > 0 ? s - 1 : s is contiguous (contiguous_index, gndt_math.hpp)."""
    s = np.asarray(s, np.int64)
    return np.where(s > 0, s - 1, s)


def extent(ref):
    """(x0, y0, z0), (X, Y, Z): the box an oracle map occupies, in contiguous indices."""
    c = [contiguous(ref[k]) for k in ("sx", "sy", "sz")]
    lo = tuple(int(v.min()) for v in c)
    return lo, tuple(int(v.max()) - l + 1 for v, l in zip(c, lo))


def plan(ref, n):
    """blocked_decide restated on an oracle map of a cloud of n points (the origin row not counted): the layout the handle must hold
    after a first build of that cloud, as TwoDmap.block_layout() reports it — or {"state": -1}."""
    (x0, y0, z0), (X, Y, Z) = extent(ref)
    nodes, biggest = int(ref["num_nodes"]), int(ref["count"].max())
    no = {"state": -1}
    if nodes < 1024 or Z > 32:
        return no
    shz = 0
    while (1 << shz) < Z:
        shz += 1
    for shz in range(shz, 6):
        shx = (9 - shz + 1) // 2
        shy = 9 - shz - shx
        nx, ny = (X + (1 << shx) - 1) >> shx, (Y + (1 << shy) - 1) >> shy
        B = nx * ny
        if B < 64 or B > K_MAX_FAN * K_MAX_FAN:
            continue
        per_block = n // B
        if per_block > 5000:
            continue
        if per_block < 1500:              # sparse boxes: mostly empty blocks
            break
        if biggest * 4 > per_block:       # a node that holds a quarter of a block's points
            break
        if nodes * 8 < B * 512:           # less than an eighth of the slots used
            break
        zpad = ((1 << shz) - Z) // 2      # the levels centred in the block's height
        buckets = (nx + 2) * (ny + 2)     # one block of margin on every side
        if buckets > K_MAX_FAN * K_MAX_FAN:
            continue
        return dict(state=1, x0=x0 - (1 << shx), y0=y0 - (1 << shy), z0=z0 - zpad, shx=shx, shy=shy, shz=shz, nx=nx + 2, ny=ny + 2,
                    buckets=buckets)
    return no


def perfect_build(ref):
    """What a build without any error of its own exports: the oracle's fp64 truth (mean64, cov64) rounded to float32, zeros where a node
    has no statistics, everything else the oracle's."""
    has = (ref["flags"].astype(np.int64) & 1) != 0
    out = {k: ref[k] for k in ("num_nodes", "num_columns", "sx", "sy", "sz", "count", "first_idx", "flags", "rough", "normal")}
    out["num_slopes"] = int(np.count_nonzero(ref["flags"].astype(np.int64) & 2))
    out["mean"] = np.where(has[:, None], ref["mean64"], 0.0).astype(np.float32)
    out["cov"] = np.where(has[:, None], ref["cov64"], 0.0).astype(np.float32)
    return out


# ---- small scenes: the same block shapes at an eighth of the points (tests/test_gpu_blocked_small.py) -----------------------------------
# The 2^20-point floor under blocked buckets is a tuning choice of the host (Tuning::blocked_min_points), not a limit of the kernel:
# with the floor lowered (GNDT_DEBUG_BLOCKED_MIN_POINTS) and strategy PARTITION_TWO_LEVEL a cloud of 131 072 points in 8 x 8 blocks of
# 2 048 points takes them.  Every small scene has the cells and origin of its large twin; its box is cut to 8 x 8 blocks around the
# large box's centre in x and y.
SMALL_POINTS = 131_072
SMALL_FLOOR = 65_536      # what the tests lower the floor to
TWO_LEVEL = 4             # GNDT_STRATEGY_PARTITION_TWO_LEVEL
HASHED, BLOCKED = 2, 7    # GNDT_STRATEGY_PARTITION, GNDT_STRATEGY_PARTITION_BLOCKED: what gndt_last_strategy reports of such builds


def _small(twin, lo, hi, nodes, box, corner, sh):
    s = SCENES[twin]
    return dict(grid_len=s["grid_len"], z_len=s["z_len"], origin=s["origin"], lo=lo, hi=hi, nodes=nodes, box=box,
                layout=dict(state=1, x0=corner[0], y0=corner[1], z0=corner[2], shx=sh[0], shy=sh[1], shz=sh[2], nx=10, ny=10, buckets=100))


# name -> the box, the oracle's node count of the seed-SEED cloud, the box its map occupies (columns along x, along y, levels) and the
# layout blocked_decide takes for it: corner (contiguous indices, margin and level padding included) and log2 of a block's sides
SMALL_SCENES = {
    "flat_1": _small("flat_1", (-64.0, -32.0, 0.05), (64.0, 32.0, 0.45), 32_180, (256, 128, 1), (-160, -80, 0), (5, 4, 0)),
    "levels_2": _small("levels_2", (-32.0, -32.0, -0.45), (32.0, 32.0, 0.45), 32_173, (128, 128, 2), (-80, -80, -1), (4, 4, 1)),
    "levels_4_at_interval": _small("levels_4_at_interval", (-32.0, -16.0, -0.16), (32.0, 16.0, 0.16), 32_183, (128, 64, 4), (-80, -40, -2),
                                   (4, 3, 2)),
    "levels_3_positive": _small("levels_3_positive", (22.0, -70.0, 0.0), (86.0, -38.0, 0.24), 24_463, (128, 64, 3), (28, -148, 0), (4, 3, 2)),
    "levels_6_padded": _small("levels_6_padded", (-19.1, -11.3, -1.95), (12.9, 20.7, -0.45), 24_452, (64, 64, 6), (-40, -40, -4), (3, 3, 3)),
    "levels_16_off_origin": _small("levels_16_off_origin", (18.0, -54.0, 1.0), (50.0, -38.0, 5.0), 32_149, (64, 32, 16), (28, -112, 4),
                                   (3, 2, 4)),
    "levels_32_moved_origin": _small("levels_32_moved_origin", (33.3, -25.7, 1.3), (41.3, -17.7, 4.5), 32_189, (32, 32, 32), (-20, -20, -16),
                                     (2, 2, 5)),
}


SMALL_FOLDED_NODES = 16_383      # (small levels_4_at_interval with its inner two levels folded outward, `folded`: levels -2 and 2 only)


def small_params(name, demand="slope", min_points=3):
    return params(name, demand, min_points)      # (the large twin's cells)


@functools.lru_cache(maxsize=16)
def small_cloud(name, seed=SEED):
    """[origin] + SMALL_POINTS points of the small scene's box, read-only (shared between tests)."""
    s = SMALL_SCENES[name]
    c = np.concatenate([np.float32([s["origin"]]), box(seed, s["lo"], s["hi"], SMALL_POINTS)], 0)
    c.setflags(write=False)
    return c


# ---- fuzzed boxes --------------------------------------------------------------------------------------------------------------------------
FUZZ_CELLS = ((0.5, 0.5), (0.5, 0.08), (0.5, 0.25), (0.25, 0.1), (1.0, 0.25), (0.2, 0.2))
FUZZ_LEVELS = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32)      # the powers of two and their neighbours
FUZZ_FAR = 30_000          # columns out at most: inside the flood's +-32 767
FUZZ_INSET = 0.06          # of a cell, between the box's faces and the cell borders: far above float32's step 15 000 m out (1e-3 m)


def _log2_ceil(v):
    s = 0
    while (1 << s) < v:
        s += 1
    return s


def _corner(r, extent, far):
    """The first contiguous index of `extent` cells along one axis: the box all-negative, ending on index -1 or starting on index 1
    (either side of the skipped 0), straddling the origin, or (columns only) thousands of cells out on either side."""
    mode = int(r.integers(6 if far else 4))
    if mode == 0:
        return -extent - int(r.integers(1, 200))
    if mode == 1:
        return -extent                                 # its last cell is signed index -1
    if mode == 2:
        return 0                                       # its first cell is signed index 1
    if mode == 3:
        return -int(r.integers(1, extent)) if extent > 1 else 0
    out = int(1000.0 * (far / 1000.0 - 1.0) ** float(r.random()))      # 1 000 .. far - 1 000 cells, every decade alike
    return out if mode == 4 else -out - extent


def random_box(seed, blocks=(8, 10), at_least=0):
    """A seeded dense box for the blocked kernel: cells from FUZZ_CELLS, 1 .. 32 levels (often a power of two or its neighbour),
    blocks[0] .. blocks[1] blocks along x and y with an extent that is NOT a multiple of the block, a corner anywhere _corner puts it
    (every fourth box all-negative on all three axes), an origin off the lattice, min_points 1, 3 or 5 and either demand.  n: 1 700 ..
    4 500 points per block and fewer than 200 000 in all — or, with `at_least`, the first block fill that gives that many points.
    -> dict(grid_len, z_len, origin, lo, hi, n, min_points, demand, box=(X, Y, Z), corner=(cx, cy, cz))."""
    r = np.random.default_rng(seed)
    grid_len, z_len = FUZZ_CELLS[int(r.integers(len(FUZZ_CELLS)))]
    Z = FUZZ_LEVELS[int(r.integers(len(FUZZ_LEVELS)))] if int(r.integers(4)) else int(r.integers(1, 33))
    shz = _log2_ceil(Z)
    shx = (9 - shz + 1) // 2
    shy = 9 - shz - shx
    nbx, nby = (int(v) for v in r.integers(blocks[0], blocks[1] + 1, 2))
    X = (nbx << shx) - int(r.integers(1, 1 << shx))
    Y = (nby << shy) - int(r.integers(1, 1 << shy))
    B = nbx * nby
    if at_least:
        per = -(-at_least // B) + int(r.integers(1, 200))
    else:
        per = int(r.integers(1700, min(4500, 199_999 // B) + 1))
    assert 1700 <= per <= 4500, (seed, B, per)
    n = B * per + int(r.integers(B))
    if int(r.integers(4)) == 0:
        corner = tuple(-e - int(r.integers(1, 200)) for e in (X, Y, Z))
    else:
        corner = (_corner(r, X, FUZZ_FAR), _corner(r, Y, FUZZ_FAR), _corner(r, Z, 0))
    origin = np.float32(r.random(3) * 40.0 - 20.0)
    cells = (grid_len, grid_len, z_len)
    lo = tuple(float(origin[a]) + (corner[a] + FUZZ_INSET) * cells[a] for a in range(3))
    hi = tuple(float(origin[a]) + (corner[a] + e - FUZZ_INSET) * cells[a] for a, e in enumerate((X, Y, Z)))
    return dict(grid_len=grid_len, z_len=z_len, origin=tuple(float(v) for v in origin), lo=lo, hi=hi, n=n,
                min_points=(1, 3, 5)[int(r.integers(3))], demand=("slope", "true")[int(r.integers(2))], box=(X, Y, Z), corner=corner)


# The seeds in use.  tests/test_blocked_scenes_host.py holds every one of them to plan() -> state 1 and to parity.compare's strict
# gates on the oracle alone, labels_of_perfect_build included; a seed that fails any is REPLACED here, not skipped or given a wider gate.  Of the seeds 100 .. 259, 74
# pass both.  The others fail the gates on the ORACLE's own map, for two reasons that have nothing to do with a build: a corner beyond
# ~5 000 columns (float32 coordinates resolve 2^-24 of the distance, so the fp32 oracle's covariances leave the fp64 truth: boxes
# begin to fail at 4 300 columns out and every one from 4 700 on does) and min_points = 1 on boxes with 3 .. 9 points per node (more than 0.1 % of
# the nodes then hold one or two points: no covariance to compare; seed 142, with 16 points per node, passes).  So the seeds in use reach
# 4 674 columns out, not the generator's 30 000.
# Among them: every cell pair; 1, 2, 4, 8, 16 and 32 levels and 7, 15, 17, 18 and 31; boxes all-negative on all three axes (108, 146, 232),
# ending on index -1 (105, 106, 182, 232) and starting on index 1 (102, 120, 133, 242); 1 100 .. 4 700 columns out on either side (117, 141,
# 142, 167, 191, 226); min_points 1, 3 and 5; both demands.
FUZZ_SEEDS = (102, 105, 106, 108, 117, 120, 133, 141, 142, 146, 167, 182, 191, 226, 232, 242)
# One more box of just over 16 384 x 32 points: more bitmap words than k_place_emit_rows takes (Tuning::place_emit_words), so its blocked
# builds order and emit through the separate passes and k_emit_rows, like a production-size one
# (seeds 1000 .. 1011: 1003 and 1011 pass the gates on the oracle alone and still cannot be used — each has ONE node whose label
#  decision lies inside the oracle's own fp32 error, labels_of_perfect_build below; 1010 has none)
FUZZ_SEED_SEPARATE_PASSES = 1010
SEPARATE_PASSES_POINTS = 16_384 * 32


def fuzz_box(seed):
    if seed == FUZZ_SEED_SEPARATE_PASSES:
        return random_box(seed, blocks=(12, 13), at_least=SEPARATE_PASSES_POINTS)
    return random_box(seed)


def fuzz_params(b):
    return dict(grid_len=b["grid_len"], z_len=b["z_len"], slope_interval=INTERVAL, demand=b["demand"], min_points=b["min_points"])


@functools.lru_cache(maxsize=4)
def fuzz_cloud(seed, cloud_seed=SEED):
    b = fuzz_box(seed)
    c = np.concatenate([np.float32([b["origin"]]), box(cloud_seed ^ seed, b["lo"], b["hi"], b["n"])], 0)
    c.setflags(write=False)
    return c


# ---- the lifetime of the layout on one handle -------------------------------------------------------------------------------------------
def fits(ref, lay):
    """Every node of the map lies in a block of the layout: a blocked build of its cloud meets no record outside the box."""
    (x0, y0, z0), (X, Y, Z) = extent(ref)
    return (lay["x0"] <= x0 and x0 + X <= lay["x0"] + (lay["nx"] << lay["shx"]) and lay["y0"] <= y0 and
            y0 + Y <= lay["y0"] + (lay["ny"] << lay["shy"]) and lay["z0"] <= z0 and z0 + Z <= lay["z0"] + (1 << lay["shz"]))


class LayoutMemory:
    """Part::blk_state / blk_n / blk_map restated (partition_launch, partition_resolve, blocked_decide, gndt_set_origin), for clouds
    without locality built eagerly by the two-level partition on a handle that never recorded a hipGraph:
      * a decision holds for a size window: n <= blk_n + blk_n / 4 and n + n / 4 >= blk_n.  Inside it a "yes" makes the build blocked
        and nothing is decided again; outside it the build is hashed and its map decides anew (plan), for its own size;
      * a blocked build that meets a record outside the box (or a region that overflows: not with these evenly filled boxes) says "no"
        for the window and is re-run hashed — one re-run;
      * an origin change resets to "not looked at".
    `retries` counts the re-runs the layout causes; a build may be re-run for room as well (a first cloud, a larger one)."""

    def __init__(self, floor=1 << 20):
        self.floor, self.state, self.n, self.layout, self.retries = floor, 0, 0, None, 0

    def in_window(self, n):
        return n <= self.n + self.n // 4 and n + n // 4 >= self.n

    def set_origin(self, changed=True):
        if changed:
            self.state = 0

    def build(self, ref, n):
        """One build of a cloud of n points (the origin row not counted) whose oracle map is `ref` -> the strategy it ends as."""
        blocked = self.state == 1 and n >= self.floor and self.in_window(n)
        if blocked and not fits(ref, self.layout):
            self.state, blocked = -1, False
            self.retries += 1
        if not blocked and not (self.state != 0 and self.in_window(n)):      # blocked_decide, behind every build that ended hashed
            self.state, self.n = -1, n
            lay = plan(ref, n)
            if lay["state"] == 1:
                self.state, self.layout = 1, lay
        return BLOCKED if blocked else HASHED

    def block_layout(self):
        """What TwoDmap.block_layout() must report: the whole layout behind a "yes", else the state alone (the rest is stale)."""
        return dict(self.layout) if self.state == 1 else {"state": self.state}


def shifted(cloud, blocks, lay, grid_len):
    """The cloud moved by `blocks` blocks of the layout along x (the origin row stays)."""
    out = cloud.copy()
    out[1:, 0] += np.float32(blocks * (1 << lay["shx"]) * grid_len)
    return out


LIFETIME_SCENE = "levels_4_at_interval"
LIFETIME_NEW_ORIGIN = (1.3, -0.7, 0.0)      # 2.6 and 1.4 cells: other keys for the same points, the same levels


@functools.lru_cache(maxsize=1)
def lifetime_script():
    """The layout's lifetime on one handle, as builds in order: (what, cloud with its origin row, set_origin first?, expected strategy,
    expected re-runs caused by the layout, expected state afterwards, a cloud the handle has already sized its buffers for?).
    A: the small LIFETIME_SCENE; S: A moved three blocks along x (out of A's box and its block of margin); S15: S's box with 1.5 x the
    points (outside A's size window); then S15 under another origin."""
    s = SMALL_SCENES[LIFETIME_SCENE]
    lay = s["layout"]
    a = small_cloud(LIFETIME_SCENE)
    sh = shifted(a, 3, lay, s["grid_len"])
    dx = 3 * (1 << lay["shx"]) * s["grid_len"]
    lo, hi = (s["lo"][0] + dx,) + tuple(s["lo"][1:]), (s["hi"][0] + dx,) + tuple(s["hi"][1:])
    n15 = SMALL_POINTS + SMALL_POINTS // 2
    s15 = np.concatenate([np.float32([s["origin"]]), box(SEED + 2, lo, hi, n15)], 0)
    moved = s15.copy()
    moved[0] = np.float32(LIFETIME_NEW_ORIGIN)
    for c in (sh, s15, moved):
        c.setflags(write=False)
    return (
        ("1: A", a, False, HASHED, 0, 1, False),
        ("1: A again", a, False, BLOCKED, 0, 1, True),
        ("2: A shifted by three blocks", sh, False, HASHED, 1, -1, True),
        ("3: the shifted cloud again", sh, False, HASHED, 0, -1, True),
        ("4: the shifted box with 1.5 x the points", s15, False, HASHED, 0, 1, False),
        ("5: the same cloud again", s15, False, BLOCKED, 0, 1, True),
        ("7: after another origin", moved, True, HASHED, 0, 1, False),
        ("7: again", moved, False, BLOCKED, 0, 1, True),
    )


@contextlib.contextmanager
def blocked_floor(points=SMALL_FLOOR):
    """gndt_debug_set_option(GNDT_DEBUG_BLOCKED_MIN_POINTS, .) for a block; the default comes back whatever happens in it"""
    import grid_ndt_amd as g
    g.TwoDmap.set_debug_option(g.TwoDmap.DEBUG_BLOCKED_MIN_POINTS, points)
    try:
        yield
    finally:
        g.TwoDmap.set_debug_option(g.TwoDmap.DEBUG_BLOCKED_MIN_POINTS, 1 << 20)


def labels_of_perfect_build(ref, interval, demand, min_points):
    """The flags a build without any error of its own gives: OcNode::isSlope (map2D.h:66-108) on the fp64 centroids rounded to float32.
    The oracle decides on its sequential fp32 centroids, which lie an ulp or two off: where |dz| of two adjacent levels falls that
    close to the interval the two labels differ, through no fault of the build, and parity.compare's strict gates (labels exact) cannot
    be met.  A fixture must have no such node: -> the flags, to be compared with ref["flags"]."""
    cz = contiguous(ref["sz"])
    key = ((ref["sx"].astype(np.int64) + (1 << 17)) << 42) | ((ref["sy"].astype(np.int64) + (1 << 17)) << 23) | (cz + (1 << 22))
    order = np.argsort(key)
    skey = key[order]
    cnt = ref["count"].astype(np.int64)
    has = cnt >= min_points
    first = ref["first_idx"].astype(np.int64)
    z = np.where(has, ref["mean64"][:, 2], 0.0).astype(np.float32)
    far = {}
    for step in (1, -1):
        pos = np.clip(np.searchsorted(skey, key + step), 0, key.size - 1)
        there = skey[pos] == key + step
        o = order[pos]
        zo = np.where(there & (first[o] < first), z[o], np.float32(0.0)).astype(np.float32)
        far[step] = there & (np.abs(zo - z) > np.float32(interval))
    flags = np.zeros(key.size, np.int64)
    if demand == "slope":
        slope = has & ~far[1]
        flags[has] |= 1
        flags[slope] |= 2
        flags[slope & far[-1]] |= 4
    else:
        flags[has] |= 3
    return flags
