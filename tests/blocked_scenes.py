"""Scenes for BLOCKED buckets (gndt_blocked.hpp) and a numpy restatement of the rule that lays the blocks out (blocked_decide,
gndt_api_build.hip): one dense, evenly filled box per block shape of k_bucket_blocked — 512, 256, 128, 64, 32 and 16 columns per block
(shz = 0 .. 5) — among them boxes that do not straddle the origin, a moved origin, a box that leaves level padding in its blocks and a
scene whose adjacent-level means lie about one slope interval apart.  Shared by tests/test_blocked_scenes_host.py (the fixtures hold
on the CPU oracle) and tests/test_gpu_blocked_shapes.py (the device takes exactly these layouts and gives the oracle's maps)."""
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
