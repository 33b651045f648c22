#!/usr/bin/env python3
"""A fixed, seeded script of PARTITION builds: the smallest shapes that take each launch variant of gndt_api_build.hip and of the owner
split (level 1 by stride, fan-out and input kind; the bucket pass by table size, statistics, second pass, blocked; both ordering tails).
After every build one line: last_strategy, retry_count, second_pass_buckets and the node / column / slope totals.

Two trees compute the same if these lines are equal and, run as
    rocprofv3 --kernel-trace --output-format csv -d <dir> -- python3 tools/launch_census.py
(alone: no counters, no other tracing), the traces hold the same sequence of (kernel name, grid, workgroup, dynamic LDS)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

P = dict(grid_len=0.5, z_len=0.1, slope_interval=0.08)


def main():
    import torch
    import grid_ndt_amd as g
    from grid_ndt_amd import scenes
    from tests import blocked_scenes as bs

    def handle(cloud, strategy, p=P):
        m = g.TwoDmap(p["grid_len"], p["z_len"], strategy=strategy)
        m.setInterval(p["slope_interval"])
        m.setCloudFirst(cloud[0, :3])
        return m

    def dev(cloud, stride=12):
        body = scenes.with_stride4(cloud)[1:] if stride == 16 else np.array(cloud[1:, :3], dtype=np.float32)      # (a copy: shared clouds are read-only)
        return torch.from_numpy(np.ascontiguousarray(body)).cuda()

    def report(label, m, totals=None):
        try:
            n, k, s = totals if totals is not None else m.sync()
        except g.GndtError as e:          # (a replay that does not fit is reported, and is a line like any other)
            n = k = s = f"error {e.code}"
        print(f"{label}: strategy {m.last_strategy()} retries {m.retry_count()} second_pass {m.second_pass_buckets()} "
              f"nodes {n} columns {k} slopes {s}", flush=True)

    def build(label, m, pts):
        m.create2DMap("slope", pts)
        report(label, m)

    def uniform(n, **kw):
        return scenes.uniform_box(n + 1, **kw)

    # exact partition; one-level partition with fan-outs 256 and 512; two-level partition -- points of 12 and 16 bytes
    # (boxes of four levels with about four points per node, near the n / 4 nodes a first build guesses: at most the staging rows are
    #  re-run for, and every build ends on the partition it started on)
    for label, strategy, cloud in (("exact 20000", 3, uniform(20_000, seed=0xCE0501, half_xy=8.0, half_z=0.2)),
                                   ("one-level fan 256, 100000", 2, uniform(100_000, seed=0xCE0502, half_xy=20.0, half_z=0.2)),
                                   ("one-level fan 512, 262144", 2, uniform(262_144, seed=0xCE0503, half_xy=30.0, half_z=0.2)),
                                   ("two-level 131072", 4, uniform(131_072, seed=0xCE0504, half_xy=20.0, half_z=0.2))):
        for stride in (12, 16):
            build(f"{label} stride {stride}", handle(cloud, strategy), dev(cloud, stride))

    # a node-heavy cloud (next to one point per node): the second build knows the node count and starts on 1024-slot tables
    cloud = uniform(400_000, seed=0xCE0505, half_xy=2000.0, half_z=2.0)
    m, pts = handle(cloud, 2), dev(cloud)
    build("node-heavy 400000, first", m, pts)
    build("node-heavy 400000, second", m, pts)

    # the second pass (tests/test_gpu_parity.py: the cloud whose 512-slot tables overflow), behind a cloud of the same size that fills
    # no table -- so that the first of the three builds finds the pass off, misses it, and the next two carry it
    cloud = scenes.uniform_box(3_000_001, seed=0x5EED0301, half_xy=50.0, half_z=1.0)
    flat = scenes.uniform_box(3_000_001, seed=0xCE0506, half_xy=50.0, half_z=0.04)
    flat[0] = cloud[0]
    m = handle(cloud, 2)
    build("second pass: flat cloud in front", m, dev(flat))
    pts = dev(cloud)
    for k in ("off", "on", "on again"):
        build(f"second pass {k}", m, pts)

    # blocked buckets on a small box: both ordering tails, the two-kernel one by the column table and by the staged nodes
    name = "levels_4_at_interval"
    cloud, bp = bs.small_cloud(name), bs.small_params(name)
    pts = dev(cloud)
    g.TwoDmap.set_debug_option(g.TwoDmap.DEBUG_BLOCKED_MIN_POINTS, bs.SMALL_FLOOR)
    for words in (16_384, 0):
        for column_dest in (1, 0):
            g.TwoDmap.set_debug_option(g.TwoDmap.DEBUG_PLACE_EMIT_WORDS, words)
            g.TwoDmap.set_debug_option(g.TwoDmap.DEBUG_COLUMN_DEST, column_dest)
            m = handle(cloud, bs.TWO_LEVEL, bp)
            build(f"blocked {name} place_emit_words {words} column_dest {column_dest}: hashed build in front", m, pts)
            build(f"blocked {name} place_emit_words {words} column_dest {column_dest}", m, pts)
    g.TwoDmap.set_debug_option(g.TwoDmap.DEBUG_PLACE_EMIT_WORDS, 16_384)
    g.TwoDmap.set_debug_option(g.TwoDmap.DEBUG_COLUMN_DEST, 1)
    g.TwoDmap.set_debug_option(g.TwoDmap.DEBUG_BLOCKED_MIN_POINTS, 1 << 20)

    # records (what an owner split of one rank hands back), in one segment and in two
    cloud = uniform(100_000, seed=0xCE0507, half_xy=20.0, half_z=0.2)
    pts, n = dev(cloud), 100_000
    recs = handle(cloud, 2).owner_split("slope", pts, 0, n, 1)[0].clone()
    for strategy in (2, 4):
        m = handle(cloud, strategy)
        m.build_records("slope", recs, n)
        report(f"records {recs.shape[0]} strategy {strategy}", m)
        a = int(recs.shape[0]) // 3
        first, room_and_second = recs[:a].clone(), recs.clone()
        room_and_second[:a] = float("nan")
        m = handle(cloud, strategy)
        m.build_records2("slope", first, room_and_second, n)
        report(f"records {a} + {recs.shape[0] - a} strategy {strategy}", m)

    # statistics only
    m = handle(cloud, 0)
    st = m.shard_stats("slope", pts)
    report("shard_stats 100000", m, (int(st["key"].shape[0]), 0, 0))

    # the owner split of two ranks: in one pass (shards of 65 536 points) and by the counting passes (shards of 20 000)
    for n, stride in ((131_072, 12), (131_072, 16), (40_000, 12)):
        cloud = uniform(n, seed=0xCE0508, half_xy=20.0, half_z=0.2)
        pts = dev(cloud, stride)
        for r in range(2):
            m = handle(cloud, 0)
            runs = m.owner_split("slope", pts[r * n // 2:(r + 1) * n // 2], r * n // 2, n, 2)
            print(f"owner split of {n} stride {stride}, rank {r}: runs {[int(x.shape[0]) for x in runs]}", flush=True)

    # a build recorded into a hipGraph after an eager build of the same cloud, replayed twice
    cloud = uniform(100_000, seed=0xCE0509, half_xy=20.0, half_z=0.2)
    other = uniform(100_000, seed=0xCE050A, half_xy=20.0, half_z=0.2)
    other[0] = cloud[0]
    m, buf = handle(cloud, 2), dev(cloud)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        m.create2DMap("slope", buf, s)
        report("captured: eager build in front", m)
        graph = torch.cuda.CUDAGraph()
        with g.graph_capture(graph, s):
            m.create2DMap("slope", buf, s)
        for k, src in enumerate((other, cloud)):
            buf.copy_(dev(src))
            graph.replay()
            s.synchronize()
            report(f"captured: replay {k}", m)


if __name__ == "__main__":
    main()
