#!/usr/bin/env python3
"""S2 with a DIFFERENT cloud every build:  python3 tools/cycle_clouds.py [--clouds 3] [--steps 21] [--points 10000000]

bench.py rebuilds the map from the same device cloud every step, so part of that cloud (120 MB of a 256 MiB last-level cache) could
still be cached when the next step's level 1 reads it — a gain that real use, where every build gets a new cloud, would not see.  This
builds `--clouds` different uniform clouds of the bench scene's box in turn on one handle (same origin, so the handle keeps its blocked
layout) and prints one JSON line: ms per step cycling over the clouds, and over the first cloud alone, timed the way bench.py times
(back-to-back launches, one wait at the end).  A/B two builds of the library with it as with bench.py (profiles/r08_ablation.txt 5)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--points", type=int, default=10_000_000)
    a = ap.parse_args()
    import torch
    import grid_ndt_amd as g
    from grid_ndt_amd import scenes
    g.build_native()
    clouds = [scenes.uniform_box(a.points + 1, seed=0x5EED0002 + 977 * k) for k in range(a.clouds)]
    origin = clouds[0][0].copy()
    dev = [torch.from_numpy(c[1:]).cuda() for c in clouds]
    del clouds
    m = g.TwoDmap(0.5, 0.5, max_nodes_hint=1 << 20)
    m.setInterval(0.08)
    m.setCloudFirst(origin)
    stream = torch.cuda.current_stream()

    def timed(pick):
        for k in range(a.warmup):
            m.create2DMap("slope", pick(k), stream)
        m.sync()
        torch.cuda.synchronize()
        r0 = m.retry_count()
        t0 = time.perf_counter()
        for k in range(a.steps):
            m.create2DMap("slope", pick(k), stream)
        nodes = m.sync()[0]
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.steps * 1e3, int(nodes), int(m.retry_count() - r0)

    one = timed(lambda k: dev[0])
    cyc = timed(lambda k: dev[k % a.clouds])
    one2 = timed(lambda k: dev[0])
    print(json.dumps({"points": a.points, "clouds": a.clouds, "steps": a.steps, "strategy": m.STRATEGY_NAMES.get(m.last_strategy(), "?"),
                      "ms_per_step_one_cloud": [round(one[0], 4), round(one2[0], 4)], "ms_per_step_cycling": round(cyc[0], 4),
                      "nodes_last": cyc[1], "retries_in_timed_regions": one[2] + cyc[2] + one2[2]}))


if __name__ == "__main__":
    main()
