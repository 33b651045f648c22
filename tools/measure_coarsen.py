#!/usr/bin/env python3
"""Map coarsening (gndt_coarsen_device) against what a user without it has to do: one process, one GPU.

  The bench map: uniform_box(10 000 001) at 0.5 m cells and levels, strategy ATOMIC (796 015 nodes).
    coarsen   TwoDmap.coarsen(2, 2) into an existing handle at 1.0 m: reset, k_coarsen over the fine node table, full finalisation,
              and the call's own waits (it returns after the kernel; the finalisation is awaited by the timing event)
    rebuild   a fresh ATOMIC build of the same 10 M device-resident points on a handle at 1.0 m (create2DMap + sync)
  Every figure is the median of `--reps` calls, in milliseconds between two HIP events on the stream and as host wall time around the
  call and its sync; the first call of each kind (allocations) is left out.  Kernel times: run it under `rocprofv3 --kernel-trace
  --stats` in a run of its own.  Prints one JSON line.

    python3 tools/measure_coarsen.py [--reps 5] [--points 10000000]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--points", type=int, default=10_000_000)
    a = ap.parse_args()
    import torch
    import grid_ndt_amd as g
    from grid_ndt_amd import scenes
    assert torch.cuda.is_available(), "measure_coarsen.py needs the GPU"
    stream = torch.cuda.current_stream()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        stream.synchronize()
        t0 = time.perf_counter()
        e0.record(stream)
        r = fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3, r

    P = dict(grid_len=0.5, z_len=0.5, slope_interval=0.08)
    cloud = scenes.uniform_box(a.points + 1)
    body = torch.from_numpy(np.ascontiguousarray(cloud[1:])).cuda()

    def handle(scale):
        m = g.TwoDmap(scale * P["grid_len"], scale * P["z_len"], strategy=1, max_nodes_hint=1 << 20)
        m.setInterval(P["slope_interval"])
        m.setCloudFirst(cloud[0])
        return m

    fine = handle(1)
    fine.create2DMap("slope", body)
    n_fine = fine.sync()
    into, again = handle(2), handle(2)
    res = {k: [] for k in ("coarsen", "coarsen_call", "rebuild", "rebuild_call")}
    for r in range(a.reps + 1):
        d, h, _ = timed(lambda: (fine.coarsen(2, 2, into=into), into.sync()))
        if r:
            res["coarsen"].append(d); res["coarsen_call"].append(h)
        d, h, _ = timed(lambda: (again.create2DMap("slope", body), again.sync()))
        if r:
            res["rebuild"].append(d); res["rebuild_call"].append(h)
    n_coarse, n_again = into.sync(), again.sync()
    assert n_coarse == n_again, (n_coarse, n_again)
    out = {"tool": "measure_coarsen", "source_hash": g._lib.source_hash()[:16], "reps": a.reps, "points": a.points,
           "fine_nodes": n_fine[0], "coarse_nodes": n_coarse[0], **{k + "_ms": float(np.median(v)) for k, v in res.items()},
           "samples": res}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
