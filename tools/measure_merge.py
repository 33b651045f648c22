#!/usr/bin/env python3
"""Map merge (gndt_merge_map_device) on the bench map: one process, one GPU.

  S2 table   the bench workload's map (10 M uniform-random points, 0.5 m cubic cells) built once by strategy ATOMIC, then
               merge_empty   its node table merged under the identity into an empty handle of the same geometry (every node inserts)
               merge_copy    the same merge into a copy of the map (no node inserts: every add meets a populated node)
               merge_pose    into an empty handle under yaw 17 degrees, pitch 4 degrees and an off-lattice translation
               coarsen_1_1   gndt_coarsen_device(1, 1) of the same map: it reads the same nodes and issues the same atomics
Every figure is the median of `--reps` calls between two HIP events on the stream, and of the host's clock around the call; a call
includes its host side (the gndt_sync of both handles, the wait for the kernel) and the destination's full re-finalisation, which the
three share.  The destination handles are made and sized before the timed calls (the first round is a warm-up and is dropped) and
reset between them.  Kernel times (k_merge_map against k_coarsen): run it under `rocprofv3 --kernel-trace --stats` in a run of its own.
Prints one JSON line.

    python3 tools/measure_merge.py [--reps 7] [--points 10000000]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--points", type=int, default=10_000_000)
    a = ap.parse_args()
    import torch
    import grid_ndt_amd as g
    from grid_ndt_amd import scenes
    assert torch.cuda.is_available(), "measure_merge.py needs the GPU"
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
    origin = cloud[0]

    def handle():
        m = g.TwoDmap(P["grid_len"], P["z_len"], strategy=1)
        m.setInterval(P["slope_interval"])
        m.setCloudFirst(origin)
        return m

    src = handle()
    src.create2DMap("slope", torch.from_numpy(np.ascontiguousarray(cloud[1:])).cuda())
    nodes = src.sync()[0]
    y, p = math.radians(17.0), math.radians(4.0)
    Rz = np.array([[math.cos(y), -math.sin(y), 0], [math.sin(y), math.cos(y), 0], [0, 0, 1]])
    Ry = np.array([[math.cos(p), 0, math.sin(p)], [0, 1, 0], [-math.sin(p), 0, math.cos(p)]])
    pose = np.concatenate([Rz @ Ry, [[0.731], [-0.419], [0.057]]], 1)
    empty, posed, copy, coarse = handle(), handle(), handle(), handle()
    res = {k: [] for k in ("merge_empty", "merge_copy", "merge_pose", "coarsen_1_1")}
    host = {k: [] for k in res}
    stats = {}
    for r in range(a.reps + 1):
        src.coarsen(1, 1, into=copy)                   # (untimed: the copy the second merge goes into)
        for m in (empty, posed):
            m.reset("slope")
        runs = (("merge_empty", lambda: empty.merge_from(src)), ("coarsen_1_1", lambda: src.coarsen(1, 1, into=coarse)),
                ("merge_copy", lambda: copy.merge_from(src)), ("merge_pose", lambda: posed.merge_from(src, pose=pose)))
        for key, fn in runs[r % 2::1] + runs[:r % 2]:  # (the order alternates between the rounds)
            d, h, st = timed(fn)
            if r:
                res[key].append(d)
                host[key].append(h)
            if isinstance(st, dict):
                stats[key] = st
    assert empty.sync()[0] == nodes and copy.sync()[0] == nodes and coarse.sync()[0] == nodes
    out = {"tool": "measure_merge", "source_hash": g._lib.source_hash()[:16], "reps": a.reps, "points": a.points, "nodes": nodes,
           "posed_nodes": posed.sync()[0], "stats": stats,
           **{k + "_ms": float(np.median(v)) for k, v in res.items()}, **{k + "_call_ms": float(np.median(v)) for k, v in host.items()},
           "merge_empty_over_coarsen": float(np.median(res["merge_empty"]) / np.median(res["coarsen_1_1"])), "samples": res}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
