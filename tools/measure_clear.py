#!/usr/bin/env python3
"""Free-space clearing (gndt_clear_rays_device) on the streaming map: one process, one GPU.

  S4 table   `--frames` LiDAR frames of 131 072 points added with gndt_update_device (60 frames: about 1 M nodes), then the next frame's
             131 072 rays from its pose (1.8 m over the ground):
               count_only      GNDT_CLEAR_COUNT_ONLY with per-row passes, extent skip on (GNDT_DEBUG_CLEAR_EXTENT = 1)
               count_only_plain  the same with the plain column-index walk (the default): the A/B of the extent skip
               clear           a clear with min_passes = 1, default walk (walk, kill, compaction of the node table, full re-finalisation)
Every figure is the median of `--reps` calls between two HIP events on the stream; a clear's figure includes its host side (the
gndt_sync it starts with, its wait for the device).  The map is rebuilt before every clear.  Kernel times: run it under
`rocprofv3 --kernel-trace --stats` in a run of its own.  Prints one JSON line.

    python3 tools/measure_clear.py [--reps 5] [--frames 60]
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
    ap.add_argument("--frames", type=int, default=60)
    a = ap.parse_args()
    import torch
    import grid_ndt_amd as g
    from grid_ndt_amd import scenes
    assert torch.cuda.is_available(), "measure_clear.py needs the GPU"
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

    ppf = scenes.FRAME_POINTS
    P = scenes.TERRAIN_PARAMS
    frames = scenes.terrain_frames(a.frames + 2)
    origin, body = frames[0], frames[1:1 + a.frames * ppf]
    tb = torch.from_numpy(np.ascontiguousarray(body)).cuda()
    nxt = torch.from_numpy(np.ascontiguousarray(frames[1 + a.frames * ppf:1 + (a.frames + 1) * ppf])).cuda()
    px, py = scenes._pose_xy(np.int64(a.frames), 200.0, 14.0)
    sensor = (float(px), float(py), float(scenes.heightfield(np.array([px]), np.array([py]), 0x5EED0003)[0]) + 1.8)

    def fresh():
        mm = g.TwoDmap(P["grid_len"], P["z_len"], strategy=1, max_nodes_hint=2_000_000, max_points_hint=len(body) + ppf + 1)
        mm.setInterval(P["slope_interval"])
        mm.setCloudFirst(origin)
        for f in range(a.frames):
            mm.change2DMap("slope", tb[f * ppf:(f + 1) * ppf])
        mm.sync()
        return mm

    out = {"tool": "measure_clear", "source_hash": g._lib.source_hash()[:16], "reps": a.reps, "frames": a.frames, "rays": ppf}
    res = {k: [] for k in ("count_only", "count_only_plain", "clear", "clear_call")}
    for r in range(a.reps + 1):
        m = fresh()
        n0 = m.sync()
        for ext, key in ((1, "count_only"), (0, "count_only_plain")):
            g.TwoDmap.set_debug_option(5, ext)
            d, _, st = timed(lambda: m.clear_rays(sensor, nxt, count_only=True, passes=True))
            if r:
                res[key].append(d)
        d, h, st_clear = timed(lambda: m.clear_rays(sensor, nxt))
        n1 = m.sync()
        if r:
            res["clear"].append(d); res["clear_call"].append(h)
        del m
    out["s4"] = {"nodes_before": n0[0], "nodes_after": n1[0], "count_only_stats": st[0], "clear_stats": st_clear,
                 **{k + "_ms": float(np.median(v)) for k, v in res.items()}, "samples": res}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
