#!/usr/bin/env python3
"""Region crop (gndt_crop_device) on the bench's maps: one process, one GPU.

  S2 rows only   bench.py's default workload (10 M uniform points in [-100,100)^2 x [-1,1), 0.5 m cells, PARTITION / AUTO build):
                 KEEP_INSIDE of the columns with sx < 0, about half the rows
  S4 table       the streaming map (100 LiDAR frames of 131 072 points added with gndt_update_device, ~1.75 M nodes): KEEP_INSIDE of
                 the columns with sx < 0, next to a full re-finalisation of the whole table (gndt_finalize_device) and a gndt_remove of
                 the points of the same columns
Every figure is the median of `--reps` calls, each between two HIP events on the stream after a fresh map (a crop changes the map), so
a crop's figure includes its host side (the gndt_sync it starts with, the launches).  Kernel times: run it under
`rocprofv3 --kernel-trace --stats` in a run of its own.  Prints one JSON line.

    python3 tools/measure_crop.py [--reps 5] [--frames 100]
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
    ap.add_argument("--frames", type=int, default=100)
    a = ap.parse_args()
    import torch
    import grid_ndt_amd as g
    from grid_ndt_amd import scenes
    assert torch.cuda.is_available(), "measure_crop.py needs the GPU"
    stream = torch.cuda.current_stream()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        stream.synchronize()
        t0 = time.perf_counter()
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3

    out = {"tool": "measure_crop", "source_hash": g._lib.source_hash()[:16], "reps": a.reps}
    # ---- S2: rows only ----
    cloud = scenes.uniform_box(a.points + 1)
    P = dict(grid_len=0.5, z_len=0.5, slope_interval=0.08)
    t = torch.from_numpy(cloud[1:]).cuda()
    m = g.TwoDmap(P["grid_len"], P["z_len"], max_nodes_hint=1 << 20)
    m.setInterval(P["slope_interval"])
    m.setCloudFirst(cloud[0])
    dev_ms, host_ms, build_ms = [], [], []
    for r in range(a.reps + 1):
        bd, _ = timed(lambda: m.create2DMap("slope", t))
        n0 = m.sync()
        cells = m.export() if r == 0 else None
        if r == 0:
            box = (int(cells["sx"].min()), -1, int(cells["sy"].min()), int(cells["sy"].max()))
        d, h = timed(lambda: m.crop_box(box, "keep_inside"))
        n1 = m.sync()
        if r:
            dev_ms.append(d); host_ms.append(h); build_ms.append(bd)
    out["s2"] = {"rows_before": n0[0], "rows_after": n1[0], "kept": n1[0] / n0[0], "crop_ms": float(np.median(dev_ms)),
                 "crop_call_ms": float(np.median(host_ms)), "build_ms": float(np.median(build_ms)), "strategy": m.STRATEGY_NAMES[m.last_strategy()]}
    del m, t
    # ---- S4: table-backed streaming map ----
    ppf = scenes.FRAME_POINTS
    frames = scenes.terrain_frames(a.frames + 1)
    origin, body = frames[0], frames[1:1 + a.frames * ppf]
    tb = torch.from_numpy(np.ascontiguousarray(body)).cuda()
    P = scenes.TERRAIN_PARAMS
    from tests import query_ref as qr
    sx, _, _, _, _ = qr.keys(body, origin, P["grid_len"], P["z_len"])
    drop_pts = tb[torch.from_numpy(sx >= 1).cuda()]

    def fresh():
        mm = g.TwoDmap(P["grid_len"], P["z_len"], strategy=1, max_nodes_hint=2_500_000, max_points_hint=len(body) + 1)
        mm.setInterval(P["slope_interval"])
        mm.setCloudFirst(origin)
        for f in range(a.frames):
            mm.change2DMap("slope", tb[f * ppf:(f + 1) * ppf])
        mm.sync()
        return mm

    res = {"crop": [], "crop_call": [], "finalize": [], "finalize_call": [], "remove": [], "remove_call": []}
    for r in range(a.reps + 1):
        mm = fresh()
        n0 = mm.sync()
        d2, h2 = timed(lambda: mm.finalize())
        assert mm.sync() == n0
        d, h = timed(lambda: mm.crop_box((-65535, -1, -65535, 65535), "keep_inside"))
        n1 = mm.sync()
        mm = fresh()
        d3, h3 = timed(lambda: mm.del2DMap("slope", drop_pts))
        assert mm.sync() == n1
        if r:
            for k, v in (("crop", d), ("crop_call", h), ("finalize", d2), ("finalize_call", h2), ("remove", d3), ("remove_call", h3)):
                res[k].append(v)
        del mm
    out["s4"] = {"nodes_before": n0[0], "nodes_after": n1[0], **{k + "_ms": float(np.median(v)) for k, v in res.items()}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
