#!/usr/bin/env python3
"""Raster export (gndt_raster_device) on MI355X: one process, one GPU.

Workloads (DESIGN.md "Raster export"):
  s2_full        bench.py's S2 map (10 M uniform points in [-100,100)^2 x [-1,1), 0.5 m cells): its full 400 x 400 box, the four map
                 layers (row, z, rough, nodes), each mode; with the column index current, and freshly rebuilt (a build, gndt_sync, then
                 the timed raster, which rebuilds the index)
  s2_export_host gndt_export_host of the same map, in the same process: the "export every row" alternative
  s4_window      the streaming map (100 LiDAR frames of 131 072 points added with gndt_update_device, ~1.75 M rows): a 256 x 256 window
                 around the last pose
  bridge_full    bridge_ground's full box
  query          tools/measure_query.py's NEAREST_SLOPE set (10 M uniform random points over S2) at ILP 1: the factored column walk
Every figure is the median of `--reps` calls, each between two HIP events on the stream (the call's host side included).  Kernel times:
run it under `rocprofv3 --kernel-trace --stats` in a run of its own.  Prints one JSON line.

    python3 tools/measure_raster.py [--reps 20] [--frames 100]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--frames", type=int, default=100)
    a = ap.parse_args()
    import torch
    import grid_ndt_amd as g
    from grid_ndt_amd import scenes
    from grid_ndt_amd._lib import Cells, CropBox, RasterLayers
    from grid_ndt_amd.map2d import _stream_ptr
    assert torch.cuda.is_available(), "measure_raster.py needs the GPU"
    stream = torch.cuda.current_stream()
    sp = _stream_ptr(None)

    def timed(fn, reps, warmup, pre=None):
        for _ in range(warmup):
            pre and pre()
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            pre and pre()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return round(float(np.median(ts)), 4), [round(t, 4) for t in ts]

    def raster_fn(m, box, mode, z_ref, layers):
        w, h = g.raster_shape(box)
        bufs = {k: torch.empty(w * h, dtype=torch.float32 if k in ("z", "rough", "h") else torch.int32, device="cuda") for k in layers}
        L = RasterLayers(*[bufs[k].data_ptr() if k in bufs else 0 for k in ("row", "z", "rough", "nodes", "h", "state")])
        b = CropBox(*box)

        def f():
            rc = m._L.gndt_raster_device(m._h, C.byref(b), mode, z_ref, C.byref(L), sp)
            assert rc == 0, m._L.gndt_last_error(m._h)
        return f, w * h

    def box_of(m):
        c = m.export_device()
        return (int(c["sx"].min()), int(c["sx"].max()), int(c["sy"].min()), int(c["sy"].max()))

    LAYERS = ("row", "z", "rough", "nodes")
    out = {"tool": "measure_raster", "device": g.device_info(0).get("name"), "source_hash": g._lib.source_hash()[:16], "reps": a.reps}

    # ---- S2 ----
    cloud = scenes.uniform_box(a.points + 1)
    P = dict(grid_len=0.5, z_len=0.5, slope_interval=0.08)
    m = g.TwoDmap(P["grid_len"], P["z_len"], max_nodes_hint=1 << 20)
    m.setInterval(P["slope_interval"])
    m.setCloudFirst(cloud[0])
    pts = torch.from_numpy(cloud[1:]).cuda()
    m.create2DMap("slope", pts)
    rows, cols, _ = m.sync()
    box = box_of(m)
    s2 = {"rows": rows, "columns": cols, "box": box}
    for name, mode in (("lowest", 0), ("highest", 1), ("nearest_z", 2)):
        f, npx = raster_fn(m, box, mode, 0.0, LAYERS)
        s2[name + "_ms"], s2[name + "_samples_ms"] = timed(f, a.reps, a.warmup)
    s2["pixels"] = npx
    f, _ = raster_fn(m, box, 0, 0.0, ("row",))
    s2["lowest_row_only_ms"], _ = timed(f, a.reps, a.warmup)
    # a fresh index: every raster follows a build (and the gndt_sync that waits for it)
    f, _ = raster_fn(m, box, 0, 0.0, LAYERS)
    s2["lowest_index_rebuilt_ms"], s2["lowest_index_rebuilt_samples_ms"] = timed(f, max(5, a.reps // 2), 1,
                                                                                  pre=lambda: (m.create2DMap("slope", pts), m.sync()))
    c = Cells()

    def export_host():
        rc = m._L.gndt_export_host(m._h, C.byref(c))
        assert rc == 0, m._L.gndt_last_error(m._h)
    s2["export_host_ms"], s2["export_host_samples_ms"] = timed(export_host, max(5, a.reps // 2), 1)
    s2["export_host_bytes"] = rows * 76
    out["s2"] = s2

    # ---- the NEAREST_SLOPE query set of tools/measure_query.py (ILP 1) on the same map ----
    n = a.points
    rng = np.random.default_rng(0x5EED00AA)
    rng.permutation(n)                                   # (measure_query.py draws its shuffle first: the same random points)
    rnd = np.empty((n, 3), np.float32)
    rnd[:, :2] = rng.uniform(-100, 100, size=(n, 2))
    rnd[:, 2] = rng.uniform(-1, 1, size=n)
    uniform = torch.from_numpy(rnd).cuda()
    qrows = torch.empty(n, dtype=torch.int32, device="cuda")

    def query():
        rc = m._L.gndt_query_device(m._h, C.c_void_p(uniform.data_ptr()), n, 12, 1, C.c_void_p(qrows.data_ptr()), None, None, sp)
        assert rc == 0, m._L.gndt_last_error(m._h)
    g.TwoDmap.set_debug_option(g.TwoDmap.DEBUG_QUERY_ILP, 1)
    q_ms, q_samples = timed(query, a.reps, a.warmup)
    out["query_nearest_slope_uniform_ilp1"] = {"queries": n, "ms": q_ms, "samples_ms": q_samples, "Mqueries_per_s": round(n / q_ms / 1e3, 1)}
    del m, pts, uniform, qrows

    # ---- S4: a 256 x 256 window of the streaming map ----
    ppf = scenes.FRAME_POINTS
    frames = scenes.terrain_frames(a.frames + 1)
    origin, body = frames[0], frames[1:1 + a.frames * ppf]
    tb = torch.from_numpy(np.ascontiguousarray(body)).cuda()
    TP = scenes.TERRAIN_PARAMS
    ms = g.TwoDmap(TP["grid_len"], TP["z_len"], strategy=1, max_nodes_hint=2_500_000, max_points_hint=len(body) + 1)
    ms.setInterval(TP["slope_interval"])
    ms.setCloudFirst(origin)
    for fr in range(a.frames):
        ms.change2DMap("slope", tb[fr * ppf:(fr + 1) * ppf])
    s4_rows, s4_cols, _ = ms.sync()
    last = body[-ppf:, :2].mean(0)
    wbox = g.crop_box_from_world(origin, TP["grid_len"], last - 25.6 + 0.5 * TP["grid_len"], last + 25.6 - 0.5 * TP["grid_len"])
    s4 = {"rows": s4_rows, "columns": s4_cols, "frames": a.frames, "box": wbox, "shape": g.raster_shape(wbox)}
    for name, mode, z in (("lowest", 0, 0.0), ("nearest_z", 2, float(body[-ppf:, 2].mean()))):
        f, _ = raster_fn(ms, wbox, mode, z, LAYERS)
        s4[name + "_ms"], s4[name + "_samples_ms"] = timed(f, a.reps, a.warmup)
    out["s4_window"] = s4
    del ms, tb

    # ---- bridge_ground ----
    bc = scenes.bridge_ground()
    BP = scenes.BRIDGE_PARAMS
    mb = g.TwoDmap(BP["grid_len"], BP["z_len"])
    mb.setInterval(BP["slope_interval"])
    mb.setCloudFirst(bc[0])
    mb.create2DMap("slope", torch.from_numpy(bc[1:]).cuda())
    b_rows, b_cols, _ = mb.sync()
    bbox = box_of(mb)
    br = {"rows": b_rows, "columns": b_cols, "box": bbox, "shape": g.raster_shape(bbox)}
    for name, mode in (("lowest", 0), ("highest", 1)):
        f, _ = raster_fn(mb, bbox, mode, 0.0, LAYERS)
        br[name + "_ms"], br[name + "_samples_ms"] = timed(f, a.reps, a.warmup)
    out["bridge_full"] = br
    out["what"] = ("median of HIP-event intervals around single gndt_raster_device / gndt_export_host / gndt_query_device calls (host side "
                   "of the call included); kernel times come from a separate rocprofv3 --kernel-trace --stats run")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
