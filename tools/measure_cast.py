#!/usr/bin/env python3
"""Ray casting (gndt_cast_rays_device) on the streaming map, next to the count-only clearing walk of the same rays: one process, one GPU.

  S4 table   `--frames` LiDAR frames of 131 072 points added with gndt_update_device (60 frames: about 1 M nodes), then the next frame's
             131 072 rays from its pose (1.8 m over the ground), tools/measure_clear.py's map and rays:
               cast_voxel      GNDT_CAST_VOXEL to the scan's own end points, all three outputs
               cast_ndt        GNDT_CAST_NDT, the same rays
               count_only      gndt_clear_rays_device, GNDT_CLEAR_COUNT_ONLY with per-row passes, the plain column-index walk: the yardstick
             and the same three with every end point pushed to 1.5 x its range (`_x15`), so that rays that miss run their full length.
Every figure is the median of `--reps` calls between two HIP events on the stream (one more call first, not counted); none of the
calls asks for its stats inside the timed region.  The share of rays that hit comes from one more call with stats.  Kernel times: run
it under `rocprofv3 --kernel-trace --stats` in a run of its own.  Prints one JSON line.

    python3 tools/measure_cast.py [--reps 5] [--frames 60]
"""
import argparse
import json
import os
import sys

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
    assert torch.cuda.is_available(), "measure_cast.py needs the GPU"
    stream = torch.cuda.current_stream()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        stream.synchronize()
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    ppf = scenes.FRAME_POINTS
    P = scenes.TERRAIN_PARAMS
    frames = scenes.terrain_frames(a.frames + 2)
    origin, body = frames[0], frames[1:1 + a.frames * ppf]
    tb = torch.from_numpy(np.ascontiguousarray(body)).cuda()
    nxt_host = np.ascontiguousarray(frames[1 + a.frames * ppf:1 + (a.frames + 1) * ppf])
    px, py = scenes._pose_xy(np.int64(a.frames), 200.0, 14.0)
    sensor = np.array([px, py, float(scenes.heightfield(np.array([px]), np.array([py]), 0x5EED0003)[0]) + 1.8], np.float32)
    far_host = (sensor[None, :] + np.float32(1.5) * (nxt_host[:, :3] - sensor[None, :])).astype(np.float32)
    rays = {"": torch.from_numpy(nxt_host).cuda(), "_x15": torch.from_numpy(far_host).cuda()}
    o_dev = torch.from_numpy(sensor).cuda()

    m = g.TwoDmap(P["grid_len"], P["z_len"], strategy=1, max_nodes_hint=2_000_000, max_points_hint=len(body) + ppf + 1)
    m.setInterval(P["slope_interval"])
    m.setCloudFirst(origin)
    for f in range(a.frames):
        m.change2DMap("slope", tb[f * ppf:(f + 1) * ppf])
    nodes = m.sync()[0]
    g.TwoDmap.set_debug_option(5, 0)           # the plain column-index walk (the default)
    passes = torch.zeros(nodes, dtype=torch.int32, device="cuda")

    # the count-only walk without its wait: the entry point itself, stats = NULL, as the casts are called
    import ctypes as C
    from grid_ndt_amd._lib import ClearParams
    from grid_ndt_amd.map2d import _stream_ptr
    cp = ClearParams(0.0, 0.0, 1, 1)
    o3 = (C.c_float * 3)(*[float(v) for v in sensor])

    def count_only(t):
        rc = m._L.gndt_clear_rays_device(m._h, o3, C.c_void_p(t.data_ptr()), t.shape[0], 4 * t.shape[1], C.byref(cp),
                                         C.c_void_p(passes.data_ptr()), None, _stream_ptr(None))
        assert rc == 0

    out = {"tool": "measure_cast", "source_hash": g._lib.source_hash()[:16], "reps": a.reps, "frames": a.frames, "rays": ppf, "nodes": nodes}
    res = {}
    for suffix, t in rays.items():
        calls = {"cast_voxel": lambda t=t: m.cast_rays(o_dev, t, mode="voxel"),
                 "cast_ndt": lambda t=t: m.cast_rays(o_dev, t, mode="ndt"),
                 "count_only": lambda t=t: count_only(t)}
        for r in range(a.reps + 1):
            for key, fn in calls.items():
                d = timed(fn)
                if r:
                    res.setdefault(key + suffix, []).append(d)
        for mode in ("voxel", "ndt"):
            _, st = m.cast_rays(o_dev, t, mode=mode, stats=True)
            out[f"stats_{mode}{suffix}"] = st
            out[f"hit_share_{mode}{suffix}"] = st["hits"] / max(st["rays"], 1)
    out["s4"] = {**{k + "_ms": float(np.median(v)) for k, v in res.items()}, "samples": res}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
