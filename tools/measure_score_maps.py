#!/usr/bin/env python3
"""Map-to-map scoring on the bench's map (gndt_score_maps_device / gndt_score_maps_derivs_device): one process, one GPU.

Builds the S2 map (bench.py's default workload: 10 M uniform points in [-100,100)^2 x [-1,1), 0.5 m cells, max_nodes_hint 2^20;
796 015 nodes) and the map of every second of its points, and scores, as the source, the map itself and the map of half its points
against it, for K = 1 and K = 4 poses within +-0.5 cell of the identity and both neighbourhoods.  Timed in the same process and run,
call by call in turns (A B C D A B C D ...):
  * the yardstick, what stitch(method="means") runs: gndt_score_poses_device and gndt_score_derivs_device on the same destination
    with the means of the source's rows that have statistics as the scan;
  * gndt_score_maps_device (no per-node outputs) and gndt_score_maps_derivs_device.
Every figure is the median of `--reps` calls after a warm-up round, each between two HIP events on the stream (so it includes the
call's host side).  Kernel times: run it under `rocprofv3 --kernel-trace --stats` in a run of its own (no counters in that run);
`--kernel-trace FILE` folds that run's kernel_trace.csv into the JSON line.
Prints one JSON line.

    python3 tools/measure_score_maps.py [--reps 7] [--kernel-trace kernel_trace.csv]
"""
import argparse
import csv
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def kernel_trace(path):
    """rocprofv3's kernel_trace.csv -> {kernel [poses in the launch, workgroups a pose]: {calls, median_us}} for the score kernels"""
    groups = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r.get("Kernel_Name", "")
            if "k_score" not in name:
                continue
            short = name.split("(")[0].replace("void ", "").replace("gndt::", "")
            if "reduce" not in short and "finish" not in short:
                short += " K=%d n=%d" % (int(r["Grid_Size_Y"]) // max(1, int(r["Workgroup_Size_Y"])), int(r["Grid_Size_X"]))
            groups.setdefault(short, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return {k: {"calls": len(v), "median_us": round(float(np.median(v)), 2)} for k, v in sorted(groups.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--kernel-trace", default=None)
    a = ap.parse_args()
    import torch
    import grid_ndt_amd as g
    from grid_ndt_amd import _lib, scenes
    from grid_ndt_amd.map2d import _stream_ptr
    assert torch.cuda.is_available(), "measure_score_maps.py needs the GPU"
    n = a.points
    stream = torch.cuda.current_stream()

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    cloud = scenes.uniform_box(n + 1)
    P = dict(grid_len=0.5, z_len=0.5, slope_interval=0.08)

    def build(points):
        m = g.TwoDmap(P["grid_len"], P["z_len"], max_nodes_hint=1 << 20)
        m.setInterval(P["slope_interval"])
        m.setCloudFirst(cloud[0])
        m.create2DMap("slope", points)
        return m

    pts = torch.from_numpy(cloud[1:]).cuda()
    dst = build(pts)
    half = build(pts[::2].contiguous())
    nodes, cols, _ = dst.sync()

    L, sp = dst._L, _stream_ptr(None)
    rng = np.random.default_rng(0x5EED005D)
    ident = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)
    near = np.tile(ident, (4, 1, 1))
    near[1:, :2, 3] = rng.uniform(-0.5, 0.5, size=(3, 2)) * P["grid_len"]
    near[1:, 2, 3] = rng.uniform(-0.5, 0.5, size=3) * P["z_len"]
    calls = {}
    for sname, src in (("self", dst), ("half", half)):
        cells = src.export_device()
        scan = cells["mean"][(cells["flags"] & 1) != 0].contiguous()
        ns = int(scan.shape[0])
        for nbh in (1, 7):
            for K, poses in ((1, ident[None]), (4, near)):
                T = torch.from_numpy(np.ascontiguousarray(poses.reshape(K, 12))).cuda()
                recs = {k: torch.zeros((K, w), dtype=torch.int64, device="cuda") for k, w in
                        (("score", 4), ("derivs", 31), ("maps", 4), ("maps_derivs", 31))}
                prm = _lib.ScoreParams(nbh, 0, 0.0, 0.0, 0.0, 0)
                p = lambda t: C.c_void_p(t.data_ptr())

                def check(rc):
                    assert rc == 0, L.gndt_last_error(dst._h)

                fns = {
                    "score": lambda: check(L.gndt_score_poses_device(dst._h, p(scan), ns, 12, p(T), K, C.byref(prm), p(recs["score"]), None, None, sp)),
                    "derivs": lambda: check(L.gndt_score_derivs_device(dst._h, p(scan), ns, 12, p(T), K, C.byref(prm), p(recs["derivs"]), sp)),
                    "maps": lambda: check(L.gndt_score_maps_device(dst._h, src._h, p(T), K, C.byref(prm), p(recs["maps"]), None, None, sp)),
                    "maps_derivs": lambda: check(L.gndt_score_maps_derivs_device(dst._h, src._h, p(T), K, C.byref(prm), p(recs["maps_derivs"]), sp)),
                }
                for _ in range(a.warmup):
                    for fn in fns.values():
                        fn()
                torch.cuda.synchronize()
                t = {k: [] for k in fns}
                for _ in range(a.reps):                     # A B C D A B C D
                    for k, fn in fns.items():
                        t[k].append(once(fn))
                r = {k: v.cpu().numpy() for k, v in recs.items()}
                assert np.array_equal(r["maps"], r["maps_derivs"][:, :4]), "the four sums are not score_map's bits"
                med = {k: float(np.median(v)) for k, v in t.items()}
                calls["%s_direct%d_k%d" % (sname, nbh, K)] = {
                    "source_rows": int(src.sync()[0]), "source_rows_with_statistics": ns,
                    "means_score_ms": round(med["score"], 4), "means_derivs_ms": round(med["derivs"], 4),
                    "maps_score_ms": round(med["maps"], 4), "maps_derivs_ms": round(med["maps_derivs"], 4),
                    "maps_x_means_score": round(med["maps"] / med["score"], 3), "maps_x_means_derivs": round(med["maps_derivs"] / med["derivs"], 3),
                    "samples_ms": {k: [round(x, 4) for x in v] for k, v in t.items()},
                    "terms_pose0": {"means": int(r["score"][0, 3]), "maps": int(r["maps"][0, 3])}}
    res = {"tool": "measure_score_maps", "points": n, "device": g.device_info(0).get("name"), "source_hash": _lib.source_hash(),
           "s2_map": {"nodes": nodes, "columns": cols}, "calls": calls,
           "what": "median of HIP-event intervals around single calls, the four calls in turns (host side of the call included); "
                   "kernel times come from rocprofv3"}
    if a.kernel_trace:
        res["kernels"] = kernel_trace(a.kernel_trace)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
