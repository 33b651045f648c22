#!/usr/bin/env python3
"""Scan scoring on the bench's map (gndt_score_poses_device): one process, one GPU.

Builds the S2 map (bench.py's default workload: 10 M uniform points in [-100,100)^2 x [-1,1), 0.5 m cells, max_nodes_hint 2^20) and
times, in the same process and run:
  * the yardstick: gndt_query_device, NODE mode, 1 query per thread, over the build's own 10 M points;
  * the score of those points: DIRECT1 at the identity (K = 1), DIRECT1 at K = 8 poses within +-0.5 cell of the identity, DIRECT7 at
    K = 1 — each with and without the per-point outputs.
Every figure is the median of `--reps` calls, each between two HIP events on the stream (so it includes the call's host side: its
gndt_sync and its two launches).  Kernel times: run it under `rocprofv3 --kernel-trace --stats` in a run of its own (no counters
in that run); `--kernel-trace FILE` folds that run's kernel_trace.csv into the JSON line.  Prints one JSON line.

    python3 tools/measure_score.py [--reps 20] [--kernel-trace kernel_trace.csv]
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
    """rocprofv3's kernel_trace.csv -> {kernel [poses in the launch]: {calls, median_us}} for the query and score kernels (a score
    launch's grid has one row of workgroups per pose)"""
    groups = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r.get("Kernel_Name", "")
            if "k_score" not in name and "k_query" not in name:
                continue
            short = name.split("(")[0].replace("void ", "").replace("gndt::", "")
            if "k_score<" in short:
                short += " K=%d" % (int(r["Grid_Size_Y"]) // max(1, int(r["Workgroup_Size_Y"])))
            groups.setdefault(short, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return {k: {"calls": len(v), "median_us": round(float(np.median(v)), 2)} for k, v in sorted(groups.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--kernel-trace", default=None)
    a = ap.parse_args()
    import torch
    import grid_ndt_amd as g
    from grid_ndt_amd import _lib, scenes
    from grid_ndt_amd.map2d import _stream_ptr
    assert torch.cuda.is_available(), "measure_score.py needs the GPU"
    n = a.points
    stream = torch.cuda.current_stream()

    def timed(fn, reps, warmup, post=None):
        for _ in range(warmup):
            fn()
            post and post()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            post and post()
            ts.append(e0.elapsed_time(e1))
        return float(np.median(ts)), [round(t, 4) for t in ts]

    cloud = scenes.uniform_box(n + 1)
    P = dict(grid_len=0.5, z_len=0.5, slope_interval=0.08)
    m = g.TwoDmap(P["grid_len"], P["z_len"], max_nodes_hint=1 << 20)
    m.setInterval(P["slope_interval"])
    m.setCloudFirst(cloud[0])
    pts = torch.from_numpy(cloud[1:]).cuda()
    build_ms, _ = timed(lambda: m.create2DMap("slope", pts), a.reps, 5, post=m.sync)
    nodes, cols, _ = m.sync()

    L, sp = m._L, _stream_ptr(None)
    rows = torch.empty(n, dtype=torch.int32, device="cuda")
    d2 = torch.empty(n, dtype=torch.float32, device="cuda")

    def query():
        rc = L.gndt_query_device(m._h, C.c_void_p(pts.data_ptr()), n, 12, 0, C.c_void_p(rows.data_ptr()), None, None, sp)
        assert rc == 0, L.gndt_last_error(m._h)

    g.TwoDmap.set_debug_option(g.TwoDmap.DEBUG_QUERY_ILP, 1)
    query_ms, query_samples = timed(query, a.reps, a.warmup)
    answered = float((rows >= 0).float().mean().item())

    rng = np.random.default_rng(0x5EED005C)
    ident = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)
    near = np.tile(ident, (8, 1, 1))
    near[1:, :2, 3] = rng.uniform(-0.5, 0.5, size=(7, 2)) * P["grid_len"]
    near[1:, 2, 3] = rng.uniform(-0.5, 0.5, size=7) * P["z_len"]
    sets = [("direct1_k1", 1, ident[None]), ("direct1_k8", 1, near), ("direct7_k1", 7, ident[None])]
    scores = {}
    for name, nbh, poses in sets:
        K = poses.shape[0]
        T = torch.from_numpy(np.ascontiguousarray(poses.reshape(K, 12))).cuda()
        rec = torch.zeros((K, 4), dtype=torch.int64, device="cuda")
        for per_point in (False, True):
            prm = _lib.ScoreParams(nbh, 0, 0.0, 0.0, 0.0, 0)

            def score():
                rc = L.gndt_score_poses_device(m._h, C.c_void_p(pts.data_ptr()), n, 12, C.c_void_p(T.data_ptr()), K, C.byref(prm),
                                               C.c_void_p(rec.data_ptr()), C.c_void_p(d2.data_ptr() if per_point else 0),
                                               C.c_void_p(rows.data_ptr() if per_point else 0), sp)
                assert rc == 0, L.gndt_last_error(m._h)
            ms, samples = timed(score, a.reps, a.warmup)
            r = rec.cpu().numpy()
            scores[name + ("_per_point" if per_point else "")] = {
                "ms": round(ms, 4), "samples_ms": samples, "ms_per_pose": round(ms / K, 4), "x_yardstick_per_pose": round(ms / K / query_ms, 3),
                "Mpairs_per_s": round(n * K / ms / 1e3, 1), "matched_share_pose0": round(int(r[0, 2]) / n, 4),
                "terms_pose0": int(r[0, 3]), "score_pose0": float(r.view(np.float64)[0, 0])}
    ratio = scores["direct1_k1"]["ms"] / query_ms
    res = {"tool": "measure_score", "points": n, "device": g.device_info(0).get("name"), "source_hash": _lib.source_hash(),
           "s2_map": {"nodes": nodes, "columns": cols}, "s2_build_ms": round(build_ms, 4),
           "yardstick_query_node_ilp1": {"ms": round(query_ms, 4), "samples_ms": query_samples, "answered": round(answered, 4)},
           "score": scores,
           "direct1_k1_x_yardstick": round(ratio, 3), "target_x_yardstick": 2.5, "target_met": bool(ratio <= 2.5),
           "k8_x_k1": round(scores["direct1_k8"]["ms"] / scores["direct1_k1"]["ms"], 3),
           "direct7_x_direct1": round(scores["direct7_k1"]["ms"] / scores["direct1_k1"]["ms"], 3),
           "what": "median of HIP-event intervals around single calls (host side of the call included); kernel times come from rocprofv3"}
    if a.kernel_trace:
        res["kernels"] = kernel_trace(a.kernel_trace)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
