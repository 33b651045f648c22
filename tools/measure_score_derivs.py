#!/usr/bin/env python3
"""Scan score derivatives and the Newton registration on the bench's map (gndt_score_derivs_device, TwoDmap.register): one process,
one GPU.

Builds the S2 map (bench.py's default workload: 10 M uniform points in [-100,100)^2 x [-1,1), 0.5 m cells, max_nodes_hint 2^20) and
times, in the same process and run, call by call in turns (A B A B ...):
  * the yardstick: gndt_score_poses_device without per-point outputs, the same neighbourhood, points and poses;
  * gndt_score_derivs_device,
for DIRECT1 at the identity (K = 1), DIRECT1 at K = 8 poses within +-0.5 cell of the identity and DIRECT7 at K = 1.  Every figure is
the median of `--reps` calls, each between two HIP events on the stream (so it includes the call's host side).  Kernel times: run it
under `rocprofv3 --kernel-trace --stats` in a run of its own (no counters in that run); `--kernel-trace FILE` folds that run's
kernel_trace.csv into the JSON line.
Registration: TwoDmap.register (DIRECT7) from two starts a fraction of a cell off, with the build's own 10 M points and with every
76th of them (131 579 points) as the scan: wall-clock ms per iteration (one derivs call, one score call of four poses, two copies to
the host, numpy's 6 x 6 eigen-decomposition), iterations, the ending and the final pose error.  The yaw of the starts is small on
purpose: the scan reaches 141 m from the origin, and a rotation has to move its farthest point by less than a cell.
Prints one JSON line.

    python3 tools/measure_score_derivs.py [--reps 20] [--kernel-trace kernel_trace.csv]
"""
import argparse
import csv
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def kernel_trace(path):
    """rocprofv3's kernel_trace.csv -> {kernel [poses in the launch]: {calls, median_us}} for the score kernels (a launch's grid has
    one row of workgroups per pose)"""
    groups = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r.get("Kernel_Name", "")
            if "k_score" not in name:
                continue
            short = name.split("(")[0].replace("void ", "").replace("gndt::", "")
            if "k_score<" in short or "k_score_derivs<" in short:
                short += " K=%d n=%d" % (int(r["Grid_Size_Y"]) // max(1, int(r["Workgroup_Size_Y"])), int(r["Grid_Size_X"]))
            groups.setdefault(short, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return {k: {"calls": len(v), "median_us": round(float(np.median(v)), 2)} for k, v in sorted(groups.items())}


def yaw(deg, t):
    a = math.radians(deg)
    return np.array([[math.cos(a), -math.sin(a), 0, t[0]], [math.sin(a), math.cos(a), 0, t[1]], [0, 0, 1, t[2]]], np.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--kernel-trace", default=None)
    ap.add_argument("--no-register", action="store_true")
    a = ap.parse_args()
    import torch
    import grid_ndt_amd as g
    from grid_ndt_amd import _lib, scenes
    from grid_ndt_amd.map2d import _stream_ptr
    assert torch.cuda.is_available(), "measure_score_derivs.py needs the GPU"
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
    m = g.TwoDmap(P["grid_len"], P["z_len"], max_nodes_hint=1 << 20)
    m.setInterval(P["slope_interval"])
    m.setCloudFirst(cloud[0])
    pts = torch.from_numpy(cloud[1:]).cuda()
    m.create2DMap("slope", pts)
    nodes, cols, _ = m.sync()

    L, sp = m._L, _stream_ptr(None)
    rng = np.random.default_rng(0x5EED005C)
    ident = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)
    near = np.tile(ident, (8, 1, 1))
    near[1:, :2, 3] = rng.uniform(-0.5, 0.5, size=(7, 2)) * P["grid_len"]
    near[1:, 2, 3] = rng.uniform(-0.5, 0.5, size=7) * P["z_len"]
    sets = [("direct1_k1", 1, ident[None]), ("direct1_k8", 1, near), ("direct7_k1", 7, ident[None])]
    calls = {}
    for name, nbh, poses in sets:
        K = poses.shape[0]
        T = torch.from_numpy(np.ascontiguousarray(poses.reshape(K, 12))).cuda()
        rec = torch.zeros((K, 4), dtype=torch.int64, device="cuda")
        drec = torch.zeros((K, 31), dtype=torch.int64, device="cuda")
        prm = _lib.ScoreParams(nbh, 0, 0.0, 0.0, 0.0, 0)

        def score():
            rc = L.gndt_score_poses_device(m._h, C.c_void_p(pts.data_ptr()), n, 12, C.c_void_p(T.data_ptr()), K, C.byref(prm),
                                           C.c_void_p(rec.data_ptr()), None, None, sp)
            assert rc == 0, L.gndt_last_error(m._h)

        def derivs():
            rc = L.gndt_score_derivs_device(m._h, C.c_void_p(pts.data_ptr()), n, 12, C.c_void_p(T.data_ptr()), K, C.byref(prm),
                                            C.c_void_p(drec.data_ptr()), sp)
            assert rc == 0, L.gndt_last_error(m._h)

        for _ in range(a.warmup):
            score()
            derivs()
        torch.cuda.synchronize()
        ts, td = [], []
        for _ in range(a.reps):                     # A B A B
            ts.append(once(score))
            td.append(once(derivs))
        r, d = rec.cpu().numpy(), drec.cpu().numpy()
        assert np.array_equal(r, d[:, :4]), "the four sums are not score_poses' bits"
        sm, dm = float(np.median(ts)), float(np.median(td))
        calls[name] = {"score_ms": round(sm, 4), "derivs_ms": round(dm, 4), "derivs_x_score": round(dm / sm, 3),
                       "score_samples_ms": [round(t, 4) for t in ts], "derivs_samples_ms": [round(t, 4) for t in td],
                       "terms_pose0": int(r[0, 3]), "g_pose0": d.view(np.float64)[0, 4:10].tolist()}
    ratio = calls["direct1_k1"]["derivs_x_score"]
    res = {"tool": "measure_score_derivs", "points": n, "device": g.device_info(0).get("name"), "source_hash": _lib.source_hash(),
           "s2_map": {"nodes": nodes, "columns": cols}, "calls": calls,
           "direct1_k1_derivs_x_score": ratio, "target_x_score": 1.5, "target_met": bool(ratio <= 1.5),
           "what": "median of HIP-event intervals around single calls, score and derivs calls in turns (host side of the call included); "
                   "kernel times come from rocprofv3"}
    if not a.no_register:
        gl, zl = P["grid_len"], P["z_len"]
        starts = {"A": yaw(0.03, (0.2 * gl, -0.15 * gl, 0.1 * zl)), "B": yaw(0.06, (0.4 * gl, 0.3 * gl, -0.2 * zl))}
        reg = {}
        for label, scan in (("10M", pts), ("131k", pts[::76].contiguous())):
            for k, T0 in starts.items():
                m.register(scan, T0, max_iterations=1)              # (warm: the scratch is grown)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = m.register(scan, T0)
                dt = (time.perf_counter() - t0) * 1e3
                R = out["T"][:, :3]
                ang = math.acos(max(-1.0, min(1.0, (np.trace(R) - 1.0) / 2.0)))
                ang0 = math.acos(max(-1.0, min(1.0, (np.trace(T0[:, :3]) - 1.0) / 2.0)))
                reg["%s_%s" % (label, k)] = {"scan_points": int(scan.shape[0]), "iterations": out["iterations"], "reason": out["reason"],
                                            "ms_total": round(dt, 3), "ms_per_iteration": round(dt / out["iterations"], 3),
                                            "start_error_m_rad": [float(np.linalg.norm(T0[:, 3])), ang0],
                                            "final_error_m_rad": [float(np.linalg.norm(out["T"][:, 3])), ang],
                                            "scores": [float(h["derivs"]["score"]) for h in out["history"]]}
        res["register_direct7"] = reg
    if a.kernel_trace:
        res["kernels"] = kernel_trace(a.kernel_trace)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
