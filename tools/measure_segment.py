#!/usr/bin/env python3
"""Scan segmentation (gndt_segment_scan_device) on MI355X: one process, one GPU.

Workloads (DESIGN.md §4.3p "Scan segmentation"):
  site   the 17 k-row drivable site's map (scenes.drivable_site, COST_PARAMS); the scan is a 131 072-point frame of it — points of the
         site's own surface in ring-major, azimuth order around the origin, as a spinning LiDAR emits them — with four boxes of 1 024
         points each that were not there when the map was made; the same points in scan order and shuffled
  s2     bench.py's S2 map (10 M uniform points in [-100,100)^2 x [-1,1), 0.5 m cells); the scan is another 10 M-point sample of a box
         half as high again, so that a sixth of it lies above the map
Per scan: the call with the list filled (cluster_cap = counts[0]) and count-only, with per-point outputs, at DIRECT7; its four counts.
The yardstick from the same run: gndt_score_poses_device with per-point outputs on the same scan, same neighbourhood, K = 1.
Every figure is the median of `--reps` calls, each between two HIP events on the stream (the call's host side included).  Prints one
JSON line.

    python3 tools/measure_segment.py [--reps 20] [--maps site,s2]

Per pass: the time of each kernel (k_seg_*, and the yardstick's k_score) comes from a run of its own under the profiler, one map and one
order at a time so that every launch of a kernel does the same work, read back by this tool:

    rocprofv3 --kernel-trace --stats --output-format csv -d trace_site -- \\
        python3 tools/measure_segment.py --maps site --orders scan --reps 3 --warmup 0
    python3 tools/measure_segment.py --kernel-stats trace_site        # needs no GPU: one JSON line, microseconds per kernel
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("k_seg_classify", "k_seg_cells", "k_seg_link", "k_seg_flatten", "k_seg_count", "k_seg_scan", "k_seg_rank", "k_seg_reduce",
           "k_seg_finish", "k_score")


def kernel_stats(root):
    """{kernel: calls, mean / min / max in microseconds} from rocprofv3's kernel statistics under `root`, the passes' sum and the
    share of classify + insert in it"""
    import csv
    import glob
    files = sorted(glob.glob(os.path.join(root, "**", "*kernel_stats.csv"), recursive=True))
    assert files, f"no *kernel_stats.csv under {root}"
    out = {"tool": "measure_segment", "kernel_stats": files}
    for f in files:
        with open(f) as fh:
            for r in csv.DictReader(fh):
                for k in KERNELS:
                    if (k + "(" in r["Name"] or k + "<" in r["Name"]) and "k_score_" not in r["Name"]:
                        out[k] = {"calls": int(r["Calls"]), "mean_us": round(float(r["AverageNs"]) / 1e3, 2),
                                  "min_us": round(float(r["MinNs"]) / 1e3, 2), "max_us": round(float(r["MaxNs"]) / 1e3, 2)}
    seg = {k: v["mean_us"] for k, v in out.items() if k.startswith("k_seg_")}
    out["passes_sum_us"] = round(sum(seg.values()), 2)
    if seg:
        out["classify_share"] = round(seg.get("k_seg_classify", 0.0) / out["passes_sum_us"], 4)
    return out


def site_frame(cloud, n=131072, box_points=1024, seed=11):
    """n points of the site's own cloud and four boxes of box_points above the ground, in ring-major, azimuth order around the origin"""
    rng = np.random.default_rng(seed)
    ground = cloud[1:n + 1, :3].astype(np.float64)
    boxes = [rng.uniform(lo, hi, size=(box_points, 3)) for lo, hi in (((-6.0, -6.0, 0.9), (-4.2, -5.2, 2.5)), ((2.0, 3.0, 1.0), (2.9, 3.4, 1.7)),
                                                                      ((9.0, -14.0, 0.8), (13.0, -12.5, 2.4)), ((-15.0, 10.0, 1.0), (-14.2, 10.8, 2.8)))]
    pts = np.concatenate([ground] + boxes)
    d = pts[:, :2] - cloud[0, :2].astype(np.float64)
    rad, az = np.hypot(d[:, 0], d[:, 1]), np.arctan2(d[:, 1], d[:, 0])
    ring = np.minimum((64 * rad / (rad.max() + 1e-9)).astype(np.int64), 63)
    return np.ascontiguousarray(pts[np.lexsort((az, ring))].astype(np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--maps", default="site,s2")
    ap.add_argument("--orders", default="scan,shuffled")
    ap.add_argument("--kernel-stats", metavar="DIR", help="print the passes' and the yardstick's kernel times from the *kernel_stats.csv files under DIR")
    a = ap.parse_args()
    if a.kernel_stats:
        print(json.dumps(kernel_stats(a.kernel_stats)))
        return
    import torch
    import grid_ndt_amd as g
    from grid_ndt_amd import scenes
    from grid_ndt_amd._lib import ScoreParams, SegmentParams
    from grid_ndt_amd.map2d import _stream_ptr
    assert torch.cuda.is_available(), "measure_segment.py needs the GPU"
    stream = torch.cuda.current_stream()
    sp = _stream_ptr(None)
    T = g.TwoDmap

    def timed(fn, reps, warmup):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return round(float(np.median(ts)), 4), [round(t, 4) for t in ts]

    def scan_case(m, pts):
        n = len(pts)
        out = {"points": n}
        prm = SegmentParams(7)
        counts = torch.zeros(4, dtype=torch.int32, device="cuda")
        cls = torch.empty(n, dtype=torch.uint8, device="cuda")
        lab = torch.empty(n, dtype=torch.int32, device="cuda")

        def call(recs, cap):
            rc = m._L.gndt_segment_scan_device(m._h, C.c_void_p(pts.data_ptr()), n, 12, None, C.byref(prm), C.c_void_p(cls.data_ptr()),
                                               C.c_void_p(lab.data_ptr()), C.c_void_p(recs.data_ptr() if cap else 0), cap,
                                               C.c_void_p(counts.data_ptr()), sp)
            assert rc == 0, m._L.gndt_last_error(m._h)
        call(None, 0)
        c = [int(v) for v in counts.cpu()]
        out.update(listed=c[0], novel_points=c[1], novel_cells=c[2], clusters=c[3])
        recs = torch.zeros((max(c[0], 1), 18), dtype=torch.int32, device="cuda")
        out["ms"], out["samples_ms"] = timed(lambda: call(recs, recs.shape[0]), a.reps, a.warmup)
        out["count_only_ms"], _ = timed(lambda: call(None, 0), a.reps, a.warmup)
        # the yardstick: scan scoring with per-point outputs, same neighbourhood, one pose
        sprm = ScoreParams(7, 0, 0.0, 0.0, 0.0, 0)
        pose = torch.from_numpy(np.eye(4)[:3].reshape(12).copy()).cuda()
        rec = torch.empty((1, 4), dtype=torch.int64, device="cuda")
        d2 = torch.empty(n, dtype=torch.float32, device="cuda")
        row = torch.empty(n, dtype=torch.int32, device="cuda")

        def score():
            rc = m._L.gndt_score_poses_device(m._h, C.c_void_p(pts.data_ptr()), n, 12, C.c_void_p(pose.data_ptr()), 1, C.byref(sprm),
                                              C.c_void_p(rec.data_ptr()), C.c_void_p(d2.data_ptr()), C.c_void_p(row.data_ptr()), sp)
            assert rc == 0, m._L.gndt_last_error(m._h)
        out["score_poses_ms"], out["score_poses_samples_ms"] = timed(score, a.reps, a.warmup)
        out["ratio_to_score"] = round(out["ms"] / out["score_poses_ms"], 3)
        return out

    def measure(cloud, P, hint, scan):
        m = T(P["grid_len"], P["z_len"], max_nodes_hint=hint)
        m.setInterval(P["slope_interval"])
        m.setCloudFirst(cloud[0])
        m.create2DMap("slope", torch.from_numpy(np.ascontiguousarray(cloud[1:, :3])).cuda())
        rows, cols, slopes = m.sync()
        out = {"rows": rows, "columns": cols}
        rng = np.random.default_rng(1)
        for order in a.orders.split(","):
            pts = scan if order == "scan" else scan[rng.permutation(len(scan))]
            out[order] = scan_case(m, torch.from_numpy(np.ascontiguousarray(pts)).cuda())
        return out

    out = {"tool": "measure_segment", "device": g.device_info(0).get("name"), "source_hash": g._lib.source_hash()[:16], "reps": a.reps}
    maps = a.maps.split(",")
    if "site" in maps:
        cloud = scenes.drivable_site()
        out["site"] = measure(cloud, scenes.COST_PARAMS, 0, site_frame(cloud))
    if "s2" in maps:
        cloud = scenes.uniform_box(a.points + 1)
        out["s2"] = measure(cloud, dict(grid_len=0.5, z_len=0.5, slope_interval=0.08), 1 << 20,
                            scenes.uniform_box(a.points, seed=0x5EED0012, half_z=1.5))
    out["what"] = ("median of HIP-event intervals around single gndt_segment_scan_device / gndt_score_poses_device calls (host side of the "
                   "call included); kernel times come from a separate rocprofv3 --kernel-trace --stats run")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
