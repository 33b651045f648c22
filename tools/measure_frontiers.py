#!/usr/bin/env python3
"""Frontier extraction (gndt_frontiers_device) on MI355X: one process, one GPU.

Workloads (DESIGN.md §4.3k "Frontier extraction"):
  s2       bench.py's S2 map (10 M uniform points in [-100,100)^2 x [-1,1), 0.5 m cells, 796 015 rows): a box, its frontier the perimeter
  terrain  scenes.terrain_cloud(2_000_000) at TERRAIN_PARAMS: LiDAR sparsity makes a large share of the rows frontiers
Per map: the call under SLOPES and, after a first gndt_compute_cost from a slope of the cloud, under REACHED, each with both open rules;
the list filled (cluster_cap = counts[0]) and count-only (cluster_cap 0); the frontier rows and clusters of each.  The yardsticks from the
same run: that first gndt_compute_cost (whose k_cost_neighbours makes the same four column probes per row) and gndt_query_device in
NODE mode for as many points as the map has rows.
Every figure is the median of `--reps` calls, each between two HIP events on the stream (the call's host side included).  Prints one
JSON line.

    python3 tools/measure_frontiers.py [--reps 20] [--maps s2,terrain] [--cases slopes_column,...]

Per pass: the time of each kernel (k_frontier_*, and the yardsticks' k_cost_neighbours and k_query) comes from a run of its own under
the profiler, one map and one case at a time so that every launch of a kernel does the same work, read back by this tool:

    rocprofv3 --kernel-trace --stats --output-format csv -d trace_s2 -- \
        python3 tools/measure_frontiers.py --maps s2 --cases slopes_column --reps 3 --warmup 0
    python3 tools/measure_frontiers.py --kernel-stats trace_s2        # needs no GPU: one JSON line, microseconds per kernel
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


KERNELS = ("k_frontier_mark", "k_frontier_link", "k_frontier_flatten", "k_frontier_count", "k_frontier_scan", "k_frontier_rank",
           "k_frontier_reduce", "k_cost_neighbours", "k_query")


def kernel_stats(root):
    """{kernel: calls, mean / min / max in microseconds} from rocprofv3's kernel statistics under `root`, and the passes' sum"""
    import csv
    import glob
    files = sorted(glob.glob(os.path.join(root, "**", "*kernel_stats.csv"), recursive=True))
    assert files, f"no *kernel_stats.csv under {root}"
    out = {"tool": "measure_frontiers", "kernel_stats": files}
    for f in files:
        with open(f) as fh:
            for r in csv.DictReader(fh):
                for k in KERNELS:
                    if k + "(" in r["Name"] or k + "<" in r["Name"]:
                        out[k] = {"calls": int(r["Calls"]), "mean_us": round(float(r["AverageNs"]) / 1e3, 2),
                                  "min_us": round(float(r["MinNs"]) / 1e3, 2), "max_us": round(float(r["MaxNs"]) / 1e3, 2)}
    out["passes_sum_us"] = round(sum(v["mean_us"] for k, v in out.items() if k.startswith("k_frontier_")), 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--terrain-points", type=int, default=2_000_000)
    ap.add_argument("--maps", default="s2,terrain")
    ap.add_argument("--cases", default="slopes_column,slopes_level1,reached_column,reached_level1", help="(a trace of one case gives that case's kernel times)")
    ap.add_argument("--kernel-stats", metavar="DIR", help="print the passes' and the yardsticks' kernel times from the *kernel_stats.csv files under DIR")
    a = ap.parse_args()
    if a.kernel_stats:
        print(json.dumps(kernel_stats(a.kernel_stats)))
        return
    import torch
    import grid_ndt_amd as g
    from grid_ndt_amd import scenes
    from grid_ndt_amd._lib import FrontierParams
    from grid_ndt_amd.map2d import _stream_ptr
    assert torch.cuda.is_available(), "measure_frontiers.py needs the GPU"
    stream = torch.cuda.current_stream()
    sp = _stream_ptr(None)

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

    def frontier_case(m, candidates, open_rule):
        prm = FrontierParams(candidates, open_rule, 1, 1, 1, 1)
        counts = torch.zeros(4, dtype=torch.int32, device="cuda")

        def call(recs, cap):
            rc = m._L.gndt_frontiers_device(m._h, None, C.byref(prm), None, C.c_void_p(recs.data_ptr() if cap else 0), cap,
                                            C.c_void_p(counts.data_ptr()), sp)
            assert rc == 0, m._L.gndt_last_error(m._h)
        call(None, 0)
        c = [int(v) for v in counts.cpu()]
        recs = torch.zeros((max(c[0], 1), 16), dtype=torch.int32, device="cuda")
        out = {"frontier_rows": c[1], "clusters": c[2]}
        out["ms"], out["samples_ms"] = timed(lambda: call(recs, recs.shape[0]), a.reps, a.warmup)
        out["count_only_ms"], _ = timed(lambda: call(None, 0), a.reps, a.warmup)
        out["largest_cluster"] = int(recs[:, 1].max()) if c[0] else 0
        return out

    def measure(cloud, P, hint):
        m = g.TwoDmap(P["grid_len"], P["z_len"], max_nodes_hint=hint)
        m.setInterval(P["slope_interval"])
        m.setCloudFirst(cloud[0])
        pts = torch.from_numpy(np.ascontiguousarray(cloud[1:, :3])).cuda()
        m.create2DMap("slope", pts)
        rows, cols, slopes = m.sync()
        out = {"rows": rows, "columns": cols, "slopes": slopes}
        for name, cand, rule in (("slopes_column", 1, 0), ("slopes_level1", 1, 1)):
            if name in cases:
                out[name] = frontier_case(m, cand, rule)
        # the yardsticks: a first flood from a slope of the cloud, and a NODE query per row
        head = pts[:4096].contiguous()
        r = m.query(head, "node").long()
        ok = torch.nonzero((r >= 0) & ((m.export_device()["flags"][r.clamp(min=0)] & 2) != 0)).flatten()
        goal = [float(v) for v in head[int(ok[0])].cpu()]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        st = m.computeCost(goal)
        e1.record(stream)
        e1.synchronize()
        out["first_compute_cost"] = {"ms": round(e0.elapsed_time(e1), 4), "rc": st["rc"], "levels": st["levels"], "traversable": st["traversable"]}
        for name, cand, rule in (("reached_column", 0, 0), ("reached_level1", 0, 1)):
            if name in cases:
                out[name] = frontier_case(m, cand, rule)
        q = pts[:rows].contiguous() if rows <= len(pts) else pts
        qrows = torch.empty(len(q), dtype=torch.int32, device="cuda")

        def query():
            rc = m._L.gndt_query_device(m._h, C.c_void_p(q.data_ptr()), len(q), 12, 0, C.c_void_p(qrows.data_ptr()), None, None, sp)
            assert rc == 0, m._L.gndt_last_error(m._h)
        out["query_node"] = {"queries": len(q)}
        out["query_node"]["ms"], out["query_node"]["samples_ms"] = timed(query, a.reps, a.warmup)
        return out

    out = {"tool": "measure_frontiers", "device": g.device_info(0).get("name"), "source_hash": g._lib.source_hash()[:16], "reps": a.reps}
    maps, cases = a.maps.split(","), a.cases.split(",")
    if "s2" in maps:
        out["s2"] = measure(scenes.uniform_box(a.points + 1), dict(grid_len=0.5, z_len=0.5, slope_interval=0.08), 1 << 20)
    if "terrain" in maps:
        out["terrain"] = measure(scenes.terrain_cloud(a.terrain_points), scenes.TERRAIN_PARAMS, 0)
    out["what"] = ("median of HIP-event intervals around single gndt_frontiers_device / gndt_query_device calls and one first "
                   "gndt_compute_cost (host side of the call included); kernel times come from a separate rocprofv3 --kernel-trace --stats run")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
