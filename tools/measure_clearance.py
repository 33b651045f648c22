#!/usr/bin/env python3
"""The clearance field (gndt_clearance_device) on MI355X: one process, one GPU.

Workloads (DESIGN.md §4.3l "Clearance field"):
  s2       bench.py's S2 map (10 M uniform points in [-100,100)^2 x [-1,1), 0.5 m cells, 796 015 rows)
  terrain  scenes.terrain_cloud(2_000_000) at TERRAIN_PARAMS
  frame    callback-sized frames, each cropped to the centred window whose map the one-workgroup kernel holds (<= 9216 rows), through
           that kernel and through a launch a hop: scenes.campus_frame(60_000) at CAMPUS_PARAMS (LiDAR sparsity: few slopes, a barrier
           never more than a step away) and the middle of scenes.drivable_site(200_000) at COST_PARAMS (slopes many steps from one)
Per map: the call (hops and nearest out) under BLOCKED and under BLOCKED | OPEN at max_hops 8 and 32, the counts of each; and at
max_hops 256 under the same sources: where the field has converged within 32 hops the extra launches find nothing left to do, and
(t256 - t32) / 224 is what an idle launch costs.
The yardstick from the same run: a first gndt_compute_cost with a robot wider than a cell (radius 0.6: its k_cost_neighbours makes the
same four column probes a slope, its k_cost_ring_round reads one word a row through the same step masks).
Every figure is the median of `--reps` calls, each between two HIP events on the stream (the call's host side included).  Prints one
JSON line.

    python3 tools/measure_clearance.py [--reps 20] [--maps s2,terrain,frame]

Per kernel: the time of each kernel (k_clearance_*, and the yardstick's k_cost_neighbours and k_cost_ring_round) comes from a run of its
own under the profiler, one map and one case at a time so that every launch of a kernel does comparable work, read back by this tool
(counters, if wanted, in yet another run):

    rocprofv3 --kernel-trace --stats --output-format csv -d trace_s2 -- \\
        python3 tools/measure_clearance.py --maps s2 --cases blocked_open --hops 32 --reps 3 --warmup 0
    python3 tools/measure_clearance.py --kernel-stats trace_s2        # needs no GPU: one JSON line, microseconds per kernel
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("k_clearance_steps", "k_clearance_round", "k_clearance_wg", "k_clearance_finish", "k_cost_neighbours", "k_cost_ring_round")
CASES = {"blocked": 1, "blocked_open": 3}


def kernel_stats(root):
    """{kernel: calls, mean / min / max in microseconds} from rocprofv3's kernel statistics under `root`"""
    import csv
    import glob
    files = sorted(glob.glob(os.path.join(root, "**", "*kernel_stats.csv"), recursive=True))
    assert files, f"no *kernel_stats.csv under {root}"
    out = {"tool": "measure_clearance", "kernel_stats": files}
    for f in files:
        with open(f) as fh:
            for r in csv.DictReader(fh):
                for k in KERNELS:
                    if k + "(" in r["Name"] or k + "<" in r["Name"]:
                        out[k] = {"calls": int(r["Calls"]), "mean_us": round(float(r["AverageNs"]) / 1e3, 2),
                                  "min_us": round(float(r["MinNs"]) / 1e3, 2), "max_us": round(float(r["MaxNs"]) / 1e3, 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--terrain-points", type=int, default=2_000_000)
    ap.add_argument("--frame-points", type=int, default=60_000, help="points of the campus frame")
    ap.add_argument("--maps", default="s2,terrain,frame")
    ap.add_argument("--cases", default="blocked,blocked_open", help="(a trace of one case gives that case's kernel times)")
    ap.add_argument("--hops", default="8,32")
    ap.add_argument("--no-yardstick", action="store_true", help="leave the flood out (a trace of the field's kernels alone)")
    ap.add_argument("--kernel-stats", metavar="DIR", help="print the field's and the yardstick's kernel times from the *kernel_stats.csv files under DIR")
    a = ap.parse_args()
    if a.kernel_stats:
        print(json.dumps(kernel_stats(a.kernel_stats)))
        return
    import torch
    import grid_ndt_amd as g
    from grid_ndt_amd import scenes
    from grid_ndt_amd._lib import ClearanceParams
    from grid_ndt_amd.map2d import _stream_ptr
    assert torch.cuda.is_available(), "measure_clearance.py needs the GPU"
    stream = torch.cuda.current_stream()
    sp = _stream_ptr(None)
    cases, hops_list = a.cases.split(","), [int(v) for v in a.hops.split(",")]

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

    def build(cloud, P, hint=0, strategy=0):
        m = g.TwoDmap(P["grid_len"], P["z_len"], max_nodes_hint=hint, strategy=strategy)
        m.setInterval(P["slope_interval"])
        m.setCloudFirst(cloud[0])
        pts = torch.from_numpy(np.ascontiguousarray(cloud[1:, :3])).cuda()
        m.create2DMap("slope", pts)
        return m, pts

    def field_case(m, rows, mask, idle=True):
        hops = torch.empty(rows, dtype=torch.int32, device="cuda")
        near = torch.empty(rows, dtype=torch.int32, device="cuda")
        counts = torch.zeros(4, dtype=torch.int32, device="cuda")

        def call(max_hops):
            prm = ClearanceParams(mask, max_hops)
            rc = m._L.gndt_clearance_device(m._h, None, C.byref(prm), C.c_void_p(hops.data_ptr()), C.c_void_p(near.data_ptr()), None,
                                            C.c_void_p(counts.data_ptr()), sp)
            assert rc == 0, m._L.gndt_last_error(m._h)
        out = {}
        for mh in hops_list + ([256] if idle else []):
            ms, samples = timed(lambda: call(mh), a.reps, a.warmup)
            c = [int(v) for v in counts.cpu()]
            out[f"hops_{mh}"] = {"ms": ms, "samples_ms": samples, "sources": c[0], "finite": c[1], "largest_hops": c[2]}
        if idle and 32 in hops_list:     # (idle launches only where the field had converged by then: largest_hops of hops_256 below 32)
            out["launch_beyond_32_us"] = round((out["hops_256"]["ms"] - out["hops_32"]["ms"]) / 224 * 1e3, 3)
        return out

    def yardstick(m, pts):
        """a first flood from a slope of the cloud, robot radius 0.6: one ring round on 0.5 m cells"""
        head = pts[:4096].contiguous()
        r = m.query(head, "node").long()
        ok = torch.nonzero((r >= 0) & ((m.export_device()["flags"][r.clamp(min=0)] & 2) != 0)).flatten()
        goal = [float(v) for v in head[int(ok[0])].cpu()]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        st = m.computeCost(goal, robot=dict(radius=0.6))
        e1.record(stream)
        e1.synchronize()
        return {"ms": round(e0.elapsed_time(e1), 4), "rc": st["rc"], "ring": st["ring"], "levels": st["levels"], "traversable": st["traversable"]}

    def measure(cloud, P, hint):
        m, pts = build(cloud, P, hint)
        rows, cols, slopes = m.sync()
        out = {"rows": rows, "columns": cols, "slopes": slopes}
        for name in cases:
            out[name] = field_case(m, rows, CASES[name])
        if not a.no_yardstick:
            out["first_compute_cost_r06"] = yardstick(m, pts)
        return out

    out = {"tool": "measure_clearance", "device": g.device_info(0).get("name"), "source_hash": g._lib.source_hash()[:16], "reps": a.reps}
    maps = a.maps.split(",")
    if "s2" in maps:
        out["s2"] = measure(scenes.uniform_box(a.points + 1), dict(grid_len=0.5, z_len=0.5, slope_interval=0.08), 1 << 20)
    if "terrain" in maps:
        out["terrain"] = measure(scenes.terrain_cloud(a.terrain_points), scenes.TERRAIN_PARAMS, 0)
    if "frame" in maps:
        out["frames"] = {}
        for name, cloud, P in (("campus", scenes.campus_frame(a.frame_points), scenes.CAMPUS_PARAMS),
                               ("site_middle", scenes.drivable_site(200_000), scenes.COST_PARAMS)):
            m, pts = build(cloud, P, strategy=1)
            rows, cols, slopes = m.sync()
            fr = {"points": len(cloud) - 1, "rows_before_crop": rows}
            while rows > 9216:                          # a centred window, a fifth narrower each time, until the map fits
                c = m.export_device()
                x0, x1, y0, y1 = (int(v) for v in (c["sx"].min(), c["sx"].max(), c["sy"].min(), c["sy"].max()))
                dx, dy = max((x1 - x0) // 10, 1), max((y1 - y0) // 10, 1)
                m.crop_box((x0 + dx, x1 - dx, y0 + dy, y1 - dy), "keep_inside")
                rows, cols, slopes = m.sync()
            fr.update(rows=rows, columns=cols, slopes=slopes)
            try:
                for path, on in (("one_workgroup", 1), ("launch_a_hop", 0)):
                    g.TwoDmap.set_debug_option(g.TwoDmap.DEBUG_CLEARANCE_ONE_WORKGROUP, on)
                    fr[path] = {case: field_case(m, rows, CASES[case], idle=not on) for case in cases}
            finally:
                g.TwoDmap.set_debug_option(g.TwoDmap.DEBUG_CLEARANCE_ONE_WORKGROUP, 1)
            out["frames"][name] = fr
    out["what"] = ("median of HIP-event intervals around single gndt_clearance_device calls and one first gndt_compute_cost (host side of "
                   "the call included); kernel times come from a separate rocprofv3 --kernel-trace --stats run")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
