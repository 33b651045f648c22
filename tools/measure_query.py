#!/usr/bin/env python3
"""Point queries on the bench's map (gndt_query_device): one process, one GPU.

Builds the S2 map (bench.py's default workload: 10 M uniform points in [-100,100)^2 x [-1,1), 0.5 m cells, max_nodes_hint 2^20), times
the build itself, then 10 M queries in four sets — NODE mode over the build's own points in order, the same points shuffled,
NEAREST_SLOPE over uniform random points of the box, NODE mode with the cost gather over uniform random points of the drivable_site
map after computeCost — each at 1, 2 and 4 queries per thread (GNDT_DEBUG_QUERY_ILP).  Every figure is the median of `--reps`
calls, each between two HIP events on the stream (so a query's figure includes the call's host side: its gndt_sync and launch).
Kernel times: run it under `rocprofv3 --kernel-trace --stats` in a run of its own.  Prints one JSON line.

    python3 tools/measure_query.py [--reps 20] [--ilps 1,2,4]
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
    ap.add_argument("--ilps", default="1,2,4")
    ap.add_argument("--points", type=int, default=10_000_000)
    a = ap.parse_args()
    import torch
    import grid_ndt_amd as g
    from grid_ndt_amd import scenes
    from grid_ndt_amd.map2d import _stream_ptr
    assert torch.cuda.is_available(), "measure_query.py needs the GPU"
    n = a.points
    stream = torch.cuda.current_stream()

    def timed(fn, reps, warmup, pre=None, post=None):
        for _ in range(warmup):
            pre and pre()
            fn()
            post and post()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            pre and pre()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            post and post()
            ts.append(e0.elapsed_time(e1))
        return float(np.median(ts)), [round(t, 4) for t in ts]

    # ---- the S2 map and its build time ----
    cloud = scenes.uniform_box(n + 1)
    P = dict(grid_len=0.5, z_len=0.5, slope_interval=0.08)
    m = g.TwoDmap(P["grid_len"], P["z_len"], max_nodes_hint=1 << 20)
    m.setInterval(P["slope_interval"])
    m.setCloudFirst(cloud[0])
    pts = torch.from_numpy(cloud[1:]).cuda()

    def build():
        m.create2DMap("slope", pts)
    build_ms, build_samples = timed(build, a.reps, 5, post=m.sync)
    retries = m.retry_count()
    nodes, cols, _ = m.sync()
    strategy = m.STRATEGY_NAMES.get(m.last_strategy(), str(m.last_strategy()))

    L, sp = m._L, _stream_ptr(None)
    rows = torch.empty(n, dtype=torch.int32, device="cuda")
    hq = torch.empty(n, dtype=torch.float32, device="cuda")
    sq = torch.empty(n, dtype=torch.int32, device="cuda")

    def query_fn(mm, x, mode, gather):
        args = (mm._h, C.c_void_p(x.data_ptr()), x.shape[0], 4 * x.shape[1], mode, C.c_void_p(rows.data_ptr()),
                C.c_void_p(hq.data_ptr() if gather else 0), C.c_void_p(sq.data_ptr() if gather else 0), sp)

        def f():
            rc = L.gndt_query_device(*args)
            assert rc == 0, L.gndt_last_error(mm._h)
        return f

    rng = np.random.default_rng(0x5EED00AA)
    perm = torch.from_numpy(rng.permutation(n)).cuda()
    shuffled = pts[perm].contiguous()
    rnd = np.empty((n, 3), np.float32)
    rnd[:, :2] = rng.uniform(-100, 100, size=(n, 2))
    rnd[:, 2] = rng.uniform(-1, 1, size=n)
    uniform = torch.from_numpy(rnd).cuda()
    # the cost gather: the drivable site (the flood's bench scene) and its cost map
    site = scenes.drivable_site(400_000)
    CP = scenes.COST_PARAMS
    ms = g.TwoDmap(CP["grid_len"], CP["z_len"])
    ms.setInterval(CP["slope_interval"])
    ms.setCloudFirst(site[0])
    ms.create2DMap("slope", torch.from_numpy(site[1:]).cuda())
    cost_stats = ms.computeCost(scenes.DRIVABLE_GOAL)
    lo, hi = site[1:].min(0), site[1:].max(0)
    srnd = np.stack([rng.uniform(lo[k], hi[k], size=n) for k in range(3)], 1).astype(np.float32)
    site_q = torch.from_numpy(srnd).cuda()

    sets = [("node_in_order", m, pts, 0, False), ("node_shuffled", m, shuffled, 0, False),
            ("nearest_slope_uniform", m, uniform, 1, False), ("node_cost_gather_site", ms, site_q, 0, True)]
    out_sets = {}
    for name, mm, x, mode, gather in sets:
        out_sets[name] = {}
        for ilp in [int(v) for v in a.ilps.split(",")]:
            g.TwoDmap.set_debug_option(g.TwoDmap.DEBUG_QUERY_ILP, ilp)
            ms_, samples = timed(query_fn(mm, x, mode, gather), a.reps, a.warmup)
            hit = float((rows >= 0).float().mean().item())
            out_sets[name][f"ilp{ilp}"] = {"ms": round(ms_, 4), "samples_ms": samples, "answered": round(hit, 4),
                                          "Mqueries_per_s": round(n / ms_ / 1e3, 1)}
    g.TwoDmap.set_debug_option(g.TwoDmap.DEBUG_QUERY_ILP, 1)
    # the first query after a build also builds the column index
    first_ms, first_samples = timed(query_fn(m, pts, 0, False), 5, 1, pre=lambda: (build(), m.sync()))
    res = {"tool": "measure_query", "points": n, "device": g.device_info(0).get("name"),
           "s2_map": {"nodes": nodes, "columns": cols, "strategy": strategy, "retries": retries},
           "s2_build_ms": round(build_ms, 4), "s2_build_samples_ms": [round(t, 4) for t in build_samples],
           "node_in_order_first_after_build_ms": round(first_ms, 4), "first_after_build_samples_ms": first_samples,
           "site_map": {"nodes": ms.sync()[0], "cost_levels": cost_stats["levels"]},
           "queries": out_sets,
           "what": "median of HIP-event intervals around single calls (host side of the call included); kernel times come from rocprofv3"}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
