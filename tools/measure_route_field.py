#!/usr/bin/env python3
"""The route field (gndt_route_field_device, gndt_descend_routes_device) on MI355X: one process, one GPU.

Workloads (DESIGN.md §4.3r "Route field"):
  site   the 17 k-row drivable site's map (scenes.drivable_site, COST_PARAMS): the field to one goal (the flood's, scenes.DRIVABLE_GOAL)
         and to the best members of frontiers(), each with the one-workgroup kernel and with a launch a sweep, the sweeps each needed;
         the same with a clearance field as hops (min_hops 1, a soft zone of 3); for scale gndt_compute_cost to the same goal and
         gndt_clearance_device at 32 hops; then descend_routes against plan_routes for K = 1 .. 4 096 starts (64 on s2) (where the field with
         its descent passes one A* search a start); and the site's middle third (the one-workgroup kernel at a smaller size)
  s2     bench.py's S2 map (10 M uniform points in [-100,100)^2 x [-1,1), 0.5 m cells, 796 k rows): the field to one goal and to 16
         goals, a launch a sweep (the map does not fit one workgroup), compute_cost and clearance for scale, the descent of 1 024 starts.
         Its slopes are islands (random points: the gates pass almost nowhere), so its field is the call's floor: the sweeps that return
         at once
  plane  4 M of the same points pressed into one level: 400 x 400 columns of one slope each (160 k rows), the goal in the middle, a
         field some 400 steps deep with a launch a sweep; descend_routes against plan_routes up to 1 024 starts
Every figure is the median of `--reps` calls, each between two HIP events on the stream (the call's host side included).  Prints one
JSON line.

    python3 tools/measure_route_field.py [--reps 10] [--maps site,s2,plane]
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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--maps", default="site,s2,plane")
    a = ap.parse_args()
    import torch
    import grid_ndt_amd as g
    from grid_ndt_amd import scenes
    from grid_ndt_amd._lib import ClearanceParams, RouteFieldParams
    from grid_ndt_amd.map2d import _stream_ptr
    assert torch.cuda.is_available(), "measure_route_field.py needs the GPU"
    stream = torch.cuda.current_stream()
    sp = _stream_ptr(None)
    T = g.TwoDmap

    def timed(fn, reps=None):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps or a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return round(float(np.median(ts)), 4), round(float(np.min(ts)), 4), round(float(np.max(ts)), 4)

    def build(cloud, P, hint):
        m = T(P["grid_len"], P["z_len"], max_nodes_hint=hint)
        m.setInterval(P["slope_interval"])
        m.setCloudFirst(cloud[0])
        m.create2DMap("slope", torch.from_numpy(np.ascontiguousarray(cloud[1:, :3])).cuda())
        return m, int(m.sync()[0])

    def field_case(m, n, goals, one_workgroup, hops=None, max_rounds=0, **rule):
        T.set_debug_option(T.DEBUG_ROUTE_FIELD_ONE_WORKGROUP, 1 if one_workgroup else 0)
        d_goals = torch.from_numpy(np.ascontiguousarray(goals, np.int32)).cuda()
        cost = torch.empty(max(n, 1), dtype=torch.float32, device="cuda")
        nxt = torch.empty(max(n, 1), dtype=torch.int32, device="cuda")
        counts = torch.zeros(8, dtype=torch.int32, device="cuda")
        prm = RouteFieldParams(0, rule.get("min_hops", 0), rule.get("soft_hops", 0), rule.get("soft_weight", 0.0), 0.0, max_rounds)

        def call():
            rc = m._L.gndt_route_field_device(m._h, None, C.byref(prm), C.c_void_p(d_goals.data_ptr()), len(goals), None,
                                              C.c_void_p(hops.data_ptr()) if hops is not None else None, C.c_void_p(cost.data_ptr()),
                                              C.c_void_p(nxt.data_ptr()), C.c_void_p(counts.data_ptr()), sp)
            assert rc == 0, m._L.gndt_last_error(m._h)
        med, lo, hi = timed(call)
        T.set_debug_option(T.DEBUG_ROUTE_FIELD_ONE_WORKGROUP, 1)
        c = [int(v) for v in counts.cpu()]
        return {"goals": len(goals), "one_workgroup": bool(one_workgroup and n <= 20448), "ms": med, "min_ms": lo, "max_ms": hi, "accepted": c[0],
                "finite": c[2], "max_cost": round(float(np.uint32(c[3]).view(np.float32)), 3), "converged": c[4], "sweeps": c[5],
                "us_per_sweep": round(1000.0 * med / max(c[5] + 1, 1), 3), "hops": hops is not None}, {"cost": cost[:n], "next": nxt[:n]}

    def clearance_case(m, n, max_hops):
        hops = torch.empty(max(n, 1), dtype=torch.int32, device="cuda")
        counts = torch.zeros(4, dtype=torch.int32, device="cuda")
        prm = ClearanceParams(1, max_hops)

        def call():
            rc = m._L.gndt_clearance_device(m._h, None, C.byref(prm), C.c_void_p(hops.data_ptr()), None, None, C.c_void_p(counts.data_ptr()), sp)
            assert rc == 0, m._L.gndt_last_error(m._h)
        med, lo, hi = timed(call)
        return {"max_hops": max_hops, "ms": med, "min_ms": lo, "max_ms": hi, "counts": [int(v) for v in counts.cpu()]}, hops[:n]

    def routes_case(m, starts, field, plan):
        out = []
        for K in (1, 16, 64, 256, 1024, 4096):
            if K > len(starts):
                break
            print(f"  routes K={K}", file=sys.stderr, flush=True)
            s = starts[:K].contiguous()
            rows, info = m.descend_routes(s, field, route_cap=256)
            row = {"K": K, "descend_ms": timed(lambda: m.descend_routes(s, field, route_cap=256))[0], "found": int((info["status"] == 0).sum()),
                   "longest": int(info["length"].max())}
            if K <= plan:
                prow, pinfo = m.plan_routes(s, start_mode="nearest_slope", route_cap=256)
                row.update(plan_ms=timed(lambda: m.plan_routes(s, start_mode="nearest_slope", route_cap=256), reps=max(a.reps // 2, 3))[0],
                           plan_found=int((pinfo["status"] == 0).sum()))
            out.append(row)
        return out

    def one_map(m, n, goal_xyz, wg_sizes, plan, max_rounds=0):
        out = {"rows": n}
        flood = timed(lambda: m.computeCost(goal_xyz))
        out["compute_cost_ms"] = flood[0]
        cl, hops = clearance_case(m, n, 32)
        out["clearance_32"] = cl
        goal = int(m.query(torch.tensor([goal_xyz], dtype=torch.float32, device="cuda"), "node")[0])
        fro = m.frontiers()
        many = np.asarray(fro["best_row"].cpu() if hasattr(fro["best_row"], "cpu") else fro["best_row"]).astype(np.int32)
        if len(many) < 2:                                          # (a map that ends nowhere inside the flood's reach)
            many = np.random.default_rng(1).choice(n, 16, replace=False).astype(np.int32)
        out["field"] = []
        field = None
        for goals, name in (([goal], "one goal"), (many, "frontier goals")):
            for wg in wg_sizes:
                print(f"  field {name} wg={wg}", file=sys.stderr, flush=True)
                row, fld = field_case(m, n, goals, wg, max_rounds=max_rounds)
                row["what"] = name
                out["field"].append(row)
                field = field if field is not None else fld
            row, _ = field_case(m, n, goals, wg_sizes[0], hops=hops, max_rounds=max_rounds, min_hops=1, soft_hops=3, soft_weight=0.5)
            row["what"] = name + ", clearance hops: min_hops 1, soft zone 3"
            out["field"].append(row)
        cells = m.export_device()
        slopes = torch.nonzero((cells["flags"][:n] & 2) != 0).flatten()
        pick = slopes[torch.from_numpy(np.random.default_rng(2).choice(len(slopes), min(4096, len(slopes)), replace=False)).cuda()]
        starts = cells["mean"][:n][pick].contiguous()
        out["routes"] = routes_case(m, starts, field, plan)
        return out

    out = {"tool": "measure_route_field", "device": g.device_info(0).get("name"), "source_hash": g._lib.source_hash()[:16], "reps": a.reps}
    maps = a.maps.split(",")
    if "site" in maps:
        cloud = scenes.drivable_site()
        m, n = build(cloud, scenes.COST_PARAMS, 0)
        out["site"] = one_map(m, n, scenes.DRIVABLE_GOAL, (True, False), plan=4096)
        # the middle third: a smaller map for the one-workgroup kernel
        cells = m.export()
        x0, x1 = int(cells["sx"].min()), int(cells["sx"].max())
        xm, w = (x0 + x1) // 2, (x1 - x0) // 6
        m.crop_box((xm - w, xm + w, -1000, 1000), "keep_inside")
        n = int(m.sync()[0])
        goal = int(m.query(torch.tensor([scenes.DRIVABLE_GOAL], dtype=torch.float32, device="cuda"), "nearest_slope")[0])
        out["site_middle"] = {"rows": n, "field": [field_case(m, n, [goal], wg)[0] for wg in (True, False)]}
    if "s2" in maps:
        cloud = scenes.uniform_box(a.points + 1)
        m, n = build(cloud, dict(grid_len=0.5, z_len=0.5, slope_interval=0.08), 1 << 20)
        cells = m.export()
        slope = np.flatnonzero((cells["flags"] & 2) != 0)
        goal_xyz = tuple(float(v) for v in cells["mean"][slope[np.argmin(np.abs(cells["mean"][slope, :2]).sum(1))]])
        out["s2"] = one_map(m, n, goal_xyz, (False,), plan=64, max_rounds=4096)
    if "plane" in maps:
        cloud = scenes.uniform_box(4_000_001)
        cloud[:, 2] = 0.25 + 0.02 * cloud[:, 2]                    # one level: 400 x 400 columns of one slope each, a field 400 steps deep
        cloud[0, 2] = 0.0
        m, n = build(cloud, dict(grid_len=0.5, z_len=0.5, slope_interval=0.08), 1 << 18)
        out["plane"] = one_map(m, n, (0.25, 0.25, 0.25), (False,), plan=1024)
    out["what"] = ("median of HIP-event intervals around single calls (host side of the call included); descend_ms and plan_ms include the "
                   "Python wrappers' output allocations")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
