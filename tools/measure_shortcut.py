#!/usr/bin/env python3
"""Route shortcutting (gndt_shortcut_routes_device) on MI355X: one process per map, one GPU.

Maps (DESIGN.md §4.3n "Route shortcutting"):
  site      scenes.drivable_site(400_000) at COST_PARAMS (17.5 k rows of drivable ground), goal scenes.DRIVABLE_GOAL, the flood's default
            robot: 1 024 plan_routes routes from random traversable starts
  terrain   scenes.terrain_cloud(2_000_000) at TERRAIN_PARAMS (381 k rows), a robot every gate lets through, goal a slope a third of the
            way through the rows: --terrain-routes long routes (route_cap 2048)
Per map:
  plan      the plan_routes call that produced the routes (median of --plan-reps HIP-event intervals)
  device    one gndt_shortcut_routes_device call over all routes, lengths read out of the plan's info (stride 32), with and without
            path_rows: median and spread of --reps HIP-event intervals on the stream (the call's host side included) after --warmup calls
  composed  yardstick 1, same process and map: the same answer from walk_paths calls in Python, one call per anchor round over all
            routes with K * window two-waypoint paths made on the device each round — what a user does without the feature.  Wall clock
            of the whole loop (best of three), its rounds, and how many routes end with other waypoints than the device call's (a start
            lookup that finds another storey than the anchor's)
  host      yardstick 2: shortcut_route on one host core through the CPU tier's shim (tests/shortcut_shim.cpp) on the handle's export,
            per route (at most --host-routes of them)
and waypoints in and out, links_tested a route, the longest anchor chain.  Every map runs in a process of its own under its own time
limit (`timeout`); the first that fails ends the run.  One JSON line a map.

    python3 tools/measure_shortcut.py [--reps 30] [--warmup 5] [--maps site,terrain]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIMITS = {"site": 240, "terrain": 420}          # seconds a map's process may take
WIDE = dict(radius=0.25, reachable_height=10.0, max_rough=1e9, max_angle_deg=90.0)


def spread(ts):
    ts = sorted(ts)
    return {"median_us": round(1e3 * float(np.median(ts)), 2), "min_us": round(1e3 * ts[0], 2), "p90_us": round(1e3 * ts[int(0.9 * (len(ts) - 1))], 2),
            "max_us": round(1e3 * ts[-1], 2)}


def one_map(name, a):
    import torch
    import grid_ndt_amd as g
    from grid_ndt_amd import scenes
    from grid_ndt_amd._lib import Robot, ShortcutParams
    from grid_ndt_amd.map2d import _stream_ptr
    assert torch.cuda.is_available(), "measure_shortcut.py needs the GPU"
    stream = torch.cuda.current_stream()
    sp = _stream_ptr(None)
    if name == "site":
        cloud, P, goal, robot, K, cap = scenes.drivable_site(400_000), scenes.COST_PARAMS, scenes.DRIVABLE_GOAL, None, 1024, 512
    else:
        cloud, P, goal, robot, K, cap = scenes.terrain_cloud(2_000_000), scenes.TERRAIN_PARAMS, None, WIDE, a.terrain_routes, 2048
    m = g.TwoDmap(P["grid_len"], P["z_len"])
    m.setInterval(P["slope_interval"])
    m.setCloudFirst(cloud[0])
    m.create2DMap("slope", torch.from_numpy(np.ascontiguousarray(cloud[1:, :3])).cuda())
    cells = m.export()
    if goal is None:
        slopes = np.flatnonzero((cells["flags"] & 2) != 0)
        goal = cells["mean"][slopes[len(slopes) // 3]]
    st = m.computeCost(tuple(float(v) for v in goal), robot)
    ce = m.cost_export()
    trav = np.flatnonzero(((cells["flags"] & 2) != 0) & (ce["state"] == 1))
    rng = np.random.default_rng(0x5EED0020)
    pick = rng.choice(trav, size=K, replace=True) if name == "site" else trav[np.argsort(ce["h"][trav])[-K:]]       # terrain: the farthest
    starts = torch.from_numpy(np.ascontiguousarray(cells["mean"][pick], np.float32)).cuda()
    window = a.window

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    plan = lambda: m.plan_routes(starts, route_cap=cap, scratch_bytes=int(a.scratch_gib * (1 << 30)))
    plan()
    torch.cuda.synchronize()
    plan_ms = [event_ms(plan) for _ in range(a.plan_reps)]
    rows, pinfo = plan()
    torch.cuda.synchronize()
    found = (pinfo["status"] == 0) & (pinfo["length"] <= cap)
    out = {"tool": "measure_shortcut", "map": name, "gpu": g.device_info(0).get("name"), "source_hash": g._lib.source_hash()[:16],
           "rows": int(cells["num_nodes"]), "slopes": int(cells["num_slopes"]), "flood_rc": st["rc"], "routes": K, "route_cap": cap, "window": window,
           "routes_found": int(found.sum()), "reps": a.reps, "warmup": a.warmup, "plan": dict(reps=a.plan_reps, **spread(plan_ms))}
    # routes without an answer take part as empty routes
    raw_info = pinfo["length"]                             # a view into the plan's records: 32 bytes apart
    raw_info[~found] = 0
    rb = None if robot is None else C.byref(Robot(robot["radius"], robot["reachable_height"], robot["max_rough"], robot["max_angle_deg"]))
    prm = ShortcutParams(window, 0, 0, 0)
    info = torch.zeros((K, 12), dtype=torch.int32, device="cuda")
    wp = torch.empty((K, cap), dtype=torch.int32, device="cuda")
    path = torch.empty((K, 2 * cap), dtype=torch.int32, device="cuda")

    def call(with_path):
        rc = m._L.gndt_shortcut_routes_device(m._h, C.c_void_p(rows.data_ptr()), K, cap, C.c_void_p(raw_info.data_ptr()), 32, rb, C.byref(prm), None,
                                              C.c_void_p(wp.data_ptr()), cap, C.c_void_p(path.data_ptr()) if with_path else None,
                                              2 * cap if with_path else 0, C.c_void_p(info.data_ptr()), sp)
        assert rc == 0, m._L.gndt_last_error(m._h)
    for _ in range(a.warmup):
        call(False), call(True)
    torch.cuda.synchronize()
    ts = {False: [], True: []}
    for _ in range(a.reps):
        for with_path in (False, True):
            ts[with_path].append(event_ms(lambda: call(with_path)))
    call(True)
    torch.cuda.synchronize()
    I = info.cpu().numpy()
    status, length_in, waypoints, path_slopes, tested, fallback = (I[:, i].astype(np.int64) for i in range(6))
    live = length_in > 0
    out["device"] = {"waypoints_only": spread(ts[False]), "with_path_rows": spread(ts[True]),
                     "status_counts": {int(s): int((status == s).sum()) for s in np.unique(status)},
                     "rows_in": int(length_in.sum()), "waypoints_out": int(waypoints.sum()), "length_in_mean": round(float(length_in[live].mean()), 1),
                     "length_in_max": int(length_in.max()), "waypoints_mean": round(float(waypoints[live].mean()), 2),
                     "links_tested_mean": round(float(tested[live].mean()), 1), "links_tested_max": int(tested.max()),
                     "fallback_links": int(fallback.sum()), "longest_anchor_chain": int((waypoints - 1).max()),
                     "cost_out_over_cost_in": round(float(I[:, 7].view(np.float32)[live].sum() / max(I[:, 6].view(np.float32)[live].sum(), 1e-9)), 4)}
    # yardstick 1: the same answer from walk_paths calls, one per anchor round
    dev_cells = m.export_device()
    n_t = raw_info.long()
    R = rows.long().clamp(min=0)
    ar = torch.arange(window, device="cuda")[None, :] + 1

    def composed():
        anchor = torch.zeros(K, dtype=torch.long, device="cuda")
        wps = [R[:, 0]]
        rounds = 0
        while bool((anchor + 1 < n_t).any()):
            j = anchor[:, None] + ar                                     # [K, window]
            valid = j <= (n_t[:, None] - 1)
            ra = R.gather(1, anchor[:, None]).expand(-1, window)
            rbw = R.gather(1, j.clamp(max=cap - 1))
            pts = m.route_waypoints(torch.stack([ra, rbw], 2).reshape(-1, 2).int())
            pts[:, 1, 2] = pts[:, 0, 2]
            pts[~valid.reshape(-1), 0, 0] = float("nan")
            got = m.walk_paths(pts, robot=robot)
            holds = ((got["status"] == 0) & (got["end_row"] == rbw.reshape(-1).int()) & (got["start_row"] == ra.reshape(-1).int())).reshape(K, window) & valid
            far = (holds * ar).max(1).values                             # the largest candidate that holds; 0: none
            moving = anchor + 1 < n_t
            anchor = torch.where(moving, anchor + far.clamp(min=1), anchor)
            wps.append(torch.where(moving, R.gather(1, anchor[:, None])[:, 0], torch.full_like(anchor, -1)))
            rounds += 1
        return torch.stack(wps, 1), rounds
    composed()
    torch.cuda.synchronize()
    best = None
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        cw, rounds = composed()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    counts = (cw >= 0).sum(1).cpu().numpy() * live
    out["composed"] = {"ms": round(1e3 * best, 2), "rounds": rounds, "walk_paths_per_round": K * window,
                       "routes_with_other_waypoint_counts": int((counts != waypoints * live).sum()),
                       "over_device_with_path": round(1e3 * best / (1e-3 * out["device"]["with_path_rows"]["median_us"]), 1),
                       "over_device_waypoints_only": round(1e3 * best / (1e-3 * out["device"]["waypoints_only"]["median_us"]), 1)}
    del dev_cells
    # yardstick 2: the same routes through shortcut_route on one host core
    if a.host_routes:
        from tests import query_ref as qr
        from tests import test_shortcut_host as H
        from tests.test_clearance_host import Table
        t = Table(cells["sx"], cells["sy"], cells["sz"], cells["flags"], qr.row_ncol(cells), cells["mean"], cells["normal"], cells["rough"])
        sel = np.flatnonzero(live)[np.linspace(0, int(live.sum()) - 1, min(int(live.sum()), a.host_routes)).astype(np.int64)]
        hr, hl = rows.cpu().numpy().view(np.uint32)[sel], length_in[sel].astype(np.uint32)
        H.run(t, cloud[0, :3], P["grid_len"], P["z_len"], hr[:1], hl[:1], robot=robot, window=window)              # (the shim loaded)
        best = None
        for _ in range(3):
            t0 = time.perf_counter()
            hinfo, hwp, _ = H.run(t, cloud[0, :3], P["grid_len"], P["z_len"], hr, hl, robot=robot, window=window, path_cap=2 * cap)
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        same = bool(np.array_equal(hwp.view(np.int32), wp.cpu().numpy()[sel]) and np.array_equal(hinfo["links_tested"], tested[sel]))
        out["host"] = {"routes": len(sel), "us_per_route": round(1e6 * best / len(sel), 1), "same_answer_as_device": same,
                       "over_device_per_route": round(1e6 * best / len(sel) / (out["device"]["with_path_rows"]["median_us"] / K), 1)}
    out["what"] = ("median / min / p90 / max of HIP-event intervals around single calls, host side of the call included; composed and host: "
                   "best of three wall-clock runs")
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--plan-reps", type=int, default=5)
    ap.add_argument("--maps", default="site,terrain")
    ap.add_argument("--window", type=int, default=64)
    ap.add_argument("--terrain-routes", type=int, default=256)
    ap.add_argument("--scratch-gib", type=float, default=8.0)
    ap.add_argument("--host-routes", type=int, default=64, help="routes of a call the host yardstick answers (0: none)")
    ap.add_argument("--one-map", help="(internal) measure this map in this process")
    a = ap.parse_args()
    if a.one_map:
        one_map(a.one_map, a)
        return
    for name in a.maps.split(","):
        cmd = ["timeout", "-k", "10", str(LIMITS[name]), sys.executable, os.path.abspath(__file__), "--one-map", name] + \
              [x for k in ("reps", "warmup", "plan_reps", "window", "terrain_routes", "scratch_gib", "host_routes")
               for x in ("--" + k.replace("_", "-"), str(getattr(a, k)))]
        rc = subprocess.call(cmd)
        if rc != 0:
            sys.exit(f"measure_shortcut: map {name} ended with status {rc}; nothing more is started")


if __name__ == "__main__":
    main()
