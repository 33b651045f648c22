#!/usr/bin/env python3
"""Path walks (gndt_walk_paths_device) on MI355X: one process per map, one GPU.

Maps (DESIGN.md §4.3m "Path walks"):
  s2        bench.py's S2 map (10 M uniform points in [-100,100)^2 x [-1,1), 0.5 m cells, 796 015 rows)
  corridor  tests/clearance_ref.corridor_cloud: a callback-sized map of 156 rows
  site      scenes.drivable_site(400_000) at COST_PARAMS (17.5 k rows of drivable ground: the walks run their whole length)
  terrain   scenes.terrain_cloud(2_000_000) at TERRAIN_PARAMS (1.2 M rows)
Workload per map: a fan of K unicycle arcs of T = 32 waypoints from one pose (rollouts.arcs), K from --ks (4096 and 64 by default), for
the flood's default robot and for a robot every gate lets through ("wide": the walks then run their whole length).  Per (robot, K):
  inline / table   one gndt_walk_paths_device call of each kernel variant, alternating call by call; median and spread of --reps HIP-event
                   intervals on the stream (the call's host side included) after --warmup calls of each
  query            yardstick 1, same process and map: one gndt_query_device NEAREST_SLOPE call of as many points as the walks stood on
                   slopes (the existing kernel with the same look-ups and no chain)
  host             yardstick 2: walk_path on one host core through the CPU tier's shim (tests/walk_shim.cpp) on the handle's export,
                   seconds over the paths of the call, per path (at most --host-paths of them)
Every map runs in a process of its own under its own time limit (`timeout`); the first that fails ends the run.  One JSON line a map.

    python3 tools/measure_walk.py [--reps 30] [--warmup 5] [--maps s2,corridor] [--ks 4096,64]
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

LIMITS = {"s2": 420, "corridor": 180, "site": 240, "terrain": 420}          # seconds a map's process may take
WIDE = dict(radius=0.25, reachable_height=10.0, max_rough=1e9, max_angle_deg=90.0)


def spread(ts):
    ts = sorted(ts)
    return {"median_us": round(1e3 * float(np.median(ts)), 2), "min_us": round(1e3 * ts[0], 2), "p90_us": round(1e3 * ts[int(0.9 * (len(ts) - 1))], 2),
            "max_us": round(1e3 * ts[-1], 2)}


def one_map(name, a):
    import torch
    import grid_ndt_amd as g
    from grid_ndt_amd import rollouts, scenes
    from grid_ndt_amd._lib import Robot, WalkParams
    from grid_ndt_amd.map2d import _stream_ptr
    assert torch.cuda.is_available(), "measure_walk.py needs the GPU"
    stream = torch.cuda.current_stream()
    sp = _stream_ptr(None)
    if name == "s2":
        cloud, P, pose = scenes.uniform_box(a.points + 1), dict(grid_len=0.5, z_len=0.5, slope_interval=0.08), (0.3, 0.2, 0.0, 0.3)
        m = g.TwoDmap(P["grid_len"], P["z_len"], max_nodes_hint=1 << 20)
    elif name in ("site", "terrain"):
        cloud, P = (scenes.drivable_site(400_000), scenes.COST_PARAMS) if name == "site" else (scenes.terrain_cloud(2_000_000), scenes.TERRAIN_PARAMS)
        mid = cloud[1 + int(np.argmin((cloud[1:, 0] - cloud[1:, 0].mean()) ** 2 + (cloud[1:, 1] - cloud[1:, 1].mean()) ** 2))]
        pose = (float(mid[0]), float(mid[1]), float(mid[2]), 0.3)          # on the ground in the middle of the cloud
        m = g.TwoDmap(P["grid_len"], P["z_len"])
    else:
        from tests import clearance_ref as cr
        cloud, P, pose = cr.corridor_cloud(), cr.CORRIDOR_P, (1.76, 0.3, 0.05, 1.45)
        m = g.TwoDmap(P["grid_len"], P["z_len"])
    m.setInterval(P["slope_interval"])
    m.setCloudFirst(cloud[0])
    m.create2DMap("slope", torch.from_numpy(np.ascontiguousarray(cloud[1:, :3])).cuda())
    rows, cols, slopes = m.sync()
    out = {"tool": "measure_walk", "map": name, "device": g.device_info(0).get("name"), "source_hash": g._lib.source_hash()[:16],
           "rows": rows, "columns": cols, "slopes": slopes, "reps": a.reps, "warmup": a.warmup, "T": a.T, "cases": {}}

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    host_table = None
    for rname, robot in (("default", None), ("wide", WIDE)):
        rb = None if robot is None else C.byref(Robot(robot["radius"], robot["reachable_height"], robot["max_rough"], robot["max_angle_deg"]))
        for K in [int(v) for v in a.ks.split(",")]:
            span = 0.25 if name == "corridor" else 1.2
            paths = rollouts.arcs(torch.tensor(pose, device="cuda"), a.speed, np.linspace(-span, span, K), a.dt, a.T).contiguous()
            raw = torch.zeros((K, 12), dtype=torch.int32, device="cuda")
            prm = WalkParams()

            def call(table):
                g.TwoDmap.set_debug_option(g.TwoDmap.DEBUG_WALK_STEP_TABLE, table)
                rc = m._L.gndt_walk_paths_device(m._h, C.c_void_p(paths.data_ptr()), K, a.T, 12, rb, C.byref(prm), None, None, 0,
                                                 C.c_void_p(raw.data_ptr()), sp)
                assert rc == 0, m._L.gndt_last_error(m._h)
            try:
                for _ in range(a.warmup):
                    call(0), call(1)
                torch.cuda.synchronize()
                ts = {0: [], 1: []}
                for _ in range(a.reps):                     # alternating: both variants see the same neighbours on the machine
                    for table in (0, 1):
                        ts[table].append(event_ms(lambda: call(table)))
                answers = []
                for table in (0, 1):
                    call(table)
                    torch.cuda.synchronize()
                    answers.append(raw.cpu().numpy().copy())
            finally:
                g.TwoDmap.set_debug_option(g.TwoDmap.DEBUG_WALK_STEP_TABLE, 2)
            assert answers[0].tobytes() == answers[1].tobytes(), "the two variants disagree"
            info = answers[0]
            status, steps = info[:, 0], info[:, 2].astype(np.int64)
            stood = int((steps + (status != 1)).sum())
            case = {"K": K, "slopes_stood_on": stood, "steps_max": int(steps.max()), "steps_mean": round(float(steps.mean()), 2),
                    "status_counts": {int(s): int((status == s).sum()) for s in np.unique(status)},
                    "inline": spread(ts[0]), "table": spread(ts[1])}
            # yardstick 1: as many NEAREST_SLOPE queries as slopes were stood on (points of the paths, cycled)
            pts = paths.reshape(-1, 3)[torch.arange(max(stood, 1), device="cuda") % (K * a.T)].contiguous()
            rws = torch.empty(len(pts), dtype=torch.int32, device="cuda")

            def query():
                rc = m._L.gndt_query_device(m._h, C.c_void_p(pts.data_ptr()), len(pts), 12, 1, C.c_void_p(rws.data_ptr()), None, None, sp)
                assert rc == 0
            for _ in range(a.warmup):
                query()
            torch.cuda.synchronize()
            case["query"] = dict(points=len(pts), **spread([event_ms(query) for _ in range(a.reps)]))
            # yardstick 2: the same paths through walk_path on one host core
            if a.host_paths:
                from tests import test_walk_host as H
                from tests import query_ref as qr
                if host_table is None:
                    c = m.export()
                    host_table = H.Table(c["sx"], c["sy"], c["sz"], c["flags"], qr.row_ncol(c), c["mean"], c["normal"], c["rough"])
                hp = paths.cpu().numpy()[np.linspace(0, K - 1, min(K, a.host_paths)).astype(np.int64)]
                H.run(host_table, cloud[0, :3], P["grid_len"], P["z_len"], hp[:1], False, robot=robot)       # (the shim loaded)
                best = None
                for _ in range(3):
                    t0 = time.perf_counter()
                    hinfo, _ = H.run(host_table, cloud[0, :3], P["grid_len"], P["z_len"], hp, False, robot=robot)
                    dt = time.perf_counter() - t0
                    best = dt if best is None else min(best, dt)
                case["host"] = {"paths": len(hp), "us_per_path": round(1e6 * best / len(hp), 2), "steps_mean": round(float(hinfo["steps"].mean()), 2)}
            out["cases"][f"{rname}_K{K}"] = case
    out["what"] = ("median / min / p90 / max of HIP-event intervals around single calls, host side of the call included; inline and table "
                   "alternate call by call; host: best of three wall-clock runs of the CPU tier's shim, call overhead included")
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--maps", default="s2,corridor")
    ap.add_argument("--ks", default="4096,64")
    ap.add_argument("--T", type=int, default=32)
    ap.add_argument("--speed", type=float, default=1.0)
    ap.add_argument("--dt", type=float, default=0.25)
    ap.add_argument("--host-paths", type=int, default=64, help="paths of a call the host yardstick walks (0: none)")
    ap.add_argument("--one-map", help="(internal) measure this map in this process")
    a = ap.parse_args()
    if a.one_map:
        one_map(a.one_map, a)
        return
    for name in a.maps.split(","):
        cmd = ["timeout", "-k", "10", str(LIMITS[name]), sys.executable, os.path.abspath(__file__), "--one-map", name] + \
              [x for k in ("reps", "warmup", "points", "ks", "T", "speed", "dt", "host_paths") for x in ("--" + k.replace("_", "-"), str(getattr(a, k)))]
        rc = subprocess.call(cmd)
        if rc != 0:
            sys.exit(f"measure_walk: map {name} ended with status {rc}; nothing more is started")


if __name__ == "__main__":
    main()
