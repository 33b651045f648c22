#!/usr/bin/env python3
"""Footprint poses (gndt_footprint_poses_device) on MI355X: one process per map, one GPU.

Maps (DESIGN.md §4.3o "Footprint poses"):
  site      scenes.drivable_site(400_000) at COST_PARAMS (17.5 k rows of drivable ground)
  corridor  tests/clearance_ref.corridor_cloud: a callback-sized map of 156 rows
  s2        bench.py's S2 map (10 M uniform points in [-100,100)^2 x [-1,1), 0.5 m cells, 796 015 rows)
Workload per map: K poses on the means of slopes drawn at random, random headings, K from --ks, for a 0.6 x 0.4 m and a 2.0 x 1.0 m
footprint.  Per (footprint, K):
  call    one gndt_footprint_poses_device call; median and spread of --reps HIP-event intervals on the stream (the call's host side
          included) after --warmup calls
  query   yardstick 1, same process and map: one gndt_query_device NEAREST_SLOPE call on the K x cells centres of the columns under the
          same poses' footprints (the look-ups alone, on code the footprints did not touch), alternating with `call` rep by rep
  host    yardstick 2: the per-pose code on one host core through the CPU tier's shim (tests/footprint_shim.cpp) on the handle's export,
          per pose (at most --host-poses of them)
  lanes   the share of the wavefront's lane slots that held a column under the vehicle: cells / (64 * ceil((2n + 1)^2 / 64))
Every map runs in a process of its own under its own time limit (`timeout`); the first that fails ends the run.  One JSON line a map.

    python3 tools/measure_footprint.py [--reps 30] [--warmup 5] [--maps site,corridor,s2] [--ks 64,4096,65536]
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

LIMITS = {"s2": 420, "corridor": 180, "site": 240}          # seconds a map's process may take
FOOTPRINTS = {"0.6x0.4": (0.3, 0.2), "2.0x1.0": (1.0, 0.5)}


def spread(ts):
    ts = sorted(ts)
    return {"median_us": round(1e3 * float(np.median(ts)), 2), "min_us": round(1e3 * ts[0], 2), "p90_us": round(1e3 * ts[int(0.9 * (len(ts) - 1))], 2),
            "max_us": round(1e3 * ts[-1], 2)}


def centres_under(poses, origin, grid_len, hl, hw, n):
    """the centres of the columns under every pose's footprint (include/gndt.h "footprint poses" 3 - 4), [M, 3] float32 with the pose's z"""
    from tests import query_ref as qr
    g = float(np.float32(grid_len))
    sx, sy, _, _, _ = qr.keys(poses[:, :3], origin, grid_len, 1.0)
    off = np.arange(-n, n + 1)
    lin = lambda s: np.where(s > 0, s - 1, s)
    idx = lambda l: np.where(l >= 0, l + 1, l)
    cen = lambda s, o: float(o) + np.where(s > 0, s - 0.5, s + 0.5) * g
    ax, ay = idx(lin(sx)[:, None] + off), idx(lin(sy)[:, None] + off)
    X = np.broadcast_to(cen(ax, origin[0])[:, None, :], (len(poses), 2 * n + 1, 2 * n + 1))
    Y = np.broadcast_to(cen(ay, origin[1])[:, :, None], X.shape)
    p = poses.astype(np.float64)
    dx, dy = X - p[:, 0, None, None], Y - p[:, 1, None, None]
    hx, hy = p[:, 3, None, None], p[:, 4, None, None]
    u, v, hh = dx * hx + dy * hy, dy * hx - dx * hy, hx * hx + hy * hy
    inside = (u * u <= hl * hl * hh) & (v * v <= hw * hw * hh)
    inside[:, n, n] = True
    Z = np.broadcast_to(p[:, 2, None, None], X.shape)
    return np.stack([X[inside], Y[inside], Z[inside]], 1).astype(np.float32)


def one_map(name, a):
    import torch
    import grid_ndt_amd as g
    from grid_ndt_amd import scenes
    from grid_ndt_amd._lib import FootprintParams
    from grid_ndt_amd.map2d import _stream_ptr
    from tests import footprint_cases as fc
    from tests import footprint_ref as fr
    assert torch.cuda.is_available(), "measure_footprint.py needs the GPU"
    stream = torch.cuda.current_stream()
    sp = _stream_ptr(None)
    if name == "s2":
        cloud, P = scenes.uniform_box(a.points + 1), dict(grid_len=0.5, z_len=0.5, slope_interval=0.08)
        m = g.TwoDmap(P["grid_len"], P["z_len"], max_nodes_hint=1 << 20)
    elif name == "site":
        cloud, P = scenes.drivable_site(400_000), scenes.COST_PARAMS
        m = g.TwoDmap(P["grid_len"], P["z_len"])
    else:
        from tests import clearance_ref as cr
        cloud, P = cr.corridor_cloud(), cr.CORRIDOR_P
        m = g.TwoDmap(P["grid_len"], P["z_len"])
    m.setInterval(P["slope_interval"])
    m.setCloudFirst(cloud[0])
    m.create2DMap("slope", torch.from_numpy(np.ascontiguousarray(cloud[1:, :3])).cuda())
    rows, cols, slopes = m.sync()
    cells = m.export()
    on = cells["mean"][(cells["flags"] & 2) != 0]
    out = {"tool": "measure_footprint", "map": name, "device": g.device_info(0).get("name"), "source_hash": g._lib.source_hash()[:16],
           "rows": rows, "columns": cols, "slopes": slopes, "reps": a.reps, "warmup": a.warmup, "cases": {}}

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    host_rows = None
    rng = np.random.default_rng(5)
    for fname, (hl, hw) in FOOTPRINTS.items():
        n = fr.box_n(hl, hw, P["grid_len"])
        for K in [int(v) for v in a.ks.split(",")]:
            poses = fc.headed(on[rng.integers(0, len(on), K)].astype(np.float64), rng.uniform(-np.pi, np.pi, K))
            d_poses = torch.from_numpy(poses).cuda()
            raw = torch.zeros((K, 16), dtype=torch.int32, device="cuda")
            prm = FootprintParams(hl, hw, 0.0, 0.0, 1)          # min_cells 1: the small footprint covers one or two 0.5 m cells

            def call():
                rc = m._L.gndt_footprint_poses_device(m._h, C.c_void_p(d_poses.data_ptr()), K, 20, None, C.byref(prm), None, 0,
                                                      C.c_void_p(raw.data_ptr()), sp)
                assert rc == 0, m._L.gndt_last_error(m._h)
            pts = torch.from_numpy(centres_under(poses, cloud[0, :3], P["grid_len"], float(np.float32(hl)), float(np.float32(hw)), n)).cuda()
            rws = torch.empty(len(pts), dtype=torch.int32, device="cuda")

            def query():
                rc = m._L.gndt_query_device(m._h, C.c_void_p(pts.data_ptr()), len(pts), 12, 1, C.c_void_p(rws.data_ptr()), None, None, sp)
                assert rc == 0
            for _ in range(a.warmup):
                call(), query()
            torch.cuda.synchronize()
            ts = {"call": [], "query": []}
            for _ in range(a.reps):                         # alternating: both see the same neighbours on the machine
                ts["call"].append(event_ms(call))
                ts["query"].append(event_ms(query))
            call()
            torch.cuda.synchronize()
            info = raw.cpu().numpy().view(np.uint32)
            status, cnt = info[:, 0], (info[:, 3] & 0xFFFF).astype(np.int64)
            assert int(cnt.sum()) == len(pts), (int(cnt.sum()), len(pts))       # the yardstick looks up the columns the call looked up
            slots = -(-(2 * n + 1) ** 2 // 64)
            case = {"K": K, "n": n, "cells_mean": round(float(cnt.mean()), 2), "support_mean": round(float((info[:, 3] >> 16).mean()), 2),
                    "lanes": round(float(cnt.mean()) / (64 * slots), 3), "status_counts": {int(s): int((status == s).sum()) for s in np.unique(status)},
                    "call": spread(ts["call"]), "query": dict(points=len(pts), **spread(ts["query"]))}
            case["call_over_query"] = round(case["call"]["median_us"] / case["query"]["median_us"], 2)
            if a.host_poses:
                if host_rows is None:
                    host_rows = fc.map_rows(cells, cloud[0, :3], P)
                hp = poses[:min(K, a.host_poses)]
                fc.run(host_rows, hp[:1], hl, hw, min_cells=1)                                 # (the shim loaded)
                best = None
                for _ in range(3):
                    t0 = time.perf_counter()
                    hinfo, _ = fc.run(host_rows, hp, hl, hw, min_cells=1)
                    dt = time.perf_counter() - t0
                    best = dt if best is None else min(best, dt)
                assert hinfo.tobytes() == info[:len(hp)].tobytes(), "the shim and the device disagree"
                case["host"] = {"poses": len(hp), "us_per_pose": round(1e6 * best / len(hp), 2)}
                case["host_core_over_call"] = round(case["host"]["us_per_pose"] * K / case["call"]["median_us"], 1)
            out["cases"][f"{fname}_K{K}"] = case
    out["what"] = ("median / min / p90 / max of HIP-event intervals around single calls, host side of the call included; call and query "
                   "alternate rep by rep; host: best of three wall-clock runs of the CPU tier's shim, call overhead included, scaled to K")
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--maps", default="site,corridor,s2")
    ap.add_argument("--ks", default="64,4096,65536")
    ap.add_argument("--host-poses", type=int, default=4096, help="poses of a call the host yardstick evaluates (0: none)")
    ap.add_argument("--one-map", help="(internal) measure this map in this process")
    a = ap.parse_args()
    if a.one_map:
        one_map(a.one_map, a)
        return
    for name in a.maps.split(","):
        cmd = ["timeout", "-k", "10", str(LIMITS[name]), sys.executable, os.path.abspath(__file__), "--one-map", name] + \
              [x for k in ("reps", "warmup", "points", "ks", "host_poses") for x in ("--" + k.replace("_", "-"), str(getattr(a, k)))]
        rc = subprocess.call(cmd)
        if rc != 0:
            sys.exit(f"measure_footprint: map {name} ended with status {rc}; nothing more is started")


if __name__ == "__main__":
    main()
