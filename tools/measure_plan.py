#!/usr/bin/env python3
"""Route planning (gndt_plan_routes_device) next to the host planner on the same maps and starts: one process, one GPU.

  site      scenes.drivable_site() (400 k points, ~17 k rows), goal scenes.DRIVABLE_GOAL
  terrain   scenes.terrain_cloud(--points) (8 M points: more than 1 M rows), goal: a slope a third of the way through the rows
Per map: one call for K = 1, 64, 1024 and 16 384 traversable starts (drawn with a fixed seed from the slopes the flood reached), the
median of `--reps` calls between two HIP events on the stream (one more call first, not counted); the starts are on the device and the
routes stay there (route_cap 64: the timing is the search's, not a transfer's).  The terrain's queries take 16 bytes a row each, so its
calls are also timed with `--scratch-gib` of scratch instead of the default 256 MiB (fewer, fuller launches; K = 16 384 only so).  Then the expansions,
queue peaks and route lengths of the K = 1024 call, and the host planner — gndt_compat::AstarPlanar in the lazy mode, tools/plan_host.cpp,
a child process — on the first `--host-starts` of the same starts: the route alone, and the route plus the gndt_export_host it needs.
Prints one JSON line.

    python3 tools/measure_plan.py [--reps 5] [--points 8000000] [--host-starts 16] [--scratch-gib 16]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KS = (1, 64, 1024, 16384)


def build_host_tool():
    from grid_ndt_amd import _lib
    exe = os.path.join(ROOT, "tools", "plan_host")
    src = exe + ".cpp"
    deps = [src, os.path.join(ROOT, "include", "gndt_compat.hpp"), os.path.join(ROOT, "include", "gndt.h"), _lib.LIB_PATH]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        csrc, hip = os.path.dirname(_lib.LIB_PATH), _lib._hip_runtime_dir()
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
                               "-o", exe, src, "-L", csrc, "-l:libgndt.so", "-L", hip, "-l:libamdhip64.so", f"-Wl,-rpath,{csrc}", f"-Wl,-rpath,{hip}"])
    return exe


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--points", type=int, default=8_000_000)
    ap.add_argument("--host-starts", type=int, default=16)
    ap.add_argument("--scratch-gib", type=float, default=16.0)
    ap.add_argument("--maps", default="site,terrain")
    a = ap.parse_args()
    import torch
    import grid_ndt_amd as g
    from grid_ndt_amd import scenes
    assert torch.cuda.is_available(), "measure_plan.py needs the GPU"
    stream = torch.cuda.current_stream()
    exe = build_host_tool()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        stream.synchronize()
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    out = {"tool": "measure_plan", "source_hash": g._lib.source_hash()[:16], "reps": a.reps, "device": g.device_info(0)}

    def one(name, cloud, P, goal, radius, scratches):
        m = g.TwoDmap(P["grid_len"], P["z_len"])
        m.setInterval(P["slope_interval"])
        m.setCloudFirst(cloud[0])
        m.create2DMap("slope", torch.from_numpy(np.ascontiguousarray(cloud[1:, :3])).cuda())
        cells = m.export()
        if goal is None:
            rows = np.flatnonzero((cells["flags"] & 2) != 0)
            goal = cells["mean"][rows[len(rows) // 3]]
        st = m.computeCost(goal, dict(radius=radius))
        ce = m.cost_export()
        trav = np.flatnonzero(((cells["flags"] & 2) != 0) & (ce["state"] == 1))
        rng = np.random.default_rng(0x5EED0010)
        starts = np.ascontiguousarray(cells["mean"][rng.choice(trav, size=max(KS), replace=True)], np.float32)
        dev = torch.from_numpy(starts).cuda()
        rec = {"points": int(cloud.shape[0] - 1), "rows": int(cells["num_nodes"]), "slopes": int(cells["num_slopes"]),
               "traversable": int(len(trav)), "flood": {k: st[k] for k in ("rc", "levels", "traversable", "closed")}, "calls": {}}
        for label, scratch, most in scratches:
            for K in [k for k in KS if k <= most]:
                fn = lambda: m.plan_routes(dev[:K], route_cap=64, scratch_bytes=scratch)
                ms = [timed(fn) for _ in range(a.reps + 1)][1:]
                rec["calls"][f"K{K}{label}"] = {"ms_median": float(np.median(ms)), "ms": ms, "us_per_route": float(np.median(ms)) * 1e3 / K}
        rows, info = m.plan_routes(dev[:1024], route_cap=64, scratch_bytes=scratches[-1][1])
        info = {k: v.cpu().numpy() for k, v in info.items()}
        ok = info["status"] == 0
        rec["routes_of_1024"] = {"found": int(ok.sum()), "status_counts": np.bincount(info["status"], minlength=5).tolist(),
                                 "expansions_mean": float(info["expansions"][ok].mean()), "expansions_max": int(info["expansions"].max()),
                                 "queue_peak_max": int(info["queue_peak"].max()), "length_mean": float(info["length"][ok].mean()),
                                 "length_max": int(info["length"].max()),
                                 "expansions_per_route_slope": float(info["expansions"][ok].sum() / max(info["length"][ok].sum(), 1))}
        # the host planner on the first starts of the same list
        hk = min(a.host_starts, len(starts))
        with tempfile.NamedTemporaryFile(suffix=".f32") as fc, tempfile.NamedTemporaryFile(suffix=".f32") as fs:
            np.ascontiguousarray(cloud[:, :3], np.float32).tofile(fc.name)
            starts[:hk].tofile(fs.name)
            cmd = [exe, fc.name, str(cloud.shape[0]), str(P["grid_len"]), str(P["z_len"]), str(P["slope_interval"]), "slope"]
            cmd += [repr(float(v)) for v in goal] + [repr(float(radius)), fs.name, str(hk)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=1500)
        rec["host_planner_lazy"] = json.loads(r.stdout.strip().splitlines()[-1]) if r.returncode == 0 else {"error": r.stdout + r.stderr}
        dk = timed(lambda: m.plan_routes(dev[:hk], route_cap=64))
        rec["device_same_starts_ms"] = float(np.median([timed(lambda: m.plan_routes(dev[:hk], route_cap=64)) for _ in range(a.reps)]))
        rec["device_same_starts_first_call_ms"] = float(dk)
        out[name] = rec

    maps = a.maps.split(",")
    if "site" in maps:
        one("drivable_site_400k", scenes.drivable_site(), scenes.COST_PARAMS, scenes.DRIVABLE_GOAL, 0.25, [("", 0, max(KS))])
    if "terrain" in maps:
        one(f"terrain_{a.points // 1_000_000}M", scenes.terrain_cloud(a.points), scenes.TERRAIN_PARAMS, None, 0.25,
            [("", 0, 1024), ("_big_scratch", int(a.scratch_gib * (1 << 30)), max(KS))])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
