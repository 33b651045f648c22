#!/usr/bin/env python3
"""View gain (gndt_view_gain_device) next to one ray cast (gndt_cast_rays_device, VOXEL) of the same K x N rays: one process, one GPU.

  site   the 17 k-row drivable site's map (scenes.drivable_site, COST_PARAMS, 0.5 m cells)
  s2     bench.py's S2 map (10 M uniform points in [-100,100)^2 x [-1,1), 0.5 m cells, 796 k rows)
On each, at a 30 m range (reach 61, a window of 123 x 123 columns, 4.7 KiB of LDS a workgroup):
  416 x 1024   on the site the poses of frontier_views (every frontiers() cluster's best slope x 8 yaws, cycled to 416); on s2, and for
  64 x 4096    the other batches, poses 1 m over random slopes with random yaws.  Fans: a full turn, +-15 degrees of elevation
  4096 x 64    (128 x 8, 256 x 16 and 32 x 2 rays).
For each: the call's time, `steps` (column visits, from the records) per microsecond, the cast of the same rays (ends formed by the
documented fp64 expression, per-ray origins) — the same walks without the set —, and the time at 64 .. 1024 threads a workgroup
(GNDT_DEBUG_VIEW_THREADS).
  windows  on the site's map with every pose lifted far above it (nothing stops a ray, so steps are the same whatever the window
           marks): 256 poses, the smallest window (a range of one cell: reach 2) with many rays, and the largest (reach 403) with
           64, the rays of the first sized to about equal steps.
Every figure is the median (min, max) of `--reps` calls between two HIP events on the stream after `--warmup` calls.  Kernel times:
run it under `rocprofv3 --kernel-trace --stats` in a run of its own.  Prints one JSON line.

    python3 tools/measure_view.py [--reps 10] [--warmup 2] [--maps site,s2] [--points 10000000]
"""
import argparse
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
    ap.add_argument("--maps", default="site,s2")
    ap.add_argument("--range", type=float, default=30.0)
    a = ap.parse_args()
    import torch
    import grid_ndt_amd as g
    from grid_ndt_amd import rollouts, scenes
    assert torch.cuda.is_available(), "measure_view.py needs the GPU"
    stream = torch.cuda.current_stream()
    T = g.TwoDmap

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return [round(float(np.median(ts)), 4), round(float(np.min(ts)), 4), round(float(np.max(ts)), 4)]

    def build(cloud, P, hint):
        m = T(P["grid_len"], P["z_len"], max_nodes_hint=hint)
        m.setInterval(P["slope_interval"])
        m.setCloudFirst(cloud[0])
        m.create2DMap("slope", torch.from_numpy(np.ascontiguousarray(cloud[1:, :3])).cuda())
        return m, int(m.sync()[0])

    def random_poses(m, n, K, seed):
        """1 m over the means of K random slopes, random yaws -> float64 [K, 12] on the device"""
        cells = m.export_device()
        slopes = torch.nonzero((cells["flags"][:n] & 2) != 0).flatten()
        rng = np.random.default_rng(seed)
        t = cells["mean"][:n][slopes[torch.from_numpy(rng.integers(0, len(slopes), K)).cuda()]].double()
        yaw = torch.from_numpy(rng.uniform(0, 2 * np.pi, K)).cuda()
        c, s, z, o = torch.cos(yaw), torch.sin(yaw), torch.zeros_like(yaw), torch.ones_like(yaw)
        return torch.stack([c, -s, z, t[:, 0], s, c, z, t[:, 1], z, z, o, t[:, 2] + 1.0], 1).contiguous()

    def case(m, poses, dirs, R, threads=(64, 128, 256, 512, 1024)):
        K, N = int(poses.shape[0]), int(dirs.shape[0])
        d = torch.from_numpy(dirs).cuda()
        out = m.view_gain(poses, d, R)
        steps = int(out["steps"].sum().item())
        row = {"K": K, "N": N, "range": R, "reach": int(np.ceil(np.float32(R) / np.float32(m.gridLen))) + 1, "steps": steps, "unknown_mean": round(float(out["unknown"].double().mean().item()), 1),
               "known_mean": round(float(out["known"].double().mean().item()), 1),
               "hit_share": round(float(out["hits"].sum().item()) / max(int(out["rays"].sum().item()), 1), 3)}
        row["view_ms"] = timed(lambda: m.view_gain(poses, d, R))
        row["view_per_ray_ms"] = timed(lambda: m.view_gain(poses, d, R, per_ray=True))
        row["steps_per_us"] = round(steps / (1000.0 * row["view_ms"][0]), 1)
        # the cast of the same rays: ends by the documented expression, one origin per ray
        P3 = poses.reshape(K, 3, 4)
        dd = d.double()
        ends = (P3[:, None, :, 3] + float(np.float32(R)) * ((P3[:, None, :, 0] * dd[None, :, 0, None] + P3[:, None, :, 1] * dd[None, :, 1, None])
                                                             + P3[:, None, :, 2] * dd[None, :, 2, None])).float().reshape(K * N, 3).contiguous()
        origins = P3[:, None, :, 3].float().expand(K, N, 3).reshape(K * N, 3).contiguous()
        row["cast_ms"] = timed(lambda: m.cast_rays(origins, ends, mode="voxel", max_range=R))
        row["view_over_cast"] = round(row["view_ms"][0] / row["cast_ms"][0], 2)
        row["by_threads_ms"] = {}
        for t in threads:
            T.set_debug_option(T.DEBUG_VIEW_THREADS, t)
            row["by_threads_ms"][str(t)] = timed(lambda: m.view_gain(poses, d, R))[0]
        T.set_debug_option(T.DEBUG_VIEW_THREADS, 1024)
        return row

    def one_map(m, n, first_poses):
        fans = {1024: rollouts.view_directions(2 * np.pi, np.deg2rad(30.0), 128, 8), 4096: rollouts.view_directions(2 * np.pi, np.deg2rad(30.0), 256, 16),
                64: rollouts.view_directions(2 * np.pi, np.deg2rad(30.0), 32, 2)}
        out = {"rows": n, "cases": []}
        for K, N, poses in ((416, 1024, first_poses), (64, 4096, None), (4096, 64, None)):
            print(f"  {K} x {N}", file=sys.stderr, flush=True)
            out["cases"].append(case(m, poses if poses is not None else random_poses(m, n, K, K), fans[N], a.range))
        return out

    out = {"tool": "measure_view", "device": g.device_info(0).get("name"), "source_hash": g._lib.source_hash()[:16], "reps": a.reps}
    maps = a.maps.split(",")
    if "site" in maps:
        cloud = scenes.drivable_site()
        m, n = build(cloud, scenes.COST_PARAMS, 0)
        assert m.computeCost(scenes.DRIVABLE_GOAL, dict(radius=0.25))["rc"] == 0
        fr = m.frontiers()
        views = m.frontier_views(fr, yaws=8, height=1.0)
        out["site_clusters"] = int(fr["size"].shape[0])
        out["site"] = one_map(m, n, views[torch.arange(416, device=views.device) % views.shape[0]].contiguous())
        # the windows at equal steps: every pose far above the map, so that no ray is stopped
        g_len = scenes.COST_PARAMS["grid_len"]
        poses = random_poses(m, n, 256, 7)
        poses[:, 11] += 1000.0
        flat = lambda k: rollouts.view_directions(2 * np.pi, 0.0, k, 1)
        large = case(m, poses, flat(64), 402.0 * g_len, threads=())
        small_n = max(64, int(round(large["steps"] / 256 / 2.3 / 64.0)) * 64)
        small = case(m, poses, flat(small_n), 1.0 * g_len, threads=())
        out["windows"] = {"largest": large, "smallest": small}
    if "s2" in maps:
        cloud = scenes.uniform_box(a.points + 1)
        m, n = build(cloud, dict(grid_len=0.5, z_len=0.5, slope_interval=0.08), 1 << 20)
        out["s2"] = one_map(m, n, random_poses(m, n, 416, 416))
    out["what"] = ("ms: [median, min, max] of HIP-event intervals around single calls (the Python wrapper's output allocations included); "
                   "steps_per_us from the median; view_over_cast: view_ms over cast_ms, the same walks without the set")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
