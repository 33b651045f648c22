#!/usr/bin/env python3
"""Surface patches (gndt_patches_device) next to frontier extraction (gndt_frontiers_device, candidates "slopes") on the same map — both
are a union-find plus a rank over the rows, so the frontiers call is the yardstick for everything but the probes and the moments — and
the moment pass on one plane against many patches: one process, one GPU.

  s2       bench.py's S2 map (10 M uniform points in [-100,100)^2 x [-1,1), 0.5 m cells, 796 k rows)
  site     the 17 k-row drivable site's map (scenes.drivable_site, COST_PARAMS)
  terrain  scenes.terrain_cloud(2 M) at TERRAIN_PARAMS (381 k rows)
For each: rows, candidates, patches, the largest patch, the patches call (its list sized to every patch) and its count-only call, the
frontiers call and its count-only call.
  plane    a flat floor of 896 x 896 cells (802 816 rows, 0.5 m cells, the frontier tests' ripple): ONE patch
  cut      the same floor in tiles of 9 x 9 cells at four heights 7 cm apart, coloured so that no two touching tiles share one, with
           max_offset 5 cm: about 10 k patches
For both: the call with and without the moment pass's LDS stage (GNDT_DEBUG_PATCH_LDS), the count-only call (mark, link, flatten,
count, scan) and their difference (rank, reduce, moments, fit).  plane_over_cut of those differences says whether the pre-combining
works.  The moment kernel's own time: run the tool under `rocprofv3 --kernel-trace --stats` in a run of its own (--maps plane,cut).
Every figure is the median (min, max) of `--reps` calls between two HIP events on the stream after `--warmup` calls.  Prints one JSON
line.

    python3 tools/measure_patches.py [--reps 10] [--warmup 2] [--maps s2,site,terrain,plane,cut] [--points 10000000]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GL, ZL = 0.5, 0.25
SIDE, TILE = 896, 9
HEIGHTS = (0.03, 0.10, 0.17, 0.24)


def floor_cloud(cut):
    """SIDE x SIDE cells of 3 x 3 points with a 2 mm ripple; cut: tiles of TILE x TILE cells at HEIGHTS[(tx % 2) + 2 (ty % 2)]"""
    ix, iy = np.divmod(np.arange(SIDE * SIDE, dtype=np.int64), SIDE)
    ab = np.array([0.12, 0.25, 0.38])
    x = np.broadcast_to((ix * GL)[:, None, None] + ab[None, :, None], (len(ix), 3, 3))
    y = np.broadcast_to((iy * GL)[:, None, None] + ab[None, None, :], (len(ix), 3, 3))
    base = np.asarray(HEIGHTS)[((ix // TILE) % 2) + 2 * ((iy // TILE) % 2)] if cut else np.full(len(ix), HEIGHTS[1])
    z = base[:, None, None] + 0.002 * np.sin(7 * x) * np.cos(5 * y)
    pts = np.empty((1 + 9 * len(ix), 3), np.float32)
    pts[0] = (0.0, 0.0, 0.0)
    pts[1:, 0], pts[1:, 1], pts[1:, 2] = x.reshape(-1), y.reshape(-1), z.reshape(-1)
    return pts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--maps", default="s2,site,terrain,plane,cut")
    a = ap.parse_args()
    import torch
    import grid_ndt_amd as g
    from grid_ndt_amd import scenes
    assert torch.cuda.is_available(), "measure_patches.py needs the GPU"
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

    def patch_times(m, row, **kw):
        p = m.patches(**kw)
        counts = [int(v) for v in p["counts"].tolist()]
        K = counts[0]
        row.update(candidates=counts[1], patches=counts[2], largest=int(p["nodes"].max().item()) if K else 0,
                   kinds={name: int(((p["kind"] & bit) != 0).sum().item()) for name, bit in (("horizontal", 1), ("vertical", 2), ("inclined", 4))})
        row["patches_ms"] = timed(lambda: m.patches(max_patches=K, **kw))
        row["patches_count_only_ms"] = timed(lambda: m.patches(max_patches=0, **kw))
        row["list_passes_ms"] = round(row["patches_ms"][0] - row["patches_count_only_ms"][0], 4)
        return K

    out = {"tool": "measure_patches", "device": g.device_info(0).get("name"), "source_hash": g._lib.source_hash()[:16], "reps": a.reps}
    maps = a.maps.split(",")
    for name in ("s2", "site", "terrain"):
        if name not in maps:
            continue
        print(f"  {name}", file=sys.stderr, flush=True)
        if name == "s2":
            cloud, P, hint = scenes.uniform_box(a.points + 1), dict(grid_len=0.5, z_len=0.5, slope_interval=0.08), 1 << 20
        elif name == "site":
            cloud, P, hint = scenes.drivable_site(), scenes.COST_PARAMS, 0
        else:
            cloud, P, hint = scenes.terrain_cloud(2_000_000), scenes.TERRAIN_PARAMS, 1 << 19
        m, n = build(cloud, P, hint)
        row = {"rows": n}
        patch_times(m, row, candidates="slopes")
        f = m.frontiers("slopes")
        row["frontier_clusters"] = int(f["counts"][0].item())
        row["frontiers_ms"] = timed(lambda: m.frontiers("slopes", max_clusters=row["frontier_clusters"]))
        row["frontiers_count_only_ms"] = timed(lambda: m.frontiers("slopes", max_clusters=0))
        row["patches_over_frontiers"] = round(row["patches_ms"][0] / row["frontiers_ms"][0], 2)
        out[name] = row
        del m
    floors = {}
    for name in ("plane", "cut"):
        if name not in maps:
            continue
        print(f"  {name}", file=sys.stderr, flush=True)
        m, n = build(floor_cloud(name == "cut"), dict(grid_len=GL, z_len=ZL, slope_interval=0.08), 1 << 20)
        row = {"rows": n}
        for lds in (1, 0):
            T.set_debug_option(T.DEBUG_PATCH_LDS, lds)
            sub = {}
            patch_times(m, sub, max_offset=0.05)
            row["lds" if lds else "no_lds"] = sub
        T.set_debug_option(T.DEBUG_PATCH_LDS, 1)
        floors[name] = out[name] = row
        del m
    if len(floors) == 2:
        out["plane_over_cut_list_passes"] = {k: round(floors["plane"][k]["list_passes_ms"] / max(floors["cut"][k]["list_passes_ms"], 1e-6), 2)
                                             for k in ("lds", "no_lds")}
    out["what"] = ("ms: [median, min, max] of HIP-event intervals around single calls (the Python wrapper's output allocations included); "
                   "list_passes_ms: the call's median minus its count-only call's (rank, reduce, moments, fit)")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
