#!/usr/bin/env python3
"""The obstacle field (gndt_obstacle_field_device) on MI355X: one process, one GPU.

Workloads (DESIGN.md §4.3q "Obstacle field"):
  site   the 17 k-row drivable site's map (scenes.drivable_site, COST_PARAMS) with tools/measure_segment.py's frame: 131 072 points of
         the site's own surface and four boxes that were not there when the map was made.  The field alone on the four boxes' index
         bounds at max_hops 4 / 8 / 32, gndt_clearance_device at the same max_hops on the same map (the yardstick), and the chain
         segment_scan -> obstacle_field (on the records and their count, where they lie) -> walk_paths of 4 096 arcs of 8 waypoints
  s2     bench.py's S2 map (10 M uniform points in [-100,100)^2 x [-1,1), 0.5 m cells, 796 k rows): the same four world boxes, the
         same three max_hops, the clearance call; then 1, 16, 256, 4 096 and 65 536 one-cell boxes on random columns and one zone of
         500 x 500 columns, at max_hops 8
Every figure is the median of `--reps` calls, each between two HIP events on the stream (the call's host side included); with each
field its counts and the mark pass's tallies (gndt_debug_obstacle_marks: window columns, worklist rows, probes that found a column,
columns listed, minima sent), from which atomics per covered row and probes per column follow.  The bytes of the final fill (8 a row:
hops and obstacle written, no base) are reported beside the time so that the two maps' difference can be set against them.  Prints one
JSON line.

    python3 tools/measure_obstacle.py [--reps 20] [--maps site,s2]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORLD_BOXES = (((-6.0, -6.0, 0.9), (-4.2, -5.2, 2.5)), ((2.0, 3.0, 1.0), (2.9, 3.4, 1.7)), ((9.0, -14.0, 0.8), (13.0, -12.5, 2.4)),
               ((-15.0, 10.0, 1.0), (-14.2, 10.8, 2.8)))            # tools/measure_segment.py site_frame's four boxes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--maps", default="site,s2")
    a = ap.parse_args()
    import torch
    import grid_ndt_amd as g
    from grid_ndt_amd import scenes
    from grid_ndt_amd._lib import ClearanceParams, ObstacleParams
    from grid_ndt_amd.map2d import _stream_ptr
    from tools.measure_segment import site_frame
    assert torch.cuda.is_available(), "measure_obstacle.py needs the GPU"
    stream = torch.cuda.current_stream()
    sp = _stream_ptr(None)
    T = g.TwoDmap
    T.set_debug_option(T.DEBUG_OBSTACLE_TALLY, 1)          # the marking pass's tallies: part of what is timed here, off in the product

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
        return round(float(np.median(ts)), 4), round(float(np.min(ts)), 4), round(float(np.max(ts)), 4)

    def build(cloud, P, hint):
        m = T(P["grid_len"], P["z_len"], max_nodes_hint=hint)
        m.setInterval(P["slope_interval"])
        m.setCloudFirst(cloud[0])
        m.create2DMap("slope", torch.from_numpy(np.ascontiguousarray(cloud[1:, :3])).cuda())
        return m, int(m.sync()[0])

    def field_case(m, n, boxes, max_hops, levels_above=4):
        d_boxes = torch.from_numpy(np.ascontiguousarray(boxes, np.int32)).cuda()
        hops = torch.empty(max(n, 1), dtype=torch.int32, device="cuda")
        owner = torch.empty(max(n, 1), dtype=torch.int32, device="cuda")
        counts = torch.zeros(8, dtype=torch.int32, device="cuda")
        prm = ObstacleParams(0, max_hops, levels_above, 0, 0)

        def call():
            rc = m._L.gndt_obstacle_field_device(m._h, None, C.c_void_p(d_boxes.data_ptr()), len(boxes), 24, None, C.byref(prm), None,
                                                 C.c_void_p(hops.data_ptr()), C.c_void_p(owner.data_ptr()), C.c_void_p(counts.data_ptr()), sp)
            assert rc == 0, m._L.gndt_last_error(m._h)
        med, lo, hi = timed(call)
        marks = (C.c_uint64 * 5)()
        assert m._L.gndt_debug_obstacle_marks(m._h, marks) == 0
        c = [int(v) for v in counts.cpu()]
        out = {"boxes": len(boxes), "max_hops": max_hops, "ms": med, "min_ms": lo, "max_ms": hi, "counts": c,
               "window_columns": int(marks[0]), "worklist_rows": int(marks[1]), "probes_found": int(marks[2]), "columns_listed": int(marks[3]),
               "cover_minima": int(marks[4]), "fill_bytes": 8 * n}
        out["probes_found_per_column"] = round(int(marks[2]) / max(int(marks[0]), 1), 4)
        out["minima_per_covered_row"] = round(int(marks[4]) / max(c[0], 1), 4)
        return out

    def clearance_case(m, n, max_hops):
        hops = torch.empty(max(n, 1), dtype=torch.int32, device="cuda")
        near = torch.empty(max(n, 1), dtype=torch.int32, device="cuda")
        counts = torch.zeros(4, dtype=torch.int32, device="cuda")
        prm = ClearanceParams(1, max_hops)

        def call():
            rc = m._L.gndt_clearance_device(m._h, None, C.byref(prm), C.c_void_p(hops.data_ptr()), C.c_void_p(near.data_ptr()), None,
                                            C.c_void_p(counts.data_ptr()), sp)
            assert rc == 0, m._L.gndt_last_error(m._h)
        med, lo, hi = timed(call)
        return {"max_hops": max_hops, "ms": med, "min_ms": lo, "max_ms": hi, "counts": [int(v) for v in counts.cpu()]}

    def four_boxes(m):
        lo, hi = np.float32([b[0] for b in WORLD_BOXES]), np.float32([b[1] for b in WORLD_BOXES])
        return m.index_boxes(lo, hi)

    def both(m, n):
        out = {"rows": n, "field": [], "clearance": []}
        boxes = four_boxes(m)
        for max_hops in (4, 8, 32):
            out["field"].append(field_case(m, n, boxes, max_hops))
            out["clearance"].append(clearance_case(m, n, max_hops))
            out["field"][-1]["ratio_to_clearance"] = round(out["field"][-1]["ms"] / out["clearance"][-1]["ms"], 4)
        return out

    out = {"tool": "measure_obstacle", "device": g.device_info(0).get("name"), "source_hash": g._lib.source_hash()[:16], "reps": a.reps}
    maps = a.maps.split(",")
    if "site" in maps:
        cloud = scenes.drivable_site()
        m, n = build(cloud, scenes.COST_PARAMS, 0)
        site = both(m, n)
        # what the tallies cost: the same calls without them
        T.set_debug_option(T.DEBUG_OBSTACLE_TALLY, 0)
        site["field_no_tally"] = [field_case(m, n, four_boxes(m), h)["ms"] for h in (4, 8, 32)]
        T.set_debug_option(T.DEBUG_OBSTACLE_TALLY, 1)
        # the chain on one stream: segment (list of 16) -> field on its records -> 4 096 arcs walked with the field
        frame = torch.from_numpy(site_frame(cloud)).cuda()
        rng = np.random.default_rng(3)
        az = rng.uniform(-np.pi, np.pi, 4096)
        curve = rng.uniform(-0.15, 0.15, 4096)
        t = np.arange(8) * 0.75
        ang = az[:, None] + curve[:, None] * t[None, :]
        arcs = np.stack([cloud[0, 0] + np.cumsum(0.75 * np.cos(ang), 1), cloud[0, 1] + np.cumsum(0.75 * np.sin(ang), 1),
                         np.full((4096, 8), float(cloud[0, 2]))], 2).astype(np.float32)
        d_arcs = torch.from_numpy(arcs).cuda()
        for max_hops in (4, 8, 32):
            def chain():
                seg = m.segment_scan(frame, max_clusters=16)
                field = m.obstacle_field(seg, max_hops=max_hops, levels_above=4)
                return seg, field, m.walk_paths(d_arcs, hops=field, min_hops=2)
            seg, field, info = chain()
            med, lo, hi = timed(chain)
            site.setdefault("chain", []).append({"max_hops": max_hops, "ms": med, "min_ms": lo, "max_ms": hi, "clusters": int(seg["counts"][0]),
                                                  "field_counts": [int(v) for v in field["counts"].cpu()],
                                                  "too_close": int((info["status"] == 5).sum()), "done": int((info["status"] == 0).sum())})
            segment_ms = timed(lambda: m.segment_scan(frame, max_clusters=16))[0]
            walk_ms = timed(lambda: m.walk_paths(d_arcs, hops=field, min_hops=2))[0]
            site["chain"][-1].update(segment_alone_ms=segment_ms, walk_alone_ms=walk_ms)
        out["site"] = site
    if "s2" in maps:
        cloud = scenes.uniform_box(a.points + 1)
        m, n = build(cloud, dict(grid_len=0.5, z_len=0.5, slope_interval=0.08), 1 << 20)
        s2 = both(m, n)
        cells = m.export()
        rng = np.random.default_rng(9)
        s2["scaling"] = []
        for count in (1, 16, 256, 4096, 65536):
            r = rng.choice(n, count, replace=False)
            boxes = np.stack([cells["sx"][r], cells["sx"][r], cells["sy"][r], cells["sy"][r], cells["sz"][r], cells["sz"][r]], 1)
            s2["scaling"].append(field_case(m, n, boxes, 8))
        s2["zone_500"] = field_case(m, n, np.int32([[-250, 250, -250, 250, -2, 2]]), 8)
        out["s2"] = s2
        if "site" in out:
            out["s2_over_site"] = [round(b["ms"] / s["ms"], 3) for s, b in zip(out["site"]["field"], s2["field"])]
    out["what"] = ("median of HIP-event intervals around single gndt_obstacle_field_device / gndt_clearance_device calls (host side of the "
                   "call included); the chain's figure includes the Python wrappers of its three calls")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
