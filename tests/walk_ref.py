"""Path walks restated from the exported rows (include/gndt.h "path walks"): the start through the queries' numpy restatement
(tests/query_ref.py), every segment's columns from free-space clearing's restatement of the ray walk (tests/clear_ref.rays, one call a
segment, both ends at waypoint 0's z), the steps of a slope through a side from the clearance field's restatement
(tests/clearance_ref.Field: its gates, its open sides, its overhead test), and the pick, the checks and the sums written here with
explicit np.float32 / np.float64.  Calls neither the library nor a shim.  Test infrastructure only."""
import numpy as np

from tests import clear_ref
from tests import clearance_ref as cr
from tests import query_ref as qr

DONE, NO_START, BLOCKED, LEFT_MAP, OVERHEAD, TOO_CLOSE, LIMIT = range(7)
NO_ROW = 0xFFFFFFFF
NO_SIDE = 0xFFFFFFFF
BEYOND = 0xFFFFFFFF
DEFAULT_STEPS = 65536
INFO_FIELDS = ("status", "stop_side", "steps", "waypoints", "start_row", "end_row", "length", "climb", "rough_max", "hops_min")
INFO_DTYPE = np.dtype([("status", np.int32), ("stop_side", np.uint32), ("steps", np.uint32), ("waypoints", np.uint32),
                       ("start_row", np.uint32), ("end_row", np.uint32), ("length", np.float32), ("climb", np.float32),
                       ("rough_max", np.float32), ("hops_min", np.uint32), ("reserved", np.uint32, 2)])


def travel(a, b):
    """the flood's TravelCost: fp32 differences, squares and root in fp64, rounded to fp32"""
    d = (np.asarray(a, np.float32) - np.asarray(b, np.float32)).astype(np.float64)
    return np.float32(np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))


class Walker:
    """The step lists of one Field (one map, one robot); walk() answers a batch of paths."""

    def __init__(self, cells, origin, grid_len, z_len, robot=None, field=None):
        self.cells, self.origin, self.grid_len, self.z_len = cells, np.asarray(origin, np.float32), grid_len, z_len
        self.robot = robot
        self.f = field if field is not None else cr.Field(cells, robot)
        n = self.n = int(cells["num_nodes"])
        self.sx, self.sy = ([int(v) for v in cells[k][:n]] for k in ("sx", "sy"))
        self.mean = np.asarray(cells["mean"], np.float32).reshape(-1, 3)[:n]
        self.rough = np.asarray(cells["rough"], np.float32)[:n]
        self.slope = (np.asarray(cells["flags"][:n]) & 2) != 0
        self.steps = {}                                     # (q, side) -> the steps of q through the side, ascending
        for q, t in sorted(zip(self.f.edge_from.tolist(), self.f.edge_to.tolist())):
            k = cr.sides_of(self.sx[q], self.sy[q]).index((self.sx[t], self.sy[t]))
            self.steps.setdefault((q, k), []).append(t)

    def start_rows(self, p0, mode):
        if mode == "node":
            r = qr.node_rows(self.cells, p0, self.origin, self.grid_len, self.z_len)
            return np.where((r >= 0) & self.slope[np.maximum(r, 0)], r, -1) if self.n else r
        return qr.nearest_slope_rows(self.cells, p0, self.origin, self.grid_len, self.z_len)

    def pick(self, q, k):
        """-> (row or None, |dz| fp32): the least fabsf(mean_z(t) - mean_z(q)), a tie going to the smaller row"""
        best, best_d = None, None
        for t in self.steps.get((q, k), ()):
            d = np.abs(np.float32(self.mean[t, 2] - self.mean[q, 2]))
            if best is None or d < best_d:
                best, best_d = t, d
        return best, best_d

    def walk(self, paths, start_mode="nearest_slope", overhead=False, hops=None, min_hops=0, max_steps=0, row_cap=0):
        """-> (info: structured array [K] of INFO_DTYPE, rows: uint32 [K, row_cap], walked: per path the full list of slopes stood on)"""
        paths = np.asarray(paths, np.float32)
        K, T = paths.shape[:2]
        max_steps = max_steps or DEFAULT_STEPS
        info = np.zeros(K, INFO_DTYPE)
        rows = np.full((K, row_cap), NO_ROW, np.uint32)
        walked = []
        starts = self.start_rows(paths[:, 0, :3], start_mode) if K and T else np.zeros(0, np.int64)
        for p in range(K):
            o = info[p]
            o["status"], o["stop_side"], o["start_row"], o["end_row"], o["hops_min"] = NO_START, NO_SIDE, NO_ROW, NO_ROW, BEYOND
            stood = []
            walked.append(stood)
            if T == 0 or starts[p] < 0:
                continue
            q = int(starts[p])
            length, climb = np.float64(0.0), np.float64(0.0)
            state = dict(rough=None, hops_min=BEYOND)

            def enter(t):
                stood.append(t)
                r = self.rough[t]
                if state["rough"] is None or r > state["rough"]:
                    state["rough"] = r
                hp = None
                if hops is not None:
                    hp = int(hops[t])
                    state["hops_min"] = min(state["hops_min"], hp)
                if overhead and self.f.overhead[t]:
                    return OVERHEAD
                if hp is not None and hp < min_hops:
                    return TOO_CLOSE
                return DONE

            o["start_row"] = q
            status = enter(q)
            waypoints, steps, stop = 1, 0, NO_SIDE
            z0 = paths[p, 0, 2]
            prev = paths[p, 0, :2]
            for j in range(1, T):
                if status != DONE:
                    break
                xy = paths[p, j, :2]
                if not np.isfinite(xy).all():
                    break
                a = np.float32([prev[0], prev[1], z0])
                b = np.float32([[xy[0], xy[1], z0]])
                ok_a = qr.keys(a[None, :], self.origin, self.grid_len, self.z_len)[4][0]
                ok, cols = clear_ref.rays(self.origin, self.grid_len, self.z_len, a, b)
                if not (ok_a and ok[0]):
                    status = LEFT_MAP
                    break
                seq = list(zip(cols["sx"].tolist(), cols["sy"].tolist()))
                assert seq[0] == (self.sx[q], self.sy[q]), (p, j, seq[0], q)
                for col in seq[1:]:
                    if steps == max_steps:
                        status = LIMIT
                        break
                    k = cr.sides_of(self.sx[q], self.sy[q]).index(col)
                    t, dz = self.pick(q, k)
                    if t is None:
                        status, stop = (LEFT_MAP if self.f.open[q, k] else BLOCKED), k
                        break
                    length += np.float64(travel(self.mean[q], self.mean[t]))
                    climb += np.float64(dz)
                    steps += 1
                    q = t
                    status = enter(q)
                    if status != DONE:
                        break
                if status == DONE:
                    waypoints = j + 1
                prev = xy
            o["status"], o["stop_side"], o["steps"], o["waypoints"], o["end_row"] = status, stop, steps, waypoints, stood[-1]
            o["length"], o["climb"], o["rough_max"], o["hops_min"] = np.float32(length), np.float32(climb), state["rough"], state["hops_min"]
            m = min(len(stood), row_cap)
            rows[p, :m] = stood[:m]
        return info, rows, walked


def same(got_info, got_rows, want_info, want_rows, what=""):
    """every field of every path and every row, for equality (floats by their bits)"""
    for k in INFO_FIELDS:
        g, w = np.asarray(got_info[k]), np.asarray(want_info[k])
        if g.dtype.kind == "f":
            g, w = g.view(np.uint32), w.view(np.uint32)
        assert np.array_equal(g, w), (what, k, np.flatnonzero(g != w)[:8], got_info[k][:8], want_info[k][:8])
    assert not np.asarray(got_info["reserved"]).any(), what
    if want_rows is not None and want_rows.size:
        assert np.array_equal(got_rows, want_rows), (what, "rows", np.argwhere(got_rows != want_rows)[:8])
