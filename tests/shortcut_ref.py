"""Route shortcutting restated from the exported rows (include/gndt.h "route shortcutting"): a link is the walks' restatement
(tests/walk_ref.Walker: the step lists of tests/clearance_ref.Field, the pick, the overhead test) over the column sequence of free-space
clearing's restatement of the ray walk (tests/clear_ref.rays) between the two columns' centres, with the start row given; the group
order, the counts and the sums are written here with explicit np.float32 / np.float64.  Calls neither the library nor a shim.  Test
infrastructure only."""
import numpy as np

from tests import clear_ref
from tests import clearance_ref as cr
from tests import query_ref as qr
from tests import walk_ref as wr

OK, EMPTY, BAD_ROUTE, LIMIT = range(4)
NO_ROW = 0xFFFFFFFF
BEYOND = 0xFFFFFFFF
DEFAULT_WINDOW, MAX_WINDOW = 64, 256
DEFAULT_LINKS, MAX_LINKS = 1 << 20, 1 << 24
INFO_FIELDS = ("status", "length_in", "waypoints", "path_slopes", "links_tested", "fallback_links", "cost_in", "cost_out", "hops_min")
INFO_DTYPE = np.dtype([("status", np.int32), ("length_in", np.uint32), ("waypoints", np.uint32), ("path_slopes", np.uint32),
                       ("links_tested", np.uint32), ("fallback_links", np.uint32), ("cost_in", np.float32), ("cost_out", np.float32),
                       ("hops_min", np.uint32), ("reserved", np.uint32, 3)])


def lin(s):
    return s - 1 if s > 0 else s


class Shortcutter:
    """The links of one Walker (one map, one robot); shortcut() answers a batch of routes."""

    def __init__(self, cells, origin, grid_len, z_len, robot=None, walker=None):
        self.w = walker if walker is not None else wr.Walker(cells, origin, grid_len, z_len, robot)
        self.origin, self.grid_len, self.z_len = np.asarray(origin, np.float32), grid_len, z_len
        self.n = self.w.n
        self._links = {}                                     # what links() has answered (a call is repeated with other caps)

    def centre(self, axis, s):
        """(float)((double)o + sign(s) * (|s| - 0.5) * (double)grid_len)"""
        a = np.float64(abs(int(s))) - np.float64(0.5)
        return np.float32(np.float64(self.origin[axis]) + (a if s > 0 else -a) * np.float64(np.float32(self.grid_len)))

    def point(self, row, z):
        return np.float32([self.centre(0, self.w.sx[row]), self.centre(1, self.w.sy[row]), z])

    def valid(self, row):
        return 0 <= row < self.n and bool(self.w.slope[row])

    def links(self, a, bs, window, overhead=False, hops=None, min_hops=0):
        """Link(a, b) for every b of bs -> [(holds, the slopes stood on, a first)]"""
        key = (a, tuple(bs), window, overhead, None if hops is None else id(hops), min_hops)
        if key not in self._links:
            self._links[key] = (self._links_of(a, bs, window, overhead, hops, min_hops), hops)       # (hops kept alive: its id is the key)
        return self._links[key][0]

    def _links_of(self, a, bs, window, overhead, hops, min_hops):
        w = self.w
        out = [(False, [])] * len(bs)
        if not self.valid(a):
            return out
        z = w.mean[a, 2]
        pa = self.point(a, z)
        kx, ky, _, _, ok = qr.keys(pa[None, :], self.origin, self.grid_len, self.z_len)
        if not ok[0] or (int(kx[0]), int(ky[0])) != (w.sx[a], w.sy[a]):
            return out
        todo, pts = [], []
        for i, b in enumerate(bs):
            if not self.valid(b):
                continue
            pb = self.point(b, z)
            kx, ky, _, _, ok = qr.keys(pb[None, :], self.origin, self.grid_len, self.z_len)
            if not ok[0] or (int(kx[0]), int(ky[0])) != (w.sx[b], w.sy[b]):
                continue
            if abs(lin(w.sx[b]) - lin(w.sx[a])) + abs(lin(w.sy[b]) - lin(w.sy[a])) > window:
                continue
            todo.append(i)
            pts.append(pb)
        if not todo:
            return out
        ok, cols = clear_ref.rays(self.origin, self.grid_len, self.z_len, pa, np.float32(pts))
        assert ok.all()

        def enter(t):
            if overhead and w.f.overhead[t]:
                return False
            return not (hops is not None and int(hops[t]) < min_hops)

        out = list(out)
        for j, i in enumerate(todo):
            sel = cols["ray"] == j
            seq = list(zip(cols["sx"][sel].tolist(), cols["sy"][sel].tolist()))
            assert seq[0] == (w.sx[a], w.sy[a]) and seq[-1] == (w.sx[bs[i]], w.sy[bs[i]])
            q, stood = a, [a]
            good = enter(a)
            for col in seq[1:]:
                if not good:
                    break
                k = cr.sides_of(w.sx[q], w.sy[q]).index(col)
                t, _ = w.pick(q, k)
                if t is None:
                    good = False
                    break
                q = t
                stood.append(q)
                good = enter(q)
            out[i] = (bool(good and q == bs[i]), stood)
        return out

    def shortcut(self, routes, lengths, window=0, overhead=False, hops=None, min_hops=0, max_links=0, waypoint_cap=None, path_cap=0):
        """routes [K, route_cap] uint32, lengths [K] -> (info [K] of INFO_DTYPE, waypoint_rows [K, waypoint_cap], path_rows [K, path_cap],
        the full (waypoints, path, the index of every fallback link's end in the path) per route)"""
        w = self.w
        routes = np.asarray(routes).astype(np.int64) & 0xFFFFFFFF
        K, route_cap = routes.shape
        window = window or DEFAULT_WINDOW
        max_links = max_links or DEFAULT_LINKS
        wcap = route_cap if waypoint_cap is None else waypoint_cap
        info = np.zeros(K, INFO_DTYPE)
        wrows = np.full((K, wcap), NO_ROW, np.uint32)
        prows = np.full((K, path_cap), NO_ROW, np.uint32)
        full = []
        for k in range(K):
            o = info[k]
            n = int(lengths[k])
            o["length_in"], o["hops_min"] = n, BEYOND
            wp, path, fb = [], [], []
            full.append((wp, path, fb))
            if n == 0:
                o["status"] = EMPTY
                continue
            if n > route_cap or not all(self.valid(int(r)) for r in routes[k, :n]):
                o["status"] = BAD_ROUTE
                continue
            r = [int(v) for v in routes[k, :n]]
            cost_in = np.float64(0.0)
            for i in range(n - 1):
                cost_in += np.float64(wr.travel(w.mean[r[i]], w.mean[r[i + 1]]))
            wp.append(r[0])
            path.append(r[0])
            tested, fallback, status, a = 0, 0, OK, 0
            while a < n - 1:
                cand = min(window, n - 1 - a)
                nxt, limit = None, False
                for g in reversed(range((cand + 63) // 64)):
                    js = list(range(a + 64 * g + 1, a + min(64 * g + 64, cand) + 1))
                    if tested + len(js) > max_links:
                        limit = True
                        break
                    tested += len(js)
                    res = self.links(r[a], [r[j] for j in js], window, overhead, hops, min_hops)
                    held = [(j, st) for j, (ok, st) in zip(js, res) if ok]
                    if held:
                        nxt, stood = held[-1]
                        break
                if limit:
                    status = LIMIT
                    for i in range(a + 1, n):
                        fb.append(len(path))
                        path.append(r[i])
                        wp.append(r[i])
                        fallback += 1
                    break
                if nxt is None:
                    nxt = a + 1
                    fallback += 1
                    fb.append(len(path))
                    path.append(r[nxt])
                else:
                    path.extend(stood[1:])
                wp.append(r[nxt])
                a = nxt
            cost_out = np.float64(0.0)
            for i in range(len(path) - 1):
                cost_out += np.float64(wr.travel(w.mean[path[i]], w.mean[path[i + 1]]))
            o["status"], o["waypoints"], o["path_slopes"], o["links_tested"], o["fallback_links"] = status, len(wp), len(path), tested, fallback
            o["cost_in"], o["cost_out"] = np.float32(cost_in), np.float32(cost_out)
            if hops is not None:
                o["hops_min"] = min(int(hops[t]) for t in path)
            wrows[k, :min(len(wp), wcap)] = wp[:wcap]
            prows[k, :min(len(path), path_cap)] = path[:path_cap]
        return info, wrows, prows, full


def same(got_info, got_wp, got_path, want_info, want_wp, want_path, what=""):
    """every field of every route and every row of both outputs, for equality (floats by their bits)"""
    for k in INFO_FIELDS:
        g, w = np.asarray(got_info[k]), np.asarray(want_info[k])
        if g.dtype.kind == "f":
            g, w = g.view(np.uint32), w.view(np.uint32)
        assert np.array_equal(g, w), (what, k, np.flatnonzero(g != w)[:8], got_info[k][:8], want_info[k][:8])
    assert not np.asarray(got_info["reserved"]).any(), what
    assert np.array_equal(np.asarray(got_wp).view(np.uint32), want_wp), (what, "waypoint_rows", np.argwhere(np.asarray(got_wp).view(np.uint32) != want_wp)[:8])
    if want_path is not None and want_path.size:
        assert np.array_equal(np.asarray(got_path).view(np.uint32), want_path), (what, "path_rows")
