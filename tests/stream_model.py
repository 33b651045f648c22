"""A model of a table-resident map through a scripted life on one handle, and the named scripts (no GPU, no torch at import).

The model of a handle is the origin, every point ever added to its stream (fp32, in stream order: the device's stream index of a point
is its position here) and an `alive` mask.  The expected map after any step is the oracle's map of origin + points[alive]; first-seen
indices are compared after the monotone remap cumsum(alive) - 1 (tests/test_gpu_parity.py::test_remove_is_the_inverse_of_update: order
and labels depend only on the relative order of the first-seen indices).  Every operation keeps the model exact, by the equivalences
the suite asserts one by one: a remove of the alive points of the frames added last (test_remove_whole_frames_equals_the_build_
without_them), a crop as the death of the points of the dropped columns (test_crop_equals_remove_of_the_dropped_columns_points), a clear
as the death of the points of the nodes tests/clear_ref.py kills on the expected export (test_clear_equals_remove_and_the_oracle), an
identity merge as the source's stream appended at the destination's stream position (test_merge_into_a_populated_map_continues_the_
stream), reset / accumulate / finalize and stats_export -> stats_merge as in test_split_accumulate_finalize_and_stats_roundtrip.

A script is a named list of operations (tuples, first the kind, second the handle's name) with checkpoints; `run` walks it, keeps one
model per handle and hands every operation to a backend: the host emulation (tests/test_stream_model_host.py) or TwoDmap on the device
(tests/test_gpu_stream_sequences.py).  The scripts are written down, not drawn, each for the transitions of the handle's host-side
state its name says; the scenes are seeded points on a gently sloped surface over a square patch, sized from the code's constants:
do_finalize's small-map test (900 nodes), kSmallMapNodes (1024), cap_for_nodes.  Test infrastructure only."""
import numpy as np

from tests import clear_ref as cr
from tests import host_emulation as he
from tests import query_ref as qr

P = dict(grid_len=0.5, z_len=0.25, slope_interval=0.08, demand="slope")
ORIGIN = np.float32([0.13, -0.21, 0.07])
ATOMIC, AUTO = 1, 0
SMALL_SEEN, SMALL_KERNEL = 900, 1024          # do_finalize: table_nodes_seen <= 900u; gndt_table.hpp: kSmallMapNodes


def surface(x, y):
    return 0.04 * x + 0.025 * y


def patch(seed, n, side, centre=(0.0, 0.0)):
    """n seeded points on the sloped surface over the square of `side` metres about `centre` (relative to the origin), 12 mm of noise"""
    rng = np.random.default_rng(1000 + seed)
    x = centre[0] + side * (rng.random(n) - 0.5)
    y = centre[1] + side * (rng.random(n) - 0.5)
    z = surface(x, y) + 0.012 * rng.standard_normal(n)
    return np.ascontiguousarray(np.stack([x, y, z], 1) + ORIGIN.astype(np.float64), np.float32)


def point_keys(pts):
    """(sx, sy, sz) of every point by the kernels' own key (gndt_math.hpp through the host shim)"""
    import ctypes as C
    L = he.shim()
    pts = np.ascontiguousarray(pts, np.float32)
    n, stride = pts.shape
    keys = np.zeros(n, np.uint64)
    ok = np.zeros(n, np.uint8)
    o = (C.c_float * 3)(*[float(v) for v in ORIGIN])
    L.shim_point_keys(C.c_void_p(pts.ctypes.data), C.c_uint64(n), C.c_int(stride), o, C.c_float(P["grid_len"]), C.c_float(P["z_len"]),
                      C.c_void_p(keys.ctypes.data), C.c_void_p(ok.ctypes.data))
    assert ok.all()
    return he.unpack(keys)


def inside(sx, sy, box):
    return (sx >= box[0]) & (sx <= box[1]) & (sy >= box[2]) & (sy <= box[3])


def empty_map():
    return {"num_nodes": 0, "num_columns": 0, "num_slopes": 0}


class Model:
    """one handle's stream: pts[i] has stream index i, frame[i] the call that added it (-1: a position nothing was added at)"""

    def __init__(self, forget=()):
        self.forget = set(forget)          # the sensitivity cases: an effect the model deliberately leaves out
        self.restart()

    def restart(self):
        self.pts = np.zeros((0, 3), np.float32)
        self.alive = np.zeros(0, bool)
        self.frame = np.zeros(0, np.int64)
        self.frames = 0
        self._expected = None

    def place(self, pts, base=None, alive=None):
        """pts at stream positions base .. base + n (default: appended)"""
        base = len(self.pts) if base is None else int(base)
        n = len(pts)
        grow = base + n - len(self.pts)
        if grow > 0:
            self.pts = np.concatenate([self.pts, np.zeros((grow, 3), np.float32)])
            self.alive = np.concatenate([self.alive, np.zeros(grow, bool)])
            self.frame = np.concatenate([self.frame, np.full(grow, -1, np.int64)])
        assert (self.frame[base:base + n] == -1).all()
        self.pts[base:base + n] = pts[:, :3]
        self.alive[base:base + n] = True if alive is None else alive
        self.frame[base:base + n] = self.frames
        self.frames += 1
        self._expected = None

    def last_frames(self, k):
        """positions of the alive points of the k frames added last that still have any (None: of all of them)"""
        live = np.unique(self.frame[self.alive])
        which = live if k is None else live[-k:]
        return np.flatnonzero(self.alive & np.isin(self.frame, which))

    def kill(self, positions, effect):
        if effect not in self.forget:
            self.alive[positions] = False
            self._expected = None

    def crop(self, box):
        a = np.flatnonzero(self.alive)
        sx, sy = he.point_columns(self.pts[a], ORIGIN, P["grid_len"], P["z_len"])
        out = a[~inside(sx, sy, box)]
        self.kill(out, "crop")
        return len(a) - len(out), len(out)

    def clear(self, sensor, ends):
        exp = self.expected()
        if exp["num_nodes"] == 0:
            return 0, 0
        words, _, _ = cr.passes(exp, ORIGIN, P["grid_len"], P["z_len"], sensor, ends)
        drop = cr.cleared_rows(words, 1)
        a = np.flatnonzero(self.alive)
        gone = np.isin(qr.pack(*point_keys(self.pts[a])), qr.pack(exp["sx"], exp["sy"], exp["sz"])[drop])
        self.kill(a[gone], "clear")
        return int(drop.sum()), int(exp["num_nodes"])

    def merge(self, src):
        if "merge" not in self.forget:
            self.place(src.pts, alive=src.alive)

    def adopt(self, src):
        """the statistics of src merged into this (reset) handle: the same stream"""
        self.pts, self.alive, self.frame, self.frames = src.pts.copy(), src.alive.copy(), src.frame.copy(), src.frames
        self._expected = None

    def cloud(self):
        return np.concatenate([ORIGIN[None, :], self.pts[self.alive]])

    def expected(self):
        """the oracle's map of origin + points[alive]; first_idx counts the alive points"""
        if self._expected is None:
            from tests import parity
            self._expected = parity.ref_from_cloud(self.cloud(), P) if self.alive.any() else empty_map()
        return self._expected

    def remap(self, out):
        """an export with the device's stream indices -> the same with first_idx = cumsum(alive) - 1 of it; a first-seen index that
        names no alive point of the stream is an error of the map"""
        if int(out["num_nodes"]) == 0:
            return out
        fi = out["first_idx"].astype(np.int64)
        assert fi.max() < len(self.alive), ("first_idx beyond the stream", int(fi.max()), len(self.alive))
        assert self.alive[fi].all(), ("first_idx names a dead point", fi[~self.alive[fi]][:8])
        out = dict(out)
        out["first_idx"] = (np.cumsum(self.alive) - 1)[fi].astype(np.uint32)
        return out

    def query_points(self):
        """37 alive points, a few dead ones and a few that were never added"""
        a = np.flatnonzero(self.alive)
        d = np.flatnonzero(~self.alive & (self.frame >= 0))
        pick = a[np.linspace(0, len(a) - 1, 37).astype(np.int64)] if len(a) else a
        dead = d[np.linspace(0, len(d) - 1, 5).astype(np.int64)] if len(d) else d
        never = ORIGIN + np.float32([[500.3, 500.2, 3.0], [-400.1, 20.3, -2.0], [0.2, 0.2, 40.0]])
        return np.ascontiguousarray(np.concatenate([self.pts[pick], self.pts[dead], never]), np.float32)


def query_rows(cells, pts):
    """the NODE answer for pts on an export: the row with the point's key, -1 where there is none"""
    if int(cells["num_nodes"]) == 0:
        return np.full(len(pts), qr.NO_ROW, np.int64)
    return qr.node_rows(cells, pts, ORIGIN, P["grid_len"], P["z_len"])


# ---- the host's table sizing, restated ----

def pow2_ceil(v):
    p = 1
    while p < v:
        p <<= 1
    return p


def cap_for_nodes(nodes):
    """gndt_handle.hpp:503: pow2_ceil(max(2048, nodes * 2))"""
    return pow2_ceil(max(2048, 2 * int(nodes)))


class TableSim:
    """ensure_capacity_for / expected_nodes_for_batch (gndt_api_table.hip:240-259) and reserve_table (:319-323) for a handle without
    hints through updates and reserves; any other mutation ends what it can say (known = False)"""

    def __init__(self):
        self.cap, self.bound, self.known = 0, 0, True

    def update(self, n, true_nodes):
        """-> the table must grow for this frame"""
        want = cap_for_nodes(self.bound + n)             # no hint: every point may open a node
        grew = False
        if self.cap == 0:
            self.cap = want
        elif want > self.cap:
            self.bound = true_nodes                      # (the table is dirty: the real count is fetched)
            want = cap_for_nodes(self.bound + n)
            if want > self.cap:
                self.cap, grew = want, True
        self.bound = min(self.bound + n, self.cap)       # do_accumulate (:132)
        return grew

    def reserve(self, max_points, max_nodes):
        want = cap_for_nodes(max(max_nodes, 1024, max_points // 4))
        grew = 0 < self.cap < want
        self.cap = max(self.cap, want)
        return grew


# ---- the driver ----

MUTATIONS = ("build", "update", "remove", "crop", "clear", "merge", "reset", "accumulate", "finalize", "stats_to")


def run(script, backend, forget=()):
    """walk `script`: the models are moved here, every operation is handed to `backend` (a method of its kind, called with the
    handle's name, what the device call needs and the models), and a log of what each step did to the model comes back"""
    models, sims, log = {}, {}, []
    for step, op in enumerate(script):
        kind, h = op[0], op[1]
        m = models.get(h)
        entry = {"step": step, "kind": kind, "h": h}
        if kind in MUTATIONS and kind != "update":
            sims[h].known = False
        if kind == "new":
            models[h], sims[h] = Model(forget), TableSim()
            backend.new(h, **op[2])
        elif kind == "build":
            m.restart()
            m.place(op[2])
            backend.build(h, op[2])
        elif kind == "update":
            entry["stream_pos"] = len(m.pts)
            if sims[h].known:
                entry["grows"] = sims[h].update(len(op[2]), int(m.expected()["num_nodes"]))
            m.place(op[2])
            backend.update(h, op[2])
        elif kind == "remove":
            entry["nodes_before"] = int(m.expected()["num_nodes"])
            pos = m.last_frames(op[2])
            pts = m.pts[pos].copy()
            m.kill(pos, "remove")
            entry["nodes_after"] = int(m.expected()["num_nodes"])
            backend.remove(h, pts)
        elif kind == "crop":
            entry["kept"], entry["dropped"] = m.crop(op[2])
            entry["to_empty"] = len(op) > 3 and op[3] == "to_empty"
            backend.crop(h, op[2])
        elif kind == "clear":
            count_only = len(op) > 4 and op[4] == "count_only"
            if not count_only:
                entry["killed"], entry["nodes"] = m.clear(op[2], op[3])
            backend.clear(h, op[2], op[3], count_only)
        elif kind == "merge":
            m.merge(models[op[2]])
            backend.merge(h, op[2])
        elif kind == "reset":
            m.restart()
            backend.reset(h)
        elif kind == "accumulate":
            m.place(op[2], base=op[3])
            backend.accumulate(h, op[2], op[3])
        elif kind == "finalize":
            backend.finalize(h)
        elif kind == "stats_to":                           # stats_export of h, stats_merge in two halves into the (reset) handle op[2]
            sims[op[2]].known = False
            if "merge" not in models[op[2]].forget:
                models[op[2]].adopt(m)
            backend.stats_to(h, op[2])
        elif kind == "reserve":                            # to op[3] times the node count of the map
            nodes = op[3] * int(m.expected()["num_nodes"])
            if sims[h].known:
                entry["grows"] = sims[h].reserve(op[2], nodes)
            backend.reserve(h, op[2], nodes)
        elif kind == "deferred":
            backend.deferred(h, op[2])
        elif kind == "query":                              # a read between checkpoints
            backend.query(h, m)
        elif kind == "refused":                            # op[2]: the call a handle without a table map refuses; op[3]: its points
            backend.refused(h, op[2], op[3] if len(op) > 3 else None)
        elif kind == "check":
            entry["label"], entry["expect"] = op[2], (op[3] if len(op) > 3 else {})
            entry["nodes"] = int(m.expected()["num_nodes"])
            entry["alive"] = int(m.alive.sum())
            backend.check(h, op[2], m)
        else:
            raise ValueError(kind)
        log.append(entry)
    return log


# ---- the scripts ----

def _small(seed):
    return patch(seed, 3000, 10.0)                         # 400 columns: well under 900 nodes


def _growth_frames(h, seed, checks=True):
    """frames of 37 / 500 / 3 000 / 12 000 / 37 / 30 000 points on patches that grow with them, on a handle without hints"""
    ops = []
    for k, (n, side) in enumerate(((37, 1.0), (500, 3.0), (3000, 8.0), (12000, 15.0), (37, 1.0), (30000, 25.0))):
        ops.append(("update", h, patch(seed + k, n, side)))
        if checks:
            ops.append(("check", h, f"frame of {n}"))
    return ops


def small_then_stream():
    a = "a"
    return [("new", a, dict(strategy=ATOMIC)),
            ("build", a, _small(1)), ("check", a, "first small build", {"nodes_max": SMALL_SEEN}),
            ("build", a, _small(2)), ("check", a, "second small build: one workgroup", {"nodes_max": SMALL_SEEN}),
            ("update", a, patch(3, 12000, 20.0)),
            ("update", a, patch(4, 12000, 20.0, (9.0, 4.0))), ("check", a, "updates past the small kernel", {"nodes_min": SMALL_KERNEL + 1}),
            ("remove", a, 1), ("check", a, "one frame removed", {"nodes_min": SMALL_KERNEL + 1}),
            ("remove", a, 1), ("check", a, "small again through n_dead", {"nodes_max": SMALL_SEEN}),
            ("update", a, patch(5, 500, 3.0, (2.0, -1.0))), ("check", a, "a small update", {"nodes_max": SMALL_SEEN})]


def small_seen_then_tails():
    a, s = "a", "s"
    big = {"nodes_min": SMALL_KERNEL + 1}
    sensor = ORIGIN + np.float32([2.0, 3.0, 6.0])
    ends = patch(16, 200, 1.5, (4.0, 5.0)) - np.float32([0.0, 0.0, 0.5])         # below the surface: the rays pass through its nodes
    return [("new", a, dict(strategy=ATOMIC)),
            ("build", a, _small(11)),
            ("build", a, _small(12)), ("check", a, "second small build: one workgroup", {"nodes_max": SMALL_SEEN}),
            ("update", a, patch(13, 12000, 20.0)),
            ("update", a, patch(14, 12000, 20.0, (8.0, 4.0))),
            ("update", a, patch(15, 3000, 8.0, (-9.0, -9.0))), ("check", a, "several thousand nodes", big),
            ("crop", a, (-16, 34, -18, 26)), ("check", a, "after the crop", big),
            ("clear", a, sensor, ends, "count_only"),
            ("clear", a, sensor, ends), ("check", a, "after the clear", big),
            ("remove", a, 1), ("check", a, "after the remove", big),
            ("new", s, dict(strategy=ATOMIC)), ("build", s, patch(17, 3000, 8.0, (16.0, -6.0))),
            ("merge", a, s), ("check", a, "after the merge", big),
            ("finalize", a), ("check", a, "after the bare finalize", big)]


def small_seen_each_tail():
    """small_seen_then_tails reaches the one-workgroup kernel through its first tail only: the fallback clears small_ok for the rest
    of the handle's life.  Here every tail is the first on a handle of its own."""
    big = {"nodes_min": SMALL_KERNEL + 1}
    small1, small2, f1, f2, nxt = _small(81), _small(82), patch(83, 12000, 20.0), patch(84, 3000, 8.0, (-9.0, -9.0)), patch(85, 500, 3.0, (6.0, 6.0))
    sensor = ORIGIN + np.float32([2.0, 3.0, 6.0])
    ends = patch(86, 200, 1.5, (4.0, 5.0)) - np.float32([0.0, 0.0, 0.5])
    tails = {"crop": [("crop", "crop", (-16, 34, -18, 26))], "clear": [("clear", "clear", sensor, ends)], "remove": [("remove", "remove", 1)],
             "merge": [("merge", "merge", "s")], "finalize": [("finalize", "finalize")]}
    ops = [("new", "s", dict(strategy=ATOMIC)), ("build", "s", patch(87, 3000, 8.0, (16.0, -6.0)))]
    for h, tail in tails.items():
        ops += [("new", h, dict(strategy=ATOMIC)), ("build", h, small1), ("build", h, small2), ("check", h, "small seen", {"nodes_max": SMALL_SEEN}),
                ("update", h, f1), ("update", h, f2)] + tail + [("check", h, "after the tail", big), ("update", h, nxt), ("check", h, "and a frame", big)]
    return ops


def deferred_crossings():
    a = "a"
    return [("new", a, dict(strategy=ATOMIC)), ("deferred", a, True),
            ("update", a, patch(21, 500, 3.0)),
            ("update", a, patch(22, 500, 3.0, (1.0, 1.0))),
            ("update", a, patch(23, 12000, 15.0)),                                  # the table grows under an un-emitted frame
            ("query", a), ("check", a, "after the growth"),
            ("update", a, patch(24, 3000, 8.0, (6.0, -5.0))), ("remove", a, 1), ("update", a, patch(25, 500, 3.0, (-5.0, 5.0))),
            ("check", a, "frame, remove, frame"),
            ("update", a, patch(26, 37, 1.0, (3.0, 3.0))),
            ("crop", a, (-12, 14, -10, 15)), ("update", a, patch(27, 3000, 8.0, (-4.0, 2.0))), ("check", a, "crop under pending frames, frame"),
            ("update", a, patch(28, 500, 3.0, (9.0, 9.0))),
            ("deferred", a, False), ("update", a, patch(29, 12000, 15.0, (2.0, -2.0))),
            ("check", a, "switched off under pending frames, frame"), ("check", a, "a second read")]


def growth_and_reserve():
    a = "a"
    return ([("new", a, dict(strategy=ATOMIC))] + _growth_frames(a, 31) +
            [("reserve", a, 60000, 4), ("check", a, "after the reserve"),               # the order's buffers move, the table stays
             ("update", a, patch(38, 3000, 8.0, (-10.0, 10.0))), ("check", a, "a frame after the reserve"),
             ("update", a, patch(39, 500, 3.0, (11.0, -11.0))), ("check", a, "and another"),
             ("reserve", a, 200000, 4), ("check", a, "after a reserve that grows the table"),
             ("update", a, patch(40, 37, 1.0, (-3.0, -3.0))), ("check", a, "a frame after it")])


def rebuild_between():
    a, p = "a", "p"
    cloud = patch(46, 66000, 30.0)                           # AUTO: PARTITION from 65 536 points on, for points in no scan order
    pts = patch(47, 500, 3.0)
    return [("new", a, dict(strategy=ATOMIC)),
            ("update", a, patch(41, 3000, 8.0)), ("update", a, patch(42, 500, 3.0, (5.0, 5.0))), ("check", a, "a stream"),
            ("build", a, patch(43, 30000, 25.0)), ("check", a, "a large cloud", {"nodes_min": SMALL_KERNEL + 1}),
            ("build", a, _small(44)), ("check", a, "large then small on the table", {"nodes_max": SMALL_SEEN}),
            ("update", a, patch(45, 3000, 8.0, (7.0, -3.0))), ("check", a, "a stream on top"),
            ("remove", a, 1), ("check", a, "and a remove"),
            ("new", p, dict(strategy=AUTO)),
            ("build", p, cloud), ("check", p, "partition build"),
            ("refused", p, "update", pts), ("refused", p, "remove", cloud[:500]), ("refused", p, "stats_export"),
            ("check", p, "unchanged after the refusals"),
            ("reset", p), ("accumulate", p, patch(48, 7000, 15.0, (3.0, 3.0)), 5000), ("accumulate", p, patch(49, 5000, 15.0), 0),
            ("finalize", p), ("check", p, "reset, accumulate, finalize"),
            ("update", p, patch(50, 3000, 8.0, (-8.0, 6.0))), ("check", p, "a stream after it")]


def to_empty_and_back():
    a = "a"
    return [("new", a, dict(strategy=ATOMIC)),
            ("update", a, patch(51, 3000, 8.0)), ("update", a, patch(52, 500, 3.0, (5.0, 0.0))), ("check", a, "a stream"),
            ("crop", a, (1000, 1010, 1000, 1010), "to_empty"), ("check", a, "nothing left", {"nodes_max": 0}),
            ("update", a, patch(53, 500, 3.0, (-2.0, 2.0))), ("check", a, "indices go on counting"),
            ("remove", a, None), ("check", a, "empty through n_dead", {"nodes_max": 0}),
            ("update", a, patch(54, 3000, 8.0, (1.0, 1.0))), ("check", a, "and back")]


def merge_and_stats():
    d, s, t = "d", "s", "t"
    return ([("new", d, dict(strategy=ATOMIC)),
             ("update", d, patch(61, 12000, 15.0)), ("update", d, patch(62, 3000, 8.0, (8.0, 2.0))), ("check", d, "a stream"),
             ("new", s, dict(strategy=ATOMIC)), ("build", s, patch(63, 3000, 8.0, (-9.0, 6.0))),
             ("merge", d, s), ("check", d, "after the merge"),
             ("update", d, patch(64, 500, 3.0, (0.0, -9.0))), ("remove", d, 1), ("check", d, "frame and its remove"),
             ("new", t, dict(strategy=ATOMIC))] + _growth_frames(t, 71, checks=False) +
            [("reserve", t, 60000, 4), ("update", t, patch(78, 3000, 8.0, (-10.0, 10.0))), ("update", t, patch(79, 500, 3.0, (11.0, -11.0))),
             ("check", t, "the life of growth_and_reserve"),
             ("reset", t), ("stats_to", d, t), ("finalize", t),
             ("check", t, "statistics merged in two halves"), ("check", d, "the exporter")])


SCRIPTS = {f.__name__: f for f in (small_then_stream, small_seen_then_tails, small_seen_each_tail, deferred_crossings, growth_and_reserve, rebuild_between,
                                   to_empty_and_back, merge_and_stats)}
