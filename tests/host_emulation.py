"""CPU emulation of libgndt's pipeline built from the SAME arithmetic header the kernels use
(grid_ndt_amd/csrc/gndt_math.hpp via tests/host_math_shim.cpp) plus numpy for the data movement.
It lets the CPU test tier check the kernel maths, the order-free restatement of the slope label and
the parity tolerances against the oracle.  Test infrastructure only."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_SO = os.path.join(_HERE, "_host_math_shim.so")
_lib = None


def load_shim(src, so_name, headers, signatures):
    """tests/<src> compiled with g++ into tests/<so_name> (again when it or one of `headers` of grid_ndt_amd/csrc is newer) and loaded;
    signatures: {function: (argtypes, restype)}"""
    csrc = os.path.join(_ROOT, "grid_ndt_amd", "csrc")
    src, so = os.path.join(_HERE, src), os.path.join(_HERE, so_name)
    deps = [src] + [os.path.join(csrc, f) for f in headers]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I", csrc, "-o", so, src])
    L = C.CDLL(so)
    for name, (argtypes, restype) in signatures.items():
        getattr(L, name).argtypes = argtypes
        getattr(L, name).restype = restype
    return L


def shim():
    global _lib
    if _lib is None:
        _lib = load_shim("host_math_shim.cpp", os.path.basename(_SO), ("gndt_math.hpp", "gndt_cost.hpp"),
                         {"shim_mean_z": ([C.c_uint32, C.c_double, C.c_double], C.c_float)})
    return _lib


_clib = None


def consumer_shim():
    """tests/consumer_shim.cpp: the queries', the raster export's and free-space clearing's per-element code, built for the host"""
    global _clib
    if _clib is None:
        vp, f, i32, u32, u64 = C.c_void_p, C.c_float, C.c_int32, C.c_uint32, C.c_uint64
        _clib = load_shim("consumer_shim.cpp", "_consumer_shim.so", ("gndt_math.hpp", "gndt_cost.hpp", "gndt_query.hpp", "gndt_ray.hpp"), {
            "build_index": ([vp, vp, vp, u64, vp, vp, u32], None),
            "qshim_query": ([C.c_int, C.c_int, C.c_int, vp, u32, u64] + [vp] * 8 + [u32, vp, vp, vp, f, f, u64, vp, vp, vp], C.c_int),
            "qshim_ctab_find": ([vp, vp, u32, i32, i32], u32),
            "rshim_index": ([i32, u32], C.c_int),
            "rshim_count": ([i32, i32], u32),
            "rshim_raster": ([C.c_int, u32, i32, i32, u32, u32, f] + [vp] * 9 + [u32] + [vp] * 8, C.c_int),
            "cshim_walk": ([vp, f, f, vp, vp, f, f, vp, i32], C.c_int),
            "cshim_passes": ([vp, f, f, vp, vp, u64, u32, f, f, C.c_int] + [vp] * 4 + [u64, vp, vp, u32, vp, vp, vp], None),
        })
    return _clib


def _pow2_at_least(v, floor=1024):
    p = floor
    while p < v:
        p <<= 1
    return p


class HostMap:
    """The rows of an oracle map, with the per-row column sizes, the column index derived on the host — at the library's size
    (column_index's rule: load <= 1/2), or with table="tight" the smallest table with a free slot (long probe chains: ctab_find) —
    and a made-up cost map drawn from `seed`; run through consumer_shim()"""

    def __init__(self, cloud, P, table="library", seed=11):
        from oracle import oracle
        from tests import query_ref as qr
        self.origin = np.asarray(cloud[0, :3], np.float32)
        self.P = P
        c = oracle.build_grid(cloud, P["grid_len"], P["z_len"], P["slope_interval"], P.get("demand", "slope"), mode=oracle.MODE_INT_OPENMP)
        self.cells = c
        self.n = int(c["num_nodes"])
        self.sx, self.sy, self.sz = (np.ascontiguousarray(c[k], np.int32) for k in ("sx", "sy", "sz"))
        self.mean = np.ascontiguousarray(c["mean"], np.float32)
        self.rough = np.ascontiguousarray(c["rough"], np.float32)
        self.flags = np.ascontiguousarray(c["flags"], np.uint32)
        self.row_ncol = qr.row_ncol(c)
        K = int((self.row_ncol > 0).sum())
        assert K == int(c["num_columns"])
        self.tsize = _pow2_at_least(2 * K) if table == "library" else _pow2_at_least(K + 1, floor=1)
        self.ctab_key = np.zeros(self.tsize, np.uint64)
        self.ctab_val = np.zeros(self.tsize, np.uint32)
        consumer_shim().build_index(self.sx.ctypes.data, self.sy.ctypes.data, self.row_ncol.ctypes.data, self.n, self.ctab_key.ctypes.data,
                                    self.ctab_val.ctypes.data, self.tsize)
        rng = np.random.default_rng(seed)
        self.h_bits = rng.integers(0, 0x7F7FFFFF, size=max(self.n, 1), dtype=np.uint32)
        self.state = rng.integers(0, 3, size=max(self.n, 1), dtype=np.uint32)

    def box(self):
        return int(self.sx.min()), int(self.sx.max()), int(self.sy.min()), int(self.sy.max())

    def query(self, pts, mode, ilp=1, threads=1, gather=False):
        """query_points over n points as k_query's `threads` threads run them -> rows (int64), with gather (rows, h, state)"""
        pts = np.ascontiguousarray(pts, np.float32)
        n = pts.shape[0]
        rows = np.full(n, 0xDEADBEEF, np.uint32)
        h = np.zeros(n, np.float32)
        st = np.full(n, 99, np.uint32)
        o = (C.c_float * 3)(*[float(v) for v in self.origin])
        rc = consumer_shim().qshim_query(mode, ilp, int(gather), pts.ctypes.data, pts.shape[1], n, self.sx.ctypes.data, self.sy.ctypes.data,
                                         self.sz.ctypes.data, self.mean.ctypes.data, self.flags.ctypes.data, self.row_ncol.ctypes.data,
                                         self.ctab_key.ctypes.data, self.ctab_val.ctypes.data, self.tsize, self.h_bits.ctypes.data,
                                         self.state.ctypes.data, o, self.P["grid_len"], self.P["z_len"], threads, rows.ctypes.data,
                                         h.ctypes.data, st.ctypes.data)
        assert rc == 0
        r = rows.view(np.int32).astype(np.int64)
        return (r, h, st) if gather else r

    def raster(self, box, mode, z_ref=0.0, gather=3, layers=("row", "z", "rough", "nodes", "h", "state")):
        """raster_pixel over every pixel of the box -> {layer: (H, W) image}"""
        from tests import raster_ref as rr
        W, H = len(rr.axis(box[0], box[1])), len(rr.axis(box[2], box[3]))
        dt = {"row": np.uint32, "z": np.float32, "rough": np.float32, "nodes": np.uint32, "h": np.float32, "state": np.uint32}
        out = {k: np.full((H, W), 0xA5A5A5A5, np.uint32).view(dt[k]) for k in layers}
        p = lambda k: C.c_void_p(out[k].ctypes.data if k in out else 0)
        rc = consumer_shim().rshim_raster(mode, gather, box[0], box[2], W, W * H, z_ref, self.sx.ctypes.data,
                                          self.sy.ctypes.data, self.sz.ctypes.data, self.mean.ctypes.data, self.rough.ctypes.data,
                                          self.flags.ctypes.data, self.row_ncol.ctypes.data, self.ctab_key.ctypes.data, self.ctab_val.ctypes.data,
                                          self.tsize, self.h_bits.ctypes.data, self.state.ctypes.data, p("row"), p("z"), p("rough"), p("nodes"),
                                          p("h"), p("state"))
        assert rc == 0
        if "row" in out:
            out["row"] = out["row"].view(np.int32)
        return out

    def want(self, box, mode, z_ref=0.0):
        """the raster's numpy restatement (tests/raster_ref.py) on the same rows and cost map"""
        from tests import raster_ref as rr
        return rr.raster(self.cells, box, mode, z_ref, self.h_bits[:self.n], self.state[:self.n])

    def passes(self, o, pts, max_range=0.0, end_margin=0.0, ext=True):
        """count-only passes of the rays from o to pts -> (per-row words, rays, skipped)"""
        pts = np.ascontiguousarray(pts, np.float32)
        oo = np.ascontiguousarray(o, np.float32)
        words = np.zeros(max(self.n, 1), np.uint32)
        extent = np.zeros((max(self.n, 1), 2), np.int32)
        stats = np.zeros(2, np.uint64)
        consumer_shim().cshim_passes(self.origin.ctypes.data, self.P["grid_len"], self.P["z_len"], oo.ctypes.data, pts.ctypes.data, len(pts),
                                     pts.shape[1], max_range, end_margin, int(ext), self.sx.ctypes.data, self.sy.ctypes.data,
                                     self.sz.ctypes.data, self.row_ncol.ctypes.data, self.n, self.ctab_key.ctypes.data,
                                     self.ctab_val.ctypes.data, self.tsize, extent.ctypes.data, words.ctypes.data, stats.ctypes.data)
        return words[:self.n], int(stats[0]), int(stats[1])


_DSO = os.path.join(_HERE, "_device_math_shim.so")
_dlib = None
DSHIM_ENTRIES = ("point_keys", "point_keys_fast", "key_offset", "centres", "finalize", "mean_z_n", "min_eigen", "jacobi",
                 "rough_normal", "cost_angle", "cost_travel", "ints")


def build_device_shim(so_path=_DSO, force=False):
    """Compile tests/device_math_shim.hip with libgndt's own hipcc flags (_lib.HIPCC_FLAGS) and link it like libgndt, against the
    HIP runtime the process shares with torch.  Cross-compiles without a GPU.  Returns the compile command."""
    from grid_ndt_amd import _lib
    src = os.path.join(_HERE, "device_math_shim.hip")
    obj = os.path.splitext(so_path)[0] + ".o"
    cmd = ([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + _lib.HIPCC_FLAGS
           + ["-I", os.path.join(_ROOT, "include"), "-I", _lib._CSRC, "-o", obj, src] + os.environ.get("GNDT_EXTRA_CXXFLAGS", "").split())
    deps = [src, os.path.abspath(__file__), os.path.abspath(_lib.__file__)] + \
        [h if os.path.isabs(h) else os.path.join(_lib._CSRC, h) for h in _lib.HEADERS]
    if force or not os.path.exists(so_path) or os.path.getmtime(so_path) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(cmd)
        libdir = _lib._hip_runtime_dir()
        tmp = so_path + ".tmp.so"
        subprocess.check_call(["g++", "-shared", "-o", tmp, obj, "-L", libdir, "-l:libamdhip64.so", "-Wl,-rpath," + libdir,
                               "-Wl,--no-undefined", "-Wl,--strip-all", "-lpthread", "-ldl"])
        os.replace(tmp, so_path)
    return cmd


def device_shim():
    """The device twin of shim(): dshim_<name>(host shim's arguments with device pointers, stream) -> hipError_t."""
    global _dlib
    if _dlib is None:
        from grid_ndt_amd import _lib
        _lib.lib()                   # torch's HIP runtime first: the shim must bind to the one libgndt and torch use
        build_device_shim()
        _dlib = C.CDLL(_DSO)
        for name in DSHIM_ENTRIES:
            getattr(_dlib, "dshim_" + name).restype = C.c_int
    return _dlib


def call(backend, name, *args):
    """shim_<name>(*args) on the host, or dshim_<name> on the current torch stream: numpy arguments are copied to the device and,
    after a synchronise, back into the same arrays (outputs are filled in place either way).  Other arguments go as they are."""
    if backend == "host":
        return getattr(shim(), "shim_" + name)(*[C.c_void_p(a.ctypes.data) if isinstance(a, np.ndarray) else a for a in args])
    import torch
    L = device_shim()
    dev = {}
    for i, a in enumerate(args):
        if isinstance(a, np.ndarray):
            assert a.flags.c_contiguous
            dev[i] = torch.from_numpy(a.reshape(-1).view(np.uint8)).cuda()
    stream = torch.cuda.current_stream()
    rc = getattr(L, "dshim_" + name)(*[C.c_void_p(dev[i].data_ptr()) if i in dev else a for i, a in enumerate(args)],
                                     C.c_void_p(stream.cuda_stream))
    assert rc == 0, f"dshim_{name}: hipError {rc}"
    stream.synchronize()
    for i, t in dev.items():
        args[i].reshape(-1).view(np.uint8)[:] = t.cpu().numpy()


def unpack(keys):
    k = keys.astype(np.uint64)
    sx = ((k >> np.uint64(43)) & np.uint64(0x1FFFFF)).astype(np.int64) - (1 << 20)
    sy = ((k >> np.uint64(22)) & np.uint64(0x1FFFFF)).astype(np.int64) - (1 << 20)
    sz = (k & np.uint64(0x3FFFFF)).astype(np.int64) - (1 << 21)
    return sx.astype(np.int32), sy.astype(np.int32), sz.astype(np.int32)


def point_columns(body, origin, grid_len, z_len):
    """(sx, sy) of every point: the column part of the kernels' own key."""
    L = shim()
    body = np.ascontiguousarray(body, np.float32)
    n, stride = body.shape
    o = (C.c_float * 3)(*[float(v) for v in origin])
    keys = np.zeros(n, np.uint64)
    ok = np.zeros(n, np.uint8)
    L.shim_point_keys(C.c_void_p(body.ctypes.data), C.c_uint64(n), C.c_int(stride), o, C.c_float(grid_len),
                      C.c_float(z_len), C.c_void_p(keys.ctypes.data), C.c_void_p(ok.ctypes.data))
    assert ok.all()
    sx, sy, _ = unpack(keys)
    return sx, sy


def accumulate(body, origin, grid_len, z_len, first_base=0, idx=None):
    """points -> (unique keys, count, first_idx, sums[.,9]) — what k_accumulate leaves in the table.
    `idx`: explicit global index of every point (records of an owner-partitioned build) instead of first_base + position."""
    L = shim()
    body = np.ascontiguousarray(body, np.float32)
    n, stride = body.shape
    o = (C.c_float * 3)(*[float(v) for v in origin])
    keys = np.zeros(n, np.uint64)
    ok = np.zeros(n, np.uint8)
    L.shim_point_keys(C.c_void_p(body.ctypes.data), C.c_uint64(n), C.c_int(stride), o, C.c_float(grid_len),
                      C.c_float(z_len), C.c_void_p(keys.ctypes.data), C.c_void_p(ok.ctypes.data))
    assert ok.all()
    uk, inv = np.unique(keys, return_inverse=True)
    cen = np.zeros((uk.size, 3), np.float64)
    L.shim_centres(C.c_void_p(uk.ctypes.data), C.c_uint64(uk.size), o, C.c_float(grid_len), C.c_float(z_len),
                   C.c_void_p(cen.ctypes.data))
    v = body[:, :3].astype(np.float64) - cen[inv]
    q = np.stack([v[:, 0], v[:, 1], v[:, 2], v[:, 0] * v[:, 0], v[:, 0] * v[:, 1], v[:, 0] * v[:, 2],
                  v[:, 1] * v[:, 1], v[:, 1] * v[:, 2], v[:, 2] * v[:, 2]], 1)
    sums = np.zeros((uk.size, 9), np.float64)
    np.add.at(sums, inv, q)
    count = np.bincount(inv, minlength=uk.size).astype(np.uint32)
    first = np.full(uk.size, np.iinfo(np.int64).max, np.int64)
    np.minimum.at(first, inv, (np.arange(n, dtype=np.int64) + first_base) if idx is None else np.asarray(idx, np.int64))
    return uk, count, first.astype(np.uint32), sums, cen


def finalize(uk, count, first, sums, cen, slope_interval, demand="slope", min_points=3):
    """table contents -> export dict in the reference's order (k_scan/k_label/sort/k_emit)."""
    L = shim()
    n = uk.size
    sx, sy, sz = unpack(uk)
    mean = np.zeros((n, 3), np.float32)
    cov = np.zeros((n, 6), np.float32)
    rough = np.zeros(n, np.float32)
    normal = np.zeros((n, 3), np.float32)
    count = np.ascontiguousarray(count, np.uint32)
    sums = np.ascontiguousarray(sums)
    cen = np.ascontiguousarray(cen)
    L.shim_finalize(C.c_void_p(count.ctypes.data), C.c_void_p(sums.ctypes.data), C.c_void_p(cen.ctypes.data),
                    C.c_uint64(n), C.c_int(min_points), C.c_void_p(mean.ctypes.data), C.c_void_p(cov.ctypes.data),
                    C.c_void_p(rough.ctypes.data), C.c_void_p(normal.ctypes.data))
    has = count >= min_points
    mean_z = np.where(has, mean[:, 2], np.float32(0)).astype(np.float32)
    lookup = {int(k): i for i, k in enumerate(uk)}
    colkey = uk & ~np.uint64(0x3FFFFF)
    col_first = {}
    for i in range(n):
        ck = int(colkey[i])
        f = int(first[i])
        if ck not in col_first or f < col_first[ck]:
            col_first[ck] = f
    flags = has.astype(np.uint32)
    iv = np.float32(slope_interval)

    def pack(x, y, z):
        return ((x + (1 << 20)) << 43) | ((y + (1 << 20)) << 22) | (z + (1 << 21))

    for i in range(n):
        if not has[i]:
            continue
        slope, down = True, False
        if demand == "slope":
            up = False
            z = int(sz[i])
            for target, is_up in ((L.shim_level_above(z), True), (L.shim_level_below(z), False)):
                j = lookup.get(pack(int(sx[i]), int(sy[i]), target))
                if j is None:
                    continue
                visited = first[j] < first[i] and has[j]
                oz = mean_z[j] if visited else np.float32(0)
                if np.abs(np.float32(oz - mean_z[i])) > iv:
                    if is_up:
                        up = True
                    else:
                        down = True
            slope = not up
        if slope:
            flags[i] |= 2
            if down:
                flags[i] |= 4
    cf = np.array([col_first[int(c)] for c in colkey], np.int64)
    order = np.lexsort((first.astype(np.int64), cf))
    out = {"sx": sx[order], "sy": sy[order], "sz": sz[order], "count": count[order], "first_idx": first[order],
           "mean": mean[order], "cov": cov[order], "rough": rough[order], "normal": normal[order], "flags": flags[order],
           "num_nodes": n, "num_columns": len(col_first), "num_slopes": int(np.count_nonzero(flags & 2))}
    return out


def build(cloud, grid_len, z_len, slope_interval, demand="slope"):
    t = accumulate(cloud[1:], cloud[0, :3], grid_len, z_len)
    return finalize(*t, slope_interval, demand)


def cost_levelsync(cells, grid_len, slope_interval, goal_key, demand="slope", robot=None):
    """The level-synchronous flood of gndt_cost.hpp run on the host (same per-slope code as the kernels).
    `goal_key` = (sx, sy, sz) of the goal.  Returns dict(rc, h, state, traversable, closed, check_pushes, ring,
    levels, ring_overflow)."""
    rb = dict(radius=0.25, reachable_height=0.15, max_rough=100.0, max_angle_deg=30.0)
    rb.update(robot or {})
    n = int(len(cells["sx"]))
    arr = {k: np.ascontiguousarray(cells[k], dtype=t) for k, t in
           (("sx", np.int32), ("sy", np.int32), ("sz", np.int32), ("mean", np.float32), ("normal", np.float32),
            ("rough", np.float32), ("flags", np.uint32))}
    h = np.zeros(n, np.float32)
    state = np.zeros(n, np.uint8)
    stats = np.zeros(8, np.int64)
    r4 = (C.c_float * 4)(float(rb["radius"]), float(rb["reachable_height"]), float(rb["max_rough"]), float(rb["max_angle_deg"]))
    L = shim()
    L.shim_cost.restype = C.c_int
    L.shim_cost.argtypes = [C.c_uint64] + [C.c_void_p] * 7 + [C.c_float, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int,
                            C.POINTER(C.c_float), C.c_void_p, C.c_void_p, C.c_void_p]
    dem = {"slope": 0, "true": 1}[demand] if isinstance(demand, str) else int(demand)
    rc = L.shim_cost(n, *[arr[k].ctypes.data for k in ("sx", "sy", "sz", "mean", "normal", "rough", "flags")],
                     float(slope_interval), dem, float(grid_len), int(goal_key[0]), int(goal_key[1]), int(goal_key[2]), r4,
                     h.ctypes.data, state.ctypes.data, stats.ctypes.data)
    return {"rc": rc, "h": h, "state": state, "traversable": int(stats[0]), "closed": int(stats[1]),
            "check_pushes": int(stats[2]), "ring": int(stats[3]), "levels": int(stats[4]), "ring_overflow": int(stats[5]),
            "records": int(stats[6]), "records_more": int(stats[7])}


def collide_all(cells, grid_len, slope_interval, demand="slope", robot=None, ring_cap=1 << 16):
    """CollisionCheck for every slope of `cells`, by the walk over the ring (cost_collide: the restatement of map2D.h:351-474) and by
    the rounds over the whole map the device runs instead (gndt_cost.hpp).  Returns (ring depth, walk, rounds): uint8 arrays, 1
    collide / 0 free / 255 not a slope (walk 2: the ring did not fit ring_cap)."""
    rb = dict(radius=0.25, reachable_height=0.15, max_rough=100.0, max_angle_deg=30.0)
    rb.update(robot or {})
    n = int(len(cells["sx"]))
    arr = {k: np.ascontiguousarray(cells[k], dtype=t) for k, t in
           (("sx", np.int32), ("sy", np.int32), ("sz", np.int32), ("mean", np.float32), ("normal", np.float32),
            ("rough", np.float32), ("flags", np.uint32))}
    walk = np.zeros(n, np.uint8)
    rounds = np.zeros(n, np.uint8)
    r4 = (C.c_float * 4)(float(rb["radius"]), float(rb["reachable_height"]), float(rb["max_rough"]), float(rb["max_angle_deg"]))
    L = shim()
    L.shim_collide_all.restype = C.c_int
    L.shim_collide_all.argtypes = [C.c_uint64] + [C.c_void_p] * 7 + [C.c_float, C.c_int, C.c_float, C.POINTER(C.c_float), C.c_int,
                                   C.c_void_p, C.c_void_p]
    dem = {"slope": 0, "true": 1}[demand] if isinstance(demand, str) else int(demand)
    ring = L.shim_collide_all(n, *[arr[k].ctypes.data for k in ("sx", "sy", "sz", "mean", "normal", "rough", "flags")],
                              float(slope_interval), dem, float(grid_len), r4, int(ring_cap), walk.ctypes.data, rounds.ctypes.data)
    return ring, walk, rounds
