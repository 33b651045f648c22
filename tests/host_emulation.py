"""CPU emulation of libgndt's pipeline built from the SAME arithmetic header the kernels use
(grid_ndt_amd/csrc/gndt_math.hpp via tests/host_math_shim.cpp) plus numpy for the data movement.
It lets the CPU test tier check the kernel maths, the order-free restatement of the slope label and
the parity tolerances against the oracle.  Test infrastructure only."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_SO = os.path.join(_HERE, "_host_math_shim.so")
_lib = None


_CSRC = os.path.join(_ROOT, "grid_ndt_amd", "csrc")


class ShimMap(C.Structure):
    """tests/shim_map.hpp's struct of the same name, field for field (load_shim checks it against every shim that takes one)"""
    _fields_ = [("n", C.c_uint64), ("sx", C.c_void_p), ("sy", C.c_void_p), ("sz", C.c_void_p), ("mean", C.c_void_p), ("normal", C.c_void_p),
                ("rough", C.c_void_p), ("flags", C.c_void_p), ("count", C.c_void_p), ("cov", C.c_void_p), ("row_ncol", C.c_void_p),
                ("ctab_key", C.c_void_p), ("ctab_val", C.c_void_p), ("ctab_size", C.c_uint32), ("h_bits", C.c_void_p), ("state", C.c_void_p),
                ("origin", C.c_float * 3), ("grid_len", C.c_float), ("z_len", C.c_float), ("slope_interval", C.c_float),
                ("demand_true", C.c_int32)]


MAP = C.POINTER(ShimMap)      # a shim's `const ShimMap*` argument


def shim_deps(*sources):
    """what a shim's binary is built from: its sources, tests/shim_map.hpp and every header of grid_ndt_amd/csrc (whichever of them it
    includes, directly or not)"""
    return list(sources) + [os.path.join(_HERE, "shim_map.hpp")] + sorted(glob.glob(os.path.join(_CSRC, "*.hpp")))


def check_shim_map(L, mirror=ShimMap):
    """the layout shim L was compiled with (shim_map.hpp's shim_map_layout / shim_map_fields) against the ctypes mirror"""
    L.shim_map_fields.restype = C.c_char_p
    words = (C.c_uint32 * 64)()
    k = L.shim_map_layout(words)
    names = L.shim_map_fields().decode().split()
    assert names == [f[0] for f in mirror._fields_], ("ShimMap: the fields of tests/shim_map.hpp and of the mirror differ", names)
    want = [C.sizeof(mirror)] + [v for f in names for v in (getattr(mirror, f).offset, getattr(mirror, f).size)]
    assert list(words[:k]) == want, ("ShimMap: the layout of tests/shim_map.hpp and of the mirror differ", list(words[:k]), want)


def load_shim(src, so_name, signatures):
    """tests/<src> compiled with g++ into tests/<so_name> (again when one of shim_deps is newer) and loaded, its ShimMap checked
    against the mirror if it takes one; signatures: {function: (argtypes, restype)}"""
    src, so = os.path.join(_HERE, src), os.path.join(_HERE, so_name)
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in shim_deps(src)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I", _CSRC, "-o", so, src])
    L = C.CDLL(so)
    if hasattr(L, "shim_map_layout"):
        check_shim_map(L)
    for name, (argtypes, restype) in signatures.items():
        getattr(L, name).argtypes = argtypes
        getattr(L, name).restype = restype
    return L


def shim():
    global _lib
    if _lib is None:
        _lib = load_shim("host_math_shim.cpp", os.path.basename(_SO), {"shim_mean_z": ([C.c_uint32, C.c_double, C.c_double], C.c_float)})
    return _lib


_clib = None


def consumer_shim():
    """tests/consumer_shim.cpp: the queries', the raster export's and free-space clearing's per-element code, built for the host"""
    global _clib
    if _clib is None:
        vp, f, i32, u32, u64 = C.c_void_p, C.c_float, C.c_int32, C.c_uint32, C.c_uint64
        _clib = load_shim("consumer_shim.cpp", "_consumer_shim.so", {
            "build_index": ([vp, vp, vp, u64, vp, vp, u32], None),
            "qshim_query": ([C.c_int, C.c_int, C.c_int, vp, u32, u64, MAP, u64, vp, vp, vp], C.c_int),
            "qshim_ctab_find": ([vp, vp, u32, i32, i32], u32),
            "rshim_index": ([i32, u32], C.c_int),
            "rshim_count": ([i32, i32], u32),
            "rshim_raster": ([C.c_int, u32, i32, i32, u32, u32, f, MAP] + [vp] * 6, C.c_int),
            "cshim_walk": ([vp, f, f, vp, vp, f, f, vp, i32], C.c_int),
            "cshim_passes": ([vp, vp, u64, u32, f, f, C.c_int, MAP, vp, vp, vp], None),
        })
    return _clib


def table_slots(columns, table="library"):
    """the column index's slots for a map of `columns` columns: "library" = column_index's rule (a power of two, at least 1024, load
    <= 1/2), "tight" = the smallest power of two with a free slot (long probe chains: ctab_find), a number = that many"""
    if not isinstance(table, str):
        assert table > columns and table & (table - 1) == 0
        return int(table)
    slots, least = (1024, 2 * columns) if table == "library" else (1, columns + 1)
    while slots < least:
        slots <<= 1
    return slots


class MapRows:
    """A map's rows as contiguous arrays of the dtypes the shims read (None: `cells` has no such array, a null pointer in the shim), the
    per-row column sizes, the column index built once with table_slots(., table), the grid's origin and parameters P where the caller
    has them, and the ShimMap that takes all of it into a shim."""
    ROWS = (("sx", np.int32), ("sy", np.int32), ("sz", np.int32), ("mean", np.float32), ("normal", np.float32), ("rough", np.float32),
            ("flags", np.uint32), ("count", np.uint32), ("cov", np.float32))
    OTHERS = (("row_ncol", np.uint32), ("ctab_key", np.uint64), ("ctab_val", np.uint32), ("h_bits", np.uint32), ("state", np.uint32))

    def __init__(self, cells, row_ncol, table="library", origin=(0.0, 0.0, 0.0), P=None, h_bits=None, state=None):
        self.cells, self.P = cells, P or {}
        self.origin = np.asarray(origin, np.float32)[:3]
        for k, t in self.ROWS:
            setattr(self, k, np.ascontiguousarray(cells[k], t) if k in cells else None)
        self.n = int(cells["num_nodes"]) if "num_nodes" in cells else len(self.sx)
        self.row_ncol = np.ascontiguousarray(row_ncol, np.uint32)
        self.h_bits, self.state = h_bits, state
        self.tsize = table_slots(int((self.row_ncol > 0).sum()), table)
        self.ctab_key = np.zeros(self.tsize, np.uint64)
        self.ctab_val = np.zeros(self.tsize, np.uint32)
        consumer_shim().build_index(self.sx.ctypes.data, self.sy.ctypes.data, self.row_ncol.ctypes.data, self.n, self.ctab_key.ctypes.data,
                                    self.ctab_val.ctypes.data, self.tsize)

    def shim_map(self, **over):
        """the ShimMap of these rows (it keeps its arrays alive); over: a field's value in place of the map's own — an array (h_bits=...),
        None for a null pointer, the grid of a map that was made without one (origin=..., grid_len=..., z_len=...)"""
        P = self.P
        val = dict(n=self.n, ctab_size=self.tsize, origin=self.origin, grid_len=P.get("grid_len", 0.0), z_len=P.get("z_len", 0.0),
                   slope_interval=P.get("slope_interval", 0.0), demand_true=int(P.get("demand", "slope") == "true"))
        val.update({k: getattr(self, k) for k, _ in self.ROWS + self.OTHERS})
        assert set(over) <= set(val), over.keys()
        val.update(over)
        m = ShimMap()
        m.keep = []
        for k, t in self.ROWS + self.OTHERS:
            a = val[k]
            if a is not None:
                a = np.ascontiguousarray(a)
                assert a.dtype == t, (k, a.dtype)       # (an array of another type would be read as this one)
                m.keep.append(a)
                val[k] = a.ctypes.data
        val["origin"] = (C.c_float * 3)(*[float(v) for v in val["origin"]])
        for k, v in val.items():
            setattr(m, k, v)
        return m


class HostMap(MapRows):
    """The rows of an oracle map, with the per-row column sizes, the column index derived on the host (table_slots) and a made-up cost
    map drawn from `seed`; run through consumer_shim()"""

    def __init__(self, cloud, P, table="library", seed=11):
        from oracle import oracle
        from tests import query_ref as qr
        c = oracle.build_grid(cloud, P["grid_len"], P["z_len"], P["slope_interval"], P.get("demand", "slope"), mode=oracle.MODE_INT_OPENMP)
        super().__init__(c, qr.row_ncol(c), table, origin=cloud[0, :3], P=P)
        assert int((self.row_ncol > 0).sum()) == int(c["num_columns"])
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
        rc = consumer_shim().qshim_query(mode, ilp, int(gather), pts.ctypes.data, pts.shape[1], n, self.shim_map(), threads, rows.ctypes.data,
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
        rc = consumer_shim().rshim_raster(mode, gather, box[0], box[2], W, W * H, z_ref, self.shim_map(), p("row"), p("z"), p("rough"),
                                          p("nodes"), p("h"), p("state"))
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
        consumer_shim().cshim_passes(oo.ctypes.data, pts.ctypes.data, len(pts), pts.shape[1], max_range, end_margin, int(ext), self.shim_map(),
                                     extent.ctypes.data, words.ctypes.data, stats.ctypes.data)
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
