"""ctypes binding of libgndt.so (the C ABI declared in include/gndt.h).

The shared library is built in-tree by `build_native()` (hipcc, gfx950).  There is no Python or CPU
implementation of the path behind it: if the library is missing, loading raises.
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# Build variants of the library: None is the product; "poison" is the same sources and flags plus -DGNDT_POISON (gndt_handle.hpp: every
# device and pinned host allocation filled with a byte before it is handed out), objects in a directory of its own.  A process chooses
# its variant with the environment variable GNDT_LIB_VARIANT, read HERE (the C library reads no environment variable); unset or
# empty, everything is the product's: same path, same commands.
VARIANTS = {None: {"lib": "libgndt.so", "objdir": None, "flags": []},
            "poison": {"lib": "libgndt_poison.so", "objdir": "obj_poison", "flags": ["-DGNDT_POISON"]}}
VARIANT = os.environ.get("GNDT_LIB_VARIANT") or None
if VARIANT not in VARIANTS:
    raise ImportError(f"GNDT_LIB_VARIANT={VARIANT!r}: the variants are {sorted(v for v in VARIANTS if v)}")


def lib_path(variant=None):
    """Path of a variant's shared library (None or "": the product's libgndt.so)."""
    return os.path.join(_CSRC, VARIANTS[variant or None]["lib"])


LIB_PATH = lib_path(VARIANT)   # what lib() loads in this process
SOURCES = ["gndt_api_core.hip", "gndt_api_table.hip", "gndt_api_build.hip", "gndt_api_dist.hip", "gndt_api_cost.hip", "gndt_api_query.hip",
           "gndt_api_crop.hip", "gndt_api_raster.hip", "gndt_api_clear.hip", "gndt_api_score.hip", "gndt_api_score_maps.hip", "gndt_api_cast.hip", "gndt_api_view.hip", "gndt_api_coarsen.hip", "gndt_api_merge.hip", "gndt_api_plan.hip", "gndt_api_frontier.hip", "gndt_api_patch.hip", "gndt_api_segment.hip", "gndt_api_clearance.hip", "gndt_api_obstacle.hip", "gndt_api_route_field.hip", "gndt_api_walk.hip", "gndt_api_shortcut.hip", "gndt_api_footprint.hip", "gndt_api_io.hip", "gndt_codec.cpp", "gndt_io.cpp"]
HEADERS = ["gndt_handle.hpp", "gndt_kernels.hpp", "gndt_table.hpp", "gndt_cost.hpp", "gndt_query.hpp", "gndt_ray.hpp", "gndt_score.hpp", "gndt_score_derivs.hpp", "gndt_score_maps.hpp", "gndt_cast.hpp", "gndt_view.hpp", "gndt_plan.hpp", "gndt_frontier.hpp", "gndt_patch.hpp", "gndt_segment.hpp", "gndt_clearance.hpp", "gndt_obstacle.hpp", "gndt_route_field.hpp", "gndt_walk.hpp", "gndt_shortcut.hpp", "gndt_footprint.hpp", "gndt_coarsen.hpp", "gndt_merge.hpp", "gndt_crop.hpp", "gndt_pack.hpp", "gndt_partition.hpp", "gndt_stream.hpp", "gndt_bucket3.hpp", "gndt_blocked.hpp", "gndt_tile.hpp", "gndt_exchange.hpp", "gndt_math.hpp", "gndt_scratch.hpp", os.path.join(_ROOT, "include", "gndt.h")]

GNDT_OK = 0
ERR_NAMES = {0: "OK", 1: "INVALID", 2: "NO_DEVICE", 3: "HIP", 4: "KEY_RANGE", 5: "CAPACITY", 6: "NOMEM", 7: "PEER"}


class GndtError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"gndt error {code} ({ERR_NAMES.get(code, '?')}): {msg}")
        self.code = code


class Params(C.Structure):
    _fields_ = [("grid_len", C.c_float), ("z_len", C.c_float), ("slope_interval", C.c_float),
                ("demand", C.c_int32), ("min_points", C.c_int32), ("device_id", C.c_int32),
                ("strategy", C.c_int32), ("max_points_hint", C.c_uint64), ("max_nodes_hint", C.c_uint64)]


class Cells(C.Structure):
    _fields_ = [("num_nodes", C.c_uint64), ("num_columns", C.c_uint64), ("num_slopes", C.c_uint64),
                ("sx", C.c_void_p), ("sy", C.c_void_p), ("sz", C.c_void_p), ("count", C.c_void_p),
                ("first_idx", C.c_void_p), ("mean", C.c_void_p), ("cov", C.c_void_p), ("rough", C.c_void_p),
                ("normal", C.c_void_p), ("flags", C.c_void_p)]


class Robot(C.Structure):
    _fields_ = [("radius", C.c_float), ("reachable_height", C.c_float), ("max_rough", C.c_float), ("max_angle_deg", C.c_float)]


class CostStats(C.Structure):
    _fields_ = [("goal_status", C.c_int32), ("ring", C.c_uint32), ("levels", C.c_uint32), ("ring_store", C.c_uint32),
                ("traversable", C.c_uint64), ("closed", C.c_uint64), ("check_pushes", C.c_uint64)]


class CropBox(C.Structure):
    _fields_ = [("sx_min", C.c_int32), ("sx_max", C.c_int32), ("sy_min", C.c_int32), ("sy_max", C.c_int32)]


class RasterLayers(C.Structure):
    _fields_ = [("row", C.c_void_p), ("z", C.c_void_p), ("rough", C.c_void_p), ("nodes", C.c_void_p), ("h", C.c_void_p), ("state", C.c_void_p)]


class ClearParams(C.Structure):
    _fields_ = [("max_range", C.c_float), ("end_margin", C.c_float), ("min_passes", C.c_uint32), ("flags", C.c_uint32)]


class ClearStats(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("skipped", C.c_uint64), ("protected_rows", C.c_uint64), ("cleared", C.c_uint64)]


class ScoreParams(C.Structure):
    _fields_ = [("neighbourhood", C.c_int32), ("min_count", C.c_int32), ("cov_rel", C.c_float), ("cov_floor", C.c_float),
                ("max_d2", C.c_float), ("point_pose", C.c_uint32)]


class PoseDerivs(C.Structure):      # (the per-item records are RECORDS' dtypes below; this one mirror stays for the GPU tier, which reads its size)
    _fields_ = [("score", C.c_double), ("d2_sum", C.c_double), ("matched", C.c_uint64), ("terms", C.c_uint64),
                ("g", C.c_double * 6), ("H", C.c_double * 21)]


class CastParams(C.Structure):
    _fields_ = [("mode", C.c_int32), ("min_count", C.c_int32), ("max_range", C.c_float), ("min_range", C.c_float),
                ("cov_rel", C.c_float), ("cov_floor", C.c_float), ("max_d2", C.c_float), ("reserved", C.c_uint32)]


class CastOut(C.Structure):
    _fields_ = [("row", C.c_void_p), ("range", C.c_void_p), ("d2", C.c_void_p)]


class CastStats(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("skipped", C.c_uint64), ("hits", C.c_uint64)]


class ViewParams(C.Structure):
    _fields_ = [("max_range", C.c_float), ("min_range", C.c_float), ("min_count", C.c_int32), ("reserved", C.c_uint32 * 5)]


class PlanParams(C.Structure):
    _fields_ = [("start_mode", C.c_int32), ("max_expansions", C.c_uint32), ("scratch_bytes", C.c_uint64), ("reserved", C.c_uint32 * 4)]


class FrontierParams(C.Structure):
    _fields_ = [("candidates", C.c_int32), ("open_rule", C.c_int32), ("level_reach", C.c_uint32), ("min_open", C.c_uint32),
                ("link_dz", C.c_uint32), ("min_size", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class PatchParams(C.Structure):
    _fields_ = [("candidates", C.c_int32), ("connectivity", C.c_uint32), ("cos_min", C.c_float), ("max_offset", C.c_float),
                ("max_var", C.c_float), ("cos_level", C.c_float), ("sin_level", C.c_float), ("min_size", C.c_uint32),
                ("reserved", C.c_uint32 * 4)]


class SegmentParams(C.Structure):
    _fields_ = [("neighbourhood", C.c_int32), ("min_count", C.c_int32), ("cov_rel", C.c_float), ("cov_floor", C.c_float),
                ("novel_d2", C.c_float), ("classes", C.c_uint32), ("min_points", C.c_uint32), ("connectivity", C.c_uint32),
                ("min_cluster_points", C.c_uint32), ("min_cluster_cells", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class ClearanceParams(C.Structure):
    _fields_ = [("sources", C.c_uint32), ("max_hops", C.c_uint32), ("reserved", C.c_uint32 * 6)]


class ObstacleParams(C.Structure):
    _fields_ = [("inflate", C.c_uint32), ("max_hops", C.c_uint32), ("levels_above", C.c_uint32), ("levels_below", C.c_uint32),
                ("max_columns", C.c_uint64), ("reserved", C.c_uint32 * 2)]


class RouteFieldParams(C.Structure):
    _fields_ = [("checks", C.c_uint32), ("min_hops", C.c_uint32), ("soft_hops", C.c_uint32), ("soft_weight", C.c_float),
                ("max_cost", C.c_float), ("max_rounds", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class DescendParams(C.Structure):
    _fields_ = [("start_mode", C.c_int32), ("max_steps", C.c_uint32), ("reserved", C.c_uint32 * 6)]


class WalkParams(C.Structure):
    _fields_ = [("start_mode", C.c_int32), ("checks", C.c_uint32), ("min_hops", C.c_uint32), ("max_steps", C.c_uint32),
                ("reserved", C.c_uint32 * 4)]


class ShortcutParams(C.Structure):
    _fields_ = [("window", C.c_uint32), ("checks", C.c_uint32), ("min_hops", C.c_uint32), ("max_links", C.c_uint32),
                ("reserved", C.c_uint32 * 4)]


class FootprintParams(C.Structure):
    _fields_ = [("half_length", C.c_float), ("half_width", C.c_float), ("max_dz", C.c_float), ("height", C.c_float),
                ("min_cells", C.c_uint32), ("min_cover", C.c_float), ("weight", C.c_uint32), ("reserved", C.c_uint32 * 5)]


class MergeParams(C.Structure):
    _fields_ = [("min_count", C.c_int32), ("reserved", C.c_uint32)]


class MergeStats(C.Structure):
    _fields_ = [("source_nodes", C.c_uint64), ("merged_nodes", C.c_uint64), ("merged_points", C.c_uint64),
                ("below_min_count", C.c_uint64), ("skipped", C.c_uint64), ("new_nodes", C.c_uint64)]


class PointLayout(C.Structure):
    _fields_ = [("point_step", C.c_uint32), ("offset_x", C.c_uint32), ("offset_y", C.c_uint32), ("offset_z", C.c_uint32)]


class Pcd(C.Structure):
    _fields_ = [("num_points", C.c_uint64), ("layout", PointLayout), ("data_kind", C.c_int32), ("reserved", C.c_int32),
                ("data", C.c_void_p)]


class Stats(C.Structure):
    _fields_ = [("num_nodes", C.c_uint64), ("key", C.c_void_p), ("sums", C.c_void_p), ("count", C.c_void_p),
                ("first_idx", C.c_void_p)]


class ExchangeTimes(C.Structure):
    _fields_ = [("shard_ms", C.c_float), ("exchange_ms", C.c_float), ("finalize_ms", C.c_float), ("ranks", C.c_uint32),
                ("local_nodes", C.c_uint64), ("global_nodes", C.c_uint64), ("bytes_reduced", C.c_uint64)]


class CommSelftest(C.Structure):
    _fields_ = [("all_gather_ms", C.c_float), ("exchange_ms", C.c_float), ("reduce_scatter_ms", C.c_float), ("all_reduce_ms", C.c_float),
                ("ok_mask", C.c_uint32), ("ranks", C.c_uint32)]


class OwnedInfo(C.Structure):
    _fields_ = [("owned_points", C.c_uint64), ("local_nodes", C.c_uint64), ("local_columns", C.c_uint64),
                ("global_nodes", C.c_uint64), ("global_columns", C.c_uint64), ("global_slopes", C.c_uint64),
                ("bytes_sent", C.c_uint64), ("bytes_received", C.c_uint64),
                ("split_ms", C.c_float), ("exchange_ms", C.c_float), ("build_ms", C.c_float), ("order_ms", C.c_float),
                ("ranks", C.c_uint32)]


def _hip_runtime_dir():
    """Directory of the HIP runtime libgndt must share with its host process.  PyTorch wheels bundle
    their own libamdhip64.so / libhsa-runtime64.so; linking libgndt against /opt/rocm's copy would put
    a second HIP runtime in the process (foreign streams, events and allocations).  GNDT_HIP_LIBDIR
    overrides (e.g. /opt/rocm/lib for a C++/ROS host without torch)."""
    env = os.environ.get("GNDT_HIP_LIBDIR")
    if env:
        return env
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec and spec.origin:
            d = os.path.join(os.path.dirname(spec.origin), "lib")
            if os.path.exists(os.path.join(d, "libamdhip64.so")):
                return d
    except Exception:
        pass
    return "/opt/rocm/lib"


def source_hash():
    """sha256 over the kernel / host sources libgndt is built from: profiles/ store it next to the PMC figures so that
    bench.py can tell whether a committed HBM-traffic measurement belongs to the code it is timing."""
    import hashlib
    h = hashlib.sha256()
    names = sorted(set(SOURCES + [x for x in HEADERS if not os.path.isabs(x)]))
    for nm in names + [os.path.join(_ROOT, "include", "gndt.h")]:
        with open(nm if os.path.isabs(nm) else os.path.join(_CSRC, nm), "rb") as f:
            h.update(os.path.basename(nm).encode() + b"\0" + f.read())
    return h.hexdigest()


# hipcc flags of every translation unit of libgndt (and of the test tier's device shim of the same headers, tests/host_emulation.py)
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-c",
               "-Wno-unused-command-line-argument", "-Wno-unused-function", "-Wno-pass-failed", "-fno-slp-vectorize",
               # the code objects drop their local symbols (rocPRIM's ~500 instantiations in gndt_api_dist carried 1 MB of them).
               # NOT --strip-all: the HIP runtime segfaults on a code object without .symtab (measured on the MI355X box)
               "-Xoffload-linker", "--discard-all"]


def build_native(force=False, verbose=False, variant=None):
    """Compile the HIP sources into grid_ndt_amd/csrc/libgndt.so for gfx950 (cross-compiles without a GPU).  `variant`: None = the one
    this process loads (GNDT_LIB_VARIANT; the product if unset), "" = the product, "poison" = csrc/libgndt_poison.so."""
    variant = VARIANT if variant is None else (variant or None)
    V, LIB_PATH = VARIANTS[variant], lib_path(variant)
    srcs = [os.path.join(_CSRC, s) for s in SOURCES]
    deps = srcs + [h if os.path.isabs(h) else os.path.join(_CSRC, h) for h in HEADERS] + [os.path.abspath(__file__)]
    if not force and os.path.exists(LIB_PATH) and all(os.path.getmtime(LIB_PATH) >= os.path.getmtime(d) for d in deps):
        return LIB_PATH
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if V["objdir"]:
        os.makedirs(os.path.join(_CSRC, V["objdir"]), exist_ok=True)
    objs, procs = [], []
    for src in srcs:                       # one hipcc per translation unit, side by side (8 small jobs)
        obj = os.path.splitext(src)[0] + ".o"
        if V["objdir"]:
            obj = os.path.join(_CSRC, V["objdir"], os.path.basename(obj))
        cmd = ([hipcc] + HIPCC_FLAGS + V["flags"] + ["-I", os.path.join(_ROOT, "include"), "-I", _CSRC, "-o", obj, src]
               + os.environ.get("GNDT_EXTRA_CXXFLAGS", "").split())
        if verbose:
            print(" ".join(cmd))
        procs.append((cmd, subprocess.Popen(cmd)))
        objs.append(obj)
    for cmd, pr in procs:
        if pr.wait() != 0:
            raise subprocess.CalledProcessError(pr.returncode, cmd)
    libdir = _hip_runtime_dir()
    link = ["g++", "-shared", "-o", LIB_PATH] + objs + ["-L", libdir, "-l:libamdhip64.so", "-Wl,-rpath," + libdir,
                                                         "-Wl,--no-undefined", "-Wl,--strip-all", "-lpthread", "-ldl"]
    if verbose:
        print(" ".join(link))
    subprocess.check_call(link)
    return LIB_PATH


# ---- the per-item records the library writes, each described ONCE: C typedef -> numpy structured dtype (tests/test_abi_layout_host.py
# checks size and offsets against include/gndt.h).  A host twin hands out the fields of a zeroed array of the dtype; a device twin the
# same fields as views of a [K, itemsize / 4] int32 tensor (record_views).  Field dtypes are the ones the host twins return — which is
# why some are signed where the C field is not (rows come back with GNDT_NO_ROW as -1).
ROUTE_INFO = np.dtype([("status", np.int32), ("length", np.uint32), ("start_row", np.uint32), ("expansions", np.uint32),
                       ("queue_peak", np.uint32), ("cost", np.float32), ("h_start", np.float32), ("reserved", np.uint32)])
WALK_INFO = np.dtype([("status", np.int32), ("stop_side", np.int32), ("steps", np.int32), ("waypoints", np.int32),
                      ("start_row", np.int32), ("end_row", np.int32), ("length", np.float32), ("climb", np.float32),
                      ("rough_max", np.float32), ("hops_min", np.int32), ("reserved", np.int32, 2)])
SHORTCUT_INFO = np.dtype([("status", np.int32), ("length_in", np.int32), ("waypoints", np.int32), ("path_slopes", np.int32),
                          ("links_tested", np.int32), ("fallback_links", np.int32), ("cost_in", np.float32),
                          ("cost_out", np.float32), ("hops_min", np.int32), ("reserved", np.int32, 3)])
FOOTPRINT_INFO = np.dtype([("status", np.int32), ("flags", np.uint32), ("centre_row", np.int32), ("cells", np.uint16),
                           ("support", np.uint16), ("gaps", np.uint16), ("unknown", np.uint16), ("z", np.float32),
                           ("normal", np.float32, 3), ("along", np.float32), ("across", np.float32), ("rms", np.float32),
                           ("step_max", np.float32), ("bump_max", np.float32), ("headroom", np.float32), ("reserved", np.uint32)])
VIEW_INFO = np.dtype([("rays", np.uint32), ("skipped", np.uint32), ("hits", np.uint32), ("unknown", np.uint32), ("known", np.uint32),
                      ("status", np.uint32), ("steps", np.uint64), ("sum_ux", np.int64), ("sum_uy", np.int64)])
POSE_SCORE = np.dtype([("score", np.float64), ("d2_sum", np.float64), ("matched", np.int64), ("terms", np.int64)])
POSE_DERIVS = np.dtype(POSE_SCORE.descr + [("g", np.float64, 6), ("H", np.float64, 21)])   # H: the upper triangle, row-major
FRONTIER = np.dtype([("label", np.int32), ("size", np.int32), ("best_row", np.int32), ("best_h", np.float32),
                     ("sx_min", np.int32), ("sx_max", np.int32), ("sy_min", np.int32), ("sy_max", np.int32),
                     ("sum_px", np.int64), ("sum_py", np.int64), ("sum_pz", np.int64), ("open_sides", np.int32), ("reserved", np.int32)])
PATCH = np.dtype([("label", np.int32), ("nodes", np.int32), ("points", np.int64),
                  ("sx_min", np.int32), ("sx_max", np.int32), ("sy_min", np.int32), ("sy_max", np.int32), ("sz_min", np.int32),
                  ("sz_max", np.int32), ("sum_px", np.int64), ("sum_py", np.int64), ("sum_pz", np.int64),
                  ("centroid", np.float64, 3), ("normal", np.float64, 3), ("var", np.float64), ("kind", np.int32), ("reserved", np.int32)])
SCAN_CLUSTER = np.dtype([("label", np.uint32), ("cells", np.uint32), ("off_surface", np.uint32), ("unmapped", np.uint32),
                         ("sx_min", np.int32), ("sx_max", np.int32), ("sy_min", np.int32), ("sy_max", np.int32),
                         ("sz_min", np.int32), ("sz_max", np.int32), ("sum_x", np.int64), ("sum_y", np.int64), ("sum_z", np.int64),
                         ("z_lo", np.float32), ("z_hi", np.float32)])
RECORDS = {"gndt_route_info": ROUTE_INFO, "gndt_walk_info": WALK_INFO, "gndt_shortcut_info": SHORTCUT_INFO,
           "gndt_footprint_info": FOOTPRINT_INFO, "gndt_view_info": VIEW_INFO, "gndt_pose_score": POSE_SCORE,
           "gndt_pose_derivs": POSE_DERIVS, "gndt_frontier": FRONTIER, "gndt_scan_cluster": SCAN_CLUSTER}
# gndt_patch (PATCH above) is described and decoded the same way; tests/test_patch_host.py holds it against the header, since
# tests/test_abi_layout_host.py names the records of this table one by one
PATCH_RECORD = {"gndt_patch": PATCH}


@functools.lru_cache(maxsize=None)
def _record_columns(dtype):
    """the fields of a record but `reserved`, as record_views needs them: (name, bytes of an element, its index among the elements of
    that size (8: among the int64 view's), elements of a sub-array or 0, float?, bit shift of a 2-byte field in its word)"""
    cols = []
    for name in dtype.names:
        if name == "reserved":
            continue
        field, offset = dtype.fields[name][:2]
        base, shape = field.subdtype or (field, ())
        size = base.itemsize
        assert size in (2, 4, 8) and offset % size == 0 and len(shape) <= 1 and (size > 2 or not shape)
        cols.append((name, size, offset // max(size, 4), shape[0] if shape else 0, base.kind == "f", 8 * (offset % 4)))
    return tuple(cols)


@functools.lru_cache(maxsize=None)
def record_fields(dtype):
    """the names a method hands out: the record's but `reserved`"""
    return tuple(c[0] for c in _record_columns(dtype))


@functools.lru_cache(maxsize=None)
def record_is_wide(dtype):
    """every field of the record is 8 bytes (gndt_pose_score, gndt_pose_derivs): its device tensor may be int64 from the start"""
    return all(size == 8 for _, size, _, _, _, _ in _record_columns(dtype))


@functools.lru_cache(maxsize=None)
def _record_decoder(dtype):
    """-> f(raw) -> {field: view} of a device tensor of records: the dict display a method would spell out by hand, written from the
    dtype's offsets once and compiled, so that a call pays no loop over the fields (and no look at torch's module)"""
    import torch
    items, sizes = [], set()
    for name, size, at, count, is_float, shift in _record_columns(dtype):
        sizes.add((size, is_float))
        if size == 2:
            expr = f"(raw[:, {at}] >> {shift}) & 0xFFFF" if shift else f"raw[:, {at}] & 0xFFFF"
        else:
            cols = "raw" if size == 4 else ("wide_f" if is_float else "wide")
            expr = f"{cols}[:, {at}:{at + count}]" if count else f"{cols}[:, {at}]"
            if size == 4 and is_float:
                expr += ".view(f32)"
        items.append(f"{name!r}: {expr}")
    env = {"f32": torch.float32, "i64": torch.int64, "f64": torch.float64}
    body = "{" + ", ".join(items) + "}"
    if (8, False) not in sizes and (8, True) not in sizes:
        return eval("lambda raw: " + body, env)
    # (an int64 tensor is its own wide view; a tensor without rows has nothing to view)
    src = ("def decode(raw):\n"
           "    wide = raw if raw.dtype == i64 else (raw.view(i64) if len(raw) else raw.new_zeros((0, raw.shape[1] // 2), dtype=i64))\n"
           + ("    wide_f = wide.view(f64)\n" if (8, True) in sizes else "")
           + "    return " + body + "\n")
    exec(src, env)
    return env["decode"]


def record_views(raw, dtype):
    """A [K, dtype.itemsize / 4] int32 torch tensor of records (or, for a record of 8-byte fields only, the [K, itemsize / 8] int64
    one) -> {field: view}, every column derived from the dtype's offsets: a 4-byte field is a column (as float32 for a float), an
    8-byte field a column of the int64 view (of its float64 view for a float), a 2-byte field its word shifted and masked (the one
    entry that is computed, not a view), a sub-array a column slice.  Integer fields are int32 / int64 whatever their sign in the
    record: the bits are the library's.  `reserved` is left out."""
    return _record_decoder(dtype)(raw)


def _prototypes():
    """name -> argtypes of every function of include/gndt.h the binding calls (None: left unset).  restype is c_int but for _RESTYPES."""
    vp, sz, u64, u32, i32, H, P = C.c_void_p, C.c_size_t, C.c_uint64, C.c_uint32, C.c_int32, C.c_void_p, C.POINTER
    f32p, i32p, u64p = P(C.c_float), P(i32), P(u64)
    T = {
        "gndt_create": [P(Params), P(H)],
        "gndt_destroy": [H],
        "gndt_last_error": [H],
        "gndt_set_origin": [H, f32p],
        "gndt_get_origin": [H, f32p],
        "gndt_build": [H, vp, sz, sz],
        "gndt_update": [H, vp, sz, sz],
        "gndt_remove": [H, vp, sz, sz],
        "gndt_reset": [H, vp],
        "gndt_accumulate_device": [H, vp, sz, sz, u64, vp],
        "gndt_finalize_device": [H, vp],
        "gndt_sync": [H, u64p, u64p, u64p],
        "gndt_export_device": [H, P(Cells)],
        "gndt_export": [H, P(Cells)],
        "gndt_export_host": [H, P(Cells)],
        "gndt_reserve": [H, u64, u64],
        "gndt_set_deferred_emit": [H, C.c_int],
        "gndt_stats_export_device": [H, P(Stats), vp],
        "gndt_stats_merge_device": [H, P(Stats), vp],
        "gndt_shard_stats_device": [H, vp, sz, sz, u64, P(Stats), vp],
        "gndt_finalize_stats_device": [H, P(Stats), u64, vp],
        "gndt_pcd_read": [C.c_char_p, P(Pcd), C.c_char_p],
        "gndt_pcd_free": [P(Pcd)],
        "gndt_pack_points_device": [H, vp, sz, P(PointLayout), vp, u64p, vp],
        "gndt_build_cloud": [H, vp, sz, P(PointLayout)],
        "gndt_compute_cost": [H, f32p, P(Robot), vp],
        "gndt_cost_export_device": [H, P(vp), P(vp), P(CostStats)],
        "gndt_cost_export": [H, vp, vp, P(CostStats)],
        "gndt_query": [H, vp, sz, sz, i32, vp, vp, vp],
        "gndt_crop": [H, P(CropBox), i32],
        "gndt_crop_box_from_world": [f32p, C.c_float, f32p, f32p, P(CropBox)],
        "gndt_raster_shape": [P(CropBox), P(u32), P(u32)],
        "gndt_raster": [H, P(CropBox), i32, C.c_float, P(RasterLayers)],
        "gndt_clear_rays": [H, f32p, vp, sz, sz, P(ClearParams), vp, P(ClearStats)],
        "gndt_score_poses": [H, vp, sz, sz, vp, u32, P(ScoreParams), vp, vp, vp],
        "gndt_score_derivs": [H, vp, sz, sz, vp, u32, P(ScoreParams), vp],
        "gndt_score_maps_device": [H, H, vp, u32, P(ScoreParams), vp, vp, vp, vp],
        "gndt_score_maps_derivs_device": [H, H, vp, u32, P(ScoreParams), vp, vp],
        "gndt_cast_rays": [H, vp, sz, vp, sz, sz, P(CastParams), P(CastOut), P(CastStats)],
        "gndt_view_gain": [H, vp, sz, vp, sz, sz, P(ViewParams), vp, vp, vp],
        "gndt_plan_routes": [H, vp, sz, sz, P(PlanParams), vp, u32, vp],
        "gndt_frontiers": [H, P(CropBox), P(FrontierParams), vp, vp, u32, vp],
        "gndt_patches": [H, P(CropBox), P(PatchParams), vp, vp, u32, vp],
        "gndt_segment_scan": [H, vp, sz, sz, vp, P(SegmentParams), vp, vp, vp, u32, vp],
        "gndt_clearance": [H, P(Robot), P(ClearanceParams), vp, vp, vp, vp],
        # (the device twin also takes the box count where it lies on the device: not the host's arguments plus a stream)
        "gndt_obstacle_field": [H, P(Robot), vp, u32, sz, P(ObstacleParams), vp, vp, vp, vp],
        "gndt_obstacle_field_device": [H, P(Robot), vp, u32, sz, vp, P(ObstacleParams), vp, vp, vp, vp, vp],
        "gndt_route_field": [H, P(Robot), P(RouteFieldParams), vp, u32, vp, vp, vp, vp, vp],
        "gndt_descend_routes": [H, vp, sz, sz, P(DescendParams), vp, vp, vp, u32, vp],
        "gndt_walk_paths": [H, vp, sz, sz, sz, P(Robot), P(WalkParams), vp, vp, u32, vp],
        "gndt_shortcut_routes": [H, vp, sz, u32, vp, sz, P(Robot), P(ShortcutParams), vp, vp, u32, vp, u32, vp],
        "gndt_footprint_poses": [H, vp, sz, sz, P(Robot), P(FootprintParams), vp, u32, vp],
        "gndt_coarsen_device": [H, H, u32, u32, vp],
        "gndt_merge_map_device": [H, H, vp, P(MergeParams), P(MergeStats), vp],
        "gndt_trans_morton_xyz": [f32p, C.c_float, C.c_float, f32p, C.c_char_p, i32p, i32p, i32p, C.c_char_p],
        "gndt_count_morton": [i32, i32, C.c_char_p],
        "gndt_morton_to_xy": [i32, i32p, i32p],
        "gndt_pack_key": [i32, i32, i32],
        "gndt_unpack_key": [u64, i32p, i32p, i32p],
        "gndt_set_profiling": [H, C.c_int],
        "gndt_get_phase_times": [H, P(C.c_double)],
        "gndt_debug_bucket_phases": [H, P(C.c_double), P(u32)],
        "gndt_debug_retry_count": [H, u64p],
        "gndt_debug_enable_stamps": [C.c_int],
        "gndt_warmup": [H, u64],
        "gndt_debug_set_option": [C.c_int, C.c_double],
        "gndt_debug_poisoned_bytes": [u64p, u64p],
        "gndt_debug_set_fp_bits": [C.c_int],
        "gndt_debug_fp_clashes": [H, u64p],
        "gndt_debug_second_pass_buckets": [H, u64p],
        "gndt_debug_block_layout": [H, i32p],
        "gndt_debug_obstacle_marks": [H, u64p],
        "gndt_debug_fail_next_alloc": [H, C.c_int],
        "gndt_comm_unique_id": [C.c_char_p],
        "gndt_comm_create": [C.c_char_p, i32, i32, i32, P(vp)],
        "gndt_comm_destroy": [vp],
        "gndt_comm_create_threads": [i32, i32, P(vp)],
        "gndt_comm_last_error": None,
        "gndt_comm_selftest": [H, vp, P(CommSelftest), vp],
        "gndt_build_global_device": [H, vp, vp, sz, sz, u64, u64, P(ExchangeTimes), vp],
        "gndt_owner_of_columns": [vp, vp, sz, u32, vp],
        "gndt_owner_sample_device": [H, vp, sz, sz, P(vp), u64p, vp],
        "gndt_owner_map_device": [H, vp, u32, vp],
        "gndt_owner_split_device": [H, vp, sz, sz, u64, u64, u32, P(vp), u64p, u64p, vp],
        "gndt_build_records_device": [H, vp, sz, u64, vp],
        "gndt_build_records2_device": [H, vp, sz, vp, sz, u64, vp],
        "gndt_owned_columns_device": [H, P(vp), u64p, vp],
        "gndt_owned_global_rows_device": [H, vp, u64, u64, P(vp), u64p, u64p, vp],
        "gndt_build_owned_device": [H, vp, vp, sz, sz, u64, u64, P(vp), P(OwnedInfo), vp],
        "gndt_gather_owned_map_device": [H, vp, i32, vp],
        "gndt_owned_pack_rows_device": [H, P(vp), u64p, vp],
        "gndt_adopt_rows_device": [H, vp, u64, u64, u64, u64, vp],
        "gndt_locality_sample": [H, vp, sz, sz, u32, P(C.c_double), vp],
        "gndt_last_strategy": [H],
        "gndt_device_info": [i32, C.c_char_p, i32p, u64p],
    }
    # the device twins whose arguments are the host twin's with the stream behind them
    for name in ("gndt_build", "gndt_update", "gndt_remove", "gndt_query", "gndt_crop", "gndt_raster", "gndt_clear_rays", "gndt_score_poses",
                 "gndt_score_derivs", "gndt_cast_rays", "gndt_view_gain", "gndt_plan_routes", "gndt_frontiers", "gndt_patches", "gndt_segment_scan",
                 "gndt_clearance", "gndt_route_field", "gndt_descend_routes", "gndt_walk_paths", "gndt_shortcut_routes",
                 "gndt_footprint_poses"):
        T[name + "_device"] = T[name] + [vp]
    return T


_RESTYPES = {"gndt_destroy": None, "gndt_last_error": C.c_char_p, "gndt_comm_last_error": C.c_char_p, "gndt_pcd_free": None,
             "gndt_pack_key": C.c_uint64, "gndt_unpack_key": None, "gndt_comm_destroy": None}

_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950).  grid_ndt_amd has no fallback implementation.")
    # One HIP runtime per process: load the copy the host process uses (torch's bundled one when torch
    # is installed) before libgndt, so libgndt's DT_NEEDED libamdhip64.so.7 binds to it by soname.
    rt = os.path.join(_hip_runtime_dir(), "libamdhip64.so")
    if os.path.exists(rt):
        C.CDLL(rt, mode=C.RTLD_GLOBAL)
    L = C.CDLL(LIB_PATH)
    for name, argtypes in _prototypes().items():
        fn = getattr(L, name)
        if argtypes is not None:
            fn.argtypes = argtypes
        fn.restype = _RESTYPES.get(name, C.c_int)
    _lib = L
    return L
