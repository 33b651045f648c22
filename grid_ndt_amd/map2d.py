"""Host-side mirror of the reference's map interface for the grid-build path, over libgndt's C ABI.

`TwoDmap` keeps the reference's method names and argument meaning (include/map2D.h:485-507,
592-668, 950-976); the loop `for i in 1..n-1: uniformDivision(points[i])` + `create2DMap(demand)`
(src/receiver.cpp:150-160) becomes one call, `create2DMap(demand, cloud)`.  PyTorch appears only as
the owner of device memory and streams.
"""
import ctypes as C
import os

import numpy as np

from . import _lib
from ._arrays import DeviceArrays, HostArrays, _stream_ptr, _stream_wait, _torch_stream_ctx   # noqa: F401 (tools read _stream_ptr here)
from ._lib import (CastOut, CastParams, CastStats, Cells, ClearanceParams, ClearParams, ClearStats, CommSelftest, CropBox, CostStats,
                   DescendParams, ExchangeTimes, FootprintParams, FrontierParams, GndtError, MergeParams, MergeStats, ObstacleParams,
                   OwnedInfo, Params, PatchParams, Pcd, PlanParams, PointLayout, RasterLayers, Robot, RouteFieldParams, ScoreParams, SegmentParams,
                   ShortcutParams, Stats, ViewParams, WalkParams)

DEMANDS = {"slope": 0, "true": 1}
FLAG_HAS_STATS, FLAG_SLOPE, FLAG_DOWN = 1, 2, 4
_ROBOT_DEFAULTS = dict(radius=0.25, reachable_height=0.15, max_rough=100.0, max_angle_deg=30.0)     # RobotSphere(0.25), robot.h:38-46


_ROUTE_HOST_AS = {"start_row": np.int32}       # gndt_route_info on the host: start_row with GNDT_NO_ROW as -1
_FOOT_HOST_AS = {"flags": np.int32}            # gndt_footprint_info on the host: the flags as the signed words the device hands out


def _enum(table, value):
    """a mode by its name in `table`, or by its number"""
    return table[value] if isinstance(value, str) else int(value)


class _DevArray:
    """Minimal __cuda_array_interface__ carrier so torch can view libgndt's device buffers zero-copy."""

    def __init__(self, ptr, shape, typestr, owner):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False),
                                         "version": 2, "strides": None}
        self._owner = owner


class TwoDmap:
    """daysun::TwoDmap for the build path (include/map2D.h:190-194, 485-507)."""

    def __init__(self, res, zres, device=0, max_nodes_hint=0, max_points_hint=0, strategy=0, min_points=3):
        self._L = _lib.lib()
        self.gridLen, self.zLen = float(res), float(zres)   # TwoDmap(res, zres), map2D.h:486
        self.slope_interval = 0.0
        self.device, self.strategy, self.min_points = int(device), int(strategy), int(min_points)
        self.max_nodes_hint, self.max_points_hint = int(max_nodes_hint), int(max_points_hint)
        self.cloudFirst = None
        self._h = None
        self._demand = None
        self._fns, self._torch_device = {}, None

    # ---- setters / getters with the reference's names (map2D.h:487-502) ----
    def getGridLen(self):
        return self.gridLen

    def getZLen(self):
        return self.zLen

    def setCloudFirst(self, p):
        self.cloudFirst = tuple(float(v) for v in p[:3])
        if self._h is not None:
            self._destroy()

    def setLen(self, length):
        self.gridLen = float(length)
        self._destroy()

    def setZLen(self, length):
        self.zLen = float(length)
        self._destroy()

    def setInterval(self, interval):
        self.slope_interval = float(interval)
        self._destroy()

    def getInterval(self):
        return self.slope_interval

    # ---- transMortonXYZ (map2D.h:950-976): host codec, same strings as the reference's map keys ----
    def transMortonXYZ(self, position):
        o = (C.c_float * 3)(*self.cloudFirst)
        p = (C.c_float * 3)(*[float(v) for v in position[:3]])
        q = C.create_string_buffer(2)
        key = C.create_string_buffer(16)
        nx, ny, sz = C.c_int32(), C.c_int32(), C.c_int32()
        rc = self._L.gndt_trans_morton_xyz(o, self.gridLen, self.zLen, p, q, C.byref(nx), C.byref(ny), C.byref(sz), key)
        if rc:
            raise GndtError(rc, "position outside the key range")
        return key.value.decode(), sz.value

    # ---- handle management ----
    def _destroy(self):
        if self._h is not None:
            self._L.gndt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self._destroy()
        except Exception:
            pass

    def _check(self, rc):
        if rc:
            msg = self._L.gndt_last_error(self._h)
            raise GndtError(rc, msg.decode() if msg else "")

    def _ensure(self, demand, need_origin=True):
        d = _enum(DEMANDS, demand)
        if self._h is not None and self._demand == d:
            return
        self._destroy()
        if self.cloudFirst is None and need_origin:
            raise GndtError(1, "setCloudFirst must be called before building (receiver.cpp:145)")
        P = Params(self.gridLen, self.zLen, self.slope_interval, d, self.min_points, self.device, self.strategy,
                   self.max_points_hint, self.max_nodes_hint)
        h = C.c_void_p()
        rc = self._L.gndt_create(C.byref(P), C.byref(h))
        if rc:
            msg = self._L.gndt_last_error(None)
            raise GndtError(rc, msg.decode() if msg else "")
        self._h, self._demand = h, d
        if self.cloudFirst is not None:
            o = (C.c_float * 3)(*self.cloudFirst)
            self._check(self._L.gndt_set_origin(self._h, o))

    def _handle(self):
        """the consumers' preamble: a map that was never built still has a handle to ask (with the demand it was last given)"""
        if self._h is None:
            self._ensure(self._demand if self._demand is not None else "slope", need_origin=False)

    def _call(self, be, name, *args):
        """gndt_<name>_device with the backend's stream behind the arguments, or gndt_<name> (the pair is looked up once a map)"""
        fns = self._fns.get(name)
        if fns is None:
            fns = self._fns[name] = (getattr(self._L, "gndt_" + name), getattr(self._L, "gndt_" + name + "_device"))
        rc = fns[1](self._h, *args, _stream_ptr(be.stream)) if be.on_dev else fns[0](self._h, *args)
        if rc:
            self._check(rc)

    def _cuda(self):
        """the handle's device as torch names it"""
        if self._torch_device is None:
            import torch
            self._torch_device = torch.device("cuda", self.device)
        return self._torch_device

    @staticmethod
    def _robot(robot):
        """-> (byref(gndt_robot) or None for the library's defaults, the dict with the defaults filled in)"""
        d = dict(_ROBOT_DEFAULTS)
        if robot is None:
            return None, d
        d.update(robot)
        return C.byref(Robot(d["radius"], d["reachable_height"], d["max_rough"], d["max_angle_deg"])), d

    def _robot_ref(self, robot):
        return None if robot is None else self._robot(robot)[0]

    @staticmethod
    def _as_input(points):
        """-> (pointer, n, stride_bytes, is_device, keepalive)"""
        try:
            import torch
            if isinstance(points, torch.Tensor):
                assert points.dtype == torch.float32 and points.dim() == 2 and points.shape[1] in (3, 4)
                t = points if points.is_contiguous() else points.contiguous()
                return t.data_ptr(), t.shape[0], 4 * t.shape[1], t.is_cuda, t
        except ImportError:
            pass
        a = np.ascontiguousarray(points, dtype=np.float32)
        assert a.ndim == 2 and a.shape[1] in (3, 4)
        return a.ctypes.data, a.shape[0], 4 * a.shape[1], False, a

    # ---- the build: receiver.cpp:150-154 + map2D.h:592 ----
    def create2DMap(self, demand, points, stream=None):
        """`points` = the cloud WITHOUT point 0 ([N,3] or [N,4] float32; torch CUDA tensor, torch CPU
        tensor or numpy).  Device input is enqueued on `stream` (default: torch's current stream)."""
        self._ensure(demand)
        ptr, n, stride, on_dev, keep = self._as_input(points)
        if on_dev:
            self._check(self._L.gndt_build_device(self._h, C.c_void_p(ptr), n, stride, _stream_ptr(stream)))
        else:
            self._check(self._L.gndt_build(self._h, C.c_void_p(ptr), n, stride))
        self._keep = keep
        return True

    def change2DMap(self, demand, points, stream=None):
        """Incremental add (intent of map2D.h:672-822 as defined in SURVEY Appendix A.7)."""
        self._ensure(demand)
        ptr, n, stride, on_dev, keep = self._as_input(points)
        if on_dev:
            self._check(self._L.gndt_update_device(self._h, C.c_void_p(ptr), n, stride, _stream_ptr(stream)))
        else:
            self._check(self._L.gndt_update(self._h, C.c_void_p(ptr), n, stride))
        self._keep = keep
        return True

    def del2DMap(self, demand, points, stream=None):
        """Incremental delete (intent of map2D.h:826-915 as defined in include/gndt.h): `points` were added before and leave
        their nodes; empty nodes are deleted, surviving nodes keep their place in the order."""
        self._ensure(demand)
        ptr, n, stride, on_dev, keep = self._as_input(points)
        if on_dev:
            self._check(self._L.gndt_remove_device(self._h, C.c_void_p(ptr), n, stride, _stream_ptr(stream)))
        else:
            self._check(self._L.gndt_remove(self._h, C.c_void_p(ptr), n, stride))
        self._keep = keep
        return True

    # ---- input side: raw records (PointCloud2 / .pcd payload) ----
    def pack_points(self, raw, point_step, offsets=(0, 4, 8), demand="slope", stream=None):
        """Raw point records on the device (torch uint8/float32 tensor of n * point_step bytes) -> packed xyz torch
        tensor [n_valid, 3]; rows with a NaN/Inf coordinate dropped, order kept (receiver.cpp:140-143, publisher.cpp:24-26)."""
        import torch
        self._ensure(demand, need_origin=False)
        nbytes = raw.numel() * raw.element_size()
        n = nbytes // int(point_step)
        out = torch.empty((max(n, 1), 3), dtype=torch.float32, device=raw.device)
        lay = PointLayout(int(point_step), int(offsets[0]), int(offsets[1]), int(offsets[2]))
        nv = C.c_uint64()
        self._check(self._L.gndt_pack_points_device(self._h, C.c_void_p(raw.data_ptr()), n, C.byref(lay), C.c_void_p(out.data_ptr()),
                                                    C.byref(nv), _stream_ptr(stream)))
        return out[:int(nv.value)]

    def build_cloud(self, demand, raw, point_step, offsets=(0, 4, 8)):
        """chatterCallback in one call (receiver.cpp:137-160): raw host records (numpy, n * point_step bytes) -> NaN
        strip on the device, origin := first valid point, build of the rest."""
        self._ensure(demand, need_origin=False)
        raw = np.ascontiguousarray(raw)
        n = raw.nbytes // int(point_step)
        lay = PointLayout(int(point_step), int(offsets[0]), int(offsets[1]), int(offsets[2]))
        self._check(self._L.gndt_build_cloud(self._h, C.c_void_p(raw.ctypes.data), n, C.byref(lay)))
        return True

    # ---- split form for sharded clouds ----
    def reset(self, demand="slope", stream=None):
        self._ensure(demand)
        self._check(self._L.gndt_reset(self._h, _stream_ptr(stream)))

    def accumulate(self, demand, points, first_idx_base=0, stream=None):
        self._ensure(demand)
        ptr, n, stride, on_dev, keep = self._as_input(points)
        if not on_dev:
            raise GndtError(1, "accumulate takes device memory")
        self._check(self._L.gndt_accumulate_device(self._h, C.c_void_p(ptr), n, stride, int(first_idx_base), _stream_ptr(stream)))
        self._keep = keep

    def finalize(self, stream=None):
        self._check(self._L.gndt_finalize_device(self._h, _stream_ptr(stream)))

    def stats_export(self, stream=None):
        """Device-resident sufficient statistics as torch tensors (views of libgndt memory)."""
        st = Stats()
        self._check(self._L.gndt_stats_export_device(self._h, C.byref(st), _stream_ptr(stream)))
        return self._stats_tensors(st)

    def _stats_tensors(self, st):
        import torch
        n = int(st.num_nodes)
        dev = f"cuda:{self.device}"
        if n == 0:
            return {"key": torch.zeros(0, dtype=torch.int64, device=dev), "sums": torch.zeros(0, 9, dtype=torch.float64, device=dev),
                    "count": torch.zeros(0, dtype=torch.int32, device=dev), "first_idx": torch.zeros(0, dtype=torch.int32, device=dev)}
        mk = lambda p, shape, ts: torch.as_tensor(_DevArray(p, shape, ts, self), device=dev)
        return {"key": mk(st.key, (n,), "<i8"), "sums": mk(st.sums, (n, 9), "<f8"),
                "count": mk(st.count, (n,), "<i4"), "first_idx": mk(st.first_idx, (n,), "<i4")}

    def shard_stats(self, demand, points, first_idx_base=0, stream=None):
        """This rank's shard of a global cloud -> the statistics of its occupied nodes (torch views of libgndt
        memory, valid until the next call): the counting-partition pipeline, no node table."""
        self._ensure(demand)
        ptr, n, stride, on_dev, keep = self._as_input(points)
        if not on_dev:
            raise GndtError(1, "shard_stats takes device memory")
        st = Stats()
        self._check(self._L.gndt_shard_stats_device(self._h, C.c_void_p(ptr), n, stride, int(first_idx_base), C.byref(st),
                                                    _stream_ptr(stream)))
        self._keep = keep
        return self._stats_tensors(st)

    def build_global(self, comm, demand, points, first_idx_base, total_points, stream=None, timed=False):
        """This rank's contiguous range of a sharded cloud -> the map of the WHOLE cloud on every rank: shard statistics,
        RCCL exchange (called from C++ inside libgndt) and finalisation in one call.  `comm`: grid_ndt_amd.dist.Communicator."""
        self._ensure(demand)
        ptr, n, stride, on_dev, keep = self._as_input(points)
        if not on_dev:
            raise GndtError(1, "build_global takes device memory")
        t = ExchangeTimes()
        self._check(self._L.gndt_build_global_device(self._h, comm.handle, C.c_void_p(ptr), n, stride, int(first_idx_base), int(total_points),
                                                     C.byref(t) if timed else None, _stream_ptr(stream)))
        self._keep = keep
        if timed:
            return {"shard_ms": t.shard_ms, "exchange_ms": t.exchange_ms, "finalize_ms": t.finalize_ms, "ranks": int(t.ranks),
                    "local_nodes": int(t.local_nodes), "global_nodes": int(t.global_nodes), "bytes_reduced": int(t.bytes_reduced)}
        return None

    # ---- owner-partitioned build of a sharded cloud (include/gndt.h): the points travel, the map stays sharded by owner ----
    def _dev_view(self, ptr, nbytes, dtype, shape):
        """torch view of device memory libgndt owns (valid until the next call on the handle)."""
        import torch
        dev = f"cuda:{self.device}"
        if nbytes == 0 or not ptr:
            return torch.empty(shape, dtype=dtype, device=dev)
        ts = {torch.float32: "<f4", torch.int64: "<i8", torch.int32: "<i4"}[dtype]
        return torch.as_tensor(_DevArray(ptr, shape, ts, self), device=dev)

    def owner_sample(self, demand, points, stream=None):
        """Evenly spaced sample of this rank's shard as the fixed-size message every rank publishes (int32 device view)."""
        import torch
        self._ensure(demand)
        ptr, n, stride, on_dev, keep = self._as_input(points)
        if not on_dev:
            raise GndtError(1, "owner_sample takes device memory")
        p, w = C.c_void_p(), C.c_uint64()
        self._check(self._L.gndt_owner_sample_device(self._h, C.c_void_p(ptr), n, stride, C.byref(p), C.byref(w), _stream_ptr(stream)))
        return self._dev_view(p.value, int(w.value) * 4, torch.int32, (int(w.value),))

    def owner_map(self, all_msgs, world, stream=None):
        """The sample messages of all ranks (int32 device tensor, rank order) -> the block ownership later owner_split calls use."""
        self._check(self._L.gndt_owner_map_device(self._h, C.c_void_p(all_msgs.data_ptr()), int(world), _stream_ptr(stream)))

    def owner_split(self, demand, points, first_idx_base, total_points, world, stream=None):
        """This rank's contiguous range of the cloud -> its points as 16-B records grouped by owner rank.
        Returns the list of runs, one [count, 4] float32 device view per owner rank."""
        self._ensure(demand)
        ptr, n, stride, on_dev, keep = self._as_input(points)
        if not on_dev:
            raise GndtError(1, "owner_split takes device memory")
        recs = C.c_void_p()
        counts = (C.c_uint64 * int(world))()
        offsets = (C.c_uint64 * int(world))()
        self._check(self._L.gndt_owner_split_device(self._h, C.c_void_p(ptr), n, stride, int(first_idx_base), int(total_points), int(world),
                                                    C.byref(recs), counts, offsets, _stream_ptr(stream)))
        self._keep = keep
        import torch
        base = recs.value or 0
        return [self._dev_view(base + 16 * int(o), int(c) * 16, torch.float32, (int(c), 4)) for c, o in zip(counts, offsets)]

    def build_records(self, demand, records, total_points, stream=None):
        """The records this rank owns ([m, 4] float32 on the device: x, y, z, index word) -> its part of the map."""
        self._ensure(demand)
        if records.dim() != 2 or records.shape[1] != 4 or not records.is_contiguous() or not records.is_cuda:
            raise GndtError(1, "records must be a contiguous [m, 4] float32 device tensor")
        self._check(self._L.gndt_build_records_device(self._h, C.c_void_p(records.data_ptr()), int(records.shape[0]), int(total_points),
                                                      _stream_ptr(stream)))
        self._keep = records

    def build_records2(self, demand, first, room_and_second, total_points, stream=None):
        """build_records from two segments: `first` [a, 4] stays where it is; `room_and_second` [a + b, 4] holds the second
        segment in its last b rows (the first a rows are room the small-build path fills)."""
        self._ensure(demand)
        a = int(first.shape[0])
        b = int(room_and_second.shape[0]) - a
        assert b >= 0 and first.is_contiguous() and room_and_second.is_contiguous()
        self._check(self._L.gndt_build_records2_device(self._h, C.c_void_p(first.data_ptr()), a, C.c_void_p(room_and_second.data_ptr() + 16 * a), b,
                                                       int(total_points), _stream_ptr(stream)))
        self._keep = (first, room_and_second)

    def owned_columns(self, stream=None):
        """(first-seen index << 32 | node count) of every column of the local map: int64 device view."""
        import torch
        p, n = C.c_void_p(), C.c_uint64()
        self._check(self._L.gndt_owned_columns_device(self._h, C.byref(p), C.byref(n), _stream_ptr(stream)))
        return self._dev_view(p.value or 0, int(n.value) * 8, torch.int64, (int(n.value),))

    def owned_global_rows(self, all_pairs, total_points, stream=None):
        """Everybody's column pairs (int64 device tensor) -> (global row of every local row: int32 device view, nodes and
        columns of the whole map)."""
        import torch
        p, gn, gc = C.c_void_p(), C.c_uint64(), C.c_uint64()
        self._check(self._L.gndt_owned_global_rows_device(self._h, C.c_void_p(all_pairs.data_ptr()), int(all_pairs.shape[0]), int(total_points),
                                                          C.byref(p), C.byref(gn), C.byref(gc), _stream_ptr(stream)))
        n = self.sync()[0]
        return self._dev_view(p.value or 0, n * 4, torch.int32, (n,)), int(gn.value), int(gc.value)

    def second_pass_buckets(self):
        """Buckets of the last resolved PARTITION build that went through the bucket kernel's second pass (1024-slot tables)."""
        r = C.c_uint64()
        self._check(self._L.gndt_debug_second_pass_buckets(self._h, C.byref(r)))
        return int(r.value)

    def debug_fail_next_alloc(self, site, demand="slope"):
        """Tests: the next allocation at `site` of the sharded builds fails once on this handle (include/gndt.h)."""
        self._ensure(demand)             # (the handle is created lazily, with the demand)
        self._check(self._L.gndt_debug_fail_next_alloc(self._h, int(site)))

    def build_owned(self, comm, demand, points, first_idx_base, total_points, stream=None):
        """Owner-partitioned build over RCCL (called from C++ inside libgndt): this rank's range of the cloud in, the columns
        this rank owns out (export()), plus the global row of each of its rows.  Returns (global_row view, info dict)."""
        import torch
        self._ensure(demand)
        ptr, n, stride, on_dev, keep = self._as_input(points)
        if not on_dev:
            raise GndtError(1, "build_owned takes device memory")
        info, p = OwnedInfo(), C.c_void_p()
        self._check(self._L.gndt_build_owned_device(self._h, comm.handle, C.c_void_p(ptr), n, stride, int(first_idx_base), int(total_points),
                                                    C.byref(p), C.byref(info), _stream_ptr(stream)))
        self._keep = keep
        d = {k: (float(getattr(info, k)) if k.endswith("_ms") else int(getattr(info, k))) for k, _ in OwnedInfo._fields_}
        return self._dev_view(p.value or 0, d["local_nodes"] * 4, torch.int32, (d["local_nodes"],)), d

    def gather_owned(self, comm, root=-1, stream=None):
        """After build_owned: the rows of all ranks gathered on rank `root` (root < 0: on every rank) and scattered by their
        global row — this map then IS the map of the whole cloud (export(), computeCost(), ... as after a single-GPU build).
        Every rank of the communicator calls it; ranks other than `root` keep the columns they own."""
        self._check(self._L.gndt_gather_owned_map_device(self._h, comm.handle, int(root), _stream_ptr(stream)))

    def comm_selftest(self, comm, stream=None, demand="slope"):
        """gndt_comm_selftest: one verified round of every collective the sharded builds use (all ranks call it together)."""
        self._ensure(demand, need_origin=False)
        rep = CommSelftest()
        self._check(self._L.gndt_comm_selftest(self._h, comm.handle, C.byref(rep), _stream_ptr(stream)))
        return {"ok_mask": int(rep.ok_mask), "ranks": int(rep.ranks), "all_gather_ms": round(float(rep.all_gather_ms), 3),
                "exchange_ms": round(float(rep.exchange_ms), 3), "reduce_scatter_ms": round(float(rep.reduce_scatter_ms), 3),
                "all_reduce_ms": round(float(rep.all_reduce_ms), 3)}

    def owned_pack_rows(self, stream=None):
        """This rank's rows as packed records [n, 21] int32 (device view, valid until the next call): for hosts with their own transport."""
        import torch
        p, n = C.c_void_p(), C.c_uint64()
        self._check(self._L.gndt_owned_pack_rows_device(self._h, C.byref(p), C.byref(n), _stream_ptr(stream)))
        return self._dev_view(p.value or 0, n.value * 21 * 4, torch.int32, (n.value, 21))

    def adopt_rows(self, rows, total_nodes, total_columns, total_slopes, stream=None):
        """Packed records of any number of ranks ([m, 21] int32 on the device; padding records skipped) -> this map's rows."""
        rows = rows.contiguous()
        self._check(self._L.gndt_adopt_rows_device(self._h, C.c_void_p(rows.data_ptr()), int(rows.shape[0]), int(total_nodes), int(total_columns),
                                                   int(total_slopes), _stream_ptr(stream)))

    def finalize_stats(self, key, sums, count, first_idx, total_points, stream=None):
        """Merged statistics of the whole cloud (unique nodes sorted by key) -> the map."""
        st = Stats(int(key.shape[0]), key.data_ptr(), sums.data_ptr(), count.data_ptr(), first_idx.data_ptr())
        self._check(self._L.gndt_finalize_stats_device(self._h, C.byref(st), int(total_points), _stream_ptr(stream)))
        self._keep = (key, sums, count, first_idx)

    def stats_merge(self, key, sums, count, first_idx, stream=None):
        st = Stats(int(key.shape[0]), key.data_ptr(), sums.data_ptr(), count.data_ptr(), first_idx.data_ptr())
        self._check(self._L.gndt_stats_merge_device(self._h, C.byref(st), _stream_ptr(stream)))
        self._keep = (key, sums, count, first_idx)

    # ---- phase timing ----
    PHASES = {1: ("clear", "accumulate", "columns", "rows", "bitmap_scan", "rank", "column_scan", "dest", "emit"),
              5: ("clear", "accumulate", "columns", "rows", "bitmap_scan", "rank", "column_scan", "dest", "emit"),
              2: ("clear", "level1", "layout", "level2", "bucket_build", "bitmap_scan", "rank", "column_scan", "dest", "emit"),
              3: ("clear", "hist", "offsets", "scatter", "bucket_build", "bitmap_scan", "rank", "column_scan", "dest", "emit"),
              6: ("clear", "level1", "layout", "ranges", "bucket_build", "bitmap_scan", "rank", "column_scan", "dest", "emit"),
              7: ("clear", "level1", "layout", "level2", "bucket_build", "bitmap_scan", "rank", "column_scan", "dest", "emit")}
    STRATEGY_NAMES = {1: "atomic", 2: "partition", 3: "partition_exact", 5: "tile", 6: "partition_one_level", 7: "partition_blocked"}
    # phase -> the kernel that fills it, and what each phase's kernel moves algorithmically (bench.py's roofline line):
    # kernels that stream the cloud 12 B/point, the bucket kernel 12 B/point + 76 B/node, node kernels 76 B/node
    KERNEL_OF_PHASE = {"accumulate": "k_accumulate", "hist": "k_part_hist", "scatter": "k_part_scatter",
                       "level1": "k_part2_level1", "level2": "k_part2_level2",
                       "bucket_build": "k_bucket_direct",
                       "columns": "k_tab_columns", "rows": "k_tab_rows", "emit": "k_emit_rows"}
    KERNEL_OF_PHASE_BLOCKED = dict(KERNEL_OF_PHASE, bucket_build="k_bucket_blocked")      # strategy 7 (gndt_blocked.hpp)
    POINT_PHASES = ("accumulate", "hist", "scatter", "level1", "level2")
    POINT_AND_NODE_PHASES = ("bucket_build",)

    def set_profiling(self, on=True, demand="slope"):
        self._ensure(demand)
        self._check(self._L.gndt_set_profiling(self._h, int(on)))

    def locality_sample(self, points, tiles=64, demand="slope", stream=None):
        """Points per partial that strategy TILE would flush, measured on `tiles` tiles of the device-resident cloud."""
        self._ensure(demand)
        ptr, n, stride, on_dev, keep = self._as_input(points)
        if not on_dev:
            raise GndtError(1, "locality_sample takes device memory")
        r = C.c_double()
        self._check(self._L.gndt_locality_sample(self._h, C.c_void_p(ptr), n, stride, int(tiles), C.byref(r), _stream_ptr(stream)))
        return r.value

    def last_strategy(self):
        """1 = ATOMIC, 2 = PARTITION (two-level), 3 = PARTITION_EXACT: what the last build actually ran."""
        return int(self._L.gndt_last_strategy(self._h))

    def phase_times_ms(self):
        arr = (C.c_double * 10)()
        self._check(self._L.gndt_get_phase_times(self._h, arr))
        names = self.PHASES[self.last_strategy()]
        return {k: arr[i] for i, k in enumerate(names)}

    def retry_count(self):
        r = C.c_uint64()
        self._check(self._L.gndt_debug_retry_count(self._h, C.byref(r)))
        return int(r.value)

    BLOCK_LAYOUT_FIELDS = ("state", "x0", "y0", "z0", "shx", "shy", "shz", "nx", "ny", "buckets")

    def block_layout(self):
        """gndt_debug_block_layout: the block layout the handle holds for blocked buckets (state 1: the next cloud of this size
        takes them; x0, y0, z0 in contiguous indices; shx, shy, shz = log2 of a block's columns along x, y and its levels)."""
        arr = (C.c_int32 * 10)()
        self._check(self._L.gndt_debug_block_layout(self._h, arr))
        return dict(zip(self.BLOCK_LAYOUT_FIELDS, (int(v) for v in arr)))

    def enable_stamps(self, on=True):
        self._L.gndt_debug_enable_stamps(int(bool(on)))

    def reserve(self, max_points, max_nodes=0, demand="slope"):
        """gndt_reserve: every buffer a build of this size can need, allocated now (capture a build on a fresh handle afterwards)."""
        self._ensure(demand, need_origin=False)
        self._check(self._L.gndt_reserve(self._h, int(max_points), int(max_nodes)))

    def warmup(self, expected_points=0, demand="slope"):
        """gndt_warmup: the kernels' code loaded (a temporary handle runs every strategy family once on a synthetic cloud of
        `expected_points` points) and, with a size known, every buffer reserved — so that the FIRST build costs what the next one does."""
        self._ensure(demand, need_origin=False)
        self._check(self._L.gndt_warmup(self._h, int(expected_points)))

    def set_deferred_emit(self, on=True, demand="slope"):
        """gndt_set_deferred_emit: updates relabel the touched columns only; the dense rows are produced when the map is read."""
        self._ensure(demand)
        self._check(self._L.gndt_set_deferred_emit(self._h, int(bool(on))))

    DEBUG_VERBOSE, DEBUG_TILE_RATIO, DEBUG_COST_ONE_WORKGROUP, DEBUG_QUERY_ILP = 1, 2, 3, 4
    DEBUG_PLAN_LDS_ENTRIES = 6
    DEBUG_POISON_BYTE = 7      # the poisoned variant of the library only (_lib.VARIANTS); the product answers GNDT_ERR_INVALID
    DEBUG_CLEARANCE_ONE_WORKGROUP = 8
    DEBUG_WALK_STEP_TABLE = 9
    DEBUG_BLOCKED_MIN_POINTS = 10   # points from which a build may take blocked buckets: 65 536 .. 1 048 576 (the default; tests lower it)
    DEBUG_COLUMN_DEST = 11          # blocked builds with the two-kernel tail: 1 (the default) orders by the column table, 0 by the staged nodes
    DEBUG_PLACE_EMIT_WORDS = 12     # bitmap words up to which ordering and emit are one kernel: 0 .. 2^24 (16 384 by default; 0: always two)
    DEBUG_ROUTE_FIELD_ONE_WORKGROUP = 14   # 0: every sweep of the route field its own launch (1 by default)
    DEBUG_VIEW_THREADS = 15                # threads of a view_gain workgroup at most: a multiple of 64 in 64 .. 1024 (1024 by default)
    DEBUG_PATCH_LDS = 16                   # 0: the patches' moment pass without its LDS stage (1 by default)
    DEBUG_OBSTACLE_TALLY = 13       # 1: the obstacle field's marking pass keeps the tallies of gndt_debug_obstacle_marks (0 by default)

    @staticmethod
    def set_debug_option(option, value):
        """gndt_debug_set_option: process-wide diagnostics and thresholds (the library reads no environment variable)."""
        rc = _lib.lib().gndt_debug_set_option(int(option), float(value))
        if rc:
            raise _lib.GndtError(rc, f"gndt_debug_set_option({option}, {value})")

    @staticmethod
    def poisoned_bytes():
        """gndt_debug_poisoned_bytes: (device bytes, pinned host bytes) the poisoned variant of the library has filled so far in this
        process; the product raises GNDT_ERR_INVALID."""
        d, h = C.c_uint64(), C.c_uint64()
        rc = _lib.lib().gndt_debug_poisoned_bytes(C.byref(d), C.byref(h))
        if rc:
            raise _lib.GndtError(rc, "gndt_debug_poisoned_bytes")
        return int(d.value), int(h.value)

    def set_fp_bits(self, bits):
        """Narrow the bucket kernel's index fingerprint (process-wide; tests: forces its exact second pass)."""
        self._L.gndt_debug_set_fp_bits(int(bits))

    def fp_clashes(self):
        r = C.c_uint64()
        self._check(self._L.gndt_debug_fp_clashes(self._h, C.byref(r)))
        return int(r.value)

    def debug_bucket_phases(self):
        """Mean shader cycles per bucket of k_bucket_build's phases (after enable_stamps())."""
        arr = (C.c_double * 10)()
        nb = C.c_uint32()
        self._check(self._L.gndt_debug_bucket_phases(self._h, arr, C.byref(nb)))
        names = ("clear", "accumulate", "columns", "rows", "-", "-", "acc:0", "acc:1", "acc:2", "acc:3")
        return dict(zip(names, list(arr))), nb.value

    # ---- cost map (TwoDmap::computeCost, map2D.h:1285-1397) ----
    def computeCost(self, goal, robot=None, stream=None):
        """Flood the finished grid from the slope under `goal` (xyz).  `robot`: dict with radius,
        reachable_height, max_rough, max_angle_deg (defaults: RobotSphere(0.25), robot.h:38-46).
        Returns the statistics dict; h / state per result row come from cost_export()."""
        g = (C.c_float * 3)(*[float(v) for v in goal])
        self._check(self._L.gndt_compute_cost(self._h, g, self._robot_ref(robot), _stream_ptr(stream)))
        st = CostStats()
        self._check(self._L.gndt_cost_export(self._h, None, None, C.byref(st)))
        return self._cost_stats(st)

    @staticmethod
    def _cost_stats(st):
        return {"rc": int(st.goal_status), "ring": int(st.ring), "levels": int(st.levels), "traversable": int(st.traversable),
                "closed": int(st.closed), "check_pushes": int(st.check_pushes), "ring_store": int(st.ring_store)}

    def cost_export(self):
        """Host copy of Slope::h (fp32, FLT_MAX = unreached) and the flood state per result row."""
        n, _, _ = self.sync()
        h = np.zeros(n, np.float32)
        state = np.zeros(n, np.uint32)
        st = CostStats()
        self._check(self._L.gndt_cost_export(self._h, h.ctypes.data, state.ctypes.data, C.byref(st)))
        out = self._cost_stats(st)
        out.update(h=h, state=state.astype(np.uint8))
        return out

    # ---- route planning (gndt_plan_routes*: AstarPlanar::findRoute, GlobalPlan.h:49-166, for a batch of starts) ----
    ROUTE_STATUS = {0: "found", 1: "no_start", 2: "no_route", 3: "limit", 4: "no_goal"}
    ROUTE_INFO_DTYPE = _lib.ROUTE_INFO

    def plan_routes(self, starts, start_mode="node", route_cap=None, max_expansions=0, stream=None, host=False, scratch_bytes=0):
        """The reference planner's routes from `starts` ([K,3] or [K,4] float32) to the goal of the last computeCost, one device call
        (include/gndt.h "route planning" defines the answer).  Returns (rows, info): rows [K, route_cap] int32, each route start
        first and goal last as rows of export(), -1 behind its end.  A route longer than route_cap (None: the map's slope count or 1024,
        whichever is less) comes back cut to its first route_cap rows with its true length in info["length"]: call again with that;
        info: dict of [K] arrays status (ROUTE_STATUS), length, start_row (int32, -1: none), expansions, queue_peak, cost, h_start.
        torch CUDA starts are answered on the device (torch tensors, enqueued on `stream`, default torch's current stream, not awaited);
        host=True or a host array goes through gndt_plan_routes (numpy)."""
        # (one of the three small calls a planner makes thousands of times a second — query and score_poses are the others: their two
        # branches stay written out, the single body over a backend costs them a microsecond in twenty)
        if self._h is None:
            self._handle()
        ptr, K, stride, on_dev, keep = self._as_input(starts)
        if route_cap is None:
            route_cap = max(min(int(self.sync()[2]), 1024), 1)
        route_cap = int(route_cap)
        prm = PlanParams(_enum(self.QUERY_MODES, start_mode), int(max_expansions), int(scratch_bytes))
        if on_dev and host:
            ptr, K, stride, on_dev, keep = self._as_input(keep.detach().cpu().numpy())
        if on_dev:
            import torch
            with _torch_stream_ctx(stream):
                rows = torch.empty((K, route_cap), dtype=torch.int32, device=keep.device)
                raw = torch.empty((K, 8), dtype=torch.int32, device=keep.device)
            self._check(self._L.gndt_plan_routes_device(self._h, C.c_void_p(ptr if K else 0), K, stride, C.byref(prm),
                                                        C.c_void_p(rows.data_ptr() if K and route_cap else 0), route_cap,
                                                        C.c_void_p(raw.data_ptr() if K else 0), _stream_ptr(stream)))
            return rows, _lib.record_views(raw, _lib.ROUTE_INFO)
        rows = np.empty((K, route_cap), np.int32)
        raw = np.zeros(K, _lib.ROUTE_INFO)
        self._check(self._L.gndt_plan_routes(self._h, C.c_void_p(ptr if K else 0), K, stride, C.byref(prm),
                                             C.c_void_p(rows.ctypes.data if K and route_cap else 0), route_cap,
                                             C.c_void_p(raw.ctypes.data if K else 0)))
        return rows, HostArrays.fields(raw, _lib.ROUTE_INFO, _ROUTE_HOST_AS)

    def findRoute(self, start):
        """AstarPlanar::findRoute(start -> the goal of the last computeCost): the route as a list of rows of export(), start slope
        first and goal slope last, or None ("not find the road", GlobalPlan.h:159-163)."""
        p = np.asarray(start, np.float32).reshape(1, -1)[:, :3]
        rows, info = self.plan_routes(p, host=True)
        if int(info["status"][0]) != 0:
            return None
        if int(info["length"][0]) > rows.shape[1]:
            rows, info = self.plan_routes(p, host=True, route_cap=int(info["length"][0]))
        return [int(r) for r in rows[0, :int(info["length"][0])]]

    # ---- point queries (the lookup of computeCost's goal, map2D.h:1291-1306, and findRoute's start / goal, GlobalPlan.h:56-61) ----
    QUERY_MODES = {"node": 0, "nearest_slope": 1}
    NO_ROW = -1        # GNDT_NO_ROW as the int32 the rows come back in

    def query(self, points, mode="node", cost=False, stream=None):
        """Rows of the finished map (export order) at `points` ([N,3] or [N,4] float32), -1 where the map has no answer.
        mode "node": the node whose key is the point's (any node: map_xy's view); "nearest_slope": the slope of the point's column
        whose mean z is nearest the point's z.  A torch CUDA tensor is answered on the device (torch int32 rows, enqueued on `stream`,
        default torch's current stream); a host array through gndt_query (numpy).  cost=True also returns the cost map's h (float32,
        FLT_MAX where there is no row) and state (int32) of every row: (rows, h, state)."""
        # (a hot small call: its two branches stay written out, see plan_routes)
        if self._h is None:
            self._handle()
        m = _enum(self.QUERY_MODES, mode)
        ptr, n, stride, on_dev, keep = self._as_input(points)
        if on_dev:
            import torch
            rows = torch.empty(n, dtype=torch.int32, device=keep.device)
            h = torch.empty(n, dtype=torch.float32, device=keep.device) if cost else None
            state = torch.empty(n, dtype=torch.int32, device=keep.device) if cost else None
            p = lambda t: C.c_void_p(t.data_ptr() if t is not None and n else 0)
            self._check(self._L.gndt_query_device(self._h, C.c_void_p(ptr if n else 0), n, stride, m, p(rows), p(h), p(state),
                                                  _stream_ptr(stream)))
        else:
            rows = np.empty(n, np.int32)
            h = np.empty(n, np.float32) if cost else None
            state = np.empty(n, np.int32) if cost else None
            p = lambda a: C.c_void_p(a.ctypes.data if a is not None and n else 0)
            self._check(self._L.gndt_query(self._h, C.c_void_p(ptr if n else 0), n, stride, m, p(rows), p(h), p(state)))
        return (rows, h, state) if cost else rows

    # ---- region crop (gndt_crop*: whole columns leave the map, without their points) ----
    CROP_MODES = {"keep_inside": 0, "drop_inside": 1}

    def crop(self, lo_xy, hi_xy, keep="inside", stream=None):
        """Drop every node of the columns outside (keep="inside": the rolling window) or inside (keep="outside") the world rectangle
        [lo_xy, hi_xy] — the columns that hold a point of it, as the codec keys them (crop_box_from_world).  Returns the index box."""
        if keep not in ("inside", "outside"):
            raise ValueError('keep must be "inside" or "outside"')
        box = crop_box_from_world(self.cloudFirst, self.gridLen, lo_xy, hi_xy)
        self.crop_box(box, "keep_inside" if keep == "inside" else "drop_inside", stream=stream)
        return box

    def crop_box(self, box, mode="keep_inside", stream=None):
        """The same for an inclusive box of signed column indices (sx_min, sx_max, sy_min, sy_max); mode "keep_inside" / "drop_inside"
        (or GNDT_CROP_*).  Enqueued on `stream` (default torch's current stream); the counts are read by the next sync / export."""
        if self._h is None:
            self._handle()
        b = CropBox(*[int(v) for v in box])
        self._check(self._L.gndt_crop_device(self._h, C.byref(b), _enum(self.CROP_MODES, mode), _stream_ptr(stream)))

    # ---- raster export (gndt_raster*: one pixel per column of a box, the reference's showBottom / showSlopeList, map2D.h:980-1284) ----
    RASTER_MODES = {"lowest": 0, "highest": 1, "nearest_z": 2}
    RASTER_LAYERS = {"row": np.int32, "z": np.float32, "rough": np.float32, "nodes": np.int32, "h": np.float32, "state": np.int32}

    def raster(self, box, mode="lowest", z_ref=None, layers=("row", "z"), stream=None, host=False):
        """The map over the inclusive box of signed column indices (sx_min, sx_max, sy_min, sy_max) — crop_box_from_world turns a world
        rectangle into one — as a (height, width) image per layer, row-major from the smallest (sx, sy) (index 0 skipped: raster_shape).
        Per pixel the slope of its column with the least sz (mode "lowest"), the greatest ("highest") or the mean z nearest z_ref
        ("nearest_z", query's "nearest_slope" rule).  Layers: "row" (int32, -1 where the column has no slope: query's rows), "z" and
        "rough" (float32, NaN there), "nodes" (int32, the column's node count, 0 = not observed), "h" (float32, FLT_MAX there) and
        "state" (int32, 0 there) of the cost map.  Torch tensors on the handle's device enqueued on `stream` (default torch's current
        stream), or numpy arrays through gndt_raster with host=True.  Also returns x0, y0 (the world centre of pixel (0, 0)) and res."""
        if self._h is None:
            self._handle()
        m = _enum(self.RASTER_MODES, mode)
        if z_ref is None:
            z_ref = float("nan") if m == self.RASTER_MODES["nearest_z"] else 0.0
        layers = tuple(layers)
        for name in layers:
            if name not in self.RASTER_LAYERS:
                raise ValueError(f"unknown raster layer {name!r} (one of {', '.join(self.RASTER_LAYERS)})")
        b = CropBox(*[int(v) for v in box])
        w, ht = raster_shape(box)
        be = HostArrays if host else DeviceArrays(self._cuda(), stream)
        out = {name: be.empty((ht, w), self.RASTER_LAYERS[name]) for name in layers}
        L = RasterLayers(*[be.ptr(out.get(name)) for name in ("row", "z", "rough", "nodes", "h", "state")])
        self._call(be, "raster", C.byref(b), m, float(z_ref), C.byref(L))
        sx0 = _first_nonzero(b.sx_min)
        sy0 = _first_nonzero(b.sy_min)
        out.update(x0=_column_centre(self.cloudFirst[0], self.gridLen, sx0), y0=_column_centre(self.cloudFirst[1], self.gridLen, sy0),
                   res=self.gridLen)
        return out

    # ---- frontier extraction (gndt_frontiers*: the slopes where the known map ends, clustered on the device) ----
    FRONTIER_CANDIDATES = {"reached": 0, "slopes": 1}
    FRONTIER_OPEN_RULES = {"column": 0, "level": 1}
    FRONTIER_DTYPE = _lib.FRONTIER

    def frontiers(self, candidates="reached", open_rule="column", level_reach=1, min_open=1, link_dz=1, min_size=1, box=None, labels=False,
                  max_clusters=None, stream=None, host=False):
        """Where the known map ends, as clusters (include/gndt.h "frontier extraction" defines every word).  A frontier row is a slope —
        candidates "reached": one the last computeCost expanded; "slopes": any — with at least min_open of its four sides open:
        open_rule "column": no such column in the map; "level": or no node of it within level_reach levels.  Frontier rows in
        8-adjacent columns at most link_dz levels apart form a cluster.  Returns a dict with one [K] array per field of gndt_frontier
        (label, size, best_row, best_h, sx_min, sx_max, sy_min, sy_max, sum_px, sum_py, sum_pz, open_sides) for the clusters of at
        least min_size rows in ascending label, `counts` ([4]: those clusters, frontier rows, clusters of any size, 0) and, with
        labels=True, `labels` (int32 per row of export(): its cluster's label, -1 for a row that is no frontier row).  box: an inclusive
        box of signed column indices (sx_min, sx_max, sy_min, sy_max), None = the whole map.  max_clusters=None sizes the list from a
        count-only first call (which waits for it on `stream`); a number is the list's capacity — counts[0] may exceed it.  Torch
        tensors on the handle's device, enqueued on `stream` (default torch's current stream) and not awaited: the arrays then have
        max_clusters entries, filled from the front, with size 0 behind the counts[0] the call found.  Or numpy arrays through
        gndt_frontiers with host=True, cut to min(counts[0], max_clusters) entries."""
        # (left with its two branches written out: the single body over a backend cost its device twin 0.9 us in 61, DESIGN 4.5b;
        # the records are decoded through the record table like everywhere else)
        if self._h is None:
            self._handle()
        prm = FrontierParams(_enum(self.FRONTIER_CANDIDATES, candidates), _enum(self.FRONTIER_OPEN_RULES, open_rule),
                             int(level_reach), int(min_open), int(link_dz), int(min_size))
        b = C.byref(CropBox(*[int(v) for v in box])) if box is not None else None
        n = int(self.sync()[0]) if labels else 0
        if host:
            counts = np.zeros(4, np.uint32)
            label = np.empty(n, np.int32) if labels else None
            call = lambda recs, cap: self._check(self._L.gndt_frontiers(
                self._h, b, C.byref(prm), C.c_void_p(label.ctypes.data if labels and n else 0),
                C.c_void_p(recs.ctypes.data if cap else 0), cap, C.c_void_p(counts.ctypes.data)))
            if max_clusters is None:
                call(None, 0)
                max_clusters = int(counts[0])
            recs = np.zeros(int(max_clusters), _lib.FRONTIER)
            call(recs, len(recs))
            recs = recs[:min(int(counts[0]), len(recs))]
            out = HostArrays.fields(recs, _lib.FRONTIER)
        else:
            import torch
            dev = f"cuda:{self.device}"
            with _torch_stream_ctx(stream):
                counts = torch.zeros(4, dtype=torch.int32, device=dev)
                label = torch.empty(n, dtype=torch.int32, device=dev) if labels else None
            call = lambda recs, cap: self._check(self._L.gndt_frontiers_device(
                self._h, b, C.byref(prm), C.c_void_p(label.data_ptr() if labels and n else 0),
                C.c_void_p(recs.data_ptr() if cap else 0), cap, C.c_void_p(counts.data_ptr()), _stream_ptr(stream)))
            if max_clusters is None:
                call(None, 0)
                with _torch_stream_ctx(stream):         # (read on the stream the count was enqueued on: the copy waits for it)
                    max_clusters = int(counts[0].item())
            with _torch_stream_ctx(stream):
                recs = torch.zeros((int(max_clusters), _lib.FRONTIER.itemsize // 4), dtype=torch.int32, device=dev)
            call(recs, recs.shape[0])
            out = _lib.record_views(recs, _lib.FRONTIER)
        out["counts"] = counts
        if labels:
            out["labels"] = label
        return out

    def frontier_points(self, fr, which="best"):
        """World points [K, 3] float32 of the clusters of frontiers(), ready for plan_routes(..., start_mode="nearest_slope"): which
        "best": the centre of the node of each cluster's best_row; "centroid": the clusters' mean position, sum_p* / size.  A column's
        centre is origin + (lin(s) + 0.5) * grid_len with lin(s) = s - 1 for s > 0, s otherwise; the same for z with z_len.  An entry
        of size 0 (behind the clusters found, in a list with room to spare) gives NaN, which the planner answers with "no start".
        Torch in, torch out (best rows are looked up in export_device()); numpy in, numpy out (export())."""
        if which not in ("best", "centroid"):
            raise ValueError('which must be "best" or "centroid"')
        on_dev = not isinstance(fr["size"], np.ndarray)
        K = int(fr["size"].shape[0])
        xp = np
        if on_dev:
            import torch as xp
        if which == "centroid":
            size = fr["size"].clip(1, None)
            lin = [(fr[k].double() if on_dev else fr[k].astype(np.float64)) / size for k in ("sum_px", "sum_py", "sum_pz")]
        else:
            cells = self.export_device() if on_dev else self.export()
            rows = fr["best_row"].long() if on_dev else fr["best_row"].astype(np.int64)
            if K == 0 or int(cells["num_nodes"]) == 0:
                return xp.zeros((0, 3), dtype=xp.float32, **({"device": fr["size"].device} if on_dev else {}))
            s = [cells[k][rows] for k in ("sx", "sy", "sz")]
            lin = [(v - (v > 0).to(v.dtype) if on_dev else v - (v > 0)) for v in s]
            lin = [v.double() if on_dev else v.astype(np.float64) for v in lin]
        o, steps = self.cloudFirst, (self.gridLen, self.gridLen, self.zLen)
        cols = [o[a] + (lin[a] + 0.5) * steps[a] for a in range(3)]
        pts = xp.stack(cols, 1).float() if on_dev else np.stack(cols, 1).astype(np.float32)
        pts[fr["size"] == 0] = float("nan")
        return pts

    # ---- surface patches (gndt_patches*: the map's nodes grown into planes on the device) ----
    PATCH_CANDIDATES = {"nodes": 0, "slopes": 1}
    PATCH_CONNECTIVITY = {6: 1, 18: 2, 26: 3}
    PATCH_HORIZONTAL, PATCH_VERTICAL, PATCH_INCLINED, PATCH_SLOPES_ONLY = 1, 2, 4, 8
    PATCH_DTYPE = _lib.PATCH

    def patch_params(self, candidates="nodes", connectivity=26, max_angle_deg=15.0, max_offset=None, max_var=None, level_deg=10.0, min_size=1):
        """gndt_patch_params of patches()'s arguments, the thresholds as the float32 the library reads: cos_min = float32(cos(
        max_angle_deg)), cos_level = float32(cos(level_deg)), sin_level = float32(sin(level_deg)); max_offset None = 0.5 zLen, max_var
        None = (0.25 zLen)^2"""
        if connectivity not in self.PATCH_CONNECTIVITY:
            raise ValueError("connectivity must be 6, 18 or 26")
        max_offset = 0.5 * self.zLen if max_offset is None else max_offset
        max_var = (0.25 * self.zLen) ** 2 if max_var is None else max_var
        cos_min = np.float32(np.cos(np.deg2rad(float(max_angle_deg))))
        cos_level, sin_level = np.float32(np.cos(np.deg2rad(float(level_deg)))), np.float32(np.sin(np.deg2rad(float(level_deg))))
        return PatchParams(_enum(self.PATCH_CANDIDATES, candidates), self.PATCH_CONNECTIVITY[connectivity], float(cos_min),
                           float(np.float32(max_offset)), float(np.float32(max_var)), float(cos_level), float(sin_level), int(min_size))

    def patches(self, candidates="nodes", connectivity=26, max_angle_deg=15.0, max_offset=None, max_var=None, level_deg=10.0, min_size=1,
                box=None, labels=False, max_patches=None, stream=None, host=False):
        """What the map is made of, as planes (include/gndt.h "surface patches" defines every word).  A candidate is a node with
        statistics — candidates "slopes": with a slope as well — whose rough / count is at most max_var (m^2; None = (0.25 zLen)^2).
        Adjacent candidates (connectivity 6, 18 or 26; two levels of one column are adjacent) link when their normals are within
        max_angle_deg of each other, sign free, and each one's mean lies within max_offset (m; None = 0.5 zLen) of the other's plane;
        the connected components are the patches: single-link growing, so a gently curved surface is ONE patch and its `var` shows it.
        Returns a dict with one [K] array per field of gndt_patch (label, nodes, points, sx_min .. sz_max, sum_px, sum_py, sum_pz, var,
        kind; centroid and normal are [K, 3]) for the patches of at least min_size nodes in ascending label, `counts` ([4]: those
        patches, candidates, patches of any size, 0) and, with labels=True, `labels` (int32 per row of export(): its patch's label, -1
        for a row that is no candidate).  kind: PATCH_HORIZONTAL (|normal_z| >= cos(level_deg)), PATCH_VERTICAL (<= sin(level_deg)) or
        PATCH_INCLINED, and PATCH_SLOPES_ONLY.  Labels, counts and integer fields are exact; centroid, normal and var are fp64 sums added
        with atomics, equal to rounding from run to run.  box, max_patches, stream and host are frontiers()'s box, max_clusters,
        stream and host: device lists keep max_patches entries with nodes 0 behind the counts[0] found, host lists are cut."""
        if self._h is None:
            self._handle()
        prm = self.patch_params(candidates, connectivity, max_angle_deg, max_offset, max_var, level_deg, min_size)
        b = C.byref(CropBox(*[int(v) for v in box])) if box is not None else None
        n = int(self.sync()[0]) if labels else 0
        be = HostArrays if host else DeviceArrays(self._cuda(), stream)
        with be.ctx():
            counts = be.zeros(4, np.uint32)
            label = be.empty(n, np.int32) if labels else None
        call = lambda recs, cap: self._call(be, "patches", b, C.byref(prm), be.ptr(label), be.ptr(recs) if cap else C.c_void_p(0), cap, be.addr(counts))
        if max_patches is None:
            call(None, 0)
            with be.ctx():                              # (read on the stream the count was enqueued on: the copy waits for it)
                max_patches = int(counts[0])
        with be.ctx():
            recs = be.records(int(max_patches), _lib.PATCH)
        call(recs, len(recs))
        if host:
            recs = recs[:min(int(counts[0]), len(recs))]
        out = be.fields(recs, _lib.PATCH)
        out["counts"] = counts
        if labels:
            out["labels"] = label
        return out

    def patch_planes(self, p):
        """The planes of patches(): (centroids [K, 3], unit normals [K, 3], offsets [K] = normal . centroid) in world coordinates, fp64;
        numpy in, numpy out; torch in, torch out.  An entry of nodes 0 (behind the patches found) gives NaN."""
        cen, nrm = p["centroid"], p["normal"]
        on_dev = not isinstance(cen, np.ndarray)
        cen, nrm = (cen.clone(), nrm.clone()) if on_dev else (cen.copy(), nrm.copy())
        none = p["nodes"] == 0
        cen[none] = float("nan")
        nrm[none] = float("nan")
        return cen, nrm, (cen * nrm).sum(1)

    def patch_rows(self, p, labels, which):
        """The member rows of patch `which` (an index into the lists of p = patches(..., labels=True)) in ascending order: int64, numpy
        or torch as `labels` is"""
        label = int(p["label"][which])
        if isinstance(labels, np.ndarray):
            return np.flatnonzero(labels == label).astype(np.int64)
        import torch
        return torch.nonzero(labels == label).reshape(-1)

    # ---- clearance field (gndt_clearance*: per slope the steps to the nearest barrier, and where it is) ----
    CLEARANCE_SOURCES = {"blocked": 1, "open": 2, "overhead": 4}
    CLEARANCE_BEYOND = -1      # GNDT_CLEARANCE_BEYOND as the int32 the hops come back in

    def clearance(self, robot=None, max_hops=32, sources=("blocked",), hops=True, nearest=True, sides=False, stream=None, host=False):
        """How far every slope is from the nearest barrier (include/gndt.h "clearance field" defines every word).  A step goes from a
        slope to a slope of a neighbour column that passes the flood's gates for `robot` (computeCost's dict; None = its defaults); a
        side whose column is in the map but offers no step is blocked, a side without a column is open.  sources: which slopes count
        as barriers, any of "blocked" (a blocked side), "open" (an open side: the map's edge), "overhead" (a surface within 2 radius
        above), or the bit mask.  Returns a dict with, per row of export(): `hops` (int32: the steps of the shortest walk to a source,
        0 for a source, -1 = CLEARANCE_BEYOND for more than max_hops, for none and for a row without a slope), `nearest` (int32: the
        smallest source row that many steps away, -1 = NO_ROW), `sides` (uint8: bits 0-3 the blocked sides, 4-7 the open ones, in
        the order left, right, forward, back; 0xFF for a row without a slope) — each only when asked for — and `counts` ([4]: sources,
        slopes with finite hops, the largest finite hops, 0).  Torch tensors on the handle's device, enqueued on `stream` (default
        torch's current stream) and not awaited; or numpy arrays through gndt_clearance with host=True."""
        if self._h is None:
            self._handle()
        if isinstance(sources, str):
            sources = (sources,)
        mask = int(sources) if not hasattr(sources, "__iter__") else sum({self.CLEARANCE_SOURCES[s] for s in sources})
        prm = ClearanceParams(mask, int(max_hops))
        rb = self._robot_ref(robot)
        want = {"hops": (hops, np.int32), "nearest": (nearest, np.int32), "sides": (sides, np.uint8)}
        n = int(self.sync()[0])
        room = max(n, 1)           # (an empty map still names its outputs: a NULL one means "not asked for")
        be = HostArrays if host else DeviceArrays(self._cuda(), stream)
        with be.ctx():
            out = {k: be.empty(room, dt) for k, (on, dt) in want.items() if on}
            out["counts"] = be.zeros(4, np.int32)
        self._call(be, "clearance", rb, C.byref(prm), *[be.ptr(out.get(k)) for k in ("hops", "nearest", "sides", "counts")])
        for k in want:
            if k in out:
                out[k] = out[k][:n]
        return out

    def clearance_vectors(self, cl):
        """[N, 3] float32 per row of export(): mean[nearest] - mean[row] for the `nearest` of clearance(), NaN where there is none — the
        direction to the barrier that `hops` names (a repulsive term pushes the other way), its norm the straight-line distance.  A
        gather and a subtraction on the exported means: torch in, torch out (export_device()); numpy in, numpy out (export())."""
        near = cl["nearest"]
        if isinstance(near, np.ndarray):
            mean = self.export()["mean"]
            none = near < 0
            vec = mean[np.where(none, 0, near)] - mean
            vec[none] = np.float32("nan")
            return vec
        import torch
        cells = self.export_device()
        if int(cells["num_nodes"]) == 0:
            return torch.zeros((0, 3), dtype=torch.float32, device=near.device)
        mean = cells["mean"]
        none = near < 0
        vec = mean[near.long().clamp(min=0)] - mean
        vec[none] = float("nan")
        return vec

    # ---- obstacle field (gndt_obstacle_field*: hops to the slopes a list of boxes stands on, for walk_paths / shortcut_routes) ----
    def obstacle_field(self, boxes, robot=None, inflate=0, max_hops=8, levels_above=None, levels_below=0, base=None, max_columns=0,
                       obstacle=True, stream=None, host=False):
        """How far every slope is from the nearest slope a transient obstacle stands on (include/gndt.h "obstacle field" defines every
        word).  boxes: [B, 6] int32 signed cell indices (sx_min, sx_max, sy_min, sy_max, sz_min, sz_max; index_boxes() makes them from
        world boxes), numpy or torch — or the dict segment_scan() returned for a device scan: its records and counts[0] are then read
        where they lie, nothing comes back to the host in between.  A box covers the slopes of the columns within `inflate` columns
        of it whose level lies within levels_above levels under / levels_below over the box (levels_above=None: ceil(2 radius /
        zLen), the robot's body); steps are clearance()'s for `robot`.  base: a clearance()'s `hops` (or its dict) to minimise with.
        max_columns: the budget of the boxes' windows (0 = 2^24), boxes beyond it are dropped and counted.  Returns a dict with, per
        row of export(), `hops` (int32, -1 = CLEARANCE_BEYOND; what walk_paths(hops=...) takes) and, with obstacle=True, `obstacle`
        (int32: the least box index that many steps away, -1 = none; the base plays no part), and `counts` ([8]: covered slopes,
        slopes with finite obstacle hops, the largest of those, boxes, boxes covering a slope, slopes in reach, dropped boxes, 0).
        Torch tensors on the handle's device, enqueued on `stream` (default torch's current stream) and not awaited, for torch boxes
        or a segment_scan() dict; numpy arrays through gndt_obstacle_field for numpy boxes or host=True."""
        if self._h is None:
            self._handle()
        rb, d = self._robot(robot)
        if levels_above is None:
            levels_above = int(np.ceil(2.0 * float(d["radius"]) / self.zLen))
        prm = ObstacleParams(int(inflate), int(max_hops), int(levels_above), int(levels_below), int(max_columns))
        if isinstance(base, dict):
            base = base["hops"]
        n = int(self.sync()[0])
        room = max(n, 1)
        if base is not None and int(base.shape[0]) != n:
            raise ValueError(f"base has {int(base.shape[0])} entries, the map {n} rows: a clearance field of another map")
        count_dev = None
        if isinstance(boxes, dict):                        # segment_scan()'s answer
            if isinstance(boxes["label"], np.ndarray) or host:
                to_np = lambda v: v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)
                six = np.stack([to_np(boxes[k]) for k in ("sx_min", "sx_max", "sy_min", "sy_max", "sz_min", "sz_max")], 1)
                boxes = six[:min(int(to_np(boxes["counts"])[0]), len(six))]
            else:                                          # on the device: the records where they lie, cut by counts[0] there
                boxes, count_dev = boxes["sx_min"], boxes["counts"]
        on_dev = hasattr(boxes, "is_cuda") and boxes.is_cuda and not host
        be = DeviceArrays(boxes.device, stream) if on_dev else HostArrays
        if count_dev is not None:
            keep, nb, stride = boxes, int(boxes.shape[0]), 4 * int(boxes.stride(0)) if boxes.shape[0] else 72
        else:
            keep = be.here(boxes, np.int32).reshape(-1, 6)
            nb, stride = int(keep.shape[0]), 24
        with be.ctx():
            out = {"hops": be.empty(room, np.int32)}
            if obstacle:
                out["obstacle"] = be.empty(room, np.int32)
            out["counts"] = be.zeros(8, np.int32)
            bs = be.here(base, np.int32)
        # (only the device twin can read the box count where a device scan left it)
        self._call(be, "obstacle_field", rb, be.ptr(keep), nb, stride, *([be.ptr(count_dev)] if be.on_dev else []), C.byref(prm), be.ptr(bs),
                   be.ptr(out["hops"]), be.ptr(out.get("obstacle")), be.ptr(out["counts"]))
        for k in ("hops", "obstacle"):
            if k in out:
                out[k] = out[k][:n]
        return out

    def index_boxes(self, lo, hi):
        """World boxes (lo, hi: [B, 3] corners, lo <= hi) -> [B, 6] int32 index boxes (sx_min, sx_max, sy_min, sy_max, sz_min, sz_max)
        for obstacle_field(), each corner keyed as the map keys a point (transMortonXYZ's arithmetic).  A corner without a key (not
        finite, or beyond the key range) gives a void box (1, 0, 1, 0, 1, 0).  Host arithmetic; numpy out."""
        lo = np.asarray(lo.cpu() if hasattr(lo, "cpu") else lo, np.float32).reshape(-1, 3)
        hi = np.asarray(hi.cpu() if hasattr(hi, "cpu") else hi, np.float32).reshape(-1, 3)
        assert lo.shape == hi.shape
        out = np.empty((len(lo), 6), np.int32)
        for b in range(len(lo)):
            ka, kb = (trans_morton_xyz(self.cloudFirst, self.gridLen, self.zLen, c) if np.isfinite(c).all() else (1,) for c in (lo[b], hi[b]))
            if ka[0] or kb[0]:
                out[b] = (1, 0, 1, 0, 1, 0)
                continue
            # the key's quadrant letter carries the signs of the two magnitudes: A (+,+)  B (+,-)  C (-,+)  D (-,-)
            (ax, ay, az), (bx, by, bz) = ((k[2] if k[1][0] in "AB" else -k[2], k[3] if k[1][0] in "AC" else -k[3], k[4]) for k in (ka, kb))
            out[b] = (ax, bx, ay, by, az, bz)
        return out

    # ---- path walks (gndt_walk_paths*: candidate polylines driven over the map's slopes under the flood's gates) ----
    WALK_STATUS = {0: "done", 1: "no_start", 2: "blocked", 3: "left_map", 4: "overhead", 5: "too_close", 6: "limit"}
    WALK_START_MODES = {"nearest_slope": 1, "node": 2}
    WALK_NO_SIDE = -1          # GNDT_WALK_NO_SIDE as the int32 stop_side comes back in
    WALK_INFO_DTYPE = _lib.WALK_INFO

    def walk_paths(self, paths, robot=None, start_mode="nearest_slope", overhead=False, hops=None, min_hops=0, max_steps=0, rows=0,
                   stream=None, host=False):
        """Drive K candidate paths of T waypoints over the map (include/gndt.h "path walks" defines every word).  paths: [K, T, 3] or
        [K, T, 4] float32, a torch CUDA tensor or a numpy array; a waypoint whose x or y is NaN ends its path.  From the slope under
        waypoint 0 (start_mode "nearest_slope" or "node") every segment is crossed column by column, each column change a step
        through the flood's gates for `robot` (computeCost's dict; None = its defaults) to the slope nearest in height.  overhead=True
        also stops under a surface too low for the robot; hops (what clearance() returned, or its "hops") with min_hops stops at a
        slope nearer than that to a barrier — the field must be of the map as it is now.  max_steps 0 = 65536.  rows > 0 also
        returns the first `rows` slopes of every walk.  Returns a dict of [K] arrays: status (WALK_STATUS), stop_side (0..3, -1 =
        none), steps, waypoints, start_row, end_row (-1 = none), length, climb, rough_max, hops_min (-1 = no hops given or seen), and
        `rows` [K, rows] (int32, -1 behind a walk's end) when asked.  torch tensors on the paths' device, enqueued on `stream` (default
        torch's current stream) and not awaited; host=True or a numpy array goes through gndt_walk_paths (numpy)."""
        if self._h is None:
            self._handle()
        on_dev = hasattr(paths, "is_cuda") and paths.is_cuda and not host
        if hasattr(paths, "detach") and not on_dev:
            paths = paths.detach().cpu().numpy()
        if len(paths.shape) != 3 or paths.shape[2] not in (3, 4):
            raise ValueError("paths must be [K, T, 3] or [K, T, 4]")
        K, T, stride = int(paths.shape[0]), int(paths.shape[1]), 4 * int(paths.shape[2])
        if isinstance(hops, dict):
            hops = hops["hops"]
        prm = WalkParams(_enum(self.WALK_START_MODES, start_mode), 1 if overhead else 0, int(min_hops), int(max_steps))
        rb = self._robot_ref(robot)
        row_cap = int(rows)
        n = int(self.sync()[0])
        if hops is not None and int(hops.shape[0]) != n:
            raise ValueError(f"hops has {int(hops.shape[0])} entries, the map {n} rows: a clearance field of another map")
        be = DeviceArrays(paths.device, stream) if on_dev else HostArrays
        with be.ctx():
            p = be.here(paths, np.float32)
            hp = be.here(hops, np.int32)
            raw = be.records(max(K, 1), _lib.WALK_INFO)
            out_rows = be.empty((K, row_cap), np.int32) if row_cap else None
        self._call(be, "walk_paths", be.ptr(p), K, T, stride, rb, C.byref(prm), be.ptr(hp), be.addr(out_rows) if row_cap else None, row_cap,
                   be.addr(raw))
        out = be.fields(raw[:K], _lib.WALK_INFO)
        if row_cap:
            out["rows"] = out_rows
        return out

    # ---- route field (gndt_route_field* / gndt_descend_routes*: cost-to-go to a set of goals that keeps clear of obstacles) ----
    def route_field(self, goals, goal_costs=None, robot=None, hops=None, min_hops=0, soft_hops=0, soft_weight=0.0, overhead=False, max_cost=0.0,
                    max_rounds=0, next=True, stream=None, host=False):
        """For every slope the least cost to reach any of `goals` along the steps a robot can take, and the slope to step to next
        (include/gndt.h "route field" defines every word).  goals: [G] rows of export() or [G, 3] points (looked up with query mode
        "nearest_slope"; a point without a slope is an ignored goal); goal_costs: [G] float32 or None = zeros.  hops (what clearance()
        or obstacle_field() returned, or its "hops") with min_hops forbids entering a slope nearer than that to a barrier, with
        soft_hops / soft_weight makes slopes inside that zone cost 1 + soft_weight * (soft_hops - hops) times as much to enter;
        overhead=True forbids slopes under a surface too low for `robot`.  max_cost > 0 cuts the field there; max_rounds bounds the
        sweeps (0 = 1024) — on a map of more than 20 448 rows every one of them is a launch of about 3 us whether it still has work or
        not, so a caller who knows how deep the map is says so.  Returns a dict: `cost` (float32 per row of export(), FLT_MAX where no route exists), `next` (int32, -1 =
        NO_ROW; only with next=True), `counts` ([8]: accepted goals, ignored goals, slopes with a finite cost, the bits of the largest,
        converged, sweeps that changed something, 0, 0) and `converged` (counts[4], a view: reading it waits for the stream).  Torch
        tensors on the handle's device, enqueued on `stream` (default torch's current stream) and not awaited; or numpy arrays through
        gndt_route_field with host=True."""
        if self._h is None:
            self._handle()
        if isinstance(hops, dict):
            hops = hops["hops"]
        n = int(self.sync()[0])
        if hops is not None and int(hops.shape[0]) != n:
            raise ValueError(f"hops has {int(hops.shape[0])} entries, the map {n} rows: a field of another map")
        prm = RouteFieldParams(1 if overhead else 0, int(min_hops), int(soft_hops), float(soft_weight), float(max_cost), int(max_rounds))
        rb = self._robot_ref(robot)
        room = max(n, 1)           # (an empty map still names its outputs: a NULL one means "not asked for")
        if len(goals.shape) == 2:  # points -> rows
            if goals.shape[1] not in (3, 4):
                raise ValueError("goals must be [G] rows or [G, 3] points")
            if host and hasattr(goals, "detach"):
                goals = goals.detach().cpu().numpy()
            if not host and isinstance(goals, np.ndarray):
                import torch
                goals = torch.as_tensor(np.ascontiguousarray(goals, np.float32), device=f"cuda:{self.device}")
            goals = self.query(goals, "nearest_slope", stream=stream)
        G = int(goals.shape[0])
        if goal_costs is not None and int(goal_costs.shape[0]) != G:
            raise ValueError("goal_costs must have one entry per goal")
        be = HostArrays if host else DeviceArrays(self._cuda(), stream)
        with be.ctx():
            g, gc, hp = be.here(goals, np.int32), be.here(goal_costs, np.float32), be.here(hops, np.int32)
            out = {"cost": be.empty(room, np.float32), "counts": be.zeros(8, np.int32)}
            if next:
                out["next"] = be.empty(room, np.int32)
        self._call(be, "route_field", rb, C.byref(prm), be.ptr(g), G, be.ptr(gc), be.ptr(hp), be.ptr(out["cost"]), be.ptr(out.get("next")),
                   be.ptr(out["counts"]))
        for k in ("cost", "next"):
            if k in out:
                out[k] = out[k][:n]
        out["converged"] = out["counts"][4]
        return out

    def descend_routes(self, starts, field, start_mode="nearest_slope", route_cap=None, max_steps=0, stream=None, host=False):
        """Routes from `starts` ([K,3] or [K,4] float32) down a route_field() of this map as it is now, by following its `next`
        (include/gndt.h "route field").  Returns (rows, info) in plan_routes' layout, which shortcut_routes and route_waypoints take
        as they are: rows [K, route_cap] int32, start first and goal last, -1 behind; info a dict of [K] arrays status
        (ROUTE_STATUS), length, start_row, expansions (the steps followed), queue_peak (0), cost and h_start (the field's cost at the
        start).  route_cap None: the map's slope count or 1024, whichever is less.  torch CUDA starts are answered on the device
        (enqueued on `stream`, not awaited); host=True or a host array goes through gndt_descend_routes (numpy)."""
        if self._h is None:
            self._handle()
        if "next" not in field:
            raise ValueError("descend_routes needs a field with `next` (route_field(next=True))")
        ptr, K, stride, on_dev, keep = self._as_input(starts)
        n, _, slopes = (int(v) for v in self.sync())
        if route_cap is None:
            route_cap = max(min(slopes, 1024), 1)
        route_cap = int(route_cap)
        cost, nxt = field["cost"], field["next"]
        if int(cost.shape[0]) != n or int(nxt.shape[0]) != n:
            raise ValueError(f"the field has {int(cost.shape[0])} entries, the map {n} rows: a field of another map")
        prm = DescendParams(_enum(self.WALK_START_MODES, start_mode), int(max_steps))
        if on_dev and host:
            ptr, K, stride, on_dev, keep = self._as_input(keep.detach().cpu().numpy())
        be = DeviceArrays(keep.device, stream) if on_dev else HostArrays
        with be.ctx():
            c, x = be.here(cost, np.float32), be.here(nxt, np.int32)
            rows = be.empty((K, route_cap), np.int32)
            raw = be.records(max(K, 1), _lib.ROUTE_INFO, zeroed=False)[:K]
            if n == 0:             # (an empty map still names its field)
                c, x = be.zeros(1, np.float32), be.zeros(1, np.int32)
        self._call(be, "descend_routes", C.c_void_p(ptr if K else 0), K, stride, C.byref(prm), be.addr(c), be.addr(x), be.ptr(rows),
                   route_cap if K else 0, be.addr(raw))
        return rows, be.fields(raw, _lib.ROUTE_INFO, _ROUTE_HOST_AS)

    # ---- route shortcutting (gndt_shortcut_routes*: slope-to-slope routes string-pulled into any-angle waypoints) ----
    SHORTCUT_STATUS = {0: "ok", 1: "empty", 2: "bad_route", 3: "limit"}
    SHORTCUT_INFO_DTYPE = _lib.SHORTCUT_INFO

    def shortcut_routes(self, routes, lengths=None, robot=None, window=64, overhead=False, hops=None, min_hops=0, waypoint_cap=None, path_cap=0,
                        max_links=0, stream=None, host=False):
        """String-pull K routes into any-angle waypoints (include/gndt.h "route shortcutting" defines every word).  routes: what
        plan_routes() returned — its rows and its info, whose lengths are read where they lie — or a [K, route_cap] int32 rows array
        with `lengths` ([K] int32).  From every anchor the farthest row of the next `window` (at most 256) that the robot can drive to
        in a straight line becomes the next anchor: the link is the path walk between the two columns' centres under the flood's gates
        for `robot` (computeCost's dict; None = its defaults), with overhead / hops / min_hops as in walk_paths; where no link holds
        the route's own next row is kept.  waypoint_cap None = route_cap; path_cap > 0 also returns the slopes stood on; max_links 0 =
        2^20 candidates a route.  Returns a dict of [K] arrays status (SHORTCUT_STATUS), length_in, waypoints, path_slopes,
        links_tested, fallback_links, cost_in, cost_out, hops_min (-1 = no hops given), `waypoint_rows` [K, waypoint_cap] and with
        path_cap `path_rows` [K, path_cap] (int32, -1 behind the end).  torch tensors on the routes' device, enqueued on `stream`
        (default torch's current stream) and not awaited; host=True or numpy arrays go through gndt_shortcut_routes (numpy)."""
        if self._h is None:
            self._handle()
        if isinstance(routes, (tuple, list)) and len(routes) == 2 and isinstance(routes[1], dict):
            routes, lengths = routes[0], routes[1]["length"]
        if lengths is None:
            raise ValueError("shortcut_routes: rows need their lengths")
        on_dev = hasattr(routes, "is_cuda") and routes.is_cuda and not host
        if len(routes.shape) != 2 or int(lengths.shape[0]) != int(routes.shape[0]) or len(lengths.shape) != 1:
            raise ValueError("routes must be [K, route_cap] and lengths [K]")
        K, route_cap = int(routes.shape[0]), int(routes.shape[1])
        wp_cap = route_cap if waypoint_cap is None else int(waypoint_cap)
        path_cap = int(path_cap)
        if isinstance(hops, dict):
            hops = hops["hops"]
        prm = ShortcutParams(int(window), 1 if overhead else 0, int(min_hops), int(max_links))
        rb = self._robot_ref(robot)
        n = int(self.sync()[0])
        if hops is not None and int(hops.shape[0]) != n:
            raise ValueError(f"hops has {int(hops.shape[0])} entries, the map {n} rows: a clearance field of another map")
        be = DeviceArrays(routes.device, stream) if on_dev else HostArrays
        with be.ctx():
            r = be.here(routes, np.int32)
            # the lengths are read where they lie (plan_routes' info is a column of its records): 4-byte integers at any whole stride
            if be.on_dev:
                ln = be.xp.as_tensor(lengths, device=r.device)
                if ln.dtype != be.xp.int32 or (K > 1 and ln.stride(0) < 1):
                    ln = be.here(ln, np.int32)
                stride = 4 * int(ln.stride(0)) if K > 1 else 4
            else:
                ln = lengths.detach().cpu().numpy() if hasattr(lengths, "detach") else np.asarray(lengths)
                if ln.dtype.itemsize != 4 or ln.dtype.kind not in "iu" or (K > 1 and (ln.strides[0] < 4 or ln.strides[0] % 4)):
                    ln = np.ascontiguousarray(ln, np.int32)
                stride = int(ln.strides[0]) if K > 1 else 4
            hp = be.here(hops, np.int32)
            raw = be.records(max(K, 1), _lib.SHORTCUT_INFO)
            wp = be.empty((K, wp_cap), np.int32)
            out_path = be.empty((K, path_cap), np.int32) if path_cap else None
        self._call(be, "shortcut_routes", be.ptr(r), K, route_cap, be.ptr(ln), stride, rb, C.byref(prm), be.ptr(hp),
                   be.addr(wp if K and wp_cap else raw), wp_cap, be.addr(out_path) if path_cap else None, path_cap, be.addr(raw))
        out = be.fields(raw[:K], _lib.SHORTCUT_INFO)
        out["waypoint_rows"] = wp
        if path_cap:
            out["path_rows"] = out_path
        return out

    def route_waypoints(self, rows):
        """World points [K, cap, 3] float32 of routes of rows ([K, cap] int32, -1 behind a route's end: plan_routes' rows, or
        shortcut_routes' waypoint_rows / path_rows): the centre of each row's column — per axis (float)(o + sign(s) (|s| - 0.5)
        grid_len) in fp64, the points the shortcut's links run between — and the row's mean z; NaN behind the end, which is the walks'
        terminator: the result goes into walk_paths as it is.  Torch in, torch out (export_device()); numpy in, numpy out (export())."""
        on_dev = not isinstance(rows, np.ndarray)
        cells = self.export_device() if on_dev else self.export()
        o = [float(np.float32(v)) for v in self.cloudFirst]
        g = float(np.float32(self.gridLen))
        if on_dev:
            import torch
            pts = torch.full(tuple(rows.shape) + (3,), float("nan"), dtype=torch.float32, device=rows.device)
            if int(cells["num_nodes"]) == 0 or rows.numel() == 0:
                return pts
            live = rows >= 0
            at = rows.long().clamp(min=0)
            for a, k in enumerate(("sx", "sy")):
                s = cells[k][at].double()
                pts[..., a] = (o[a] + torch.sign(s) * (s.abs() - 0.5) * g).float()
            pts[..., 2] = cells["mean"][at, 2]
            pts[~live] = float("nan")
            return pts
        pts = np.full(rows.shape + (3,), np.nan, np.float32)
        if int(cells["num_nodes"]) == 0 or rows.size == 0:
            return pts
        live = rows >= 0
        at = np.where(live, rows, 0).astype(np.int64)
        for a, k in enumerate(("sx", "sy")):
            s = cells[k][at].astype(np.float64)
            pts[..., a] = (o[a] + np.sign(s) * (np.abs(s) - 0.5) * g).astype(np.float32)
        pts[..., 2] = cells["mean"][at, 2]
        pts[~live] = np.nan
        return pts

    # ---- footprint poses (gndt_footprint_poses*: the plane under a rectangular vehicle, its tilt, step and headroom) ----
    FOOT_STATUS = {0: "ok", 1: "bad_pose", 2: "no_ground", 3: "sparse"}
    FOOT_FLAGS = {"tilt": 1, "step": 2, "cover": 4, "low": 8}
    FOOT_WEIGHTS = {"cell": 0, "count": 1}
    FOOT_INFO_DTYPE = _lib.FOOTPRINT_INFO

    def footprints(self, poses, half_length, half_width, robot=None, max_dz=0.0, height=0.0, min_cells=0, min_cover=0.0, weight="cell",
                   rows=0, stream=None, host=False):
        """The stance of a rectangular vehicle at K poses (include/gndt.h "footprint poses" defines every word).  poses: [K, 5] float32
        x, y, z, hx, hy with (hx, hy) the heading as a vector of any non-zero length, or [K, 4] x, y, z, yaw, from which the vector
        (cos yaw, sin yaw) is formed here; a torch CUDA tensor or a numpy array.  The rectangle reaches half_length along the heading
        and half_width across it, each way.  Under it the map's slopes nearest the centre slope (within max_dz of it, 0 = any) merge
        into one Gaussian whose flattest direction is the supporting plane.  robot: computeCost's dict (None = its defaults;
        reachable_height and max_angle_deg are read).  height > 0 asks for the headroom verdict, min_cells (0 = 3) and min_cover for
        the sparse status and the cover verdict, weight "cell" or "count".  rows > 0 also returns the first `rows` supports of every
        pose in box order.  Returns a dict of [K] arrays: status (FOOT_STATUS), flags (FOOT_FLAGS bits), centre_row (-1 = none),
        cells, support, gaps, unknown, z, normal [K, 3], along, across (rise per metre), rms, step_max, bump_max, headroom, and
        pitch = arctan(along), roll = arctan(across), ok = (status == 0) & (flags == 0); `rows` [K, rows] (int32, -1 behind the
        last) when asked.  torch tensors on the poses' device, enqueued on `stream` (default torch's current stream) and not
        awaited; host=True or a numpy array goes through gndt_footprint_poses (numpy)."""
        if self._h is None:
            self._handle()
        on_dev = hasattr(poses, "is_cuda") and poses.is_cuda and not host
        if hasattr(poses, "detach") and not on_dev:
            poses = poses.detach().cpu().numpy()
        if len(poses.shape) != 2 or poses.shape[1] not in (4, 5):
            raise ValueError("poses must be [K, 5] (x, y, z, hx, hy) or [K, 4] (x, y, z, yaw)")
        K = int(poses.shape[0])
        prm = FootprintParams(float(half_length), float(half_width), float(max_dz), float(height), int(min_cells), float(min_cover),
                              _enum(self.FOOT_WEIGHTS, weight))
        rb = self._robot_ref(robot)
        row_cap = int(rows)
        be = DeviceArrays(poses.device, stream) if on_dev else HostArrays
        xp = be.xp
        with be.ctx():
            p = be.here(poses, np.float32)
            if p.shape[1] == 4:
                p = xp.concatenate([p[:, :3], xp.cos(p[:, 3:4]), xp.sin(p[:, 3:4])], 1)
            raw = be.records(max(K, 1), _lib.FOOTPRINT_INFO)
            out_rows = be.empty((K, row_cap), np.int32) if row_cap else None
        # (K = 0: no poses is a NULL pointer, and rows NULL goes with a cap of 0)
        self._call(be, "footprint_poses", be.ptr(p), K, 20, rb, C.byref(prm), be.addr(out_rows) if row_cap and K else None,
                   row_cap if K else 0, be.addr(raw))
        with be.ctx():
            out = be.fields(raw[:K], _lib.FOOTPRINT_INFO, host_as=_FOOT_HOST_AS)
            out["pitch"], out["roll"] = xp.arctan(out["along"]), xp.arctan(out["across"])
            out["ok"] = (out["status"] == 0) & (out["flags"] == 0)
        if row_cap:
            out["rows"] = out_rows
        return out

    def footprints_along(self, paths, half_length, half_width, **kw):
        """footprints() at every waypoint of K paths of T waypoints ([K, T, 3|4], walk_paths' layout: a waypoint whose x or y is NaN
        ends its path), each heading the vector to the next finite waypoint (rollouts.headings).  Returns footprints()' dict with
        [K, T] fields (normal [K, T, 3]; rows [K, T, rows]) and `stands` [K]: every waypoint before the path's terminator is ok.  A
        waypoint at or behind the terminator has status bad_pose and does not count against its path; another bad pose does."""
        from . import rollouts
        poses = rollouts.headings(paths)
        K, T = int(poses.shape[0]), int(poses.shape[1])
        out = self.footprints(poses.reshape(K * T, 5), half_length, half_width, **kw)
        out = {k: v.reshape((K, T) + tuple(v.shape[1:])) for k, v in out.items()}
        ended = poses[..., 0] != poses[..., 0]          # (headings' NaN at and behind the terminator)
        if hasattr(out["ok"], "is_cuda") and not hasattr(ended, "is_cuda"):
            import torch
            ended = torch.as_tensor(ended, device=out["ok"].device)
        elif hasattr(ended, "is_cuda") and not hasattr(out["ok"], "is_cuda"):
            ended = ended.cpu().numpy()
        out["stands"] = (out["ok"] | ended).all(1)
        return out

    # ---- free-space clearing (gndt_clear_rays*: nodes that sensor rays pass through leave the map) ----
    CLEAR_PROTECTED = 0x80000000

    def clear_rays(self, origin, points, max_range=0.0, end_margin=0.0, min_passes=1, count_only=False, passes=False, stream=None):
        """Drop every node that at least `min_passes` rays from the sensor `origin` (xyz) to the end `points` ([N,3] or [N,4] float32)
        pass through, unless an end point lies in it (include/gndt.h "free-space clearing" defines the walk).  max_range > 0 walks at
        most that far from the origin, end_margin leaves the last metres before every end point.  count_only=True changes nothing: the
        dry run.  A torch CUDA tensor is walked on the device (enqueued on `stream`, default torch's current stream), a host array
        through gndt_clear_rays.  Returns the stats dict {rays, skipped, protected_rows, cleared}; with passes=True also the per-row
        words of the map as it was before the call (bits 0-30 the pass count, bit 31 CLEAR_PROTECTED): a torch int32 tensor on the device
        for device points, a numpy uint32 array otherwise: (stats, passes).  The stats are awaited, so the call always waits."""
        if self._h is None:
            self._handle()
        o = (C.c_float * 3)(*[float(v) for v in origin[:3]])
        prm = ClearParams(float(max_range), float(end_margin), int(min_passes), 1 if count_only else 0)
        st = ClearStats()
        ptr, n, stride, on_dev, keep = self._as_input(points)
        be = DeviceArrays(keep.device, stream) if on_dev else HostArrays
        rows = be.zeros(self.sync()[0], np.uint32) if passes else None
        self._call(be, "clear_rays", o, C.c_void_p(ptr if n else 0), n, stride, C.byref(prm), be.ptr(rows), C.byref(st))
        out = {"rays": int(st.rays), "skipped": int(st.skipped), "protected_rows": int(st.protected_rows), "cleared": int(st.cleared)}
        return (out, rows) if passes else out

    # ---- ray casting (gndt_cast_rays*: the first map node along each ray of a batch) ----
    CAST_MODES = {"voxel": 0, "ndt": 1}

    def cast_rays(self, origins, ends, mode="voxel", min_count=0, max_range=0.0, min_range=0.0, cov_rel=0.0, cov_floor=0.0, max_d2=0.0,
                  stats=False, stream=None):
        """Where every ray from `origins` ((3,): one origin for all; or [N,3] / [N,4] float32) to `ends` ([N,3] or [N,4] float32) first
        hits the map (include/gndt.h "ray casting" defines the answer).  mode "voxel": the first node with count >= min_count (0 = 1)
        the walk visits, the range to where the ray enters its voxel; "ndt": nodes with statistics (min_count 0 = max(min_points, 3)),
        the range to the point of the ray nearest the node's distribution (cov_rel, cov_floor as in score_poses; max_d2 > 0: a node
        the ray passes farther from than this does not stop it).  max_range > 0 walks at most that far, candidates nearer than
        min_range do not count.  Returns {"row" (int32, -1: none), "range", "d2" (float32: inf for a miss, NaN for a skipped ray)}: torch
        tensors for torch CUDA ends (enqueued on `stream`, default torch's current stream, not awaited), numpy arrays through
        gndt_cast_rays otherwise.  stats=True waits and returns (that dict, {rays, skipped, hits})."""
        if self._h is None:
            self._handle()
        prm = CastParams(_enum(self.CAST_MODES, mode), int(min_count), float(max_range), float(min_range),
                         float(cov_rel), float(cov_floor), float(max_d2), 0)
        eptr, n, estride, on_dev, keep = self._as_input(ends)
        st = CastStats()
        be = DeviceArrays(keep.device, stream) if on_dev else HostArrays
        with be.ctx():      # (the origins' upload and the outputs belong to the stream the kernel runs on)
            o = be.here(origins, np.float32)
            # (one element at least: the call wants an output pointer whatever n is)
            buf = {k: be.empty(max(n, 1), dt) for k, dt in (("row", np.int32), ("range", np.float32), ("d2", np.float32))}
        co = CastOut(*[be.addr(buf[k]) for k in ("row", "range", "d2")])
        oshape = tuple(o.shape)
        if len(oshape) == 1 and oshape[0] in (3, 4):
            ostride = 0
        elif len(oshape) == 2 and oshape[0] == n and oshape[1] in (3, 4):
            ostride = 4 * oshape[1]
        else:
            raise ValueError("origins must be (3,) or (n, 3|4) with one row per end point")
        self._call(be, "cast_rays", be.addr(o) if n else None, ostride, C.c_void_p(eptr if n else 0), n, estride, C.byref(prm), C.byref(co),
                   C.byref(st) if stats else None)
        out = {k: v[:n] for k, v in buf.items()}
        if stats:
            return out, {"rays": int(st.rays), "skipped": int(st.skipped), "hits": int(st.hits)}
        return out

    def cast_scan(self, pose, directions, max_range, **kw):
        """The scan a sensor at `pose` (3 x 4 or 4 x 4 [R | t], map <- sensor) expects of the map: one ray per row of `directions`
        ([N,3] unit vectors in the sensor frame) from t to t + max_range * R dir.  The ends are formed on the device in float64,
        end_a = t_a + max_range * ((R_a0 x + R_a1 y) + R_a2 z), and rounded once to float32; the origin is float32(t).  Returns
        cast_rays' result for those rays (keyword arguments are cast_rays'): range is inf where nothing lies within max_range."""
        import torch
        T = self._as_poses(pose)[0].reshape(3, 4)
        dev = f"cuda:{self.device}"
        with _torch_stream_ctx(kw.get("stream")):
            d = (directions if isinstance(directions, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(directions)))
            d = d.to(device=dev, dtype=torch.float64)
            x, y, z = d[:, 0], d[:, 1], d[:, 2]
            ends = torch.stack([float(T[a, 3]) + float(max_range) * ((float(T[a, 0]) * x + float(T[a, 1]) * y) + float(T[a, 2]) * z)
                                for a in range(3)], 1).to(torch.float32)
        return self.cast_rays(np.asarray(T[:, 3], np.float32), ends, **kw)

    # ---- view gain (gndt_view_gain*: the unknown columns a sensor would see from each of K poses) ----
    VIEW_INFO_DTYPE = _lib.VIEW_INFO

    def view_gain(self, poses, directions, max_range, min_count=0, min_range=0.0, per_ray=False, stream=None, host=False):
        """How much a sensor would learn at each of K `poses` ([K, 12], [K, 3, 4], [K, 4, 4] or one matrix, [R | t], map <- sensor): the
        rays t -> t + max_range * R dir of the fan `directions` ([N, 3|4] float32, sensor frame; rollouts.view_directions) are walked
        through the map until a node with count >= min_count (0 = 1) at least min_range away stops them, and the DISTINCT columns they
        cross are counted (include/gndt.h "view gain" defines every word).  Returns a dict of [K] arrays, one per field of
        gndt_view_info: rays, skipped, hits, unknown (crossed columns that are not in the map: what there is to learn), known, status (1:
        the pose's origin is not finite or has no key), steps (column visits: the work), sum_ux, sum_uy (sums of the unknown columns'
        contiguous cell indices: sum / unknown is where the unknown lies); with per_ray=True also `row` and `range` [K, N], cast_rays'
        for every ray.  max_range / grid_len is limited by the LDS of a workgroup (GndtError beyond; coarsen() the map for longer
        ranges).  Torch tensors on the handle's device, enqueued on `stream` (default torch's current stream) and not awaited; numpy
        arrays through gndt_view_gain with host=True."""
        if self._h is None:
            self._handle()
        prm = ViewParams(float(max_range), float(min_range), int(min_count))
        def flat(p):
            """numpy poses -> float64 [K, 12]: also the flat [K, 12] frontier_views returns, and one pose as [12]"""
            p = p.detach().cpu().numpy() if hasattr(p, "detach") else np.asarray(p, np.float64)
            if p.ndim in (1, 2) and p.shape[-1] == 12:
                return np.ascontiguousarray(p, np.float64).reshape(-1, 12)
            return self._as_poses(p)
        be = HostArrays if host else DeviceArrays(self._cuda(), stream)
        with be.ctx():
            if be.on_dev and getattr(poses, "is_cuda", False):          # (poses on the device are shaped there)
                T = poses.to(be.xp.float64)
                if T.dim() == 1:
                    T = T[None]
                elif T.dim() == 2 and T.shape[1] != 12:
                    T = T[None]
                if T.dim() == 3:
                    if T.shape[1] not in (3, 4) or T.shape[2] != 4:
                        raise ValueError("poses must be [K, 12], [K, 3, 4], [K, 4, 4] or one such matrix")
                    T = T[:, :3, :].reshape(-1, 12)
                T = T.contiguous()
            else:
                T = be.here(flat(poses), np.float64)
            d = be.here(directions, np.float32)
            if len(d.shape) != 2 or d.shape[1] not in (3, 4):
                raise ValueError("directions must be [N, 3] or [N, 4]")
            K, n = int(T.shape[0]), int(d.shape[0])
            raw = be.records(K, _lib.VIEW_INFO)
            row = be.full((K, n), -1, np.int32) if per_ray else None
            rng = be.full((K, n), float("nan"), np.float32) if per_ray else None
        self._call(be, "view_gain", be.ptr(T), K, be.ptr(d), n, 4 * int(d.shape[1]), C.byref(prm), be.ptr(raw), be.ptr(row), be.ptr(rng))
        out = be.fields(raw, _lib.VIEW_INFO)    # (views: nothing is enqueued behind the caller's stream)
        if per_ray:
            out.update(row=row, range=rng)
        return out

    def frontier_views(self, fr, yaws=8, height=1.0, which="best"):
        """Candidate sensor poses for view_gain: per cluster of frontiers() and per yaw j * 2 pi / yaws (about the map's z), the pose
        whose origin is frontier_points(fr, which) lifted by `height` and whose x axis (view_directions' forward) looks along the yaw.
        Returns float64 [K * yaws, 12] (pose k * yaws + j; row-major 3 x 4 [R | t]), torch for a torch `fr`, numpy otherwise.  A cluster
        of size 0 gives NaN poses, which view_gain answers with status 1."""
        pts = self.frontier_points(fr, which)
        on_dev = not isinstance(pts, np.ndarray)
        yaws = int(yaws)
        a = np.arange(yaws, dtype=np.float64) * (2.0 * np.pi / yaws)
        R = np.zeros((yaws, 3, 4))
        R[:, 0, 0], R[:, 0, 1], R[:, 1, 0], R[:, 1, 1], R[:, 2, 2] = np.cos(a), -np.sin(a), np.sin(a), np.cos(a), 1.0
        if on_dev:
            import torch
            Rt = torch.from_numpy(R).to(pts.device)
            T = Rt[None].repeat(pts.shape[0], 1, 1, 1)
            t = pts.double()
            t = torch.stack([t[:, 0], t[:, 1], t[:, 2] + float(height)], 1)
            T[:, :, :, 3] = t[:, None, :]
            T[torch.isnan(t).any(1)] = float("nan")
            return T.reshape(-1, 12)
        T = np.repeat(R[None], pts.shape[0], axis=0)
        t = pts.astype(np.float64) + np.array([0.0, 0.0, float(height)])
        T[:, :, :, 3] = t[:, None, :]
        T[np.isnan(t).any(1)] = np.nan
        return T.reshape(-1, 12)

    # ---- scan scoring (gndt_score_poses*: the NDT match score of a scan for a batch of poses) ----
    @staticmethod
    def _as_poses(poses):
        """-> contiguous float64 [K, 12] from [K, 3, 4], [K, 4, 4] (last row dropped) or a single 3 x 4 / 4 x 4 matrix, any float dtype"""
        try:
            import torch
            if isinstance(poses, torch.Tensor):
                poses = poses.detach().cpu().numpy()
        except ImportError:
            pass
        a = np.asarray(poses, dtype=np.float64)
        if a.ndim == 2:
            a = a[None]
        if a.ndim != 3 or a.shape[1] not in (3, 4) or a.shape[2] != 4:
            raise ValueError("poses must be [K, 3, 4], [K, 4, 4] or one such matrix")
        return np.ascontiguousarray(a[:, :3, :]).reshape(a.shape[0], 12)

    def score_poses(self, points, poses, neighbourhood=1, min_count=0, cov_rel=0.0, cov_floor=0.0, max_d2=0.0, per_point=None, stream=None):
        """How well the scan `points` ([N,3] or [N,4] float32) fits the map at each of the K `poses` ([K,3,4] or [K,4,4] or one matrix,
        map <- scan): include/gndt.h "scan scoring" defines the sum.  neighbourhood 1 scores every moved point against the node it falls
        in, 7 also against that node's six face neighbours; 0 takes the default of min_count (max(min_points, 3)), cov_rel (0.01) and
        cov_floor (1e-6 m^2); max_d2 > 0 leaves out candidates beyond that Mahalanobis distance squared.  Returns a dict of length-K
        arrays: score and d2_sum (float64), matched (points with a term) and terms (int64); with per_point=k also d2 (float32, the least
        d2 of every point at pose k, inf where it met no node) and row (int32, that node's row, -1).  A torch CUDA tensor is scored on
        the device (torch tensors, enqueued on `stream`, default torch's current stream, not awaited); a host array through
        gndt_score_poses (numpy)."""
        # (a hot small call: its two branches stay written out, see plan_routes)
        if self._h is None:
            self._handle()
        T = self._as_poses(poses)
        K = T.shape[0]
        ptr, n, stride, on_dev, keep = self._as_input(points)
        want = per_point is not None
        prm = ScoreParams(int(neighbourhood), int(min_count), float(cov_rel), float(cov_floor), float(max_d2), int(per_point) if want else 0)
        if on_dev:
            import torch
            with _torch_stream_ctx(stream):     # (the poses' upload and the outputs belong to the stream the kernels run on)
                Td = torch.from_numpy(T).to(keep.device)
                rec = torch.empty((K, 4), dtype=torch.int64, device=keep.device)
                d2 = torch.empty(n, dtype=torch.float32, device=keep.device) if want else None
                row = torch.empty(n, dtype=torch.int32, device=keep.device) if want else None
            p = lambda t: C.c_void_p(t.data_ptr() if t is not None and t.numel() else 0)
            self._check(self._L.gndt_score_poses_device(self._h, C.c_void_p(ptr if n else 0), n, stride, p(Td), K, C.byref(prm), p(rec),
                                                        p(d2), p(row), _stream_ptr(stream)))
            out = _lib.record_views(rec, _lib.POSE_SCORE)       # (views: nothing is enqueued behind the caller's stream)
        else:
            rec = np.zeros(K, _lib.POSE_SCORE)
            d2 = np.empty(n, np.float32) if want else None
            row = np.empty(n, np.int32) if want else None
            p = lambda a: C.c_void_p(a.ctypes.data if a is not None and a.size else 0)
            self._check(self._L.gndt_score_poses(self._h, C.c_void_p(ptr if n else 0), n, stride, p(T), K, C.byref(prm), p(rec), p(d2), p(row)))
            out = HostArrays.fields(rec, _lib.POSE_SCORE)
        if want:
            out.update(d2=d2, row=row)
        return out

    # ---- scan segmentation (gndt_segment_scan*: the points of a scan the map does not explain, clustered) ----
    SEG_UNKEYED, SEG_EXPLAINED, SEG_OFF_SURFACE, SEG_UNMAPPED = 0, 1, 2, 3
    SEG_CLASSES = {"off_surface": 1 << 2, "unmapped": 1 << 3}
    SEG_DTYPE = _lib.SCAN_CLUSTER

    def segment_scan(self, points, pose=None, neighbourhood=7, novel_d2=0.0, classes=None, min_points=1, connectivity=26,
                     min_cluster_points=1, min_cluster_cells=1, labels=False, max_clusters=None, stream=None, min_count=0, cov_rel=0.0,
                     cov_floor=0.0):
        """What in the scan `points` ([N,3] or [N,4] float32) is not in the map, as clusters (include/gndt.h "scan segmentation" defines
        every word).  pose: one [3,4] / [4,4] matrix, map <- scan (None: the identity).  A point is explained when its least
        Mahalanobis d2 against the node it falls in (neighbourhood 7: and its six face neighbours) is at most novel_d2 (0 = 11.345),
        off_surface when candidates count but none is that near, unmapped when none counts; classes: which of "off_surface" /
        "unmapped" (or the bit mask; None = both) are novel.  Cells of the map's grid with at least min_points novel points that touch
        (connectivity 26 or 6) form a cluster.  Returns a dict with one [K] array per field of gndt_scan_cluster (label, cells,
        off_surface, unmapped, sx_min .. sz_max, sum_x, sum_y, sum_z, z_lo, z_hi) for the clusters of at least min_cluster_points
        points and min_cluster_cells cells in ascending label, `counts` ([4]: those clusters, novel points, novel cells, clusters of
        any size) and, with labels=True, `point_class` (uint8 [N]) and `point_label` (int32 [N]: the label of the point's cluster,
        -1 for none).  max_clusters=None sizes the list from a count-only first call (which waits for it on `stream`); a number is
        the list's capacity — counts[0] may exceed it.  A torch CUDA tensor is segmented on the device (torch tensors, enqueued on
        `stream`, default torch's current stream, not awaited: the arrays then have max_clusters entries, filled from the front); a
        host array through gndt_segment_scan (numpy, cut to min(counts[0], max_clusters) entries)."""
        if self._h is None:
            self._handle()
        if classes is None:
            mask = 0
        elif isinstance(classes, int):
            mask = classes
        else:
            mask = 0
            for c in ([classes] if isinstance(classes, str) else classes):
                mask |= self.SEG_CLASSES[c]
        prm = SegmentParams(int(neighbourhood), int(min_count), float(cov_rel), float(cov_floor), float(novel_d2), int(mask), int(min_points),
                            int(connectivity), int(min_cluster_points), int(min_cluster_cells))
        T = self._as_poses(pose)[0] if pose is not None else None
        ptr, n, stride, on_dev, keep = self._as_input(points)
        be = DeviceArrays(keep.device, stream) if on_dev else HostArrays
        with be.ctx():
            Td = be.here(T, np.float64)
            counts = be.zeros(4, np.uint32)
            cls = be.empty(n, np.uint8) if labels else None
            lab = be.empty(n, np.int32) if labels else None

        def call(recs):     # (the count-only first call asks for no labels)
            fill = recs is not None
            self._call(be, "segment_scan", C.c_void_p(ptr if n else 0), n, stride, be.ptr(Td), C.byref(prm), be.ptr(cls if fill else None),
                       be.ptr(lab if fill else None), be.ptr(recs), len(recs) if fill else 0, be.ptr(counts))
        if max_clusters is None:
            call(None)
            with be.ctx():                      # (read on the stream the count was enqueued on: the copy waits for it)
                max_clusters = int(counts[0].item())
        with be.ctx():
            recs = be.records(int(max_clusters), _lib.SCAN_CLUSTER)
        call(recs)
        if not be.on_dev:                       # (the host list is cut to the clusters found, the device list is not awaited)
            recs = recs[:min(int(counts[0]), len(recs))]
        out = be.fields(recs, _lib.SCAN_CLUSTER)
        out["counts"] = counts
        if labels:
            out.update(point_class=cls, point_label=lab)
        return out

    def cluster_boxes(self, seg):
        """World-frame boxes and centroids of the clusters of segment_scan(): (boxes [K, 2, 3] float32, the min and the max corner of
        the cluster's cells, and centroids [K, 3] float32, sum / points / 1024).  A cell of signed index s spans origin + lin(s) * len
        to origin + (lin(s) + 1) * len with lin(s) = s - 1 for s > 0, s otherwise, and len the grid's length in x and y, the level's
        height in z.  Entries behind counts[0] (a list with room to spare) are NaN.  Torch in, torch out; numpy in, numpy out."""
        on_dev = not isinstance(seg["label"], np.ndarray)
        xp = np
        if on_dev:
            import torch as xp
        f64 = (lambda v: v.double()) if on_dev else (lambda v: v.astype(np.float64))
        lin = lambda v: f64(v) - f64(v > 0)
        o, steps = self.cloudFirst, (self.gridLen, self.gridLen, self.zLen)
        lo = xp.stack([float(o[a]) + lin(seg[k]) * float(steps[a]) for a, k in enumerate(("sx_min", "sy_min", "sz_min"))], 1)
        hi = xp.stack([float(o[a]) + (lin(seg[k]) + 1.0) * float(steps[a]) for a, k in enumerate(("sx_max", "sy_max", "sz_max"))], 1)
        pts = f64(seg["off_surface"]) + f64(seg["unmapped"])
        pts = pts.clamp(min=1.0) if on_dev else np.maximum(pts, 1.0)
        cen = xp.stack([f64(seg[k]) / pts / 1024.0 for k in ("sum_x", "sum_y", "sum_z")], 1)
        boxes = xp.stack([lo, hi], 1)
        K = int(seg["label"].shape[0])
        found = seg["counts"][0]
        behind = (xp.arange(K, device=seg["label"].device) >= found) if on_dev else (np.arange(K) >= int(found))
        boxes[behind] = float("nan")
        cen[behind] = float("nan")
        return (boxes.float(), cen.float()) if on_dev else (boxes.astype(np.float32), cen.astype(np.float32))

    # ---- scan score derivatives (gndt_score_derivs*) and the Newton registration driven from them (registration.py) ----
    _H_INDEX = None

    @classmethod
    def _h_index(cls):
        """[36] positions in the record's 21 upper-triangle values of the 6 x 6 Hessian's entries, row-major"""
        if cls._H_INDEX is None:
            tri = {}
            for a in range(6):
                for b in range(a, 6):
                    tri[(a, b)] = len(tri)
            cls._H_INDEX = np.array([tri[(min(a, b), max(a, b))] for a in range(6) for b in range(6)], np.int64)
        return cls._H_INDEX

    def score_derivs(self, points, poses, neighbourhood=1, min_count=0, cov_rel=0.0, cov_floor=0.0, max_d2=0.0, stream=None):
        """The score of score_poses with its gradient and Hessian with respect to a left pose perturbation xi = (v, w) (include/gndt.h
        "scan score derivatives"), for each of the K `poses`.  Arguments as score_poses (no per-point outputs).  Returns a dict of
        score, d2_sum (float64 [K], the bits score_poses gives), matched, terms (int64 [K]), g (float64 [K, 6]) and H (float64
        [K, 6, 6], symmetric, filled from the record's 21 values).  A torch CUDA tensor is scored on the device (torch tensors,
        enqueued on `stream`, default torch's current stream, not awaited); a host array through gndt_score_derivs (numpy)."""
        if self._h is None:
            self._handle()
        T = self._as_poses(poses)
        K = T.shape[0]
        ptr, n, stride, on_dev, keep = self._as_input(points)
        prm = ScoreParams(int(neighbourhood), int(min_count), float(cov_rel), float(cov_floor), float(max_d2), 0)
        be = DeviceArrays(keep.device, stream) if on_dev else HostArrays
        with be.ctx():      # (the poses' upload, the outputs and the Hessian's gather belong to the stream the kernels run on)
            Td = be.here(T, np.float64)
            rec = be.records(K, _lib.POSE_DERIVS, zeroed=False)
            self._call(be, "score_derivs", C.c_void_p(ptr if n else 0), n, stride, be.ptr(Td), K, C.byref(prm), be.ptr(rec))
            return self._with_hessian(be, be.fields(rec, _lib.POSE_DERIVS))

    def _with_hessian(self, be, out):
        """gndt_pose_derivs' fields with H, the record's 21 upper-triangle values, gathered into the symmetric [K, 6, 6] (on the
        device the gather is a kernel: call it under be.ctx())"""
        tri = out["H"]
        out["H"] = tri[:, be.here(self._h_index(), np.int64)].reshape(tri.shape[0], 6, 6)
        return out

    def register(self, points, T0, neighbourhood=7, min_count=0, cov_rel=0.0, cov_floor=0.0, max_d2=0.0, step_t=None, step_r=0.05,
                 tol_t=1e-4, tol_r=1e-5, max_iterations=30, stream=None, pyramid=None):
        """The pose near `T0` ([3, 4] / [4, 4], or [K, ...] for K starts run side by side) at which the scan `points` fits the map
        best: registration.register's saddle-free Newton iteration, its derivatives from score_derivs and its line search from
        score_poses.  One iteration is one call of each and two small device-to-host copies.  step_t defaults to half a cell.  Returns
        what registration.register returns (T, reason, iterations, history; a list of those for K starts).  The default neighbourhood
        is 7: the six neighbours smooth the score across the cell faces.
        pyramid: coarser maps of the same stream, coarsest first (what self.pyramid(levels) returns) — the iteration runs on each of
        them in turn, with step_t half of that map's own cell, every level starting from the level before; this map runs last (with
        `step_t`, if given).  A start several cells off, beyond the score's basin on this map, is recovered that way.  The result is
        the last level's with one more entry, levels: every level's result (registration.register_pyramid)."""
        from . import registration
        kw = dict(neighbourhood=neighbourhood, min_count=min_count, cov_rel=cov_rel, cov_floor=cov_floor, max_d2=max_d2, stream=stream)

        def callables(m):
            def evaluate(T):
                return _to_host(stream, m.score_derivs(points, T, **kw), ("score", "d2_sum", "matched", "terms", "g", "H"))

            def score(T):
                return _to_host(stream, m.score_poses(points, T, **kw), ("score",))["score"]

            return evaluate, score

        own_step = 0.5 * self.gridLen if step_t is None else step_t
        if pyramid is None:
            evaluate, score = callables(self)
            return registration.register(evaluate, score, T0, step_t=own_step, step_r=step_r, tol_t=tol_t, tol_r=tol_r,
                                         max_iterations=max_iterations)
        stages = [callables(m) + (0.5 * m.gridLen,) for m in pyramid] + [callables(self) + (own_step,)]
        return registration.register_pyramid(stages, T0, step_r=step_r, tol_t=tol_t, tol_r=tol_r, max_iterations=max_iterations)

    # ---- map pyramids (gndt_coarsen_device: a coarser map of the same point stream, from this map's node table) ----
    def coarsen(self, factor_xy=2, factor_z=None, demand=None, into=None, stream=None):
        """The map a build of this map's point stream at factor_xy times the cell length and factor_z (default: factor_xy) times the
        level height would give — keys, counts, first-seen indices, order and labels exactly, statistics to fp64 rounding — computed on
        the device from this map alone (include/gndt.h "map pyramids"): it works on a map grown by change2DMap, cropped or cleared,
        whose points are gone.  Factors are powers of two, 1 .. 1024.  Returns a new ATOMIC-strategy TwoDmap on the same device with
        the same interval and min_points (demand: this map's unless given), or fills `into`, an existing map at the multiplied
        lengths, whose own map is replaced.  This map must hold its map in the node table (strategy ATOMIC / TILE, or built by
        change2DMap); it is only read.  Enqueued on `stream` (default torch's current stream); the call waits for the device."""
        if self._h is None:
            raise GndtError(1, "coarsen: this map has no finished build")
        fxy = int(factor_xy)
        fz = fxy if factor_z is None else int(factor_z)
        d = self._demand if demand is None else _enum(DEMANDS, demand)
        if into is None:
            # (the handle's lengths are fp32: the multiplied fp32 values, which a power of two keeps exact)
            into = TwoDmap(float(np.float32(self.gridLen) * np.float32(fxy)), float(np.float32(self.zLen) * np.float32(fz)),
                           device=self.device, strategy=1, min_points=self.min_points)
            into.slope_interval = self.slope_interval
        into._ensure(d, need_origin=False)
        rc = self._L.gndt_coarsen_device(self._h, into._h, fxy, fz, _stream_ptr(stream))
        if rc:
            msg = self._L.gndt_last_error(into._h)
            raise GndtError(rc, msg.decode() if msg else "")
        into.cloudFirst = self.cloudFirst      # (the call gave the handle this map's origin)
        return into

    def pyramid(self, levels, factor=2):
        """`levels` coarser maps of this one, each `factor` times the one before in all three lengths: [coarsest, ..., this map x
        factor], the order register(pyramid=...) takes.  This map itself is not in the list."""
        out, m = [], self
        for _ in range(int(levels)):
            m = m.coarsen(factor)
            out.append(m)
        return out[::-1]

    # ---- map merge (gndt_merge_map_device: another map's node table, moved by a pose, added into this map's) ----
    def merge_from(self, other, pose=None, min_count=0, stream=None):
        """Fold the map `other` into this one under `pose` ([3, 4] / [4, 4] [R | t], this map <- other; None = identity): every node of
        `other` with at least min_count points (0 = 1) is moved as a Gaussian with a count and added, moment-matched, to the node of
        this map its mean falls into (include/gndt.h "map merge").  Computed on the device from the two node tables alone: it works on
        maps whose points are gone.  This map needs an origin and may be empty; its lengths, origin, demand and min_points may differ
        from `other`'s, which must hold its map in the node table (strategy ATOMIC / TILE, or built by change2DMap) and is only read.
        Afterwards every row of this map is re-finalised and change2DMap / del2DMap go on.  Enqueued on `stream` (default torch's
        current stream); the call waits for the kernel.  Returns the tallies: source_nodes, merged_nodes, merged_points,
        below_min_count, skipped (the moved mean has no key in this map) and new_nodes."""
        if other._h is None:
            raise GndtError(1, "merge_from: the other map has no finished build")
        if self._h is None:
            self._handle()
        T = None if pose is None else self._as_poses(pose)
        if T is not None and T.shape[0] != 1:
            raise ValueError("merge_from takes one pose")
        prm = MergeParams(int(min_count), 0)
        st = MergeStats()
        rc = self._L.gndt_merge_map_device(self._h, other._h, C.c_void_p(T.ctypes.data if T is not None else 0), C.byref(prm), C.byref(st),
                                           _stream_ptr(stream))
        self._check(rc)
        return {k: int(getattr(st, k)) for k, _ in MergeStats._fields_}

    # ---- map-to-map scoring (gndt_score_maps*: the other map's nodes scored as Gaussians against this map) ----
    def _maps_call(self, other, poses, prm, stream, dtype, per_node):
        """the two entry points' common part: -> (the backend, records of `dtype` on the device, d2, row)"""
        if self._h is None:
            self._handle()
        if other._h is None:
            raise GndtError(1, "score_map: the other map has no finished build")
        T = self._as_poses(poses)
        K = T.shape[0]
        be = DeviceArrays(self._cuda(), stream)
        with be.ctx():      # (the poses' upload and the outputs belong to the stream the kernels run on)
            Td = be.here(T, np.float64)
            rec = be.records(K, dtype, zeroed=False)
            d2 = row = None
            if per_node:
                n = other.sync()[0]
                d2 = be.empty(n, np.float32)
                row = be.empty(n, np.int32)
            if dtype is _lib.POSE_SCORE:
                rc = self._L.gndt_score_maps_device(self._h, other._h, be.ptr(Td), K, C.byref(prm), be.ptr(rec), be.ptr(d2), be.ptr(row),
                                                    _stream_ptr(stream))
            else:
                rc = self._L.gndt_score_maps_derivs_device(self._h, other._h, be.ptr(Td), K, C.byref(prm), be.ptr(rec), _stream_ptr(stream))
            self._check(rc)
        return be, rec, d2, row

    def score_map(self, other, poses, neighbourhood=1, min_count=0, cov_rel=0.0, cov_floor=0.0, max_d2=0.0, per_node=None, stream=None):
        """How well the map `other` fits this map at each of the K `poses` (this map <- other): every node of `other` that has
        statistics is scored as a Gaussian against the nodes of this map its moved mean lands on, the covariance of the difference
        being the sum of the two, `other`'s rotated by the pose (include/gndt.h "map-to-map scoring").  Arguments as score_poses;
        min_count 0 is max(both maps' min_points, 3).  Both maps are only read and may be the same map.  Returns score_poses' dict of
        device tensors; with per_node=k also d2 (float32, per row of `other` the least d2 at pose k: inf where it met no node, NaN
        where the row has no statistics) and row (int32, that node's row in this map, -1).  Enqueued on `stream` (default torch's
        current stream), not awaited."""
        want = per_node is not None
        prm = ScoreParams(int(neighbourhood), int(min_count), float(cov_rel), float(cov_floor), float(max_d2), int(per_node) if want else 0)
        be, rec, d2, row = self._maps_call(other, poses, prm, stream, _lib.POSE_SCORE, want)
        out = be.fields(rec, _lib.POSE_SCORE)
        if want:
            out.update(d2=d2, row=row)
        return out

    def score_map_derivs(self, other, poses, neighbourhood=1, min_count=0, cov_rel=0.0, cov_floor=0.0, max_d2=0.0, stream=None):
        """score_map's score with its gradient and Hessian with respect to a left pose perturbation xi = (v, w), which moves the means
        and rotates the covariances of `other`'s nodes (include/gndt.h "map-to-map scoring").  Returns score_derivs' dict of device
        tensors: score, d2_sum (the bits score_map gives), matched, terms, g [K, 6] and H [K, 6, 6]."""
        prm = ScoreParams(int(neighbourhood), int(min_count), float(cov_rel), float(cov_floor), float(max_d2), 0)
        be, rec, _, _ = self._maps_call(other, poses, prm, stream, _lib.POSE_DERIVS, False)
        with be.ctx():      # (the Hessian's gather runs behind the kernels)
            return self._with_hessian(be, be.fields(rec, _lib.POSE_DERIVS))

    def register_map(self, other, T0, neighbourhood=7, min_count=0, cov_rel=0.0, cov_floor=0.0, max_d2=0.0, step_t=None, step_r=0.05,
                     tol_t=1e-4, tol_r=1e-5, max_iterations=30, stream=None, pyramid=None, other_pyramid=None):
        """The pose near `T0` at which the map `other` fits this map best: register's iteration (registration.register, unchanged)
        with its derivatives from score_map_derivs and its line search from score_map, so every node of `other` takes part with its
        count's worth of shape, not as a bare point.  Arguments and result as register.  pyramid: coarser maps of this one, coarsest
        first, as for register; other_pyramid, if given, `other`'s maps of the same levels — otherwise `other` itself is scored at
        every level."""
        from . import registration
        kw = dict(neighbourhood=neighbourhood, min_count=min_count, cov_rel=cov_rel, cov_floor=cov_floor, max_d2=max_d2, stream=stream)

        def callables(m, o):
            def evaluate(T):
                return _to_host(stream, m.score_map_derivs(o, T, **kw), ("score", "d2_sum", "matched", "terms", "g", "H"))

            def score(T):
                return _to_host(stream, m.score_map(o, T, **kw), ("score",))["score"]

            return evaluate, score

        own_step = 0.5 * self.gridLen if step_t is None else step_t
        if pyramid is None:
            evaluate, score = callables(self, other)
            return registration.register(evaluate, score, T0, step_t=own_step, step_r=step_r, tol_t=tol_t, tol_r=tol_r,
                                         max_iterations=max_iterations)
        others = [other] * len(pyramid) if other_pyramid is None else list(other_pyramid)
        if len(others) != len(pyramid):
            raise ValueError("register_map: other_pyramid must hold one map per level of pyramid")
        stages = [callables(m, o) + (0.5 * m.gridLen,) for m, o in zip(pyramid, others)] + [callables(self, other) + (own_step,)]
        return registration.register_pyramid(stages, T0, step_r=step_r, tol_t=tol_t, tol_r=tol_r, max_iterations=max_iterations)

    def stitch(self, other, T0, method="means", **register_kw):
        """Register the map `other` against this one from the start `T0` ([3, 4] / [4, 4], this map <- other) and fold it in at the
        pose found.  method "means" (the default): the means of `other`'s rows that have statistics are the scan of
        self.register(scan, T0, **register_kw).  method "d2d": self.register_map(other, T0, **register_kw), which scores `other`'s
        nodes as Gaussians.  merge_from(other, pose=result["T"]) follows.  Returns (the registration's result, merge_from's tallies)."""
        if method not in ("means", "d2d"):
            raise ValueError("stitch: method is 'means' or 'd2d'")
        if method == "d2d":
            if np.asarray(T0).ndim != 2:
                raise ValueError("stitch takes one start pose")
            result = self.register_map(other, T0, **register_kw)
            return result, self.merge_from(other, pose=result["T"], stream=register_kw.get("stream"))
        import torch
        cells = other.export_device()
        if cells["num_nodes"] == 0:
            raise GndtError(1, "stitch: the other map is empty")
        scan = cells["mean"][(cells["flags"] & FLAG_HAS_STATS) != 0].contiguous()
        if np.asarray(T0).ndim != 2:
            raise ValueError("stitch takes one start pose")
        result = self.register(scan, T0, **register_kw)
        return result, self.merge_from(other, pose=result["T"], stream=register_kw.get("stream"))

    # ---- results ----
    def sync(self):
        n, k, s = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self._L.gndt_sync(self._h, C.byref(n), C.byref(k), C.byref(s)))
        return n.value, k.value, s.value

    def export(self):
        """Host copy of the SoA result (numpy), nodes in the reference's order."""
        n, k, s = self.sync()
        arrs = {"sx": np.zeros(n, np.int32), "sy": np.zeros(n, np.int32), "sz": np.zeros(n, np.int32),
                "count": np.zeros(n, np.uint32), "first_idx": np.zeros(n, np.uint32),
                "mean": np.zeros((n, 3), np.float32), "cov": np.zeros((n, 6), np.float32),
                "rough": np.zeros(n, np.float32), "normal": np.zeros((n, 3), np.float32), "flags": np.zeros(n, np.uint32)}
        c = Cells()
        for name, a in arrs.items():
            setattr(c, name, a.ctypes.data)
        self._check(self._L.gndt_export(self._h, C.byref(c)))
        arrs.update(num_nodes=int(c.num_nodes), num_columns=int(c.num_columns), num_slopes=int(c.num_slopes))
        return arrs

    def export_device(self):
        """Zero-copy torch views of the device-resident SoA (valid until the next build)."""
        import torch
        c = Cells()
        self._check(self._L.gndt_export_device(self._h, C.byref(c)))
        n = int(c.num_nodes)
        dev = f"cuda:{self.device}"
        out = {"num_nodes": n, "num_columns": int(c.num_columns), "num_slopes": int(c.num_slopes)}
        if n == 0:
            return out
        mk = lambda p, shape, ts: torch.as_tensor(_DevArray(p, shape, ts, self), device=dev)
        for name, shape, ts in (("sx", (n,), "<i4"), ("sy", (n,), "<i4"), ("sz", (n,), "<i4"), ("count", (n,), "<i4"),
                                ("first_idx", (n,), "<i4"), ("mean", (n, 3), "<f4"), ("cov", (n, 6), "<f4"),
                                ("rough", (n,), "<f4"), ("normal", (n, 3), "<f4"), ("flags", (n,), "<i4")):
            out[name] = mk(getattr(c, name), shape, ts)
        return out


def _to_host(stream, out, names):
    """register's and register_map's reads: wait for `stream`, then the named entries of `out` as numpy arrays"""
    _stream_wait(stream)
    return {k: (out[k].cpu().numpy() if hasattr(out[k], "cpu") else np.asarray(out[k])) for k in names}


def count_morton(a, b):
    """countMorton (Stopwatch.h:116-147)."""
    buf = C.create_string_buffer(16)
    rc = _lib.lib().gndt_count_morton(int(a), int(b), buf)
    if rc:
        raise GndtError(rc, "count_morton")
    return buf.value.decode()


def morton_to_xy(m):
    """mortonToXY (Stopwatch.h:171-189)."""
    a, b = C.c_int32(), C.c_int32()
    rc = _lib.lib().gndt_morton_to_xy(int(m), C.byref(a), C.byref(b))
    if rc:
        raise GndtError(rc, "morton_to_xy")
    return a.value, b.value


def trans_morton_xyz(origin, grid_len, z_len, p):
    o = (C.c_float * 3)(*[float(v) for v in origin])
    q = (C.c_float * 3)(*[float(v) for v in p])
    quad = C.create_string_buffer(2)
    key = C.create_string_buffer(16)
    nx, ny, sz = C.c_int32(), C.c_int32(), C.c_int32()
    rc = _lib.lib().gndt_trans_morton_xyz(o, float(grid_len), float(z_len), q, quad, C.byref(nx), C.byref(ny), C.byref(sz), key)
    return rc, key.value.decode(), nx.value, ny.value, sz.value


def crop_box_from_world(origin, grid_len, lo_xy, hi_xy):
    """gndt_crop_box_from_world: (sx_min, sx_max, sy_min, sy_max) of the columns holding a point of [lo_xy, hi_xy] (host, no GPU)."""
    o = (C.c_float * 3)(*[float(v) for v in origin[:3]])
    lo = (C.c_float * 2)(*[float(v) for v in lo_xy[:2]])
    hi = (C.c_float * 2)(*[float(v) for v in hi_xy[:2]])
    b = CropBox()
    rc = _lib.lib().gndt_crop_box_from_world(o, float(grid_len), lo, hi, C.byref(b))
    if rc:
        raise GndtError(rc, "crop_box_from_world: lo > hi, a non-finite value or grid_len <= 0")
    return int(b.sx_min), int(b.sx_max), int(b.sy_min), int(b.sy_max)


def raster_shape(box):
    """gndt_raster_shape: (width, height) of the image of an inclusive box of signed column indices — the non-zero integers of each
    axis (host, no GPU)."""
    b = CropBox(*[int(v) for v in box])
    w, h = C.c_uint32(), C.c_uint32()
    rc = _lib.lib().gndt_raster_shape(C.byref(b), C.byref(w), C.byref(h))
    if rc:
        raise GndtError(rc, "raster_shape: min > max, an index beyond +-65535, an axis without a non-zero index or more than 2^31 pixels")
    return int(w.value), int(h.value)


def _first_nonzero(lo):
    return 1 if lo == 0 else int(lo)


def _column_centre(o, grid_len, s):
    """World coordinate of the centre of column s on an axis (no index 0): o + sign(s) * (|s| - 0.5) * grid_len"""
    return float(o) + (1.0 if s > 0 else -1.0) * (abs(s) - 0.5) * float(grid_len)


def device_info(device=0):
    name = C.create_string_buffer(128)
    cu, mem = C.c_int32(), C.c_uint64()
    rc = _lib.lib().gndt_device_info(int(device), name, C.byref(cu), C.byref(mem))
    if rc:
        raise GndtError(rc, "no device")
    return {"name": name.value.decode(), "compute_units": cu.value, "hbm_bytes": mem.value}


def read_pcd(path):
    """pcl::io::loadPCDFile's part of src/publisher.cpp:19: header + payload of a .pcd file (`DATA ascii` or `binary`).
    Returns (raw, point_step, (off_x, off_y, off_z)): raw = numpy uint8 array of num_points * point_step bytes."""
    L = _lib.lib()
    p = Pcd()
    err = C.create_string_buffer(256)
    rc = L.gndt_pcd_read(str(path).encode(), C.byref(p), err)
    if rc:
        raise GndtError(rc, err.value.decode())
    try:
        nbytes = int(p.num_points) * int(p.layout.point_step)
        raw = np.ctypeslib.as_array((C.c_uint8 * max(nbytes, 1)).from_address(p.data))[:nbytes].copy() if nbytes else np.zeros(0, np.uint8)
    finally:
        L.gndt_pcd_free(C.byref(p))
    return raw, int(p.layout.point_step), (int(p.layout.offset_x), int(p.layout.offset_y), int(p.layout.offset_z))


import contextlib as _contextlib


@_contextlib.contextmanager
def graph_capture(graph, stream=None):
    """`with torch.cuda.graph(graph, stream=stream)` with Python's cycle collector paused for the duration of the capture.
    A collection that starts in the middle of a capture can run the destructor of ANOTHER object — a handle of an earlier test
    (gndt_destroy: hipStreamSynchronize, hipFree), a torch tensor, an abandoned CUDAGraph — and in torch's (global) capture mode any
    such call invalidates the capture; torch then aborts the process inside capture_end (seen once in the GPU tier, in a test that
    had just had a capture refused on purpose).  Reference-counted destruction is not affected: do not drop handles inside the block."""
    import gc
    import torch
    gc.collect()
    was_enabled = gc.isenabled()
    gc.disable()
    try:
        if stream is None:
            with torch.cuda.graph(graph):
                yield
        else:
            with torch.cuda.graph(graph, stream=stream):
                yield
    finally:
        if was_enabled:
            gc.enable()
