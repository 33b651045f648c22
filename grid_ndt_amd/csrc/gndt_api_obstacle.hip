// gndt_api_obstacle.hip — the obstacle field (gndt_obstacle.hpp): per slope the steps to the nearest slope that a box of the caller's
// list stands on, and that box's index.  A reader of the map like the clearance field: runs after the point queries' steps (query_sync)
// on the map's column index (column_index); launches on the caller's stream, nothing awaited — the number of boxes, the windows' prefix
// sums and the worklist's length stay on the device, grids are sized from the map's rows and the list's capacity, and every kernel
// behind an empty worklist returns at once.  The stamped marks and the per-call scratch live in the handle.
#include "gndt_handle.hpp"
#include "gndt_obstacle.hpp"

using namespace gndt;
using namespace gndt_host;

static_assert(sizeof(gndt_obstacle_params) == 32, "the ABI of include/gndt.h \"obstacle field\"");
static_assert(offsetof(gndt_scan_cluster, sx_min) % 4 == 0 && sizeof(gndt_scan_cluster) % 4 == 0 && sizeof(gndt_scan_cluster) >= 24 &&
              offsetof(gndt_scan_cluster, sz_max) - offsetof(gndt_scan_cluster, sx_min) == 20, "segmentation's records are read where they lie");

namespace gndt_host {

void free_obstacle(gndt_handle* h) {
    if (h->obstacle.marks) (void)hipFree(h->obstacle.marks);
    free_scratch(h->obstacle.scratch);
    h->obstacle = gndt_handle::Obstacle{};
}

namespace {

constexpr const char* kObstacleCapture = "gndt_obstacle_field: an obstacle field call is not recorded into a hipGraph";

// Arguments (every GNDT_ERR_INVALID of include/gndt.h but the handle's state) -> the rule the kernels apply
int obstacle_args(gndt_handle* h, const void* boxes, uint32_t n_boxes, size_t stride, const gndt_obstacle_params* p, const uint32_t* hops,
                  const uint32_t* obstacle, const uint32_t* counts, ObstacleRule& F) {
    if (!p) { h->err = "gndt_obstacle_field: null params"; return GNDT_ERR_INVALID; }
    if (!counts) { h->err = "gndt_obstacle_field: null counts"; return GNDT_ERR_INVALID; }
    if (!boxes && n_boxes > 0) { h->err = "gndt_obstacle_field: null boxes with n_boxes > 0"; return GNDT_ERR_INVALID; }
    if (!hops && !obstacle) { h->err = "gndt_obstacle_field: hops and obstacle are both NULL"; return GNDT_ERR_INVALID; }
    if (stride < 24 || (stride & 3u)) { h->err = "gndt_obstacle_field: box_stride_bytes must be a multiple of 4 and at least 24"; return GNDT_ERR_INVALID; }
    if (reinterpret_cast<uintptr_t>(boxes) & 3u) { h->err = "gndt_obstacle_field: boxes must be aligned to 4 bytes"; return GNDT_ERR_INVALID; }
    if (n_boxes > kObsMaxBoxes) { h->err = "gndt_obstacle_field: n_boxes > 2^20"; return GNDT_ERR_INVALID; }
    if (p->inflate > kObsMaxInflate) { h->err = "gndt_obstacle_field: inflate > 1024"; return GNDT_ERR_INVALID; }
    if (p->max_hops > kClrMaxHops) { h->err = "gndt_obstacle_field: max_hops > 1024 (it bounds the launches of a call)"; return GNDT_ERR_INVALID; }
    if (p->max_columns > kObsMaxColumns) { h->err = "gndt_obstacle_field: max_columns > 2^28 (it bounds the marking pass)"; return GNDT_ERR_INVALID; }
    for (uint32_t r : p->reserved)
        if (r != 0u) { h->err = "gndt_obstacle_field: reserved must be 0"; return GNDT_ERR_INVALID; }
    F = ObstacleRule{p->inflate, p->max_hops ? p->max_hops : 8u, p->levels_above, p->levels_below, p->max_columns ? p->max_columns : kObsDefaultColumns};
    return GNDT_OK;
}

// The stamped marks for a map of n rows and the stamp of this call.  Fresh memory and a stamp about to wrap are set to "never" (stamp 0,
// cover all ones) on the stream; otherwise nothing is cleared.
int obstacle_marks(gndt_handle* h, uint32_t n, hipStream_t s, ObstacleMarks& M, uint32_t& stamp) {
    auto& ob = h->obstacle;
    bool fresh = false;
    if (n > ob.marks_rows) {
        const uint64_t rows = (uint64_t)n + n / 4;          // (a map that grows by updates does not reallocate on every frame)
        if (ob.marks) (void)hipFree(ob.marks);
        ob.marks = nullptr; ob.marks_bytes = 0; ob.marks_rows = 0;
        Carver sizer;
        obstacle_carve_marks(sizer, rows, M);
        HIP_TRY(h, hipMalloc(&ob.marks, sizer.pos));
        ob.marks_bytes = sizer.pos; ob.marks_rows = rows;
        fresh = true;
    }
    Carver c(ob.marks);
    obstacle_carve_marks(c, ob.marks_rows, M);
    if (fresh || ob.stamp >= 0xFFFFFFF0u) {
        HIP_TRY(h, hipMemsetAsync(M.cover, 0xFF, ob.marks_rows * 8, s));
        HIP_TRY(h, hipMemsetAsync(M.cstamp, 0, ob.marks_rows * 4, s));
        ob.stamp = 0u;
    }
    stamp = ++ob.stamp;
    return GNDT_OK;
}

// The handle's state (query_sync has run): the stream and the column index, then the passes of gndt_obstacle.hpp.  Nothing is awaited.
// Everything that can fail comes before the first launch: a refused call writes nothing.
int obstacle_enqueue(gndt_handle* h, const Robot& R, const ObstacleRule& F, const void* boxes, uint32_t n_boxes, size_t stride,
                     const uint32_t* n_boxes_dev, const uint32_t* base, uint32_t* hops, uint32_t* obstacle, uint32_t* counts, hipStream_t s) {
    int rc = use_stream(h, s);
    if (rc || (rc = rows_fit_32(h, "gndt_obstacle_field"))) return rc;
    const uint32_t n = (uint32_t)h->res_nodes;
    if (n && (rc = column_index(h, s))) return rc;
    ObstacleScratch S;
    if ((rc = carve_scratch(h, h->obstacle.scratch, S, n, n_boxes))) return rc;
    ObstacleMarks M{};
    M.covers = S.covers;
    M.list = S.list;
    M.len = &S.hdr->len;
    const dim3 block(256);
    uint32_t stamp = 0u;
    if (n != 0u && (rc = obstacle_marks(h, n, s, M, stamp))) return rc;
    hipLaunchKernelGGL(k_obstacle_windows, dim3(1), dim3(kObsWinThreads), 0, s, boxes, n_boxes, stride, n_boxes_dev, F, n != 0u, S.W, M.covers, S.hdr, counts,
                       S.flags, n ? F.max_hops + 1u : 0u);
    if (n != 0u) {
        const CostView V = query_view(h).V;
        // The grids are sized from the map's rows and the list's capacity, the only sizes the host has: one zone of 500 x 500 columns
        // is one box.  The loops are grid-stride over the device's own counts, and a workgroup behind them returns at once.
        const uint64_t side = 2ull * (F.inflate + F.max_hops) + 1;
        const uint64_t most = std::min<uint64_t>(F.max_columns, std::max<uint64_t>(n, (uint64_t)n_boxes * side * side));
        const dim3 grid_mark(grid_for(std::max<uint64_t>(most, n), 256, 2048)), grid4(grid_for(4 * (uint64_t)n, 256, 2048));
        hipLaunchKernelGGL(k_obstacle_mark, grid_mark, block, 0, s, V, F, boxes, stride, S.W, S.hdr, stamp, M, n, base, hops, obstacle,
                           tuning().obstacle_tally);
        hipLaunchKernelGGL(k_obstacle_steps, grid4, block, 0, s, V, R, S.hdr, stamp, M, S.step, S.tall, S.key[0], S.flags);
        for (uint32_t round = 1; round <= F.max_hops; ++round)
            hipLaunchKernelGGL(k_obstacle_round, grid4, block, 0, s, V, R, S.hdr, round, M.list, S.step, S.tall, S.key[(round - 1) & 1], S.key[round & 1], S.flags);
        hipLaunchKernelGGL(k_obstacle_finish, dim3(grid_for(n, 256, kClrFinishBlocks)), block, 0, s, V, S.hdr, M.list,
                           S.key[F.max_hops & 1], F.max_hops, base, hops, obstacle, M.covers, counts);
    }
    HIP_TRY(h, hipGetLastError());
    return GNDT_OK;
}

}  // namespace

}  // namespace gndt_host

extern "C" {

int gndt_obstacle_field_device(gndt_handle* h, const gndt_robot* robot, const void* boxes_dev, uint32_t n_boxes, size_t box_stride_bytes,
                               const uint32_t* n_boxes_dev, const gndt_obstacle_params* params, const uint32_t* base_hops_dev,
                               uint32_t* hops_dev, uint32_t* obstacle_dev, uint32_t* counts_dev, void* hip_stream) {
    int rc = check_ready(h);
    if (rc) return rc;
    ObstacleRule F;
    if ((rc = obstacle_args(h, boxes_dev, n_boxes, box_stride_bytes, params, hops_dev, obstacle_dev, counts_dev, F))) return rc;
    if (misaligned(3u, {hops_dev, obstacle_dev, counts_dev, base_hops_dev, n_boxes_dev})) {
        h->err = "gndt_obstacle_field_device: n_boxes_dev, base_hops_dev, hops_dev, obstacle_dev and counts_dev must be aligned to 4 bytes";
        return GNDT_ERR_INVALID;
    }
    const hipStream_t s = stream_of(h, hip_stream);
    if ((rc = query_sync(h, false, s, kObstacleCapture))) return rc;
    return obstacle_enqueue(h, robot_of(robot), F, boxes_dev, n_boxes, box_stride_bytes, n_boxes_dev, hops_dev ? base_hops_dev : nullptr, hops_dev,
                            obstacle_dev, counts_dev, s);
}

int gndt_obstacle_field(gndt_handle* h, const gndt_robot* robot, const void* boxes_host, uint32_t n_boxes, size_t box_stride_bytes,
                        const gndt_obstacle_params* params, const uint32_t* base_hops_host, uint32_t* hops_host, uint32_t* obstacle_host,
                        uint32_t* counts_host) {
    int rc = check_ready(h);
    if (rc) return rc;
    ObstacleRule F;
    if ((rc = obstacle_args(h, boxes_host, n_boxes, box_stride_bytes, params, hops_host, obstacle_host, counts_host, F))) return rc;
    const hipStream_t s = h->own_stream;
    // the steps that fix the row count first (staging is sized by it)
    if ((rc = query_sync(h, false, s, kObstacleCapture))) return rc;
    const uint64_t rows = h->res_nodes;
    IoPiece io[4] = {io_in(boxes_host, (uint64_t)n_boxes * box_stride_bytes),
                     {base_hops_host, hops_host, hops_host ? rows * 4 : 0},      // the base travels in the hops' piece and is merged in place
                     io_out(obstacle_host, rows * 4),
                     io_out(counts_host, 8 * sizeof(uint32_t))};
    if ((rc = stage_in(h, io, s))) return rc;
    const bool merge = base_hops_host && io[1].bytes;
    if ((rc = obstacle_enqueue(h, robot_of(robot), F, io[0].dev, n_boxes, box_stride_bytes, nullptr, merge ? io[1].as<uint32_t>() : nullptr,
                               io[1].as<uint32_t>(), io[2].as<uint32_t>(), io[3].as<uint32_t>(), s)))
        return rc;
    return stage_out(h, io, s);
}

int gndt_debug_obstacle_marks(gndt_handle* h, uint64_t out[5]) {
    if (!h || !out) return GNDT_ERR_INVALID;
    for (int k = 0; k < 5; ++k) out[k] = 0;
    if (!h->obstacle.scratch.p || !h->obstacle.stamp) return GNDT_OK;
    ObstacleHeader hdr;
    HIP_TRY(h, hipStreamSynchronize(h->last_stream));
    HIP_TRY(h, hipMemcpy(&hdr, h->obstacle.scratch.p, sizeof hdr, hipMemcpyDeviceToHost));
    out[0] = hdr.items; out[1] = hdr.len; out[2] = hdr.probes; out[3] = hdr.claims; out[4] = hdr.cover_atomics;
    return GNDT_OK;
}

}  // extern "C"
