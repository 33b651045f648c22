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
    if (h->obstacle.scratch) (void)hipFree(h->obstacle.scratch);
    h->obstacle = gndt_handle::Obstacle{};
}

namespace {

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
        HIP_TRY(h, hipMalloc(&ob.marks, rows * 16));
        ob.marks_bytes = rows * 16; ob.marks_rows = rows;
        fresh = true;
    }
    M.cover = static_cast<unsigned long long*>(ob.marks);
    M.cstamp = reinterpret_cast<uint32_t*>(M.cover + ob.marks_rows);
    M.slot = M.cstamp + ob.marks_rows;
    if (fresh || ob.stamp >= 0xFFFFFFF0u) {
        HIP_TRY(h, hipMemsetAsync(M.cover, 0xFF, ob.marks_rows * 8, s));
        HIP_TRY(h, hipMemsetAsync(M.cstamp, 0, ob.marks_rows * 4, s));
        ob.stamp = 0u;
    }
    stamp = ++ob.stamp;
    return GNDT_OK;
}

// Arguments checked: the queries' steps (capture, finished map, gndt_sync), the stream and the column index, then the passes of
// gndt_obstacle.hpp.  Nothing is awaited.  Everything that can fail comes before the first launch: a refused call writes nothing.
int obstacle_enqueue(gndt_handle* h, const Robot& R, const ObstacleRule& F, const void* boxes, uint32_t n_boxes, size_t stride,
                     const uint32_t* n_boxes_dev, const uint32_t* base, uint32_t* hops, uint32_t* obstacle, uint32_t* counts, hipStream_t s) {
    int rc = query_sync(h, false, s, "gndt_obstacle_field: an obstacle field call is not recorded into a hipGraph");
    if (rc) return rc;
    if ((rc = use_stream(h, s))) return rc;
    const uint64_t rows = h->res_nodes;
    if (rows >= 0xFFFFFFFFull) { h->err = "gndt_obstacle_field: row numbers do not fit 32 bits"; return GNDT_ERR_CAPACITY; }
    const uint32_t n = (uint32_t)rows;
    if (n && (rc = column_index(h, s))) return rc;
    // header | W [n_boxes] (8 B) | keys [2][n] (8 B) | steps [4 n] (8 B) | the rounds' flags | covers [n_boxes] | list [n] | tall [n] (bytes)
    constexpr uint64_t kFlagWords = kClrMaxHops + 8u, kHeader = 64;
    static_assert(sizeof(ObstacleHeader) <= kHeader, "the header's room");
    auto& ob = h->obstacle;
    if ((rc = grow_scratch(h, ob.scratch, ob.bytes, kHeader + (uint64_t)n_boxes * 12 + (uint64_t)n * 53 + kFlagWords * 4))) return rc;
    ObstacleHeader* hdr = static_cast<ObstacleHeader*>(ob.scratch);
    unsigned long long* W = reinterpret_cast<unsigned long long*>(static_cast<char*>(ob.scratch) + kHeader);
    unsigned long long* key[2] = {W + n_boxes, W + n_boxes + n};
    ClearanceStep* step = reinterpret_cast<ClearanceStep*>(key[1] + n);
    uint32_t* flags = reinterpret_cast<uint32_t*>(step + 4 * (uint64_t)n);
    ObstacleMarks M{};
    M.covers = flags + kFlagWords;
    M.list = M.covers + n_boxes;
    M.len = &hdr->len;
    uint8_t* tall = reinterpret_cast<uint8_t*>(M.list + n);
    const dim3 block(256);
    uint32_t stamp = 0u;
    if (n != 0u && (rc = obstacle_marks(h, n, s, M, stamp))) return rc;
    hipLaunchKernelGGL(k_obstacle_windows, dim3(1), dim3(kObsWinThreads), 0, s, boxes, n_boxes, stride, n_boxes_dev, F, n != 0u, W, M.covers, hdr, counts,
                       flags, n ? F.max_hops + 1u : 0u);
    if (n != 0u) {
        const CostView V = query_view(h).V;
        // The grids are sized from the map's rows and the list's capacity, the only sizes the host has: one zone of 500 x 500 columns
        // is one box.  The loops are grid-stride over the device's own counts, and a workgroup behind them returns at once.
        const uint64_t side = 2ull * (F.inflate + F.max_hops) + 1;
        const uint64_t most = std::min<uint64_t>(F.max_columns, std::max<uint64_t>(n, (uint64_t)n_boxes * side * side));
        const dim3 grid_mark(grid_for(std::max<uint64_t>(most, n), 256, 2048)), grid4(grid_for(4 * (uint64_t)n, 256, 2048));
        hipLaunchKernelGGL(k_obstacle_mark, grid_mark, block, 0, s, V, F, boxes, stride, W, hdr, stamp, M, n, base, hops, obstacle,
                           tuning().obstacle_tally);
        hipLaunchKernelGGL(k_obstacle_steps, grid4, block, 0, s, V, R, hdr, stamp, M, step, tall, key[0], flags);
        for (uint32_t round = 1; round <= F.max_hops; ++round)
            hipLaunchKernelGGL(k_obstacle_round, grid4, block, 0, s, V, R, hdr, round, M.list, step, tall, key[(round - 1) & 1], key[round & 1], flags);
        hipLaunchKernelGGL(k_obstacle_finish, dim3(grid_for(n, 256, kClrFinishBlocks)), block, 0, s, V, hdr, M.list,
                           key[F.max_hops & 1], F.max_hops, base, hops, obstacle, M.covers, counts);
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
    if ((reinterpret_cast<uintptr_t>(hops_dev) & 3u) || (reinterpret_cast<uintptr_t>(obstacle_dev) & 3u) || (reinterpret_cast<uintptr_t>(counts_dev) & 3u) ||
        (reinterpret_cast<uintptr_t>(base_hops_dev) & 3u) || (reinterpret_cast<uintptr_t>(n_boxes_dev) & 3u)) {
        h->err = "gndt_obstacle_field_device: n_boxes_dev, base_hops_dev, hops_dev, obstacle_dev and counts_dev must be aligned to 4 bytes";
        return GNDT_ERR_INVALID;
    }
    return obstacle_enqueue(h, robot_of(robot), F, boxes_dev, n_boxes, box_stride_bytes, n_boxes_dev, hops_dev ? base_hops_dev : nullptr, hops_dev,
                            obstacle_dev, counts_dev, stream_of(h, hip_stream));
}

int gndt_obstacle_field(gndt_handle* h, const gndt_robot* robot, const void* boxes_host, uint32_t n_boxes, size_t box_stride_bytes,
                        const gndt_obstacle_params* params, const uint32_t* base_hops_host, uint32_t* hops_host, uint32_t* obstacle_host,
                        uint32_t* counts_host) {
    int rc = check_ready(h);
    if (rc) return rc;
    ObstacleRule F;
    if ((rc = obstacle_args(h, boxes_host, n_boxes, box_stride_bytes, params, hops_host, obstacle_host, counts_host, F))) return rc;
    const hipStream_t s = h->own_stream;
    // the steps that fix the row count first (staging is sized by it): what obstacle_enqueue does again, then as no-ops
    if ((rc = query_sync(h, false, s, "gndt_obstacle_field: an obstacle field call is not recorded into a hipGraph"))) return rc;
    const uint64_t rows = h->res_nodes;
    // the base travels into the hops' piece and is merged in place
    const uint64_t bytes[4] = {(uint64_t)n_boxes * box_stride_bytes, hops_host ? rows * 4 : 0, obstacle_host ? rows * 4 : 0, 8 * sizeof(uint32_t)};
    void* dev[4];
    if ((rc = stage_pieces(h, bytes, dev, 4))) return rc;
    if (bytes[0]) HIP_TRY(h, hipMemcpyAsync(dev[0], boxes_host, bytes[0], hipMemcpyHostToDevice, s));
    const bool merge = base_hops_host && bytes[1];
    if (merge) HIP_TRY(h, hipMemcpyAsync(dev[1], base_hops_host, bytes[1], hipMemcpyHostToDevice, s));
    if ((rc = obstacle_enqueue(h, robot_of(robot), F, dev[0], n_boxes, box_stride_bytes, nullptr, merge ? static_cast<uint32_t*>(dev[1]) : nullptr,
                               static_cast<uint32_t*>(dev[1]), static_cast<uint32_t*>(dev[2]), static_cast<uint32_t*>(dev[3]), s)))
        return rc;
    void* host[4] = {nullptr, hops_host, obstacle_host, counts_host};
    for (int k = 1; k < 4; ++k)
        if (bytes[k]) HIP_TRY(h, hipMemcpyAsync(host[k], dev[k], bytes[k], hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    return GNDT_OK;
}

int gndt_debug_obstacle_marks(gndt_handle* h, uint64_t out[5]) {
    if (!h || !out) return GNDT_ERR_INVALID;
    for (int k = 0; k < 5; ++k) out[k] = 0;
    if (!h->obstacle.scratch || !h->obstacle.stamp) return GNDT_OK;
    ObstacleHeader hdr;
    HIP_TRY(h, hipStreamSynchronize(h->last_stream));
    HIP_TRY(h, hipMemcpy(&hdr, h->obstacle.scratch, sizeof hdr, hipMemcpyDeviceToHost));
    out[0] = hdr.items; out[1] = hdr.len; out[2] = hdr.probes; out[3] = hdr.claims; out[4] = hdr.cover_atomics;
    return GNDT_OK;
}

}  // extern "C"
