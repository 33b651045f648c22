// gndt_api_walk.hip — path walks (gndt_walk.hpp): K candidate polylines driven over the map's slopes under the flood's gates.  A reader
// of the map like the clearance field: runs after the point queries' steps (query_sync) on the map's column index (column_index);
// launches on the caller's stream, nothing awaited; no cost map needed.  The table variant's steps table lives in a scratch area of
// the handle and is made again by every call that takes it (k_clearance_steps for the call's robot: nothing can go stale).
#include "gndt_handle.hpp"
#include "gndt_walk.hpp"

using namespace gndt;
using namespace gndt_host;

static_assert(sizeof(gndt_walk_params) == 32 && sizeof(gndt_walk_info) == 48 && sizeof(WalkInfo) == 48, "the ABI of include/gndt.h \"path walks\"");
static_assert(GNDT_WALK_DONE == kWalkDone && GNDT_WALK_NO_START == kWalkNoStart && GNDT_WALK_BLOCKED == kWalkBlocked &&
              GNDT_WALK_LEFT_MAP == kWalkLeftMap && GNDT_WALK_OVERHEAD == kWalkOverhead && GNDT_WALK_TOO_CLOSE == kWalkTooClose &&
              GNDT_WALK_LIMIT == kWalkLimit && GNDT_WALK_CHECK_OVERHEAD == kWalkCheckOverhead && GNDT_WALK_NO_SIDE == kWalkNoSide,
              "gndt_walk.hpp's constants are gndt.h's");

namespace gndt_host {

namespace {

// Arguments (every GNDT_ERR_INVALID of include/gndt.h but the handle's state) -> the rule the kernel applies
int walk_args(gndt_handle* h, const void* paths, size_t K, size_t T, size_t stride_bytes, const gndt_walk_params* p, const uint32_t* rows,
              uint32_t row_cap, const gndt_walk_info* info, WalkRule& F) {
    if (!p) { h->err = "gndt_walk_paths: null params"; return GNDT_ERR_INVALID; }
    if (!info) { h->err = "gndt_walk_paths: null info"; return GNDT_ERR_INVALID; }
    if (K && T && !paths) { h->err = "gndt_walk_paths: null paths"; return GNDT_ERR_INVALID; }
    if (K >= (1ull << 31) || T >= (1ull << 31) || (uint64_t)K * T >= (1ull << 31)) {
        h->err = "gndt_walk_paths: 2^31 or more waypoints in one call";
        return GNDT_ERR_INVALID;
    }
    if (stride_bytes != 12 && stride_bytes != 16) { h->err = "gndt_walk_paths: stride_bytes must be 12 or 16"; return GNDT_ERR_INVALID; }
    if (p->start_mode != 0 && p->start_mode != GNDT_WALK_START_NEAREST_SLOPE && p->start_mode != GNDT_WALK_START_NODE) {
        h->err = "gndt_walk_paths: unknown start_mode";
        return GNDT_ERR_INVALID;
    }
    if (p->checks & ~(uint32_t)GNDT_WALK_CHECK_OVERHEAD) { h->err = "gndt_walk_paths: unknown check bits"; return GNDT_ERR_INVALID; }
    if (p->max_steps > kWalkMaxSteps) { h->err = "gndt_walk_paths: max_steps > 2^20 (it bounds a lane's loop)"; return GNDT_ERR_INVALID; }
    for (uint32_t r : p->reserved)
        if (r != 0u) { h->err = "gndt_walk_paths: reserved must be 0"; return GNDT_ERR_INVALID; }
    if ((rows == nullptr) != (row_cap == 0u)) { h->err = "gndt_walk_paths: rows is NULL exactly when row_cap is 0"; return GNDT_ERR_INVALID; }
    F = WalkRule{p->start_mode == GNDT_WALK_START_NODE ? kQueryNode : kQueryNearestSlope, p->checks, p->min_hops,
                 p->max_steps ? p->max_steps : kWalkDefaultSteps};
    return GNDT_OK;
}

// The handle's state (query_sync has run): the stream, the column index, the steps table when the call takes that variant, the kernel.
// Nothing is awaited.
int walk_enqueue(gndt_handle* h, const Robot& R, const WalkRule& F, const float* paths, uint32_t sf, uint64_t K, uint32_t T, const uint32_t* hops,
                 uint32_t* rows, uint32_t row_cap, WalkInfo* info, hipStream_t s) {
    int rc = use_stream(h, s);
    if (rc) return rc;
    const uint64_t n = h->res_nodes;
    if ((rc = rows_fit_32(h, "gndt_walk_paths")) || (rc = column_index(h, s))) return rc;
    const QueryView Q = query_view(h);
    // one wavefront a workgroup; at most 8192 of them (32 on each of the 256 CUs: what the chip holds at once), grid-stride beyond
    const dim3 grid(grid_for(K, kWalkThreads, 8192)), block(kWalkThreads);
    // Which variant: the table costs a pass over the map's rows and saves the gates on every step of a lane's chain;
    // a call takes as long as its longest chains, whose steps grow with T and not with K
    const int mode = tuning().walk_step_table;
    const bool table = n != 0 && (mode == 1 || (mode == 2 && n <= (uint64_t)kWalkTableRowsPerWaypoint * T));
    if (table) {
        WalkScratch S;
        if ((rc = carve_scratch(h, h->walk, S, n))) return rc;
        hipLaunchKernelGGL(k_clearance_steps, dim3(grid_for(4 * n, 256, 2048)), dim3(256), 0, s, Q.V, R, ClearanceRule{kClrBlocked, 1u}, (uint32_t)n,
                           S.step, S.tall, S.key0, static_cast<uint8_t*>(nullptr), S.flag);
        hipLaunchKernelGGL(k_walk_paths<true>, grid, block, 0, s, Q, R, F, WalkTable{S.step, S.tall}, hops, paths, sf, K, T, rows, row_cap, info);
    } else {
        hipLaunchKernelGGL(k_walk_paths<false>, grid, block, 0, s, Q, R, F, WalkTable{nullptr, nullptr}, hops, paths, sf, K, T, rows, row_cap, info);
    }
    HIP_TRY(h, hipGetLastError());
    return GNDT_OK;
}

constexpr const char* kWalkCapture = "gndt_walk_paths: a walk call is not recorded into a hipGraph";

}  // namespace

}  // namespace gndt_host

extern "C" {

int gndt_walk_paths_device(gndt_handle* h, const void* paths_dev, size_t K, size_t T, size_t stride_bytes, const gndt_robot* robot,
                           const gndt_walk_params* params, const uint32_t* hops_dev, uint32_t* rows_dev, uint32_t row_cap,
                           gndt_walk_info* info_dev, void* hip_stream) {
    int rc = check_ready(h);
    if (rc) return rc;
    WalkRule F;
    if ((rc = walk_args(h, paths_dev, K, T, stride_bytes, params, rows_dev, row_cap, info_dev, F))) return rc;
    if (misaligned(15u, {info_dev}) || misaligned(3u, {rows_dev, paths_dev, hops_dev})) {
        h->err = "gndt_walk_paths_device: info_dev must be 16-byte aligned (it is written 16 bytes at a time), paths, hops and rows 4-byte";
        return GNDT_ERR_INVALID;
    }
    const hipStream_t s = stream_of(h, hip_stream);
    if ((rc = query_sync(h, false, s, kWalkCapture))) return rc;
    if (K == 0 || T == 0) return GNDT_OK;
    return walk_enqueue(h, robot_of(robot), F, static_cast<const float*>(paths_dev), (uint32_t)(stride_bytes / 4), K, (uint32_t)T, hops_dev, rows_dev,
                        row_cap, reinterpret_cast<WalkInfo*>(info_dev), s);
}

int gndt_walk_paths(gndt_handle* h, const void* paths_host, size_t K, size_t T, size_t stride_bytes, const gndt_robot* robot,
                    const gndt_walk_params* params, const uint32_t* hops_host, uint32_t* rows_host, uint32_t row_cap, gndt_walk_info* info_host) {
    int rc = check_ready(h);
    if (rc) return rc;
    WalkRule F;
    if ((rc = walk_args(h, paths_host, K, T, stride_bytes, params, rows_host, row_cap, info_host, F))) return rc;
    const hipStream_t s = h->own_stream;
    if ((rc = query_sync(h, false, s, kWalkCapture))) return rc;
    if (K == 0 || T == 0) return GNDT_OK;
    IoPiece io[4] = {io_in(paths_host, (uint64_t)K * T * stride_bytes),
                     io_in(hops_host, h->res_nodes * 4),
                     io_out(rows_host, (uint64_t)K * row_cap * 4),
                     io_out(info_host, (uint64_t)K * sizeof(WalkInfo))};
    if ((rc = stage_in(h, io, s))) return rc;
    // (a map without rows: hops has no entry and no slope is stood on)
    if ((rc = walk_enqueue(h, robot_of(robot), F, io[0].as<const float>(), (uint32_t)(stride_bytes / 4), K, (uint32_t)T, io[1].as<const uint32_t>(),
                           io[2].as<uint32_t>(), row_cap, io[3].as<WalkInfo>(), s)))
        return rc;
    return stage_out(h, io, s);
}

}  // extern "C"
