// gndt_api_footprint.hip — footprint poses (gndt_footprint.hpp): K poses of a rectangular vehicle, per pose the plane fitted to the
// slopes under it, its tilt along and across the heading, step, bump, headroom and the verdict bits.  A reader of the map like the
// path walks: runs after the point queries' steps (query_sync) on the map's column index (column_index); one kernel on the caller's
// stream, nothing awaited; no cost map and no work memory of the handle's beyond the host call's staging.
#include <math.h>

#include "gndt_handle.hpp"
#include "gndt_footprint.hpp"

using namespace gndt;
using namespace gndt_host;

static_assert(sizeof(gndt_footprint_params) == 48 && sizeof(gndt_footprint_info) == 64 && sizeof(FootInfo) == 64,
              "the ABI of include/gndt.h \"footprint poses\"");
static_assert(GNDT_FOOT_OK == kFootOk && GNDT_FOOT_BAD_POSE == kFootBadPose && GNDT_FOOT_NO_GROUND == kFootNoGround &&
              GNDT_FOOT_SPARSE == kFootSparse && GNDT_FOOT_TILT == kFootTilt && GNDT_FOOT_STEP == kFootStep && GNDT_FOOT_COVER == kFootCover &&
              GNDT_FOOT_LOW == kFootLow && GNDT_FOOT_WEIGHT_CELL == kFootWeightCell && GNDT_FOOT_WEIGHT_COUNT == kFootWeightCount,
              "gndt_footprint.hpp's constants are gndt.h's");
static_assert((2 * kFootMaxN + 1) * (2 * kFootMaxN + 1) <= kFootTable && kFootSlots * kFootLanes == kFootTable, "the box fits a wavefront's table");

namespace gndt_host {

namespace {

// Arguments (every GNDT_ERR_INVALID of include/gndt.h but the handle's state and the device pointers' alignment) -> the rule the kernel applies
int footprint_args(gndt_handle* h, const void* poses, size_t K, size_t stride, const gndt_robot* robot, const gndt_footprint_params* p,
                   const uint32_t* rows, uint32_t row_cap, const gndt_footprint_info* info, FootRule& F) {
    if (!p) { h->err = "gndt_footprint_poses: null params"; return GNDT_ERR_INVALID; }
    if (!info) { h->err = "gndt_footprint_poses: null info"; return GNDT_ERR_INVALID; }
    if (K && !poses) { h->err = "gndt_footprint_poses: null poses"; return GNDT_ERR_INVALID; }
    if ((uint64_t)K * kFootTable >= (1ull << 31)) { h->err = "gndt_footprint_poses: K * 1024 must stay below 2^31"; return GNDT_ERR_INVALID; }
    if (stride < 20 || (stride & 3u)) { h->err = "gndt_footprint_poses: stride_bytes must be a multiple of 4, at least 20"; return GNDT_ERR_INVALID; }
    if (!(isfinite(p->half_length) && p->half_length > 0.f && isfinite(p->half_width) && p->half_width > 0.f)) {
        h->err = "gndt_footprint_poses: half_length and half_width must be finite and greater than 0";
        return GNDT_ERR_INVALID;
    }
    if (!(isfinite(p->max_dz) && p->max_dz >= 0.f && isfinite(p->height) && p->height >= 0.f && isfinite(p->min_cover) && p->min_cover >= 0.f)) {
        h->err = "gndt_footprint_poses: max_dz, height and min_cover must be finite and not negative";
        return GNDT_ERR_INVALID;
    }
    if (p->weight != GNDT_FOOT_WEIGHT_CELL && p->weight != GNDT_FOOT_WEIGHT_COUNT) { h->err = "gndt_footprint_poses: unknown weight"; return GNDT_ERR_INVALID; }
    for (uint32_t r : p->reserved)
        if (r != 0u) { h->err = "gndt_footprint_poses: reserved must be 0"; return GNDT_ERR_INVALID; }
    if ((rows == nullptr) != (row_cap == 0u)) { h->err = "gndt_footprint_poses: rows is NULL exactly when row_cap is 0"; return GNDT_ERR_INVALID; }
    // the box: n = ceil(sqrt(half_length^2 + half_width^2) / grid_len), once, in fp64
    const double len2 = (double)p->half_length * (double)p->half_length, wid2 = (double)p->half_width * (double)p->half_width;
    const double n = ceil(sqrt(len2 + wid2) / (double)h->P.grid_len);
    if (!(n <= (double)kFootMaxN)) {
        h->err = "gndt_footprint_poses: the footprint's box exceeds 31 x 31 columns (it bounds a lane's loop and a wavefront's table)";
        return GNDT_ERR_INVALID;
    }
    const Robot R = robot_of(robot);
    F.len2 = len2; F.wid2 = wid2;
    F.cos_max = cos((double)R.angle * (M_PI / 180.0));
    F.min_cover = (double)p->min_cover;
    F.max_dz = p->max_dz; F.height = p->height; F.reach = R.reach;
    F.min_cells = p->min_cells ? p->min_cells : kFootDefaultCells;
    F.weight = p->weight;
    F.n = n < 1.0 ? 1u : (uint32_t)n;
    return GNDT_OK;
}

// The handle's state (query_sync has run): the stream, the column index, the kernel.  Nothing is awaited.
int footprint_enqueue(gndt_handle* h, const Robot& R, const FootRule& F, const void* poses, uint64_t K, uint64_t stride, uint32_t* rows,
                      uint32_t row_cap, FootInfo* info, hipStream_t s) {
    int rc = use_stream(h, s);
    if (rc) return rc;
    if ((rc = rows_fit_32(h, "gndt_footprint_poses")) || (rc = column_index(h, s))) return rc;
    const ScoreView S{query_view(h), h->out.count, h->out.cov};
    // one pose a wavefront: at most kFootMaxBlocks workgroups of kFootWaves (16 wavefronts on each of the 256 CUs), grid-stride beyond
    const dim3 grid(grid_for(K, kFootWaves, kFootMaxBlocks)), block(kFootThreads);
    hipLaunchKernelGGL(k_footprint_poses, grid, block, 0, s, S, R, F, static_cast<const char*>(poses), K, stride, rows, row_cap, info);
    HIP_TRY(h, hipGetLastError());
    return GNDT_OK;
}

constexpr const char* kFootCapture = "gndt_footprint_poses: a footprint call is not recorded into a hipGraph";

}  // namespace

}  // namespace gndt_host

extern "C" {

int gndt_footprint_poses_device(gndt_handle* h, const void* poses_dev, size_t K, size_t stride_bytes, const gndt_robot* robot,
                                const gndt_footprint_params* params, uint32_t* rows_dev, uint32_t row_cap, gndt_footprint_info* info_dev,
                                void* hip_stream) {
    int rc = check_ready(h);
    if (rc) return rc;
    FootRule F;
    if ((rc = footprint_args(h, poses_dev, K, stride_bytes, robot, params, rows_dev, row_cap, info_dev, F))) return rc;
    if (misaligned(15u, {info_dev}) || misaligned(3u, {rows_dev, poses_dev})) {
        h->err = "gndt_footprint_poses_device: info_dev must be 16-byte aligned (it is written 16 bytes at a time), poses and rows 4-byte";
        return GNDT_ERR_INVALID;
    }
    const hipStream_t s = stream_of(h, hip_stream);
    if ((rc = query_sync(h, false, s, kFootCapture))) return rc;
    if (K == 0) return GNDT_OK;
    return footprint_enqueue(h, robot_of(robot), F, poses_dev, K, stride_bytes, rows_dev, row_cap, reinterpret_cast<FootInfo*>(info_dev), s);
}

int gndt_footprint_poses(gndt_handle* h, const void* poses_host, size_t K, size_t stride_bytes, const gndt_robot* robot,
                         const gndt_footprint_params* params, uint32_t* rows_host, uint32_t row_cap, gndt_footprint_info* info_host) {
    int rc = check_ready(h);
    if (rc) return rc;
    FootRule F;
    if ((rc = footprint_args(h, poses_host, K, stride_bytes, robot, params, rows_host, row_cap, info_host, F))) return rc;
    const hipStream_t s = h->own_stream;
    if ((rc = query_sync(h, false, s, kFootCapture))) return rc;
    if (K == 0) return GNDT_OK;
    // (the last pose's record ends after its five floats: a caller's array need not be padded to the stride)
    IoPiece io[3] = {io_in(poses_host, (uint64_t)(K - 1) * stride_bytes + 20),
                     io_out(rows_host, (uint64_t)K * row_cap * 4),
                     io_out(info_host, (uint64_t)K * sizeof(FootInfo))};
    if ((rc = stage_in(h, io, s))) return rc;
    if ((rc = footprint_enqueue(h, robot_of(robot), F, io[0].dev, K, stride_bytes, io[1].as<uint32_t>(), row_cap, io[2].as<FootInfo>(), s))) return rc;
    return stage_out(h, io, s);
}

}  // extern "C"
