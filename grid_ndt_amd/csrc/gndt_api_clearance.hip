// gndt_api_clearance.hip — the clearance field (gndt_clearance.hpp): per slope the steps to the nearest slope with a barrier beside it,
// and that slope's row.  A reader of the map like frontier extraction: runs after the point queries' steps (query_sync) on the map's
// column index (column_index); launches on the caller's stream, nothing awaited — not even between the rounds: a round that finds
// nothing changed by the one before returns at once.  The steps table and the keys live in a scratch area of the handle.
#include "gndt_handle.hpp"
#include "gndt_clearance.hpp"

using namespace gndt;
using namespace gndt_host;

static_assert(sizeof(gndt_clearance_params) == 32, "the ABI of include/gndt.h \"clearance field\"");
static_assert(GNDT_CLEARANCE_BLOCKED == kClrBlocked && GNDT_CLEARANCE_OPEN == kClrOpen && GNDT_CLEARANCE_OVERHEAD == kClrOverhead &&
              GNDT_CLEARANCE_BEYOND == kClrBeyond && GNDT_NO_ROW == kNoRow, "gndt_clearance.hpp's constants are gndt.h's");
static_assert(sizeof(ClearanceStep) == 8, "a side of the steps table is one 8-byte load");

namespace gndt_host {

namespace {

constexpr const char* kClearanceCapture = "gndt_clearance: a clearance call is not recorded into a hipGraph";

// Arguments (every GNDT_ERR_INVALID of include/gndt.h but the handle's state) -> the rule the kernels apply
int clearance_args(gndt_handle* h, const gndt_clearance_params* p, const uint32_t* hops, const uint32_t* nearest, const uint8_t* sides,
                   const uint32_t* counts, ClearanceRule& F) {
    if (!p) { h->err = "gndt_clearance: null params"; return GNDT_ERR_INVALID; }
    if (!counts) { h->err = "gndt_clearance: null counts"; return GNDT_ERR_INVALID; }
    if (!hops && !nearest && !sides) { h->err = "gndt_clearance: hops, nearest and sides are all NULL"; return GNDT_ERR_INVALID; }
    if (p->sources & ~(uint32_t)(GNDT_CLEARANCE_BLOCKED | GNDT_CLEARANCE_OPEN | GNDT_CLEARANCE_OVERHEAD)) {
        h->err = "gndt_clearance: unknown source bits";
        return GNDT_ERR_INVALID;
    }
    if (p->max_hops > kClrMaxHops) { h->err = "gndt_clearance: max_hops > 1024 (it bounds the launches of a call)"; return GNDT_ERR_INVALID; }
    for (uint32_t r : p->reserved)
        if (r != 0u) { h->err = "gndt_clearance: reserved must be 0"; return GNDT_ERR_INVALID; }
    F = ClearanceRule{p->sources ? p->sources : kClrBlocked, p->max_hops ? p->max_hops : 32u};
    return GNDT_OK;
}

// The handle's state (query_sync has run): the stream and the column index, then the passes of gndt_clearance.hpp.  Nothing is awaited.
int clearance_enqueue(gndt_handle* h, const Robot& R, const ClearanceRule& F, uint32_t* hops, uint32_t* nearest, uint8_t* sides,
                      uint32_t* counts, hipStream_t s) {
    int rc = use_stream(h, s);
    if (rc) return rc;
    HIP_TRY(h, hipMemsetAsync(counts, 0, 4 * sizeof(uint32_t), s));
    const uint64_t rows = h->res_nodes;
    if (rows == 0) return GNDT_OK;                     // nothing that indexes rows
    if ((rc = rows_fit_32(h, "gndt_clearance")) || (rc = column_index(h, s))) return rc;
    const uint32_t n = (uint32_t)rows;
    ClearanceScratch S;
    if ((rc = carve_scratch(h, h->clearance, S, n))) return rc;
    const CostView V = query_view(h).V;
    static LdsGrant grant;                             // k_clearance_wg's 144 KB
    const bool wg = tuning().clearance_one_workgroup && n <= kClrLdsRows && lds_granted(h, (const void*)&k_clearance_wg, kClrLdsRows * 16u + kClrLdsTail, grant);
    if (!wg) HIP_TRY(h, hipMemsetAsync(S.flags, 0, ((uint64_t)F.max_hops + 1) * sizeof(uint32_t), s));
    // the row passes: at most 2048 workgroups of 256 threads (what the chip holds at once), grid-stride beyond
    const dim3 grid4(grid_for(4 * (uint64_t)n, 256, 2048)), block(256);
    hipLaunchKernelGGL(k_clearance_steps, grid4, block, 0, s, V, R, F, n, S.step, S.tall, S.key[0], sides, S.flags);
    if (wg) {
        hipLaunchKernelGGL(k_clearance_wg, dim3(1), dim3(kClrWgThreads), (size_t)n * 16 + kClrLdsTail, s, V, R, n, F.max_hops, S.step, S.tall, S.key[0],
                           hops, nearest, counts);
    } else {
        for (uint32_t round = 1; round <= F.max_hops; ++round)
            hipLaunchKernelGGL(k_clearance_round, grid4, block, 0, s, V, R, n, round, S.step, S.tall, S.key[(round - 1) & 1], S.key[round & 1], S.flags);
        hipLaunchKernelGGL(k_clearance_finish, dim3(grid_for(n, 256, kClrFinishBlocks)), block, 0, s, S.key[F.max_hops & 1], n, F.max_hops, hops, nearest, counts);
    }
    HIP_TRY(h, hipGetLastError());
    return GNDT_OK;
}

}  // namespace

}  // namespace gndt_host

extern "C" {

int gndt_clearance_device(gndt_handle* h, const gndt_robot* robot, const gndt_clearance_params* params, uint32_t* hops_dev,
                          uint32_t* nearest_dev, uint8_t* sides_dev, uint32_t* counts_dev, void* hip_stream) {
    int rc = check_ready(h);
    if (rc) return rc;
    ClearanceRule F;
    if ((rc = clearance_args(h, params, hops_dev, nearest_dev, sides_dev, counts_dev, F))) return rc;
    if (misaligned(3u, {hops_dev, nearest_dev, counts_dev})) {
        h->err = "gndt_clearance_device: hops_dev, nearest_dev and counts_dev must be aligned to 4 bytes";
        return GNDT_ERR_INVALID;
    }
    const hipStream_t s = stream_of(h, hip_stream);
    if ((rc = query_sync(h, false, s, kClearanceCapture))) return rc;
    return clearance_enqueue(h, robot_of(robot), F, hops_dev, nearest_dev, sides_dev, counts_dev, s);
}

int gndt_clearance(gndt_handle* h, const gndt_robot* robot, const gndt_clearance_params* params, uint32_t* hops_host, uint32_t* nearest_host,
                   uint8_t* sides_host, uint32_t* counts_host) {
    int rc = check_ready(h);
    if (rc) return rc;
    ClearanceRule F;
    if ((rc = clearance_args(h, params, hops_host, nearest_host, sides_host, counts_host, F))) return rc;
    const hipStream_t s = h->own_stream;
    // the steps that fix the row count first (staging is sized by it)
    if ((rc = query_sync(h, false, s, kClearanceCapture))) return rc;
    const uint64_t rows = h->res_nodes;
    IoPiece io[4] = {io_out(hops_host, rows * 4),
                     io_out(nearest_host, rows * 4),
                     io_out(sides_host, rows),
                     io_out(counts_host, 4 * sizeof(uint32_t))};
    if ((rc = stage_in(h, io, s))) return rc;
    if ((rc = clearance_enqueue(h, robot_of(robot), F, io[0].as<uint32_t>(), io[1].as<uint32_t>(), io[2].as<uint8_t>(), io[3].as<uint32_t>(), s)))
        return rc;
    return stage_out(h, io, s);
}

}  // extern "C"
