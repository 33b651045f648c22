// gndt_api_clearance.hip — the clearance field (gndt_clearance.hpp): per slope the steps to the nearest slope with a barrier beside it,
// and that slope's row.  A reader of the map like frontier extraction: runs after the point queries' steps (query_sync) on the map's
// column index (column_index); launches on the caller's stream, nothing awaited — not even between the rounds: a round that finds
// nothing changed by the one before returns at once.  The steps table and the keys live in a scratch area of the handle.
#include <atomic>

#include "gndt_handle.hpp"
#include "gndt_clearance.hpp"

using namespace gndt;
using namespace gndt_host;

static_assert(sizeof(gndt_clearance_params) == 32, "the ABI of include/gndt.h \"clearance field\"");
static_assert(GNDT_CLEARANCE_BLOCKED == kClrBlocked && GNDT_CLEARANCE_OPEN == kClrOpen && GNDT_CLEARANCE_OVERHEAD == kClrOverhead &&
              GNDT_CLEARANCE_BEYOND == kClrBeyond && GNDT_NO_ROW == kNoRow, "gndt_clearance.hpp's constants are gndt.h's");
static_assert(sizeof(ClearanceStep) == 8, "a side of the steps table is one 8-byte load");

namespace gndt_host {

void free_clearance(gndt_handle* h) {
    if (h->clearance.scratch) (void)hipFree(h->clearance.scratch);
    h->clearance = gndt_handle::Clearance{};
}

namespace {

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

// 144 KB of dynamic LDS have to be asked for once per device (the attribute belongs to the function ON the current device, which
// check_ready has made the handle's): gndt_api_cost.hip's rule for k_cost_flood_wg<true>
bool clearance_lds_granted(const gndt_handle* h) {
    static std::atomic<int> state[64];                 // per device: 0 not asked yet, 1 granted, 2 refused
    if (h->device < 0 || h->device >= 64) return false;
    int st = state[h->device].load(std::memory_order_acquire);
    if (st == 0) {
        st = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_clearance_wg), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)(kClrLdsRows * 16u + kClrLdsTail)) == hipSuccess ? 1 : 2;
        if (st == 2) (void)hipGetLastError();
        state[h->device].store(st, std::memory_order_release);
    }
    return st == 1;
}

// Arguments checked: the queries' steps (capture, finished map, gndt_sync), the stream and the column index, then the passes of
// gndt_clearance.hpp.  Nothing is awaited.
int clearance_enqueue(gndt_handle* h, const Robot& R, const ClearanceRule& F, uint32_t* hops, uint32_t* nearest, uint8_t* sides,
                      uint32_t* counts, hipStream_t s) {
    int rc = query_sync(h, false, s, "gndt_clearance: a clearance call is not recorded into a hipGraph");
    if (rc) return rc;
    if ((rc = use_stream(h, s))) return rc;
    HIP_TRY(h, hipMemsetAsync(counts, 0, 4 * sizeof(uint32_t), s));
    const uint64_t rows = h->res_nodes;
    if (rows == 0) return GNDT_OK;                     // nothing that indexes rows
    if (rows >= 0xFFFFFFFFull) { h->err = "gndt_clearance: row numbers do not fit 32 bits"; return GNDT_ERR_CAPACITY; }
    if ((rc = column_index(h, s))) return rc;
    const uint32_t n = (uint32_t)rows;
    // steps [4 n] (8 B) | keys [2][n] (8 B) | the rounds' flags [kClrMaxHops + 1, padded] | tall columns [n] (bytes): 49 B a row
    constexpr uint64_t kFlagWords = kClrMaxHops + 8u;
    auto& cl = h->clearance;
    if ((rc = grow_scratch(h, cl.scratch, cl.bytes, (uint64_t)n * 49 + kFlagWords * 4))) return rc;
    ClearanceStep* step = static_cast<ClearanceStep*>(cl.scratch);
    unsigned long long* key[2] = {reinterpret_cast<unsigned long long*>(step + 4 * (uint64_t)n), nullptr};
    key[1] = key[0] + n;
    uint32_t* flags = reinterpret_cast<uint32_t*>(key[1] + n);
    uint8_t* tall = reinterpret_cast<uint8_t*>(flags + kFlagWords);
    const CostView V = query_view(h).V;
    const bool wg = tuning().clearance_one_workgroup && n <= kClrLdsRows && clearance_lds_granted(h);
    if (!wg) HIP_TRY(h, hipMemsetAsync(flags, 0, ((uint64_t)F.max_hops + 1) * sizeof(uint32_t), s));
    // the row passes: at most 2048 workgroups of 256 threads (what the chip holds at once), grid-stride beyond
    const dim3 grid4(grid_for(4 * (uint64_t)n, 256, 2048)), block(256);
    hipLaunchKernelGGL(k_clearance_steps, grid4, block, 0, s, V, R, F, n, step, tall, key[0], sides, flags);
    if (wg) {
        hipLaunchKernelGGL(k_clearance_wg, dim3(1), dim3(kClrWgThreads), (size_t)n * 16 + kClrLdsTail, s, V, R, n, F.max_hops, step, tall, key[0],
                           hops, nearest, counts);
    } else {
        for (uint32_t round = 1; round <= F.max_hops; ++round)
            hipLaunchKernelGGL(k_clearance_round, grid4, block, 0, s, V, R, n, round, step, tall, key[(round - 1) & 1], key[round & 1], flags);
        hipLaunchKernelGGL(k_clearance_finish, dim3(grid_for(n, 256, kClrFinishBlocks)), block, 0, s, key[F.max_hops & 1], n, F.max_hops, hops, nearest, counts);
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
    if ((reinterpret_cast<uintptr_t>(hops_dev) & 3u) || (reinterpret_cast<uintptr_t>(nearest_dev) & 3u) || (reinterpret_cast<uintptr_t>(counts_dev) & 3u)) {
        h->err = "gndt_clearance_device: hops_dev, nearest_dev and counts_dev must be aligned to 4 bytes";
        return GNDT_ERR_INVALID;
    }
    return clearance_enqueue(h, robot_of(robot), F, hops_dev, nearest_dev, sides_dev, counts_dev, stream_of(h, hip_stream));
}

int gndt_clearance(gndt_handle* h, const gndt_robot* robot, const gndt_clearance_params* params, uint32_t* hops_host, uint32_t* nearest_host,
                   uint8_t* sides_host, uint32_t* counts_host) {
    int rc = check_ready(h);
    if (rc) return rc;
    ClearanceRule F;
    if ((rc = clearance_args(h, params, hops_host, nearest_host, sides_host, counts_host, F))) return rc;
    const hipStream_t s = h->own_stream;
    // the steps that fix the row count first (staging is sized by it): what clearance_enqueue does again, then as no-ops
    if ((rc = query_sync(h, false, s, "gndt_clearance: a clearance call is not recorded into a hipGraph"))) return rc;
    const uint64_t rows = h->res_nodes;
    const uint64_t bytes[4] = {hops_host ? rows * 4 : 0, nearest_host ? rows * 4 : 0, sides_host ? rows : 0, 4 * sizeof(uint32_t)};
    void* dev[4];
    if ((rc = stage_pieces(h, bytes, dev, 4))) return rc;
    if ((rc = clearance_enqueue(h, robot_of(robot), F, static_cast<uint32_t*>(dev[0]), static_cast<uint32_t*>(dev[1]),
                                static_cast<uint8_t*>(dev[2]), static_cast<uint32_t*>(dev[3]), s)))
        return rc;
    void* host[4] = {hops_host, nearest_host, sides_host, counts_host};
    for (int k = 0; k < 4; ++k)
        if (bytes[k]) HIP_TRY(h, hipMemcpyAsync(host[k], dev[k], bytes[k], hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    return GNDT_OK;
}

}  // extern "C"
