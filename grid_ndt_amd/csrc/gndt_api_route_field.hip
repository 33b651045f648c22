// gndt_api_route_field.hip — the route field (gndt_route_field.hpp): per slope the least cost to reach any of a set of goals along the
// clearance field's steps without entering a slope the caller's hops forbid, and the step to take; and the routes K starts get by
// following it.  Readers of the map like the clearance field: they run after the point queries' steps (query_sync) on the map's column
// index (column_index); launches on the caller's stream, nothing awaited — not even between the sweeps: a sweep that finds nothing
// changed by the one before returns at once.  The steps tables, the weights and the keys live in a scratch area of the handle.
#include <math.h>

#include <atomic>

#include "gndt_handle.hpp"
#include "gndt_route_field.hpp"

using namespace gndt;
using namespace gndt_host;

static_assert(sizeof(gndt_route_field_params) == 32 && sizeof(gndt_descend_params) == 32, "the ABI of include/gndt.h \"route field\"");
static_assert(sizeof(gndt_route_info) == 32 && sizeof(RouteInfo) == 32, "a route's record is two 16-byte stores");
static_assert(GNDT_ROUTE_FOUND == kRouteFound && GNDT_ROUTE_NO_START == kRouteNoStart && GNDT_ROUTE_NO_ROUTE == kRouteNoRoute &&
              GNDT_ROUTE_LIMIT == kRouteLimit && GNDT_WALK_CHECK_OVERHEAD == kRouteCheckOverhead && GNDT_NO_ROW == kNoRow,
              "gndt_route_field.hpp's constants are gndt.h's");
static_assert(sizeof(RouteFirst) == 8 && sizeof(ClearanceStep) == 8, "a side of either steps table is one 8-byte load");
static_assert(kRouteLdsRows * 8u + kRouteLdsTail <= 160u * 1024u && kRouteWgSlots <= 32u, "k_route_wg's keys fit the CU's LDS, its slots a word");

namespace gndt_host {

void free_route_field(gndt_handle* h) {
    if (h->route_field.scratch) (void)hipFree(h->route_field.scratch);
    h->route_field = gndt_handle::RouteField{};
}

namespace {

constexpr const char* kRouteCapture = "gndt_route_field: a route field call is not recorded into a hipGraph";
constexpr const char* kDescendCapture = "gndt_descend_routes: a descent is not recorded into a hipGraph";

// Arguments (every GNDT_ERR_INVALID of include/gndt.h but the handle's state) -> the rule the kernels apply
int route_args(gndt_handle* h, const gndt_route_field_params* p, const uint32_t* goals, uint32_t G, const float* cost, const uint32_t* next,
               const uint32_t* counts, RouteRule& F) {
    if (!p) { h->err = "gndt_route_field: null params"; return GNDT_ERR_INVALID; }
    if (!counts) { h->err = "gndt_route_field: null counts"; return GNDT_ERR_INVALID; }
    if (!cost && !next) { h->err = "gndt_route_field: cost and next are both NULL"; return GNDT_ERR_INVALID; }
    if (G && !goals) { h->err = "gndt_route_field: null goals"; return GNDT_ERR_INVALID; }
    if (G > kRouteMaxGoals) { h->err = "gndt_route_field: more than 2^20 goals"; return GNDT_ERR_INVALID; }
    if (p->checks & ~(uint32_t)GNDT_WALK_CHECK_OVERHEAD) { h->err = "gndt_route_field: unknown check bits"; return GNDT_ERR_INVALID; }
    if (!(p->soft_weight >= 0.f) || !(p->soft_weight <= FLT_MAX)) { h->err = "gndt_route_field: soft_weight must be finite and >= 0"; return GNDT_ERR_INVALID; }
    if (!(p->max_cost >= 0.f) || !(p->max_cost <= FLT_MAX)) { h->err = "gndt_route_field: max_cost must be finite and >= 0"; return GNDT_ERR_INVALID; }
    if (p->max_rounds > kRouteMaxRounds) { h->err = "gndt_route_field: max_rounds > 4096 (it bounds the launches of a call)"; return GNDT_ERR_INVALID; }
    for (uint32_t r : p->reserved)
        if (r != 0u) { h->err = "gndt_route_field: reserved must be 0"; return GNDT_ERR_INVALID; }
    F = RouteRule{p->checks, p->min_hops, p->soft_hops, p->soft_weight, p->max_cost, p->max_rounds ? p->max_rounds : kRouteDefaultRounds};
    return GNDT_OK;
}

// ~160 KiB of dynamic LDS have to be asked for once per device (clearance_lds_granted's rule)
bool route_lds_granted(const gndt_handle* h) {
    static std::atomic<int> state[64];                 // per device: 0 not asked yet, 1 granted, 2 refused
    if (h->device < 0 || h->device >= 64) return false;
    int st = state[h->device].load(std::memory_order_acquire);
    if (st == 0) {
        st = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_route_wg), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)(kRouteLdsRows * 8u + kRouteLdsTail)) == hipSuccess ? 1 : 2;
        if (st == 2) (void)hipGetLastError();
        state[h->device].store(st, std::memory_order_release);
    }
    return st == 1;
}

// The handle's state (query_sync has run): the stream, the column index, then the passes of gndt_route_field.hpp.  Nothing is awaited.
int route_enqueue(gndt_handle* h, const Robot& R, const RouteRule& F, const uint32_t* goals, uint32_t G, const float* goal_cost, const uint32_t* hops,
                  float* cost, uint32_t* next, uint32_t* counts, hipStream_t s) {
    int rc = use_stream(h, s);
    if (rc) return rc;
    HIP_TRY(h, hipMemsetAsync(counts, 0, 8 * sizeof(uint32_t), s));
    const uint64_t rows = h->res_nodes;
    if (rows == 0) {                                   // nothing that indexes rows: no sweep, so none that changed anything
        HIP_TRY(h, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(counts + 4), 1, 1, s));
        return GNDT_OK;
    }
    if (rows >= 0xFFFFFFFFull) { h->err = "gndt_route_field: row numbers do not fit 32 bits"; return GNDT_ERR_CAPACITY; }
    if ((rc = column_index(h, s))) return rc;
    const uint32_t n = (uint32_t)rows;
    // first steps [4 n] (8 B) | rest of the steps [4 n] (8 B) | keys [n] (8 B) | the sweeps' flags [kRouteMaxRounds + 1, padded] |
    // weights [n] (4 B) | "more" bits [n] (bytes): 77 B a row
    constexpr uint64_t kFlagWords = kRouteMaxRounds + 8u;
    auto& rf = h->route_field;
    if ((rc = grow_scratch(h, rf.scratch, rf.bytes, (uint64_t)n * 77 + kFlagWords * 4))) return rc;
    RouteFirst* first = static_cast<RouteFirst*>(rf.scratch);
    ClearanceStep* rest = reinterpret_cast<ClearanceStep*>(first + 4 * (uint64_t)n);
    unsigned long long* key = reinterpret_cast<unsigned long long*>(rest + 4 * (uint64_t)n);
    uint32_t* flags = reinterpret_cast<uint32_t*>(key + n);
    float* w = reinterpret_cast<float*>(flags + kFlagWords);
    uint8_t* more = reinterpret_cast<uint8_t*>(w + n);
    const CostView V = query_view(h).V;
    const bool wg = tuning().route_field_one_workgroup && n <= kRouteLdsRows && route_lds_granted(h);
    HIP_TRY(h, hipMemsetAsync(flags, 0, ((uint64_t)F.max_rounds + 1) * sizeof(uint32_t), s));
    // the row passes: at most 2048 workgroups of 256 threads (what the chip holds at once), grid-stride beyond
    const dim3 grid4(grid_for(4 * (uint64_t)n, 256, 2048)), grid1(grid_for(n, 256, 2048)), block(256);
    hipLaunchKernelGGL(k_route_enter, grid1, block, 0, s, V, R, F, n, hops, w, key);
    if (G) hipLaunchKernelGGL(k_route_goals, dim3(grid_for(G, 256, 2048)), block, 0, s, n, w, goals, goal_cost, G, key, counts);
    hipLaunchKernelGGL(k_route_steps, grid4, block, 0, s, V, R, n, w, first, rest, more, flags);
    if (wg) {
        hipLaunchKernelGGL(k_route_wg, dim3(1), dim3(kRouteWgThreads), (size_t)n * 8 + kRouteLdsTail, s, V, R, F.max_cost, n, F.max_rounds, first, rest,
                           more, w, key, cost, next, counts);
    } else {
        for (uint32_t round = 1; round <= F.max_rounds; ++round)
            hipLaunchKernelGGL(k_route_sweep, grid4, block, 0, s, V, R, F.max_cost, n, round, first, rest, more, w, key, flags);
        hipLaunchKernelGGL(k_route_finish, dim3(grid_for(n, 256, kRouteFinishBlocks)), block, 0, s, key, n, F.max_rounds, flags, cost, next, counts);
    }
    HIP_TRY(h, hipGetLastError());
    return GNDT_OK;
}

int descend_args(gndt_handle* h, const void* starts, size_t K, size_t stride_bytes, const gndt_descend_params* p, const float* cost,
                 const uint32_t* next, const uint32_t* rows, uint32_t route_cap, const gndt_route_info* info, DescendRule& F) {
    if (!p) { h->err = "gndt_descend_routes: null params"; return GNDT_ERR_INVALID; }
    if (!cost || !next) { h->err = "gndt_descend_routes: null cost or next"; return GNDT_ERR_INVALID; }
    if (!info) { h->err = "gndt_descend_routes: null info"; return GNDT_ERR_INVALID; }
    if (K && !starts) { h->err = "gndt_descend_routes: null starts"; return GNDT_ERR_INVALID; }
    if (K >= (1ull << 31)) { h->err = "gndt_descend_routes: 2^31 or more starts in one call"; return GNDT_ERR_INVALID; }
    if (stride_bytes != 12 && stride_bytes != 16) { h->err = "gndt_descend_routes: stride_bytes must be 12 or 16"; return GNDT_ERR_INVALID; }
    if (p->start_mode != 0 && p->start_mode != GNDT_WALK_START_NEAREST_SLOPE && p->start_mode != GNDT_WALK_START_NODE) {
        h->err = "gndt_descend_routes: unknown start_mode";
        return GNDT_ERR_INVALID;
    }
    if (p->max_steps > kWalkMaxSteps) { h->err = "gndt_descend_routes: max_steps > 2^20 (it bounds a lane's loop)"; return GNDT_ERR_INVALID; }
    for (uint32_t r : p->reserved)
        if (r != 0u) { h->err = "gndt_descend_routes: reserved must be 0"; return GNDT_ERR_INVALID; }
    if ((rows == nullptr) != (route_cap == 0u)) { h->err = "gndt_descend_routes: route_rows is NULL exactly when route_cap is 0"; return GNDT_ERR_INVALID; }
    F = DescendRule{p->start_mode == GNDT_WALK_START_NODE ? kQueryNode : kQueryNearestSlope, p->max_steps ? p->max_steps : kWalkDefaultSteps};
    return GNDT_OK;
}

int descend_enqueue(gndt_handle* h, const DescendRule& F, const float* starts, uint32_t sf, uint64_t K, const float* cost, const uint32_t* next,
                    uint32_t* rows, uint32_t route_cap, RouteInfo* info, hipStream_t s) {
    int rc = use_stream(h, s);
    if (rc) return rc;
    const uint64_t n = h->res_nodes;
    if (n >= 0xFFFFFFFFull) { h->err = "gndt_descend_routes: row numbers do not fit 32 bits"; return GNDT_ERR_CAPACITY; }
    if ((rc = column_index(h, s))) return rc;
    // one wavefront a workgroup; at most 8192 of them (k_walk_paths' grid), grid-stride beyond
    hipLaunchKernelGGL(k_route_descend, dim3(grid_for(K, kRouteDescendThreads, 8192)), dim3(kRouteDescendThreads), 0, s, query_view(h), F, (uint32_t)n, cost,
                       next, starts, sf, K, rows, route_cap, info);
    HIP_TRY(h, hipGetLastError());
    return GNDT_OK;
}

}  // namespace

}  // namespace gndt_host

extern "C" {

int gndt_route_field_device(gndt_handle* h, const gndt_robot* robot, const gndt_route_field_params* params, const uint32_t* goals_dev,
                            uint32_t G, const float* goal_cost_dev, const uint32_t* hops_dev, float* cost_dev, uint32_t* next_dev,
                            uint32_t* counts_dev, void* hip_stream) {
    int rc = check_ready(h);
    if (rc) return rc;
    RouteRule F;
    if ((rc = route_args(h, params, goals_dev, G, cost_dev, next_dev, counts_dev, F))) return rc;
    if ((reinterpret_cast<uintptr_t>(goals_dev) & 3u) || (reinterpret_cast<uintptr_t>(goal_cost_dev) & 3u) || (reinterpret_cast<uintptr_t>(hops_dev) & 3u) ||
        (reinterpret_cast<uintptr_t>(cost_dev) & 3u) || (reinterpret_cast<uintptr_t>(next_dev) & 3u) || (reinterpret_cast<uintptr_t>(counts_dev) & 3u)) {
        h->err = "gndt_route_field_device: goals_dev, goal_cost_dev, hops_dev, cost_dev, next_dev and counts_dev must be aligned to 4 bytes";
        return GNDT_ERR_INVALID;
    }
    const hipStream_t s = stream_of(h, hip_stream);
    if ((rc = query_sync(h, false, s, kRouteCapture))) return rc;
    return route_enqueue(h, robot_of(robot), F, goals_dev, G, goal_cost_dev, hops_dev, cost_dev, next_dev, counts_dev, s);
}

int gndt_route_field(gndt_handle* h, const gndt_robot* robot, const gndt_route_field_params* params, const uint32_t* goals_host, uint32_t G,
                     const float* goal_cost_host, const uint32_t* hops_host, float* cost_host, uint32_t* next_host, uint32_t* counts_host) {
    int rc = check_ready(h);
    if (rc) return rc;
    RouteRule F;
    if ((rc = route_args(h, params, goals_host, G, cost_host, next_host, counts_host, F))) return rc;
    const hipStream_t s = h->own_stream;
    // the steps that fix the row count first (staging is sized by it)
    if ((rc = query_sync(h, false, s, kRouteCapture))) return rc;
    const uint64_t rows = h->res_nodes;
    const uint64_t bytes[6] = {(uint64_t)G * 4, goal_cost_host ? (uint64_t)G * 4 : 0, hops_host ? rows * 4 : 0, cost_host ? rows * 4 : 0,
                               next_host ? rows * 4 : 0, 8 * sizeof(uint32_t)};
    void* dev[6];
    if ((rc = stage_pieces(h, bytes, dev, 6))) return rc;
    const void* in[3] = {goals_host, goal_cost_host, hops_host};
    for (int k = 0; k < 3; ++k)
        if (bytes[k]) HIP_TRY(h, hipMemcpyAsync(dev[k], in[k], bytes[k], hipMemcpyHostToDevice, s));
    // (a map without rows: hops has no entry and no row is read; the outputs have none either, and route_args has seen the caller's)
    if ((rc = route_enqueue(h, robot_of(robot), F, static_cast<const uint32_t*>(dev[0]), G, static_cast<const float*>(dev[1]),
                            static_cast<const uint32_t*>(dev[2]), static_cast<float*>(dev[3]), static_cast<uint32_t*>(dev[4]),
                            static_cast<uint32_t*>(dev[5]), s)))
        return rc;
    void* out[3] = {cost_host, next_host, counts_host};
    for (int k = 0; k < 3; ++k)
        if (bytes[3 + k]) HIP_TRY(h, hipMemcpyAsync(out[k], dev[3 + k], bytes[3 + k], hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    return GNDT_OK;
}

int gndt_descend_routes_device(gndt_handle* h, const void* starts_dev, size_t K, size_t stride_bytes, const gndt_descend_params* params,
                               const float* cost_dev, const uint32_t* next_dev, uint32_t* route_rows_dev, uint32_t route_cap,
                               gndt_route_info* info_dev, void* hip_stream) {
    int rc = check_ready(h);
    if (rc) return rc;
    DescendRule F;
    if ((rc = descend_args(h, starts_dev, K, stride_bytes, params, cost_dev, next_dev, route_rows_dev, route_cap, info_dev, F))) return rc;
    if ((reinterpret_cast<uintptr_t>(info_dev) & 15u) || (reinterpret_cast<uintptr_t>(route_rows_dev) & 3u) || (reinterpret_cast<uintptr_t>(starts_dev) & 3u) ||
        (reinterpret_cast<uintptr_t>(cost_dev) & 3u) || (reinterpret_cast<uintptr_t>(next_dev) & 3u)) {
        h->err = "gndt_descend_routes_device: info_dev must be 16-byte aligned (it is written 16 bytes at a time), starts, cost, next and route_rows 4-byte";
        return GNDT_ERR_INVALID;
    }
    const hipStream_t s = stream_of(h, hip_stream);
    if ((rc = query_sync(h, false, s, kDescendCapture))) return rc;
    if (K == 0) return GNDT_OK;
    return descend_enqueue(h, F, static_cast<const float*>(starts_dev), (uint32_t)(stride_bytes / 4), K, cost_dev, next_dev, route_rows_dev, route_cap,
                           reinterpret_cast<RouteInfo*>(info_dev), s);
}

int gndt_descend_routes(gndt_handle* h, const void* starts_host, size_t K, size_t stride_bytes, const gndt_descend_params* params,
                        const float* cost_host, const uint32_t* next_host, uint32_t* route_rows_host, uint32_t route_cap, gndt_route_info* info_host) {
    int rc = check_ready(h);
    if (rc) return rc;
    DescendRule F;
    if ((rc = descend_args(h, starts_host, K, stride_bytes, params, cost_host, next_host, route_rows_host, route_cap, info_host, F))) return rc;
    const hipStream_t s = h->own_stream;
    if ((rc = query_sync(h, false, s, kDescendCapture))) return rc;
    if (K == 0) return GNDT_OK;
    const uint64_t rows = h->res_nodes;
    const uint64_t bytes[5] = {(uint64_t)K * stride_bytes, rows * 4, rows * 4, (uint64_t)K * route_cap * 4, (uint64_t)K * sizeof(RouteInfo)};
    void* dev[5];
    if ((rc = stage_pieces(h, bytes, dev, 5))) return rc;
    const void* in[3] = {starts_host, cost_host, next_host};
    for (int k = 0; k < 3; ++k)
        if (bytes[k]) HIP_TRY(h, hipMemcpyAsync(dev[k], in[k], bytes[k], hipMemcpyHostToDevice, s));
    if ((rc = descend_enqueue(h, F, static_cast<const float*>(dev[0]), (uint32_t)(stride_bytes / 4), K, static_cast<const float*>(dev[1]),
                              static_cast<const uint32_t*>(dev[2]), static_cast<uint32_t*>(dev[3]), route_cap, static_cast<RouteInfo*>(dev[4]), s)))
        return rc;
    if (bytes[3]) HIP_TRY(h, hipMemcpyAsync(route_rows_host, dev[3], bytes[3], hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipMemcpyAsync(info_host, dev[4], bytes[4], hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    return GNDT_OK;
}

}  // extern "C"
