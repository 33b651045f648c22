// gndt_api_route_field.hip — the route field (gndt_route_field.hpp): per slope the least cost to reach any of a set of goals along the
// clearance field's steps without entering a slope the caller's hops forbid, and the step to take; and the routes K starts get by
// following it.  Readers of the map like the clearance field: they run after the point queries' steps (query_sync) on the map's column
// index (column_index); launches on the caller's stream, nothing awaited — not even between the sweeps: a sweep that finds nothing
// changed by the one before returns at once.  The steps tables, the weights and the keys live in a scratch area of the handle.
#include <math.h>

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
    if ((rc = rows_fit_32(h, "gndt_route_field")) || (rc = column_index(h, s))) return rc;
    const uint32_t n = (uint32_t)rows;
    RouteScratch S;
    if ((rc = carve_scratch(h, h->route_field, S, n))) return rc;
    const CostView V = query_view(h).V;
    static LdsGrant grant;                             // k_route_wg's ~160 KiB
    const bool wg = tuning().route_field_one_workgroup && n <= kRouteLdsRows && lds_granted(h, (const void*)&k_route_wg, kRouteLdsRows * 8u + kRouteLdsTail, grant);
    HIP_TRY(h, hipMemsetAsync(S.flags, 0, ((uint64_t)F.max_rounds + 1) * sizeof(uint32_t), s));
    // the row passes: at most 2048 workgroups of 256 threads (what the chip holds at once), grid-stride beyond
    const dim3 grid4(grid_for(4 * (uint64_t)n, 256, 2048)), grid1(grid_for(n, 256, 2048)), block(256);
    hipLaunchKernelGGL(k_route_enter, grid1, block, 0, s, V, R, F, n, hops, S.w, S.key);
    if (G) hipLaunchKernelGGL(k_route_goals, dim3(grid_for(G, 256, 2048)), block, 0, s, n, S.w, goals, goal_cost, G, S.key, counts);
    hipLaunchKernelGGL(k_route_steps, grid4, block, 0, s, V, R, n, S.w, S.first, S.rest, S.more, S.flags);
    if (wg) {
        hipLaunchKernelGGL(k_route_wg, dim3(1), dim3(kRouteWgThreads), (size_t)n * 8 + kRouteLdsTail, s, V, R, F.max_cost, n, F.max_rounds, S.first, S.rest,
                           S.more, S.w, S.key, cost, next, counts);
    } else {
        for (uint32_t round = 1; round <= F.max_rounds; ++round)
            hipLaunchKernelGGL(k_route_sweep, grid4, block, 0, s, V, R, F.max_cost, n, round, S.first, S.rest, S.more, S.w, S.key, S.flags);
        hipLaunchKernelGGL(k_route_finish, dim3(grid_for(n, 256, kRouteFinishBlocks)), block, 0, s, S.key, n, F.max_rounds, S.flags, cost, next, counts);
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
    if ((rc = rows_fit_32(h, "gndt_descend_routes")) || (rc = column_index(h, s))) return rc;
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
    if (misaligned(3u, {goals_dev, goal_cost_dev, hops_dev, cost_dev, next_dev, counts_dev})) {
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
    IoPiece io[6] = {io_in(goals_host, (uint64_t)G * 4),
                     io_in(goal_cost_host, (uint64_t)G * 4),
                     io_in(hops_host, rows * 4),
                     io_out(cost_host, rows * 4),
                     io_out(next_host, rows * 4),
                     io_out(counts_host, 8 * sizeof(uint32_t))};
    if ((rc = stage_in(h, io, s))) return rc;
    // (a map without rows: hops has no entry and no row is read; the outputs have none either, and route_args has seen the caller's)
    if ((rc = route_enqueue(h, robot_of(robot), F, io[0].as<const uint32_t>(), G, io[1].as<const float>(), io[2].as<const uint32_t>(),
                            io[3].as<float>(), io[4].as<uint32_t>(), io[5].as<uint32_t>(), s)))
        return rc;
    return stage_out(h, io, s);
}

int gndt_descend_routes_device(gndt_handle* h, const void* starts_dev, size_t K, size_t stride_bytes, const gndt_descend_params* params,
                               const float* cost_dev, const uint32_t* next_dev, uint32_t* route_rows_dev, uint32_t route_cap,
                               gndt_route_info* info_dev, void* hip_stream) {
    int rc = check_ready(h);
    if (rc) return rc;
    DescendRule F;
    if ((rc = descend_args(h, starts_dev, K, stride_bytes, params, cost_dev, next_dev, route_rows_dev, route_cap, info_dev, F))) return rc;
    if (misaligned(15u, {info_dev}) || misaligned(3u, {route_rows_dev, starts_dev, cost_dev, next_dev})) {
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
    IoPiece io[5] = {io_in(starts_host, (uint64_t)K * stride_bytes),
                     io_in(cost_host, rows * 4),
                     io_in(next_host, rows * 4),
                     io_out(route_rows_host, (uint64_t)K * route_cap * 4),
                     io_out(info_host, (uint64_t)K * sizeof(RouteInfo))};
    if ((rc = stage_in(h, io, s))) return rc;
    if ((rc = descend_enqueue(h, F, io[0].as<const float>(), (uint32_t)(stride_bytes / 4), K, io[1].as<const float>(), io[2].as<const uint32_t>(),
                              io[3].as<uint32_t>(), route_cap, io[4].as<RouteInfo>(), s)))
        return rc;
    return stage_out(h, io, s);
}

}  // extern "C"
