// gndt_api_plan.hip — route planning (gndt_plan.hpp): AstarPlanar::findRoute from a batch of starts to the goal of the last cost flood.
// A reader of the map and of the cost map like the gathered point queries: no capture, a finished map, the current cost map and the
// tables its flood kept; launches on the caller's stream, nothing awaited.  Per-query state lives in a scratch area of the handle;
// queries that do not fit the caller's budget together run in consecutive launches.
#include "gndt_handle.hpp"
#include "gndt_plan.hpp"

using namespace gndt;
using namespace gndt_host;

static_assert(sizeof(gndt_plan_params) == 32 && sizeof(gndt_route_info) == 32 && sizeof(RouteInfo) == 32, "the ABI of include/gndt.h \"route planning\"");
static_assert(GNDT_ROUTE_FOUND == kRouteFound && GNDT_ROUTE_NO_START == kRouteNoStart && GNDT_ROUTE_NO_ROUTE == kRouteNoRoute &&
              GNDT_ROUTE_LIMIT == kRouteLimit && GNDT_ROUTE_NO_GOAL == kRouteNoGoal, "gndt_plan.hpp's status codes are gndt.h's");

namespace gndt_host {

namespace {

constexpr uint64_t kPlanDefaultScratch = 256ull << 20;
constexpr uint64_t kMaxQueries = 0x7FFFFFFFull;

// Arguments (every GNDT_ERR_INVALID of include/gndt.h but the handle's state)
int plan_check_args(gndt_handle* h, const void* starts, size_t K, size_t stride_bytes, const gndt_plan_params* p, const uint32_t* route_rows,
                    uint32_t route_cap, const gndt_route_info* info) {
    if (!p) { h->err = "gndt_plan_routes: null params"; return GNDT_ERR_INVALID; }
    if (K && (!starts || !info)) { h->err = "gndt_plan_routes: null starts or info"; return GNDT_ERR_INVALID; }
    if (K > kMaxQueries) { h->err = "gndt_plan_routes: more than 2^31 - 1 starts in one call"; return GNDT_ERR_INVALID; }
    if (stride_bytes != 12 && stride_bytes != 16) { h->err = "gndt_plan_routes: stride_bytes must be 12 or 16"; return GNDT_ERR_INVALID; }
    if (p->start_mode != GNDT_QUERY_NODE && p->start_mode != GNDT_QUERY_NEAREST_SLOPE) { h->err = "gndt_plan_routes: unknown start_mode"; return GNDT_ERR_INVALID; }
    for (uint32_t r : p->reserved)
        if (r != 0u) { h->err = "gndt_plan_routes: reserved must be 0"; return GNDT_ERR_INVALID; }
    if (K && (route_rows == nullptr) != (route_cap == 0u)) { h->err = "gndt_plan_routes: route_rows is NULL exactly when route_cap is 0"; return GNDT_ERR_INVALID; }
    return GNDT_OK;
}

// The handle's state: no capture, a finished map, the cost map of that map and the tables its flood kept
int plan_sync(gndt_handle* h, hipStream_t s) {
    int rc = refuse_capture(h, s, "gndt_plan_routes: a planning call is not recorded into a hipGraph");
    if (!rc) rc = finished_map(h, "no finished build to plan on (findRoute runs after create2DMap and computeCost, receiver.cpp:160-176)", false);
    if (!rc) rc = cost_map_check(h);
    if (!rc && h->cost.h_cc->goal_status == 0 && !(h->res_columns && map_current(h, h->cost.tables_serial))) {
        h->err = "gndt_plan_routes: the flood's tables are not the current map's (a handle that has recorded a hipGraph keeps none)";
        rc = GNDT_ERR_INVALID;
    }
    return rc;
}

PlanView plan_view(gndt_handle* h) {
    PlanView P{};
    CostView& V = P.V = query_view(h).V;
    V.nbr = h->cost.nbr; V.self = h->cost.nbr + 8 * h->cost.node_cap; V.edges = h->cost.edges;
    const float* r = h->cost.tables_robot;
    P.R = Robot{r[0], r[1], r[2], r[3]};
    P.h_bits = h->cost.h_bits;
    P.goal_row = h->cost.h_cc->goal_row;
    P.num_rows = (uint32_t)h->res_nodes;
    return P;
}

// Everything on the device, on stream s; waits for nothing.
int plan_launch(gndt_handle* h, const float* starts, uint32_t sf, uint64_t K, const gndt_plan_params* p, uint32_t* route, uint32_t route_cap,
                RouteInfo* info, hipStream_t s) {
    if (h->cost.h_cc->goal_status != 0) {          // the last flood found no goal slope: nothing to search for
        hipLaunchKernelGGL(k_plan_fill, dim3(grid_for(std::max<uint64_t>(K, (uint64_t)K * route_cap))), dim3(256), 0, s, K, (int32_t)kRouteNoGoal,
                           route, (uint64_t)K * route_cap, info);
        HIP_TRY(h, hipGetLastError());
        return GNDT_OK;
    }
    auto& pl = h->plan;
    const uint64_t rows = h->res_nodes;
    const uint32_t entries = plan_queue_entries(h->res_slopes);
    const uint32_t cap0 = (uint32_t)tuning().plan_lds_entries;
    const uint32_t cap1 = entries > cap0 ? entries - cap0 : 0u;
    const uint64_t slot_bytes = (rows * sizeof(PlanRowState) + (uint64_t)cap1 * 8 + 255) & ~255ull;
    const uint64_t budget = p->scratch_bytes ? p->scratch_bytes : kPlanDefaultScratch;
    const uint64_t per_launch = std::min<uint64_t>(K, budget / slot_bytes);
    if (per_launch == 0) {
        h->err = "gndt_plan_routes: one query's state (" + std::to_string(slot_bytes) + " bytes) does not fit scratch_bytes";
        return GNDT_ERR_CAPACITY;
    }
    const uint64_t want = per_launch * slot_bytes;
    // Stamps (gndt_plan.hpp PlanRowState) stand for "cleared": the area is zeroed when it is new, when a slot's layout changes (another
    // map size moves the words a stamp is read from) and when the stamps run out.
    const bool fresh = want > pl.scratch.bytes || pl.slot_bytes != slot_bytes || pl.rows != rows;
    int rc = grow_scratch(h, pl.scratch.p, pl.scratch.bytes, want);
    if (rc) return rc;
    const uint32_t max_exp = p->max_expansions ? p->max_expansions : plan_default_expansions(h->res_slopes);
    const PlanView P = plan_view(h);
    const QueryView Q = query_view(h);
    for (uint64_t first = 0; first < K; first += per_launch) {
        const uint64_t count = std::min<uint64_t>(per_launch, K - first);
        if ((fresh && first == 0) || pl.stamp >= 0x7FFFFFFEu) {
            HIP_TRY(h, hipMemsetAsync(pl.scratch.p, 0, pl.scratch.bytes, s));
            pl.stamp = 0; pl.slot_bytes = slot_bytes; pl.rows = rows;
        }
        const uint32_t stamp = ++pl.stamp;
        if (p->start_mode == GNDT_QUERY_NODE)
            hipLaunchKernelGGL((k_plan<kQueryNode>), dim3((uint32_t)count), dim3(64), 0, s, P, Q, starts, sf, first, static_cast<char*>(pl.scratch.p),
                               slot_bytes, cap0, cap1, stamp, max_exp, route, route_cap, info);
        else
            hipLaunchKernelGGL((k_plan<kQueryNearestSlope>), dim3((uint32_t)count), dim3(64), 0, s, P, Q, starts, sf, first,
                               static_cast<char*>(pl.scratch.p), slot_bytes, cap0, cap1, stamp, max_exp, route, route_cap, info);
    }
    HIP_TRY(h, hipGetLastError());
#if defined(GNDT_PLAN_STAMPS)
    {   // the diagnostic build waits and reports: cycles per expansion of a wavefront, by phase (gndt_plan.hpp)
        unsigned long long v[8];
        HIP_TRY(h, hipStreamSynchronize(s));
        HIP_TRY(h, hipMemcpyFromSymbol(v, HIP_SYMBOL(g_plan_stamps), sizeof(v)));
        const double e = (double)std::max<unsigned long long>(v[6], 1), qn = (double)std::max<unsigned long long>(v[7], 1);
        std::fprintf(stderr, "[gndt plan stamps] queries %llu expansions %llu; cycles per expansion: pop %.0f, temp's state + records %.0f, "
                     "neighbours' h + state %.0f, relaxations %.0f, close + compact %.0f; father walk per query %.0f\n", v[7], v[6], v[0] / e,
                     v[1] / e, v[2] / e, v[3] / e, v[4] / e, v[5] / qn);
        const unsigned long long zero[8] = {};
        HIP_TRY(h, hipMemcpyToSymbol(HIP_SYMBOL(g_plan_stamps), zero, sizeof(zero)));
    }
#endif
    return GNDT_OK;
}

}  // namespace

}  // namespace gndt_host

extern "C" {

int gndt_plan_routes_device(gndt_handle* h, const void* starts_dev, size_t K, size_t stride_bytes, const gndt_plan_params* params,
                            uint32_t* route_rows_dev, uint32_t route_cap, gndt_route_info* info_dev, void* hip_stream) {
    int rc = check_ready(h);
    if (rc) return rc;
    if ((rc = plan_check_args(h, starts_dev, K, stride_bytes, params, route_rows_dev, route_cap, info_dev))) return rc;
    const hipStream_t s = stream_of(h, hip_stream);
    if ((rc = plan_sync(h, s))) return rc;
    if (K == 0) return GNDT_OK;
    if ((rc = use_stream(h, s)) || (rc = column_index(h, s))) return rc;
    if (misaligned(15u, {info_dev}) || misaligned(3u, {route_rows_dev, starts_dev})) {
        h->err = "gndt_plan_routes_device: info_dev must be 16-byte aligned (it is written 16 bytes at a time), starts and route_rows 4-byte";
        return GNDT_ERR_INVALID;
    }
    return plan_launch(h, static_cast<const float*>(starts_dev), (uint32_t)(stride_bytes / 4), K, params, route_rows_dev, route_cap,
                       reinterpret_cast<RouteInfo*>(info_dev), s);
}

int gndt_plan_routes(gndt_handle* h, const void* starts_host, size_t K, size_t stride_bytes, const gndt_plan_params* params,
                     uint32_t* route_rows_host, uint32_t route_cap, gndt_route_info* info_host) {
    int rc = check_ready(h);
    if (rc) return rc;
    if ((rc = plan_check_args(h, starts_host, K, stride_bytes, params, route_rows_host, route_cap, info_host))) return rc;
    const hipStream_t s = h->own_stream;
    if ((rc = plan_sync(h, s))) return rc;
    if (K == 0) return GNDT_OK;
    if ((rc = use_stream(h, s)) || (rc = column_index(h, s))) return rc;
    IoPiece io[3] = {io_in(starts_host, (uint64_t)K * stride_bytes),
                     io_out(route_rows_host, (uint64_t)K * route_cap * 4),
                     io_out(info_host, (uint64_t)K * sizeof(RouteInfo))};
    if ((rc = stage_in(h, io, s))) return rc;
    if ((rc = plan_launch(h, io[0].as<const float>(), (uint32_t)(stride_bytes / 4), K, params, io[1].as<uint32_t>(), route_cap, io[2].as<RouteInfo>(), s)))
        return rc;
    return stage_out(h, io, s);
}

}  // extern "C"
