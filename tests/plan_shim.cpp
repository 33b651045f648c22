// plan_shim.cpp — route planning's shared header (grid_ndt_amd/csrc/gndt_plan.hpp) built for the host: plan_query over a batch of starts
// as k_plan's wavefronts run it, the wave-cooperative steps as a loop over 64 lanes (PlanWaveHost).  The flood's CostEdge records are
// made here with cost_edge_record, as k_cost_neighbours makes them; neighbour columns and Slope::countUp probe the column index.
// Test infrastructure only (tests/test_plan_host.py, tests/plan_queue_main.cpp).
#include <cstring>
#include <vector>

#include "gndt_plan.hpp"
#include "shim_map.hpp"

using namespace gndt;

namespace {

// The planner's views of a map with the flood's records made for them
struct PlanMap {
    PlanView P;
    QueryView Q;
    std::vector<CostEdge> edges;
    uint64_t num_slopes = 0;
};

void make_map(PlanMap& M, const ShimMap& m, const float* robot4, uint32_t goal_row) {
    M.Q = view_of(m);
    M.Q.state = nullptr;
    CostView& V = M.Q.V;
    const uint64_t n = m.n;
    const Robot R{robot4[0], robot4[1], robot4[2], robot4[3]};
    M.edges.assign(4 * (size_t)n, CostEdge{kNoColumn, 0u, 0.f, 0.f});
    for (uint32_t row = 0; row < n; ++row) {
        if (!row_has_slope(V, row)) continue;
        ++M.num_slopes;
        for (uint32_t k = 0; k < 4u; ++k) {
            uint32_t c, ncol;
            neighbour_column(V, row, k, c, ncol);
            M.edges[4 * (size_t)row + k] = cost_edge_record(V, R, row, c, ncol);
        }
    }
    V.edges = M.edges.data();
    M.P.V = V; M.P.R = R; M.P.h_bits = m.h_bits; M.P.goal_row = goal_row; M.P.num_rows = (uint32_t)n;
}

}  // namespace

extern "C" {

uint32_t planshim_default_expansions(uint64_t num_slopes) { return plan_default_expansions(num_slopes); }
uint32_t planshim_queue_entries(uint64_t num_slopes) { return plan_queue_entries(num_slopes); }

// K queries, one after the other in ONE state area and one queue (stamps 1, 2, ...: nothing is cleared in between, as on the device).
// mode: kQueryNode / kQueryNearestSlope.  max_expansions 0, queue_entries 0: the library's defaults.  lds_entries: the first tier's size.
// route: K x route_cap (may be null with 0).  info: K x 8 words (gndt_route_info).  tally: K x 2 counters (may be null): pops of closed
// slopes, entries inserted below the popped key.
int planshim_routes(const ShimMap* m, const float* robot4, uint32_t goal_row, int mode, const float* starts, uint32_t sf, uint64_t K,
                    uint32_t max_expansions, uint32_t lds_entries, uint32_t queue_entries, uint32_t* route, uint32_t route_cap,
                    RouteInfo* info, uint32_t* tally) {
    PlanMap M;
    make_map(M, *m, robot4, goal_row);
    const uint64_t n = m->n;
    const uint32_t entries = queue_entries ? queue_entries : plan_queue_entries(M.num_slopes);
    const uint32_t cap0 = lds_entries < entries ? lds_entries : entries, cap1 = entries - cap0;
    const uint32_t max_exp = max_expansions ? max_expansions : plan_default_expansions(M.num_slopes);
    std::vector<PlanRowState> st(n ? n : 1, PlanRowState{0u, 0u, 0u, 0u});
    std::vector<uint32_t> t0(2 * (size_t)cap0 + 1), t1(2 * (size_t)cap1 + 1);
    for (uint64_t i = 0; i < K; ++i) {
        PlanQueue q;
        q.cap0 = cap0; q.cap1 = cap1; q.f0 = t0.data(); q.r0 = t0.data() + cap0; q.f1 = t1.data(); q.r1 = t1.data() + cap1;
        q.n = 0u; q.live = 0u;
        const float* p = starts + i * sf;
        const uint32_t start = mode == kQueryNode ? plan_start_row<kQueryNode>(M.Q, p[0], p[1], p[2])
                                                  : plan_start_row<kQueryNearestSlope>(M.Q, p[0], p[1], p[2]);
        uint32_t two[2] = {0u, 0u};
        plan_query<PlanWaveHost>(M.P, start, st.data(), (uint32_t)(i + 1), q, max_exp, route ? route + i * route_cap : nullptr,
                                 route ? route_cap : 0u, info[i], two);
        if (tally) { tally[2 * i] = two[0]; tally[2 * i + 1] = two[1]; }
    }
    return 0;
}

}  // extern "C"
