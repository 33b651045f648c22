// Host build of the path walks' per-path code (grid_ndt_amd/csrc/gndt_walk.hpp: walk_start, walk_step, walk_enter, walk_path) for the CPU
// test tier, compiled with g++: one path after another.  table = 1 first makes the per-side steps table the way k_clearance_steps'
// lanes do (clearance_side on every slope's four sides) and walks through walk_path<true>.  Test infrastructure only
// (tests/test_walk_host.py).
#include <stdint.h>

#include <vector>

#include "gndt_walk.hpp"
#include "shim_map.hpp"

using namespace gndt;

static_assert(sizeof(WalkInfo) == 48, "gndt_walk_info");

extern "C" {

// robot: {radius, reachable_height, max_rough, max_angle_deg}; rule: {start_mode (kQueryNode / kQueryNearestSlope), checks, min_hops,
// max_steps (resolved)}.  info [K] (48 bytes each), rows [K * row_cap] as gndt_walk_paths writes them.  Returns 0.
int wshim_walk(int table, const float* robot, const uint32_t* rule, const ShimMap* m, const uint32_t* hops, const float* paths, uint32_t sf,
               uint64_t K, uint32_t T, uint32_t* rows, uint32_t row_cap, WalkInfo* info) {
    const QueryView Q = view_of(*m);
    const CostView& V = Q.V;
    const uint32_t n = (uint32_t)m->n;
    const Robot R{robot[0], robot[1], robot[2], robot[3]};
    const WalkRule P{(int)rule[0], rule[1], rule[2], rule[3]};
    std::vector<ClearanceStep> step;
    std::vector<uint8_t> tall;
    if (table) {
        step.resize(4 * (size_t)n + 1);
        tall.resize((size_t)n + 1);
        for (uint32_t row = 0; row < n; ++row) {
            uint32_t tb = 0u;
            for (uint32_t k = 0; k < 4u; ++k) {
                ClearanceStep st{kNoColumn, 0u};
                const uint32_t bits = row_has_slope(V, row) ? clearance_side(V, R, row, k, st) : 0u;
                step[4 * (size_t)row + k] = st;
                tb |= (bits & kClrSideTall) ? 1u << k : 0u;
            }
            tall[row] = (uint8_t)tb;
        }
    }
    const WalkTable W{step.data(), tall.data()};
    for (uint64_t p = 0; p < K; ++p) {
        uint32_t* r = rows ? rows + p * row_cap : nullptr;
        if (table) walk_path<true>(Q, R, P, W, hops, paths + p * T * sf, sf, T, r, row_cap, info[p]);
        else walk_path<false>(Q, R, P, W, hops, paths + p * T * sf, sf, T, r, row_cap, info[p]);
    }
    return 0;
}

}  // extern "C"
