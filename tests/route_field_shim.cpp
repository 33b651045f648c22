// Host build of the route field's per-row code (grid_ndt_amd/csrc/gndt_route_field.hpp: route_weight, route_seed, route_side,
// route_sweep_side / route_sweep_row / route_cand, route_finish_row / route_fold, route_descend) for the CPU test tier, compiled with
// g++: the passes run one row after another.  Mode 0 is the slowest schedule the definition allows: every sweep reads the keys the
// sweep before left (a copy), a row side by side as the launch-a-sweep kernel's lanes walk it — the schedule "L + 1 sweeps suffice"
// speaks of.  Mode 1 relaxes the one key array in place in ascending row order through route_sweep_row (the one-workgroup kernel's
// walk), mode 2 in place in descending row order: two of the interleavings the device may take.  Every mode stops like the device:
// after max_rounds sweeps, or behind the first sweep that changes nothing.  Test infrastructure only (tests/test_route_field_host.py).
#include <stdint.h>

#include <vector>

#include "gndt_route_field.hpp"
#include "shim_map.hpp"

using namespace gndt;

extern "C" {

uint32_t rfshim_lds_rows() { return kRouteLdsRows; }

// robot: {radius, reachable_height, max_rough, max_angle_deg}; rule: {checks, min_hops, soft_hops, max_rounds}, fr: {soft_weight,
// max_cost}.  cost, next [n] and counts [8] as gndt_route_field writes them.  Returns 0.
int rfshim_field(int mode, const float* robot, const uint32_t* rule, const float* fr, const ShimMap* m, const uint32_t* goals, uint32_t G,
                 const float* goal_cost, const uint32_t* hops, float* cost, uint32_t* next, uint32_t* counts) {
    const CostView V = view_of(*m).V;
    const uint32_t n = (uint32_t)m->n;
    const Robot R{robot[0], robot[1], robot[2], robot[3]};
    const RouteRule F{rule[0], rule[1], rule[2], fr[0], fr[1], rule[3] ? rule[3] : kRouteDefaultRounds};
    using Ops = RouteSerialOps;
    for (int k = 0; k < 8; ++k) counts[k] = 0u;
    if (n == 0u) { counts[4] = 1u; return 0; }
    std::vector<float> w(n);
    std::vector<unsigned long long> key(n, kRouteNoKey), prev;
    for (uint32_t row = 0; row < n; ++row) w[row] = route_weight(V, R, F, hops, row);
    for (uint32_t g = 0; g < G; ++g) {
        const unsigned long long seed = route_seed(n, w.data(), goals[g], goal_cost ? goal_cost[g] : 0.f);
        if (seed == kRouteNoKey) { counts[1] += 1u; continue; }
        counts[0] += 1u;
        Ops::min_key(&key[goals[g]], seed);
    }
    std::vector<RouteFirst> first(4 * (size_t)n);
    std::vector<ClearanceStep> rest(4 * (size_t)n);
    std::vector<uint8_t> more(n);
    for (uint32_t row = 0; row < n; ++row) {
        uint32_t mb = 0u;
        for (uint32_t k = 0; k < 4u; ++k) {
            ClearanceStep st{kNoColumn, 0u}, rs{kNoColumn, 0u};
            RouteFirst f{kNoRow, 0u};
            if (row_has_slope(V, row)) {
                const bool tall = (clearance_side(V, R, row, k, st) & kClrSideTall) != 0u;
                if (route_side(V, row, st, tall, w.data(), f, rs)) mb |= 1u << k;
                if (tall) mb |= 16u << k;
            }
            first[4 * (size_t)row + k] = f;
            rest[4 * (size_t)row + k] = rs;
        }
        more[row] = (uint8_t)mb;
    }
    const auto relax = [&](uint32_t row, const unsigned long long* in) -> bool {
        if (!row_has_slope(V, row)) return false;
        unsigned long long least = kRouteNoKey;
        const uint32_t mb = more[row];
        if (mode == 0) {
            for (uint32_t k = 0; k < 4u; ++k) {
                const unsigned long long c = route_sweep_side<Ops>(V, R, F.max_cost, row, first[4 * (size_t)row + k], rest[4 * (size_t)row + k],
                                                                   ((mb >> k) & 1u) | (((mb >> (4u + k)) & 1u) << 4), w.data(), in);
                least = c < least ? c : least;
            }
        } else {
            least = route_sweep_row<Ops>(V, R, F.max_cost, row, &first[4 * (size_t)row], &rest[4 * (size_t)row], mb, w.data(), in);
        }
        if (least != kRouteNoKey && least < Ops::load_key(&key[row])) { Ops::store_key(&key[row], least); return true; }
        return false;
    };
    uint32_t converged = 0u;
    for (uint32_t round = 1; round <= F.max_rounds; ++round) {
        bool changed = false;
        if (mode == 0) {
            prev = key;
            for (uint32_t row = 0; row < n; ++row) changed |= relax(row, prev.data());
        } else if (mode == 1) {
            for (uint32_t row = 0; row < n; ++row) changed |= relax(row, key.data());
        } else {
            for (uint32_t row = n; row-- > 0u;) changed |= relax(row, key.data());
        }
        if (!changed) { converged = 1u; break; }
        counts[5] += 1u;
    }
    counts[4] = converged;
    for (uint32_t row = 0; row < n; ++row) {
        RouteTally t{0u, 0u};
        uint32_t cb, nx;
        route_finish_row(key[row], cb, nx, t);
        if (cost) cost[row] = bits_float(cb);
        if (next) next[row] = nx;
        route_fold<Ops>(counts, t);
    }
    return 0;
}

// gndt_descend_routes' lanes one after another: info [K] gndt_route_info records (8 words each)
int rfshim_descend(const ShimMap* m, int start_node, uint32_t max_steps, const float* cost, const uint32_t* next, const float* starts,
                   uint32_t sf, uint32_t K, uint32_t* rows, uint32_t route_cap, uint32_t* info) {
    const QueryView Q = view_of(*m);
    const DescendRule P{start_node ? kQueryNode : kQueryNearestSlope, max_steps ? max_steps : kWalkDefaultSteps};
    for (uint32_t p = 0; p < K; ++p) {
        RouteInfo o;
        route_descend(Q, P, (uint32_t)m->n, cost, next, starts + (size_t)p * sf, rows ? rows + (size_t)p * route_cap : nullptr, route_cap, o);
        uint32_t* out = info + 8 * (size_t)p;
        out[0] = (uint32_t)o.status; out[1] = o.length; out[2] = o.start_row; out[3] = o.expansions; out[4] = o.queue_peak;
        out[5] = float_bits(o.cost); out[6] = float_bits(o.h_start); out[7] = 0u;
    }
    return 0;
}

}  // extern "C"
