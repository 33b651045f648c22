// Host build of the clearance field's per-row code (grid_ndt_amd/csrc/gndt_clearance.hpp: clearance_side, clearance_key0,
// clearance_round_side / clearance_round_row / clearance_relax / clearance_round_stores, clearance_finish_row / clearance_fold) for the CPU test tier, compiled
// with g++: the steps pass, the rounds and the finish run one row after another.  Mode 0 is the device's schedule: max_hops ping-pong
// rounds, each looking at the flag of the one before, the second key array starting as garbage.  Mode 1 relaxes ONE key array in place
// in row order until a sweep changes nothing and clamps at the end: what any interleaving of threads would converge to (and it walks a
// row through clearance_round_row, as the one-workgroup kernel does; mode 0 side by side, as the launch-a-hop kernel's lanes do).
// Test infrastructure only (tests/test_clearance_host.py).
#include <stdint.h>

#include <vector>

#include "gndt_clearance.hpp"
#include "shim_map.hpp"

using namespace gndt;

extern "C" {

uint32_t clshim_step_rows() { return kStepRows; }

// robot: {radius, reachable_height, max_rough, max_angle_deg}.  hops, nearest [n], sides [n], counts [4] as gndt_clearance writes them;
// info[0] = the rounds that did any work (mode 0) or the sweeps (mode 1).  Returns 0.
int clshim_clearance(int mode, const float* robot, uint32_t sources, uint32_t max_hops, const ShimMap* m, uint32_t* hops, uint32_t* nearest,
                     uint8_t* sides, uint32_t* counts, uint32_t* info) {
    const CostView V = view_of(*m).V;
    const uint32_t n = (uint32_t)m->n;
    const Robot R{robot[0], robot[1], robot[2], robot[3]};
    const ClearanceRule F{sources, max_hops};
    using Ops = ClearanceSerialOps;
    std::vector<ClearanceStep> step(4 * (size_t)n);
    std::vector<uint8_t> tall(n);
    std::vector<unsigned long long> key[2] = {std::vector<unsigned long long>(n), std::vector<unsigned long long>(n, 0xA5A5A5A5A5A5A5A5ull)};
    // the steps pass
    for (uint32_t row = 0; row < n; ++row) {
        const bool slope = row_has_slope(V, row);
        uint32_t sb = 0u;
        for (uint32_t k = 0; k < 4u; ++k) {
            ClearanceStep st{kNoColumn, 0u};
            const uint32_t bits = slope ? clearance_side(V, R, row, k, st) : 0u;
            step[4 * (size_t)row + k] = st;
            sb |= ((bits & kClrSideBlocked) ? 1u << k : 0u) | ((bits & kClrSideOpen) ? 16u << k : 0u) | ((bits & kClrSideTall) ? 256u << k : 0u);
        }
        tall[row] = (uint8_t)(sb >> 8);
        if (sides) sides[row] = slope ? (uint8_t)sb : (uint8_t)0xFFu;
        key[0][row] = slope ? clearance_key0(V, R, F, row, sb & 0xFFu) : kClrNoKey;
    }
    // mode 0 walks a row side by side (the launch-a-hop kernel's lanes), mode 1 through clearance_round_row (the one-workgroup kernel's)
    const auto least_of = [&](uint32_t row, const unsigned long long* key_in) {
        if (mode == 1) return clearance_round_row<Ops>(V, R, row, &step[4 * (size_t)row], tall[row], key_in);
        unsigned long long least = kClrNoKey;
        for (uint32_t k = 0; k < 4u; ++k) {
            const unsigned long long m = clearance_round_side<Ops>(V, R, row, step[4 * (size_t)row + k], (tall[row] >> k) & 1u, key_in);
            least = m < least ? m : least;
        }
        return least;
    };
    const unsigned long long* answer = key[0].data();
    uint32_t worked = 0;
    if (mode == 0) {
        std::vector<uint32_t> flag(max_hops + 1, 0u);
        flag[0] = 1u;
        for (uint32_t round = 1; round <= max_hops; ++round) {
            if (!flag[round - 1]) continue;                 // the launch returns at once
            ++worked;
            const unsigned long long* key_in = key[(round - 1) & 1].data();
            unsigned long long* key_out = key[round & 1].data();
            for (uint32_t row = 0; row < n; ++row) {
                const unsigned long long own = key_in[row];
                const bool relax = own == kClrNoKey && row_has_slope(V, row);
                const unsigned long long k2 = clearance_relax(own, relax ? least_of(row, key_in) : kClrNoKey);
                if (clearance_round_stores(k2, round)) key_out[row] = k2;
                if (k2 != own) flag[round] = 1u;
            }
        }
        answer = key[max_hops & 1].data();
    } else {
        unsigned long long* k = key[0].data();
        for (uint32_t sweep = 0; sweep <= n + 1; ++sweep) {
            bool changed = false;
            ++worked;
            for (uint32_t row = 0; row < n; ++row) {
                if (!row_has_slope(V, row)) continue;
                const unsigned long long k2 = clearance_relax(k[row], least_of(row, k));      // (a key found early may still get shorter)
                if (k2 != k[row]) { k[row] = k2; changed = true; }
            }
            if (!changed) break;
        }
    }
    // the finish
    counts[0] = counts[1] = counts[2] = counts[3] = 0u;
    for (uint32_t row = 0; row < n; ++row) {
        ClearanceTally t{0u, 0u, 0u};
        uint32_t hp, nr;
        clearance_finish_row(answer[row], max_hops, hp, nr, t);
        if (hops) hops[row] = hp;
        if (nearest) nearest[row] = nr;
        clearance_fold<Ops>(counts, t);
    }
    if (info) info[0] = worked;
    return 0;
}

}  // extern "C"
