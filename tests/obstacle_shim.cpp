// Host build of the obstacle field's per-element code (grid_ndt_amd/csrc/gndt_obstacle.hpp: obstacle_window, obstacle_box_of,
// obstacle_mark_item / obstacle_mark_column, obstacle_side, obstacle_key0, obstacle_round_side, obstacle_finish_row, and through them
// the clearance field's clearance_side / clearance_round_side / clearance_relax / clearance_round_stores / clearance_finish_row) for the
// CPU test tier, compiled with g++: the passes of gndt_api_obstacle.hip run one element after another.  The prefix sums of the windows
// kernel are a plain running sum here.  order 0 marks the items of the concatenated windows front to back, order 1 back to front: the
// worklist then holds the columns in another order, and the answer must not care.  The stamped marks (cstamp, slot, cover) are the
// caller's, so that a test can run call after call on the same words, or on words full of garbage below the stamp.
// Test infrastructure only (tests/test_obstacle_host.py).
#include <stdint.h>

#include <vector>

#include "gndt_obstacle.hpp"
#include "shim_map.hpp"

using namespace gndt;

extern "C" {

// prm: {inflate, max_hops, levels_above, levels_below} already resolved (max_hops >= 1), max_columns >= 1.  n_boxes_dev < 0: none.
// hops, obstacle [n] (either may be null), counts [8] as gndt_obstacle_field writes them; info[0] = the worklist's length, info[1] =
// the rounds that did any work, info[2..4] = probes, claims, cover atomics of the mark pass.  Returns 0.
int obshim_field(int order, const float* robot, const void* boxes, uint32_t n_boxes, uint64_t stride, int64_t n_boxes_dev, const uint32_t* prm,
                 uint64_t max_columns, const ShimMap* m, uint32_t stamp, uint32_t* cstamp, uint32_t* slot, unsigned long long* cover,
                 const uint32_t* base, uint32_t* hops, uint32_t* obstacle, uint32_t* counts, uint32_t* info) {
    const CostView V = view_of(*m).V;
    const uint32_t n = (uint32_t)m->n;
    const Robot R{robot[0], robot[1], robot[2], robot[3]};
    const ObstacleRule F{prm[0], prm[1], prm[2], prm[3], max_columns};
    using Ops = ObstacleSerialOps;
    for (int k = 0; k < 8; ++k) counts[k] = 0u;
    // the windows
    const uint32_t B = n_boxes_dev < 0 ? n_boxes : ((uint64_t)n_boxes_dev < n_boxes ? (uint32_t)n_boxes_dev : n_boxes);
    std::vector<unsigned long long> W(n_boxes + 1u);
    std::vector<uint32_t> covers(n_boxes + 1u, 0xA5A5A5A5u);
    unsigned long long sum = 0ull, items = 0ull;
    uint32_t dropped = 0u;
    for (uint32_t b = 0; b < B; ++b) {
        const int32_t* box = obstacle_box(boxes, stride, b);
        const bool solid = !obstacle_void(box);
        ObstacleWindow w;
        if (solid) sum += obstacle_window(box, F.inflate + F.max_hops, w);
        W[b] = sum;
        covers[b] = 0u;
        if (solid && sum <= F.max_columns) items = sum;
        if (solid && sum > F.max_columns) ++dropped;
    }
    counts[3] = B;
    if (n == 0u) return 0;
    counts[6] = dropped;
    // the fill
    for (uint32_t row = 0; row < n; ++row) {
        if (hops && hops != base) hops[row] = base ? base[row] : kClrBeyond;
        if (obstacle) obstacle[row] = kNoRow;
    }
    // the marks
    std::vector<uint32_t> list(n, 0xA5A5A5A5u);
    uint32_t len = 0u;
    ObstacleMarks M{cstamp, slot, cover, list.data(), &len, covers.data()};
    ObstacleMarkTally tally{0u, 0u, 0u};
    for (unsigned long long k = 0; k < items; ++k)
        obstacle_mark_item<Ops>(V, F, boxes, stride, W.data(), B, order ? items - 1ull - k : k, stamp, M, tally);
    // the steps
    std::vector<ClearanceStep> step(4 * (size_t)len);
    std::vector<uint8_t> tall(len);
    std::vector<unsigned long long> key[2] = {std::vector<unsigned long long>(len), std::vector<unsigned long long>(len, 0xA5A5A5A5A5A5A5A5ull)};
    for (uint32_t i = 0; i < len; ++i) {
        const uint32_t row = list[i];
        uint32_t tb = 0u;
        for (uint32_t k = 0; k < 4u; ++k) {
            ClearanceStep st{kNoColumn, 0u};
            const uint32_t bits = row_has_slope(V, row) ? obstacle_side(V, R, row, k, stamp, M, st) : 0u;
            step[4 * (size_t)i + k] = st;
            tb |= (bits & kClrSideTall) ? 1u << k : 0u;
        }
        tall[i] = (uint8_t)tb;
        key[0][i] = obstacle_key0(V, list[i], stamp, M);
    }
    // the rounds: the device's schedule (k_obstacle_round)
    std::vector<uint32_t> flag(F.max_hops + 1u, 0u);
    flag[0] = len ? 1u : 0u;
    uint32_t worked = 0u;
    for (uint32_t round = 1; round <= F.max_hops; ++round) {
        if (!flag[round - 1]) continue;
        ++worked;
        const unsigned long long* key_in = key[(round - 1) & 1].data();
        unsigned long long* key_out = key[round & 1].data();
        for (uint32_t i = 0; i < len; ++i) {
            const unsigned long long own = key_in[i];
            unsigned long long least = kClrNoKey;
            if (own == kClrNoKey && row_has_slope(V, list[i]))
                for (uint32_t k = 0; k < 4u; ++k) {
                    const unsigned long long s = obstacle_round_side<Ops>(V, R, list[i], step[4 * (size_t)i + k], (tall[i] >> k) & 1u, list.data(), key_in);
                    least = s < least ? s : least;
                }
            const unsigned long long k2 = clearance_relax(own, least);
            if (clearance_round_stores(k2, round)) key_out[i] = k2;
            if (k2 != own) flag[round] = 1u;
        }
    }
    // the finish
    const unsigned long long* answer = key[F.max_hops & 1].data();
    uint32_t in_reach = 0u, covering = 0u;
    for (uint32_t i = 0; i < len; ++i) {
        ClearanceTally t{0u, 0u, 0u};
        obstacle_finish_row(V, list[i], answer[i], F.max_hops, base, hops, obstacle, t, in_reach);
        clearance_fold<Ops>(counts, t);
    }
    for (uint32_t b = 0; b < B; ++b) covering += covers[b] ? 1u : 0u;
    counts[4] = covering;
    counts[5] = in_reach;
    if (info) { info[0] = len; info[1] = worked; info[2] = tally.probes; info[3] = tally.claims; info[4] = tally.cover_atomics; }
    return 0;
}

}  // extern "C"
