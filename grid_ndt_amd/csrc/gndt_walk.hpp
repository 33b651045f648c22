// gndt_walk.hpp — path walks (include/gndt.h "path walks"): K candidate polylines of T waypoints driven over the map's slopes.  Per
// path: the start slope through the query's own code (query_key / query_chunk / query_rest), then every segment crossed column by
// column in the ray walk's column sequence (ray_begin / ray_next, gndt_ray.hpp: one 4-neighbour step at a time), every column change a
// step through one side of the slope stood on, to the step (clearance's "steps of q through the side": GNDT_FLAG_SLOPE and the flood's
// cost_gates seen from q) whose mean z is nearest; the per-slope checks (row_above_hits_in, the caller's clearance hops) and the sums in
// walk order.  A dependent chain per path, independent across paths: one path a lane, like a route a wavefront in gndt_plan.hpp.
//   k_walk_paths<false>   the step found on the chain: probe -> row_ncol -> the rows' flags / rough / normal / mean -> gates (acosf) -> pick
//   k_walk_paths<true>    the step read from the per-side table k_clearance_steps makes once per call (ClearanceStep {c, mask}: 32 B a
//                         row); only the mean z comparison is left on the chain.  Columns of more than kStepRows rows: the gates again
//                         for the rows beyond the mask, as clearance_round_side does.
// Everything up to the kernel is callable on the host, so that the CPU test tier runs the kernel's own code (tests/walk_shim.cpp).
#pragma once
#include <math.h>
#include <stdint.h>

#include "gndt_clearance.hpp"
#include "gndt_ray.hpp"

namespace gndt {

constexpr int kWalkDone = 0, kWalkNoStart = 1, kWalkBlocked = 2, kWalkLeftMap = 3, kWalkOverhead = 4, kWalkTooClose = 5, kWalkLimit = 6;
constexpr uint32_t kWalkCheckOverhead = 1u;              // GNDT_WALK_CHECK_OVERHEAD
constexpr uint32_t kWalkNoSide = 0xFFFFFFFFu;
constexpr uint32_t kWalkDefaultSteps = 65536u, kWalkMaxSteps = 1u << 20;
constexpr uint32_t kWalkTableRowsPerWaypoint = 2048u;    // a map of up to this many rows per waypoint of a path walks through the steps table

struct WalkRule {                // gndt_walk_params with its defaults resolved
    int start_mode;              // kQueryNode / kQueryNearestSlope
    uint32_t checks, min_hops, max_steps;
};

struct WalkTable {               // k_clearance_steps' output for the call's robot (the table variant only)
    const ClearanceStep* step;   // [4 row + k]
    const uint8_t* tall;         // [row], bit k: side k's column has more than kStepRows rows
};

struct WalkInfo {                // gndt_walk_info
    int32_t status;
    uint32_t stop_side, steps, waypoints;
    uint32_t start_row, end_row;
    float length, climb;
    float rough_max;
    uint32_t hops_min;
    uint32_t reserved[2];
};

// The start: waypoint 0 through the query's lookup.  -> the row (kNoRow: none), its column's first row c and the column (sx, sy)
template <int MODE>
GNDT_HD uint32_t walk_start(const QueryView& Q, float px, float py, float pz, uint32_t& c, int& sx, int& sy) {
    const QueryKey k = query_key<MODE>(Q, px, py, pz);
    const uint32_t slot = query_slot(Q, k);
    c = query_column(Q, k, Q.V.ctab_key[slot], Q.V.ctab_val[slot]);
    const uint32_t ncol = c != kNoColumn ? Q.V.row_ncol[c] : 0u;
    QueryBest b;
    b.row = kNoRow; b.d = 0.f; b.sz = 0;
    query_chunk<MODE>(Q, c, ncol, 0u, k, pz, b);
    query_rest<MODE>(Q, c, ncol, k, pz, b);
    sx = k.sx; sy = k.sy;
    if (MODE == kQueryNode && b.row != kNoRow && !row_has_slope(Q.V, b.row)) return kNoRow;
    return b.row;
}

// one candidate of a step: the least fabsf(mean_z(t) - mean_z(q)) in fp32, rows offered in ascending order (a tie keeps the smaller)
GNDT_HD void walk_offer(const CostView& V, float mzq, uint32_t t, uint32_t& best, float& best_d) {
    const float d = fabsf(V.mean[3 * (size_t)t + 2] - mzq);
    if (best == kNoRow || d < best_d) { best = t; best_d = d; }
}

// The step of slope q into the neighbour column (nx, ny) through side k: the chosen row, or kNoRow with c == kNoColumn (the column is
// not in the map, or its index is beyond the codec's range) or c the column's first row (it offers no step).  dz: |mean_z(t) - mean_z(q)|.
template <bool TABLE>
GNDT_HD uint32_t walk_step(const CostView& V, const Robot& R, const WalkTable& W, uint32_t q, uint32_t k, int nx, int ny, uint32_t& c, float& dz) {
    const float* nq = V.normal + 3 * (size_t)q;
    const float* mq = V.mean + 3 * (size_t)q;
    uint32_t best = kNoRow;
    dz = 0.f;
    if (TABLE) {
#if defined(__HIP_DEVICE_COMPILE__)
        const uint2 e = reinterpret_cast<const uint2*>(W.step)[4 * (size_t)q + k];
        const ClearanceStep st{e.x, e.y};
#else
        const ClearanceStep st = W.step[4 * (size_t)q + k];
#endif
        c = st.c;
        if (c == kNoColumn) return kNoRow;
        const float mzq = mq[2];
        for (uint32_t mask = st.mask; mask; mask &= mask - 1u) walk_offer(V, mzq, c + (uint32_t)__builtin_ctz(mask), best, dz);
        if ((W.tall[q] >> k) & 1u) {                    // (a column of more than kStepRows rows: the rest through the gates)
            const uint32_t ncol = V.row_ncol[c];
            for (uint32_t j = kStepRows; j < ncol; ++j)
                if ((V.flags[c + j] & 2u) && cost_gates(V, R, c + j, nq, mq)) walk_offer(V, mzq, c + j, best, dz);
        }
        return best;
    }
    c = kNoColumn;
    if (nx < -kMaxXY || nx > kMaxXY || ny < -kMaxXY || ny > kMaxXY) return kNoRow;
    c = ctab_find(V, nx, ny);
    if (c == kNoColumn) return kNoRow;
    const uint32_t ncol = V.row_ncol[c];
    const float mzq = mq[2];
    for (uint32_t j = 0; j < ncol; ++j)
        if ((V.flags[c + j] & 2u) && cost_gates(V, R, c + j, nq, mq)) walk_offer(V, mzq, c + j, best, dz);
    return best;
}

// Slope t (the `stood`-th the path stands on, its column's first row c) is entered: its row goes out, the maxima take it, then the
// checks.  -> kWalkDone or the status that ends the path
GNDT_HD int walk_enter(const CostView& V, const Robot& R, const WalkRule& P, const uint32_t* hops, uint32_t t, uint32_t c, uint32_t stood,
                       uint32_t* rows, uint32_t row_cap, WalkInfo& o) {
    if (stood < row_cap) rows[stood] = t;
    o.end_row = t;
    const float r = V.rough[t];
    if (stood == 0u || r > o.rough_max) o.rough_max = r;
    uint32_t hp = kClrBeyond;
    if (hops) {
        hp = hops[t];
        o.hops_min = hp < o.hops_min ? hp : o.hops_min;
    }
    if ((P.checks & kWalkCheckOverhead) && row_above_hits_in(V, R, t, c)) return kWalkOverhead;
    if (hops && hp < P.min_hops) return kWalkTooClose;
    return kWalkDone;
}

// One path: wp[j * sf + 0..2] its T waypoints, rows[row_cap] (or null with 0) the slopes it stands on, o its answer.  Q.V.normal is set.
template <bool TABLE>
GNDT_HD void walk_path(const QueryView& Q, const Robot& R, const WalkRule& P, const WalkTable& W, const uint32_t* hops, const float* wp,
                       uint32_t sf, uint32_t T, uint32_t* rows, uint32_t row_cap, WalkInfo& o) {
    const CostView& V = Q.V;
    o.status = kWalkNoStart; o.stop_side = kWalkNoSide; o.steps = 0u; o.waypoints = 0u;
    o.start_row = kNoRow; o.end_row = kNoRow; o.length = 0.f; o.climb = 0.f; o.rough_max = 0.f; o.hops_min = kClrBeyond;
    o.reserved[0] = o.reserved[1] = 0u;
    uint32_t stood = 0u;                                 // slopes stood on so far
    double length = 0.0, climb = 0.0;
    const float x0 = wp[0], y0 = wp[1], z0 = wp[2];
    uint32_t c;
    int cx, cy;                                          // the column stood in
    uint32_t q = P.start_mode == kQueryNode ? walk_start<kQueryNode>(Q, x0, y0, z0, c, cx, cy)
                                            : walk_start<kQueryNearestSlope>(Q, x0, y0, z0, c, cx, cy);
    if (q != kNoRow) {
        o.start_row = q;
        o.waypoints = 1u;
        o.status = walk_enter(V, R, P, hops, q, c, stood++, rows, row_cap, o);
        RayGrid G;
        G.ox = Q.ox; G.oy = Q.oy; G.oz = Q.oz; G.grid_len = Q.grid_len; G.z_len = Q.z_len;
        G.rx = G.ry = G.rz = 0.f; G.max_range = 0.f; G.end_margin = 0.f;
        float px = x0, py = y0;
        for (uint32_t j = 1; j < T && o.status == kWalkDone; ++j) {
            const float x = wp[(size_t)j * sf], y = wp[(size_t)j * sf + 1];
            if (!(isfinite(x) && isfinite(y))) break;    // the terminator: the path ends here
            RayWalk w;
            if (!ray_begin(G, px, py, z0, x, y, z0, w)) { o.status = kWalkLeftMap; break; }
            RayColumn rc;
            ray_next(G, w, rc);                          // (the column stood in: both segments key the same float point)
            while (ray_next(G, w, rc)) {
                if (o.steps == P.max_steps) { o.status = kWalkLimit; break; }
                const uint32_t k = rc.sx == cx ? (rc.sy < cy ? 0u : 1u) : (rc.sx > cx ? 2u : 3u);
                float dz;
                const uint32_t t = walk_step<TABLE>(V, R, W, q, k, rc.sx, rc.sy, c, dz);
                if (t == kNoRow) {
                    o.status = c == kNoColumn ? kWalkLeftMap : kWalkBlocked;
                    o.stop_side = k;
                    break;
                }
                length += (double)cost_travel(V.mean + 3 * (size_t)q, V.mean + 3 * (size_t)t);
                climb += (double)dz;
                o.steps += 1u;
                q = t; cx = rc.sx; cy = rc.sy;
                if ((o.status = walk_enter(V, R, P, hops, q, c, stood++, rows, row_cap, o)) != kWalkDone) break;
            }
            if (o.status == kWalkDone) o.waypoints = j + 1u;
            px = x; py = y;
        }
    }
    o.length = (float)length;
    o.climb = (float)climb;
    for (uint32_t i = stood; i < row_cap; ++i) rows[i] = kNoRow;
}

// The table variant's scratch for a map of n rows (gndt_api_walk.hip): what k_clearance_steps writes
struct WalkScratch {
    ClearanceStep* step;             // [4 n] the steps table
    unsigned long long* key0;        // [n] its round-0 keys (not read)
    uint32_t* flag;                  // [2] its flag word, padded
    uint8_t* tall;                   // [n] the tall-column bits
    WalkScratch() = default;
    WalkScratch(Carver& c, uint64_t n)
        : step(c.take<ClearanceStep>(4 * n)), key0(c.take<unsigned long long>(n)), flag(c.take<uint32_t>(2)), tall(c.take<uint8_t>(n)) {}
};

}  // namespace gndt

#if defined(__HIPCC__)
namespace gndt {

// One path a lane, one wavefront a workgroup: the walk is a chain of dependent loads per path and nothing is shared between paths (no
// LDS), so what hides the latency is the number of wavefronts in flight and what a wavefront costs is its longest path — 64-thread
// workgroups spread a call of a few thousand paths over as many CUs as it has wavefronts.  info: three 16-byte stores a path.
constexpr int kWalkThreads = 64;
template <bool TABLE>
static __global__ void __launch_bounds__(kWalkThreads) k_walk_paths(QueryView Q, Robot R, WalkRule P, WalkTable W, const uint32_t* __restrict__ hops,
                                                                    const float* __restrict__ paths, uint32_t sf, uint64_t K, uint32_t T,
                                                                    uint32_t* __restrict__ rows, uint32_t row_cap, WalkInfo* __restrict__ info) {
    const uint64_t gsz = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < K; p += gsz) {
        WalkInfo o;
        walk_path<TABLE>(Q, R, P, W, hops, paths + p * T * sf, sf, T, rows ? rows + p * row_cap : nullptr, row_cap, o);
        uint4* out = reinterpret_cast<uint4*>(info + p);
        out[0] = make_uint4((uint32_t)o.status, o.stop_side, o.steps, o.waypoints);
        out[1] = make_uint4(o.start_row, o.end_row, float_bits(o.length), float_bits(o.climb));
        out[2] = make_uint4(float_bits(o.rough_max), o.hops_min, 0u, 0u);
    }
}

}  // namespace gndt
#endif  // __HIPCC__
