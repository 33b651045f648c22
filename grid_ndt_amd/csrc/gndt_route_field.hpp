// gndt_route_field.hpp — the route field (include/gndt.h "route field"): for every slope the least cost to reach any of a set of goals
// along the clearance field's steps, never entering a slope the caller's hops forbid, and the slope to step to next; and the routes K
// starts get by following `next`.
//   k_route_enter     row -> its weight w (0: may not be entered, else the factor on the cost of a step INTO it) and the empty key
//   k_route_goals     goal -> accepted (a 64-bit minimum on its row's key: the seed) or ignored, counted
//   k_route_steps     (row, side) -> the side's first step that may be taken with its cost, the rest of its steps, the "more" bits
//   k_route_sweep     one sweep over all rows, keys relaxed IN PLACE (one launch = one sweep)                        8 + 4 x (8 + 8) B a slope
//   k_route_wg        every sweep in one launch, one workgroup, the keys in LDS (maps of up to kRouteLdsRows rows)
//   k_route_finish    keys -> cost, next; the call's counts
//   k_route_descend   one lane a start: the start's row through the queries' lookup, then the chain of `next`
// key = bits(cost) << 32 | next row, kRouteNoKey while no walk is known: costs are non-negative floats, whose bits order as they do, so
// one unsigned minimum picks the least cost and, among the steps that give it, the smallest row.  The field is the fixed point of
// key(q) = min(seed(q), min over steps t of q that may be entered of cand(key(t), c(q, t), t)); fl(c + a) is monotone in a, so a key
// only ever falls, every value a row reads of another row is an upper bound of that row's final key, and any order of relaxations
// ends at the same keys.  In place therefore: a row's key has ONE writer (the quad's first lane, or the row's thread in the
// one-workgroup kernel), which stores it whole (8 aligned bytes); readers see the old key or the new, both bounds.
// The per-row logic is host-callable so that the CPU test tier runs the kernels' own code one row after another
// (tests/route_field_shim.cpp); memory operations go through an Ops policy.
#pragma once
#include <float.h>
#include <stdint.h>

#include "gndt_clearance.hpp"
#include "gndt_walk.hpp"

namespace gndt {

constexpr unsigned long long kRouteNoKey = ~0ull;
constexpr uint32_t kRouteCheckOverhead = 1u;              // GNDT_WALK_CHECK_OVERHEAD
constexpr uint32_t kRouteDefaultRounds = 1024u, kRouteMaxRounds = 4096u;
constexpr uint32_t kRouteMaxGoals = 1u << 20;
constexpr uint32_t kRouteLdsRows = 20448u;               // k_route_wg's limit, 144 x 142: one key array of 8 B a row, 159.75 of the CU's 160 KiB
constexpr uint32_t kRouteFltMaxBits = 0x7F7FFFFFu;
constexpr int kRouteFound = 0, kRouteNoStart = 1, kRouteNoRoute = 2, kRouteLimit = 3;      // GNDT_ROUTE_*

struct RouteRule {               // gndt_route_field_params with its defaults resolved
    uint32_t checks, min_hops, soft_hops;
    float soft_weight, max_cost;
    uint32_t max_rounds;
};

// a side's first step that may be taken: the row stepped to (kNoRow: none among the column's first kStepRows rows) and the step's cost
struct RouteFirst {
    uint32_t t, d_bits;
};

struct RouteInfo {               // gndt_route_info
    int32_t status;
    uint32_t length, start_row, expansions, queue_peak;
    float cost, h_start;
    uint32_t reserved;
};

struct DescendRule {             // gndt_descend_params with its defaults resolved
    int start_mode;              // kQueryNode / kQueryNearestSlope
    uint32_t max_steps;
};

// w(row): 0 for a row that may not be entered (no slope, fewer than min_hops hops, something overhead), else the factor on the cost
// of a step into it: 1, or 1 + soft_weight * (soft_hops - hops) inside the soft zone
GNDT_HD float route_weight(const CostView& V, const Robot& R, const RouteRule& F, const uint32_t* hops, uint32_t row) {
    GNDT_FP_STRICT
    if (!row_has_slope(V, row)) return 0.f;
    const uint32_t hp = hops ? hops[row] : kClrBeyond;
    if (hp < F.min_hops) return 0.f;
    if ((F.checks & kRouteCheckOverhead) && row_above_hits_in(V, R, row, clearance_own_column(V, row))) return 0.f;
    if (hp >= F.soft_hops) return 1.f;
    const float pen = F.soft_weight * (float)(F.soft_hops - hp);
    return 1.0f + pen;
}

// c(q, t) = fl(TravelCost(mean q, mean t) * w(t))
GNDT_HD float route_step_cost(const CostView& V, uint32_t q, uint32_t t, float wt) {
    GNDT_FP_STRICT
    const float d = cost_travel(V.mean + 3 * (size_t)q, V.mean + 3 * (size_t)t);
    return d * wt;
}

// The seed of a goal: its cost's bits above GNDT_NO_ROW; kRouteNoKey for a goal that is ignored (a row out of range or without a slope
// or that may not be entered, a cost that is not finite or is negative).  -0 counts as 0.
GNDT_HD unsigned long long route_seed(uint32_t n, const float* w, uint32_t row, float gc) {
    if (row >= n || w[row] == 0.f) return kRouteNoKey;
    if (!(gc >= 0.f) || !(gc <= FLT_MAX)) return kRouteNoKey;
    return ((unsigned long long)float_bits(gc == 0.f ? 0.f : gc) << 32) | kNoRow;
}

// What the step to t at cost d offers, given t's key: kRouteNoKey if t has none, if the sum is not below FLT_MAX, or above max_cost
GNDT_HD unsigned long long route_cand(unsigned long long key_t, float d, uint32_t t, float max_cost) {
    GNDT_FP_STRICT
    if (key_t == kRouteNoKey) return kRouteNoKey;
    const float s = d + bits_float((uint32_t)(key_t >> 32));
    if (!(s < FLT_MAX) || (max_cost > 0.f && s > max_cost)) return kRouteNoKey;
    return ((unsigned long long)float_bits(s) << 32) | t;
}

// One side of a slope for the sweeps.  st: clearance_side's answer (the steps the gates allow); first: the first of them that may be
// entered, priced; rest: the others that may be entered, as a mask behind the same column.  -> does a sweep have to look past
// `first` (more steps in the mask, or a column taller than the mask)?
GNDT_HD bool route_side(const CostView& V, uint32_t row, const ClearanceStep& st, bool tall, const float* w, RouteFirst& first, ClearanceStep& rest) {
    first.t = kNoRow; first.d_bits = 0u;
    rest.c = st.c; rest.mask = 0u;
    if (st.c == kNoColumn) return false;
    uint32_t mask = 0u;
    for (uint32_t m = st.mask; m; m &= m - 1u) {
        const uint32_t j = (uint32_t)__builtin_ctz(m);
        if (w[st.c + j] != 0.f) mask |= 1u << j;
    }
    if (mask) {
        first.t = st.c + (uint32_t)__builtin_ctz(mask);
        first.d_bits = float_bits(route_step_cost(V, row, first.t, w[first.t]));
        rest.mask = mask & (mask - 1u);
    }
    return rest.mask != 0u || tall;
}

// One thread after another (the CPU tier)
struct RouteSerialOps {
    static inline unsigned long long load_key(const unsigned long long* p) { return *p; }
    static inline void store_key(unsigned long long* p, unsigned long long v) { *p = v; }
    static inline void min_key(unsigned long long* p, unsigned long long v) { if (v < *p) *p = v; }
    static inline void add_u32(uint32_t* p, uint32_t v) { *p += v; }
    static inline void max_u32(uint32_t* p, uint32_t v) { if (v > *p) *p = v; }
};

// the steps of a side behind its first: the rest of the mask, and the rows of a tall column beyond it through the gates again
template <class Ops>
GNDT_HD unsigned long long route_sweep_rest(const CostView& V, const Robot& R, float max_cost, uint32_t row, const ClearanceStep& rest, bool tall,
                                            const float* w, const unsigned long long* key) {
    unsigned long long best = kRouteNoKey;
    for (uint32_t m = rest.mask; m; m &= m - 1u) {
        const uint32_t t = rest.c + (uint32_t)__builtin_ctz(m);
        const unsigned long long c = route_cand(Ops::load_key(key + t), route_step_cost(V, row, t, w[t]), t, max_cost);
        best = c < best ? c : best;
    }
    if (tall) {
        const uint32_t ncol = V.row_ncol[rest.c];
        const float* nq = V.normal + 3 * (size_t)row;
        const float* mq = V.mean + 3 * (size_t)row;
        for (uint32_t j = kStepRows; j < ncol; ++j) {
            const uint32_t t = rest.c + j;
            if (!(V.flags[t] & 2u) || w[t] == 0.f || !cost_gates(V, R, t, nq, mq)) continue;
            const unsigned long long c = route_cand(Ops::load_key(key + t), route_step_cost(V, row, t, w[t]), t, max_cost);
            best = c < best ? c : best;
        }
    }
    return best;
}

// One sweep, one side: the least candidate among the steps of `row` through it (kRouteNoKey: none)
template <class Ops>
GNDT_HD unsigned long long route_sweep_side(const CostView& V, const Robot& R, float max_cost, uint32_t row, const RouteFirst& first,
                                            const ClearanceStep& rest, uint32_t more, const float* w, const unsigned long long* key) {
    unsigned long long best = kRouteNoKey;
    if (first.t != kNoRow) best = route_cand(Ops::load_key(key + first.t), bits_float(first.d_bits), first.t, max_cost);
    if (more & 1u) {
        const unsigned long long m = route_sweep_rest<Ops>(V, R, max_cost, row, rest, (more & 16u) != 0u, w, key);
        best = m < best ? m : best;
    }
    return best;
}

// One sweep, all four sides of a row in one thread: the first step's key of every side is asked for before any is looked at
// (clearance_round_row's order: one wait instead of four).  more: bit k side k has steps behind its first, bit 4 + k its column is tall.
template <class Ops>
GNDT_HD unsigned long long route_sweep_row(const CostView& V, const Robot& R, float max_cost, uint32_t row, const RouteFirst* first,
                                           const ClearanceStep* rest, uint32_t more, const float* w, const unsigned long long* key) {
    unsigned long long kt[4];
    for (uint32_t k = 0; k < 4u; ++k) kt[k] = first[k].t != kNoRow ? Ops::load_key(key + first[k].t) : kRouteNoKey;
    unsigned long long least = kRouteNoKey;
    for (uint32_t k = 0; k < 4u; ++k) {
        const unsigned long long c = route_cand(kt[k], bits_float(first[k].d_bits), first[k].t, max_cost);
        least = c < least ? c : least;
        if ((more >> k) & 1u) {
            const unsigned long long m = route_sweep_rest<Ops>(V, R, max_cost, row, rest[k], ((more >> (4u + k)) & 1u) != 0u, w, key);
            least = m < least ? m : least;
        }
    }
    return least;
}

// What a row's key says: cost and next, and what it adds to the counts
struct RouteTally {
    uint32_t finite, max_bits;
};
GNDT_HD void route_finish_row(unsigned long long key, uint32_t& cost_bits, uint32_t& next, RouteTally& t) {
    const bool ok = key != kRouteNoKey;
    cost_bits = ok ? (uint32_t)(key >> 32) : kRouteFltMaxBits;
    next = ok ? (uint32_t)key : kNoRow;
    if (ok) {
        t.finite += 1u;
        t.max_bits = cost_bits > t.max_bits ? cost_bits : t.max_bits;
    }
}
// counts[2] = slopes with a finite cost, counts[3] = the bits of the largest: an integer sum and a maximum, any order
template <class Ops>
GNDT_HD void route_fold(uint32_t* counts, const RouteTally& t) {
    if (t.finite) Ops::add_u32(counts + 2, t.finite);
    if (t.max_bits) Ops::max_u32(counts + 3, t.max_bits);
}

// One start: p its point, cost / next the field (n entries each, and nothing outside them is read), rows[route_cap] (or null with 0) the
// route, start first.  A `next` entry that is neither kNoRow nor a row ends the chain like the step guard does: GNDT_ROUTE_LIMIT, no
// route (length 0, every entry kNoRow).
GNDT_HD void route_descend(const QueryView& Q, const DescendRule& P, uint32_t n, const float* cost, const uint32_t* next, const float* p,
                           uint32_t* rows, uint32_t route_cap, RouteInfo& o) {
    o.status = kRouteNoStart; o.length = 0u; o.start_row = kNoRow; o.expansions = 0u; o.queue_peak = 0u;
    o.cost = FLT_MAX; o.h_start = FLT_MAX; o.reserved = 0u;
    uint32_t c;
    int cx, cy;
    uint32_t q = n == 0u ? kNoRow
               : P.start_mode == kQueryNode ? walk_start<kQueryNode>(Q, p[0], p[1], p[2], c, cx, cy)
                                            : walk_start<kQueryNearestSlope>(Q, p[0], p[1], p[2], c, cx, cy);
    uint32_t len = 0u;
    if (q != kNoRow && q < n) {
        o.start_row = q;
        const float hs = cost[q];
        o.status = kRouteNoRoute;
        if (float_bits(hs) != kRouteFltMaxBits) {
            o.cost = o.h_start = hs;
            o.status = kRouteFound;
            if (len < route_cap) rows[len] = q;
            ++len;
            for (;;) {
                const uint32_t nx = next[q];
                if (nx == kNoRow) break;
                if (nx >= n || o.expansions == P.max_steps) { o.status = kRouteLimit; break; }
                o.expansions += 1u;
                q = nx;
                if (len < route_cap) rows[len] = q;
                ++len;
            }
            if (o.status == kRouteLimit) {
                o.cost = FLT_MAX;
                len = 0u;
            }
        }
    }
    o.length = len;
    for (uint32_t i = len; i < route_cap; ++i) rows[i] = kNoRow;
}

// A call's scratch for a map of n rows (gndt_api_route_field.hip)
constexpr uint64_t kRouteFlagWords = kRouteMaxRounds + 8u;   // one word a sweep, kRouteMaxRounds + 1 of them, padded
struct RouteScratch {
    RouteFirst* first;               // [4 n] the first step of a side with its cost
    ClearanceStep* rest;             // [4 n] the rest of its steps
    unsigned long long* key;         // [n] relaxed in place by the sweeps
    uint32_t* flags;                 // [kRouteFlagWords]
    float* w;                        // [n] the weight of entering the row
    uint8_t* more;                   // [n] the "more" bits
    RouteScratch() = default;
    RouteScratch(Carver& c, uint64_t n)
        : first(c.take<RouteFirst>(4 * n)), rest(c.take<ClearanceStep>(4 * n)), key(c.take<unsigned long long>(n)),
          flags(c.take<uint32_t>(kRouteFlagWords)), w(c.take<float>(n)), more(c.take<uint8_t>(n)) {}
};

}  // namespace gndt

#if defined(__HIPCC__)
namespace gndt {

constexpr int kRouteWgThreads = 1024;
constexpr uint32_t kRouteLdsTail = 64u;                // bytes behind the keys: the sweeps' changed flags
constexpr uint32_t kRouteWgSlots = (kRouteLdsRows + kRouteWgThreads - 1) / kRouteWgThreads;

// the keys in global memory, relaxed in place: whole 8-byte loads and stores that the compiler neither splits, repeats nor keeps
struct RouteDeviceOps {
    static __device__ __forceinline__ unsigned long long load_key(const unsigned long long* p) {
        return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    static __device__ __forceinline__ void store_key(unsigned long long* p, unsigned long long v) {
        __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    static __device__ __forceinline__ void min_key(unsigned long long* p, unsigned long long v) { atomicMin(p, v); }
    static __device__ __forceinline__ void add_u32(uint32_t* p, uint32_t v) { atomicAdd(p, v); }
    static __device__ __forceinline__ void max_u32(uint32_t* p, uint32_t v) { atomicMax(p, v); }
};
// the keys in LDS (k_route_wg)
struct RouteLdsOps : RouteDeviceOps {
    static __device__ __forceinline__ unsigned long long load_key(const unsigned long long* p) {
        return *(const volatile __attribute__((address_space(3))) unsigned long long*)p;
    }
    static __device__ __forceinline__ void store_key(unsigned long long* p, unsigned long long v) {
        *(volatile __attribute__((address_space(3))) unsigned long long*)p = v;
    }
};

// One thread a row: its weight, and the key no walk has reached
static __global__ void __launch_bounds__(256) k_route_enter(CostView V, Robot R, RouteRule F, uint32_t n, const uint32_t* __restrict__ hops,
                                                            float* __restrict__ w, unsigned long long* __restrict__ key) {
    const uint64_t gsz = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t row = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; row < n; row += gsz) {
        w[row] = route_weight(V, R, F, hops, (uint32_t)row);
        key[row] = kRouteNoKey;
    }
}

// One thread a goal.  counts[0] / counts[1]: accepted / ignored, a wave's tally in one lane's atomics.
static __global__ void __launch_bounds__(256) k_route_goals(uint32_t n, const float* __restrict__ w, const uint32_t* __restrict__ goals,
                                                            const float* __restrict__ goal_cost, uint32_t G, unsigned long long* __restrict__ key,
                                                            uint32_t* __restrict__ counts) {
    const uint32_t gsz = gridDim.x * blockDim.x;
    uint32_t ok = 0u, bad = 0u;
    for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < G; g += gsz) {
        const uint32_t row = goals[g];
        const unsigned long long seed = route_seed(n, w, row, goal_cost ? goal_cost[g] : 0.f);
        if (seed == kRouteNoKey) { ++bad; continue; }
        ++ok;
        RouteDeviceOps::min_key(key + row, seed);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ok += (uint32_t)__shfl_xor((int)ok, o, 64);
        bad += (uint32_t)__shfl_xor((int)bad, o, 64);
    }
    if ((threadIdx.x & 63u) == 0u) {
        if (ok) atomicAdd(counts, ok);
        if (bad) atomicAdd(counts + 1, bad);
    }
}

// Four lanes a row, one per side (k_clearance_steps' spread): first[4 row + k], rest[4 row + k], more[row].  flag0: the sweeps' flag
// word 0, set here so that sweep 1 runs.
static __global__ void __launch_bounds__(256) k_route_steps(CostView V, Robot R, uint32_t n, const float* __restrict__ w, RouteFirst* __restrict__ first,
                                                            ClearanceStep* __restrict__ rest, uint8_t* __restrict__ more, uint32_t* __restrict__ flag0) {
    const uint64_t total = 4ull * n, gsz = (uint64_t)gridDim.x * blockDim.x;
    if (blockIdx.x == 0 && threadIdx.x == 0) *flag0 = 1u;
    for (uint64_t t0 = (uint64_t)blockIdx.x * blockDim.x; t0 < total; t0 += gsz) {      // (uniform: the quad exchanges below)
        const uint64_t t = t0 + threadIdx.x;
        const bool live = t < total;
        const uint32_t row = live ? (uint32_t)(t >> 2) : 0u, k = (uint32_t)t & 3u;
        const bool slope = live && row_has_slope(V, row);
        ClearanceStep st{kNoColumn, 0u}, rs{kNoColumn, 0u};
        RouteFirst f{kNoRow, 0u};
        uint32_t mb = 0u;
        if (slope) {
            const bool tall = (clearance_side(V, R, row, k, st) & kClrSideTall) != 0u;
            if (route_side(V, row, st, tall, w, f, rs)) mb |= 1u << k;
            if (tall) mb |= 16u << k;
        }
        if (live) {
            reinterpret_cast<uint2*>(first)[t] = make_uint2(f.t, f.d_bits);
            reinterpret_cast<uint2*>(rest)[t] = make_uint2(rs.c, rs.mask);
        }
        mb |= (uint32_t)__shfl_xor((int)mb, 1, 64);
        mb |= (uint32_t)__shfl_xor((int)mb, 2, 64);
        if (live && k == 0u) more[row] = (uint8_t)mb;
    }
}

// Sweep `round` over every row, in place.  flags[round - 1]: did the sweep before change anything (flags[0] is set by k_route_steps)?
// If not, the keys are the fixed point: nothing to do, here and in every later sweep.
static __global__ void __launch_bounds__(256) k_route_sweep(CostView V, Robot R, float max_cost, uint32_t n, uint32_t round,
                                                            const RouteFirst* __restrict__ first, const ClearanceStep* __restrict__ rest,
                                                            const uint8_t* __restrict__ more, const float* __restrict__ w, unsigned long long* key,
                                                            uint32_t* __restrict__ flags) {
    if (flags[round - 1u] == 0u) return;
    const uint64_t total = 4ull * n, gsz = (uint64_t)gridDim.x * blockDim.x;
    bool changed = false;
    for (uint64_t t0 = (uint64_t)blockIdx.x * blockDim.x; t0 < total; t0 += gsz) {      // (uniform: the quad exchanges)
        const uint64_t t = t0 + threadIdx.x;
        const bool live = t < total;
        const uint32_t row = live ? (uint32_t)(t >> 2) : 0u, k = (uint32_t)t & 3u;
        unsigned long long least = kRouteNoKey;
        if (live && row_has_slope(V, row)) {
            const uint2 e = reinterpret_cast<const uint2*>(first)[t];
            const uint32_t mb = more[row];
            ClearanceStep rs{kNoColumn, 0u};
            if ((mb >> k) & 1u) {
                const uint2 r = reinterpret_cast<const uint2*>(rest)[t];
                rs = ClearanceStep{r.x, r.y};
            }
            least = route_sweep_side<RouteDeviceOps>(V, R, max_cost, row, RouteFirst{e.x, e.y}, rs, ((mb >> k) & 1u) | (((mb >> (4u + k)) & 1u) << 4), w, key);
        }
        least = clearance_quad_min(least);
        if (live && k == 0u && least != kRouteNoKey && least < RouteDeviceOps::load_key(key + row)) {
            RouteDeviceOps::store_key(key + row, least);
            changed = true;
        }
    }
    if (__any(changed) && (threadIdx.x & 63u) == 0u) flags[round] = 1u;
}

// a wave's tally -> the counts: combined over the wave first, one lane's atomics
__device__ __forceinline__ void route_flush(RouteTally t, uint32_t* __restrict__ counts) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        t.finite += (uint32_t)__shfl_xor((int)t.finite, o, 64);
        t.max_bits = max(t.max_bits, (uint32_t)__shfl_xor((int)t.max_bits, o, 64));
    }
    if ((threadIdx.x & 63u) == 0u) route_fold<RouteDeviceOps>(counts, t);
}

// counts[0..1] are the goals pass's; a workgroup's waves add up in LDS first (k_clearance_finish's reason).  Workgroup 0 also reads the
// sweeps' flags: counts[4] = 1 if the last sweep the call could launch found nothing to change (or an earlier one did: the flags
// behind it were never set), counts[5] = the sweeps that changed something.
constexpr int kRouteFinishBlocks = 512;
static __global__ void __launch_bounds__(256) k_route_finish(const unsigned long long* __restrict__ key, uint32_t n, uint32_t max_rounds,
                                                             const uint32_t* __restrict__ flags, float* __restrict__ cost, uint32_t* __restrict__ next,
                                                             uint32_t* __restrict__ counts) {
    __shared__ uint32_t s_counts[4];
    if (threadIdx.x < 4u) s_counts[threadIdx.x] = 0u;
    __syncthreads();
    const uint64_t gsz = (uint64_t)gridDim.x * blockDim.x;
    RouteTally t{0u, 0u};
    for (uint64_t row = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; row < n; row += gsz) {
        uint32_t cb, nx;
        route_finish_row(key[row], cb, nx, t);
        if (cost) cost[row] = bits_float(cb);
        if (next) next[row] = nx;
    }
    route_flush(t, s_counts);
    if (blockIdx.x == 0u) {
        uint32_t worked = 0u;
        for (uint32_t r = 1u + threadIdx.x; r <= max_rounds; r += blockDim.x) worked += flags[r] != 0u ? 1u : 0u;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) worked += (uint32_t)__shfl_xor((int)worked, o, 64);
        if ((threadIdx.x & 63u) == 0u && worked) atomicAdd(s_counts, worked);
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
        route_fold<RouteDeviceOps>(counts, RouteTally{s_counts[2], s_counts[3]});
        if (blockIdx.x == 0u) {
            counts[4] = flags[max_rounds] == 0u ? 1u : 0u;
            counts[5] = s_counts[0];
        }
    }
}

// Every sweep in one launch: one workgroup, the keys in LDS (n <= kRouteLdsRows), relaxed in place, a workgroup barrier between
// sweeps, out at the first sweep that changes nothing or after max_rounds; then the finish.  One thread a row, a thread's rows (tid,
// tid + 1024, ...) in fixed slots.  Dynamic LDS: the keys [n], then three flag words.
static __global__ void __launch_bounds__(kRouteWgThreads) k_route_wg(CostView V, Robot R, float max_cost, uint32_t n, uint32_t max_rounds,
                                                                     const RouteFirst* __restrict__ first, const ClearanceStep* __restrict__ rest,
                                                                     const uint8_t* __restrict__ more, const float* __restrict__ w,
                                                                     const unsigned long long* __restrict__ key0, float* __restrict__ cost,
                                                                     uint32_t* __restrict__ next, uint32_t* __restrict__ counts) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long s_rkey[];         // [n], then the flags
    uint32_t* const s_flag = reinterpret_cast<uint32_t*>(s_rkey + n);
    uint32_t slopes = 0u;                               // bit j: slot j's row has a slope
    for (uint32_t j = 0; j < kRouteWgSlots; ++j) {
        const uint32_t row = threadIdx.x + j * kRouteWgThreads;
        if (row >= n) break;
        RouteLdsOps::store_key(s_rkey + row, key0[row]);
        if (row_has_slope(V, row)) slopes |= 1u << j;
    }
    if (threadIdx.x < 3u) s_flag[threadIdx.x] = 0u;
    __syncthreads();
    uint32_t worked = 0u, converged = 0u;
    for (uint32_t round = 1u; round <= max_rounds; ++round) {
        if (threadIdx.x == 0u) s_flag[(round + 1u) % 3u] = 0u;      // (the next sweep's; nobody looks at it during this one)
        bool changed = false;
        // (Asking for the steps of four of the thread's rows before looking at the first was measured equal, 3.12 against 3.00 ms on the
        //  site: with 17 rows a thread the sweep is bound by the one CU's instruction rate, not by its round trips to L2.)
        for (uint32_t bits = slopes; bits; bits &= bits - 1u) {
            const uint32_t row = threadIdx.x + ((uint32_t)__ffs((int)bits) - 1u) * kRouteWgThreads;
            const uint4 a = reinterpret_cast<const uint4*>(first)[2 * (size_t)row], b = reinterpret_cast<const uint4*>(first)[2 * (size_t)row + 1];
            const RouteFirst f[4] = {{a.x, a.y}, {a.z, a.w}, {b.x, b.y}, {b.z, b.w}};
            const uint32_t mb = more[row];
            ClearanceStep rs[4] = {{kNoColumn, 0u}, {kNoColumn, 0u}, {kNoColumn, 0u}, {kNoColumn, 0u}};
            if (mb & 15u) {
                const uint4 c = reinterpret_cast<const uint4*>(rest)[2 * (size_t)row], d = reinterpret_cast<const uint4*>(rest)[2 * (size_t)row + 1];
                rs[0] = ClearanceStep{c.x, c.y}; rs[1] = ClearanceStep{c.z, c.w}; rs[2] = ClearanceStep{d.x, d.y}; rs[3] = ClearanceStep{d.z, d.w};
            }
            const unsigned long long least = route_sweep_row<RouteLdsOps>(V, R, max_cost, row, f, rs, mb, w, s_rkey);
            if (least != kRouteNoKey && least < RouteLdsOps::load_key(s_rkey + row)) {
                RouteLdsOps::store_key(s_rkey + row, least);
                changed = true;
            }
        }
        if (__any(changed) && (threadIdx.x & 63u) == 0u) s_flag[round % 3u] = 1u;
        __syncthreads();
        if (s_flag[round % 3u] == 0u) { converged = 1u; break; }    // (uniform: one word, read behind the barrier)
        ++worked;
    }
    RouteTally tl{0u, 0u};
    for (uint32_t row = threadIdx.x; row < n; row += kRouteWgThreads) {
        uint32_t cb, nx;
        route_finish_row(RouteLdsOps::load_key(s_rkey + row), cb, nx, tl);
        if (cost) cost[row] = bits_float(cb);
        if (next) next[row] = nx;
    }
    route_flush(tl, counts);
    if (threadIdx.x == 0u) { counts[4] = converged; counts[5] = worked; }
}

// One start a lane, one wavefront a workgroup (k_walk_paths' reasons: a chain of dependent loads per start, nothing shared).  info: two
// 16-byte stores a start.
constexpr int kRouteDescendThreads = 64;
static __global__ void __launch_bounds__(kRouteDescendThreads) k_route_descend(QueryView Q, DescendRule P, uint32_t n, const float* __restrict__ cost,
                                                                               const uint32_t* __restrict__ next, const float* __restrict__ starts,
                                                                               uint32_t sf, uint64_t K, uint32_t* __restrict__ rows, uint32_t route_cap,
                                                                               RouteInfo* __restrict__ info) {
    const uint64_t gsz = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < K; p += gsz) {
        RouteInfo o;
        route_descend(Q, P, n, cost, next, starts + p * sf, rows ? rows + p * route_cap : nullptr, route_cap, o);
        uint4* out = reinterpret_cast<uint4*>(info + p);
        out[0] = make_uint4((uint32_t)o.status, o.length, o.start_row, o.expansions);
        out[1] = make_uint4(o.queue_peak, float_bits(o.cost), float_bits(o.h_start), 0u);
    }
}

}  // namespace gndt
#endif  // __HIPCC__
