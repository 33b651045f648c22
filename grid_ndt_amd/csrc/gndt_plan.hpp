// gndt_plan.hpp — route planning on the device-resident grid (include/gndt.h "route planning"): AstarPlanar::findRoute
// (include/GlobalPlan.h:49-166) from a batch of starts to the goal of the last cost flood, one query per wavefront.
//
// What a query returns is what the reference's loop returns on a FRESH map whose Slope::h is the current cost map, quirks included:
//   - the open queue is a multimap on f with plain `<` (GlobalPlan.h:9-13): the front is the least (f, insertion order);
//   - isContaninedOpen (GlobalPlan.h:30-45) walks from the FRONT of the queue and stops at the first key that differs from the
//     candidate's current f: a slope that is open with any other key is not found, gets g, f and its father overwritten
//     unconditionally and a SECOND entry; nothing tests "closed" at the pop, so such an entry expands its slope again;
//   - neighbours come cell by cell (left, right, forward, back), ascending morton_z inside a cell (map_slope is a std::map).
//
// The queue.  Entries (f bits, row) live in ONE array in insertion order: positions [0, cap0) in LDS, [cap0, cap0 + cap1) in the
// query's spill area in global memory.  An erase leaves a tombstone; compaction is stable.  The array is therefore always in
// insertion order, and "(f, insertion order)" is "(f bits, position)": a pop is one lane-parallel pass for the least
// (f bits << 32 | position) and a shuffle reduction, the front-run test one pass for the first position that holds (front key, row).
// f is a sum of non-negative floats, never NaN, so its bit pattern orders like its value.
//
// Everything that decides a route is here and host-callable; the wave-cooperative steps go through a `W` policy — PlanWaveDevice
// (lanes, shuffles) for the kernel, PlanWaveHost (a loop over 64 lanes) for the CPU tier (tests/plan_shim.cpp).  Values that decide
// control flow are wave-uniform: every lane runs the same loop, lane 0 (W::leader) stores.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "gndt_math.hpp"
#include "gndt_cost.hpp"
#include "gndt_query.hpp"

namespace gndt {

constexpr int kRouteFound = 0, kRouteNoStart = 1, kRouteNoRoute = 2, kRouteLimit = 3, kRouteNoGoal = 4;   // GNDT_ROUTE_*
constexpr uint32_t kPlanLanes = 64;
constexpr uint32_t kPlanLdsEntries = 1024;       // the LDS tier of a query's queue: 8 KB a wavefront (the measured peaks are ~500)
constexpr uint32_t kPlanDeadBits = 0xFFFFFFFFu;  // f of a tombstone: above every float's bit pattern

struct RouteInfo {           // gndt_route_info
    int32_t status;
    uint32_t length, start_row, expansions, queue_peak;
    float cost, h_start;
    uint32_t reserved;
};

// Per query and row: g, f, the father's row, and (stamp << 1 | closed).  A row whose stamp is not the launch's has not been touched by
// this query: g = f = FLT_MAX, no father, open (what create2DMap leaves, map2D.h:637) — nothing is cleared between queries.
struct alignas(16) PlanRowState {
    uint32_t g, f, father, mark;
};

struct PlanView {
    CostView V;              // rows, column index, and the flood's kept tables: nbr / self / edges (self may be null: the index is probed)
    Robot R;
    const uint32_t* h_bits;  // the cost map
    uint32_t goal_row, num_rows;
};

// the guard's default and the entries a query's queue can hold (both tiers together), from the map's slope count
GNDT_HD uint32_t plan_default_expansions(uint64_t num_slopes) {
    const uint64_t v = 4ull * num_slopes + 1024ull;
    return v > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)v;
}
GNDT_HD uint32_t plan_queue_entries(uint64_t num_slopes) {
    const uint64_t v = 2ull * num_slopes + 1024ull;
    return v > 0x7FFFFFFFull ? 0x7FFFFFFFu : (uint32_t)v;
}

struct PlanWaveHost {
    template <typename F> static uint64_t min_u64(F f) {
        uint64_t m = ~0ull;
        for (uint32_t l = 0; l < kPlanLanes; ++l) { const uint64_t v = f(l); m = v < m ? v : m; }
        return m;
    }
    template <typename F> static uint32_t sum_u32(F f) {
        uint32_t s = 0;
        for (uint32_t l = 0; l < kPlanLanes; ++l) s += f(l);
        return s;
    }
    template <typename F> static void each(F f) { for (uint32_t l = 0; l < kPlanLanes; ++l) f(l); }
    static bool leader() { return true; }
    static void sync() {}
    static void edges(const CostEdge* e, CostEdge out[4]) { for (int k = 0; k < 4; ++k) out[k] = e[k]; }
};

// ---- the queue ---------------------------------------------------------------------------------------------------------------
struct PlanQueue {
    uint32_t *f0, *r0;       // first tier: cap0 entries (the kernel: LDS)
    uint32_t *f1, *r1;       // spill tier: cap1 entries
    uint32_t cap0, cap1;
    uint32_t n, live;        // entries with tombstones, entries without
};
GNDT_HD uint32_t plan_q_f(const PlanQueue& q, uint32_t i) { return i < q.cap0 ? q.f0[i] : q.f1[i - q.cap0]; }
GNDT_HD uint32_t plan_q_row(const PlanQueue& q, uint32_t i) { return i < q.cap0 ? q.r0[i] : q.r1[i - q.cap0]; }
GNDT_HD void plan_q_set(const PlanQueue& q, uint32_t i, uint32_t f, uint32_t row) {
    if (i < q.cap0) { q.f0[i] = f; q.r0[i] = row; } else { q.f1[i - q.cap0] = f; q.r1[i - q.cap0] = row; }
}

// the front: (f bits << 32 | position) of the least (f, insertion order); f bits == kPlanDeadBits: the queue is empty
template <typename W>
GNDT_HD uint64_t plan_queue_front(const PlanQueue& q) {
    W::sync();
    return W::min_u64([&](uint32_t lane) {
        uint64_t m = ~0ull;
        for (uint32_t i = lane; i < q.n; i += kPlanLanes) {
            const uint64_t k = ((uint64_t)plan_q_f(q, i) << 32) | i;
            m = k < m ? k : m;
        }
        return m;
    });
}

// isContaninedOpen's walk for a slope whose f equals the front key: the first entry of the front run that holds `row` (kNoRow: none)
template <typename W>
GNDT_HD uint32_t plan_queue_find_in_front_run(const PlanQueue& q, uint32_t front_bits, uint32_t row) {
    W::sync();
    const uint64_t m = W::min_u64([&](uint32_t lane) {
        uint64_t best = ~0ull;
        for (uint32_t i = lane; i < q.n; i += kPlanLanes)
            if (plan_q_f(q, i) == front_bits && plan_q_row(q, i) == row && (uint64_t)i < best) best = i;
        return best;
    });
    return m == ~0ull ? kNoRow : (uint32_t)m;
}

// Stable compaction (tombstones leave, order stays); `track`: a live position to follow.  The moves are the leader's: a compaction
// of n entries follows at least n / 2 erases, two moves per pop on average.
template <typename W>
GNDT_HD void plan_queue_compact(PlanQueue& q, uint32_t& track) {
    W::sync();
    const uint32_t before = W::sum_u32([&](uint32_t lane) {
        uint32_t c = 0;
        for (uint32_t i = lane; i < q.n && i < track; i += kPlanLanes) c += plan_q_row(q, i) != kNoRow ? 1u : 0u;
        return c;
    });
    if (W::leader()) {
        uint32_t o = 0;
        for (uint32_t i = 0; i < q.n; ++i) {
            const uint32_t r = plan_q_row(q, i);
            if (r == kNoRow) continue;
            if (o != i) plan_q_set(q, o, plan_q_f(q, i), r);
            ++o;
        }
    }
    if (track != kNoRow) track = before;
    q.n = q.live;
}

GNDT_HD void plan_queue_erase(PlanQueue& q, uint32_t i, bool leader) {
    if (leader) plan_q_set(q, i, kPlanDeadBits, kNoRow);
    --q.live;
}

// std::multimap::insert: behind every entry of an equal key.  false: both tiers are full of live entries.
template <typename W>
GNDT_HD bool plan_queue_push(PlanQueue& q, uint32_t f_bits, uint32_t row, uint32_t& track) {
    if (q.n == q.cap0 + q.cap1) {
        if (q.live == q.n) return false;
        plan_queue_compact<W>(q, track);
    }
    if (W::leader()) plan_q_set(q, q.n, f_bits, row);
    ++q.n; ++q.live;
    return true;
}

// ---- the start ---------------------------------------------------------------------------------------------------------------
// gndt_query's rule for the point (query_points' steps for one query): the row, or kNoRow
template <int MODE>
GNDT_HD uint32_t plan_start_row(const QueryView& Q, float px, float py, float pz) {
    const QueryKey k = query_key<MODE>(Q, px, py, pz);
    const uint32_t slot = query_slot(Q, k);
    const uint32_t c = query_column(Q, k, Q.V.ctab_key[slot], Q.V.ctab_val[slot]);
    const uint32_t ncol = c != kNoColumn ? Q.V.row_ncol[c] : 0u;
    QueryBest b;
    b.row = kNoRow; b.d = 0.f; b.sz = 0;
    query_chunk<MODE>(Q, c, ncol, 0u, k, pz, b);
    query_rest<MODE>(Q, c, ncol, k, pz, b);
    return b.row;
}

// ---- the arithmetic ----------------------------------------------------------------------------------------------------------
// temp->g + TravelCost(temp->mean, s->mean) and s->g + s->h (GlobalPlan.h:120-135): fp32 additions, never contracted
GNDT_HD float plan_add(float a, float b) {
    GNDT_FP_STRICT
    return a + b;
}

// Diagnostic build (GNDT_EXTRA_CXXFLAGS=-DGNDT_PLAN_STAMPS for build_native; the call then waits and prints to stderr): where a wavefront's cycles go, summed over the queries of the
// process in g_plan_stamps — the pop's scan, temp's state and records, the neighbours' h and state, the relaxations (front-run test,
// stores, pushes), closing temp and compaction, the father walk; then the expansions and the queries counted.
#if defined(GNDT_PLAN_STAMPS) && defined(__HIP_DEVICE_COMPILE__)
static __device__ unsigned long long g_plan_stamps[8];
#define GNDT_PLAN_STAMP(k) do { const unsigned long long now_ = clock64(); ph_[k] += now_ - last_; last_ = now_; } while (0)
#define GNDT_PLAN_STAMPS_BEGIN unsigned long long ph_[6] = {0, 0, 0, 0, 0, 0}, last_ = clock64();
#define GNDT_PLAN_STAMPS_END(expansions) do { if (leader) { for (int k_ = 0; k_ < 6; ++k_) atomicAdd(&g_plan_stamps[k_], ph_[k_]); \
    atomicAdd(&g_plan_stamps[6], (unsigned long long)(expansions)); atomicAdd(&g_plan_stamps[7], 1ull); } } while (0)
#else
#if defined(GNDT_PLAN_STAMPS) && defined(__HIPCC__)
static __device__ unsigned long long g_plan_stamps[8];
#endif
#define GNDT_PLAN_STAMP(k) do { } while (0)
#define GNDT_PLAN_STAMPS_BEGIN
#define GNDT_PLAN_STAMPS_END(expansions) do { } while (0)
#endif

// ---- one query ---------------------------------------------------------------------------------------------------------------
// start_row: plan_start_row's answer.  st: the query's per-row state (num_rows entries; stamp: see PlanRowState).  q: an empty queue.
// route: route_cap rows (null with route_cap 0).  tally (optional, the CPU tier's two counters): pops of a slope that was already closed;
// entries that went into the queue below the key of the slope being expanded.
template <typename W>
GNDT_HD void plan_query(const PlanView& P, uint32_t start_row, PlanRowState* st, uint32_t stamp, PlanQueue& q, uint32_t max_expansions,
                        uint32_t* route, uint32_t route_cap, RouteInfo& info, uint32_t* tally = nullptr) {
    const CostView& V = P.V;
    const bool leader = W::leader();
    info.status = kRouteNoStart; info.length = 0u; info.start_row = kNoRow; info.expansions = 0u; info.queue_peak = 0u;
    info.cost = FLT_MAX; info.h_start = FLT_MAX; info.reserved = 0u;
    uint32_t length = 0u;
    q.n = 0u; q.live = 0u;
    GNDT_PLAN_STAMPS_BEGIN
    if (start_row != kNoRow && start_row < P.num_rows && row_has_slope(V, start_row)) {
        info.start_row = start_row;
        const uint32_t hs = P.h_bits[start_row];
        info.h_start = bits_float(hs);
        uint32_t none = kNoRow;
        {   // first->g = 0; first->f = first->g + first->h; open_queue.insert (GlobalPlan.h:66-68)
            PlanRowState s0;
            s0.g = 0u; s0.f = float_bits(plan_add(0.f, bits_float(hs))); s0.father = kNoRow; s0.mark = stamp << 1;
            if (leader) st[start_row] = s0;
            (void)plan_queue_push<W>(q, s0.f, start_row, none);
            info.queue_peak = 1u;
        }
        for (;;) {
            if (q.live == 0u) { info.status = kRouteNoRoute; break; }
            const uint64_t front = plan_queue_front<W>(q);
            const uint32_t front_bits = (uint32_t)(front >> 32);
            uint32_t at = (uint32_t)front;                       // temp's entry: it stays in the queue while temp is expanded
            const uint32_t temp = plan_q_row(q, at);
            GNDT_PLAN_STAMP(0);
            if (temp == P.goal_row) { info.status = kRouteFound; break; }
            if (info.expansions >= max_expansions) { info.status = kRouteLimit; break; }
            ++info.expansions;
            // everything that only needs temp, requested together: its state and the four records (one 64-byte access)
            PlanRowState ts = st[temp];
            CostEdge e[4];
            W::edges(V.edges + 4 * (size_t)temp, e);
            if (tally && (ts.mark & 1u)) ++tally[0];
            const float g_temp = bits_float(ts.g);
            GNDT_PLAN_STAMP(1);
            bool full = false;
            // The queue's least key while temp is expanded: temp's own, until a neighbour goes in below it (h is a flood's label, not a
            // consistent heuristic: f may fall along an edge).  isContaninedOpen walks from THAT entry, so it is that key a neighbour's f
            // has to equal.  (An erase here takes an entry of the least key only to put a smaller one in.)
            uint32_t lead_bits = front_bits;
            // GlobalPlan.h:104-137 for one accessible neighbour s at travel cost d, its h and state already read
            auto relax = [&](uint32_t s, float d, uint32_t h_s, PlanRowState ss) {
                if (full) return;
                if ((ss.mark >> 1) != stamp) { ss.g = 0x7F7FFFFFu; ss.f = 0x7F7FFFFFu; ss.father = kNoRow; ss.mark = stamp << 1; }
                if ((ss.mark & 1u) || h_s == 0x7F7FFFFFu) return;                    // isContainedClosed(s) || s->h == FLT_MAX
                if (V.demand_true && row_up(V, s)) return;                          // comand 4 evaluates countUp (map2D.h:281-284)
                uint32_t found = kNoRow;
                if (bits_float(ss.f) == bits_float(lead_bits)) found = plan_queue_find_in_front_run<W>(q, lead_bits, s);
                const float cand = plan_add(g_temp, d);
                if (found != kNoRow) {
                    if (!(bits_float(ss.g) > cand)) return;
                    plan_queue_erase(q, found, leader);
                }
                ss.g = float_bits(cand);
                ss.f = float_bits(plan_add(cand, bits_float(h_s)));
                ss.father = temp;
                if (leader) st[s] = ss;
                if (!plan_queue_push<W>(q, ss.f, s, at)) { full = true; return; }
                if (tally && ss.f < front_bits) ++tally[1];
                lead_bits = ss.f < lead_bits ? ss.f : lead_bits;
                info.queue_peak = q.live > info.queue_peak ? q.live : info.queue_peak;
            };
            // the neighbours the records name: rows, h and state of all of them read before any is looked at
            uint32_t t[4][2], hb[4][2];
            int tz[4][2];
            PlanRowState ns[4][2];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
            for (int k = 0; k < 4; ++k) {
                const uint32_t n = (e[k].info & kEdgeMore) || e[k].c == kNoColumn ? 0u : (e[k].info >> 16) & 3u;
                t[k][0] = n > 0u ? e[k].c + (e[k].info & 0xFFu) : kNoRow;
                t[k][1] = n > 1u ? e[k].c + ((e[k].info >> 8) & 0xFFu) : kNoRow;
                for (int j = 0; j < 2; ++j) {
                    hb[k][j] = 0x7F7FFFFFu; tz[k][j] = 0; ns[k][j] = PlanRowState{0u, 0u, 0u, 0u};
                    if (t[k][j] != kNoRow) { hb[k][j] = P.h_bits[t[k][j]]; ns[k][j] = st[t[k][j]]; tz[k][j] = V.sz[t[k][j]]; }
                }
            }
            GNDT_PLAN_STAMP(2);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
            for (int k = 0; k < 4; ++k) {
                if (e[k].c == kNoColumn) continue;
                if (!(e[k].info & kEdgeMore)) {
                    // ascending morton_z inside the cell (the records name rows in row order)
                    const bool swap = t[k][1] != kNoRow && tz[k][1] < tz[k][0];
                    const uint32_t ra = swap ? t[k][1] : t[k][0], rb = swap ? t[k][0] : t[k][1];
                    const uint32_t ha = swap ? hb[k][1] : hb[k][0], hb2 = swap ? hb[k][0] : hb[k][1];
                    const float da = swap ? e[k].d1 : e[k].d0, db = swap ? e[k].d0 : e[k].d1;
                    PlanRowState sa, sb;
                    sa.g = swap ? ns[k][1].g : ns[k][0].g; sa.f = swap ? ns[k][1].f : ns[k][0].f;
                    sa.father = swap ? ns[k][1].father : ns[k][0].father; sa.mark = swap ? ns[k][1].mark : ns[k][0].mark;
                    sb.g = swap ? ns[k][0].g : ns[k][1].g; sb.f = swap ? ns[k][0].f : ns[k][1].f;
                    sb.father = swap ? ns[k][0].father : ns[k][1].father; sb.mark = swap ? ns[k][0].mark : ns[k][1].mark;
                    if (ra != kNoRow) relax(ra, da, ha, sa);
                    if (rb != kNoRow) relax(rb, db, hb2, sb);
                } else {
                    // a cell the record could not hold: its slopes in ascending morton_z, the three gates against temp
                    uint32_t c, ncol;
                    neighbour_column(V, temp, (uint32_t)k, c, ncol);
                    bool any = false;
                    int last = 0;
                    for (;;) {
                        uint32_t pick = kNoRow;
                        int pz = 0;
                        for (uint32_t r = c; r < c + ncol; ++r) {
                            if (!row_has_slope(V, r)) continue;
                            const int z = V.sz[r];
                            if (any && z <= last) continue;
                            if (pick == kNoRow || z < pz) { pick = r; pz = z; }
                        }
                        if (pick == kNoRow) break;
                        any = true; last = pz;
                        if (!cost_gates(V, P.R, pick, V.normal + 3 * (size_t)temp, V.mean + 3 * (size_t)temp)) continue;
                        relax(pick, cost_travel(V.mean + 3 * (size_t)temp, V.mean + 3 * (size_t)pick), P.h_bits[pick], st[pick]);
                    }
                }
            }
            GNDT_PLAN_STAMP(3);
            if (full) { info.status = kRouteLimit; break; }          // (the queue's two tiers are full of live entries: see gndt.h)
            // closed_list.push_back(temp); open_queue.erase(it_open)
            ts.mark |= 1u;
            if (leader) st[temp] = ts;
            plan_queue_erase(q, at, leader);
            if (q.n >= 2u * kPlanLanes && q.n - q.live > q.live) { uint32_t none2 = kNoRow; plan_queue_compact<W>(q, none2); }
            GNDT_PLAN_STAMP(4);
        }
        (void)none;
    }
    // the father chain from the goal (GlobalPlan.h:150-157), written start first
    if (info.status == kRouteFound) {
        W::sync();
        info.cost = bits_float(st[P.goal_row].g);
        for (uint32_t r = P.goal_row; r != kNoRow && length <= P.num_rows; r = st[r].father) ++length;
        uint32_t at = length;
        for (uint32_t r = P.goal_row; r != kNoRow && at > 0u; r = st[r].father) {
            --at;
            if (leader && at < route_cap) route[at] = r;
        }
    }
    info.length = length;
    GNDT_PLAN_STAMP(5);
    GNDT_PLAN_STAMPS_END(info.expansions);
    const uint32_t filled = length < route_cap ? length : route_cap;
    W::each([&](uint32_t lane) { for (uint32_t i = filled + lane; i < route_cap; i += kPlanLanes) route[i] = kNoRow; });
}

#if defined(__HIPCC__)
struct PlanWaveDevice {
    template <typename F> static __device__ __forceinline__ uint64_t min_u64(F f) {
        unsigned long long v = f((uint32_t)(threadIdx.x & 63u));
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long w = __shfl_xor(v, o, 64);
            v = w < v ? w : v;
        }
        return v;
    }
    template <typename F> static __device__ __forceinline__ uint32_t sum_u32(F f) {
        uint32_t v = f((uint32_t)(threadIdx.x & 63u));
        for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
        return v;
    }
    template <typename F> static __device__ __forceinline__ void each(F f) { f((uint32_t)(threadIdx.x & 63u)); }
    static __device__ __forceinline__ bool leader() { return (threadIdx.x & 63u) == 0u; }
    // the workgroup is the wavefront: what the leader stored (LDS, or global memory through the CU's own cache) is what every lane
    // reads after this
    static __device__ __forceinline__ void sync() { __syncthreads(); }
    // lanes 0..3 read one 16-byte record each — the wave's one 64-byte access — and hand them round
    static __device__ __forceinline__ void edges(const CostEdge* e, CostEdge out[4]) {
        const uint4 mine = reinterpret_cast<const uint4*>(e)[threadIdx.x & 3u];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            out[k].c = (uint32_t)__shfl((int)mine.x, k, 64);
            out[k].info = (uint32_t)__shfl((int)mine.y, k, 64);
            out[k].d0 = bits_float((uint32_t)__shfl((int)mine.z, k, 64));
            out[k].d1 = bits_float((uint32_t)__shfl((int)mine.w, k, 64));
        }
    }
};

// One query per single-wavefront workgroup: query first + blockIdx.x in slot blockIdx.x of the scratch area
// (slot: num_rows PlanRowState, then the queue's spill tier: cap1 f words, cap1 row words).
template <int MODE>
static __global__ void __launch_bounds__(64) k_plan(PlanView P, QueryView Q, const float* __restrict__ starts, uint32_t sf, uint64_t first,
                                                   char* __restrict__ scratch, uint64_t slot_bytes, uint32_t cap0, uint32_t cap1, uint32_t stamp,
                                                   uint32_t max_expansions, uint32_t* __restrict__ route, uint32_t route_cap,
                                                   RouteInfo* __restrict__ info) {
    __shared__ uint32_t s_q[2 * kPlanLdsEntries];
    const uint64_t i = first + blockIdx.x;
    char* slot = scratch + (uint64_t)blockIdx.x * slot_bytes;
    PlanRowState* st = reinterpret_cast<PlanRowState*>(slot);
    PlanQueue q;
    q.cap0 = cap0 < kPlanLdsEntries ? cap0 : kPlanLdsEntries; q.cap1 = cap1;
    q.f0 = s_q; q.r0 = s_q + kPlanLdsEntries;
    q.f1 = reinterpret_cast<uint32_t*>(slot + (uint64_t)P.num_rows * sizeof(PlanRowState)); q.r1 = q.f1 + cap1;
    q.n = 0u; q.live = 0u;
    const float* p = starts + i * sf;
    const uint32_t start_row = plan_start_row<MODE>(Q, p[0], p[1], p[2]);
    RouteInfo out;
    plan_query<PlanWaveDevice>(P, start_row, st, stamp, q, max_expansions, route ? route + i * route_cap : nullptr, route ? route_cap : 0u, out);
    if ((threadIdx.x & 63u) == 0u)
        reinterpret_cast<uint4*>(info)[2 * i] = make_uint4((uint32_t)out.status, out.length, out.start_row, out.expansions),
        reinterpret_cast<uint4*>(info)[2 * i + 1] = make_uint4(out.queue_peak, float_bits(out.cost), float_bits(out.h_start), 0u);
}

// every query the same answer without a search (no goal: GNDT_ROUTE_NO_GOAL)
static __global__ void __launch_bounds__(256) k_plan_fill(uint64_t K, int32_t status, uint32_t* __restrict__ route, uint64_t route_words,
                                                         RouteInfo* __restrict__ info) {
    const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, gsz = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = gid; i < route_words; i += gsz) route[i] = kNoRow;
    for (uint64_t i = gid; i < K; i += gsz) {
        reinterpret_cast<uint4*>(info)[2 * i] = make_uint4((uint32_t)status, 0u, kNoRow, 0u);
        reinterpret_cast<uint4*>(info)[2 * i + 1] = make_uint4(0u, 0x7F7FFFFFu, 0x7F7FFFFFu, 0u);
    }
}
#endif  // __HIPCC__

}  // namespace gndt
