// gndt_obstacle.hpp — the obstacle field (include/gndt.h "obstacle field"): for every slope, the number of steps to the nearest slope
// that a box of a caller's list stands on, and which box that is.  Steps are the clearance field's (gndt_clearance.hpp: clearance_side,
// the flood's gates seen from the slope); the sources are not a property of the map but a list of boxes of signed indices, so the call's
// cost follows the boxes: a slope can only lie within max_hops steps of a box if its column lies in the box's WINDOW (the box grown by
// inflate + max_hops columns), and everything but the final fill of the outputs touches the rows of those columns alone.
//   k_obstacle_windows   per box its window's columns, their inclusive prefix sum W over the list, the budget's verdict     one workgroup
//   k_obstacle_mark      the two [num_nodes] outputs as they are without any box (the only pass over the map); then one thread a column
//                        of the concatenated admitted windows (found in W by bisection): the column joins the worklist once (a stamp
//                        per column), the box's index goes into its covered slopes (a stamped 64-bit minimum)
//   k_obstacle_steps     (worklist row, side) -> the steps in worklist places, the row's round-0 key                       4 probes a slope
//   k_obstacle_round     one Jacobi step over the worklist (one launch = one hop); flags as in k_clearance_round
//   k_obstacle_finish    worklist keys -> hops (merged with the base), obstacle; the call's counts
// The worklist holds every row of a column in reach in the column's order, so a column's rows are adjacent in it as they are in the map:
// a side's step mask (bit j = the column's j-th row) means the same in both, and the clearance field's round code reads the compact key
// arrays unchanged.  key = hops << 32 | box index, kClrNoKey while no walk is known (clearance's key with a box for the source row).
// The per-element logic is host-callable (tests/obstacle_shim.cpp runs it one element after another); memory operations go through an
// Ops policy (ObstacleSerialOps here, the device's with the kernels).
#pragma once
#include <stdint.h>

#include "gndt_clearance.hpp"

namespace gndt {

constexpr uint32_t kObsMaxInflate = 1024u, kObsMaxBoxes = 1u << 20;
constexpr uint64_t kObsMaxColumns = 1ull << 28, kObsDefaultColumns = 1ull << 24;
constexpr int kObsLinMin = -kMaxXY, kObsLinMax = kMaxXY - 1;       // lin of the indices that exist on x and y: -65535 .. -1, 1 .. 65535

struct ObstacleRule {
    uint32_t inflate, max_hops, levels_above, levels_below;        // max_hops: 1..kClrMaxHops (the entry point turns 0 into 8)
    uint64_t max_columns;                                          // 1..kObsMaxColumns (0 turned into kObsDefaultColumns)
};

// the window of a box on x and y in lin space: nx * ny columns, x fastest
struct ObstacleWindow {
    int32_t x0, y0;
    uint32_t nx, ny;
};

// Per map row (stamped, so nothing is cleared between calls): cstamp[c] == stamp: the column whose first row is c is in the worklist
// from place slot[c] on; cover[row] >> 32 == ~stamp: the slope is covered, by box (uint32_t)cover[row] at the least.  A later call's
// stamp is larger, its cover words smaller: both atomics (a maximum, a minimum) take a stale word for "not yet".
// Per worklist place: list (the map row).  len: the worklist's length.  covers[b]: box b covers a slope.
struct ObstacleMarks {
    uint32_t *cstamp, *slot;
    unsigned long long* cover;
    uint32_t *list, *len, *covers;
};

GNDT_HD long long obstacle_lin(int s) { return s > 0 ? (long long)s - 1 : (long long)s; }
GNDT_HD int obstacle_unlin(int l) { return l >= 0 ? l + 1 : l; }
GNDT_HD const int32_t* obstacle_box(const void* boxes, size_t stride, uint32_t b) {
    return reinterpret_cast<const int32_t*>(static_cast<const char*>(boxes) + (size_t)b * stride);
}
GNDT_HD bool obstacle_void(const int32_t* box) { return box[0] > box[1] || box[2] > box[3] || box[4] > box[5]; }

// one axis of a window: the indices that exist with lin in [lin(lo) - K, lin(hi) + K] -> how many, and the first one's lin
GNDT_HD uint32_t obstacle_axis(int lo, int hi, uint32_t K, int32_t& first) {
    long long a = obstacle_lin(lo) - (long long)K, b = obstacle_lin(hi) + (long long)K;
    a = a < kObsLinMin ? (long long)kObsLinMin : a;
    b = b > kObsLinMax ? (long long)kObsLinMax : b;
    first = b < a ? 0 : (int32_t)a;
    return b < a ? 0u : (uint32_t)(b - a + 1);
}

// the window of a box that is not void -> its columns (0: wholly outside the indices that exist)
GNDT_HD uint64_t obstacle_window(const int32_t* box, uint32_t K, ObstacleWindow& w) {
    w.nx = obstacle_axis(box[0], box[1], K, w.x0);
    w.ny = obstacle_axis(box[2], box[3], K, w.y0);
    return (uint64_t)w.nx * w.ny;
}

// does the box cover a slope at (sx, sy, sz)?
GNDT_HD bool obstacle_covers(const int32_t* box, const ObstacleRule& F, int sx, int sy, int sz) {
    const long long x = obstacle_lin(sx), y = obstacle_lin(sy), z = obstacle_lin(sz), in = F.inflate;
    return obstacle_lin(box[0]) - in <= x && x <= obstacle_lin(box[1]) + in && obstacle_lin(box[2]) - in <= y && y <= obstacle_lin(box[3]) + in &&
           obstacle_lin(box[4]) <= z + (long long)F.levels_above && obstacle_lin(box[5]) >= z - (long long)F.levels_below;
}

// Column c of the concatenated windows belongs to the first box whose inclusive prefix W passes c (W never falls, and a box that adds
// nothing — void, dropped boxes behind the budget aside — has its predecessor's): at most 21 halvings for 2^20 boxes
GNDT_HD uint32_t obstacle_box_of(const unsigned long long* W, uint32_t B, unsigned long long c) {
    uint32_t lo = 0u, hi = B;                           // the answer lies in [lo, hi)
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;       // W[mid - 1] > c: the answer is in front of mid
        if (W[mid - 1u] > c) hi = mid; else lo = mid;
    }
    return lo;
}

// One thread after another (the CPU tier)
struct ObstacleSerialOps : ClearanceSerialOps {
    static inline uint32_t load_u32(const uint32_t* p) { return *p; }
    static inline unsigned long long load_u64(const unsigned long long* p) { return *p; }
    static inline uint32_t max_u32_old(uint32_t* p, uint32_t v) { const uint32_t o = *p; if (v > o) *p = v; return o; }
    static inline uint32_t add_u32_old(uint32_t* p, uint32_t v) { const uint32_t o = *p; *p = o + v; return o; }
    static inline void min_u64(unsigned long long* p, unsigned long long v) { if (v < *p) *p = v; }
};

struct ObstacleMarkTally {
    uint32_t probes, claims, cover_atomics;             // index probes that found a column, columns this thread put on the list, minima sent
};

// Column (sx, sy) of box b's window: the column joins the worklist if no thread of this call has listed it, and b goes into its slopes
// that b covers.  A word that already says so is left alone (the plain read in front of each atomic).
template <class Ops>
GNDT_HD void obstacle_mark_column(const CostView& V, const ObstacleRule& F, const int32_t* box, uint32_t b, int sx, int sy, uint32_t stamp,
                                  const ObstacleMarks& M, ObstacleMarkTally& t) {
    const uint32_t c = ctab_find(V, sx, sy);
    if (c == kNoColumn) return;
    t.probes += 1u;
    const uint32_t ncol = V.row_ncol[c];
    if (Ops::load_u32(M.cstamp + c) != stamp && Ops::max_u32_old(M.cstamp + c, stamp) != stamp) {
        const uint32_t base = Ops::add_u32_old(M.len, ncol);
        M.slot[c] = base;
        for (uint32_t j = 0; j < ncol; ++j) M.list[base + j] = c + j;
        t.claims += 1u;
    }
    const unsigned long long word = ((unsigned long long)~stamp << 32) | b;
    bool any = false;
    for (uint32_t j = 0; j < ncol; ++j) {
        const uint32_t row = c + j;
        if (!(V.flags[row] & 2u) || !obstacle_covers(box, F, sx, sy, V.sz[row])) continue;
        any = true;
        if (Ops::load_u64(M.cover + row) > word) { Ops::min_u64(M.cover + row, word); t.cover_atomics += 1u; }
    }
    if (any) M.covers[b] = 1u;
}

// Item `item` of the concatenated admitted windows: its box (bisection in W), its place in that box's window, the column
template <class Ops>
GNDT_HD void obstacle_mark_item(const CostView& V, const ObstacleRule& F, const void* boxes, size_t stride, const unsigned long long* W,
                                uint32_t B, unsigned long long item, uint32_t stamp, const ObstacleMarks& M, ObstacleMarkTally& t) {
    const uint32_t b = obstacle_box_of(W, B, item);
    const int32_t* box = obstacle_box(boxes, stride, b);
    ObstacleWindow w;
    const unsigned long long cols = obstacle_window(box, F.inflate + F.max_hops, w);
    const unsigned long long local = item - (W[b] - cols);
    const int sx = obstacle_unlin(w.x0 + (int32_t)(local % w.nx)), sy = obstacle_unlin(w.y0 + (int32_t)(local / w.nx));
    obstacle_mark_column<Ops>(V, F, box, b, sx, sy, stamp, M, t);
}

// The k-th side of worklist row `row` for the rounds: clearance_side's answer with the neighbour column named by its first place in the
// worklist — a column that is not in reach has no key, so no step into it can matter: the side is left without a column
GNDT_HD uint32_t obstacle_side(const CostView& V, const Robot& R, uint32_t row, uint32_t k, uint32_t stamp, const ObstacleMarks& M, ClearanceStep& st) {
    uint32_t bits = clearance_side(V, R, row, k, st);
    if (st.c == kNoColumn) return bits;
    if (M.cstamp[st.c] == stamp) { st.c = M.slot[st.c]; return bits; }
    st.c = kNoColumn; st.mask = 0u;
    return bits & ~kClrSideTall;
}

// round 0 of a worklist row: the least box that covers it, at no steps
GNDT_HD unsigned long long obstacle_key0(const CostView& V, uint32_t row, uint32_t stamp, const ObstacleMarks& M) {
    const unsigned long long w = M.cover[row];
    return row_has_slope(V, row) && (uint32_t)(w >> 32) == ~stamp ? (unsigned long long)(uint32_t)w : kClrNoKey;
}

// One round, one side of worklist row `row` (a map row), st in worklist places, key_in the compact keys: the masked steps through the
// clearance field's code; of a tall column the rows behind the mask with the gates again, as clearance_round_side does in map rows
template <class Ops>
GNDT_HD unsigned long long obstacle_round_side(const CostView& V, const Robot& R, uint32_t row, const ClearanceStep& st, bool tall,
                                               const uint32_t* list, const unsigned long long* key_in) {
    if (st.c == kNoColumn) return kClrNoKey;
    unsigned long long best = clearance_round_side<Ops>(V, R, row, st, false, key_in);
    if (tall) {
        const uint32_t c = list[st.c], ncol = V.row_ncol[c];
        const float* nq = V.normal + 3 * (size_t)row;
        const float* mq = V.mean + 3 * (size_t)row;
        for (uint32_t j = kStepRows; j < ncol; ++j) {
            if (!(V.flags[c + j] & 2u) || !cost_gates(V, R, c + j, nq, mq)) continue;
            const unsigned long long kp = Ops::load_key(key_in + st.c + j);
            best = kp < best ? kp : best;
        }
    }
    return best;
}

// What a worklist row's key says, merged with the caller's base; what it adds to counts[0..2] (clearance's tally) and counts[5]
GNDT_HD void obstacle_finish_row(const CostView& V, uint32_t row, unsigned long long key, uint32_t max_hops, const uint32_t* base, uint32_t* hops,
                                 uint32_t* obstacle, ClearanceTally& t, uint32_t& in_reach) {
    uint32_t hp, ob;
    clearance_finish_row(key, max_hops, hp, ob, t);
    in_reach += row_has_slope(V, row) ? 1u : 0u;
    if (hops) {
        const uint32_t bh = base ? base[row] : kClrBeyond;
        hops[row] = bh < hp ? bh : hp;
    }
    if (obstacle) obstacle[row] = ob;
}

// the call's words on the device: what the later kernels size their loops by
struct ObstacleHeader {
    unsigned long long items;          // columns of the concatenated admitted windows: the largest W within the budget
    uint32_t B, len;                   // the boxes of the call; the worklist's length (k_obstacle_mark adds to it)
    unsigned long long probes, claims, cover_atomics;       // the mark pass's tallies (tools/measure_obstacle.py; only with `tally`)
};

// The stamped marks of `rows` map rows (gndt_api_obstacle.hip obstacle_marks): 16 B a row
inline void obstacle_carve_marks(Carver& c, uint64_t rows, ObstacleMarks& M) {
    M.cover = c.take<unsigned long long>(rows);
    M.cstamp = c.take<uint32_t>(rows);
    M.slot = c.take<uint32_t>(rows);
}

// A call's scratch for a map of n rows and a list of n_boxes boxes (gndt_api_obstacle.hip)
constexpr uint64_t kObsHeaderBytes = 64;
static_assert(sizeof(ObstacleHeader) <= kObsHeaderBytes && alignof(ObstacleHeader) == alignof(unsigned long long), "the header's room");
struct ObstacleScratch {
    ObstacleHeader* hdr;             // kObsHeaderBytes of room
    unsigned long long* W;           // [n_boxes] the windows' prefix sums
    unsigned long long* key[2];      // [n] each: the rounds' ping-pong
    ClearanceStep* step;             // [4 n] the steps table
    uint32_t* flags;                 // [kClrFlagWords]
    uint32_t* covers;                // [n_boxes] box b covers a slope
    uint32_t* list;                  // [n] the worklist
    uint8_t* tall;                   // [n] the tall-column bits
    ObstacleScratch() = default;
    ObstacleScratch(Carver& c, uint64_t n, uint64_t n_boxes)
        : hdr(reinterpret_cast<ObstacleHeader*>(c.take<unsigned long long>(kObsHeaderBytes / 8))), W(c.take<unsigned long long>(n_boxes)),
          key{c.take<unsigned long long>(n), c.take<unsigned long long>(n)}, step(c.take<ClearanceStep>(4 * n)),
          flags(c.take<uint32_t>(kClrFlagWords)), covers(c.take<uint32_t>(n_boxes)), list(c.take<uint32_t>(n)), tall(c.take<uint8_t>(n)) {}
};

}  // namespace gndt

#if defined(__HIPCC__)
namespace gndt {

constexpr int kObsWinThreads = 1024;

struct ObstacleDeviceOps : ClearanceDeviceOps {
    // (plain reads beside the atomics: a stale word only sends an atomic that changes nothing)
    static __device__ __forceinline__ uint32_t load_u32(const uint32_t* p) { return *p; }
    static __device__ __forceinline__ unsigned long long load_u64(const unsigned long long* p) { return *p; }
    static __device__ __forceinline__ uint32_t max_u32_old(uint32_t* p, uint32_t v) { return atomicMax(p, v); }
    static __device__ __forceinline__ uint32_t add_u32_old(uint32_t* p, uint32_t v) { return atomicAdd(p, v); }
    static __device__ __forceinline__ void min_u64(unsigned long long* p, unsigned long long v) { atomicMin(p, v); }
};

// One workgroup: tiles of 1024 boxes, an inclusive scan of the windows' columns across the tile with the carry of the tiles before.
// W[b] for every box of the call, covers[b] = 0, the header, the counts zeroed but counts[3] = B and, with a map that has rows, counts[6] =
// the dropped boxes; the rounds' n_flags flag words zeroed.
static __global__ void __launch_bounds__(kObsWinThreads) k_obstacle_windows(const void* __restrict__ boxes, uint32_t n_boxes, size_t stride,
                                                                            const uint32_t* __restrict__ n_boxes_dev, ObstacleRule F, bool rows,
                                                                            unsigned long long* __restrict__ W, uint32_t* __restrict__ covers,
                                                                            ObstacleHeader* __restrict__ hdr, uint32_t* __restrict__ counts,
                                                                            uint32_t* __restrict__ flags, uint32_t n_flags) {
    __shared__ unsigned long long s_wave[kObsWinThreads / 64], s_carry, s_items;
    __shared__ uint32_t s_dropped;
    const uint32_t B = n_boxes_dev ? min(*n_boxes_dev, n_boxes) : n_boxes;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0u) { s_carry = 0ull; s_items = 0ull; s_dropped = 0u; }
    if (threadIdx.x < 8u) counts[threadIdx.x] = 0u;                     // (the call's first kernel: no fills in front of it)
    for (uint32_t i = threadIdx.x; i < n_flags; i += kObsWinThreads) flags[i] = 0u;
    __syncthreads();
    for (uint32_t b0 = 0; b0 < B; b0 += kObsWinThreads) {              // (uniform: B is one word)
        const uint32_t b = b0 + threadIdx.x;
        unsigned long long w = 0ull;
        bool solid = false;
        if (b < B) {
            const int32_t* box = obstacle_box(boxes, stride, b);
            solid = !obstacle_void(box);
            ObstacleWindow win;
            if (solid) w = obstacle_window(box, F.inflate + F.max_hops, win);
        }
        unsigned long long v = w;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long u = (unsigned long long)__shfl_up((long long)v, o, 64);
            if ((int)lane >= o) v += u;
        }
        if (lane == 63u) s_wave[wave] = v;
        __syncthreads();
        unsigned long long before = s_carry;
        for (uint32_t k = 0; k < wave; ++k) before += s_wave[k];
        const unsigned long long incl = before + v;
        if (b < B) {
            W[b] = incl;
            covers[b] = 0u;
            if (solid && incl <= F.max_columns) atomicMax(&s_items, incl);
            if (solid && incl > F.max_columns) atomicAdd(&s_dropped, 1u);
        }
        __syncthreads();
        if (threadIdx.x == kObsWinThreads - 1) s_carry = incl;
        __syncthreads();
    }
    if (threadIdx.x == 0u) {
        hdr->items = rows ? s_items : 0ull;
        hdr->B = B; hdr->len = 0u;
        hdr->probes = 0ull; hdr->claims = 0ull; hdr->cover_atomics = 0ull;
        counts[3] = B;
        if (rows) counts[6] = s_dropped;
    }
}

// First the outputs of a call without boxes — the base (or BEYOND) and NO_ROW for every row of the map, the only pass over the map;
// hops == base: nothing to copy — which k_obstacle_finish, a later launch, overwrites on the worklist's rows.  Then one thread a
// column of the concatenated admitted windows, grid-stride: the trips are bounded by max_columns whatever the boxes say.
static __global__ void __launch_bounds__(256) k_obstacle_mark(CostView V, ObstacleRule F, const void* __restrict__ boxes, size_t stride,
                                                              const unsigned long long* __restrict__ W, ObstacleHeader* __restrict__ hdr,
                                                              uint32_t stamp, ObstacleMarks M, uint32_t n, const uint32_t* base, uint32_t* hops,
                                                              uint32_t* __restrict__ obstacle, bool tally) {
    const unsigned long long items = hdr->items, gsz = (unsigned long long)gridDim.x * blockDim.x;
    const bool copy = hops && hops != base;
    for (unsigned long long row = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; row < n; row += gsz) {
        if (copy) hops[row] = base ? base[row] : kClrBeyond;
        if (obstacle) obstacle[row] = kNoRow;
    }
    const uint32_t B = hdr->B;
    ObstacleMarkTally t{0u, 0u, 0u};
    for (unsigned long long item = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; item < items; item += gsz)
        obstacle_mark_item<ObstacleDeviceOps>(V, F, boxes, stride, W, B, item, stamp, M, t);
    // the tallies are gndt_debug_obstacle_marks' alone: kept only while GNDT_DEBUG_OBSTACLE_TALLY is set
    if (!tally || (unsigned long long)blockIdx.x * blockDim.x >= items) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        t.probes += (uint32_t)__shfl_xor((int)t.probes, o, 64);
        t.claims += (uint32_t)__shfl_xor((int)t.claims, o, 64);
        t.cover_atomics += (uint32_t)__shfl_xor((int)t.cover_atomics, o, 64);
    }
    if ((threadIdx.x & 63u) == 0u) {
        if (t.probes) atomicAdd(&hdr->probes, (unsigned long long)t.probes);
        if (t.claims) atomicAdd(&hdr->claims, (unsigned long long)t.claims);
        if (t.cover_atomics) atomicAdd(&hdr->cover_atomics, (unsigned long long)t.cover_atomics);
    }
}

// Four lanes a worklist row, one per side (k_clearance_steps' spread): step[4 i + k] in worklist places, tall[i], key0[i]
static __global__ void __launch_bounds__(256) k_obstacle_steps(CostView V, Robot R, const ObstacleHeader* __restrict__ hdr, uint32_t stamp, ObstacleMarks M,
                                                               ClearanceStep* __restrict__ step, uint8_t* __restrict__ tall,
                                                               unsigned long long* __restrict__ key0, uint32_t* __restrict__ flag0) {
    const uint64_t total = 4ull * hdr->len, gsz = (uint64_t)gridDim.x * blockDim.x;
    if (blockIdx.x == 0 && threadIdx.x == 0) *flag0 = total ? 1u : 0u;
    for (uint64_t t0 = (uint64_t)blockIdx.x * blockDim.x; t0 < total; t0 += gsz) {      // (uniform: the quad exchanges below)
        const uint64_t t = t0 + threadIdx.x;
        const bool live = t < total;
        const uint32_t i = live ? (uint32_t)(t >> 2) : 0u, k = (uint32_t)t & 3u;
        const uint32_t row = live ? M.list[i] : 0u;
        const bool slope = live && row_has_slope(V, row);
        ClearanceStep st{kNoColumn, 0u};
        uint32_t bits = 0u;
        if (slope) bits = obstacle_side(V, R, row, k, stamp, M, st);
        if (live) reinterpret_cast<uint2*>(step)[t] = make_uint2(st.c, st.mask);
        uint32_t tb = (bits & kClrSideTall) ? 1u << k : 0u;
        tb |= (uint32_t)__shfl_xor((int)tb, 1, 64);
        tb |= (uint32_t)__shfl_xor((int)tb, 2, 64);
        if (live && k == 0u) {
            tall[i] = (uint8_t)tb;
            key0[i] = obstacle_key0(V, row, stamp, M);
        }
    }
}

// Round `round` over the worklist: k_clearance_round with compact keys
static __global__ void __launch_bounds__(256) k_obstacle_round(CostView V, Robot R, const ObstacleHeader* __restrict__ hdr, uint32_t round,
                                                               const uint32_t* __restrict__ list, const ClearanceStep* __restrict__ step,
                                                               const uint8_t* __restrict__ tall, const unsigned long long* __restrict__ key_in,
                                                               unsigned long long* __restrict__ key_out, uint32_t* __restrict__ flags) {
    if (flags[round - 1u] == 0u) return;
    const uint64_t total = 4ull * hdr->len, gsz = (uint64_t)gridDim.x * blockDim.x;
    bool changed = false;
    for (uint64_t t0 = (uint64_t)blockIdx.x * blockDim.x; t0 < total; t0 += gsz) {      // (uniform: the quad exchanges)
        const uint64_t t = t0 + threadIdx.x;
        const bool live = t < total;
        const uint32_t i = live ? (uint32_t)(t >> 2) : 0u, k = (uint32_t)t & 3u;
        const unsigned long long own = live ? key_in[i] : kClrNoKey;
        const uint32_t row = live ? list[i] : 0u;
        const bool relax = live && own == kClrNoKey && row_has_slope(V, row);
        unsigned long long least = kClrNoKey;
        if (relax) {
            const uint2 e = reinterpret_cast<const uint2*>(step)[t];
            least = obstacle_round_side<ObstacleDeviceOps>(V, R, row, ClearanceStep{e.x, e.y}, (tall[i] >> k) & 1u, list, key_in);
        }
        const unsigned long long key = clearance_relax(own, clearance_quad_min(least));
        if (live && k == 0u) {
            if (clearance_round_stores(key, round)) key_out[i] = key;
            changed = changed || key != own;
        }
    }
    if (__any(changed) && (threadIdx.x & 63u) == 0u) flags[round] = 1u;
}

// The worklist's keys into the outputs (behind k_obstacle_mark's fill on the stream) and the counts: [0..2] as clearance folds them, [5] the
// slopes in reach; workgroup 0 also counts the boxes that cover a slope into [4]
static __global__ void __launch_bounds__(256) k_obstacle_finish(CostView V, const ObstacleHeader* __restrict__ hdr, const uint32_t* __restrict__ list,
                                                                const unsigned long long* __restrict__ key, uint32_t max_hops,
                                                                const uint32_t* base, uint32_t* hops, uint32_t* __restrict__ obstacle,
                                                                const uint32_t* __restrict__ covers, uint32_t* __restrict__ counts) {
    __shared__ uint32_t s_counts[4], s_more[2];
    const uint32_t len = hdr->len, B = hdr->B;
    if ((uint64_t)blockIdx.x * blockDim.x >= len && blockIdx.x != 0) return;
    if (threadIdx.x < 4u) s_counts[threadIdx.x] = 0u;
    if (threadIdx.x < 2u) s_more[threadIdx.x] = 0u;
    __syncthreads();
    const uint64_t gsz = (uint64_t)gridDim.x * blockDim.x;
    ClearanceTally t{0u, 0u, 0u};
    uint32_t in_reach = 0u, covering = 0u;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += gsz)
        obstacle_finish_row(V, list[i], key[i], max_hops, base, hops, obstacle, t, in_reach);
    if (blockIdx.x == 0)
        for (uint32_t b = threadIdx.x; b < B; b += blockDim.x) covering += covers[b] ? 1u : 0u;
    clearance_flush(t, s_counts);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        in_reach += (uint32_t)__shfl_xor((int)in_reach, o, 64);
        covering += (uint32_t)__shfl_xor((int)covering, o, 64);
    }
    if ((threadIdx.x & 63u) == 0u) {
        if (in_reach) atomicAdd(&s_more[0], in_reach);
        if (covering) atomicAdd(&s_more[1], covering);
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
        clearance_fold<ClearanceDeviceOps>(counts, ClearanceTally{s_counts[0], s_counts[1], s_counts[2]});
        if (s_more[0]) atomicAdd(counts + 5, s_more[0]);
        if (s_more[1]) atomicAdd(counts + 4, s_more[1]);
    }
}

}  // namespace gndt
#endif  // __HIPCC__
