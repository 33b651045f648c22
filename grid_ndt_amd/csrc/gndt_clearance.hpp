// gndt_clearance.hpp — the clearance field (include/gndt.h "clearance field"): for every slope, the number of steps to the nearest
// slope that has a barrier beside it, and which slope that is.  A step goes from a slope to a slope of one of its four neighbour
// columns that passes the flood's three gates seen from it (cost_gates: the steps of cost_expand_column); a side with a column and
// no step is blocked, a side without a column is open.
//   k_clearance_steps    (row, side) -> the column's first row, the step mask, the side's bits; the row's round-0 key     4 probes a slope
//   k_clearance_round    one Jacobi step key_in -> key_out over all rows (one launch = one hop)                           <= 8 + 4 x 8 B a slope
//   k_clearance_wg       every round in one launch, both key arrays in LDS, one workgroup (maps of up to kClrLdsRows rows)
//   k_clearance_finish   keys -> hops, nearest; the call's counts
// key = hops << 32 | source row, kClrNoKey while no walk is known: one unsigned minimum picks the fewest steps and, among the sources
// that many steps away, the smallest row.  The field is the fixed point of key(q) = min(key(q), min over steps p of key(p) + 2^32);
// a Jacobi round r makes every row with hops r final (a later candidate is longer), so rounds never disagree about a final row and the
// answer does not depend on the order threads work in.
// The per-row logic is host-callable so that the CPU test tier runs the kernels' own code one row after another
// (tests/clearance_shim.cpp); memory operations go through an Ops policy (ClearanceSerialOps here, the device's with the kernels).
#pragma once
#include <stdint.h>

#include "gndt_query.hpp"
#include "gndt_scratch.hpp"

namespace gndt {

constexpr uint32_t kClrBlocked = 1u, kClrOpen = 2u, kClrOverhead = 4u;     // GNDT_CLEARANCE_BLOCKED / _OPEN / _OVERHEAD
constexpr uint32_t kClrBeyond = 0xFFFFFFFFu;                               // GNDT_CLEARANCE_BEYOND
constexpr uint32_t kClrMaxHops = 1024u;
constexpr unsigned long long kClrNoKey = ~0ull;
constexpr unsigned long long kClrHop = 1ull << 32;
constexpr uint32_t kClrSideBlocked = 1u, kClrSideOpen = 2u, kClrSideTall = 4u;      // clearance_side's answer

struct ClearanceRule {
    uint32_t sources, max_hops;        // max_hops: 1..kClrMaxHops (the entry point turns 0 into 32, sources 0 into BLOCKED)
};

// one side of a slope as the rounds read it: the neighbour column's first row (kNoColumn: none) and the steps into it, bit j = row
// c + j for the column's first kStepRows rows
struct ClearanceStep {
    uint32_t c, mask;
};

GNDT_HD uint32_t clearance_hops(unsigned long long key) { return (uint32_t)(key >> 32); }

// The k-th side of slope `row`, k in neighbour_column's order (left, right, forward, back).  open: the column is not in the map (an
// index beyond the codec's range is not); blocked: it is and none of its rows is a step; tall: it has more than kStepRows rows, so
// the rounds walk the rest with the gates again (as ring_round_cell does).
GNDT_HD uint32_t clearance_side(const CostView& V, const Robot& R, uint32_t row, uint32_t k, ClearanceStep& st) {
    const int sx = V.sx[row], sy = V.sy[row];
    const int nx = k == 2u ? step_skip0(sx, +1) : k == 3u ? step_skip0(sx, -1) : sx;
    const int ny = k == 0u ? step_skip0(sy, -1) : k == 1u ? step_skip0(sy, +1) : sy;
    st.c = kNoColumn; st.mask = 0u;
    if (nx < -kMaxXY || nx > kMaxXY || ny < -kMaxXY || ny > kMaxXY) return kClrSideOpen;
    const uint32_t c = ctab_find(V, nx, ny);
    if (c == kNoColumn) return kClrSideOpen;
    const uint32_t ncol = V.row_ncol[c];
    const float* nq = V.normal + 3 * (size_t)row;
    const float* mq = V.mean + 3 * (size_t)row;
    bool any = false;
    for (uint32_t j = 0; j < ncol; ++j) {
        const uint32_t t = c + j;
        if (!(V.flags[t] & 2u) || !cost_gates(V, R, t, nq, mq)) continue;
        any = true;
        if (j < kStepRows) st.mask |= 1u << j;
    }
    st.c = c;
    return (any ? 0u : kClrSideBlocked) | (ncol > kStepRows ? kClrSideTall : 0u);
}

// the first row of the row's own column: a column's rows are adjacent and its first row is the one that names its size
GNDT_HD uint32_t clearance_own_column(const CostView& V, uint32_t row) {
    uint32_t c = row;
    while (V.row_ncol[c] == 0u && c > 0u) --c;
    return c;
}

// Round 0 of a slope: its own row at no steps if it is a source.  sides: bits 0-3 its blocked sides, 4-7 its open sides.
GNDT_HD unsigned long long clearance_key0(const CostView& V, const Robot& R, const ClearanceRule& F, uint32_t row, uint32_t sides) {
    bool src = ((F.sources & kClrBlocked) && (sides & 0x0Fu)) || ((F.sources & kClrOpen) && (sides & 0xF0u));
    if (!src && (F.sources & kClrOverhead)) src = row_above_hits_in(V, R, row, clearance_own_column(V, row));
    return src ? (unsigned long long)row : kClrNoKey;
}

// One thread after another (the CPU tier)
struct ClearanceSerialOps {
    static inline unsigned long long load_key(const unsigned long long* p) { return *p; }
    static inline void add_u32(uint32_t* p, uint32_t v) { *p += v; }
    static inline void max_u32(uint32_t* p, uint32_t v) { if (v > *p) *p = v; }
};

// One round, one side: the least key among the steps of `row` through it (kClrNoKey: none has one yet)
template <class Ops>
GNDT_HD unsigned long long clearance_round_side(const CostView& V, const Robot& R, uint32_t row, const ClearanceStep& st, bool tall,
                                                const unsigned long long* key_in) {
    unsigned long long best = kClrNoKey;
    if (st.c == kNoColumn) return best;
    uint32_t mask = st.mask;
    while (mask) {
        uint32_t j = 0;
        while (!((mask >> j) & 1u)) ++j;
        mask &= mask - 1u;
        const unsigned long long kp = Ops::load_key(key_in + st.c + j);
        best = kp < best ? kp : best;
    }
    if (tall) {                                         // (a column of more than kStepRows rows)
        const uint32_t ncol = V.row_ncol[st.c];
        const float* nq = V.normal + 3 * (size_t)row;
        const float* mq = V.mean + 3 * (size_t)row;
        for (uint32_t j = kStepRows; j < ncol; ++j) {
            const uint32_t t = st.c + j;
            if (!(V.flags[t] & 2u) || !cost_gates(V, R, t, nq, mq)) continue;
            const unsigned long long kp = Ops::load_key(key_in + t);
            best = kp < best ? kp : best;
        }
    }
    return best;
}

// One round, all four sides of a row in one thread: the first step of every side is asked for before any is looked at (a side rarely
// has more: one wait instead of four), then what is left of each side
template <class Ops>
GNDT_HD unsigned long long clearance_round_row(const CostView& V, const Robot& R, uint32_t row, const ClearanceStep* st, uint32_t tall_bits,
                                               const unsigned long long* key_in) {
    unsigned long long first[4];
    for (uint32_t k = 0; k < 4u; ++k) {
        const bool any = st[k].c != kNoColumn && st[k].mask != 0u;
        first[k] = any ? Ops::load_key(key_in + st[k].c + (uint32_t)__builtin_ctz(any ? st[k].mask : 1u)) : kClrNoKey;
    }
    unsigned long long least = kClrNoKey;
    for (uint32_t k = 0; k < 4u; ++k) {
        least = first[k] < least ? first[k] : least;
        const ClearanceStep rest{st[k].c, st[k].mask & (st[k].mask - 1u)};
        if (rest.mask || ((tall_bits >> k) & 1u)) {
            const unsigned long long m = clearance_round_side<Ops>(V, R, row, rest, (tall_bits >> k) & 1u, key_in);
            least = m < least ? m : least;
        }
    }
    return least;
}

// A row's key after a round: what it had, or one step more than the least key among its steps
GNDT_HD unsigned long long clearance_relax(unsigned long long own, unsigned long long least) {
    const unsigned long long cand = least == kClrNoKey ? kClrNoKey : least + kClrHop;
    return cand < own ? cand : own;
}

// Must round `round` (1, 2, ...) of the ping-pong store a row's new key?  The buffer it writes holds the row's key of two rounds ago
// (round 1: nothing yet): that differs only for a key found in this round or the one before.
GNDT_HD bool clearance_round_stores(unsigned long long key_new, uint32_t round) {
    return round == 1u || (key_new != kClrNoKey && clearance_hops(key_new) + 1u >= round);
}

// What a row's key says: hops and nearest (anything beyond max_hops is no answer), and what it adds to the counts
struct ClearanceTally {
    uint32_t sources, finite, max_hops;
};
GNDT_HD void clearance_finish_row(unsigned long long key, uint32_t max_hops, uint32_t& hops, uint32_t& nearest, ClearanceTally& t) {
    const bool ok = key != kClrNoKey && clearance_hops(key) <= max_hops;
    hops = ok ? clearance_hops(key) : kClrBeyond;
    nearest = ok ? (uint32_t)key : kNoRow;
    if (ok) {
        t.sources += hops == 0u ? 1u : 0u;
        t.finite += 1u;
        t.max_hops = hops > t.max_hops ? hops : t.max_hops;
    }
}

// counts[4] = {sources, slopes with finite hops, the largest finite hops, 0}: integer sums and a maximum, any order
template <class Ops>
GNDT_HD void clearance_fold(uint32_t* counts, const ClearanceTally& t) {
    if (t.sources) Ops::add_u32(counts, t.sources);
    if (t.finite) Ops::add_u32(counts + 1, t.finite);
    if (t.max_hops) Ops::max_u32(counts + 2, t.max_hops);
}

// A call's scratch for a map of n rows (gndt_api_clearance.hip; the obstacle field's flags have the same room)
constexpr uint64_t kClrFlagWords = kClrMaxHops + 8u;   // one word a round, kClrMaxHops + 1 of them, padded
struct ClearanceScratch {
    ClearanceStep* step;             // [4 n] the steps table, a side a record
    unsigned long long* key[2];      // [n] each: the rounds' ping-pong
    uint32_t* flags;                 // [kClrFlagWords]
    uint8_t* tall;                   // [n] the tall-column bits
    ClearanceScratch() = default;
    ClearanceScratch(Carver& c, uint64_t n)
        : step(c.take<ClearanceStep>(4 * n)), key{c.take<unsigned long long>(n), c.take<unsigned long long>(n)},
          flags(c.take<uint32_t>(kClrFlagWords)), tall(c.take<uint8_t>(n)) {}
};

}  // namespace gndt

#if defined(__HIPCC__)
namespace gndt {

constexpr int kClrWgThreads = 1024;
constexpr uint32_t kClrLdsRows = 9216u;                // two key arrays of 8 B a row: 144 KB of the CU's 160 KiB
constexpr uint32_t kClrLdsTail = 64u;                  // bytes behind the keys: the rounds' changed flags

struct ClearanceDeviceOps {
    static __device__ __forceinline__ unsigned long long load_key(const unsigned long long* p) { return *p; }
    static __device__ __forceinline__ void add_u32(uint32_t* p, uint32_t v) { atomicAdd(p, v); }
    static __device__ __forceinline__ void max_u32(uint32_t* p, uint32_t v) { atomicMax(p, v); }
};
// the keys in LDS (k_clearance_wg)
struct ClearanceLdsOps : ClearanceDeviceOps {
    static __device__ __forceinline__ unsigned long long load_key(const unsigned long long* p) {
        return *(const __attribute__((address_space(3))) unsigned long long*)p;
    }
    static __device__ __forceinline__ void store_key(unsigned long long* p, unsigned long long v) {
        *(__attribute__((address_space(3))) unsigned long long*)p = v;
    }
};

__device__ __forceinline__ unsigned long long clearance_quad_min(unsigned long long v) {
    unsigned long long o = (unsigned long long)__shfl_xor((long long)v, 1, 64);
    v = o < v ? o : v;
    o = (unsigned long long)__shfl_xor((long long)v, 2, 64);
    return o < v ? o : v;
}

// Four lanes a row, one per side (k_cost_neighbours' spread).  step[4 row + k], tall[row] (bit k: side k's column is tall) and
// key0[row] for every row; sides[row] (optional: the caller's) is 0xFF for a row without a slope.  flag0: the rounds' flag word 0,
// set here so that round 1 runs.
static __global__ void __launch_bounds__(256) k_clearance_steps(CostView V, Robot R, ClearanceRule F, uint32_t n, ClearanceStep* __restrict__ step,
                                                                uint8_t* __restrict__ tall, unsigned long long* __restrict__ key0,
                                                                uint8_t* __restrict__ sides, uint32_t* __restrict__ flag0) {
    const uint64_t total = 4ull * n, gsz = (uint64_t)gridDim.x * blockDim.x;
    if (blockIdx.x == 0 && threadIdx.x == 0) *flag0 = 1u;
    for (uint64_t t0 = (uint64_t)blockIdx.x * blockDim.x; t0 < total; t0 += gsz) {      // (uniform: the quad exchanges below)
        const uint64_t t = t0 + threadIdx.x;
        const bool live = t < total;
        const uint32_t row = live ? (uint32_t)(t >> 2) : 0u, k = (uint32_t)t & 3u;
        const bool slope = live && row_has_slope(V, row);
        ClearanceStep st{kNoColumn, 0u};
        uint32_t bits = 0u;
        if (slope) bits = clearance_side(V, R, row, k, st);
        if (live) reinterpret_cast<uint2*>(step)[t] = make_uint2(st.c, st.mask);
        // the row's byte: blocked sides in bits 0-3, open in 4-7; tall columns likewise in four bits
        uint32_t sb = ((bits & kClrSideBlocked) ? 1u << k : 0u) | ((bits & kClrSideOpen) ? 16u << k : 0u) | ((bits & kClrSideTall) ? 256u << k : 0u);
        sb |= (uint32_t)__shfl_xor((int)sb, 1, 64);
        sb |= (uint32_t)__shfl_xor((int)sb, 2, 64);
        if (live && k == 0u) {
            tall[row] = (uint8_t)(sb >> 8);
            if (sides) sides[row] = slope ? (uint8_t)sb : (uint8_t)0xFFu;
            key0[row] = slope ? clearance_key0(V, R, F, row, sb & 0xFFu) : kClrNoKey;
        }
    }
}

// One row's round on its four lanes -> the row's new key (every lane of the quad holds it).  A row that has a key is final.
template <class Ops>
__device__ __forceinline__ unsigned long long clearance_round_quad(const CostView& V, const Robot& R, uint32_t row, uint32_t k, bool slope,
                                                                   const ClearanceStep* __restrict__ step, const uint8_t* __restrict__ tall,
                                                                   const unsigned long long* key_in, unsigned long long own) {
    unsigned long long least = kClrNoKey;
    if (slope && own == kClrNoKey) {
        const uint2 e = reinterpret_cast<const uint2*>(step)[4 * (size_t)row + k];
        const ClearanceStep st{e.x, e.y};
        if (st.c != kNoColumn) least = clearance_round_side<Ops>(V, R, row, st, (tall[row] >> k) & 1u, key_in);
    }
    return clearance_relax(own, clearance_quad_min(least));
}

// Round `round` for every row.  flags[round - 1]: did the round before change anything (flags[0] is set by k_clearance_steps)?  If not,
// the two buffers are equal and stay so: nothing to do, here and in every later round.
static __global__ void __launch_bounds__(256) k_clearance_round(CostView V, Robot R, uint32_t n, uint32_t round, const ClearanceStep* __restrict__ step,
                                                                const uint8_t* __restrict__ tall, const unsigned long long* __restrict__ key_in,
                                                                unsigned long long* __restrict__ key_out, uint32_t* __restrict__ flags) {
    if (flags[round - 1u] == 0u) return;
    const uint64_t total = 4ull * n, gsz = (uint64_t)gridDim.x * blockDim.x;
    bool changed = false;
    for (uint64_t t0 = (uint64_t)blockIdx.x * blockDim.x; t0 < total; t0 += gsz) {      // (uniform: the quad exchanges)
        const uint64_t t = t0 + threadIdx.x;
        const bool live = t < total;
        const uint32_t row = live ? (uint32_t)(t >> 2) : 0u, k = (uint32_t)t & 3u;
        const unsigned long long own = live ? key_in[row] : kClrNoKey;
        const bool slope = live && own == kClrNoKey && row_has_slope(V, row);
        const unsigned long long key = clearance_round_quad<ClearanceDeviceOps>(V, R, row, k, slope, step, tall, key_in, own);
        if (live && k == 0u) {
            if (clearance_round_stores(key, round)) key_out[row] = key;
            changed = changed || key != own;
        }
    }
    if (__any(changed) && (threadIdx.x & 63u) == 0u) flags[round] = 1u;
}

// a wave's tally -> the counts: combined over the wave first, one lane's atomics
__device__ __forceinline__ void clearance_flush(ClearanceTally t, uint32_t* __restrict__ counts) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        t.sources += (uint32_t)__shfl_xor((int)t.sources, o, 64);
        t.finite += (uint32_t)__shfl_xor((int)t.finite, o, 64);
        t.max_hops = max(t.max_hops, (uint32_t)__shfl_xor((int)t.max_hops, o, 64));
    }
    if ((threadIdx.x & 63u) == 0u) clearance_fold<ClearanceDeviceOps>(counts, t);
}

// counts were zeroed on the stream before the call's first kernel.  A workgroup's waves add up in LDS first: same-address atomics retire
// at ~90 a microsecond at the memory side, and one set per wave of an 800 k-row map took 227 us where the rows stream in 10
// (the host launches at most kClrFinishBlocks workgroups).
constexpr int kClrFinishBlocks = 512;
static __global__ void __launch_bounds__(256) k_clearance_finish(const unsigned long long* __restrict__ key, uint32_t n, uint32_t max_hops,
                                                                 uint32_t* __restrict__ hops, uint32_t* __restrict__ nearest,
                                                                 uint32_t* __restrict__ counts) {
    __shared__ uint32_t s_counts[4];
    if (threadIdx.x < 4u) s_counts[threadIdx.x] = 0u;
    __syncthreads();
    const uint64_t gsz = (uint64_t)gridDim.x * blockDim.x;
    ClearanceTally t{0u, 0u, 0u};
    for (uint64_t row = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; row < n; row += gsz) {
        uint32_t hp, nr;
        clearance_finish_row(key[row], max_hops, hp, nr, t);
        if (hops) hops[row] = hp;
        if (nearest) nearest[row] = nr;
    }
    clearance_flush(t, s_counts);
    __syncthreads();
    if (threadIdx.x == 0u) clearance_fold<ClearanceDeviceOps>(counts, ClearanceTally{s_counts[0], s_counts[1], s_counts[2]});
}

// Every round in one launch: one workgroup, both key arrays in LDS (n <= kClrLdsRows), a workgroup barrier between rounds, out at the
// first round that changes nothing; then the finish.  One thread a row here, a thread's rows (tid, tid + 1024, ...) in fixed slots, and a
// round only looks at the slopes still without a key (`pending`, a bit a slot) — measured on the 7 598-row middle of the drivable site, 26 hops deep: 496 us with four lanes a row
// walking every row in every round (a chain of a global and an LDS round trip per 1 024 sides), against 148 us for a launch a hop.
// Both arrays start as round 0, so a key found in round r is stored for round r + 1 to read and copied to the other array in round
// r + 1 (`fresh`): the arrays then hold what clearance_round_stores leaves in the launch-a-hop path, and the same bytes go out.
// Dynamic LDS: key arrays [2][n], then three flag words (all of the kernel's LDS is dynamic, so the 8-byte keys sit on an aligned base).
constexpr uint32_t kClrWgSlots = (kClrLdsRows + kClrWgThreads - 1) / kClrWgThreads;
static __global__ void __launch_bounds__(kClrWgThreads) k_clearance_wg(CostView V, Robot R, uint32_t n, uint32_t max_hops,
                                                                       const ClearanceStep* __restrict__ step, const uint8_t* __restrict__ tall,
                                                                       const unsigned long long* __restrict__ key0, uint32_t* __restrict__ hops,
                                                                       uint32_t* __restrict__ nearest, uint32_t* __restrict__ counts) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long s_key[];       // [2][n], then the flags
    uint32_t* const s_flag = reinterpret_cast<uint32_t*>(s_key + 2 * (size_t)n);
    uint32_t pending = 0u, fresh = 0u;                  // bit j: slot j's row has no key yet / got its key in the round before
    for (uint32_t j = 0; j < kClrWgSlots; ++j) {
        const uint32_t row = threadIdx.x + j * kClrWgThreads;
        if (row >= n) break;
        const unsigned long long k0 = key0[row];
        ClearanceLdsOps::store_key(s_key + row, k0);
        ClearanceLdsOps::store_key(s_key + n + row, k0);
        if (k0 == kClrNoKey && row_has_slope(V, row)) pending |= 1u << j;
    }
    if (threadIdx.x < 3u) s_flag[threadIdx.x] = 0u;
    __syncthreads();
    uint32_t last = 0u;                                 // the round whose output is the answer
    for (uint32_t round = 1u; round <= max_hops; ++round) {
        const unsigned long long* key_in = s_key + ((round - 1u) & 1u) * (size_t)n;
        unsigned long long* key_out = s_key + (round & 1u) * (size_t)n;
        if (threadIdx.x == 0u) s_flag[(round + 1u) % 3u] = 0u;      // (the next round's; nobody looks at it during this one)
        for (uint32_t bits = fresh; bits; bits &= bits - 1u) {
            const uint32_t row = threadIdx.x + ((uint32_t)__ffs((int)bits) - 1u) * kClrWgThreads;
            ClearanceLdsOps::store_key(key_out + row, ClearanceLdsOps::load_key(key_in + row));
        }
        uint32_t found = 0u;
        // The thread's i-th pending row in the wave's i-th pass: as many passes as the busiest lane has rows left, few in the late rounds.
        // (Asking for the steps of three or five rows before looking at the first — one round trip to L2 instead of several — and
        //  walking fixed slots instead of set bits were both measured slower or equal on the site's middle: 79 / 131 against 75 us.)
        for (uint32_t bits = pending; bits; bits &= bits - 1u) {
            const uint32_t j = (uint32_t)__ffs((int)bits) - 1u, row = threadIdx.x + j * kClrWgThreads;
            const uint4 a = reinterpret_cast<const uint4*>(step)[2 * (size_t)row], b = reinterpret_cast<const uint4*>(step)[2 * (size_t)row + 1];
            const ClearanceStep st[4] = {{a.x, a.y}, {a.z, a.w}, {b.x, b.y}, {b.z, b.w}};
            const unsigned long long least = clearance_round_row<ClearanceLdsOps>(V, R, row, st, tall[row], key_in);
            if (least == kClrNoKey) continue;
            ClearanceLdsOps::store_key(key_out + row, clearance_relax(kClrNoKey, least));
            found |= 1u << j;
        }
        pending &= ~found;
        fresh = found;
        if (__any(found != 0u) && (threadIdx.x & 63u) == 0u) s_flag[round % 3u] = 1u;
        __syncthreads();
        last = round;
        if (s_flag[round % 3u] == 0u) break;            // (uniform: one word, read behind the barrier)
    }
    const unsigned long long* key = s_key + (last & 1u) * (size_t)n;
    ClearanceTally tl{0u, 0u, 0u};
    for (uint32_t row = threadIdx.x; row < n; row += kClrWgThreads) {
        uint32_t hp, nr;
        clearance_finish_row(ClearanceLdsOps::load_key(key + row), max_hops, hp, nr, tl);
        if (hops) hops[row] = hp;
        if (nearest) nearest[row] = nr;
    }
    clearance_flush(tl, counts);
}

}  // namespace gndt
#endif  // __HIPCC__
