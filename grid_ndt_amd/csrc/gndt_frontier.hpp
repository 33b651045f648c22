// gndt_frontier.hpp — frontier extraction (include/gndt.h "frontier extraction"): the slopes at which the known map ends, clustered
// into connected components on the device.  Every definition is integer or bit-pattern arithmetic, so the answer does not depend on
// the order in which threads work.
//   k_frontier_mark     rows -> parent[row] = row for a frontier row, kNoRow otherwise; its open sides       a candidate: 4 column probes
//   k_frontier_link     frontier rows -> lock-free union-find over parent (4 of the 8 neighbour columns each)   frontier rows only
//   k_frontier_flatten  frontier rows -> parent[row] = label[row] = root; members counted at the root          4 B a row
//   k_frontier_count    rows -> frontier rows, roots and listed roots per tile of kCropTile rows               8 B a row
//   k_frontier_scan     tile counts -> tile offsets of the listed roots, the call's four counts (one workgroup)
//   k_frontier_rank     roots -> place in the list; the listed clusters' records initialised                   8 B a row
//   k_frontier_reduce   frontier rows -> their cluster's record, integer atomics only                          frontier rows only
// Union-find: the larger root is always hooked under the smaller with a CAS, so parent[x] <= x holds throughout, a chain of parents
// strictly decreases (no cycle can form, a find ends after at most x steps) and every component's root ends as its smallest row: the
// label.  Finds use path halving; a halving store only ever names an ancestor, and a row that has stopped being a root never becomes
// one again, so plain stores to non-roots and CASes on roots do not disturb each other.
// The per-row logic is host-callable so that the CPU test tier runs the kernels' own code one row after another
// (tests/frontier_shim.cpp); memory operations go through an Ops policy (FrontierSerialOps here, FrontierDeviceOps with the kernels).
#pragma once
#include <stdint.h>

#include "gndt_query.hpp"
#include "gndt_scratch.hpp"

namespace gndt {

constexpr int kFrontierReached = 0, kFrontierSlopes = 1;            // GNDT_FRONTIER_REACHED / _SLOPES
constexpr int kFrontierOpenColumn = 0, kFrontierOpenLevel = 1;      // GNDT_FRONTIER_OPEN_COLUMN / _OPEN_LEVEL
constexpr uint32_t kFrontierNone = 0xFFu;                           // frontier_mark: not a frontier row
constexpr uint32_t kFrontierFltMax = 0x7F7FFFFFu;                   // best_h without a cost map

struct FrontierRule {
    int candidates, open_rule;
    uint32_t level_reach, min_open, link_dz;       // min_open: 1..4 (the entry point turns 0 into 1)
    int boxed, sx_min, sx_max, sy_min, sy_max;     // boxed 0: the whole map
};

// gndt_frontier as the kernels write it: best_row (low word) and best_h's bit pattern (high word) are one 64-bit word, so that one
// unsigned minimum picks the least h (h >= 0: its bit pattern orders like the number) and, among equal h, the smaller row
struct FrontierRecord {
    uint32_t label, size;
    unsigned long long best;
    int32_t sx_min, sx_max, sy_min, sy_max;
    long long sum_px, sum_py, sum_pz;
    uint32_t open_sides, reserved;
};
static_assert(sizeof(FrontierRecord) == 64, "gndt_frontier is 64 bytes");

// what one row, or several rows of one cluster combined, add to the cluster's record
struct FrontierSum {
    long long px, py, pz;
    int32_t sx_min, sx_max, sy_min, sy_max;
    unsigned long long best;
    uint32_t open;
};

// the position of a signed index on a line without the hole at 0
GNDT_HD int frontier_lin(int s) { return s > 0 ? s - 1 : s; }

// |lin(a) - lin(b)| <= reach (indices are below 2^21 in size: the difference cannot overflow)
GNDT_HD bool frontier_within(int a, int b, uint32_t reach) {
    const int d = frontier_lin(a) - frontier_lin(b);
    return (uint32_t)(d < 0 ? -d : d) <= reach;
}

GNDT_HD bool frontier_in_range(int sx, int sy) { return sx >= -kMaxXY && sx <= kMaxXY && sy >= -kMaxXY && sy <= kMaxXY; }

// Is the side of a slope at level sz towards column (nx, ny) open?  OPEN_COLUMN: the column is not in the map (an index beyond the
// codec's range is not).  OPEN_LEVEL: or it holds no node (any node: map_xy's view) within level_reach levels of sz.
GNDT_HD bool frontier_side_open(const QueryView& Q, const FrontierRule& F, int nx, int ny, int sz) {
    if (!frontier_in_range(nx, ny)) return true;
    const uint32_t c = ctab_find(Q.V, nx, ny);
    if (c == kNoColumn) return true;
    if (F.open_rule == kFrontierOpenColumn) return false;
    const uint32_t e = c + Q.V.row_ncol[c];
    for (uint32_t t = c; t < e; ++t)
        if (frontier_within(Q.V.sz[t], sz, F.level_reach)) return false;
    return true;
}

// The open sides (1..4) of a frontier row, kFrontierNone for every other row.  A candidate is a slope inside the box that, under
// REACHED, the flood expanded (state 1); it is a frontier row with at least min_open open sides.  Loads in the order that lets most
// rows stop early: flags, state, then the indices; only candidates probe the column index.
GNDT_HD uint32_t frontier_mark(const QueryView& Q, const FrontierRule& F, uint32_t row) {
    if (!(Q.V.flags[row] & 2u)) return kFrontierNone;
    if (F.candidates == kFrontierReached && Q.state[row] != 1u) return kFrontierNone;
    const int sx = Q.V.sx[row], sy = Q.V.sy[row];
    if (F.boxed && !(sx >= F.sx_min && sx <= F.sx_max && sy >= F.sy_min && sy <= F.sy_max)) return kFrontierNone;
    const int sz = Q.V.sz[row];
    uint32_t open = 0;
    open += frontier_side_open(Q, F, step_skip0(sx, -1), sy, sz) ? 1u : 0u;
    open += frontier_side_open(Q, F, step_skip0(sx, +1), sy, sz) ? 1u : 0u;
    open += frontier_side_open(Q, F, sx, step_skip0(sy, -1), sz) ? 1u : 0u;
    open += frontier_side_open(Q, F, sx, step_skip0(sy, +1), sz) ? 1u : 0u;
    return open >= F.min_open ? open : kFrontierNone;
}

// One thread after another (the CPU tier)
struct FrontierSerialOps {
    static inline uint32_t load(const uint32_t* p) { return *p; }
    static inline void store(uint32_t* p, uint32_t v) { *p = v; }
    static inline uint32_t cas(uint32_t* p, uint32_t expect, uint32_t v) { const uint32_t old = *p; if (old == expect) *p = v; return old; }
    static inline void add_u32(uint32_t* p, uint32_t v) { *p += v; }
    static inline void add_i64(long long* p, long long v) { *p += v; }
    static inline void min_i32(int32_t* p, int32_t v) { if (v < *p) *p = v; }
    static inline void max_i32(int32_t* p, int32_t v) { if (v > *p) *p = v; }
    static inline void min_u64(unsigned long long* p, unsigned long long v) { if (v < *p) *p = v; }
};

// The root of x, with path halving.  The chain strictly decreases, so it ends within x steps; the bound (n: the map's rows) is there
// because the device is shared and a loop on it must end whatever memory holds.
template <class Ops>
GNDT_HD uint32_t frontier_find(uint32_t* parent, uint32_t x, uint32_t n) {
    for (uint32_t step = 0; step < n; ++step) {
        const uint32_t p = Ops::load(parent + x);
        if (p == x || p >= n) return x;
        const uint32_t gp = Ops::load(parent + p);
        if (gp >= n) return p;
        if (gp != p) Ops::store(parent + x, gp);
        x = gp;
    }
    return x;
}

// The root of x without a store: the flatten pass, where the one store to parent[x] is its own thread's (a halving store of another
// thread, decided before that one, could otherwise land after it and leave an ancestor that is no root)
template <class Ops>
GNDT_HD uint32_t frontier_root(const uint32_t* parent, uint32_t x, uint32_t n) {
    for (uint32_t step = 0; step < n; ++step) {
        const uint32_t p = Ops::load(parent + x);
        if (p == x || p >= n) return x;
        x = p;
    }
    return x;
}

// Unite the sets of frontier rows a and b: the larger root goes under the smaller.  A CAS fails only because another thread hooked
// that root in the meantime (at most n - 1 hooks ever happen): retry from fresh finds, at most n times.
template <class Ops>
GNDT_HD void frontier_unite(uint32_t* parent, uint32_t a, uint32_t b, uint32_t n) {
    for (uint32_t tries = 0; tries < n; ++tries) {
        a = frontier_find<Ops>(parent, a, n);
        b = frontier_find<Ops>(parent, b, n);
        if (a == b) return;
        const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
        if (Ops::cas(parent + hi, hi, lo) == hi) return;
    }
}

// Frontier row a against the frontier rows of four of its eight neighbour columns — (+1, 0), (+1, +1), (0, +1), (-1, +1); the other
// four are the same pairs seen from the other row.  Whether a row is a frontier row (parent != kNoRow) never changes during the pass.
// after_unite(a, t): the CPU tier's look at the invariant.
template <class Ops, class AfterUnite>
GNDT_HD void frontier_link(const QueryView& Q, const FrontierRule& F, uint32_t* parent, uint32_t a, uint32_t n, AfterUnite after_unite) {
    const int sx = Q.V.sx[a], sy = Q.V.sy[a], sz = Q.V.sz[a];
    for (int k = 0; k < 4; ++k) {
        const int dx = k < 2 ? 1 : k == 2 ? 0 : -1, dy = k == 0 ? 0 : 1;
        const int nx = dx ? step_skip0(sx, dx) : sx, ny = dy ? step_skip0(sy, dy) : sy;
        if (!frontier_in_range(nx, ny)) continue;
        const uint32_t c = ctab_find(Q.V, nx, ny);
        if (c == kNoColumn) continue;
        const uint32_t e = c + Q.V.row_ncol[c];
        for (uint32_t t = c; t < e; ++t) {
            if (Ops::load(parent + t) == kNoRow) continue;
            if (!frontier_within(Q.V.sz[t], sz, F.link_dz)) continue;
            frontier_unite<Ops>(parent, a, t, n);
            after_unite(a, t);
        }
    }
}

struct FrontierNoLook { GNDT_HD void operator()(uint32_t, uint32_t) const {} };

// What frontier row `row` with `open` open sides adds to its cluster
GNDT_HD FrontierSum frontier_term(const QueryView& Q, const FrontierRule& F, uint32_t row, uint32_t open) {
    FrontierSum s;
    const int sx = Q.V.sx[row], sy = Q.V.sy[row];
    s.px = frontier_lin(sx); s.py = frontier_lin(sy); s.pz = frontier_lin(Q.V.sz[row]);
    s.sx_min = s.sx_max = sx; s.sy_min = s.sy_max = sy;
    const uint32_t hb = F.candidates == kFrontierReached ? Q.h_bits[row] : kFrontierFltMax;
    s.best = ((unsigned long long)hb << 32) | row;
    s.open = open;
    return s;
}

// The record of a cluster before its first member: label and size are known when the list is made
GNDT_HD FrontierRecord frontier_record_init(uint32_t label, uint32_t size) {
    FrontierRecord r;
    r.label = label; r.size = size; r.best = ~0ull;
    r.sx_min = r.sy_min = 0x7FFFFFFF; r.sx_max = r.sy_max = -0x7FFFFFFF - 1;
    r.sum_px = r.sum_py = r.sum_pz = 0;
    r.open_sides = 0u; r.reserved = 0u;
    return r;
}

// Integer sums, minima and maxima only: any order gives the same record
template <class Ops>
GNDT_HD void frontier_fold(FrontierRecord* r, const FrontierSum& s) {
    Ops::add_u32(&r->open_sides, s.open);
    Ops::add_i64(&r->sum_px, s.px); Ops::add_i64(&r->sum_py, s.py); Ops::add_i64(&r->sum_pz, s.pz);
    Ops::min_i32(&r->sx_min, s.sx_min); Ops::max_i32(&r->sx_max, s.sx_max);
    Ops::min_i32(&r->sy_min, s.sy_min); Ops::max_i32(&r->sy_max, s.sy_max);
    Ops::min_u64(&r->best, s.best);
}

// A call's scratch for a map of n rows in `tiles` tiles of the ordered compaction (gndt_api_frontier.hip)
struct FrontierScratch {
    uint32_t* parent;                // [n] the union-find
    uint32_t* size_at;               // [n] a root's member count, then its place in the list
    uint32_t* tile_cnt;              // [3 tiles]
    uint8_t* open;                   // [n] the open sides
    uint8_t* slack;                  // [16]
    FrontierScratch() = default;
    FrontierScratch(Carver& c, uint64_t n, uint64_t tiles)
        : parent(c.take<uint32_t>(n)), size_at(c.take<uint32_t>(n)), tile_cnt(c.take<uint32_t>(3 * tiles)), open(c.take<uint8_t>(n)),
          slack(c.take<uint8_t>(16)) {}
};

}  // namespace gndt

#if defined(__HIPCC__)
#include "gndt_crop.hpp"      // crop_block_scan, kCropT / kCropV / kCropTile: the ordered compaction of the crop

namespace gndt {

// Many threads: parent is read and written past the CU's cache (another CU's hook must be seen by the next find), the records take
// returning-nothing integer atomics
struct FrontierDeviceOps {
    static __device__ __forceinline__ uint32_t load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    static __device__ __forceinline__ void store(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    static __device__ __forceinline__ uint32_t cas(uint32_t* p, uint32_t expect, uint32_t v) { return atomicCAS(p, expect, v); }
    static __device__ __forceinline__ void add_u32(uint32_t* p, uint32_t v) { atomicAdd(p, v); }
    static __device__ __forceinline__ void add_i64(long long* p, long long v) { atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v); }
    static __device__ __forceinline__ void min_i32(int32_t* p, int32_t v) { atomicMin(p, v); }
    static __device__ __forceinline__ void max_i32(int32_t* p, int32_t v) { atomicMax(p, v); }
    static __device__ __forceinline__ void min_u64(unsigned long long* p, unsigned long long v) { atomicMin(p, v); }
};

// Every row: is it a frontier row, and how many of its sides are open.  size_at[row] = 0: the roots' member counts start here.
static __global__ void __launch_bounds__(256) k_frontier_mark(QueryView Q, FrontierRule F, uint32_t n, uint32_t* __restrict__ parent,
                                                              uint8_t* __restrict__ open, uint32_t* __restrict__ size_at) {
    const uint32_t gsz = gridDim.x * blockDim.x;
    for (uint64_t row = blockIdx.x * blockDim.x + threadIdx.x; row < n; row += gsz) {      // (64-bit: row + gsz cannot wrap)
        const uint32_t o = frontier_mark(Q, F, (uint32_t)row);
        parent[row] = o != kFrontierNone ? (uint32_t)row : kNoRow;
        open[row] = (uint8_t)o;
        size_at[row] = 0u;
    }
}

static __global__ void __launch_bounds__(256) k_frontier_link(QueryView Q, FrontierRule F, uint32_t n, uint32_t* __restrict__ parent) {
    const uint32_t gsz = gridDim.x * blockDim.x;
    for (uint64_t row = blockIdx.x * blockDim.x + threadIdx.x; row < n; row += gsz) {
        if (FrontierDeviceOps::load(parent + row) == kNoRow) continue;
        frontier_link<FrontierDeviceOps>(Q, F, parent, (uint32_t)row, n, FrontierNoLook{});
    }
}

// Every frontier row's parent becomes its root (written while other threads still walk through it: a root is an ancestor like any
// other; nobody else writes: frontier_root), the label goes out, and the roots count their members — rows of one wave that share a root first add up among themselves
// (a ring around a large map is one cluster of thousands of rows: one atomic a wave instead of 64 on one word).
static __global__ void __launch_bounds__(256) k_frontier_flatten(uint32_t n, uint32_t* __restrict__ parent, uint32_t* __restrict__ size_at,
                                                                 uint32_t* __restrict__ label) {
    const uint32_t gsz = gridDim.x * blockDim.x;
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t r0 = (uint64_t)blockIdx.x * blockDim.x; r0 < n; r0 += gsz) {      // (uniform over the workgroup: the ballots below)
        const uint64_t row = r0 + threadIdx.x;
        uint32_t root = kNoRow;
        if (row < n && FrontierDeviceOps::load(parent + row) != kNoRow) {
            root = frontier_root<FrontierDeviceOps>(parent, (uint32_t)row, n);
            if (root != (uint32_t)row) FrontierDeviceOps::store(parent + row, root);
        }
        if (label && row < n) label[row] = root;
        unsigned long long todo = __ballot(root != kNoRow);
        while (todo) {
            const uint32_t leader = (uint32_t)__ffsll((long long)todo) - 1u;
            const uint32_t lr = (uint32_t)__shfl((int)root, (int)leader, 64);
            const unsigned long long m = __ballot(root == lr);
            if (lane == leader) atomicAdd(size_at + lr, (uint32_t)__popcll(m));
            todo &= ~m;
        }
    }
}

// the frontier rows, roots and listed roots (size >= min_size) among this thread's kCropV rows from r0 on
__device__ __forceinline__ void frontier_tally(const uint32_t* __restrict__ parent, const uint32_t* __restrict__ size_at, uint32_t r0,
                                               uint32_t n, uint32_t min_size, uint32_t& rows, uint32_t& roots, uint32_t& listed_mask) {
    rows = roots = listed_mask = 0u;
#pragma unroll
    for (uint32_t j = 0; j < (uint32_t)kCropV; ++j) {
        const uint64_t r = (uint64_t)r0 + j;
        if (r >= n) break;
        const uint32_t p = parent[r];
        if (p == kNoRow) continue;
        ++rows;
        if (p != (uint32_t)r) continue;
        ++roots;
        if (size_at[r] >= min_size) listed_mask |= 1u << j;
    }
}

static __global__ void __launch_bounds__(kCropT) k_frontier_count(const uint32_t* __restrict__ parent, const uint32_t* __restrict__ size_at,
                                                                  uint32_t n, uint32_t min_size, uint32_t* __restrict__ tile_cnt) {
    const uint64_t r0 = (uint64_t)blockIdx.x * kCropTile + threadIdx.x * kCropV;
    uint32_t rows = 0, roots = 0, mask = 0;
    if (r0 < n) frontier_tally(parent, size_at, (uint32_t)r0, n, min_size, rows, roots, mask);
    uint32_t t_rows, t_roots, t_listed;
    (void)crop_block_scan<kCropT>(rows, &t_rows);
    (void)crop_block_scan<kCropT>(roots, &t_roots);
    (void)crop_block_scan<kCropT>((uint32_t)__popc(mask), &t_listed);
    if (threadIdx.x == 0) { tile_cnt[3 * blockIdx.x] = t_listed; tile_cnt[3 * blockIdx.x + 1] = t_rows; tile_cnt[3 * blockIdx.x + 2] = t_roots; }
}

// tile_cnt[3 t] -> exclusive offsets of the listed roots (in place); counts = {listed clusters, frontier rows, clusters, 0}
static __global__ void __launch_bounds__(kCropScanT) k_frontier_scan(uint32_t* __restrict__ tile_cnt, uint32_t tiles, uint32_t* __restrict__ counts) {
    uint32_t carry = 0, rows = 0, roots = 0;
    for (uint32_t base = 0; base < tiles; base += kCropScanT) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < tiles ? tile_cnt[3 * i] : 0u;
        uint32_t total, t_rows, t_roots;
        const uint32_t ex = crop_block_scan<kCropScanT>(v, &total);
        (void)crop_block_scan<kCropScanT>(i < tiles ? tile_cnt[3 * i + 1] : 0u, &t_rows);
        (void)crop_block_scan<kCropScanT>(i < tiles ? tile_cnt[3 * i + 2] : 0u, &t_roots);
        if (i < tiles) tile_cnt[3 * i] = carry + ex;
        carry += total; rows += t_rows; roots += t_roots;
    }
    if (threadIdx.x == 0) { counts[0] = carry; counts[1] = rows; counts[2] = roots; counts[3] = 0u; }
}

// Roots are in row order, so the listed ones' places are a prefix sum: size_at[root] becomes the cluster's place in the list (kNoRow:
// not listed, or beyond cluster_cap), and the listed clusters' records start as label, size and the identities of the reduction.
static __global__ void __launch_bounds__(kCropT) k_frontier_rank(const uint32_t* __restrict__ parent, uint32_t* __restrict__ size_at, uint32_t n,
                                                                 uint32_t min_size, const uint32_t* __restrict__ tile_cnt,
                                                                 FrontierRecord* __restrict__ clusters, uint32_t cluster_cap) {
    const uint64_t r0 = (uint64_t)blockIdx.x * kCropTile + threadIdx.x * kCropV;
    uint32_t rows = 0, roots = 0, mask = 0;
    if (r0 < n) frontier_tally(parent, size_at, (uint32_t)r0, n, min_size, rows, roots, mask);
    uint32_t total;
    uint32_t place = tile_cnt[3 * blockIdx.x] + crop_block_scan<kCropT>((uint32_t)__popc(mask), &total);
#pragma unroll
    for (uint32_t j = 0; j < (uint32_t)kCropV; ++j) {
        const uint64_t r = r0 + j;
        if (r >= n || parent[r] != (uint32_t)r) continue;
        uint32_t at = kNoRow;
        if (mask & (1u << j)) {
            if (place < cluster_cap) {
                at = place;
                clusters[place] = frontier_record_init((uint32_t)r, size_at[r]);
            }
            ++place;
        }
        size_at[r] = at;
    }
}

__device__ __forceinline__ long long frontier_shfl_xor(long long v, int o) { return __shfl_xor(v, o, 64); }

// Every frontier row of a listed cluster -> the cluster's record.  Rows of one wave that share a cluster are combined first (four or
// more of them: one butterfly over the wave with the identities in the other lanes, one lane's atomics; fewer: their own atomics).
static __global__ void __launch_bounds__(256) k_frontier_reduce(QueryView Q, FrontierRule F, uint32_t n, const uint32_t* __restrict__ parent,
                                                                const uint32_t* __restrict__ place_at, const uint8_t* __restrict__ open,
                                                                FrontierRecord* __restrict__ clusters) {
    const uint32_t gsz = gridDim.x * blockDim.x;
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t r0 = (uint64_t)blockIdx.x * blockDim.x; r0 < n; r0 += gsz) {      // (uniform: ballots and shuffles below)
        const uint64_t row = r0 + threadIdx.x;
        uint32_t at = kNoRow;
        if (row < n) {
            const uint32_t root = parent[row];
            if (root != kNoRow) at = place_at[root];
        }
        FrontierSum s{};
        if (at != kNoRow) s = frontier_term(Q, F, (uint32_t)row, open[row]);
        unsigned long long todo = __ballot(at != kNoRow);
        while (todo) {
            const uint32_t leader = (uint32_t)__ffsll((long long)todo) - 1u;
            const uint32_t la = (uint32_t)__shfl((int)at, (int)leader, 64);
            const bool mine = at == la;
            const unsigned long long m = __ballot(mine);
            todo &= ~m;
            if (__popcll(m) < 4) {
                if (mine) frontier_fold<FrontierDeviceOps>(clusters + la, s);
                continue;
            }
            FrontierSum t = s;
            if (!mine) {
                t.px = t.py = t.pz = 0; t.open = 0u; t.best = ~0ull;
                t.sx_min = t.sy_min = 0x7FFFFFFF; t.sx_max = t.sy_max = -0x7FFFFFFF - 1;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                t.px += frontier_shfl_xor(t.px, o); t.py += frontier_shfl_xor(t.py, o); t.pz += frontier_shfl_xor(t.pz, o);
                t.open += (uint32_t)__shfl_xor((int)t.open, o, 64);
                t.sx_min = min(t.sx_min, __shfl_xor(t.sx_min, o, 64)); t.sx_max = max(t.sx_max, __shfl_xor(t.sx_max, o, 64));
                t.sy_min = min(t.sy_min, __shfl_xor(t.sy_min, o, 64)); t.sy_max = max(t.sy_max, __shfl_xor(t.sy_max, o, 64));
                const unsigned long long ob = (unsigned long long)frontier_shfl_xor((long long)t.best, o);
                t.best = ob < t.best ? ob : t.best;
            }
            if (lane == leader) frontier_fold<FrontierDeviceOps>(clusters + la, t);
        }
    }
}

}  // namespace gndt
#endif  // __HIPCC__
