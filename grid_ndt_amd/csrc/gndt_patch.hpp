// gndt_patch.hpp — surface patches (include/gndt.h "surface patches"): the map's nodes grown into planes over their normals and means,
// each patch with its bounds, its members merged as Gaussians and the plane fitted to them.  Labels, counts and every integer field are
// integer or bit-pattern arithmetic (the link rule is fp32, one rounded operation at a time): exact in any thread order.  The plane
// fields come from fp64 sums added with atomics: reproducible to fp64 rounding only.
//   k_patch_mark      rows -> parent[row] = row for a candidate, kNoRow otherwise                                 12 B a row, 16 a candidate
//   k_patch_link      candidates -> lock-free union-find (gndt_frontier.hpp's) over 13 of the 26 neighbour keys   5 column probes each
//   k_frontier_flatten / _count / _scan   the frontiers' own: roots, member counts, tile counts, the four counts
//   k_patch_rank      roots -> place in the list; the listed patches' records and ten sums initialised            8 B a row
//   k_patch_reduce    candidates -> their patch's integer fields, lanes of one patch combined in the wave first, carried over the loop
//   k_patch_moments   candidates -> their patch's ten fp64 sums: lanes of one patch combined in the wave, the waves of a workgroup in
//                     LDS (kPatchSlots tagged slots), one set of global atomics a slot and workgroup
//   k_patch_fit       listed patches -> centroid, normal, var, kind (one thread each: the fp64 eigen solve)
// The per-row logic is host-callable (tests/patch_shim.cpp runs it one row after another); memory operations go through the frontiers'
// Ops policies.
#pragma once
#include <stdint.h>

#include "gndt_coarsen.hpp"      // coarsen_sums: a node's statistics moved to another reference point
#include "gndt_frontier.hpp"
#include "gndt_score.hpp"        // ScoreView: the query view with count and cov

namespace gndt {

constexpr int kPatchNodes = 0, kPatchSlopes = 1;                            // GNDT_PATCH_NODES / _SLOPES
constexpr uint32_t kPatchHorizontal = 1u, kPatchVertical = 2u, kPatchInclined = 4u, kPatchSlopesOnly = 8u;     // GNDT_PATCH_*
constexpr int kPatchMoments = 10;                                           // N, S1 (3), S2 (xx xy xz yy yz zz)

struct PatchRule {
    int candidates;
    uint32_t connectivity;                         // 1..3 (the entry point turns 0 into 3)
    float cos_min, max_offset, max_var;
    double cos_level, sin_level;                   // the params' floats, widened
    int boxed, sx_min, sx_max, sy_min, sy_max;     // boxed 0: the whole map
};

struct PatchRecord {             // gndt_patch
    uint32_t label, nodes;
    unsigned long long points;
    int32_t sx_min, sx_max, sy_min, sy_max, sz_min, sz_max;
    long long sum_px, sum_py, sum_pz;
    double centroid[3], normal[3], var;
    uint32_t kind, reserved;     // kind holds the members that are slopes between k_patch_reduce and k_patch_fit
};
static_assert(sizeof(PatchRecord) == 128, "gndt_patch is 128 bytes");

// what one row, or several rows of one patch combined, add to the patch's integer fields
struct PatchSum {
    long long px, py, pz;
    unsigned long long points;
    int32_t sx_min, sx_max, sy_min, sy_max, sz_min, sz_max;
    uint32_t slopes;
};

// Is the row a candidate?  Loads in the order that lets most rows stop early.  rough is the stored value (0 -> 0.01 included).
GNDT_HD bool patch_mark(const ScoreView& S, const PatchRule& F, uint32_t row) {
    const CostView& V = S.Q.V;
    const uint32_t fl = V.flags[row];
    if (!(fl & 1u)) return false;
    if (F.candidates == kPatchSlopes && !(fl & 2u)) return false;
    if (F.boxed) {
        const int sx = V.sx[row], sy = V.sy[row];
        if (!(sx >= F.sx_min && sx <= F.sx_max && sy >= F.sy_min && sy <= F.sy_max)) return false;
    }
    const float room = F.max_var * (float)S.count[row];
    return V.rough[row] <= room;
}

// The link rule between candidates a and b (adjacency is the caller's).  fp32, one rounded operation after the other in the order of
// include/gndt.h (the library and the host shim are built with contraction off); symmetric to the bit: d is exactly antisymmetric.
GNDT_HD bool patch_links(const CostView& V, const PatchRule& F, uint32_t a, uint32_t b) {
    GNDT_FP_STRICT
    const float* na = V.normal + 3 * (size_t)a;
    const float* nb = V.normal + 3 * (size_t)b;
    const float c = (na[0] * nb[0] + na[1] * nb[1]) + na[2] * nb[2];
    if (!(fabsf(c) >= F.cos_min)) return false;
    const float* ma = V.mean + 3 * (size_t)a;
    const float* mb = V.mean + 3 * (size_t)b;
    const float dx = mb[0] - ma[0], dy = mb[1] - ma[1], dz = mb[2] - ma[2];
    const float ea = fabsf((na[0] * dx + na[1] * dy) + na[2] * dz);
    const float eb = fabsf((nb[0] * dx + nb[1] * dy) + nb[2] * dz);
    return ea <= F.max_offset && eb <= F.max_offset;
}

// Candidate a against the candidates at 13 of its 26 neighbour keys — the columns (+1, 0), (+1, +1), (0, +1), (-1, +1) at the levels
// -1, 0, +1 and its own column one level up; the other 13 are the same pairs seen from the other row.  Whether a row is a candidate
// (parent != kNoRow) never changes during the pass.  after_unite(a, t): the CPU tier's look at the invariant.
template <class Ops, class AfterUnite>
GNDT_HD void patch_link(const ScoreView& S, const PatchRule& F, uint32_t* parent, uint32_t a, uint32_t n, AfterUnite after_unite) {
    const CostView& V = S.Q.V;
    const int sx = V.sx[a], sy = V.sy[a], sz = V.sz[a];
    const int la = frontier_lin(sz);
    for (int k = 0; k < 5; ++k) {
        const int dx = k == 0 ? 0 : k < 3 ? 1 : k == 3 ? 0 : -1, dy = k == 0 ? 0 : k == 1 ? 0 : 1;
        const uint32_t axes_xy = (dx ? 1u : 0u) + (dy ? 1u : 0u);
        if (axes_xy > F.connectivity) continue;
        const int nx = dx ? step_skip0(sx, dx) : sx, ny = dy ? step_skip0(sy, dy) : sy;
        if (!frontier_in_range(nx, ny)) continue;
        const uint32_t c = ctab_find(V, nx, ny);
        if (c == kNoColumn) continue;
        const uint32_t e = c + V.row_ncol[c];
        for (uint32_t t = c; t < e; ++t) {
            const int dl = frontier_lin(V.sz[t]) - la;
            if (k == 0 ? dl != 1 : (dl < -1 || dl > 1)) continue;
            if (axes_xy + (dl ? 1u : 0u) > F.connectivity) continue;
            if (Ops::load(parent + t) == kNoRow) continue;
            if (!patch_links(V, F, a, t)) continue;
            frontier_unite<Ops>(parent, a, t, n);
            after_unite(a, t);
        }
    }
}

// What candidate `row` adds to its patch's integer fields
GNDT_HD PatchSum patch_term(const ScoreView& S, uint32_t row) {
    const CostView& V = S.Q.V;
    PatchSum s;
    const int sx = V.sx[row], sy = V.sy[row], sz = V.sz[row];
    s.px = frontier_lin(sx); s.py = frontier_lin(sy); s.pz = frontier_lin(sz);
    s.points = S.count[row];
    s.sx_min = s.sx_max = sx; s.sy_min = s.sy_max = sy; s.sz_min = s.sz_max = sz;
    s.slopes = (V.flags[row] & 2u) ? 1u : 0u;
    return s;
}

// the identity of the integer reduction
GNDT_HD PatchSum patch_sum_none() {
    PatchSum s;
    s.px = s.py = s.pz = 0; s.points = 0ull; s.slopes = 0u;
    s.sx_min = s.sy_min = s.sz_min = 0x7FFFFFFF; s.sx_max = s.sy_max = s.sz_max = -0x7FFFFFFF - 1;
    return s;
}

// The record of a patch before its first member: label and nodes are known when the list is made; the plane fields are k_patch_fit's
GNDT_HD PatchRecord patch_record_init(uint32_t label, uint32_t nodes) {
    PatchRecord r;
    const PatchSum z = patch_sum_none();
    r.label = label; r.nodes = nodes; r.points = 0ull;
    r.sx_min = z.sx_min; r.sx_max = z.sx_max; r.sy_min = z.sy_min; r.sy_max = z.sy_max; r.sz_min = z.sz_min; r.sz_max = z.sz_max;
    r.sum_px = r.sum_py = r.sum_pz = 0;
    for (int a = 0; a < 3; ++a) r.centroid[a] = r.normal[a] = 0.0;
    r.var = 0.0;
    r.kind = 0u; r.reserved = 0u;
    return r;
}

// Integer sums, minima and maxima only: any order gives the same record
template <class Ops>
GNDT_HD void patch_fold(PatchRecord* r, const PatchSum& s) {
    Ops::add_i64(reinterpret_cast<long long*>(&r->points), (long long)s.points);
    Ops::add_i64(&r->sum_px, s.px); Ops::add_i64(&r->sum_py, s.py); Ops::add_i64(&r->sum_pz, s.pz);
    Ops::min_i32(&r->sx_min, s.sx_min); Ops::max_i32(&r->sx_max, s.sx_max);
    Ops::min_i32(&r->sy_min, s.sy_min); Ops::max_i32(&r->sy_max, s.sy_max);
    Ops::min_i32(&r->sz_min, s.sz_min); Ops::max_i32(&r->sz_max, s.sz_max);
    Ops::add_u32(&r->kind, s.slopes);
}

// The ten sums candidate `row` adds to the patch whose label row is `ref`: the node as a Gaussian (count, mean, stored scatter about
// its mean) moved to the label row's mean by the coarsening's moment match — out[0] = count, out[1..3] = count d, out[4..9] = scatter +
// count d d^T with d = mean - mean_ref in fp64
GNDT_HD void patch_moments(const ScoreView& S, uint32_t row, uint32_t ref, double out[kPatchMoments]) {
    const float* m = S.Q.V.mean + 3 * (size_t)row;
    const float* r = S.Q.V.mean + 3 * (size_t)ref;
    const float* cv = S.cov + 6 * (size_t)row;
    const uint32_t cnt = S.count[row];
    const double d[3] = {(double)m[0] - (double)r[0], (double)m[1] - (double)r[1], (double)m[2] - (double)r[2]};
    const double sums[9] = {0.0, 0.0, 0.0, (double)cv[0], (double)cv[1], (double)cv[2], (double)cv[3], (double)cv[4], (double)cv[5]};
    out[0] = (double)cnt;
    coarsen_sums(cnt, sums, d, out + 1);
}

// The plane of a patch from its ten sums about `ref` (the label row's mean) and the slope tally the reduction left in kind
GNDT_HD void patch_fit(const PatchRule& F, const double q[kPatchMoments], const float* ref, PatchRecord* r) {
    const double N = q[0];
    const double m[3] = {q[1] / N, q[2] / N, q[3] / N};
    const double C[6] = {q[4] - q[1] * m[0], q[5] - q[1] * m[1], q[6] - q[1] * m[2], q[7] - q[2] * m[1], q[8] - q[2] * m[2], q[9] - q[3] * m[2]};
    double lam, v[3];
    min_eigenpair_sym3<false>(C, lam, v);       // (no fp32 trigonometric start value: nothing but +, x, / and sqrt in fp64)
    if (v[2] < 0.0 || (v[2] == 0.0 && (v[1] < 0.0 || (v[1] == 0.0 && v[0] < 0.0)))) { v[0] = -v[0]; v[1] = -v[1]; v[2] = -v[2]; }
    for (int a = 0; a < 3; ++a) { r->centroid[a] = (double)ref[a] + m[a]; r->normal[a] = v[a]; }
    r->var = (lam > 0.0 ? lam : 0.0) / N;
    const double az = fabs(v[2]);
    uint32_t kind = az >= F.cos_level ? kPatchHorizontal : az <= F.sin_level ? kPatchVertical : kPatchInclined;
    if (r->kind == r->nodes) kind |= kPatchSlopesOnly;
    r->kind = kind;
}

// A call's scratch for a map of n rows in `tiles` tiles and a list of `cap` patches (gndt_api_patch.hip)
struct PatchScratch {
    double* moments;                 // [10 cap] the listed patches' fp64 sums
    uint32_t* parent;                // [n] the union-find
    uint32_t* size_at;               // [n] a root's member count, then its place in the list
    uint32_t* tile_cnt;              // [3 tiles]
    uint32_t* slack;                 // [4]
    PatchScratch() = default;
    PatchScratch(Carver& c, uint64_t n, uint64_t tiles, uint64_t cap)
        : moments(c.take<double>((uint64_t)kPatchMoments * cap)), parent(c.take<uint32_t>(n)), size_at(c.take<uint32_t>(n)),
          tile_cnt(c.take<uint32_t>(3 * tiles)), slack(c.take<uint32_t>(4)) {}
};

}  // namespace gndt

#if defined(__HIPCC__)

namespace gndt {

constexpr uint32_t kPatchSlots = 8;              // k_patch_moments: tagged LDS slots of a workgroup (a power of two)
constexpr uint32_t kPatchWaveMin = 4;            // rows of one patch in a wave from which they are combined before the atomics

static __global__ void __launch_bounds__(256) k_patch_mark(ScoreView S, PatchRule F, uint32_t n, uint32_t* __restrict__ parent,
                                                           uint32_t* __restrict__ size_at) {
    const uint32_t gsz = gridDim.x * blockDim.x;
    for (uint64_t row = blockIdx.x * blockDim.x + threadIdx.x; row < n; row += gsz) {      // (64-bit: row + gsz cannot wrap)
        parent[row] = patch_mark(S, F, (uint32_t)row) ? (uint32_t)row : kNoRow;
        size_at[row] = 0u;
    }
}

static __global__ void __launch_bounds__(256) k_patch_link(ScoreView S, PatchRule F, uint32_t n, uint32_t* __restrict__ parent) {
    const uint32_t gsz = gridDim.x * blockDim.x;
    for (uint64_t row = blockIdx.x * blockDim.x + threadIdx.x; row < n; row += gsz) {
        if (FrontierDeviceOps::load(parent + row) == kNoRow) continue;
        patch_link<FrontierDeviceOps>(S, F, parent, (uint32_t)row, n, FrontierNoLook{});
    }
}

// k_frontier_rank for the patches' records: size_at[root] becomes the patch's place in the list (kNoRow: not listed, or beyond
// patch_cap); a listed patch's record starts as label, nodes and the identities of the reduction, its ten sums as zeros
static __global__ void __launch_bounds__(kCropT) k_patch_rank(const uint32_t* __restrict__ parent, uint32_t* __restrict__ size_at, uint32_t n,
                                                              uint32_t min_size, const uint32_t* __restrict__ tile_cnt,
                                                              PatchRecord* __restrict__ patches, double* __restrict__ moments, uint32_t patch_cap) {
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
            if (place < patch_cap) {
                at = place;
                patches[place] = patch_record_init((uint32_t)r, size_at[r]);
#pragma unroll
                for (int k = 0; k < kPatchMoments; ++k) moments[(size_t)kPatchMoments * place + k] = 0.0;
            }
            ++place;
        }
        size_at[r] = at;
    }
}

// b joins a (both sums of rows of one patch)
__device__ __forceinline__ void patch_sum_join(PatchSum& a, const PatchSum& b) {
    a.px += b.px; a.py += b.py; a.pz += b.pz; a.points += b.points; a.slopes += b.slopes;
    a.sx_min = min(a.sx_min, b.sx_min); a.sx_max = max(a.sx_max, b.sx_max);
    a.sy_min = min(a.sy_min, b.sy_min); a.sy_max = max(a.sy_max, b.sy_max);
    a.sz_min = min(a.sz_min, b.sz_min); a.sz_max = max(a.sz_max, b.sz_max);
}

// Every candidate of a listed patch -> the patch's integer fields, as k_frontier_reduce does it: rows of one wave that share a patch are
// combined first (kPatchWaveMin or more of them: one butterfly over the wave with the identities in the other lanes; fewer: their own
// atomics).  A combined sum is not sent at once: the wave carries it (it is the same in every lane) while the next combined sum is the
// same patch's, over the trips of its loop, and sends it when another patch comes or the loop ends — on a floor that owns the map a
// wave's eleven atomics go out once, not once a trip (one record took 1.4 ms of them on an 803 k-row plane; the launch is 512
// workgroups for that).  Integer sums, minima and maxima: the record does not depend on who carried what.
static __global__ void __launch_bounds__(256) k_patch_reduce(ScoreView S, uint32_t n, const uint32_t* __restrict__ parent,
                                                             const uint32_t* __restrict__ place_at, PatchRecord* __restrict__ patches) {
    const uint32_t gsz = gridDim.x * blockDim.x;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t carry_at = kNoRow;
    PatchSum carry = patch_sum_none();
    for (uint64_t r0 = (uint64_t)blockIdx.x * blockDim.x; r0 < n; r0 += gsz) {      // (uniform: ballots and shuffles below)
        const uint64_t row = r0 + threadIdx.x;
        uint32_t at = kNoRow;
        if (row < n) {
            const uint32_t root = parent[row];
            if (root != kNoRow) at = place_at[root];
        }
        PatchSum s = patch_sum_none();
        if (at != kNoRow) s = patch_term(S, (uint32_t)row);
        unsigned long long todo = __ballot(at != kNoRow);
        while (todo) {
            const uint32_t leader = (uint32_t)__ffsll((long long)todo) - 1u;
            const uint32_t la = (uint32_t)__shfl((int)at, (int)leader, 64);
            const bool mine = at == la;
            const unsigned long long m = __ballot(mine);
            todo &= ~m;
            if ((uint32_t)__popcll(m) < kPatchWaveMin) {
                if (mine) patch_fold<FrontierDeviceOps>(patches + la, s);
                continue;
            }
            PatchSum t = mine ? s : patch_sum_none();
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                t.px += frontier_shfl_xor(t.px, o); t.py += frontier_shfl_xor(t.py, o); t.pz += frontier_shfl_xor(t.pz, o);
                t.points += (unsigned long long)frontier_shfl_xor((long long)t.points, o);
                t.slopes += (uint32_t)__shfl_xor((int)t.slopes, o, 64);
                t.sx_min = min(t.sx_min, __shfl_xor(t.sx_min, o, 64)); t.sx_max = max(t.sx_max, __shfl_xor(t.sx_max, o, 64));
                t.sy_min = min(t.sy_min, __shfl_xor(t.sy_min, o, 64)); t.sy_max = max(t.sy_max, __shfl_xor(t.sy_max, o, 64));
                t.sz_min = min(t.sz_min, __shfl_xor(t.sz_min, o, 64)); t.sz_max = max(t.sz_max, __shfl_xor(t.sz_max, o, 64));
            }
            if (la == carry_at) { patch_sum_join(carry, t); continue; }      // (la, carry_at and t are the same in every lane)
            if (carry_at != kNoRow && lane == 0) patch_fold<FrontierDeviceOps>(patches + carry_at, carry);
            carry_at = la;
            carry = t;
        }
    }
    if (carry_at != kNoRow && lane == 0) patch_fold<FrontierDeviceOps>(patches + carry_at, carry);
}

// Every candidate of a listed patch -> the patch's ten fp64 sums.  On a warehouse floor one patch owns most rows, and every wave's ten
// atomics would queue at one record: rows of one wave that share a patch are combined first (as above), and with LDS the waves of a
// workgroup then meet in one of kPatchSlots tagged LDS slots (slot = place mod kPatchSlots, claimed by the first wave that comes with a
// CAS on its tag; a wave whose slot is another patch's goes to memory itself), which the workgroup sends to memory once, behind its
// loop: ten atomics a workgroup and patch instead of ten a wave.
template <bool LDS>
static __global__ void __launch_bounds__(256) k_patch_moments(ScoreView S, uint32_t n, const uint32_t* __restrict__ parent,
                                                              const uint32_t* __restrict__ place_at, double* __restrict__ moments) {
    __shared__ uint32_t s_tag[kPatchSlots];
    __shared__ double s_sum[kPatchSlots][kPatchMoments];
    if (LDS) {
        if (threadIdx.x < kPatchSlots) s_tag[threadIdx.x] = kNoRow;
        if (threadIdx.x < kPatchSlots * kPatchMoments) (&s_sum[0][0])[threadIdx.x] = 0.0;
        __syncthreads();
    }
    const uint32_t gsz = gridDim.x * blockDim.x;
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t r0 = (uint64_t)blockIdx.x * blockDim.x; r0 < n; r0 += gsz) {      // (uniform: ballots and shuffles below)
        const uint64_t row = r0 + threadIdx.x;
        uint32_t at = kNoRow, root = kNoRow;
        if (row < n) {
            root = parent[row];
            if (root != kNoRow) at = place_at[root];
        }
        double q[kPatchMoments];
#pragma unroll
        for (int k = 0; k < kPatchMoments; ++k) q[k] = 0.0;
        if (at != kNoRow) patch_moments(S, (uint32_t)row, root, q);
        unsigned long long todo = __ballot(at != kNoRow);
        while (todo) {
            const uint32_t leader = (uint32_t)__ffsll((long long)todo) - 1u;
            const uint32_t la = (uint32_t)__shfl((int)at, (int)leader, 64);
            const bool mine = at == la;
            const unsigned long long m = __ballot(mine);
            todo &= ~m;
            double* dst = moments + (size_t)kPatchMoments * la;
            if ((uint32_t)__popcll(m) < kPatchWaveMin) {
                if (mine) {
#pragma unroll
                    for (int k = 0; k < kPatchMoments; ++k) unsafeAtomicAdd(dst + k, q[k]);
                }
                continue;
            }
            double t[kPatchMoments];
#pragma unroll
            for (int k = 0; k < kPatchMoments; ++k) t[k] = mine ? q[k] : 0.0;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
                for (int k = 0; k < kPatchMoments; ++k) t[k] += __shfl_xor(t[k], o, 64);
            }
            if (lane != leader) continue;
            bool in_lds = false;
            if (LDS) {
                const uint32_t slot = la & (kPatchSlots - 1u);
                const uint32_t old = atomicCAS(&s_tag[slot], kNoRow, la);
                in_lds = old == kNoRow || old == la;
                if (in_lds) {
#pragma unroll
                    for (int k = 0; k < kPatchMoments; ++k) atomicAdd(&s_sum[slot][k], t[k]);
                }
            }
            if (!in_lds) {
#pragma unroll
                for (int k = 0; k < kPatchMoments; ++k) unsafeAtomicAdd(dst + k, t[k]);
            }
        }
    }
    if (LDS) {
        __syncthreads();
        if (threadIdx.x < kPatchSlots * kPatchMoments) {
            const uint32_t slot = threadIdx.x / kPatchMoments, k = threadIdx.x - slot * kPatchMoments;
            const uint32_t tag = s_tag[slot];
            if (tag != kNoRow) unsafeAtomicAdd(moments + (size_t)kPatchMoments * tag + k, s_sum[slot][k]);
        }
    }
}

// One thread per listed patch (counts[0] of them, at most patch_cap): the plane from the ten sums
static __global__ void __launch_bounds__(64) k_patch_fit(ScoreView S, PatchRule F, const uint32_t* __restrict__ counts, uint32_t patch_cap,
                                                         const double* __restrict__ moments, PatchRecord* __restrict__ patches) {
    const uint32_t listed = min(counts[0], patch_cap);
    const uint32_t gsz = gridDim.x * blockDim.x;
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < listed; p += gsz) {
        double q[kPatchMoments];
#pragma unroll
        for (int k = 0; k < kPatchMoments; ++k) q[k] = moments[(size_t)kPatchMoments * p + k];
        patch_fit(F, q, S.Q.V.mean + 3 * (size_t)patches[p].label, patches + p);
    }
}

}  // namespace gndt
#endif  // __HIPCC__
