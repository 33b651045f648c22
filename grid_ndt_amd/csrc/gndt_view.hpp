// gndt_view.hpp — view gain (include/gndt.h "view gain"): how many columns that are not in the map a sensor's fan of rays would cross
// from each of K poses before something stops them.
//
// A ray is ray casting's (gndt_cast.hpp) in VOXEL mode, from float32(t) to the end point view_end forms from the pose and a direction of
// the sensor frame; the walk is the cast's loop with one thing added per column visit: the column is marked in one of two bitmaps, by
// the answer of the probe the cast makes anyway (kNoColumn: unknown, else known).  The bitmaps cover the window of columns a ray of
// the pose can be handed (view_reach) and belong to the pose: one workgroup per pose, both bitmaps in LDS, rays strided over the
// workgroup's threads.  A mark reads its word first and sends the atomic OR only when the bit is clear (all rays of a fan start in
// the same column; gndt_ray.hpp's clear_pass does the same); the thread whose OR returns the word with the bit clear owns the column
// and counts it.  Counts and the two coordinate sums are integers: wave shuffles, one LDS slot per wave, one thread into the record;
// no floating-point sum and no global atomic, so the record is the same whatever the block size and the order of the rays.
// Everything per ray is callable on the host as well (tests/view_shim.cpp: the mark with a plain OR).
#pragma once
#include <math.h>
#include <stdint.h>

#include "gndt_cast.hpp"

namespace gndt {

constexpr uint32_t kViewLdsBytes = 160u * 1024u;       // the CU's LDS: what one workgroup can be granted
constexpr uint32_t kViewLdsDefault = 64u * 1024u;      // dynamic LDS a launch gets without asking (lds_granted beyond)
constexpr uint32_t kViewMaxThreads = 1024u;
constexpr uint32_t kViewTallies = 8u;                  // rays, skipped, hits, unknown, known, steps, sum_ux, sum_uy
constexpr uint32_t kViewLdsTail = (kViewMaxThreads / 64u) * kViewTallies * 8u;     // bytes behind the bitmaps: a slot per wave and tally

struct ViewRule {                    // gndt_view_params with the defaults filled in, and the window
    uint32_t min_count;
    double min_range;
    float max_range;
    uint32_t reach;                  // the window holds the columns within `reach` of the origin's, W = 2 reach + 1 a side
    uint32_t words;                  // words of one bitmap: ceil(W * W / 32)
};

struct ViewInfo {                    // gndt_view_info
    uint32_t rays, skipped, hits, unknown, known, status;
    uint64_t steps;
    int64_t sum_ux, sum_uy;
};

struct ViewTally {                   // what one thread (one wave, one pose) has counted
    unsigned long long v[kViewTallies];
};
enum { kViewRays = 0, kViewSkipped, kViewHits, kViewUnknown, kViewKnown, kViewSteps, kViewSumX, kViewSumY };

// Columns between the origin's column and the farthest a ray can be handed, on either axis.  The cut point lies within max_range of
// the origin, so its cell is at most ceil(max_range / grid_len) cells from the origin's and the walk stays between the two; one more
// for the float32 rounding of the cut point.
GNDT_HD uint32_t view_reach(float max_range, float grid_len) {
    const double r = ceil((double)max_range / (double)grid_len) + 1.0;
    return r < 4294967295.0 ? (uint32_t)r : 0xFFFFFFFFu;
}

// Words of one bitmap of the window of `reach` (64-bit: a reach that does not fit anything still has a size)
GNDT_HD uint64_t view_words(uint32_t reach) {
    const uint64_t W = 2ull * reach + 1ull;
    return (W * W + 31ull) >> 5;
}

// LDS of a launch: the two bitmaps and the tail
GNDT_HD uint64_t view_lds_bytes(uint32_t reach) { return 2ull * 4ull * view_words(reach) + kViewLdsTail; }

// The largest reach whose launch fits `bytes` of LDS
inline uint32_t view_max_reach(uint32_t bytes) {
    uint32_t r = 0;
    while (view_lds_bytes(r + 1u) <= bytes) ++r;
    return r;
}

// The end point of direction (x, y, z) of the sensor frame under the pose T (row-major 3 x 4 [R | t], fp64): cast_scan's expression
GNDT_HD void view_end(const double* T, float x, float y, float z, float max_range, float e[3]) {
    const double dx = (double)x, dy = (double)y, dz = (double)z, R = (double)max_range;
    for (int a = 0; a < 3; ++a) e[a] = (float)(T[4 * a + 3] + R * ((T[4 * a] * dx + T[4 * a + 1] * dy) + T[4 * a + 2] * dz));
}

// Bit `bit` of a bitmap: true for the one caller that set it.  or_(word pointer, mask) -> the word before (atomic on the device).
template <typename OR>
GNDT_HD bool view_mark(uint32_t* words, uint32_t bit, const OR& or_) {
    uint32_t* w = words + (bit >> 5);
    const uint32_t m = 1u << (bit & 31u);
    if (*w & m) return false;
    return !(or_(w, m) & m);
}

// One ray of a pose whose origin (ox, oy, oz) stands in the cell (lx0, ly0): the cast's walk, every column handed out marked in
// known / unknown (a column outside the window is not marked: it cannot be handed, view_reach) -> the cast's outcome, res filled on a hit
template <typename OR>
GNDT_HD int view_ray(const ScoreView& S, const CastParams& P, const RayGrid& G, const ViewRule& F, int lx0, int ly0, float ox, float oy, float oz,
                     const float e[3], uint32_t* known, uint32_t* unknown, const OR& or_, ViewTally& t, CastResult& res) {
    RayWalk w;
    if (!ray_begin(G, ox, oy, oz, e[0], e[1], e[2], w)) return kCastSkipped;
    const uint32_t W = 2u * F.reach + 1u;
    RayColumn rc;
    RayCross x;
    double t_in = 0.0;
    while (ray_next(G, w, rc, x)) {
        ++t.v[kViewSteps];
        uint32_t ncol;
        const uint32_t c = clear_column<false>(S.Q, nullptr, rc, ncol);
        const int lx = ray_lin(rc.sx), ly = ray_lin(rc.sy);
        const uint32_t wx = (uint32_t)(lx - lx0) + F.reach, wy = (uint32_t)(ly - ly0) + F.reach;
        if (wx < W && wy < W) {
            const uint32_t bit = wy * W + wx;
            if (c == kNoColumn) {
                if (view_mark(unknown, bit, or_)) {
                    ++t.v[kViewUnknown];
                    t.v[kViewSumX] += (unsigned long long)(long long)lx;
                    t.v[kViewSumY] += (unsigned long long)(long long)ly;
                }
            } else if (view_mark(known, bit, or_)) {
                ++t.v[kViewKnown];
            }
        }
        if (ncol != 0u && cast_column<kCastVoxel>(S, P, G, w, c, ncol, rc, x, t_in, res)) return kCastHit;
        t_in = x.t;
    }
    return kCastMiss;
}

// Ray i of pose k (T its 12 doubles; sd: floats between directions) into the tallies and the per-ray outputs (each may be null)
template <typename OR>
GNDT_HD void view_one(const ScoreView& S, const CastParams& P, const RayGrid& G, const ViewRule& F, const double* T, int lx0, int ly0,
                      const float* dirs, uint32_t sd, uint32_t i, uint32_t* known, uint32_t* unknown, const OR& or_, ViewTally& t, uint32_t* row,
                      float* range) {
    const float* d = dirs + (uint64_t)i * sd;
    float e[3];
    view_end(T, d[0], d[1], d[2], F.max_range, e);
    CastResult res;
    const int rc = view_ray(S, P, G, F, lx0, ly0, (float)T[3], (float)T[7], (float)T[11], e, known, unknown, or_, t, res);
    if (rc == kCastSkipped) ++t.v[kViewSkipped]; else ++t.v[kViewRays];
    if (rc == kCastHit) ++t.v[kViewHits];
    if (rc != kCastHit) {
        res.row = kNoRow;
        res.range = bits_float(rc == kCastMiss ? 0x7F800000u : 0x7FC00000u);       // +inf; quiet NaN
    }
    if (row) row[i] = res.row;
    if (range) range[i] = res.range;
}

// The origin of pose T: false (status 1) when it is not finite or has no key; the cell it stands in otherwise
GNDT_HD bool view_origin(const RayGrid& G, const double* T, int& lx0, int& ly0) {
    const float ox = (float)T[3], oy = (float)T[7], oz = (float)T[11];
    lx0 = ly0 = 0;
    if (!ray_point_ok(G, ox, oy, oz)) return false;
    const PointKey k = point_key(ox, oy, oz, G.ox, G.oy, G.oz, G.grid_len, G.z_len);
    lx0 = ray_lin(k.sx); ly0 = ray_lin(k.sy);
    return true;
}

// The tallies of a pose -> its record
GNDT_HD void view_record(const ViewTally& t, bool origin_ok, ViewInfo& o) {
    o.rays = (uint32_t)t.v[kViewRays]; o.skipped = (uint32_t)t.v[kViewSkipped]; o.hits = (uint32_t)t.v[kViewHits];
    o.unknown = (uint32_t)t.v[kViewUnknown]; o.known = (uint32_t)t.v[kViewKnown]; o.status = origin_ok ? 0u : 1u;
    o.steps = t.v[kViewSteps];
    o.sum_ux = (int64_t)t.v[kViewSumX]; o.sum_uy = (int64_t)t.v[kViewSumY];
}

#if defined(__HIPCC__)
struct ViewOrLds {
    __device__ __forceinline__ uint32_t operator()(uint32_t* w, uint32_t m) const { return atomicOr(w, m); }
};

// One workgroup per pose (grid-stride beyond the grid), any multiple of 64 threads up to kViewMaxThreads.  Dynamic LDS: known[words],
// unknown[words], then kViewLdsTail bytes of per-wave tallies.  LDS keeps what the workgroup before left in it: both bitmaps are
// cleared before the first ray of every pose.
static __global__ void __launch_bounds__(kViewMaxThreads) k_view_gain(ScoreView S, CastParams P, RayGrid G, ViewRule F, const double* __restrict__ poses,
                                                                      uint32_t K, const float* __restrict__ dirs, uint32_t sd, uint32_t N,
                                                                      uint32_t* __restrict__ row, float* __restrict__ range, ViewInfo* __restrict__ info) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_view[];
    uint32_t* known = s_view;
    uint32_t* unknown = s_view + F.words;
    unsigned long long* tail = reinterpret_cast<unsigned long long*>(s_view + 2u * F.words);      // (an even word: 8-byte aligned)
    const uint32_t waves = blockDim.x >> 6, wave = threadIdx.x >> 6;
    const ViewOrLds or_;
    for (uint32_t k = blockIdx.x; k < K; k += gridDim.x) {
        for (uint32_t j = threadIdx.x; j < 2u * F.words; j += blockDim.x) s_view[j] = 0u;
        __syncthreads();
        const double* Tk = poses + 12ull * k;
        double T[12];
#pragma unroll
        for (int a = 0; a < 12; ++a) T[a] = Tk[a];
        int lx0, ly0;
        const bool ok = view_origin(G, T, lx0, ly0);
        ViewTally t{};
        for (uint32_t i = threadIdx.x; i < N; i += blockDim.x)
            view_one(S, P, G, F, T, lx0, ly0, dirs, sd, i, known, unknown, or_, t, row ? row + (uint64_t)k * N : nullptr,
                     range ? range + (uint64_t)k * N : nullptr);
#pragma unroll
        for (uint32_t a = 0; a < kViewTallies; ++a) {
            unsigned long long v = t.v[a];
            for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
            if (__lane_id() == 0) tail[wave * kViewTallies + a] = v;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            ViewTally sum{};
            for (uint32_t wv = 0; wv < waves; ++wv)
                for (uint32_t a = 0; a < kViewTallies; ++a) sum.v[a] += tail[wv * kViewTallies + a];
            ViewInfo o;
            view_record(sum, ok, o);
            info[k] = o;
        }
        __syncthreads();                               // (the tail and the bitmaps are the next pose's from here)
    }
}
#endif

}  // namespace gndt
