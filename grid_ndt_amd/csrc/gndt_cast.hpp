// gndt_cast.hpp — ray casting (include/gndt.h "ray casting"): the first map node along each ray of a batch, and how far away it is.
//
// The walk of a ray is free-space clearing's (gndt_ray.hpp: ray_begin with the ray's own origin, ray_next with the step's crossing
// parameter), without an end margin.  Per column one probe of the column index (clear_column), then the column's sz in the query's
// chunks (kQueryChunk), count next to sz: among the rows with count >= min_count whose level lies in the column's level range and beyond
// the levels already looked at, the one nearest the entry level is the next candidate (a column's levels differ, so "in visit order"
// is "by sz, from the entry level on").
// The loop ends at the first candidate that counts.
//
// The arithmetic of one candidate, in this order (tests/cast_ref.py keeps to it), everything fp64; o, d = p - o, |d|, the cut factor f and
// the crossing parameters are RayWalk's:
//     t_in  = 0 in the first column, else the crossing parameter of the step that entered the column
//     t_out = the crossing parameter of the step that leaves it, f in the last column            t_hi = t_in < t_out ? t_out : t_in
//   VOXEL  (count >= min_count)
//     t = t_in                                                  when the node's level is the column's entry level, else
//     t = ray_cross(oz, z_len, k, o_z, d_z)                     k = ray_lin(sz) going up, ray_lin(sz) + 1 going down
//     t_hit = t;  if (!(t_hit >= t_in)) t_hit = t_in;  if (t_hit > t_hi) t_hit = t_hi                       d2 = 0
//   NDT    (count >= min_count; A's cofactors c_ij and det: score_cofactors, gndt_score.hpp)
//     w_i = (c_i0 d_x + c_i1 d_y) + c_i2 d_z                    g = mean - o
//     t = ((g_x w_x + g_y w_y) + g_z w_z) / ((d_x w_x + d_y w_y) + d_z w_z);  t = 0 when |d| = 0
//     t_hit = t clamped as above (a NaN t — a denominator that underflowed to 0 — takes t_in)
//     q_a = o_a + t_hit d_a                                     the term's d = q - mean with q in fp64, then score_d2: u = adj(A) d,
//     d2 = ((d_x u_x + d_y u_y) + d_z u_z) / det                gated by max_d2 as in scoring
//   both:  range = t_hit |d|;  a candidate with range < min_range does not count
// No product is fused with a sum (-ffp-contract=off); no exp, no floating-point atomics: the same bits in every run, on every stream.
// Everything but the kernel is callable on the host as well (tests/cast_shim.cpp).
#pragma once
#include <math.h>
#include <stdint.h>

#include "gndt_ray.hpp"
#include "gndt_score.hpp"

namespace gndt {

constexpr int kCastVoxel = 0, kCastNdt = 1;          // GNDT_CAST_VOXEL, GNDT_CAST_NDT
constexpr int kCastSkipped = 0, kCastMiss = 1, kCastHit = 2;

struct CastParams {                  // gndt_cast_params with the defaults filled in
    uint32_t min_count;
    double min_range;
    double cov_rel, cov_floor, max_d2;      // NDT mode: scoring's (max_d2 = 0: no gate)
};

struct CastOut {                     // gndt_cast_out: one pointer per output, null = not written
    uint32_t* row;
    float* range;
    float* d2;
};

struct CastResult {
    uint32_t row;
    float range, d2;
};

// Row t (level sz, count c >= min_count) of a column visited over [t_in, t_hi] with entry level lev_in, going up or down: true if it
// stops the ray (res filled)
template <int MODE>
GNDT_HD bool cast_candidate(const ScoreView& S, const CastParams& P, const RayGrid& G, const RayWalk& w, uint32_t t, int sz, uint32_t c,
                            int lev_in, bool up, double t_in, double t_hi, CastResult& res) {
    double th, d2 = 0.0;
    if (MODE == kCastVoxel) {
        th = sz == lev_in ? t_in : ray_cross(G.oz, G.z_len, up ? ray_lin(sz) : ray_lin(sz) + 1, w.r[2], w.d[2]);
        if (!(th >= t_in)) th = t_in;
        if (th > t_hi) th = t_hi;
    } else {
        const float* m = S.Q.V.mean + 3 * (size_t)t;
        const float* s = S.cov + 6 * (size_t)t;
        const float mx = m[0], my = m[1], mz = m[2];
        const float s0 = s[0], s1 = s[1], s2 = s[2], s3 = s[3], s4 = s[4], s5 = s[5];
        ScoreTerm T;
        score_cofactors(c, s0, s1, s2, s3, s4, s5, P.cov_rel, P.cov_floor, T);
        const double wx = (T.c00 * w.d[0] + T.c01 * w.d[1]) + T.c02 * w.d[2];
        const double wy = (T.c01 * w.d[0] + T.c11 * w.d[1]) + T.c12 * w.d[2];
        const double wz = (T.c02 * w.d[0] + T.c12 * w.d[1]) + T.c22 * w.d[2];
        const double gx = (double)mx - w.r[0], gy = (double)my - w.r[1], gz = (double)mz - w.r[2];
        th = 0.0;
        if (w.len > 0.0) th = ((gx * wx + gy * wy) + gz * wz) / ((w.d[0] * wx + w.d[1] * wy) + w.d[2] * wz);
        if (!(th >= t_in)) th = t_in;
        if (th > t_hi) th = t_hi;
        T.dx = (w.r[0] + th * w.d[0]) - (double)mx;
        T.dy = (w.r[1] + th * w.d[1]) - (double)my;
        T.dz = (w.r[2] + th * w.d[2]) - (double)mz;
        score_d2(T);
        d2 = T.d2;
        if (P.max_d2 > 0.0 && d2 > P.max_d2) return false;
    }
    const double range = th * w.len;
    if (range < P.min_range) return false;
    res.row = t; res.range = (float)range; res.d2 = (float)d2;
    return true;
}

// The rows of column c (ncol nodes) with a level in [rc.lo, rc.hi] and count >= min_count, in visit order from x.lev_in towards
// x.lev_out, until one stops the ray.  sz and count of a chunk are loaded together, so one scan of the column yields its first
// candidate; the column is scanned again only behind a candidate that max_d2 or min_range turned down.
template <int MODE>
GNDT_HD bool cast_column(const ScoreView& S, const CastParams& P, const RayGrid& G, const RayWalk& w, uint32_t c, uint32_t ncol,
                         const RayColumn& rc, const RayCross& x, double t_in, CastResult& res) {
    const bool up = x.lev_in <= x.lev_out;
    const double t_hi = t_in < x.t ? x.t : t_in;
    int lo = rc.lo, hi = rc.hi;                      // the levels not looked at yet
    while (lo <= hi) {
        uint32_t best = kNoRow, bc = 0u;
        int bz = 0;
        for (uint32_t from = 0; from < ncol; from += kQueryChunk) {
            int szv[kQueryChunk];
            uint32_t cnt[kQueryChunk];
#pragma unroll
            for (uint32_t u = 0; u < kQueryChunk; ++u) {
                szv[u] = 0; cnt[u] = 0u;                     // (0 is no level)
                if (from + u < ncol) { szv[u] = S.Q.V.sz[c + from + u]; cnt[u] = S.count[c + from + u]; }
            }
#pragma unroll
            for (uint32_t u = 0; u < kQueryChunk; ++u) {
                const int z = szv[u];
                if (from + u < ncol && z >= lo && z <= hi && cnt[u] >= P.min_count && (best == kNoRow || (up ? z < bz : z > bz))) {
                    best = c + from + u; bz = z; bc = cnt[u];
                }
            }
        }
        if (best == kNoRow) return false;
        if (cast_candidate<MODE>(S, P, G, w, best, bz, bc, x.lev_in, up, t_in, t_hi, res)) return true;
        if (up) lo = bz + 1; else hi = bz - 1;
    }
    return false;
}

// One ray from o to p: kCastSkipped (o or p not finite or without a key), kCastMiss, or kCastHit with res filled
template <int MODE>
GNDT_HD int cast_ray(const ScoreView& S, const CastParams& P, const RayGrid& G, float ox, float oy, float oz, float px, float py, float pz,
                     CastResult& res) {
    RayWalk w;
    if (!ray_begin(G, ox, oy, oz, px, py, pz, w)) return kCastSkipped;
    RayColumn rc;
    RayCross x;
    double t_in = 0.0;
    while (ray_next(G, w, rc, x)) {
        uint32_t ncol;
        const uint32_t c = clear_column<false>(S.Q, nullptr, rc, ncol);
        if (ncol != 0u && cast_column<MODE>(S, P, G, w, c, ncol, rc, x, t_in, res)) return kCastHit;
        t_in = x.t;
    }
    return kCastMiss;
}

// Ray i of a batch into the outputs (so: floats between origins, 0 = one origin for all; se: floats between end points) -> its outcome
template <int MODE>
GNDT_HD int cast_one(const ScoreView& S, const CastParams& P, const RayGrid& G, const float* origins, uint32_t so, const float* ends,
                     uint32_t se, uint64_t i, const CastOut& o) {
    const float* a = origins + i * so;
    const float* p = ends + i * se;
    CastResult res;
    const int rc = cast_ray<MODE>(S, P, G, a[0], a[1], a[2], p[0], p[1], p[2], res);
    if (rc != kCastHit) {
        res.row = kNoRow;
        res.range = res.d2 = bits_float(rc == kCastMiss ? 0x7F800000u : 0x7FC00000u);      // +inf; quiet NaN
    }
    if (o.row) o.row[i] = res.row;
    if (o.range) o.range[i] = res.range;
    if (o.d2) o.d2[i] = res.d2;
    return rc;
}

#if defined(__HIPCC__)
// One ray per lane, in input order.  TALLY: stats = {rays, skipped, hits}, one add per wave and counter (whole waves run the tally);
// without it the kernel reads and writes no counter.
template <int MODE, bool TALLY>
static __global__ void __launch_bounds__(256) k_cast(ScoreView S, CastParams P, RayGrid G, const float* __restrict__ origins, uint32_t so,
                                                     const float* __restrict__ ends, uint32_t se, uint64_t n, CastOut o,
                                                     unsigned long long* __restrict__ stats) {
    const uint64_t gsz = (uint64_t)gridDim.x * blockDim.x;
    if (!TALLY) {
        for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gsz) (void)cast_one<MODE>(S, P, G, origins, so, ends, se, i, o);
        return;
    }
    const uint64_t n_round = (n + 63) & ~63ull;
    unsigned long long rays = 0, skipped = 0, hits = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_round; i += gsz) {
        if (i >= n) continue;
        const int rc = cast_one<MODE>(S, P, G, origins, so, ends, se, i, o);
        if (rc == kCastSkipped) ++skipped; else ++rays;
        if (rc == kCastHit) ++hits;
    }
    for (int off = 32; off > 0; off >>= 1) {
        rays += __shfl_down(rays, off, 64);
        skipped += __shfl_down(skipped, off, 64);
        hits += __shfl_down(hits, off, 64);
    }
    if (__lane_id() == 0) {
        if (rays) atomicAdd(&stats[0], rays);
        if (skipped) atomicAdd(&stats[1], skipped);
        if (hits) atomicAdd(&stats[2], hits);
    }
}
#endif

}  // namespace gndt
