// gndt_score_derivs.hpp — scan score derivatives (include/gndt.h "scan score derivatives"): the score of gndt_score.hpp for K poses with
// its gradient and its full Hessian with respect to a left pose perturbation xi = (v, w), q(xi) = Exp([w]x) q + v.  The sum that is
// differentiated is the frozen one: every point keeps the candidates it has at the pose itself, and q is a real vector.
//
// The lookup and the arithmetic of a term are gndt_score.hpp's (score_point, whose sink receives every counted candidate).  What a
// term adds, in this order, everything fp64, no product fused with a sum, e = exp(-0.5 d2) the value the score itself adds:
//     r    = 1 / det                  ub_i = u_i * r                  B_ij = c_ij * r          (B = A^-1, ub = A^-1 d)
//     w3_i += e * ub_i                                                                          (i = x, y, z)
//     M_ij += e * (ub_i * ub_j - B_ij)                                                          (ij = xx, xy, xz, yy, yz, zz)
// w3 and M are sums over the point's counted candidates in the candidates' order, from 0.  The pose Jacobian of a point is common
// to its candidates, so the nine sums are expanded once per point (score_derivs_expand), q = the fp32 q widened:
//     g_v   = (-w3_x, -w3_y, -w3_z)
//     g_w   = (-(q_y w3_z - q_z w3_y), -(q_z w3_x - q_x w3_z), -(q_x w3_y - q_y w3_x))
//     H_vv  = M
//     P     = H_vw:  P_i0 = M_iz q_y - M_iy q_z     P_i1 = M_ix q_z - M_iz q_x     P_i2 = M_iy q_x - M_ix q_y        (i = x, y, z)
//     wq    = (w3_x q_x + w3_y q_y) + w3_z q_z
//     W_0b  = q_y P_2b - q_z P_1b      W_1b = q_z P_0b - q_x P_2b      W_2b = q_x P_1b - q_y P_0b                   (b >= a only)
//     H_ww: H_aa = W_aa - (w3_a q_a - wq)           H_ab = W_ab - 0.5 * (w3_a q_b + w3_b q_a)                       (a < b)
// A point without a counted candidate adds +0 to all 27 values (so a pose with a NaN, or off the map, gives exact zeros).
// The 27 values of a point, in the record's order: g[6], then H's upper triangle row-major: M_xx M_xy M_xz P_00 P_01 P_02 | M_yy M_yz
// P_10 P_11 P_12 | M_zz P_20 P_21 P_22 | H_33 H_34 H_35 | H_44 H_45 | H_55.
// Sums: a workgroup owns the kScoreTile points k_score's workgroup owns and adds each of its 4 + 27 values in score_block_sum's
// tree (the wave by __shfl_xor, the four wave sums as (w0 + w1) + (w2 + w3)); the wave sums of all values go to LDS behind ONE
// barrier.  A pose's tiles are then added as k_score_reduce adds them: "thread" t of 1024 adds tiles t, t + 1024, ... in that order
// from 0, the 64 threads of a wave are added by the butterfly, the 16 wave sums pairwise.  Here each of the 16 waves is a workgroup
// of its own (k_score_derivs_reduce: the pass reads 240 bytes a tile, which one workgroup would read on one CU) and the 16 wave
// sums are added by k_score_derivs_finish: the same additions in the same order, so score, d2_sum, matched and terms have the bits
// gndt_score_poses gives.  No floating-point atomics.
// Everything but the kernels is callable on the host as well (tests/score_derivs_shim.cpp).
#pragma once
#include "gndt_score.hpp"

namespace gndt {

constexpr int kDerivValues = 27;                         // g[6] + H[21]
constexpr int kDerivDoubles = 2 + kDerivValues;          // score, d2_sum, g, H
constexpr uint32_t kDerivReduceWaves = kScoreReduceBlock / 64;

struct ScoreDerivSink {             // the nine sums of one point
    double w[3], m[6];
    GNDT_HD void operator()(uint32_t, const ScoreTerm& t, double e) {
        const double r = 1.0 / t.det;
        const double ubx = t.ux * r, uby = t.uy * r, ubz = t.uz * r;
        const double b00 = t.c00 * r, b01 = t.c01 * r, b02 = t.c02 * r, b11 = t.c11 * r, b12 = t.c12 * r, b22 = t.c22 * r;
        w[0] += e * ubx; w[1] += e * uby; w[2] += e * ubz;
        m[0] += e * (ubx * ubx - b00); m[1] += e * (ubx * uby - b01); m[2] += e * (ubx * ubz - b02);
        m[3] += e * (uby * uby - b11); m[4] += e * (uby * ubz - b12); m[5] += e * (ubz * ubz - b22);
    }
};

// The 27 values of one point from its nine sums (the order of the header comment)
GNDT_HD void score_derivs_expand(float qxf, float qyf, float qzf, const double* w, const double* m, double* o) {
    const double qx = (double)qxf, qy = (double)qyf, qz = (double)qzf;
    const double mxx = m[0], mxy = m[1], mxz = m[2], myy = m[3], myz = m[4], mzz = m[5];
    o[0] = -w[0]; o[1] = -w[1]; o[2] = -w[2];
    o[3] = -(qy * w[2] - qz * w[1]); o[4] = -(qz * w[0] - qx * w[2]); o[5] = -(qx * w[1] - qy * w[0]);
    const double p00 = mxz * qy - mxy * qz, p01 = mxx * qz - mxz * qx, p02 = mxy * qx - mxx * qy;
    const double p10 = myz * qy - myy * qz, p11 = mxy * qz - myz * qx, p12 = myy * qx - mxy * qy;
    const double p20 = mzz * qy - myz * qz, p21 = mxz * qz - mzz * qx, p22 = myz * qx - mxz * qy;
    const double wq = (w[0] * qx + w[1] * qy) + w[2] * qz;
    double* h = o + 6;
    h[0] = mxx; h[1] = mxy; h[2] = mxz; h[3] = p00; h[4] = p01; h[5] = p02;
    h[6] = myy; h[7] = myz; h[8] = p10; h[9] = p11; h[10] = p12;
    h[11] = mzz; h[12] = p20; h[13] = p21; h[14] = p22;
    h[15] = (qy * p20 - qz * p10) - (w[0] * qx - wq);
    h[16] = (qy * p21 - qz * p11) - 0.5 * (w[0] * qy + w[1] * qx);
    h[17] = (qy * p22 - qz * p12) - 0.5 * (w[0] * qz + w[2] * qx);
    h[18] = (qz * p01 - qx * p21) - (w[1] * qy - wq);
    h[19] = (qz * p02 - qx * p22) - 0.5 * (w[1] * qz + w[2] * qy);
    h[20] = (qx * p12 - qy * p02) - (w[2] * qz - wq);
}

// One point at one pose: its share of the four sums into a, its 27 values into o (+0 when it has no counted candidate)
template <int NBH>
GNDT_HD void score_derivs_point(const ScoreView& S, const ScoreParams& P, float qx, float qy, float qz, ScoreAcc& a, double* o) {
    ScoreDerivSink sink;
#pragma unroll
    for (int j = 0; j < 3; ++j) sink.w[j] = 0.0;
#pragma unroll
    for (int j = 0; j < 6; ++j) sink.m[j] = 0.0;
    ScoreBest b;
    b.d2 = (double)INFINITY; b.row = kNoRow;
    const uint32_t before = a.matched;
    score_point<NBH>(S, P, qx, qy, qz, a, b, sink);
    if (a.matched != before) score_derivs_expand(qx, qy, qz, sink.w, sink.m, o);
    else {
#pragma unroll
        for (int j = 0; j < kDerivValues; ++j) o[j] = 0.0;
    }
}

struct ScoreDerivPartial {          // one workgroup's sums: partial[pose][tile]
    double v[kDerivDoubles];        // score, d2_sum, g[6], H[21]
    uint32_t matched, terms;
};

struct ScoreDerivWaves {            // the 16 wave sums of a pose's tiles: waves[pose]
    double v[kDerivDoubles][kDerivReduceWaves];
    unsigned long long matched[kDerivReduceWaves], terms[kDerivReduceWaves];
};

struct ScoreDerivRecord {           // gndt_pose_derivs
    double score, d2_sum;
    uint64_t matched, terms;
    double g[6], H[21];
};

#if defined(__HIPCC__)
// One thread per (point, pose), tile and grid as k_score.  partial[pose * tiles + tile] = the workgroup's sums.
template <int NBH>
static __global__ void __launch_bounds__(kScoreTile) k_score_derivs(ScoreView S, ScoreParams P, const float* __restrict__ xyz, uint32_t sf,
                                                                    uint64_t n, const double* __restrict__ poses,
                                                                    ScoreDerivPartial* __restrict__ partial) {
    constexpr int NW = kScoreTile / 64;
    static_assert(NW == 4, "the four wave sums are added as (w0 + w1) + (w2 + w3)");
    __shared__ double s_v[kDerivDoubles][NW];
    __shared__ uint32_t s_c[2][NW];
    const uint32_t pose = blockIdx.y;
    const uint64_t i = (uint64_t)blockIdx.x * kScoreTile + threadIdx.x;
    ScoreAcc a;
    a.score = 0.0; a.d2_sum = 0.0; a.matched = 0u; a.terms = 0u;
    double o[kDerivValues];
#pragma unroll
    for (int j = 0; j < kDerivValues; ++j) o[j] = 0.0;
    if (i < n) {
        const float* p = xyz + i * sf;
        float qx, qy, qz;
        score_transform(poses + 12 * (size_t)pose, p[0], p[1], p[2], qx, qy, qz);
        score_derivs_point<NBH>(S, P, qx, qy, qz, a, o);
    }
    const uint32_t wave = threadIdx.x >> 6;
    const bool first = (threadIdx.x & 63u) == 0u;
    {
        const double score = score_wave_sum(a.score), d2_sum = score_wave_sum(a.d2_sum);
        const uint32_t matched = score_wave_sum(a.matched), terms = score_wave_sum(a.terms);
        if (first) { s_v[0][wave] = score; s_v[1][wave] = d2_sum; s_c[0][wave] = matched; s_c[1][wave] = terms; }
    }
#pragma unroll
    for (int j = 0; j < kDerivValues; ++j) {
        const double v = score_wave_sum(o[j]);
        if (first) s_v[2 + j][wave] = v;
    }
    __syncthreads();
    ScoreDerivPartial* out = partial + (size_t)pose * gridDim.x + blockIdx.x;
    if (threadIdx.x < (uint32_t)kDerivDoubles) {
        const double* w = s_v[threadIdx.x];
        out->v[threadIdx.x] = (w[0] + w[1]) + (w[2] + w[3]);
    } else if (threadIdx.x == (uint32_t)kDerivDoubles) {
        out->matched = (s_c[0][0] + s_c[0][1]) + (s_c[0][2] + s_c[0][3]);
        out->terms = (s_c[1][0] + s_c[1][1]) + (s_c[1][2] + s_c[1][3]);
    }
}

// Wave blockIdx.x of the 16 that add a pose's (blockIdx.y) tiles: thread t = 64 blockIdx.x + lane adds tiles t, t + 1024, ... in
// that order (two records in flight), then the butterfly.  waves[pose] takes the wave's sums.
static __global__ void __launch_bounds__(64) k_score_derivs_reduce(const ScoreDerivPartial* __restrict__ partial, uint32_t tiles,
                                                                   ScoreDerivWaves* __restrict__ waves) {
    const ScoreDerivPartial* p = partial + (size_t)blockIdx.y * tiles;
    double v[kDerivDoubles];
#pragma unroll
    for (int j = 0; j < kDerivDoubles; ++j) v[j] = 0.0;
    unsigned long long matched = 0ull, terms = 0ull;
    for (uint32_t t0 = blockIdx.x * 64u + threadIdx.x; t0 < tiles; t0 += 2u * kScoreReduceBlock) {
        ScoreDerivPartial r[2];
#pragma unroll
        for (uint32_t u = 0; u < 2u; ++u) {
            const uint32_t t = t0 + u * kScoreReduceBlock;      // (tiles < 2^31: no wrap)
#pragma unroll
            for (int j = 0; j < kDerivDoubles; ++j) r[u].v[j] = 0.0;      // (adding a zero record changes no bit)
            r[u].matched = 0u; r[u].terms = 0u;
            if (t < tiles) r[u] = p[t];
        }
#pragma unroll
        for (uint32_t u = 0; u < 2u; ++u) {
#pragma unroll
            for (int j = 0; j < kDerivDoubles; ++j) v[j] += r[u].v[j];
            matched += r[u].matched; terms += r[u].terms;
        }
    }
    ScoreDerivWaves* o = waves + blockIdx.y;
#pragma unroll
    for (int j = 0; j < kDerivDoubles; ++j) {
        const double s = score_wave_sum(v[j]);
        if (threadIdx.x == 0u) o->v[j][blockIdx.x] = s;
    }
    matched = score_wave_sum(matched); terms = score_wave_sum(terms);
    if (threadIdx.x == 0u) { o->matched[blockIdx.x] = matched; o->terms[blockIdx.x] = terms; }
}

// The 16 wave sums of a pose pairwise, as score_block_sum adds them: thread j its value j, then the record
static __global__ void __launch_bounds__(64) k_score_derivs_finish(const ScoreDerivWaves* __restrict__ waves, ScoreDerivRecord* __restrict__ out) {
    constexpr int NW = (int)kDerivReduceWaves;
    const ScoreDerivWaves* w = waves + blockIdx.x;
    ScoreDerivRecord* o = out + blockIdx.x;
    const uint32_t j = threadIdx.x;
    if (j < (uint32_t)kDerivDoubles) {
        double s[NW];
#pragma unroll
        for (int k = 0; k < NW; ++k) s[k] = w->v[j][k];
#pragma unroll
        for (int k = NW; k > 1; k >>= 1)
#pragma unroll
            for (int i = 0; i < k / 2; ++i) s[i] = s[2 * i] + s[2 * i + 1];
        if (j == 0u) o->score = s[0];
        else if (j == 1u) o->d2_sum = s[0];
        else if (j < 8u) o->g[j - 2u] = s[0];
        else o->H[j - 8u] = s[0];
    } else if (j < (uint32_t)kDerivDoubles + 2u) {
        const unsigned long long* c = j == (uint32_t)kDerivDoubles ? w->matched : w->terms;
        unsigned long long s[NW];
#pragma unroll
        for (int k = 0; k < NW; ++k) s[k] = c[k];
#pragma unroll
        for (int k = NW; k > 1; k >>= 1)
#pragma unroll
            for (int i = 0; i < k / 2; ++i) s[i] = s[2 * i] + s[2 * i + 1];
        if (j == (uint32_t)kDerivDoubles) o->matched = s[0]; else o->terms = s[0];
    }
}
#endif

}  // namespace gndt
