// gndt_score_maps.hpp — map-to-map scoring (include/gndt.h "map-to-map scoring"): the distribution-to-distribution NDT score of the
// source map's nodes against the destination map for K poses, and that score with its gradient and Hessian.  A source node is a
// Gaussian (count, mean, scatter) like a destination node; the covariance of the difference of the two is the sum of theirs, the
// source's rotated by the pose.
//
// Per (source row, pose) pair, everything fp64 from the rows' fp32 values, no product fused with a sum:
//     q    = score_transform(T, m_s)                       (scan scoring's step 1: the fp32 q is all the lookup sees)
//     r_s  = 1 / (c_s - 1)                                 C_ab = S_s,ab * r_s                      (ab = xx xy xz yy yz zz)
//     W_ib = (R_i0 C_0b + R_i1 C_1b) + R_i2 C_2b           Sg_ij = (W_i0 R_j0 + W_i1 R_j1) + W_i2 R_j2, i <= j       (score_maps_sigma)
// The candidates are score_point's, in its order: its sink is handed every destination row with count >= min_count and works the
// pair's own term out from the row (score_maps_pair; the term score_point made of the row is not looked at):
//     r_d  = 1 / (c_d - 1)                                 P_ab = Sg_ab + S_d,ab * r_d
//     eps  = max(cov_rel * (((P_xx + P_yy) + P_zz) / 3), cov_floor)           A = P + eps I
//     the cofactors c_ij of A, det, d = q - m_d, u and d2 as gndt_score.hpp states them (score_d2); term e = exp(-0.5 d2)
// With Sg = 0 that is score_node's term to the bit.
// What a pair adds to the 6 + 21 values (score_maps_derivs_add), with r = 1 / det, ub_i = u_i * r, B_ij = c_ij * r:
//     p_i   = (Sg_i0 ub_x + Sg_i1 ub_y) + Sg_i2 ub_z       z = q - p                                (q the fp32 q widened)
//     t_0i  = Sg_i2 ub_y - Sg_i1 ub_z      t_1i = Sg_i0 ub_z - Sg_i2 ub_x      t_2i = Sg_i1 ub_x - Sg_i0 ub_y       (t_a = Sg (e_a x ub))
//     r_a   = e_a x z + t_a (a = 0, 1, 2: the rotations; the translations' r_a is e_a):
//             r_0 = (t_00, t_01 - z_z, t_02 + z_y)   r_1 = (t_10 + z_z, t_11, t_12 - z_x)   r_2 = (t_20 - z_y, t_21 + z_x, t_22)
//     f_a   = phi_a / 2:  translations ub_a;  rotations 0.5 * ((ub_x w_x + ub_y w_y) + ub_z w_z), w = e_a x q + r_a per coordinate
//     Br_a  = B r_a,  (Br_a)_i = (B_i0 r_a0 + B_i1 r_a1) + B_i2 r_a2
//     rho   = r_a^T B r_b:  B_ab (two translations), (Br_b)_a (translation a, rotation b), (r_a0 Br_b0 + r_a1 Br_b1) + r_a2 Br_b2
//     k_ab  = (e_a x ub) . t_b:  k_0b = ub_y t_b2 - ub_z t_b1     k_1b = ub_z t_b0 - ub_x t_b2     k_2b = ub_x t_b1 - ub_y t_b0
//     uz    = (ub_x z_x + ub_y z_y) + ub_z z_z
//     x_aa  = (ub_a z_a - uz) - k_aa                       x_ab = 0.5 * (ub_a z_b + ub_b z_a) - k_ab  (a < b)      (two rotations only)
//     g_a  -= e * f_a                                      H_ab += e * ((f_a f_b - rho_ab) - x_ab)   (x_ab = 0 unless both rotate)
// These are the header's r_a = d_a - A_a ub, phi_a and phi_ab with A_a ub = e_a x p - t_a worked in (G_a^T = -G_a, Sg symmetric).
// The 27 values in the record's order (scan score derivatives'): g[6], then H's upper triangle row-major.  A thread adds its pairs in
// the candidates' order, from +0: a row without a term adds +0 to everything.
// Sums: one thread per (source row, pose); row r sits in tile r / kScoreTile whether it counts or not; the trees are the score's
// (score_block_sum; k_score_derivs' for the derivatives), and a pose's tiles are added by the score's own reduce kernels, which read
// the same partial records.  No floating-point atomics.
// Everything but the kernels is callable on the host as well (tests/score_maps_shim.cpp).
#pragma once
#include "gndt_score_derivs.hpp"

namespace gndt {

constexpr uint32_t kFlagHasStats = 1u;                   // GNDT_FLAG_HAS_STATS

struct MapsSource {                 // the source map's rows
    const uint32_t* count;
    const float* mean;              // [rows][3]
    const float* cov;               // [rows][6]
    const uint32_t* flags;
};

struct MapsNode {                   // a counted source row at a pose: the moved mean and the rotated covariance
    float qx, qy, qz;
    double s00, s01, s02, s11, s12, s22;
};

// Sg = R C R^T of the source row's covariance C = S / (c - 1) (the order of the header comment)
GNDT_HD void score_maps_sigma(const double* T, uint32_t c, const float* s, MapsNode& n) {
    const double r = 1.0 / (double)(c - 1u);
    const double c00 = (double)s[0] * r, c01 = (double)s[1] * r, c02 = (double)s[2] * r, c11 = (double)s[3] * r, c12 = (double)s[4] * r,
                 c22 = (double)s[5] * r;
    double w[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double r0 = T[4 * i], r1 = T[4 * i + 1], r2 = T[4 * i + 2];
        w[i][0] = (r0 * c00 + r1 * c01) + r2 * c02;
        w[i][1] = (r0 * c01 + r1 * c11) + r2 * c12;
        w[i][2] = (r0 * c02 + r1 * c12) + r2 * c22;
    }
    n.s00 = (w[0][0] * T[0] + w[0][1] * T[1]) + w[0][2] * T[2];
    n.s01 = (w[0][0] * T[4] + w[0][1] * T[5]) + w[0][2] * T[6];
    n.s02 = (w[0][0] * T[8] + w[0][1] * T[9]) + w[0][2] * T[10];
    n.s11 = (w[1][0] * T[4] + w[1][1] * T[5]) + w[1][2] * T[6];
    n.s12 = (w[1][0] * T[8] + w[1][1] * T[9]) + w[1][2] * T[10];
    n.s22 = (w[2][0] * T[8] + w[2][1] * T[9]) + w[2][2] * T[10];
}

// The term of the moved source node n against the destination row (the order of the header comment); false: the row is not a
// candidate (too few points, or beyond max_d2)
GNDT_HD bool score_maps_pair(const ScoreView& D, const ScoreParams& P, const MapsNode& n, uint32_t row, ScoreTerm& t) {
    const uint32_t c = D.count[row];
    const float* m = D.Q.V.mean + 3 * (size_t)row;
    const float* s = D.cov + 6 * (size_t)row;
    const float mx = m[0], my = m[1], mz = m[2];
    const float s0 = s[0], s1 = s[1], s2 = s[2], s3 = s[3], s4 = s[4], s5 = s[5];
    if (c < P.min_count) return false;
    const double r = 1.0 / (double)(c - 1u);
    const double pxx = n.s00 + (double)s0 * r, pxy = n.s01 + (double)s1 * r, pxz = n.s02 + (double)s2 * r, pyy = n.s11 + (double)s3 * r,
                 pyz = n.s12 + (double)s4 * r, pzz = n.s22 + (double)s5 * r;
    const double eps = fmax(P.cov_rel * (((pxx + pyy) + pzz) / 3.0), P.cov_floor);
    const double a00 = pxx + eps, a11 = pyy + eps, a22 = pzz + eps, a01 = pxy, a02 = pxz, a12 = pyz;
    t.c00 = a11 * a22 - a12 * a12; t.c01 = a02 * a12 - a01 * a22; t.c02 = a01 * a12 - a02 * a11;
    t.c11 = a00 * a22 - a02 * a02; t.c12 = a01 * a02 - a00 * a12; t.c22 = a00 * a11 - a01 * a01;
    t.det = (a00 * t.c00 + a01 * t.c01) + a02 * t.c02;
    t.dx = (double)n.qx - (double)mx; t.dy = (double)n.qy - (double)my; t.dz = (double)n.qz - (double)mz;
    score_d2(t);
    return !(P.max_d2 > 0.0 && t.d2 > P.max_d2);
}

// What the pair of term t (e = exp(-0.5 d2)) adds to the 27 values o (the order of the header comment)
GNDT_HD void score_maps_derivs_add(const MapsNode& n, const ScoreTerm& t, double e, double* o) {
    const double r = 1.0 / t.det;
    const double ux = t.ux * r, uy = t.uy * r, uz = t.uz * r;
    const double b00 = t.c00 * r, b01 = t.c01 * r, b02 = t.c02 * r, b11 = t.c11 * r, b12 = t.c12 * r, b22 = t.c22 * r;
    const double qx = (double)n.qx, qy = (double)n.qy, qz = (double)n.qz;
    const double zx = qx - ((n.s00 * ux + n.s01 * uy) + n.s02 * uz);
    const double zy = qy - ((n.s01 * ux + n.s11 * uy) + n.s12 * uz);
    const double zz = qz - ((n.s02 * ux + n.s12 * uy) + n.s22 * uz);
    const double t00 = n.s02 * uy - n.s01 * uz, t01 = n.s12 * uy - n.s11 * uz, t02 = n.s22 * uy - n.s12 * uz;
    const double t10 = n.s00 * uz - n.s02 * ux, t11 = n.s01 * uz - n.s12 * ux, t12 = n.s02 * uz - n.s22 * ux;
    const double t20 = n.s01 * ux - n.s00 * uy, t21 = n.s11 * ux - n.s01 * uy, t22 = n.s12 * ux - n.s02 * uy;
    // r_a of the three rotations
    const double r00 = t00, r01 = t01 - zz, r02 = t02 + zy;
    const double r10 = t10 + zz, r11 = t11, r12 = t12 - zx;
    const double r20 = t20 - zy, r21 = t21 + zx, r22 = t22;
    // f_a = phi_a / 2
    const double f0 = ux, f1 = uy, f2 = uz;
    const double f3 = 0.5 * ((ux * r00 + uy * (r01 - qz)) + uz * (r02 + qy));
    const double f4 = 0.5 * ((ux * (r10 + qz) + uy * r11) + uz * (r12 - qx));
    const double f5 = 0.5 * ((ux * (r20 - qy) + uy * (r21 + qx)) + uz * r22);
    // Br_a = B r_a
    const double v00 = (b00 * r00 + b01 * r01) + b02 * r02, v01 = (b01 * r00 + b11 * r01) + b12 * r02, v02 = (b02 * r00 + b12 * r01) + b22 * r02;
    const double v10 = (b00 * r10 + b01 * r11) + b02 * r12, v11 = (b01 * r10 + b11 * r11) + b12 * r12, v12 = (b02 * r10 + b12 * r11) + b22 * r12;
    const double v20 = (b00 * r20 + b01 * r21) + b02 * r22, v21 = (b01 * r20 + b11 * r21) + b12 * r22, v22 = (b02 * r20 + b12 * r21) + b22 * r22;
    // the second-order part of two rotations
    const double uzs = (ux * zx + uy * zy) + uz * zz;
    const double x00 = (ux * zx - uzs) - (uy * t02 - uz * t01);
    const double x01 = 0.5 * (ux * zy + uy * zx) - (uy * t12 - uz * t11);
    const double x02 = 0.5 * (ux * zz + uz * zx) - (uy * t22 - uz * t21);
    const double x11 = (uy * zy - uzs) - (uz * t10 - ux * t12);
    const double x12 = 0.5 * (uy * zz + uz * zy) - (uz * t20 - ux * t22);
    const double x22 = (uz * zz - uzs) - (ux * t21 - uy * t20);
    o[0] -= e * f0; o[1] -= e * f1; o[2] -= e * f2; o[3] -= e * f3; o[4] -= e * f4; o[5] -= e * f5;
    double* h = o + 6;
    h[0] += e * (f0 * f0 - b00); h[1] += e * (f0 * f1 - b01); h[2] += e * (f0 * f2 - b02);
    h[3] += e * (f0 * f3 - v00); h[4] += e * (f0 * f4 - v10); h[5] += e * (f0 * f5 - v20);
    h[6] += e * (f1 * f1 - b11); h[7] += e * (f1 * f2 - b12);
    h[8] += e * (f1 * f3 - v01); h[9] += e * (f1 * f4 - v11); h[10] += e * (f1 * f5 - v21);
    h[11] += e * (f2 * f2 - b22);
    h[12] += e * (f2 * f3 - v02); h[13] += e * (f2 * f4 - v12); h[14] += e * (f2 * f5 - v22);
    h[15] += e * ((f3 * f3 - ((r00 * v00 + r01 * v01) + r02 * v02)) - x00);
    h[16] += e * ((f3 * f4 - ((r00 * v10 + r01 * v11) + r02 * v12)) - x01);
    h[17] += e * ((f3 * f5 - ((r00 * v20 + r01 * v21) + r02 * v22)) - x02);
    h[18] += e * ((f4 * f4 - ((r10 * v10 + r11 * v11) + r12 * v12)) - x11);
    h[19] += e * ((f4 * f5 - ((r10 * v20 + r11 * v21) + r12 * v22)) - x12);
    h[20] += e * ((f5 * f5 - ((r20 * v20 + r21 * v21) + r22 * v22)) - x22);
}

// score_point's sink: every destination row with count >= min_count arrives here in the candidates' order
template <bool DERIVS>
struct MapsSink {
    const ScoreView& D;
    const ScoreParams& P;
    const MapsNode& n;
    ScoreAcc& a;
    ScoreBest& b;
    double* o;                      // DERIVS: the thread's 27 values
    uint32_t found;
    GNDT_HD void operator()(uint32_t row, const ScoreTerm&, double) {
        ScoreTerm t;
        if (!score_maps_pair(D, P, n, row, t)) return;
        const double e = exp(-0.5 * t.d2);
        a.score += e;
        a.d2_sum += t.d2;
        ++a.terms;
        ++found;
        if (t.d2 < b.d2 || (t.d2 == b.d2 && row < b.row)) { b.d2 = t.d2; b.row = row; }
        if (DERIVS) score_maps_derivs_add(n, t, e, o);
    }
};

// Source row r at pose T: false when the row does not count (no statistics, or fewer than min_count points); otherwise its terms into
// a (matched: at least one), its nearest destination row into b and, DERIVS, its share of the 27 values into o
template <int NBH, bool DERIVS>
GNDT_HD bool score_maps_row(const ScoreView& D, const ScoreParams& P, const MapsSource& src, uint64_t r, const double* T, ScoreAcc& a,
                            ScoreBest& b, double* o) {
    const uint32_t c = src.count[r];
    if (!(src.flags[r] & kFlagHasStats) || c < P.min_count) return false;
    const float* m = src.mean + 3 * r;
    MapsNode n;
    score_transform(T, m[0], m[1], m[2], n.qx, n.qy, n.qz);
    score_maps_sigma(T, c, src.cov + 6 * r, n);
    ScoreParams L = P;
    L.max_d2 = 0.0;                 // (the lookup hands over every row with enough points: the gate is the pair's)
    ScoreAcc la;
    la.score = 0.0; la.d2_sum = 0.0; la.matched = 0u; la.terms = 0u;
    ScoreBest lb;
    lb.d2 = (double)INFINITY; lb.row = kNoRow;
    MapsSink<DERIVS> sink{D, P, n, a, b, o, 0u};
    score_point<NBH>(D, L, n.qx, n.qy, n.qz, la, lb, sink);
    if (sink.found) ++a.matched;
    return true;
}

#if defined(__HIPCC__)
// One thread per (source row, pose): blockIdx.x the tile of kScoreTile rows, blockIdx.y the pose.  partial[pose * tiles + tile] = the
// workgroup's sums (k_score's record: k_score_reduce adds them).  NODEWISE: the workgroups of `node_pose` also store every source row's
// least d2 (fp32; +inf: no term, NaN: the row does not count) and that destination row (kNoRow) where the pointers are not null.
template <int NBH, bool NODEWISE>
static __global__ void __launch_bounds__(kScoreTile) k_score_maps(ScoreView D, ScoreParams P, MapsSource src, uint64_t n,
                                                                  const double* __restrict__ poses, uint32_t node_pose,
                                                                  ScorePartial* __restrict__ partial, float* __restrict__ node_d2,
                                                                  uint32_t* __restrict__ node_row) {
    __shared__ double s_score[4], s_d2[4];
    __shared__ uint32_t s_matched[4], s_terms[4];
    const uint32_t pose = blockIdx.y;
    const uint64_t i = (uint64_t)blockIdx.x * kScoreTile + threadIdx.x;
    ScoreAcc a;
    a.score = 0.0; a.d2_sum = 0.0; a.matched = 0u; a.terms = 0u;
    if (i < n) {
        ScoreBest b;
        b.d2 = (double)INFINITY; b.row = kNoRow;
        const bool counted = score_maps_row<NBH, false>(D, P, src, i, poses + 12 * (size_t)pose, a, b, nullptr);
        if (NODEWISE && pose == node_pose) {
            if (node_d2) node_d2[i] = counted ? (float)b.d2 : NAN;
            if (node_row) node_row[i] = b.row;
        }
    }
    constexpr int NW = kScoreTile / 64;
    const double score = score_block_sum<NW>(a.score, s_score), d2_sum = score_block_sum<NW>(a.d2_sum, s_d2);
    const uint32_t matched = score_block_sum<NW>(a.matched, s_matched), terms = score_block_sum<NW>(a.terms, s_terms);
    if (threadIdx.x == 0u) {
        ScorePartial* o = partial + (size_t)pose * gridDim.x + blockIdx.x;
        o->score = score; o->d2_sum = d2_sum; o->matched = matched; o->terms = terms;
    }
}

// The same with the 27 values: tile, grid, tree and partial record as k_score_derivs (k_score_derivs_reduce / _finish add them)
template <int NBH>
static __global__ void __launch_bounds__(kScoreTile) k_score_maps_derivs(ScoreView D, ScoreParams P, MapsSource src, uint64_t n,
                                                                         const double* __restrict__ poses,
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
        ScoreBest b;
        b.d2 = (double)INFINITY; b.row = kNoRow;
        (void)score_maps_row<NBH, true>(D, P, src, i, poses + 12 * (size_t)pose, a, b, o);
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
#endif

}  // namespace gndt
