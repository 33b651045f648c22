// gndt_score.hpp — scan scoring (include/gndt.h "scan scoring"): the NDT match score of n scan points against the finished grid for K
// poses at once.  The map's nodes are read as what the build made them — normal distributions (count, mean, un-normalised scatter) —
// which no other consumer does: the flood, the queries, the rasters, crop and clear read the rows as geometry only.
//
// Per (point, pose) pair: the pose applied in fp64 (score_transform), the GNDT_QUERY_NODE key of the moved point (query_key), the
// query's lookup chain (query_slot -> query_column -> row_ncol -> the column's sz in chunks), then count, mean and cov of every
// candidate row and one Mahalanobis distance each (score_node).  DIRECT7 adds the six face neighbours: the two vertical ones come out
// of the walk of the point's own column, the four side columns cost one probe each, all four issued before any is waited for.
//
// The arithmetic of one term, in this order (tests/score_ref.py keeps to it), everything fp64 from the rows' fp32 values:
//     r   = 1 / (count - 1)                        C_ij = S_ij * r                 (S = cov: xx, xy, xz, yy, yz, zz)
//     eps = max(cov_rel * (((C_xx + C_yy) + C_zz) / 3), cov_floor)
//     a00 = C_xx + eps, a11 = C_yy + eps, a22 = C_zz + eps, a01 = C_xy, a02 = C_xz, a12 = C_yz
//     c00 = a11 a22 - a12 a12     c01 = a02 a12 - a01 a22     c02 = a01 a12 - a02 a11          (cofactors: the adjugate is symmetric)
//     c11 = a00 a22 - a02 a02     c12 = a01 a02 - a00 a12     c22 = a00 a11 - a01 a01
//     det = (a00 c00 + a01 c01) + a02 c02
//     d   = q - mean                               u_i = (c_i0 d_x + c_i1 d_y) + c_i2 d_z
//     d2  = ((d_x u_x + d_y u_y) + d_z u_z) / det  term = exp(-0.5 d2)
// No product is fused with a sum (the library is built with -ffp-contract=off).  eps > 0 always, so det > 0: with cov_rel = 0.01 the
// condition number of A is at most 301 whatever the node's shape.
// A thread adds its terms in the candidates' order: the point's node, x - 1, x + 1, y - 1, y + 1, the level above, the level below.
// A workgroup owns kScoreTile consecutive points of one pose and adds its threads' sums in a fixed tree (the 64 lanes by __shfl_xor,
// then the waves pairwise through LDS); k_score_reduce adds a pose's tiles in tile order per thread, then in the same tree.  No
// floating-point atomics: a pose's record has the same bits in every run, in every batch and on every stream.
// score_point hands every counted candidate (ScoreTerm: d, the cofactors, det, u, d2) and its term to a sink: plain scoring passes
// ScoreNoSink, the score's derivatives (gndt_score_derivs.hpp) add their per-point sums there, on the same lookup.
// Everything but the kernels is callable on the host as well (tests/score_shim.cpp).
#pragma once
#include <math.h>
#include <stdint.h>

#include "gndt_query.hpp"

namespace gndt {

constexpr int kScoreDirect1 = 1, kScoreDirect7 = 7;      // GNDT_SCORE_DIRECT1, GNDT_SCORE_DIRECT7
constexpr uint32_t kScoreTile = 256;                     // points of one workgroup: fixed, so that a pose's partial sums do not depend on K
constexpr uint32_t kScoreReduceBlock = 1024;             // threads of the workgroup that adds a pose's tiles

struct ScoreView {
    QueryView Q;                    // the rows, the column index, origin and cell sizes as the point queries read them
    const uint32_t* count;
    const float* cov;               // [rows][6]
};

struct ScoreParams {                // gndt_score_params with the defaults filled in
    uint32_t min_count;
    double cov_rel, cov_floor, max_d2;      // the struct's floats, widened; max_d2 = 0: no gate
};

struct ScoreAcc {                   // one thread's (then one workgroup's) share of a pose's record
    double score, d2_sum;
    uint32_t matched, terms;
};

struct ScoreBest {                  // the point's nearest candidate (in d2): +inf / kNoRow when it has no term
    double d2;
    uint32_t row;
};

// q = (float)(T p), T = [R | t] row-major 3 x 4: fp64, left to right, one rounding to fp32 per coordinate
GNDT_HD void score_transform(const double* T, float x, float y, float z, float& qx, float& qy, float& qz) {
    const double dx = (double)x, dy = (double)y, dz = (double)z;
    qx = (float)(((T[0] * dx + T[1] * dy) + T[2] * dz) + T[3]);
    qy = (float)(((T[4] * dx + T[5] * dy) + T[6] * dz) + T[7]);
    qz = (float)(((T[8] * dx + T[9] * dy) + T[10] * dz) + T[11]);
}

// One counted candidate as a sink of score_point receives it: d = q - mean, the cofactors of A, det, u = adj(A) d and d2
struct ScoreTerm {
    double dx, dy, dz;
    double c00, c01, c02, c11, c12, c22, det;
    double ux, uy, uz, d2;
};

// The cofactors of A and its determinant from a node's count and scatter (the order of the header comment): the one statement of it,
// shared by score_node and ray casting's NDT mode (gndt_cast.hpp)
GNDT_HD void score_cofactors(uint32_t c, float s0, float s1, float s2, float s3, float s4, float s5, double cov_rel, double cov_floor,
                             ScoreTerm& t) {
    const double r = 1.0 / (double)(c - 1u);
    const double cxx = (double)s0 * r, cxy = (double)s1 * r, cxz = (double)s2 * r, cyy = (double)s3 * r, cyz = (double)s4 * r,
                 czz = (double)s5 * r;
    const double eps = fmax(cov_rel * (((cxx + cyy) + czz) / 3.0), cov_floor);
    const double a00 = cxx + eps, a11 = cyy + eps, a22 = czz + eps, a01 = cxy, a02 = cxz, a12 = cyz;
    t.c00 = a11 * a22 - a12 * a12; t.c01 = a02 * a12 - a01 * a22; t.c02 = a01 * a12 - a02 * a11;
    t.c11 = a00 * a22 - a02 * a02; t.c12 = a01 * a02 - a00 * a12; t.c22 = a00 * a11 - a01 * a01;
    t.det = (a00 * t.c00 + a01 * t.c01) + a02 * t.c02;
}

// u = adj(A) d and d2 = d^T u / det from t's d, cofactors and det
GNDT_HD void score_d2(ScoreTerm& t) {
    t.ux = (t.c00 * t.dx + t.c01 * t.dy) + t.c02 * t.dz;
    t.uy = (t.c01 * t.dx + t.c11 * t.dy) + t.c12 * t.dz;
    t.uz = (t.c02 * t.dx + t.c12 * t.dy) + t.c22 * t.dz;
    t.d2 = ((t.dx * t.ux + t.dy * t.uy) + t.dz * t.uz) / t.det;
}

// The term of q against the node of `row` (the order of the header comment); false: the node is not a candidate (too few points, or
// beyond max_d2)
GNDT_HD bool score_node(const ScoreView& S, const ScoreParams& P, uint32_t row, float qx, float qy, float qz, ScoreTerm& t) {
    const uint32_t c = S.count[row];
    const float* m = S.Q.V.mean + 3 * (size_t)row;
    const float* s = S.cov + 6 * (size_t)row;
    const float mx = m[0], my = m[1], mz = m[2];
    const float s0 = s[0], s1 = s[1], s2 = s[2], s3 = s[3], s4 = s[4], s5 = s[5];
    if (c < P.min_count) return false;
    score_cofactors(c, s0, s1, s2, s3, s4, s5, P.cov_rel, P.cov_floor, t);
    t.dx = (double)qx - (double)mx; t.dy = (double)qy - (double)my; t.dz = (double)qz - (double)mz;
    score_d2(t);
    return !(P.max_d2 > 0.0 && t.d2 > P.max_d2);
}

// d2 alone
GNDT_HD bool score_node(const ScoreView& S, const ScoreParams& P, uint32_t row, float qx, float qy, float qz, double& d2) {
    ScoreTerm t;
    const bool counted = score_node(S, P, row, qx, qy, qz, t);
    d2 = t.d2;
    return counted;
}

// The rows of column c (ncol nodes) whose levels are lv[0 .. NT): row[t], left alone where the column has no such level or !want[t].
// The query's walk (kQueryChunk levels loaded, then compared); a one-level walk stops at its node.
template <int NT>
GNDT_HD void score_walk(const CostView& V, uint32_t c, uint32_t ncol, const int* lv, const bool* want, uint32_t* row) {
    for (uint32_t from = 0; from < ncol && !(NT == 1 && row[0] != kNoRow); from += kQueryChunk) {
        int szv[kQueryChunk];
#pragma unroll
        for (uint32_t u = 0; u < kQueryChunk; ++u) szv[u] = from + u < ncol ? V.sz[c + from + u] : 0;      // (0 is no level)
#pragma unroll
        for (uint32_t u = 0; u < kQueryChunk; ++u)
#pragma unroll
            for (int t = 0; t < NT; ++t)
                if (want[t] && from + u < ncol && szv[u] == lv[t]) row[t] = c + from + u;
    }
}

// The sink of plain scoring: a counted candidate is looked at by nobody else
struct ScoreNoSink {
    GNDT_HD void operator()(uint32_t, const ScoreTerm&, double) const {}
};

// One candidate row into the thread's sums and the point's best (equal d2: the lower row); sink(row, term, exp(-d2 / 2)) for a counted one
template <typename SINK>
GNDT_HD void score_add(const ScoreView& S, const ScoreParams& P, uint32_t row, float qx, float qy, float qz, ScoreAcc& a, ScoreBest& b,
                       uint32_t& found, SINK& sink) {
    if (row == kNoRow) return;
    ScoreTerm t;
    if (!score_node(S, P, row, qx, qy, qz, t)) return;
    const double e = exp(-0.5 * t.d2);
    a.score += e;
    a.d2_sum += t.d2;
    ++a.terms;
    ++found;
    if (t.d2 < b.d2 || (t.d2 == b.d2 && row < b.row)) { b.d2 = t.d2; b.row = row; }
    sink(row, t, e);
}

// The moved point q against the map: its terms into a (matched: at least one), its nearest candidate into b, every counted candidate
// to the sink in the candidates' order
template <int NBH, typename SINK>
GNDT_HD void score_point(const ScoreView& S, const ScoreParams& P, float qx, float qy, float qz, ScoreAcc& a, ScoreBest& b, SINK& sink) {
    const QueryView& Q = S.Q;
    const QueryKey k = query_key<kQueryNode>(Q, qx, qy, qz);
    uint32_t found = 0u;
    if (NBH == kScoreDirect1) {
        const uint32_t slot = query_slot(Q, k);
        const uint64_t skey = Q.V.ctab_key[slot];
        const uint32_t sval = Q.V.ctab_val[slot];
        const uint32_t c = query_column(Q, k, skey, sval);
        const uint32_t ncol = c != kNoColumn ? Q.V.row_ncol[c] : 0u;
        uint32_t row[1] = {kNoRow};
        const int lv[1] = {k.sz};
        const bool want[1] = {true};
        score_walk<1>(Q.V, c, ncol, lv, want, row);
        score_add(S, P, row[0], qx, qy, qz, a, b, found, sink);
    } else {
        // columns: the point's own, x - 1, x + 1, y - 1, y + 1 (signed indices skip 0; beyond the codec's range: no candidate)
        QueryKey kc[5];
        kc[0] = k;
#pragma unroll
        for (int j = 1; j < 5; ++j) {
            kc[j] = k;
            const int d = (j & 1) ? -1 : +1;
            if (j <= 2) kc[j].sx = step_skip0(k.sx, d); else kc[j].sy = step_skip0(k.sy, d);
            const int v = j <= 2 ? kc[j].sx : kc[j].sy;
            kc[j].ok = k.ok && v >= -kMaxXY && v <= kMaxXY;
        }
        uint32_t slot[5], sval[5], c[5], ncol[5];
        uint64_t skey[5];
#pragma unroll
        for (int j = 0; j < 5; ++j) {               // the five probes together
            slot[j] = query_slot(Q, kc[j]);
            skey[j] = Q.V.ctab_key[slot[j]];
            sval[j] = Q.V.ctab_val[slot[j]];
        }
#pragma unroll
        for (int j = 0; j < 5; ++j) {               // then the five node counts
            c[j] = query_column(Q, kc[j], skey[j], sval[j]);
            ncol[j] = c[j] != kNoColumn ? Q.V.row_ncol[c[j]] : 0u;
        }
        // the point's own column gives its node and the levels above and below it
        uint32_t own[3] = {kNoRow, kNoRow, kNoRow};
        const int lv[3] = {k.sz, level_above(k.sz), level_below(k.sz)};
        const bool want[3] = {true, lv[1] <= kMaxZ, lv[2] >= -kMaxZ};
        score_walk<3>(Q.V, c[0], ncol[0], lv, want, own);
        uint32_t side[4] = {kNoRow, kNoRow, kNoRow, kNoRow};
#pragma unroll
        for (int j = 1; j < 5; ++j) score_walk<1>(Q.V, c[j], ncol[j], lv, want, side + (j - 1));
        score_add(S, P, own[0], qx, qy, qz, a, b, found, sink);
#pragma unroll
        for (int j = 0; j < 4; ++j) score_add(S, P, side[j], qx, qy, qz, a, b, found, sink);
        score_add(S, P, own[1], qx, qy, qz, a, b, found, sink);
        score_add(S, P, own[2], qx, qy, qz, a, b, found, sink);
    }
    if (found) ++a.matched;
}

template <int NBH>
GNDT_HD void score_point(const ScoreView& S, const ScoreParams& P, float qx, float qy, float qz, ScoreAcc& a, ScoreBest& b) {
    ScoreNoSink none;
    score_point<NBH>(S, P, qx, qy, qz, a, b, none);
}

struct ScorePartial {               // one workgroup's sums: partial[pose][tile]
    double score, d2_sum;
    uint32_t matched, terms;
};

struct ScoreRecord {                // gndt_pose_score
    double score, d2_sum;
    uint64_t matched, terms;
};

#if defined(__HIPCC__)
// The fixed tree: lane l ends with the sum of its wave, formed as ((v_l + v_{l^32}) + ...) — the same bits in every lane
template <typename T>
static __device__ __forceinline__ T score_wave_sum(T v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// The workgroup's NW wave sums through LDS, added pairwise: ((w0 + w1) + (w2 + w3)) + ... — the same bits in every thread
template <int NW, typename T>
static __device__ __forceinline__ T score_block_sum(T v, T* lds) {
    v = score_wave_sum(v);
    if ((threadIdx.x & 63u) == 0u) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    T s[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) s[w] = lds[w];
#pragma unroll
    for (int w = NW; w > 1; w >>= 1)
#pragma unroll
        for (int i = 0; i < w / 2; ++i) s[i] = s[2 * i] + s[2 * i + 1];
    return s[0];
}

// One thread per (point, pose): blockIdx.x the tile of kScoreTile points, blockIdx.y the pose (uniform over the workgroup: its twelve
// doubles are scalar loads).  partial[pose * tiles + tile] = the workgroup's sums.  POINTWISE: the workgroups of `point_pose` also
// store every point's least d2 (fp32, +inf: no term) and that node's row (kNoRow) where the pointers are not null.
template <int NBH, bool POINTWISE>
static __global__ void __launch_bounds__(kScoreTile) k_score(ScoreView S, ScoreParams P, const float* __restrict__ xyz, uint32_t sf, uint64_t n,
                                                             const double* __restrict__ poses, uint32_t point_pose,
                                                             ScorePartial* __restrict__ partial, float* __restrict__ point_d2,
                                                             uint32_t* __restrict__ point_row) {
    __shared__ double s_score[4], s_d2[4];
    __shared__ uint32_t s_matched[4], s_terms[4];
    const uint32_t pose = blockIdx.y;
    const uint64_t i = (uint64_t)blockIdx.x * kScoreTile + threadIdx.x;
    ScoreAcc a;
    a.score = 0.0; a.d2_sum = 0.0; a.matched = 0u; a.terms = 0u;
    if (i < n) {
        const float* p = xyz + i * sf;
        float qx, qy, qz;
        score_transform(poses + 12 * (size_t)pose, p[0], p[1], p[2], qx, qy, qz);
        ScoreBest b;
        b.d2 = (double)INFINITY; b.row = kNoRow;
        score_point<NBH>(S, P, qx, qy, qz, a, b);
        if (POINTWISE && pose == point_pose) {
            if (point_d2) point_d2[i] = (float)b.d2;
            if (point_row) point_row[i] = b.row;
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

// One workgroup of kScoreReduceBlock threads per pose: thread t adds tiles t, t + kScoreReduceBlock, ... in that order (four loads
// in flight: the walk is bound by their latency), then the same tree over its 16 waves
static __global__ void __launch_bounds__(kScoreReduceBlock) k_score_reduce(const ScorePartial* __restrict__ partial, uint32_t tiles,
                                                                           ScoreRecord* __restrict__ out) {
    constexpr int NW = kScoreReduceBlock / 64;
    __shared__ double s_score[NW], s_d2[NW];
    __shared__ unsigned long long s_matched[NW], s_terms[NW];
    const ScorePartial* p = partial + (size_t)blockIdx.x * tiles;
    double score = 0.0, d2_sum = 0.0;
    unsigned long long matched = 0ull, terms = 0ull;
    for (uint32_t t0 = threadIdx.x; t0 < tiles; t0 += 4u * kScoreReduceBlock) {
        ScorePartial r[4];
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j) {
            const uint32_t t = t0 + j * kScoreReduceBlock;      // (tiles < 2^31: no wrap)
            r[j].score = 0.0; r[j].d2_sum = 0.0; r[j].matched = 0u; r[j].terms = 0u;      // (adding a zero record changes no bit)
            if (t < tiles) r[j] = p[t];
        }
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j) { score += r[j].score; d2_sum += r[j].d2_sum; matched += r[j].matched; terms += r[j].terms; }
    }
    score = score_block_sum<NW>(score, s_score); d2_sum = score_block_sum<NW>(d2_sum, s_d2);
    matched = score_block_sum<NW>(matched, s_matched); terms = score_block_sum<NW>(terms, s_terms);
    if (threadIdx.x == 0u) {
        ScoreRecord* o = out + blockIdx.x;
        o->score = score; o->d2_sum = d2_sum; o->matched = matched; o->terms = terms;
    }
}
#endif

}  // namespace gndt
