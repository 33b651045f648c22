// gndt_footprint.hpp — footprint poses (include/gndt.h "footprint poses"): for K poses (x, y, z, hx, hy) of a rectangular vehicle the
// surface its footprint rests on.  The slopes under the rectangle are Gaussians (count, mean, scatter) and merge in closed form; the
// smallest eigenpair of the merged scatter (min_eigenpair_sym3<false>: no libm in its start value) is the supporting plane, from which tilt along and across the heading,
// the step between adjacent columns, the bump off the plane and the headroom follow.
//   k_footprint_poses   one pose a wavefront, kFootWaves wavefronts a workgroup.  The 64 lanes take the box positions p = lane, lane + 64,
//                       ... (at most kFootSlots = 16 each, in batches of kFootBatch whose loads are issued together, each step for the
//                       whole batch before the next one waits).  Per wavefront one table of the supports' mean z in LDS, addressed by
//                       box position, which the step between neighbours reads.  Nothing is atomic and nothing depends on arrival.
// THE ORDER OF THE SUMS (W, M, Q of the merge; part of the definition, see gndt.h): a lane adds the terms of its own positions in
// ascending p, starting from +0; then the 64 lane sums are folded in six rounds, offset = 32, 16, 8, 4, 2, 1: every lane l replaces
// its sum by sum[l] + sum[l ^ offset].  Addition commutes, so after each round lanes l and l ^ offset hold the same bits and after the
// sixth every lane holds the total.  Maxima and minima (step, bump, headroom) and the integer counts do not depend on any order.
// Everything up to the kernel is callable on the host: the CPU test tier runs the same code lane after lane (FootWaveHost,
// tests/footprint_shim.cpp).
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "gndt_score.hpp"

namespace gndt {

constexpr int kFootOk = 0, kFootBadPose = 1, kFootNoGround = 2, kFootSparse = 3;                   // GNDT_FOOT_* statuses
constexpr uint32_t kFootTilt = 1u, kFootStep = 2u, kFootCover = 4u, kFootLow = 8u;                 // GNDT_FOOT_* verdict bits
constexpr uint32_t kFootWeightCell = 0u, kFootWeightCount = 1u;
constexpr uint32_t kFootLanes = 64u, kFootSlots = 16u, kFootBatch = 4u, kFootMaxN = 15u, kFootTable = 1024u;
constexpr uint32_t kFootDefaultCells = 3u;
constexpr uint32_t kFootNoSupport = 0xFFFFFFFFu;         // the table's word for a position without a support (no finite float)

struct FootRule {                // gndt_footprint_params with its defaults resolved, and what the host forms once in fp64
    double len2, wid2;           // half_length^2, half_width^2
    double cos_max;              // cos(max_angle_deg)
    double min_cover;
    float max_dz, height, reach;
    uint32_t min_cells, weight;
    uint32_t n;                  // the box holds (2n + 1)^2 columns
};

struct FootInfo {                // gndt_footprint_info
    int32_t status;
    uint32_t flags, centre_row;
    uint16_t cells, support, gaps, unknown;
    float z, normal[3], along, across, rms, step_max, bump_max, headroom;
    uint32_t reserved;
};

struct FootLane {                // what one lane keeps between the passes
    uint32_t row[kFootSlots];    // the support of its s-th position (kNoRow: none)
    uint32_t col[kFootSlots];    // that column's first row
    double acc[10];              // W, M[3], Q[6] (xx, xy, xz, yy, yz, zz)
    uint32_t cells, support, gaps, unknown;
    double bump, head;           // the lane's largest |nrm . (d - dbar)| and least clearance above the plane
    float step;
};

struct FootPose {                // steps 1 - 3: the same in every lane
    double x, y, hx, hy, hh;
    float z0;
    uint32_t row, side, cells_in_box, centre;
    int sx_lo, sy_lo;
};

struct FootPlane {               // steps 6 - 7
    double W, dbar[3], nrm[3], lambda;
};

// The smallest index of a box axis: n non-zero indices below c
GNDT_HD int foot_lo(int c, int n) { return c > 0 && c - n <= 0 ? c - n - 1 : c - n; }

// A column's rows [c + from, c + min(from + kQueryChunk, ncol)) against z0 under the band: loads first, then the comparisons
GNDT_HD void foot_chunk(const QueryView& Q, uint32_t c, uint32_t ncol, uint32_t from, float z0, float max_dz, QueryBest& b) {
    int szv[kQueryChunk];
    uint32_t fl[kQueryChunk];
    float mz[kQueryChunk];
#pragma unroll
    for (uint32_t u = 0; u < kQueryChunk; ++u) {
        szv[u] = 0; fl[u] = 0u; mz[u] = 0.f;
        if (from + u < ncol) {
            const uint32_t t = c + from + u;
            szv[u] = Q.V.sz[t];
            fl[u] = Q.V.flags[t];
            mz[u] = Q.V.mean[3 * (size_t)t + 2];
        }
    }
    QueryKey k;
    k.sx = k.sy = k.sz = 0; k.ok = true;
#pragma unroll
    for (uint32_t u = 0; u < kQueryChunk; ++u)
        if (from + u < ncol && (max_dz == 0.f || fabsf(mz[u] - z0) <= max_dz))
            query_eval<kQueryNearestSlope>(c + from + u, szv[u], fl[u], mz[u], k, z0, b);
}

// Steps 1 - 3.  Returns the status (kFootOk: go on)
GNDT_HD int foot_centre(const QueryView& Q, const FootRule& F, const float* pose, FootPose& C) {
    const float x = pose[0], y = pose[1], z = pose[2], hx = pose[3], hy = pose[4];
    C.row = kNoRow;
    if (!(isfinite(x) && isfinite(y) && isfinite(z) && isfinite(hx) && isfinite(hy)) || (hx == 0.f && hy == 0.f)) return kFootBadPose;
    const QueryKey k = query_key<kQueryNearestSlope>(Q, x, y, z);
    const uint32_t slot = query_slot(Q, k);
    const uint32_t c = query_column(Q, k, Q.V.ctab_key[slot], Q.V.ctab_val[slot]);
    const uint32_t ncol = c != kNoColumn ? Q.V.row_ncol[c] : 0u;
    QueryBest b;
    b.row = kNoRow; b.d = 0.f; b.sz = 0;
    query_chunk<kQueryNearestSlope>(Q, c, ncol, 0u, k, z, b);
    query_rest<kQueryNearestSlope>(Q, c, ncol, k, z, b);
    if (b.row == kNoRow) return kFootNoGround;
    C.row = b.row;
    C.z0 = Q.V.mean[3 * (size_t)b.row + 2];
    C.x = (double)x; C.y = (double)y; C.hx = (double)hx; C.hy = (double)hy;
    C.hh = C.hx * C.hx + C.hy * C.hy;
    C.side = 2u * F.n + 1u;
    C.cells_in_box = C.side * C.side;
    C.centre = F.n * C.side + F.n;
    C.sx_lo = foot_lo(k.sx, (int)F.n);
    C.sy_lo = foot_lo(k.sy, (int)F.n);
    return kFootOk;
}

// Steps 4 - 6 for one lane's positions: the inside test, the support of every column under the vehicle, the lane's part of the sums.
// tab[p] = the support's mean z as bits, kFootNoSupport where position p has none.
GNDT_HD void foot_gather(const ScoreView& S, const FootRule& F, const FootPose& C, uint32_t lane, FootLane& L, uint32_t* tab) {
    const QueryView& Q = S.Q;
#pragma unroll
    for (uint32_t s = 0; s < kFootSlots; ++s) { L.row[s] = kNoRow; L.col[s] = kNoColumn; }
#pragma unroll
    for (int a = 0; a < 10; ++a) L.acc[a] = 0.0;
    L.cells = L.support = L.gaps = L.unknown = 0u;
#pragma unroll
    for (uint32_t s0 = 0; s0 < kFootSlots; s0 += kFootBatch) {
        if (s0 * kFootLanes >= C.cells_in_box) continue;    // (the same in every lane; no break: the loop unrolls, the arrays stay registers)
        bool in[kFootBatch];
        QueryKey k[kFootBatch];
        uint64_t skey[kFootBatch];
        uint32_t sval[kFootBatch], c[kFootBatch], ncol[kFootBatch];
        QueryBest b[kFootBatch];
#pragma unroll
        for (uint32_t u = 0; u < kFootBatch; ++u) {          // 4. inside; the first probe of the column index
            const uint32_t p = lane + (s0 + u) * kFootLanes;
            in[u] = false;
            k[u].sx = k[u].sy = 1; k[u].sz = 0; k[u].ok = false;
            skey[u] = kEmptyKey; sval[u] = kNoColumn;
            if (p < C.cells_in_box) {
                const uint32_t j = p / C.side, i = p - j * C.side;
                const int sx = raster_index(C.sx_lo, i), sy = raster_index(C.sy_lo, j);
                const double dx = axis_centre(sx, Q.ox, Q.grid_len) - C.x, dy = axis_centre(sy, Q.oy, Q.grid_len) - C.y;
                const double uu = dx * C.hx + dy * C.hy, vv = dy * C.hx - dx * C.hy;
                in[u] = (uu * uu <= F.len2 * C.hh && vv * vv <= F.wid2 * C.hh) || p == C.centre;
                k[u].sx = sx; k[u].sy = sy;
                k[u].ok = in[u] && sx >= -kMaxXY && sx <= kMaxXY && sy >= -kMaxXY && sy <= kMaxXY;
                if (k[u].ok) {
                    const uint32_t slot = query_slot(Q, k[u]);
                    skey[u] = Q.V.ctab_key[slot];
                    sval[u] = Q.V.ctab_val[slot];
                }
            }
        }
#pragma unroll
        for (uint32_t u = 0; u < kFootBatch; ++u) {          // 5. the column and its node count
            c[u] = query_column(Q, k[u], skey[u], sval[u]);
            ncol[u] = c[u] != kNoColumn ? Q.V.row_ncol[c[u]] : 0u;
        }
#pragma unroll
        for (uint32_t u = 0; u < kFootBatch; ++u) {          //    its rows: the first chunk of every position, then what is left
            b[u].row = kNoRow; b[u].d = 0.f; b[u].sz = 0;
            foot_chunk(Q, c[u], ncol[u], 0u, C.z0, F.max_dz, b[u]);
        }
#pragma unroll
        for (uint32_t u = 0; u < kFootBatch; ++u)
            for (uint32_t from = kQueryChunk; from < ncol[u]; from += kQueryChunk) foot_chunk(Q, c[u], ncol[u], from, C.z0, F.max_dz, b[u]);
#pragma unroll
        for (uint32_t u = 0; u < kFootBatch; ++u) {          // 6. the lane's sums, in ascending p
            const uint32_t p = lane + (s0 + u) * kFootLanes;
            if (p >= C.cells_in_box) continue;
            uint32_t word = kFootNoSupport;
            if (in[u]) {
                L.cells += 1u;
                const uint32_t row = p == C.centre ? C.row : b[u].row;
                if (c[u] == kNoColumn) L.unknown += 1u;
                else if (row == kNoRow) L.gaps += 1u;
                else {
                    L.support += 1u;
                    L.row[s0 + u] = row;
                    L.col[s0 + u] = c[u];
                    const float* m = Q.V.mean + 3 * (size_t)row;
                    const float* cv = S.cov + 6 * (size_t)row;
                    const double cnt = (double)S.count[row];
                    const double w = F.weight == kFootWeightCount ? cnt : 1.0, sc = w / cnt;
                    const double d[3] = {(double)m[0] - C.x, (double)m[1] - C.y, (double)m[2] - (double)C.z0};
                    const double wd[3] = {w * d[0], w * d[1], w * d[2]};
                    L.acc[0] += w;
                    L.acc[1] += wd[0]; L.acc[2] += wd[1]; L.acc[3] += wd[2];
                    L.acc[4] += wd[0] * d[0] + sc * (double)cv[0];
                    L.acc[5] += wd[0] * d[1] + sc * (double)cv[1];
                    L.acc[6] += wd[0] * d[2] + sc * (double)cv[2];
                    L.acc[7] += wd[1] * d[1] + sc * (double)cv[3];
                    L.acc[8] += wd[1] * d[2] + sc * (double)cv[4];
                    L.acc[9] += wd[2] * d[2] + sc * (double)cv[5];
                    word = float_bits(m[2]);
                }
            }
            tab[p] = word;
        }
    }
}

// Steps 6 - 7 from the folded sums
GNDT_HD void foot_plane(const double acc[10], FootPlane& P) {
    P.W = acc[0];
    for (int a = 0; a < 3; ++a) P.dbar[a] = acc[1 + a] / P.W;
    const double* q = acc + 4;
    const double wx = P.W * P.dbar[0], wy = P.W * P.dbar[1], wz = P.W * P.dbar[2];
    const double Sm[6] = {q[0] - wx * P.dbar[0], q[1] - wx * P.dbar[1], q[2] - wx * P.dbar[2],
                          q[3] - wy * P.dbar[1], q[4] - wy * P.dbar[2], q[5] - wz * P.dbar[2]};
    min_eigenpair_sym3<false>(Sm, P.lambda, P.nrm);     // (no fp32 trigonometric start value: the host must return the device's bits)
    if (P.nrm[2] < 0.0) { P.nrm[0] = -P.nrm[0]; P.nrm[1] = -P.nrm[1]; P.nrm[2] = -P.nrm[2]; }
}

// The plane's z above (x + ex, y + ey)
GNDT_HD double foot_plane_z(const FootPose& C, const FootPlane& P, double ex, double ey) {
    const double zc = (double)C.z0 + P.dbar[2];
    if (P.nrm[2] == 0.0) return zc;
    return zc - (P.nrm[0] * (ex - P.dbar[0]) + P.nrm[1] * (ey - P.dbar[1])) / P.nrm[2];
}

// Step 8 for one lane's positions
GNDT_HD void foot_shape(const ScoreView& S, const Robot& R, const FootPose& C, const FootPlane& P, uint32_t lane, FootLane& L,
                        const uint32_t* tab) {
    const QueryView& Q = S.Q;
    L.step = 0.f; L.bump = 0.0; L.head = DBL_MAX;
#pragma unroll
    for (uint32_t s = 0; s < kFootSlots; ++s) {
        const uint32_t p = lane + s * kFootLanes;
        if (p >= C.cells_in_box || L.row[s] == kNoRow) continue;
        const uint32_t row = L.row[s], j = p / C.side, i = p - j * C.side;
        const float* m = Q.V.mean + 3 * (size_t)row;
        const float mz = m[2];
        if (i + 1u < C.side && tab[p + 1u] != kFootNoSupport) L.step = fmaxf(L.step, fabsf(bits_float(tab[p + 1u]) - mz));
        if (j + 1u < C.side && tab[p + C.side] != kFootNoSupport) L.step = fmaxf(L.step, fabsf(bits_float(tab[p + C.side]) - mz));
        const double e[3] = {((double)m[0] - C.x) - P.dbar[0], ((double)m[1] - C.y) - P.dbar[1], ((double)mz - (double)C.z0) - P.dbar[2]};
        L.bump = fmax(L.bump, fabs((P.nrm[0] * e[0] + P.nrm[1] * e[1]) + P.nrm[2] * e[2]));
        const uint32_t c = L.col[s], ncol = Q.V.row_ncol[c];
        const double ex = axis_centre(raster_index(C.sx_lo, i), Q.ox, Q.grid_len) - C.x;
        const double ey = axis_centre(raster_index(C.sy_lo, j), Q.oy, Q.grid_len) - C.y;
        const double zp = foot_plane_z(C, P, ex, ey);
        const float over = mz + R.reach;
        for (uint32_t t = c; t < c + ncol; ++t) {
            const float tz = Q.V.mean[3 * (size_t)t + 2];
            if ((Q.V.flags[t] & 1u) && tz > over) L.head = fmin(L.head, (double)tz - zp);
        }
    }
}

// Steps 7 - 9: the record of an OK or SPARSE pose from the folded counts, sums and extremes
GNDT_HD void foot_finish(const Robot& R, const FootRule& F, const FootPose& C, const FootPlane& P, bool sparse, const FootLane& T, FootInfo& o) {
    o.status = sparse ? kFootSparse : kFootOk;
    o.flags = 0u;
    o.centre_row = C.row;
    o.cells = (uint16_t)T.cells; o.support = (uint16_t)T.support; o.gaps = (uint16_t)T.gaps; o.unknown = (uint16_t)T.unknown;
    o.z = 0.f; o.normal[0] = o.normal[1] = o.normal[2] = 0.f; o.along = o.across = 0.f;
    o.rms = o.step_max = o.bump_max = o.headroom = 0.f;
    o.reserved = 0u;
    if (sparse) return;
    const double nz = P.nrm[2];
    o.rms = (float)sqrt(fmax(P.lambda, 0.0) / P.W);
    o.normal[0] = (float)P.nrm[0]; o.normal[1] = (float)P.nrm[1]; o.normal[2] = (float)nz;
    if (nz == 0.0) {
        o.z = (float)((double)C.z0 + P.dbar[2]);
    } else {
        const double rh = sqrt(C.hh), fx = C.hx / rh, fy = C.hy / rh;
        o.z = (float)(((double)C.z0 + P.dbar[2]) + (P.nrm[0] * P.dbar[0] + P.nrm[1] * P.dbar[1]) / nz);
        o.along = (float)(-(P.nrm[0] * fx + P.nrm[1] * fy) / nz);
        o.across = (float)(-(P.nrm[1] * fx - P.nrm[0] * fy) / nz);
    }
    o.step_max = T.step;
    o.bump_max = (float)T.bump;
    o.headroom = T.head == DBL_MAX ? FLT_MAX : (float)T.head;
    if (nz < F.cos_max) o.flags |= kFootTilt;
    if (o.step_max > R.reach) o.flags |= kFootStep;
    if ((double)T.support < F.min_cover * (double)T.cells) o.flags |= kFootCover;
    if (F.height > 0.f && o.headroom < F.height) o.flags |= kFootLow;
}

GNDT_HD void foot_none(int status, uint32_t centre_row, FootInfo& o) {
    o.status = status; o.flags = 0u; o.centre_row = centre_row;
    o.cells = o.support = o.gaps = o.unknown = 0;
    o.z = 0.f; o.normal[0] = o.normal[1] = o.normal[2] = 0.f; o.along = o.across = 0.f;
    o.rms = o.step_max = o.bump_max = o.headroom = 0.f;
    o.reserved = 0u;
}

// One pose through a wavefront w (FootWaveDevice / FootWaveHost): rows[row_cap] (or null with 0) the supports in box order
template <typename W>
GNDT_HD void foot_pose(const ScoreView& S, const Robot& R, const FootRule& F, const float* pose, uint32_t* rows, uint32_t row_cap, W& w, FootInfo& o) {
    FootPose C;
    const int st = foot_centre(S.Q, F, pose, C);
    if (st != kFootOk) {
        foot_none(st, kNoRow, o);
        w.each([&](uint32_t lane, FootLane&) { for (uint32_t i = lane; i < row_cap; i += kFootLanes) rows[i] = kNoRow; });
        return;
    }
    uint32_t* tab = w.table();
    w.fence();                                               // (the last pose's readers of the table are done)
    w.each([&](uint32_t lane, FootLane& L) { foot_gather(S, F, C, lane, L, tab); });
    w.fence();
    w.fold_sums();
    const FootLane& T = w.total();
    const bool sparse = T.support < F.min_cells;
    FootPlane P;
    P.W = 0.0; P.lambda = 0.0;
    P.dbar[0] = P.dbar[1] = P.dbar[2] = 0.0; P.nrm[0] = P.nrm[1] = 0.0; P.nrm[2] = 1.0;
    if (!sparse) {
        foot_plane(T.acc, P);
        w.each([&](uint32_t lane, FootLane& L) { foot_shape(S, R, C, P, lane, L, tab); });
        w.fold_shape();
    }
    foot_finish(R, F, C, P, sparse, w.total(), o);
    if (row_cap) {
        uint32_t base = 0u;
#pragma unroll
        for (uint32_t s = 0; s < kFootSlots; ++s) {
            if (s * kFootLanes >= C.cells_in_box) continue;
            const uint64_t have = w.ballot([&](uint32_t, const FootLane& L) { return L.row[s] != kNoRow; });
            w.each([&](uint32_t lane, FootLane& L) {
                const uint32_t at = base + (uint32_t)__builtin_popcountll(have & ((1ull << lane) - 1ull));
                if (((have >> lane) & 1ull) && at < row_cap) rows[at] = L.row[s];
            });
            base += (uint32_t)__builtin_popcountll(have);
        }
        w.each([&](uint32_t lane, FootLane&) { for (uint32_t i = base + lane; i < row_cap; i += kFootLanes) rows[i] = kNoRow; });
    }
}

struct FootWaveHost {            // the wavefront lane after lane: the collectives in the kernel's order
    FootLane L[kFootLanes];
    uint32_t tab[kFootTable];
    uint32_t* table() { return tab; }
    void fence() {}
    template <typename F> void each(F f) { for (uint32_t l = 0; l < kFootLanes; ++l) f(l, L[l]); }
    template <typename F> uint64_t ballot(F f) {
        uint64_t m = 0;
        for (uint32_t l = 0; l < kFootLanes; ++l) m |= f(l, (const FootLane&)L[l]) ? 1ull << l : 0ull;
        return m;
    }
    void fold_sums() {
        for (uint32_t off = 32u; off; off >>= 1) {
            double t[kFootLanes][10];
            uint32_t n[kFootLanes][4];
            for (uint32_t l = 0; l < kFootLanes; ++l) {
                const FootLane &a = L[l], &b = L[l ^ off];
                for (int i = 0; i < 10; ++i) t[l][i] = a.acc[i] + b.acc[i];
                n[l][0] = a.cells + b.cells; n[l][1] = a.support + b.support; n[l][2] = a.gaps + b.gaps; n[l][3] = a.unknown + b.unknown;
            }
            for (uint32_t l = 0; l < kFootLanes; ++l) {
                for (int i = 0; i < 10; ++i) L[l].acc[i] = t[l][i];
                L[l].cells = n[l][0]; L[l].support = n[l][1]; L[l].gaps = n[l][2]; L[l].unknown = n[l][3];
            }
        }
    }
    void fold_shape() {
        for (uint32_t l = 1; l < kFootLanes; ++l) {
            L[0].step = fmaxf(L[0].step, L[l].step); L[0].bump = fmax(L[0].bump, L[l].bump); L[0].head = fmin(L[0].head, L[l].head);
        }
    }
    const FootLane& total() const { return L[0]; }
};

}  // namespace gndt

#if defined(__HIPCC__)
namespace gndt {

struct FootWaveDevice {
    FootLane L;
    uint32_t* tab;               // this wavefront's table in LDS
    __device__ __forceinline__ uint32_t* table() { return tab; }
    // the table is written by some lanes and read by others of the same wavefront: order the LDS accesses across the lanes
    __device__ __forceinline__ void fence() {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    template <typename F> __device__ __forceinline__ void each(F f) { f((uint32_t)(threadIdx.x & 63u), L); }
    template <typename F> __device__ __forceinline__ uint64_t ballot(F f) {
        return __ballot(f((uint32_t)(threadIdx.x & 63u), (const FootLane&)L) ? 1 : 0);
    }
    __device__ __forceinline__ void fold_sums() {
#pragma unroll
        for (int off = 32; off; off >>= 1) {
#pragma unroll
            for (int i = 0; i < 10; ++i) L.acc[i] = L.acc[i] + __shfl_xor(L.acc[i], off, 64);
            L.cells += __shfl_xor(L.cells, off, 64);
            L.support += __shfl_xor(L.support, off, 64);
            L.gaps += __shfl_xor(L.gaps, off, 64);
            L.unknown += __shfl_xor(L.unknown, off, 64);
        }
    }
    __device__ __forceinline__ void fold_shape() {
#pragma unroll
        for (int off = 32; off; off >>= 1) {
            L.step = fmaxf(L.step, __shfl_xor(L.step, off, 64));
            L.bump = fmax(L.bump, __shfl_xor(L.bump, off, 64));
            L.head = fmin(L.head, __shfl_xor(L.head, off, 64));
        }
    }
    __device__ __forceinline__ const FootLane& total() const { return L; }
};

// One pose a wavefront, kFootWaves wavefronts a workgroup that share nothing but the LDS array (a table each, no barrier); grid-stride
// over the poses.  info: four 16-byte stores a pose, by the wavefront's first lane.
constexpr int kFootWaves = 4, kFootThreads = kFootWaves * 64, kFootMaxBlocks = 1024;
static __global__ void __launch_bounds__(kFootThreads) k_footprint_poses(ScoreView S, Robot R, FootRule F, const char* __restrict__ poses,
                                                                        uint64_t K, uint64_t stride, uint32_t* __restrict__ rows,
                                                                        uint32_t row_cap, FootInfo* __restrict__ info) {
    __shared__ uint32_t tab[kFootWaves][kFootTable];
    FootWaveDevice w;
    w.tab = tab[threadIdx.x >> 6];
    const uint64_t waves = (uint64_t)gridDim.x * kFootWaves;
    for (uint64_t k = (uint64_t)blockIdx.x * kFootWaves + (threadIdx.x >> 6); k < K; k += waves) {
        FootInfo o;
        foot_pose(S, R, F, reinterpret_cast<const float*>(poses + k * stride), rows ? rows + k * row_cap : nullptr, row_cap, w, o);
        if ((threadIdx.x & 63u) == 0u) {
            uint4* out = reinterpret_cast<uint4*>(info + k);
            out[0] = make_uint4((uint32_t)o.status, o.flags, o.centre_row, (uint32_t)o.cells | ((uint32_t)o.support << 16));
            out[1] = make_uint4((uint32_t)o.gaps | ((uint32_t)o.unknown << 16), float_bits(o.z), float_bits(o.normal[0]), float_bits(o.normal[1]));
            out[2] = make_uint4(float_bits(o.normal[2]), float_bits(o.along), float_bits(o.across), float_bits(o.rms));
            out[3] = make_uint4(float_bits(o.step_max), float_bits(o.bump_max), float_bits(o.headroom), 0u);
        }
    }
}

}  // namespace gndt
#endif  // __HIPCC__
