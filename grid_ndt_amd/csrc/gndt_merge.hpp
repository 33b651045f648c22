// gndt_merge.hpp — map merge (gndt_merge_map_device, include/gndt.h): one map folded into another under a rigid transform, from the
// source's node table alone.
//
// A source node is a Gaussian with a count: n points, mean m = c + Sum v / n, central scatter S = Sum v v^T - Sum v (Sum v)^T / n about
// its centre c.  Under x' = R x + t the mean goes to m' = R m + t and the scatter to S' = R S R^T; the node whose cell m' falls into (the
// destination's origin and lengths) receives the n points' statistics about ITS centre c', with u = m' - c':
//     Sum v'        = n u
//     Sum v' v'^T_ab = S'_ab + n u_a u_b
// Counts add, first-seen indices take the minimum with base + first (base: the destination's stream position before the call).  A node
// is kept whole: the moment match does not split a source node that straddles destination cells.
//   k_merge_map   source node list -> destination node table, one pass      reads 4 + 88 B per source node, eleven atomics per node out
// The per-node arithmetic is GNDT_HD: tests/merge_shim.cpp compiles it for the host.
#pragma once
#include <stdint.h>

#include "gndt_math.hpp"

namespace gndt {

struct MergeParams {
    double R[9], t[3];                       // row-major [R | t], destination <- source
    float so[3], sgl, szl;                   // the source's origin, grid_len, z_len
    float dorg[3], dgl, dzl;                 // the destination's
    uint32_t min_count;                      // source nodes with fewer points stay behind
    uint32_t base;                           // the destination's stream position before the call
    uint32_t new_pos;                        // ... and after it: base + the source's
};

// One source node (key, n >= 1 points, sums[9] about its centre) -> the destination key and the nine sums about that node's centre.
// false: the moved mean has a non-finite coordinate or no key in the codec's range — the node does not travel.
// Evaluation order (fp64, one IEEE operation at a time, no FMA contraction; tests/merge_ref.py follows it bit for bit):
//   1. mu_a = sums[a] / (double)n                      m_a = c_a + mu_a                       c = axis_centre of the key, SOURCE geometry
//   2. S_ab = sums[3+ab] - sums[a] * mu_b              ab = xx, xy, xz, yy, yz, zz
//   3. m'_i = ((R_i0 m_x + R_i1 m_y) + R_i2 m_z) + t_i
//   4. key' = point_key((float)m'_x, (float)m'_y, (float)m'_z)                                DESTINATION geometry
//   5. W_ib = (R_i0 S_0b + R_i1 S_1b) + R_i2 S_2b      S'_ij = (W_i0 R_j0 + W_i1 R_j1) + W_i2 R_j2      (S symmetric, i <= j)
//   6. c' = axis_centre of key'                                                               DESTINATION geometry
//   7. u_a = m'_a - c'_a     nu_a = (double)n * u_a    out[a] = nu_a    out[3+ab] = S'_ab + nu_a * u_b
GNDT_HD bool merge_node(uint64_t key, uint32_t n, const double sums[9], const MergeParams& P, uint64_t& key_out, double out[9]) {
    int sx, sy, sz;
    unpack_key(key, sx, sy, sz);
    const double c[3] = {axis_centre(sx, P.so[0], P.sgl), axis_centre(sy, P.so[1], P.sgl), axis_centre(sz, P.so[2], P.szl)};
    const double dn = (double)n;
    double mu[3], m[3];
    for (int a = 0; a < 3; ++a) { mu[a] = sums[a] / dn; m[a] = c[a] + mu[a]; }
    double S[3][3];
    int k = 3;
    for (int a = 0; a < 3; ++a)
        for (int b = a; b < 3; ++b, ++k) {
            const double p = sums[a] * mu[b];
            S[a][b] = S[b][a] = sums[k] - p;
        }
    double mp[3];
    float mf[3];
    for (int i = 0; i < 3; ++i) {
        const double p0 = P.R[3 * i] * m[0], p1 = P.R[3 * i + 1] * m[1], p2 = P.R[3 * i + 2] * m[2];
        mp[i] = ((p0 + p1) + p2) + P.t[i];
        mf[i] = (float)mp[i];
        if (!(fabsf(mf[i]) <= 3.4028234663852886e38f)) return false;      // inf or NaN (a finite double beyond fp32 rounds to inf)
    }
    const PointKey pk = point_key(mf[0], mf[1], mf[2], P.dorg[0], P.dorg[1], P.dorg[2], P.dgl, P.dzl);
    if (!pk.ok) return false;
    key_out = pack_key(pk.sx, pk.sy, pk.sz);
    double W[3][3];
    for (int i = 0; i < 3; ++i)
        for (int b = 0; b < 3; ++b) {
            const double p0 = P.R[3 * i] * S[0][b], p1 = P.R[3 * i + 1] * S[1][b], p2 = P.R[3 * i + 2] * S[2][b];
            W[i][b] = (p0 + p1) + p2;
        }
    const double cd[3] = {axis_centre(pk.sx, P.dorg[0], P.dgl), axis_centre(pk.sy, P.dorg[1], P.dgl), axis_centre(pk.sz, P.dorg[2], P.dzl)};
    double u[3], nu[3];
    for (int a = 0; a < 3; ++a) { u[a] = mp[a] - cd[a]; nu[a] = dn * u[a]; out[a] = nu[a]; }
    k = 3;
    for (int i = 0; i < 3; ++i)
        for (int j = i; j < 3; ++j, ++k) {
            const double p0 = W[i][0] * P.R[3 * j], p1 = W[i][1] * P.R[3 * j + 1], p2 = W[i][2] * P.R[3 * j + 2];
            const double Sp = (p0 + p1) + p2;
            const double q = nu[i] * u[j];
            out[k] = Sp + q;
        }
    return true;
}

}  // namespace gndt

#if defined(__HIPCC__)
#include "gndt_kernels.hpp"

namespace gndt {

// stats: {source nodes with a point, below min_count, skipped, merged nodes, merged points}
constexpr int kMergeStats = 5;

// One source node per thread-iteration, a sibling of k_coarsen: its key and 80-byte NodeAcc -> merge_node -> added into the
// destination's table (find_or_insert, wave-aggregated append to the node list, nine fp64 adds, the count, the minimum of the
// first-seen index).  Source nodes that meet in one destination node are not adjacent in the node list (first-seen order), so nothing
// is combined in front of the memory-side atomics: eleven of them per node bound the kernel, not its ~150 fp64 operations.
// Whole waves run the loop (append_new_nodes ballots): n is rounded up to 64.  The tallies are kept per lane and added up once per
// wave and counter behind the loop.  Workgroup 0 raises the destination's stream position, whether or not a node travels.
static __global__ void __launch_bounds__(kBlock) k_merge_map(const uint64_t* __restrict__ skeys, const NodeAcc* __restrict__ sacc,
                                                      const uint32_t* __restrict__ snode_slot, uint32_t scap_mask,
                                                      const Counters* __restrict__ scnt, MergeParams P, uint64_t* __restrict__ keys,
                                                      NodeAcc* __restrict__ acc, uint32_t cap_mask, uint32_t* __restrict__ node_slot,
                                                      uint32_t* __restrict__ index_of_slot, Counters* __restrict__ cnt,
                                                      unsigned long long* __restrict__ stats) {
    const uint32_t n = min(scnt->num_nodes, scap_mask + 1u);
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicMax(&cnt->stream_pos, P.new_pos);
    const uint64_t n_round = ((uint64_t)n + 63) & ~63ull;
    unsigned long long t_src = 0, t_below = 0, t_skip = 0, t_nodes = 0, t_points = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_round; i += (uint64_t)gridDim.x * blockDim.x) {
        bool live = false;
        uint64_t key = kEmptyKey;
        NodeAcc a;
        if (i < n) {
            const uint32_t ss = snode_slot[i];
            if (ss <= scap_mask) {
                key = skeys[ss];
                a = sacc[ss];
                live = key != kEmptyKey && a.count != 0u;
            }
        }
        uint64_t dkey = kEmptyKey;
        double q[9];
        if (live) {
            ++t_src;
            if (a.count < P.min_count) { ++t_below; live = false; }
            else if (!merge_node(key, a.count, a.s, P, dkey, q)) { ++t_skip; live = false; }
        }
        bool inserted = false;
        uint32_t slot = cap_mask + 1;
        if (live) {
            slot = find_or_insert(keys, cap_mask, dkey, inserted);
            if (slot > cap_mask) { atomicAdd(&cnt->err_table_full, 1u); inserted = false; }
        }
        append_new_nodes(inserted, slot, node_slot, index_of_slot, cnt);
        if (live && slot <= cap_mask) {
            NodeAcc* d = acc + slot;
#pragma unroll
            for (int k = 0; k < 9; ++k) unsafeAtomicAdd(&d->s[k], q[k]);
            atomicAdd(&d->count, a.count);
            if (a.first != 0xFFFFFFFFu) atomicMin(&d->first, P.base + a.first);      // (statistics merged in without an index keep none)
            ++t_nodes;
            t_points += a.count;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        t_src += __shfl_down(t_src, off, 64);
        t_below += __shfl_down(t_below, off, 64);
        t_skip += __shfl_down(t_skip, off, 64);
        t_nodes += __shfl_down(t_nodes, off, 64);
        t_points += __shfl_down(t_points, off, 64);
    }
    if (__lane_id() == 0) {
        if (t_src) atomicAdd(&stats[0], t_src);
        if (t_below) atomicAdd(&stats[1], t_below);
        if (t_skip) atomicAdd(&stats[2], t_skip);
        if (t_nodes) atomicAdd(&stats[3], t_nodes);
        if (t_points) atomicAdd(&stats[4], t_points);
    }
}

}  // namespace gndt
#endif
