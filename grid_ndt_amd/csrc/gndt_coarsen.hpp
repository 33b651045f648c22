// gndt_coarsen.hpp — map pyramids (gndt_coarsen_device, include/gndt.h): the map a build of the same point stream at f times the cell
// lengths would give, from the fine map's node table alone.
//
// For a power-of-two factor f the coarse index of a point is a function of its fine index s (there is no index 0):
//     parent_index(s, f) = sign(s) * ceil(|s| / f)
// because fl32(|d| / (f L)) = fl32(|d| / L) / f (a division by a power of two is exact) and ceil(x / f) = ceil(ceil(x) / f) for x > 0.
// A node's additive statistics (count, Sum v, Sum v v^T about the node's centre c) move to the parent's centre c' with d = c - c':
//     Sum v'        = Sum v + n d
//     Sum v' v'^T_ab = Sum v v^T_ab + d_a Sum v_b + d_b Sum v_a + n d_a d_b
// and the parents' statistics are the sums over their children: counts add, first-seen indices take the minimum.
//   k_coarsen   source node list -> destination node table, one pass        reads 4 + 88 B per source node, at most 88 B per parent out
// The per-node arithmetic is GNDT_HD: tests/coarsen_shim.cpp compiles it for the host.
#pragma once
#include <stdint.h>

#include "gndt_math.hpp"

namespace gndt {

// the coarse index of fine index s (s != 0) for a factor f >= 1; powers of two are what the identity above holds for
GNDT_HD int parent_index(int s, int f) { return s > 0 ? (s + f - 1) / f : -((-s + f - 1) / f); }

GNDT_HD uint64_t parent_key(uint64_t key, int fxy, int fz) {
    int sx, sy, sz;
    unpack_key(key, sx, sy, sz);
    return pack_key(parent_index(sx, fxy), parent_index(sy, fxy), parent_index(sz, fz));
}

// delta[a] = centre of the child - centre of its parent along axis a, both by axis_centre in fp64 (fine and coarse lengths as the two
// handles hold them in fp32)
GNDT_HD void coarsen_delta(uint64_t key, int fxy, int fz, const float o[3], float grid_len, float z_len, float coarse_grid_len,
                           float coarse_z_len, double delta[3]) {
    int sx, sy, sz;
    unpack_key(key, sx, sy, sz);
    delta[0] = axis_centre(sx, o[0], grid_len) - axis_centre(parent_index(sx, fxy), o[0], coarse_grid_len);
    delta[1] = axis_centre(sy, o[1], grid_len) - axis_centre(parent_index(sy, fxy), o[1], coarse_grid_len);
    delta[2] = axis_centre(sz, o[2], z_len) - axis_centre(parent_index(sz, fz), o[2], coarse_z_len);
}

// The statistics of n points about c, moved to c' = c - delta.  Evaluation order (fp64, no FMA contraction; tests/coarsen_ref.py
// follows it bit for bit), with nd_a = (double)n * delta_a:
//     out[a]    = sums[a] + nd_a                                                               a = 0, 1, 2
//     out[3+ab] = ((sums[3+ab] + delta_a * sums[b]) + delta_b * sums[a]) + nd_a * delta_b      ab = xx, xy, xz, yy, yz, zz
GNDT_HD void coarsen_sums(uint32_t n, const double sums[9], const double delta[3], double out[9]) {
    const double nd[3] = {(double)n * delta[0], (double)n * delta[1], (double)n * delta[2]};
    for (int a = 0; a < 3; ++a) out[a] = sums[a] + nd[a];
    int k = 3;
    for (int a = 0; a < 3; ++a)
        for (int b = a; b < 3; ++b, ++k) {
            const double p1 = delta[a] * sums[b], p2 = delta[b] * sums[a], p3 = nd[a] * delta[b];
            out[k] = ((sums[k] + p1) + p2) + p3;
        }
}

}  // namespace gndt

#if defined(__HIPCC__)
#include "gndt_kernels.hpp"

namespace gndt {

struct CoarsenParams {
    float o[3];                               // the origin both maps share
    float grid_len, z_len;                    // the source's lengths
    float coarse_grid_len, coarse_z_len;      // the destination's: (float)(factor * length), exact for a power of two
    int fxy, fz;
};

// One source node per thread-iteration: its key and 80-byte NodeAcc -> parent key, statistics about the parent's centre -> added into
// the destination's table (what k_stats_merge does for unshifted statistics: find_or_insert, wave-aggregated append to the node list,
// nine fp64 adds, the count, the minimum of the first-seen index).  Up to fxy^2 * fz siblings meet in one parent; they are not adjacent
// in the node list (first-seen order), so nothing is combined in front of the memory-side atomics.  The destination's stream position
// becomes at least the source's (`src_pos`: the host's mirror of it, for a source whose device word lags).
// Whole waves run the loop (append_new_nodes ballots): n is rounded up to 64.
static __global__ void __launch_bounds__(kBlock) k_coarsen(const uint64_t* __restrict__ skeys, const NodeAcc* __restrict__ sacc,
                                                    const uint32_t* __restrict__ snode_slot, uint32_t scap_mask,
                                                    const Counters* __restrict__ scnt, CoarsenParams P, uint32_t src_pos,
                                                    uint64_t* __restrict__ keys, NodeAcc* __restrict__ acc, uint32_t cap_mask,
                                                    uint32_t* __restrict__ node_slot, uint32_t* __restrict__ index_of_slot,
                                                    Counters* __restrict__ cnt) {
    const uint32_t n = min(scnt->num_nodes, scap_mask + 1u);
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicMax(&cnt->stream_pos, max(scnt->stream_pos, src_pos));
    const uint64_t n_round = ((uint64_t)n + 63) & ~63ull;
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
        bool inserted = false;
        uint32_t slot = cap_mask + 1;
        if (live) {
            slot = find_or_insert(keys, cap_mask, parent_key(key, P.fxy, P.fz), inserted);
            if (slot > cap_mask) { atomicAdd(&cnt->err_table_full, 1u); inserted = false; }
        }
        append_new_nodes(inserted, slot, node_slot, index_of_slot, cnt);
        if (live && slot <= cap_mask) {
            double delta[3], q[9];
            coarsen_delta(key, P.fxy, P.fz, P.o, P.grid_len, P.z_len, P.coarse_grid_len, P.coarse_z_len, delta);
            coarsen_sums(a.count, a.s, delta, q);
            NodeAcc* d = acc + slot;
#pragma unroll
            for (int k = 0; k < 9; ++k) unsafeAtomicAdd(&d->s[k], q[k]);
            atomicAdd(&d->count, a.count);
            atomicMin(&d->first, a.first);
        }
    }
}

}  // namespace gndt
#endif
