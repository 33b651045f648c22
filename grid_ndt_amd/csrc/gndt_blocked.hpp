// gndt_blocked.hpp — k_bucket_blocked: the bucket kernel for clouds whose occupied key range is a dense, evenly filled box.
//
// The hashed bucket kernel (gndt_bucket3.hpp) spends 25 of its 115 us of accumulate time on the bench scene FINDING a record's node
// (index window, fingerprint, key confirm) and 38 us grouping the nodes into columns afterwards (hash table of columns, per-column
// arrays: ~25 dependent LDS round trips per bucket) — profiles/r06_ablation.txt 1.  Both are the price of buckets that hold an
// arbitrary set of columns.  If a bucket is instead a spatial BLOCK of 2^shx x 2^shy columns x 2^shz levels = 512 nodes
// (GridParams::blk), a node's slot is a function of its key,
//        slot = (cz - z0) << (shx + shy) | (cy - y0 & mask_y) << shx | (cx - x0 & mask_x),
// the accumulate phase is a counting sort by slot with no search (see BlockedLds), and a node's column is the 2^shz slots that differ in the level bits: the
// column phases are eight independent LDS reads.  What it needs: every column of a block in ONE bucket and blocks of similar fill —
// i.e. a box of bounded height, evenly filled (the bench scene; a levelled site; not a LiDAR sweep, whose hottest hashed bucket is
// already 20 x the mean).  The host takes this kernel when the map of the previous build on the handle says so (partition_launch); a
// record that does not belong to its bucket's block (the cloud outgrew the box) raises PartCounters::blk_miss and the build is
// re-run with hashed buckets — the kernel is an optimisation of the same map, never another answer.
// Same outputs as k_bucket_direct: RawNode staging rows (a column's rows adjacent, first-seen order), ord_cf / ord_idx (or the column table in their place), the columns'
// votes in the bitmap / word weights, node / column / slope counts.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gndt_bucket3.hpp"
#include "gndt_stream.hpp"

namespace gndt {

// The accumulate phase sorts a bucket's records by slot, kBlkChunk records at a time, and thread s adds slot s's run into registers:
// per record ONE returning LDS atomic (its rank inside its slot), one 16-byte LDS write and one 16-byte LDS read.  It replaced eleven
// LDS atomics per record (count, nine fp64 sums, first-seen) whose issue and bank-conflict queue made two thirds of the kernel
// (profiles/r07_ablation.txt).  A contribution is computed by the same fp64 expressions as before; only the order in which a node's
// contributions are summed differs (it was the atomics' arrival order, and now is the order of the records in the image).
constexpr uint32_t kBlkChunk = 2048;                     // records per chunk: 32 KB of image
constexpr int kBlkPer = (int)kBlkChunk / 512;             // records per thread and chunk
constexpr uint32_t kBlkNone = 0xFFFFFFFFu;                // (slot_rank of a record that is not added)
struct BlockedLds {            // 43 KB: three workgroups per CU
    float4 image[kBlkChunk];   // a chunk's raw records, sorted by slot
    uint32_t hist[2][512];     // per chunk parity: a slot's records in the chunk (its ranks), then the slot's first entry inside its wave's part
    uint32_t wpre[2][8];       // per chunk parity: records of the chunk in the waves before wave w
    uint2 fz[512];             // {first-seen index (0xFFFFFFFF: no node in this slot), fp32 mean z of a node that has statistics, else 0}: what a
                               //   node's look at its column reads of the others, one 8-byte load per level
    uint32_t cpre[512];        // per COLUMN (the first 2^(shx+shy) entries): first row of the column inside the bucket
    uint32_t wave_tot[8];
    uint32_t n_nodes, n_cols, n_slopes, stage_base, err_range, miss;
};

// Inclusive add scan over the 64 lanes of a wave without the LDS: four shifts inside each row of 16 lanes (zero fill), then lane 15
// of rows 0 and 2 into rows 1 and 3, then lane 31 into rows 2 and 3.  Six DPP adds, no wait — against six ds_bpermute_b32 round
// trips with their address arithmetic for a __shfl_up scan.  FULL wave only: every lane must be active at the call (a lane that is not reads as zero and the sums behind it are wrong).  total = lane 63's value.
__device__ __forceinline__ uint32_t full_wave_scan_add(uint32_t x, uint32_t& total) {
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xF, 0xF, true);       // row_shr:1
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xF, 0xF, true);       // row_shr:2
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xF, 0xF, true);       // row_shr:4
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xF, 0xF, true);       // row_shr:8
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xA, 0xF, false);      // row_bcast:15, rows 1 and 3
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xC, 0xF, false);      // row_bcast:31, rows 2 and 3
    total = (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
    return x;
}

// One workgroup per bucket (the hardware's dynamic scheduling), three resident per CU.  The staging rows of a bucket are reserved with one
// memory-side atomic whose answer takes ~3 us; to have it in time the bucket's node count is known the moment the accumulate phase
// ends — every slot's count is in its thread's registers then: a ballot per wave — and the answer travels while the columns are
// worked out.  (Built and measured on the way, profiles/r06_ablation.txt 8: the count
// after the accumulate phase: ~5 k of 58 k cycles per bucket waiting; the rows of a bucket written behind the NEXT bucket's
// accumulate phase from registers: slower — the held row spills, and every vector-memory wait that follows stores waits for them.)
//
// col_tab (nullable): the COLUMN TABLE, one 16-byte record {first-seen index, first staging row, nodes, 0} per column `col` of bucket
// b at (b << (shx + shy)) + col, for the ordering pass that runs over columns (gndt_partition.hpp k_order_dest_table).  A block's
// columns are known by position, so the table needs no reservation and no search.  With it the kernel writes neither ord_cf nor
// ord_idx (who reads those: partition_launch, gndt_api_build.hip).  The table is NOT cleared between builds, a re-used handle holds
// the last build's records: every bucket therefore writes ALL 2^(shx + shy) records of its block in every build — nodes = 0 for a
// column without nodes (margin blocks and lo == hi take the ordinary path and write zeros' worth of columns), and zero records on
// both early ways out (a record outside the block, the staging rows run out).  The grid stride covers every bucket, so the pass never
// meets a record of another build and needs no flag to tell; what it reads of a build that is re-run is as consistent as its rows.
// (Round 10 also sent the staging rows out through the dead record image, in whole lines: 1.7 us of the kernel, inside its run-to-run
//  spread — built, measured, taken out again: profiles/r10_ablation.txt 2.)
template <int T>
__global__ void __launch_bounds__(T) __attribute__((amdgpu_waves_per_eu(6, 6))) k_bucket_blocked(const float4* __restrict__ recs, BucketRanges ranges, uint32_t num_buckets, GridParams P,
                                                      RawNode* __restrict__ stage, uint32_t stage_cap,
                                                      uint32_t* __restrict__ ord_cf, uint32_t* __restrict__ ord_idx, ColumnOrder O,
                                                      Counters* __restrict__ cnt, PartCounters* __restrict__ pc,
                                                      unsigned long long* __restrict__ dbg, uint4* __restrict__ col_tab) {
    static_assert(T == 512, "one table slot per thread");
    __shared__ BlockedLds L;
    const int tid = threadIdx.x;
    const BlockMap K = P.blk;
    const int sh_xy = K.shx + K.shy;
    const uint32_t col_mask = (1u << sh_xy) - 1u, n_levels = 1u << K.shz;
    if (blockIdx.x == 0 && tid == 0) { const uint32_t e = pc->l1_err; if (e) atomicAdd(&cnt->err_key_range, e); }   // (FoldClear, gndt_partition.hpp)
    for (uint32_t bucket = blockIdx.x; bucket < num_buckets; bucket += gridDim.x) {
#define GNDT_STAMPB(k) do { if (dbg && tid == 0) dbg[(size_t)bucket * 16 + (k)] = __builtin_amdgcn_s_memtime(); } while (0)
        uint32_t lo, hi;
        bucket_range(ranges, bucket, lo, hi);
        GNDT_STAMPB(0);
        // this bucket's block: contiguous indices bx0 .. bx0 + 2^shx - 1 (x), by0 .. (y), z0 .. z0 + 2^shz - 1 (levels)
        const int bx0 = K.x0 + (int)((bucket / (uint32_t)K.ny) << K.shx), by0 = K.y0 + (int)((bucket % (uint32_t)K.ny) << K.shy);
        // (s: thread s owns slot s.  It and the grid's parameters are opaque to the compiler, so that what it derives from them — the
        //  slot's centre, the fp64 constants, a zero — is recomputed per bucket: hoisted out of the bucket loop, those values spilled)
        uint32_t s = (uint32_t)tid;
        asm volatile("" : "+v"(s));
        const uint32_t zero = s - (uint32_t)tid;
        float f_len = P.grid_len, f_zlen = P.z_len, f_ox = P.ox, f_oy = P.oy, f_oz = P.oz;
        asm volatile("" : "+s"(f_len), "+s"(f_zlen), "+s"(f_ox), "+s"(f_oy), "+s"(f_oz));
        const double hx = 0.5 * (double)f_len, hz = 0.5 * (double)f_zlen;
        const double ox = (double)f_ox, oy = (double)f_oy, oz = (double)f_oz;
        L.hist[0][s] = zero; L.hist[1][s] = zero;
        if (s < 16) L.wpre[s >> 3][s & 7] = zero;
        if (s == 0) { L.n_nodes = zero; L.n_cols = zero; L.n_slopes = zero; L.stage_base = zero; L.err_range = zero; L.miss = zero; }
        lds_barrier();
        GNDT_STAMPB(1);
        // ---- accumulate, a chunk of kBlkChunk records at a time: rank inside the slot (ONE returning LDS atomic per record), prefix over
        //      the slots, the raw records sorted into the image by slot, then thread s walks slot s's run and adds into registers ----
        const uint32_t col = s & col_mask, lz = s >> sh_xy;
        // signed indices of this slot's node, and its centre on each axis (axis_index_offset's fma: a record of this slot has c = |n|)
        const int cxi = bx0 + (int)(col & ((1u << K.shx) - 1u)), cyi = by0 + (int)(col >> K.shx), czi = K.z0 + (int)lz;
        const int nsx = cxi >= 0 ? cxi + 1 : cxi, nsy = cyi >= 0 ? cyi + 1 : cyi, nsz = czi >= 0 ? czi + 1 : czi;
        const double ctx = fma((double)(float)(nsx > 0 ? 2 * nsx - 1 : 2 * nsx + 1), hx, ox),
                     cty = fma((double)(float)(nsy > 0 ? 2 * nsy - 1 : 2 * nsy + 1), hx, oy),
                     ctz = fma((double)(float)(nsz > 0 ? 2 * nsz - 1 : 2 * nsz + 1), hz, oz);
        const uint32_t n_rec = hi - lo, n_chunks = (n_rec + kBlkChunk - 1u) / kBlkChunk;
        uint32_t my_n = 0, my_first = 0xFFFFFFFFu;
        double sums[9];
#pragma unroll
        for (int j = 0; j < 9; ++j) sums[j] = 0.0;
        float4 rec[kBlkPer];
#pragma unroll
        for (int j = 0; j < kBlkPer; ++j) rec[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (lo < hi) {
#pragma unroll
            for (int j = 0; j < kBlkPer; ++j) rec[j] = load_once(recs + min(lo + (uint32_t)(j * T + tid), hi - 1u));      // (gndt_stream.hpp: the staging rows stay cached, not the records)
        }
        for (uint32_t ch = 0; ch < n_chunks; ++ch) {
            const uint32_t par = ch & 1u, c0 = lo + ch * kBlkChunk;
            uint32_t slot_rank[kBlkPer];        // slot << 16 | rank inside the slot; kBlkNone: the record is not added
#pragma unroll
            for (int j = 0; j < kBlkPer; ++j) {
                bool use = c0 + (uint32_t)(j * T + tid) < hi;
                bool und = false;
                float fx = axis_ceil_try(rec[j].x, P.ox, P.inv_grid, und);
                float fy = axis_ceil_try(rec[j].y, P.oy, P.inv_grid, und);
                float fz = axis_ceil_try(rec[j].z, P.oz, P.inv_z, und);
                if (und) {                                 // (rare: within ~2 ulp of a cell border the reference's own divide decides)
                    fx = ceilf(fabsf(rec[j].x - P.ox) / P.grid_len);
                    fy = ceilf(fabsf(rec[j].y - P.oy) / P.grid_len);
                    fz = ceilf(fabsf(rec[j].z - P.oz) / P.z_len);
                }
                bool ok = true;
                int sx, sy, sz;
                double v0, v1, v2;
                axis_index_offset(rec[j].x, P.ox, fx, (float)kMaxXY, hx, ox, ok, sx, v0);
                axis_index_offset(rec[j].y, P.oy, fy, (float)kMaxXY, hx, oy, ok, sy, v1);
                axis_index_offset(rec[j].z, P.oz, fz, (float)kMaxZ, hz, oz, ok, sz, v2);
                (void)v0; (void)v1; (void)v2;               // (recomputed by the slot's thread from the slot's centre: the same fma)
                if (use && !ok) { atomicAdd(&L.err_range, 1u); use = false; }      // |nz| beyond the key range (x, y: the partition)
                const uint32_t lx = (uint32_t)(contiguous_index(sx) - bx0), ly = (uint32_t)(contiguous_index(sy) - by0),
                               lz2 = (uint32_t)(contiguous_index(sz) - K.z0);
                if (use && ((lx >> K.shx) | (ly >> K.shy) | (lz2 >> K.shz)) != 0u) { L.miss = 1u; use = false; }      // not this block's: the build is re-run hashed
                const uint32_t rs = (lz2 << sh_xy) | (ly << K.shx) | lx;
                slot_rank[j] = use ? (rs << 16) | atomicAdd(&L.hist[par][rs], 1u) : kBlkNone;
            }
            lds_barrier();
            {   // exclusive prefix of the slots' counts: by DPP adds inside a wave (full_wave_scan_add: all 512 threads are here), the wave totals added into the later waves' entries
                const uint32_t c = L.hist[par][s];
                const int lane = tid & 63, wv = tid >> 6;
                uint32_t wtot;
                const uint32_t incl = full_wave_scan_add(c, wtot);
                L.hist[par][s] = incl - c;
                if (lane > wv && lane < T / 64 && wtot) atomicAdd(&L.wpre[par][lane], wtot);
                // (the other parity's arrays were last read before the previous chunk's walk: cleared here for the next chunk)
                L.hist[par ^ 1u][s] = 0u;
                if (tid < T / 64) L.wpre[par ^ 1u][tid] = 0u;
                lds_barrier();
#pragma unroll
                for (int j = 0; j < kBlkPer; ++j) {
                    const uint32_t sr = slot_rank[j];
                    if (sr != kBlkNone) L.image[L.hist[par][sr >> 16] + L.wpre[par][sr >> 22] + (sr & 0xFFFFu)] = rec[j];
                }
                const uint32_t b0 = incl - c + L.wpre[par][wv];
                // the next chunk's records: in flight during the walk
                if (ch + 1u < n_chunks) {
#pragma unroll
                    for (int j = 0; j < kBlkPer; ++j) rec[j] = load_once(recs + min(c0 + kBlkChunk + (uint32_t)(j * T + tid), hi - 1u));
                }
                lds_barrier();
                // slot s's run: today's contributions (weighted records included), added in the image's order
#pragma unroll 1
                for (uint32_t i = b0; i < b0 + c; ++i) {
                    const float4 r = L.image[i];
                    const double v0 = (double)r.x - ctx, v1 = (double)r.y - cty, v2 = (double)r.z - ctz;
                    const uint32_t iw = __float_as_uint(r.w);
                    uint32_t cn = 1u, cf = iw;
                    double w0 = v0, w1 = v1, w2 = v2;
                    if (__any((iw & kWeight64Flag) != 0u)) {              // weighted records: 64 or 512 identical points in one
                        cn = record_weight(iw); cf = record_index(iw);
                        const double wf = (double)cn;
                        w0 = wf * v0; w1 = wf * v1; w2 = wf * v2;
                    }
                    my_n += cn; my_first = min(my_first, cf);
                    sums[0] += w0; sums[1] += w1; sums[2] += w2;
                    sums[3] += w0 * v0; sums[4] += w0 * v1; sums[5] += w0 * v2;
                    sums[6] += w1 * v1; sums[7] += w1 * v2; sums[8] += w2 * v2;
                }
            }
        }
        const bool live = my_n != 0u;
        {   // the bucket's node count: per wave, one ballot and one LDS atomic
            const uint32_t w = (uint32_t)__popcll(__ballot(live));
            if ((tid & 63) == 0 && w) atomicAdd(&L.n_nodes, w);
        }
        lds_barrier();
        GNDT_STAMPB(2);
        if (L.miss) {                                  // (uniform)
            if (tid == 0) atomicAdd(&pc->blk_miss, 1u);
            if (col_tab && s <= col_mask) col_tab[((size_t)bucket << sh_xy) + s] = make_uint4(zero, zero, zero, zero);      // (no columns: see col_tab above; `zero`: a constant vector would be hoisted out of the bucket loop and spill)
            lds_barrier();
            continue;
        }
        const uint32_t M = L.n_nodes;
        // the staging rows: asked for now, the answer is awaited in front of the rows (thread T - 1 keeps it in a register until then)
        uint32_t stage_base_reg = 0;
        if (tid == T - 1 && M) stage_base_reg = atomicAdd(&cnt->num_nodes, M);
        if (tid == 0 && L.err_range) atomicAdd(&cnt->err_key_range, L.err_range);
        // ---- the bucket's nodes: slot s in thread s; its statistics are in registers, {first-seen, mean z} go to LDS ----
        const float cz = (live && my_n >= (uint32_t)P.min_points) ? node_mean_z(my_n, sums[2], axis_centre(nsz, P.oz, P.z_len)) : 0.f;
        L.fz[s] = make_uint2(my_first, __float_as_uint(cz));
        lds_barrier();
        // ---- the column of every node: the slots that differ in the level bits — independent 8-byte reads, no search.  The thread of a
        //      column's level-0 slot walks the column whether that slot holds a node or not: its node count is what the prefix over the
        //      columns (first row of every column inside the bucket) is made of ----
        uint32_t icol = 0, ncol = 0, cfirst = 0xFFFFFFFFu;
        bool up = false, down = false;
        if (live || s <= col_mask) {
            for (uint32_t k0 = 0; k0 < n_levels; k0 += 4) {
                uint2 tt[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) tt[j] = L.fz[min(((k0 + (uint32_t)j) << sh_xy) | col, 511u)];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t k = k0 + (uint32_t)j, tf = tt[j].x;
                    if (k >= n_levels || tf == 0xFFFFFFFFu) continue;
                    ++ncol;
                    cfirst = min(cfirst, tf);
                    if (k == lz) continue;
                    icol += (tf < my_first) ? 1u : 0u;
                    // OcNode::isSlope (map2D.h:66-108): the node one level up / down counts with its centroid only if it was seen
                    // earlier AND has statistics (its mean z is 0 below min_points), else with 0.0f.  In contiguous level indices "one
                    // level up" is k == lz + 1 — level_above / level_below skip the index 0 that does not exist.
                    if (k == lz + 1u || k + 1u == lz) {
                        const float oz2 = (tf < my_first) ? __uint_as_float(tt[j].y) : 0.f;
                        const bool far = fabsf(oz2 - cz) > P.slope_interval;
                        if (k == lz + 1u) up = far; else down = far;
                    }
                }
            }
        }
        {   // exclusive prefix of the columns' node counts: by DPP adds inside a wave; a column of the second wave (blocks of 128
            // columns) adds the first wave's total when it reads its entry
            const uint32_t my_col_nodes = s <= col_mask ? ncol : 0u;
            uint32_t wtot;
            const uint32_t incl = full_wave_scan_add(my_col_nodes, wtot);
            if (s <= col_mask) L.cpre[s] = incl - my_col_nodes;
            if ((tid & 63) == 0) L.wave_tot[tid >> 6] = wtot;
            if (s <= col_mask && my_col_nodes) atomicAdd(&L.n_cols, 1u);
            if (tid == T - 1) L.stage_base = stage_base_reg;      // (the reservation's answer: waited for here, by one thread)
            lds_barrier();
        }
        GNDT_STAMPB(3);
        const uint32_t sbase = L.stage_base;
        if (sbase + M > stage_cap) {                   // uniform: the staging rows ran out, the build is re-run with more
            if (tid == 0 && M) atomicAdd(&pc->stage_overflow, M);
            if (col_tab && s <= col_mask) col_tab[((size_t)bucket << sh_xy) + s] = make_uint4(zero, zero, zero, zero);
            lds_barrier();
            continue;
        }
        uint32_t my_slopes = 0, cbase = 0;
        if (live || s <= col_mask) {                    // the column's first row inside the bucket
            cbase = L.cpre[col];
            for (uint32_t w = 0; w < (col >> 6); ++w) cbase += L.wave_tot[w];      // (columns 64 .. 127 of a 128-column block: behind the first wave's)
        }
        // the column's record, by the thread of its level-0 slot, live or not (ncol = 0: the block has no such column)
        if (col_tab && s <= col_mask) col_tab[((size_t)bucket << sh_xy) + s] = make_uint4(cfirst, sbase + cbase, ncol, 0u);
        if (live) {
            uint32_t fl = (my_n >= (uint32_t)P.min_points) ? 1u : 0u;
            if (fl) {
                bool slope = true;
                if (P.demand == 0) slope = !up; else down = false;
                if (slope) { fl |= 2u; if (down) fl |= 4u; ++my_slopes; }
            }
            RawNode row;
            row.key = pack_key(nsx, nsy, nsz); row.count = my_n; row.first = my_first;
#pragma unroll
            for (int j = 0; j < 9; ++j) row.sum[j] = sums[j];
            row.info = fl | (icol << 3);
            row.ncol = ncol;
            const uint32_t dst = sbase + cbase + icol;
            stage[dst] = row;
            if (!col_tab) {                             // (the node-order passes' keys: gndt_partition.hpp)
                ord_cf[dst] = cfirst;
                ord_idx[dst] = icol ? icol : (kOrdHeadFlag | ncol);       // (a column's first row carries the column's size)
            }
            if (icol == 0) note_column(O, cfirst, ncol);
        }
        if (my_slopes) atomicAdd(&L.n_slopes, my_slopes);
        lds_barrier();
        if (tid == 0) {
            // (ONE atomic, on the partition counters' line — PartCounters::cols_slopes: not on the line the row reservations wait on)
            if (L.n_cols | L.n_slopes) atomicAdd(&pc->cols_slopes, ((unsigned long long)L.n_slopes << 32) | (unsigned long long)L.n_cols);
        }
        GNDT_STAMPB(4);
        lds_barrier();          // (the table is re-initialised by the next bucket)
#undef GNDT_STAMPB
    }
}

// The box a finished map occupies, in contiguous indices: min / max of cx, cy, cz over its rows and the largest node (what decides whether
// the next build of a cloud like it may take blocked buckets).  64 workgroups, one LDS reduction each, twelve memory-side atomics per
// workgroup; out[0..5] = min x, y, z (as biased uint32: + 2^30), max x, y, z, out[6] = largest count — initialised by the caller.
static __global__ void __launch_bounds__(1024) k_key_extent(const int32_t* __restrict__ sx, const int32_t* __restrict__ sy, const int32_t* __restrict__ sz,
                                                            const uint32_t* __restrict__ count, uint32_t n, uint32_t* __restrict__ out) {
    __shared__ uint32_t red[7];
    if (threadIdx.x < 3) red[threadIdx.x] = 0xFFFFFFFFu;
    else if (threadIdx.x < 7) red[threadIdx.x] = 0u;
    __syncthreads();
    uint32_t mn[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, mx[3] = {0u, 0u, 0u}, big = 0u;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t c[3] = {(uint32_t)(contiguous_index(sx[i]) + (1 << 30)), (uint32_t)(contiguous_index(sy[i]) + (1 << 30)),
                               (uint32_t)(contiguous_index(sz[i]) + (1 << 30))};
#pragma unroll
        for (int k = 0; k < 3; ++k) { mn[k] = min(mn[k], c[k]); mx[k] = max(mx[k], c[k]); }
        big = max(big, count[i]);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        for (int off = 32; off > 0; off >>= 1) {
            mn[k] = min(mn[k], (uint32_t)__shfl_down((int)mn[k], off, 64));
            mx[k] = max(mx[k], (uint32_t)__shfl_down((int)mx[k], off, 64));
        }
    }
    for (int off = 32; off > 0; off >>= 1) big = max(big, (uint32_t)__shfl_down((int)big, off, 64));
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { atomicMin(&red[k], mn[k]); atomicMax(&red[3 + k], mx[k]); }
        atomicMax(&red[6], big);
    }
    __syncthreads();
    if (threadIdx.x < 3) atomicMin(&out[threadIdx.x], red[threadIdx.x]);
    else if (threadIdx.x < 7) atomicMax(&out[threadIdx.x], red[threadIdx.x]);
}

}  // namespace gndt
