// gndt_crop.hpp — region crop (gndt_crop*, include/gndt.h): every node of the columns a box of signed column indices drops leaves the map.
//
// Whole columns leave, and the slope labels only look at nodes of their own column (isSlope, map2D.h:66-108), so every surviving row is
// the row it was: the crop is a pure, order-preserving compaction of the result rows, with no arithmetic.
//   k_crop_count    rows -> kept rows per tile of kCropTile rows                              reads 8 B/row (sx, sy)
//   k_crop_scan     tile counts -> tile offsets, kept total (one workgroup)                    ~4 B per tile
//   k_crop_scatter  rows -> kept rows in the second set of result arrays, column / slope counts reads 80 B/row, writes 80 B/kept row
// The keep decision is a function of the row's own (sx, sy), so it needs no look-up of the column's first row.
// A map held in the node table also leaves the table (k_crop_table): the node list is exported with the dropped nodes' counts zeroed,
// the listed slots and column entries are cleared in place, and k_stats_merge (gndt_kernels.hpp) puts the survivors back.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gndt_kernels.hpp"

namespace gndt {

constexpr int kCropT = 256;                           // threads per workgroup of the row kernels
constexpr int kCropV = 4;                             // consecutive rows per thread: one 16-byte load per 4-byte array
constexpr uint32_t kCropTile = kCropT * kCropV;       // rows per workgroup
constexpr int kCropScanT = 1024;                      // k_crop_scan: one workgroup

struct CropBox {
    int sx_min, sx_max, sy_min, sy_max;
    int keep_inside;                                  // 1: GNDT_CROP_KEEP_INSIDE, 0: GNDT_CROP_DROP_INSIDE
};

GNDT_HD bool crop_keeps(const CropBox& b, int sx, int sy) {
    const bool in = sx >= b.sx_min && sx <= b.sx_max && sy >= b.sy_min && sy <= b.sy_max;
    return in == (b.keep_inside != 0);
}

// Exclusive prefix of `v` over the workgroup (NT threads, wave64); *total = the sum.  Every thread must call it.
template <int NT>
__device__ __forceinline__ uint32_t crop_block_scan(uint32_t v, uint32_t* total) {
    static_assert(NT % 64 == 0 && NT / 64 <= 64, "wave64 workgroup");
    __shared__ uint32_t s_wave[NT / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)inc, off, 64);
        if (lane >= off) inc += o;
    }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) {
        const uint32_t t = s_wave[w];
        before += w < wave ? t : 0u;
        all += t;
    }
    __syncthreads();                                  // (s_wave is written again by the next call)
    *total = all;
    return before + inc - v;
}

// Keep bits of the kCropV rows of this thread from row r0 on (16-byte loads when all of them exist; no bit for a row past n)
__device__ __forceinline__ uint32_t crop_keep_mask(const int32_t* __restrict__ sx, const int32_t* __restrict__ sy, uint32_t r0, uint32_t n,
                                                   const CropBox& B) {
    int4 x, y;
    if (r0 + kCropV <= n) {
        x = *reinterpret_cast<const int4*>(sx + r0);
        y = *reinterpret_cast<const int4*>(sy + r0);
    } else {
        int tx[kCropV] = {0, 0, 0, 0}, ty[kCropV] = {0, 0, 0, 0};
        for (int j = 0; j < kCropV; ++j)
            if (r0 + j < n) { tx[j] = sx[r0 + j]; ty[j] = sy[r0 + j]; }
        x = make_int4(tx[0], tx[1], tx[2], tx[3]);
        y = make_int4(ty[0], ty[1], ty[2], ty[3]);
    }
    uint32_t m = 0;
    m |= (r0 + 0 < n && crop_keeps(B, x.x, y.x)) ? 1u : 0u;
    m |= (r0 + 1 < n && crop_keeps(B, x.y, y.y)) ? 2u : 0u;
    m |= (r0 + 2 < n && crop_keeps(B, x.z, y.z)) ? 4u : 0u;
    m |= (r0 + 3 < n && crop_keeps(B, x.w, y.w)) ? 8u : 0u;
    return m;
}

static __global__ void __launch_bounds__(kCropT) k_crop_count(const int32_t* __restrict__ sx, const int32_t* __restrict__ sy, uint32_t n,
                                                              CropBox B, uint32_t* __restrict__ tile_cnt) {
    const uint32_t r0 = blockIdx.x * kCropTile + threadIdx.x * kCropV;
    const uint32_t k = (uint32_t)__popc(crop_keep_mask(sx, sy, r0, n, B));
    uint32_t total;
    (void)crop_block_scan<kCropT>(k, &total);
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = total;
}

// tile counts -> exclusive offsets (in place); the kept total becomes the map's node count; the column / slope tallies start at zero
static __global__ void __launch_bounds__(kCropScanT) k_crop_scan(uint32_t* __restrict__ tile_cnt, uint32_t tiles, Counters* __restrict__ cnt) {
    uint32_t carry = 0;
    for (uint32_t base = 0; base < tiles; base += kCropScanT) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < tiles ? tile_cnt[i] : 0u;
        uint32_t total;
        const uint32_t ex = crop_block_scan<kCropScanT>(v, &total);
        if (i < tiles) tile_cnt[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) { cnt->num_nodes = carry; cnt->num_columns = 0u; cnt->num_slopes = 0u; cnt->ticket = 0u; }
}

// The kept rows of tile blockIdx.x -> dst from tile_off[tile] on, in order.  Loads are 16 bytes wide (4 rows of a 4-byte array, 4 rows of
// mean / normal in three, of cov in six); stores go row by row (a kept row's place has no alignment).  The last workgroup to finish
// copies the counters into the host's pinned mirror (gndt_sync reads the counts from there: no copy command behind the crop).
static __global__ void __launch_bounds__(kCropT) k_crop_scatter(OutView src, const uint32_t* __restrict__ ncol_src, OutView dst,
                                                                uint32_t* __restrict__ ncol_dst, uint32_t n, CropBox B,
                                                                const uint32_t* __restrict__ tile_off, Counters* __restrict__ cnt,
                                                                Counters* __restrict__ host_cnt) {
    const uint32_t r0 = blockIdx.x * kCropTile + threadIdx.x * kCropV;
    const uint32_t m = crop_keep_mask(src.sx, src.sy, r0, n, B);
    uint32_t total;
    const uint32_t ex = crop_block_scan<kCropT>((uint32_t)__popc(m), &total);
    uint32_t d = tile_off[blockIdx.x] + ex;
    uint32_t cols = 0, slopes = 0;
    if (m) {
        int32_t vsx[kCropV], vsy[kCropV], vsz[kCropV];
        uint32_t vcount[kCropV], vfirst[kCropV], vflags[kCropV], vncol[kCropV];
        float vrough[kCropV], vmean[3 * kCropV], vnormal[3 * kCropV], vcov[6 * kCropV];
        if (r0 + kCropV <= n) {
            const auto ld4 = [](const void* p, uint32_t* o) {
                const uint4 v = *reinterpret_cast<const uint4*>(p);
                o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
            };
            ld4(src.sx + r0, (uint32_t*)vsx); ld4(src.sy + r0, (uint32_t*)vsy); ld4(src.sz + r0, (uint32_t*)vsz);
            ld4(src.count + r0, vcount); ld4(src.first_idx + r0, vfirst); ld4(src.flags + r0, vflags); ld4(ncol_src + r0, vncol);
            ld4(src.rough + r0, (uint32_t*)vrough);
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                ld4(src.mean + 3 * (uint64_t)r0 + 4 * q, (uint32_t*)vmean + 4 * q);
                ld4(src.normal + 3 * (uint64_t)r0 + 4 * q, (uint32_t*)vnormal + 4 * q);
            }
#pragma unroll
            for (int q = 0; q < 6; ++q) ld4(src.cov + 6 * (uint64_t)r0 + 4 * q, (uint32_t*)vcov + 4 * q);
        } else {
            for (int j = 0; j < kCropV; ++j) {
                if (!(m & (1u << j))) continue;      // (m has no bit for a row past n)
                const uint64_t r = r0 + j;
                vsx[j] = src.sx[r]; vsy[j] = src.sy[r]; vsz[j] = src.sz[r];
                vcount[j] = src.count[r]; vfirst[j] = src.first_idx[r]; vflags[j] = src.flags[r]; vncol[j] = ncol_src[r];
                vrough[j] = src.rough[r];
                for (int k = 0; k < 3; ++k) { vmean[3 * j + k] = src.mean[3 * r + k]; vnormal[3 * j + k] = src.normal[3 * r + k]; }
                for (int k = 0; k < 6; ++k) vcov[6 * j + k] = src.cov[6 * r + k];
            }
        }
#pragma unroll
        for (int j = 0; j < kCropV; ++j) {
            if (!(m & (1u << j))) continue;
            const uint64_t o = d++;
            dst.sx[o] = vsx[j]; dst.sy[o] = vsy[j]; dst.sz[o] = vsz[j];
            dst.count[o] = vcount[j]; dst.first_idx[o] = vfirst[j]; dst.flags[o] = vflags[j]; ncol_dst[o] = vncol[j];
            dst.rough[o] = vrough[j];
#pragma unroll
            for (int k = 0; k < 3; ++k) { dst.mean[3 * o + k] = vmean[3 * j + k]; dst.normal[3 * o + k] = vnormal[3 * j + k]; }
#pragma unroll
            for (int k = 0; k < 3; ++k)                // (cov rows are 24 bytes: 8-byte aligned)
                reinterpret_cast<float2*>(dst.cov + 6 * o)[k] = make_float2(vcov[6 * j + 2 * k], vcov[6 * j + 2 * k + 1]);
            cols += vncol[j] != 0u ? 1u : 0u;          // (non-zero exactly on a column's first row)
            slopes += (vflags[j] & GNDT_FLAG_SLOPE) ? 1u : 0u;
        }
    }
    uint32_t tc, ts;
    (void)crop_block_scan<kCropT>(cols, &tc);
    (void)crop_block_scan<kCropT>(slopes, &ts);
    if (threadIdx.x == 0) {
        if (tc) atomicAdd(&cnt->num_columns, tc);
        if (ts) atomicAdd(&cnt->num_slopes, ts);
        __threadfence();
        if (atomicAdd(&cnt->ticket, 1u) == gridDim.x - 1u) {     // the last workgroup: every tally is in
            __threadfence();
            cnt->ticket = 0u;
            Counters c = *cnt;
            c.num_columns = atomicAdd(&cnt->num_columns, 0u);
            c.num_slopes = atomicAdd(&cnt->num_slopes, 0u);
            if (host_cnt) *host_cnt = c;
        }
    }
}

// A map held in the node table: the node list [0, num_nodes) -> compact statistics (st_*), the count of a node the box drops written as 0 so that
// k_stats_merge skips it; every listed slot and, for the first np nodes (those that went through a finalisation), its column entry are
// cleared on the way — the table is then empty and the merge puts the survivors back in place (no reallocation, table_gen unchanged).
// Each node is read and cleared by its own thread; nodes of one column clear the same column entry with the same values.
static __global__ void __launch_bounds__(kBlock) k_crop_table(const uint32_t* __restrict__ node_slot, const uint32_t* __restrict__ col_slot_of_node,
                                                              uint64_t* __restrict__ keys, NodeAcc* __restrict__ acc, uint64_t* __restrict__ col_keys,
                                                              uint32_t* __restrict__ col_first, uint32_t* __restrict__ col_cnt,
                                                              uint32_t* __restrict__ col_head, uint32_t cap, uint32_t n_host, CropBox B,
                                                              const Counters* __restrict__ cnt, uint64_t* __restrict__ okey,
                                                              double* __restrict__ osums, uint32_t* __restrict__ ocount, uint32_t* __restrict__ ofirst) {
    const uint32_t n = min(n_host, cnt->num_nodes), np = cnt->prev_nodes;     // (entries [n, n_host) of the export: count 0, skipped)
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_host; i += gridDim.x * blockDim.x) {
        const uint32_t slot = i < n ? node_slot[i] : 0xFFFFFFFFu;
        if (slot >= cap) { okey[i] = kEmptyKey; ocount[i] = 0u; ofirst[i] = 0xFFFFFFFFu; continue; }
        const uint64_t key = keys[slot];
        const NodeAcc a = acc[slot];
        int sx, sy, sz;
        unpack_key(key, sx, sy, sz);
        const bool keep = key != kEmptyKey && crop_keeps(B, sx, sy);
        okey[i] = key;
#pragma unroll
        for (int k = 0; k < 9; ++k) osums[9 * (uint64_t)i + k] = keep ? a.s[k] : 0.0;
        ocount[i] = keep ? a.count : 0u;
        ofirst[i] = a.first;
        keys[slot] = kEmptyKey;
        NodeAcc z;
#pragma unroll
        for (int k = 0; k < 9; ++k) z.s[k] = 0.0;
        z.count = 0u; z.first = 0xFFFFFFFFu;
        acc[slot] = z;
        if (i < np) {
            const uint32_t cs = col_slot_of_node[i];
            if (cs < cap) { col_keys[cs] = kEmptyKey; col_first[cs] = 0xFFFFFFFFu; col_cnt[cs] = 0u; col_head[cs] = 0xFFFFFFFFu; }
        }
    }
}

// the table is empty: its node list restarts (the stream position and everything else stay)
static __global__ void k_crop_table_restart(Counters* cnt) {
    if (threadIdx.x == 0 && blockIdx.x == 0) { cnt->num_nodes = 0u; cnt->prev_nodes = 0u; }
}

}  // namespace gndt
