// gndt_segment.hpp — scan segmentation (include/gndt.h "scan segmentation"): the points of a scan that the map does not explain,
// clustered into connected components of grid cells on the device.  The class of a point is scan scoring's (score_point, its least d2
// rounded to fp32); everything after it is integer or bit-pattern arithmetic, so the answer does not depend on the order threads work in.
//   k_seg_classify   points -> class; a novel point's cell into the call's cell table (first index, count)     two atomics a novel point
//   k_seg_cells      points -> parent[i] = i where i is the id of a novel cell, kNoRow elsewhere                  8 B a point + a slot
//   k_seg_link       cell ids -> lock-free union-find over parent (13 or 3 forward neighbours probed each)      cell ids only
//   k_seg_flatten    points -> their cluster's label; cell ids: parent = root, the roots count cells and points
//   k_seg_count      indices -> novel points, cells, roots and listed roots per tile of kCropTile indices         9 B an index
//   k_seg_scan       tile counts -> tile offsets of the listed roots, the call's four counts (one workgroup)
//   k_seg_rank       roots -> place in the list; the listed clusters' records initialised
//   k_seg_reduce     points of listed clusters -> the cluster's record, integer atomics only
//   k_seg_finish     records -> z_lo / z_hi back from their integer images
// The cell table is the call's own: open addressing over the packed key of the POINT's cell (the map's codec, but keyed by the scan),
// linear probing, an insert in the manner of tab_column_slot (gndt_table.hpp); a power of two >= 2 n slots, so n cells stay at or below
// half load whatever the scan.  A cell stands in the union-find at its id — the smallest index of its novel points — so a root is its
// cluster's smallest point index: the label.  frontier_find / frontier_unite (gndt_frontier.hpp) as they are: parent[x] <= x throughout.
// The per-element logic is host-callable (tests/segment_shim.cpp runs it one item after another); memory operations go through an Ops
// policy (SegSerialOps here, SegDeviceOps with the kernels).
#pragma once
#include <math.h>
#include <stdint.h>

#include "gndt_frontier.hpp"
#include "gndt_score.hpp"

namespace gndt {

constexpr uint32_t kSegUnkeyed = 0, kSegExplained = 1, kSegOffSurface = 2, kSegUnmapped = 3;      // GNDT_SEG_*
constexpr uint32_t kSegMinSlots = 1024;

struct SegRule {                    // gndt_segment_params with the defaults filled in (the score's parameters travel as ScoreParams)
    float novel_d2;
    uint32_t classes, min_points, connectivity, min_cluster_points, min_cluster_cells;
};

struct SegTable {                   // key: kEmptyKey = free; first: the least index of the cell's novel points; count: how many
    uint64_t* key;
    uint32_t* first;
    uint32_t* count;
    uint32_t mask;
};

struct SegRecord {                  // gndt_scan_cluster; z_lo / z_hi hold the floats' integer images until k_seg_finish
    uint32_t label, cells, off_surface, unmapped;
    int32_t sx_min, sx_max, sy_min, sy_max, sz_min, sz_max;
    long long sum_x, sum_y, sum_z;
    uint32_t z_lo, z_hi;
};
static_assert(sizeof(SegRecord) == 72, "gndt_scan_cluster is 72 bytes");

struct SegSum {                     // what one point, or several points of one cluster combined, add to the cluster's record
    long long x, y, z;
    int32_t sx_min, sx_max, sy_min, sy_max, sz_min, sz_max;
    uint32_t z_lo, z_hi, off_surface, unmapped;
};

// slots of the cell table for n points: the smallest power of two >= max(2 n, kSegMinSlots)
GNDT_HD uint64_t seg_table_slots(uint64_t n) {
    uint64_t s = kSegMinSlots;
    while (s < 2 * n) s <<= 1;
    return s;
}

// The order-preserving image of a float: a < b as floats (-0 below +0) exactly when image(a) < image(b) as unsigned integers
GNDT_HD uint32_t seg_z_image(float f) {
    const uint32_t u = float_bits(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
GNDT_HD uint32_t seg_z_bits(uint32_t image) { return (image & 0x80000000u) ? (image & 0x7FFFFFFFu) : ~image; }

// q of a point: scan scoring's transform, or the point itself without a pose
GNDT_HD void seg_transform(const double* pose, const float* p, float& qx, float& qy, float& qz) {
    if (pose) score_transform(pose, p[0], p[1], p[2], qx, qy, qz);
    else { qx = p[0]; qy = p[1]; qz = p[2]; }
}

// The class of q and its key.  score_point with max_d2 = 0 (P.max_d2) gives the nearest counting candidate; its d2 is compared as the
// fp32 number gndt_score_poses reports per point.
template <int NBH>
GNDT_HD uint32_t seg_class(const ScoreView& S, const ScoreParams& P, float novel_d2, float qx, float qy, float qz, QueryKey& k) {
    k = query_key<kQueryNode>(S.Q, qx, qy, qz);
    if (!k.ok) return kSegUnkeyed;
    ScoreAcc a;
    a.score = 0.0; a.d2_sum = 0.0; a.matched = 0u; a.terms = 0u;
    ScoreBest b;
    b.d2 = (double)INFINITY; b.row = kNoRow;
    score_point<NBH>(S, P, qx, qy, qz, a, b);
    if (b.row == kNoRow) return kSegUnmapped;
    return (float)b.d2 <= novel_d2 ? kSegExplained : kSegOffSurface;
}

GNDT_HD bool seg_is_novel(const SegRule& R, uint32_t cls) { return ((R.classes >> cls) & 1u) != 0u; }

// One thread after another (the CPU tier): the frontier's, and what the cell table and the z images need
struct SegSerialOps : FrontierSerialOps {
    static inline uint64_t cas_u64(uint64_t* p, uint64_t expect, uint64_t v) { const uint64_t old = *p; if (old == expect) *p = v; return old; }
    static inline void min_u32(uint32_t* p, uint32_t v) { if (v < *p) *p = v; }
    static inline void max_u32(uint32_t* p, uint32_t v) { if (v > *p) *p = v; }
};

// The slot of a cell's key, inserting it if new.  A key, once in a slot, stays: a plain load that sees another cell's key may walk on.
// kNoRow: no free slot on the whole walk (cannot happen at half load; the loop is bounded because the device is shared).
template <class Ops>
GNDT_HD uint32_t seg_insert(const SegTable& T, uint64_t key) {
    uint32_t s = (uint32_t)mix64(key) & T.mask;
    for (uint32_t probe = 0; probe <= T.mask; ++probe) {
        const uint64_t k = T.key[s];
        if (k == key) return s;
        if (k == kEmptyKey) {
            const uint64_t old = Ops::cas_u64(T.key + s, kEmptyKey, key);
            if (old == kEmptyKey || old == key) return s;
        }
        s = (s + 1) & T.mask;
    }
    return kNoRow;
}

// A novel point of index i joins its cell
template <class Ops>
GNDT_HD uint32_t seg_join(const SegTable& T, uint64_t key, uint32_t i) {
    const uint32_t s = seg_insert<Ops>(T, key);
    if (s == kNoRow) return kNoRow;
    Ops::min_u32(T.first + s, i);
    Ops::add_u32(T.count + s, 1u);
    return s;
}

// The slot of a cell's key in the finished table, kNoRow if no point fell into that cell
GNDT_HD uint32_t seg_find(const SegTable& T, uint64_t key) {
    uint32_t s = (uint32_t)mix64(key) & T.mask;
    for (uint32_t probe = 0; probe <= T.mask; ++probe) {
        const uint64_t k = T.key[s];
        if (k == key) return s;
        if (k == kEmptyKey) return kNoRow;
        s = (s + 1) & T.mask;
    }
    return kNoRow;
}

// The id of the cell in slot s (kNoRow: no slot, or fewer than min_points novel points)
GNDT_HD uint32_t seg_cell_id(const SegTable& T, const SegRule& R, uint32_t s) {
    if (s == kNoRow) return kNoRow;
    return T.count[s] >= R.min_points ? T.first[s] : kNoRow;
}

// parent[i] before the links: i where point i is the id of a novel cell
GNDT_HD uint32_t seg_parent_init(const SegTable& T, const SegRule& R, uint32_t i, uint32_t slot) {
    return seg_cell_id(T, R, slot) == i ? i : kNoRow;
}

// Cell id i (in slot `slot`) against the novel cells among its forward neighbours: the 13 of 26 (dx, dy, dz) that come after (0, 0, 0)
// in lexicographic order, under connectivity 6 the three unit steps; the others are the same pairs seen from the other cell.  Steps go
// over the hole at 0; an index beyond the codec's range does not exist.  The first probes are all issued before any is looked at.
// after_unite(a, b): the CPU tier's look at the invariant.
template <class Ops, class AfterUnite>
GNDT_HD void seg_link(const SegTable& T, const SegRule& R, uint32_t* parent, uint32_t i, uint32_t slot, uint32_t n, AfterUnite after_unite) {
    int sx, sy, sz;
    unpack_key(T.key[slot], sx, sy, sz);
    uint64_t nk[13], k0[13];
    uint32_t s0[13];
#pragma unroll
    for (int j = 0; j < 13; ++j) {
        const int c = 14 + j, dx = c / 9 - 1, dy = (c / 3) % 3 - 1, dz = c % 3 - 1;
        const int nx = dx ? step_skip0(sx, dx) : sx, ny = dy ? step_skip0(sy, dy) : sy, nz = dz ? step_skip0(sz, dz) : sz;
        const int steps = (dx ? 1 : 0) + (dy ? 1 : 0) + (dz ? 1 : 0);
        const bool exists = nx >= -kMaxXY && nx <= kMaxXY && ny >= -kMaxXY && ny <= kMaxXY && nz >= -kMaxZ && nz <= kMaxZ &&
                            (R.connectivity == 26u || steps == 1);
        nk[j] = exists ? pack_key(nx, ny, nz) : kEmptyKey;
        s0[j] = (uint32_t)mix64(nk[j]) & T.mask;
        k0[j] = exists ? T.key[s0[j]] : kEmptyKey;
    }
#pragma unroll
    for (int j = 0; j < 13; ++j) {
        if (nk[j] == kEmptyKey || k0[j] == kEmptyKey) continue;
        const uint32_t s = k0[j] == nk[j] ? s0[j] : seg_find(T, nk[j]);
        const uint32_t id = seg_cell_id(T, R, s);
        if (id == kNoRow) continue;
        frontier_unite<Ops>(parent, i, id, n);
        after_unite(i, id);
    }
}

// What a point of class cls at q with key k adds to its cluster
GNDT_HD SegSum seg_term(const QueryKey& k, float qx, float qy, float qz, uint32_t cls) {
    SegSum s;
    s.x = llrint((double)qx * 1024.0); s.y = llrint((double)qy * 1024.0); s.z = llrint((double)qz * 1024.0);
    s.sx_min = s.sx_max = k.sx; s.sy_min = s.sy_max = k.sy; s.sz_min = s.sz_max = k.sz;
    s.z_lo = s.z_hi = seg_z_image(qz);
    s.off_surface = cls == kSegOffSurface ? 1u : 0u;
    s.unmapped = cls == kSegUnmapped ? 1u : 0u;
    return s;
}

// The identities of the reduction
GNDT_HD SegSum seg_sum_none() {
    SegSum s;
    s.x = s.y = s.z = 0;
    s.sx_min = s.sy_min = s.sz_min = 0x7FFFFFFF; s.sx_max = s.sy_max = s.sz_max = -0x7FFFFFFF - 1;
    s.z_lo = 0xFFFFFFFFu; s.z_hi = 0u; s.off_surface = s.unmapped = 0u;
    return s;
}

// Two sums of one cluster as one
GNDT_HD SegSum seg_sum_add(const SegSum& a, const SegSum& b) {
    SegSum s;
    s.x = a.x + b.x; s.y = a.y + b.y; s.z = a.z + b.z;
    s.sx_min = a.sx_min < b.sx_min ? a.sx_min : b.sx_min; s.sx_max = a.sx_max > b.sx_max ? a.sx_max : b.sx_max;
    s.sy_min = a.sy_min < b.sy_min ? a.sy_min : b.sy_min; s.sy_max = a.sy_max > b.sy_max ? a.sy_max : b.sy_max;
    s.sz_min = a.sz_min < b.sz_min ? a.sz_min : b.sz_min; s.sz_max = a.sz_max > b.sz_max ? a.sz_max : b.sz_max;
    s.z_lo = a.z_lo < b.z_lo ? a.z_lo : b.z_lo; s.z_hi = a.z_hi > b.z_hi ? a.z_hi : b.z_hi;
    s.off_surface = a.off_surface + b.off_surface; s.unmapped = a.unmapped + b.unmapped;
    return s;
}

// The record of a cluster before its first point: label and cells are known when the list is made
GNDT_HD SegRecord seg_record_init(uint32_t label, uint32_t cells) {
    SegRecord r;
    r.label = label; r.cells = cells; r.off_surface = r.unmapped = 0u;
    r.sx_min = r.sy_min = r.sz_min = 0x7FFFFFFF; r.sx_max = r.sy_max = r.sz_max = -0x7FFFFFFF - 1;
    r.sum_x = r.sum_y = r.sum_z = 0;
    r.z_lo = 0xFFFFFFFFu; r.z_hi = 0u;
    return r;
}

// Integer sums, minima and maxima only: any order gives the same record
template <class Ops>
GNDT_HD void seg_fold(SegRecord* r, const SegSum& s) {
    if (s.off_surface) Ops::add_u32(&r->off_surface, s.off_surface);
    if (s.unmapped) Ops::add_u32(&r->unmapped, s.unmapped);
    Ops::add_i64(&r->sum_x, s.x); Ops::add_i64(&r->sum_y, s.y); Ops::add_i64(&r->sum_z, s.z);
    Ops::min_i32(&r->sx_min, s.sx_min); Ops::max_i32(&r->sx_max, s.sx_max);
    Ops::min_i32(&r->sy_min, s.sy_min); Ops::max_i32(&r->sy_max, s.sy_max);
    Ops::min_i32(&r->sz_min, s.sz_min); Ops::max_i32(&r->sz_max, s.sz_max);
    Ops::min_u32(&r->z_lo, s.z_lo); Ops::max_u32(&r->z_hi, s.z_hi);
}

// z_lo / z_hi of a finished record: the floats' bits back from their images
GNDT_HD void seg_record_finish(SegRecord* r) { r->z_lo = seg_z_bits(r->z_lo); r->z_hi = seg_z_bits(r->z_hi); }

// A call's scratch for n points, a cell table of `slots` slots (seg_table_slots) and `tiles` tiles of the ordered compaction
// (gndt_api_segment.hip).  Two pairs are cleared by one memset each, so each is ONE piece and its second array starts where the first
// ends: the table's key | first (12 B a slot, all ones) and cells_at | points_at (8 B a point, zero).
struct SegmentScratch {
    SegTable T;                      // key [slots] | first [slots], count [slots]
    uint32_t* slot_root;             // [n] a point's slot, then its root
    uint32_t* parent;                // [n] the union-find
    uint32_t *cells_at, *points_at;  // [n] | [n] a root's cells and points, then its place
    uint32_t* tile_cnt;              // [4 tiles]
    uint8_t* cls_of;                 // [n] the class
    uint8_t* slack;                  // [16]
    SegmentScratch() = default;
    SegmentScratch(Carver& c, uint64_t n, uint64_t slots, uint64_t tiles) {
        T.key = c.take<uint64_t>(slots + slots / 2);             // 12 B a slot; slots is a power of two (seg_table_slots)
        T.first = T.key ? reinterpret_cast<uint32_t*>(T.key + slots) : nullptr;
        T.count = c.take<uint32_t>(slots);
        T.mask = (uint32_t)(slots - 1);
        slot_root = c.take<uint32_t>(n);  parent = c.take<uint32_t>(n);
        cells_at = c.take<uint32_t>(2 * n);
        points_at = cells_at ? cells_at + n : nullptr;
        tile_cnt = c.take<uint32_t>(4 * tiles);  cls_of = c.take<uint8_t>(n);  slack = c.take<uint8_t>(16);
    }
};

}  // namespace gndt

#if defined(__HIPCC__)
#include "gndt_crop.hpp"      // crop_block_scan, kCropT / kCropV / kCropTile: the ordered compaction of the crop

namespace gndt {

struct SegDeviceOps : FrontierDeviceOps {
    static __device__ __forceinline__ uint64_t cas_u64(uint64_t* p, uint64_t expect, uint64_t v) {
        return (uint64_t)atomicCAS(reinterpret_cast<unsigned long long*>(p), (unsigned long long)expect, (unsigned long long)v);
    }
    static __device__ __forceinline__ void min_u32(uint32_t* p, uint32_t v) { atomicMin(p, v); }
    static __device__ __forceinline__ void max_u32(uint32_t* p, uint32_t v) { atomicMax(p, v); }
};

// Every point: its class, and a novel point into its cell.  slot_of[i] = the cell's slot (kNoRow: not novel), cls_of[i] the class.
// Every novel point issues its own two atomics on its cell: letting the first lane of a run of equal keys in a wave issue them for the
// run measured no faster on a scan in sensor order and no slower on a shuffled one, so it is not here.
template <int NBH>
static __global__ void __launch_bounds__(256) k_seg_classify(ScoreView S, ScoreParams P, SegRule R, const float* __restrict__ xyz, uint32_t sf,
                                                             uint32_t n, const double* __restrict__ pose, SegTable T,
                                                             uint32_t* __restrict__ slot_of, uint8_t* __restrict__ cls_of,
                                                             uint8_t* __restrict__ point_class) {
    const uint32_t gsz = gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gsz) {
        float qx, qy, qz;
        seg_transform(pose, xyz + i * sf, qx, qy, qz);
        QueryKey k;
        const uint32_t cls = seg_class<NBH>(S, P, R.novel_d2, qx, qy, qz, k);
        slot_of[i] = seg_is_novel(R, cls) ? seg_join<SegDeviceOps>(T, pack_key(k.sx, k.sy, k.sz), (uint32_t)i) : kNoRow;
        cls_of[i] = (uint8_t)cls;
        if (point_class) point_class[i] = (uint8_t)cls;
    }
}

static __global__ void __launch_bounds__(256) k_seg_cells(SegTable T, SegRule R, uint32_t n, const uint32_t* __restrict__ slot_of,
                                                          uint32_t* __restrict__ parent) {
    const uint32_t gsz = gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gsz) parent[i] = seg_parent_init(T, R, (uint32_t)i, slot_of[i]);
}

static __global__ void __launch_bounds__(256) k_seg_link(SegTable T, SegRule R, uint32_t n, const uint32_t* __restrict__ slot_of,
                                                         uint32_t* __restrict__ parent) {
    const uint32_t gsz = gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gsz) {
        if (SegDeviceOps::load(parent + i) == kNoRow) continue;
        seg_link<SegDeviceOps>(T, R, parent, (uint32_t)i, slot_of[i], n, FrontierNoLook{});
    }
}

// Every point: root_of[i] = the root of its cell's id (kNoRow: not novel, or a cell below min_points), which is its label; a cell id
// also stores the root as its parent (its own thread's store only: frontier_root) and adds its cell and its points to the root's
// tallies — cell ids of one wave that share a root add up among themselves first.  slot_of and root_of are one array: a thread reads
// its own slot before it stores its root.
static __global__ void __launch_bounds__(256) k_seg_flatten(SegTable T, SegRule R, uint32_t n, uint32_t* __restrict__ parent,
                                                            uint32_t* __restrict__ slot_root, uint32_t* __restrict__ cells_at,
                                                            uint32_t* __restrict__ points_at, uint32_t* __restrict__ point_label) {
    const uint32_t gsz = gridDim.x * blockDim.x;
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t r0 = (uint64_t)blockIdx.x * blockDim.x; r0 < n; r0 += gsz) {      // (uniform over the workgroup: the ballots below)
        const uint64_t i = r0 + threadIdx.x;
        uint32_t root = kNoRow, mine = 0u;             // mine: this thread is a cell id with that many points
        if (i < n) {
            const uint32_t slot = slot_root[i];
            const uint32_t id = seg_cell_id(T, R, slot);
            if (id != kNoRow) {
                root = frontier_root<SegDeviceOps>(parent, id, n);
                if (id == (uint32_t)i) {
                    mine = T.count[slot];
                    if (root != id) SegDeviceOps::store(parent + i, root);
                }
            }
            slot_root[i] = root;
            if (point_label) point_label[i] = root;
        }
        unsigned long long todo = __ballot(mine != 0u);
        while (todo) {
            const uint32_t leader = (uint32_t)__ffsll((long long)todo) - 1u;
            const uint32_t lr = (uint32_t)__shfl((int)root, (int)leader, 64);
            const bool same = mine != 0u && root == lr;
            const unsigned long long m = __ballot(same);
            uint32_t pts = same ? mine : 0u;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) pts += (uint32_t)__shfl_xor((int)pts, o, 64);
            if (lane == leader) { atomicAdd(cells_at + lr, (uint32_t)__popcll(m)); atomicAdd(points_at + lr, pts); }
            todo &= ~m;
        }
    }
}

struct SegTally { uint32_t novel, cells, roots, listed_mask; };

// the novel points, cell ids, roots and listed roots among this thread's kCropV indices from r0 on
__device__ __forceinline__ SegTally seg_tally(const SegRule& R, const uint32_t* __restrict__ parent, const uint8_t* __restrict__ cls_of,
                                              const uint32_t* __restrict__ cells_at, const uint32_t* __restrict__ points_at, uint32_t r0,
                                              uint32_t n) {
    SegTally t{0u, 0u, 0u, 0u};
#pragma unroll
    for (uint32_t j = 0; j < (uint32_t)kCropV; ++j) {
        const uint64_t r = (uint64_t)r0 + j;
        if (r >= n) break;
        if (seg_is_novel(R, cls_of[r])) ++t.novel;
        const uint32_t p = parent[r];
        if (p == kNoRow) continue;
        ++t.cells;
        if (p != (uint32_t)r) continue;
        ++t.roots;
        if (points_at[r] >= R.min_cluster_points && cells_at[r] >= R.min_cluster_cells) t.listed_mask |= 1u << j;
    }
    return t;
}

static __global__ void __launch_bounds__(kCropT) k_seg_count(SegRule R, const uint32_t* __restrict__ parent, const uint8_t* __restrict__ cls_of,
                                                             const uint32_t* __restrict__ cells_at, const uint32_t* __restrict__ points_at,
                                                             uint32_t n, uint32_t* __restrict__ tile_cnt) {
    const uint64_t r0 = (uint64_t)blockIdx.x * kCropTile + threadIdx.x * kCropV;
    SegTally t{0u, 0u, 0u, 0u};
    if (r0 < n) t = seg_tally(R, parent, cls_of, cells_at, points_at, (uint32_t)r0, n);
    uint32_t t_listed, t_novel, t_cells, t_roots;
    (void)crop_block_scan<kCropT>((uint32_t)__popc(t.listed_mask), &t_listed);
    (void)crop_block_scan<kCropT>(t.novel, &t_novel);
    (void)crop_block_scan<kCropT>(t.cells, &t_cells);
    (void)crop_block_scan<kCropT>(t.roots, &t_roots);
    if (threadIdx.x == 0) {
        uint32_t* o = tile_cnt + 4 * (size_t)blockIdx.x;
        o[0] = t_listed; o[1] = t_novel; o[2] = t_cells; o[3] = t_roots;
    }
}

// tile_cnt[4 t] -> exclusive offsets of the listed roots (in place); counts = {listed clusters, novel points, novel cells, clusters}
static __global__ void __launch_bounds__(kCropScanT) k_seg_scan(uint32_t* __restrict__ tile_cnt, uint32_t tiles, uint32_t* __restrict__ counts) {
    uint32_t carry = 0, sum[3] = {0, 0, 0};
    for (uint32_t base = 0; base < tiles; base += kCropScanT) {
        const uint32_t i = base + threadIdx.x;
        uint32_t total;
        const uint32_t ex = crop_block_scan<kCropScanT>(i < tiles ? tile_cnt[4 * (size_t)i] : 0u, &total);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            uint32_t t;
            (void)crop_block_scan<kCropScanT>(i < tiles ? tile_cnt[4 * (size_t)i + 1 + k] : 0u, &t);
            sum[k] += t;
        }
        if (i < tiles) tile_cnt[4 * (size_t)i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) { counts[0] = carry; counts[1] = sum[0]; counts[2] = sum[1]; counts[3] = sum[2]; }
}

// Roots are in index order, so the listed ones' places are a prefix sum: points_at[root] becomes the cluster's place in the list
// (kNoRow: not listed, or beyond cluster_cap), and the listed clusters' records start as label, cells and the reduction's identities.
static __global__ void __launch_bounds__(kCropT) k_seg_rank(SegRule R, const uint32_t* __restrict__ parent, const uint8_t* __restrict__ cls_of,
                                                            const uint32_t* __restrict__ cells_at, uint32_t* __restrict__ points_at, uint32_t n,
                                                            const uint32_t* __restrict__ tile_cnt, SegRecord* __restrict__ clusters,
                                                            uint32_t cluster_cap) {
    const uint64_t r0 = (uint64_t)blockIdx.x * kCropTile + threadIdx.x * kCropV;
    SegTally t{0u, 0u, 0u, 0u};
    if (r0 < n) t = seg_tally(R, parent, cls_of, cells_at, points_at, (uint32_t)r0, n);
    uint32_t total;
    uint32_t place = tile_cnt[4 * (size_t)blockIdx.x] + crop_block_scan<kCropT>((uint32_t)__popc(t.listed_mask), &total);
#pragma unroll
    for (uint32_t j = 0; j < (uint32_t)kCropV; ++j) {
        const uint64_t r = r0 + j;
        if (r >= n || parent[r] != (uint32_t)r) continue;
        uint32_t at = kNoRow;
        if (t.listed_mask & (1u << j)) {
            if (place < cluster_cap) {
                at = place;
                clusters[place] = seg_record_init((uint32_t)r, cells_at[r]);
            }
            ++place;
        }
        points_at[r] = at;
    }
}

__device__ __forceinline__ long long seg_shfl_xor(long long v, int o) { return __shfl_xor(v, o, 64); }

// Every point of a listed cluster -> the cluster's record; q and the key are made again from the point (12 bytes read instead of 24
// kept).  Points of one wave that share a cluster are combined first (four or more of them: one butterfly over the wave with the
// identities in the other lanes; fewer: their own atomics) — an object's points sit next to each other in a scan.  A combined sum is
// not folded at once: the wave holds it (every lane the same copy) until it combines another cluster, so a cluster that fills the
// wave trip after trip costs one fold a wave, not one a trip (all of them on the same record: they would queue at its cache line).
static __global__ void __launch_bounds__(256) k_seg_reduce(QueryView Q, const float* __restrict__ xyz, uint32_t sf, uint32_t n,
                                                           const double* __restrict__ pose, const uint32_t* __restrict__ root_of,
                                                           const uint32_t* __restrict__ place_at, const uint8_t* __restrict__ cls_of,
                                                           SegRecord* __restrict__ clusters) {
    const uint32_t gsz = gridDim.x * blockDim.x;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t held_at = kNoRow;                         // (uniform over the wave, like held)
    SegSum held = seg_sum_none();
    for (uint64_t r0 = (uint64_t)blockIdx.x * blockDim.x; r0 < n; r0 += gsz) {      // (uniform: ballots and shuffles below)
        const uint64_t i = r0 + threadIdx.x;
        uint32_t at = kNoRow;
        if (i < n) {
            const uint32_t root = root_of[i];
            if (root != kNoRow) at = place_at[root];
        }
        SegSum s = seg_sum_none();
        if (at != kNoRow) {
            float qx, qy, qz;
            seg_transform(pose, xyz + i * sf, qx, qy, qz);
            s = seg_term(query_key<kQueryNode>(Q, qx, qy, qz), qx, qy, qz, cls_of[i]);
        }
        unsigned long long todo = __ballot(at != kNoRow);
        while (todo) {
            const uint32_t leader = (uint32_t)__ffsll((long long)todo) - 1u;
            const uint32_t la = (uint32_t)__shfl((int)at, (int)leader, 64);
            const bool mine = at == la;
            const unsigned long long m = __ballot(mine);
            todo &= ~m;
            if (__popcll(m) < 4) {
                if (mine) seg_fold<SegDeviceOps>(clusters + la, s);
                continue;
            }
            SegSum t = mine ? s : seg_sum_none();
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                SegSum u;
                u.x = seg_shfl_xor(t.x, o); u.y = seg_shfl_xor(t.y, o); u.z = seg_shfl_xor(t.z, o);
                u.sx_min = __shfl_xor(t.sx_min, o, 64); u.sx_max = __shfl_xor(t.sx_max, o, 64);
                u.sy_min = __shfl_xor(t.sy_min, o, 64); u.sy_max = __shfl_xor(t.sy_max, o, 64);
                u.sz_min = __shfl_xor(t.sz_min, o, 64); u.sz_max = __shfl_xor(t.sz_max, o, 64);
                u.z_lo = (uint32_t)__shfl_xor((int)t.z_lo, o, 64); u.z_hi = (uint32_t)__shfl_xor((int)t.z_hi, o, 64);
                u.off_surface = (uint32_t)__shfl_xor((int)t.off_surface, o, 64); u.unmapped = (uint32_t)__shfl_xor((int)t.unmapped, o, 64);
                t = seg_sum_add(t, u);
            }
            if (la == held_at) {
                held = seg_sum_add(held, t);
            } else {
                if (held_at != kNoRow && lane == 0u) seg_fold<SegDeviceOps>(clusters + held_at, held);
                held_at = la;
                held = t;
            }
        }
    }
    if (held_at != kNoRow && lane == 0u) seg_fold<SegDeviceOps>(clusters + held_at, held);
}

// the records the call wrote: min(counts[0], cluster_cap) of them
static __global__ void __launch_bounds__(256) k_seg_finish(SegRecord* __restrict__ clusters, uint32_t cluster_cap, const uint32_t* __restrict__ counts) {
    const uint32_t written = min(counts[0], cluster_cap);
    const uint32_t gsz = gridDim.x * blockDim.x;
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < written; j += gsz) seg_record_finish(clusters + j);
}

}  // namespace gndt
#endif  // __HIPCC__
