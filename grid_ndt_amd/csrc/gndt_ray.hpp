// gndt_ray.hpp — free-space clearing (include/gndt.h "free-space clearing"): the nodes sensor rays pass through leave the map.
//
// The walk of one ray is a DEFINITION (the header states it; tests/clear_ref.py restates it in numpy, fp64): a cut point on the segment,
// the codec's columns of the ray's origin and of the cut point, exactly |dx| + |dy| unit steps between them, each across the lattice
// plane the segment meets first (fp64 crossing parameter, a tie stepping x), and in every column the levels between the ray's z at the
// column's entry and at its exit (the codec's level of the origin / the cut point at the ends, the codec's rule in fp64 inside).
// Everything up to the rows is callable on the host as well, so that the CPU test tier runs the kernel's own code (tests/consumer_shim.cpp).
// Ray casting (gndt_cast.hpp) walks the same way from an origin per ray: ray_begin's second overload checks that origin like an end
// point, ray_next's second overload also hands out the step's crossing parameter and the column's entry and exit levels (RayCross).
//
// Kernels (gndt_api_clear.hip launches them in this order):
//   k_clear_extent   (GNDT_DEBUG_CLEAR_EXTENT only) per column, at its first row: the least and greatest sz of its rows (the walk skips a column whose extent misses
//                    the ray's level range without reading its rows)
//   k_clear_protect  the NODE query of every uncut end point (the query's own code); its row gets bit 31.  Counts rays and skipped points.
//   k_clear_walk     one ray per lane, in input order: per column one probe of the query's column index, then the rows whose sz lies in
//                    the level range get a pass.  A wave whose active lanes all stand in the same column adds once per row.
//   k_clear_kill     per row: the protected rows are counted; while clearing, a row with passes >= min_passes that is not protected
//                    loses its node (find_slot of its key, count 0, n_dead + 1) and its count is clamped to min_passes.
#pragma once
#include <math.h>
#include <stdint.h>

#include "gndt_query.hpp"

namespace gndt {

constexpr uint32_t kClearProtected = 0x80000000u;    // GNDT_CLEAR_PROTECTED
constexpr uint32_t kClearCount = 0x7FFFFFFFu;        // bits 0-30: the pass count

struct RayGrid {                 // the map's lattice (the handle's origin and cell sizes) and the call's ray parameters
    float ox, oy, oz, grid_len, z_len;
    float rx, ry, rz;            // the sensor origin
    float max_range, end_margin;
};

struct LevelExtent {             // the least and greatest sz of a column's rows
    int32_t lo, hi;
};

// Signed axis index (no 0) <-> lattice cell: cell l spans the planes l and l + 1 (in grid_len from the map origin)
GNDT_HD int ray_lin(int s) { return s > 0 ? s - 1 : s; }
GNDT_HD int ray_signed(int l) { return l >= 0 ? l + 1 : l; }

// The codec's level rule in fp64: sign * max(1, ceil(|z - oz| / z_len)), + iff z > oz (clamped to the codec's range)
GNDT_HD int ray_level(double z, float oz, float z_len) {
    const double q = fabs(z - (double)oz) / (double)z_len;
    double c = ceil(q);
    if (c < 1.0) c = 1.0;
    if (c > (double)kMaxZ) c = (double)kMaxZ;
    const int n = (int)c;
    return z > (double)oz ? n : -n;
}

// Where the ray r + t d meets the lattice plane k of an axis, t clamped to [0, 1] (1 on an axis the ray does not move along)
GNDT_HD double ray_cross(float o_axis, float len, int k, double r, double d) {
    if (d == 0.0) return 1.0;
    const double t = ((double)o_axis + (double)k * (double)len - r) / d;
    return t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
}

struct RayWalk {
    double r[3], d[3];           // the ray's origin and its UNCUT direction p - o, fp64
    double f, len;               // the cut factor (e = o + d f; 1: nothing is cut) and |d|
    int lx, ly, lx1, ly1;        // the current column and the last one, as lattice cells
    int lev_in, sz_end;          // the current column's entry level; the cut point's level
    bool done;
};

struct RayColumn {
    int sx, sy, lo, hi;          // a column the ray walks, and the levels it walks there (lo <= hi)
};

struct RayCross {                // what ray casting (gndt_cast.hpp) needs of a column visit besides RayColumn
    double t;                    // the crossing parameter of the step that leaves the column, in units of the uncut d (the last column: the cut factor)
    int lev_in, lev_out;         // the levels at the column's entry and exit: lo / hi in walk order
};

// The walk from the keyed, finite origin (rx, ry, rz) to the keyed, finite end point p (G.rx / ry / rz are not read)
GNDT_HD void ray_setup(const RayGrid& G, float rx, float ry, float rz, float px, float py, float pz, RayWalk& w) {
    w.r[0] = (double)rx; w.r[1] = (double)ry; w.r[2] = (double)rz;
    w.d[0] = (double)px - w.r[0]; w.d[1] = (double)py - w.r[1]; w.d[2] = (double)pz - w.r[2];
    // the cut point e = o + d * min(1, max_range / |d|, max(0, |d| - end_margin) / |d|), fp64; e = p when nothing is cut
    const double L = sqrt(w.d[0] * w.d[0] + w.d[1] * w.d[1] + w.d[2] * w.d[2]);
    double f = 1.0;
    if (L > 0.0) {
        if (G.max_range > 0.f) f = fmin(f, (double)G.max_range / L);
        f = fmin(f, fmax(0.0, L - (double)G.end_margin) / L);
    }
    float e[3] = {px, py, pz};
    if (f < 1.0)
        for (int a = 0; a < 3; ++a) e[a] = (float)(w.r[a] + w.d[a] * f);
    const PointKey ko = point_key(rx, ry, rz, G.ox, G.oy, G.oz, G.grid_len, G.z_len);
    const PointKey ke = point_key(e[0], e[1], e[2], G.ox, G.oy, G.oz, G.grid_len, G.z_len);
    w.f = f; w.len = L;
    w.lx = ray_lin(ko.sx); w.ly = ray_lin(ko.sy);
    w.lx1 = ray_lin(ke.sx); w.ly1 = ray_lin(ke.sy);
    w.lev_in = ko.sz; w.sz_end = ke.sz;
    w.done = false;
}

// A point a ray can start or end at: finite, and keyed by the codec
GNDT_HD bool ray_point_ok(const RayGrid& G, float x, float y, float z) {
    if (!(isfinite(x) && isfinite(y) && isfinite(z))) return false;
    return point_key(x, y, z, G.ox, G.oy, G.oz, G.grid_len, G.z_len).ok;
}

// The ray to end point p: false if p is not finite or has no key (the point is skipped).  The sensor origin is keyed (checked by the host).
GNDT_HD bool ray_begin(const RayGrid& G, float px, float py, float pz, RayWalk& w) {
    if (!ray_point_ok(G, px, py, pz)) return false;
    ray_setup(G, G.rx, G.ry, G.rz, px, py, pz, w);
    return true;
}

// The ray from an origin of its own (ray casting: one per ray, checked here like the end point)
GNDT_HD bool ray_begin(const RayGrid& G, float rx, float ry, float rz, float px, float py, float pz, RayWalk& w) {
    if (!ray_point_ok(G, rx, ry, rz) || !ray_point_ok(G, px, py, pz)) return false;
    ray_setup(G, rx, ry, rz, px, py, pz, w);
    return true;
}

// The next column of the walk, its level range and (x) the step that leaves it; false once the cut point's column has been given
GNDT_HD bool ray_next(const RayGrid& G, RayWalk& w, RayColumn& c, RayCross& x) {
    if (w.done) return false;
    const bool mx = w.lx != w.lx1, my = w.ly != w.ly1;
    int lev_out;
    bool step_x = false;
    if (!mx && !my) {
        lev_out = w.sz_end;
        x.t = w.f;
        w.done = true;
    } else {
        double tx = 2.0, ty = 2.0;
        if (mx) tx = ray_cross(G.ox, G.grid_len, w.lx1 > w.lx ? w.lx + 1 : w.lx, w.r[0], w.d[0]);
        if (my) ty = ray_cross(G.oy, G.grid_len, w.ly1 > w.ly ? w.ly + 1 : w.ly, w.r[1], w.d[1]);
        step_x = mx && (!my || tx <= ty);
        const double t = step_x ? tx : ty;
        lev_out = ray_level(w.r[2] + t * w.d[2], G.oz, G.z_len);
        x.t = t;
    }
    x.lev_in = w.lev_in; x.lev_out = lev_out;
    c.sx = ray_signed(w.lx); c.sy = ray_signed(w.ly);
    c.lo = w.lev_in < lev_out ? w.lev_in : lev_out;
    c.hi = w.lev_in < lev_out ? lev_out : w.lev_in;
    if (!w.done) {
        if (step_x) w.lx += w.lx1 > w.lx ? 1 : -1;
        else w.ly += w.ly1 > w.ly ? 1 : -1;
        w.lev_in = lev_out;
    }
    return true;
}

// The column and its level range alone (free-space clearing)
GNDT_HD bool ray_next(const RayGrid& G, RayWalk& w, RayColumn& c) {
    RayCross x;
    return ray_next(G, w, c, x);
}

// A walked column -> its first row (kNoColumn: not in the map) and the rows to look at: its node count, or 0 when (EXT) the column's
// level extent misses [lo, hi]
template <bool EXT>
GNDT_HD uint32_t clear_column(const QueryView& Q, const LevelExtent* ext, const RayColumn& rc, uint32_t& ncol) {
    QueryKey k;
    k.sx = rc.sx; k.sy = rc.sy; k.sz = 0; k.ok = true;
    const uint32_t slot = query_slot(Q, k);
    const uint32_t c = query_column(Q, k, Q.V.ctab_key[slot], Q.V.ctab_val[slot]);
    ncol = 0u;
    if (c == kNoColumn) return c;
    if (EXT) {
        const LevelExtent e = ext[c];
        if (e.hi < rc.lo || e.lo > rc.hi) return c;
    }
    ncol = Q.V.row_ncol[c];
    return c;
}

// The NODE row of an end point (GNDT_QUERY_NODE: the query's own code), kNoRow if none
GNDT_HD uint32_t clear_node_row(const QueryView& Q, float px, float py, float pz) {
    const QueryKey k = query_key<kQueryNode>(Q, px, py, pz);
    const uint32_t slot = query_slot(Q, k);
    const uint32_t c = query_column(Q, k, Q.V.ctab_key[slot], Q.V.ctab_val[slot]);
    const uint32_t ncol = c != kNoColumn ? Q.V.row_ncol[c] : 0u;
    QueryBest b;
    b.row = kNoRow; b.d = 0.f; b.sz = 0;
    query_chunk<kQueryNode>(Q, c, ncol, 0u, k, pz, b);
    query_rest<kQueryNode>(Q, c, ncol, k, pz, b);
    return b.row;
}

// The extent of the column whose first row is r (rows with row_ncol[r] == 0 are not first rows and are not written)
GNDT_HD void clear_extent_of(const QueryView& Q, uint32_t r, LevelExtent* ext) {
    const uint32_t ncol = Q.V.row_ncol[r];
    if (ncol == 0u) return;
    int lo = Q.V.sz[r], hi = lo;
    for (uint32_t u = 1; u < ncol; ++u) {
        const int z = Q.V.sz[r + u];
        lo = z < lo ? z : lo;
        hi = z > hi ? z : hi;
    }
    ext[r].lo = lo; ext[r].hi = hi;
}

#if defined(__HIPCC__)
static __global__ void __launch_bounds__(256) k_clear_extent(QueryView Q, uint32_t rows, LevelExtent* __restrict__ ext) {
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += gridDim.x * blockDim.x) clear_extent_of(Q, r, ext);
}

// stats: {rays, skipped, protected rows, cleared}
static __global__ void __launch_bounds__(256) k_clear_protect(QueryView Q, RayGrid G, const float* __restrict__ xyz, uint32_t sf, uint64_t n,
                                                              uint32_t* __restrict__ passes, unsigned long long* __restrict__ stats) {
    const uint64_t gsz = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t n_round = (n + 63) & ~63ull;          // whole waves, so that the tally below has every lane
    unsigned long long rays = 0, skipped = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_round; i += gsz) {
        if (i >= n) continue;
        const float* p = xyz + i * sf;
        const float px = p[0], py = p[1], pz = p[2];
        const bool ok = isfinite(px) && isfinite(py) && isfinite(pz) && point_key(px, py, pz, G.ox, G.oy, G.oz, G.grid_len, G.z_len).ok;
        if (!ok) { ++skipped; continue; }
        ++rays;
        const uint32_t row = clear_node_row(Q, px, py, pz);
        // (many end points share a node: the bit is set once, the others see it and do not write)
        if (row != kNoRow && !(passes[row] & kClearProtected)) atomicOr(&passes[row], kClearProtected);
    }
    for (int off = 32; off > 0; off >>= 1) {
        rays += __shfl_down(rays, off, 64);
        skipped += __shfl_down(skipped, off, 64);
    }
    if (__lane_id() == 0) {
        if (rays) atomicAdd(&stats[0], rays);
        if (skipped) atomicAdd(&stats[1], skipped);
    }
}

// One pass (k of them) for row t.  Count-only: exact.  Clearing: nothing for a protected row or one that already has min_passes (a
// stale read can add a few more: k_clear_kill clamps).
template <bool CLEAR>
__device__ __forceinline__ void clear_pass(uint32_t* passes, uint32_t t, uint32_t k, uint32_t min_passes) {
    if (CLEAR) {
        const uint32_t v = passes[t];
        if ((v & kClearProtected) || v >= min_passes) return;
    }
    atomicAdd(&passes[t], k);
}

template <bool CLEAR, bool EXT>
static __global__ void __launch_bounds__(256) k_clear_walk(QueryView Q, RayGrid G, const float* __restrict__ xyz, uint32_t sf, uint64_t n,
                                                           const LevelExtent* __restrict__ ext, uint32_t* __restrict__ passes, uint32_t min_passes) {
    const uint64_t gsz = (uint64_t)gridDim.x * blockDim.x;
    const int lane = (int)__lane_id();
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gsz) {
        const float* p = xyz + i * sf;
        RayWalk w;
        if (!ray_begin(G, p[0], p[1], p[2], w)) continue;
        RayColumn rc;
        while (ray_next(G, w, rc)) {
            uint32_t ncol;
            const uint32_t c = clear_column<EXT>(Q, ext, rc, ncol);
            const unsigned long long act = __ballot(1);
            const int first = __ffsll(act) - 1;
            const uint32_t c0 = (uint32_t)__shfl((int)c, first, 64);
            if (__ballot(c != c0) == 0ull) {
                // every active lane stands in the same column (the origin's for all rays of a frame; the first columns of rays that
                // leave together): one add per row, by the first lane, of the lanes whose level range holds the row
                const unsigned long long has = __ballot(ncol != 0u);
                if (c0 == kNoColumn || has == 0ull) continue;
                const uint32_t nc = (uint32_t)__shfl((int)ncol, __ffsll(has) - 1, 64);
                for (uint32_t t = c0; t < c0 + nc; ++t) {
                    const int z = Q.V.sz[t];
                    const unsigned long long m = __ballot(z >= rc.lo && z <= rc.hi);
                    if (lane == first && m) clear_pass<CLEAR>(passes, t, (uint32_t)__popcll(m), min_passes);
                }
            } else {
                for (uint32_t t = c; t < c + ncol; ++t) {
                    const int z = Q.V.sz[t];
                    if (z >= rc.lo && z <= rc.hi) clear_pass<CLEAR>(passes, t, 1u, min_passes);
                }
            }
        }
    }
}

// Per row: the protected ones are counted; while clearing, a row with at least min_passes that is not protected loses its node in the
// node table (count 0: the compaction that follows drops it, gndt_remove's path) and every count is clamped to min_passes.
template <bool CLEAR>
static __global__ void __launch_bounds__(256) k_clear_kill(const int32_t* __restrict__ sx, const int32_t* __restrict__ sy, const int32_t* __restrict__ sz,
                                                           uint32_t rows, uint32_t* __restrict__ passes, uint32_t min_passes,
                                                           const uint64_t* __restrict__ keys, NodeAcc* __restrict__ acc, uint32_t cap_mask,
                                                           Counters* __restrict__ cnt, unsigned long long* __restrict__ stats) {
    const uint32_t gsz = gridDim.x * blockDim.x;
    const uint32_t r_round = (rows + 63u) & ~63u;
    unsigned long long prot = 0, dead = 0;
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < r_round; r += gsz) {
        if (r >= rows) continue;
        const uint32_t v = passes[r];
        if (v & kClearProtected) { ++prot; continue; }
        if (!CLEAR) continue;
        if (v >= min_passes) {
            if (v != min_passes) passes[r] = min_passes;
            const uint32_t slot = find_slot(keys, cap_mask, pack_key(sx[r], sy[r], sz[r]));
            if (slot <= cap_mask) { acc[slot].count = 0u; ++dead; }
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        prot += __shfl_down(prot, off, 64);
        dead += __shfl_down(dead, off, 64);
    }
    if (__lane_id() == 0) {
        if (prot) atomicAdd(&stats[2], prot);
        if (dead) { atomicAdd(&stats[3], dead); atomicAdd(&cnt->n_dead, (uint32_t)dead); }
    }
}
#endif

}  // namespace gndt
