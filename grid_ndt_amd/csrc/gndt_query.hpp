// gndt_query.hpp — batched point queries against the finished grid (include/gndt.h "point queries"): which node, or which slope of the
// column, is at a position, and what the cost map says there.
//
// Reference behaviour reproduced: the lookup the reference writes out wherever a consumer needs the slope at a position,
//   transMortonXYZ(p)  ->  map_cell.find(morton_xy)  ->  map_slope.find(morton_z)
// (the goal of TwoDmap::computeCost, include/map2D.h:1291-1306; start and goal of AstarPlanar::findRoute, include/GlobalPlan.h:56-61).
//
// Per query: the point, its key (point_key: the build's own codec), one probe of the (sx, sy) -> first-row index the cost flood also
// uses (k_cost_columns / ctab_find, gndt_cost.hpp), the column's node count (row_ncol), then the column's rows.  Each step needs the
// previous one: a chain of four dependent loads.  query_points can work on ILP independent queries at once, each step issued for all of
// them before the next one waits — but measured on the S2 map (DESIGN.md "Point queries") 2 and 4 were no faster than 1: with 32 waves
// per CU the kernel is bound by the cache lines its four random loads per query fetch (key, value, row_ncol, sz: 128-byte lines for 4-8
// useful bytes, from L2 or the Infinity Cache), not by their latency.  The default is 1 (GNDT_DEBUG_QUERY_ILP selects 2 or 4).
// Everything here is callable on the host as well, so that the CPU test tier runs the kernel's own code (tests/consumer_shim.cpp).
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "gndt_math.hpp"
#include "gndt_cost.hpp"

namespace gndt {

constexpr uint32_t kNoRow = 0xFFFFFFFFu;                 // GNDT_NO_ROW
constexpr int kQueryNode = 0, kQueryNearestSlope = 1;    // GNDT_QUERY_NODE, GNDT_QUERY_NEAREST_SLOPE
constexpr int kWalkLowest = 2, kWalkHighest = 3;         // the raster's other selections (GNDT_RASTER_LOWEST / _HIGHEST)
constexpr uint32_t kQueryChunk = 4;                      // rows of a column read together (S2: 4 levels per column)

struct QueryView {
    CostView V;                     // sx, sy, sz, mean, flags, row_ncol and the column index (ctab_key / ctab_val / ctab_mask)
    const uint32_t* h_bits;         // the cost map of the grid (gather only)
    const uint32_t* state;
    float ox, oy, oz, grid_len, z_len;
};

struct QueryKey {
    int sx, sy, sz;
    bool ok;
};

// The key of a query point.  NODE: the key the build gives the point (point_key), all three axes in range.  NEAREST_SLOPE: x and y only
// (the same axis_index point_key calls); z only has to be finite.  A non-finite coordinate is no key: tested first, as the build's input
// never holds one (the publisher strips them, src/publisher.cpp:24-26).
template <int MODE>
GNDT_HD QueryKey query_key(const QueryView& Q, float px, float py, float pz) {
    QueryKey k;
    const bool finite = isfinite(px) && isfinite(py) && isfinite(pz);
    if (MODE == kQueryNode) {
        const PointKey p = point_key(px, py, pz, Q.ox, Q.oy, Q.oz, Q.grid_len, Q.z_len);
        k.sx = p.sx; k.sy = p.sy; k.sz = p.sz; k.ok = finite && p.ok;
    } else {
        bool ok = finite;
        k.sx = axis_index(px, Q.ox, Q.grid_len, ok, kMaxXY);
        k.sy = axis_index(py, Q.oy, Q.grid_len, ok, kMaxXY);
        k.sz = 0;
        k.ok = ok;
    }
    return k;
}

// First slot of the column's probe sequence (in the table whatever the key: axis_index clamps what it cannot key)
GNDT_HD uint32_t query_slot(const QueryView& Q, const QueryKey& k) { return (uint32_t)mix64(column_pack(k.sx, k.sy)) & Q.V.ctab_mask; }

// The column's first row from what the first slot held; ctab_find walks on if another column took that slot (load <= 1/2: rare)
GNDT_HD uint32_t query_column(const QueryView& Q, const QueryKey& k, uint64_t slot_key, uint32_t slot_val) {
    if (!k.ok) return kNoColumn;
    const uint64_t key = column_pack(k.sx, k.sy);
    if (slot_key == key) return slot_val;
    if (slot_key == kEmptyKey) return kNoColumn;
    return ctab_find(Q.V, k.sx, k.sy);
}

struct QueryBest {
    uint32_t row;
    float d;
    int sz;
};

// One row of the query's column.  NODE: the row whose level is the point's (map_xy's view: any node, with or without statistics or a
// slope).  NEAREST_SLOPE: among the rows with a slope, the least fabsf(mean_z - z) in fp32, a tie going to the smaller sz.  The raster's
// other selections walk the same rows (k_raster): LOWEST / HIGHEST, the slope with the least / greatest sz (a column's levels differ).
template <int MODE>
GNDT_HD void query_eval(uint32_t t, int sz_t, uint32_t flags_t, float mz_t, const QueryKey& k, float pz, QueryBest& b) {
    if (MODE == kQueryNode) {
        if (b.row == kNoRow && sz_t == k.sz) b.row = t;
    } else if (flags_t & 2u) {
        if (MODE == kQueryNearestSlope) {
            const float d = fabsf(mz_t - pz);
            if (b.row == kNoRow || d < b.d || (d == b.d && sz_t < b.sz)) { b.row = t; b.d = d; b.sz = sz_t; }
        } else if (b.row == kNoRow || (MODE == kWalkLowest ? sz_t < b.sz : sz_t > b.sz)) {
            b.row = t; b.sz = sz_t;
        }
    }
}

// Rows [c + from, c + min(from + kQueryChunk, ncol)) of the column: loads first, then the comparisons
template <int MODE>
GNDT_HD void query_chunk(const QueryView& Q, uint32_t c, uint32_t ncol, uint32_t from, const QueryKey& k, float pz, QueryBest& b) {
    int szv[kQueryChunk];
    uint32_t fl[kQueryChunk];
    float mz[kQueryChunk];
#pragma unroll
    for (uint32_t u = 0; u < kQueryChunk; ++u) {
        szv[u] = 0; fl[u] = 0u; mz[u] = 0.f;
        if (from + u < ncol) {
            const uint32_t t = c + from + u;
            szv[u] = Q.V.sz[t];
            if (MODE != kQueryNode) fl[u] = Q.V.flags[t];
            if (MODE == kQueryNearestSlope) mz[u] = Q.V.mean[3 * (size_t)t + 2];
        }
    }
#pragma unroll
    for (uint32_t u = 0; u < kQueryChunk; ++u)
        if (from + u < ncol) query_eval<MODE>(c + from + u, szv[u], fl[u], mz[u], k, pz, b);
}

// The column's rows after the first chunk (a NODE walk stops at its node)
template <int MODE>
GNDT_HD void query_rest(const QueryView& Q, uint32_t c, uint32_t ncol, const QueryKey& k, float pz, QueryBest& b) {
    for (uint32_t from = kQueryChunk; from < ncol && !(MODE == kQueryNode && b.row != kNoRow); from += kQueryChunk)
        query_chunk<MODE>(Q, c, ncol, from, k, pz, b);
}

// Queries i0, i0 + step, ..., i0 + (ILP - 1) step (those below n): row_out[i] = the row or kNoRow; with GATHER also the cost map's h
// (FLT_MAX for kNoRow) and state (0).  xyz: sf floats per point (3 or 4).
template <int ILP, int MODE, bool GATHER>
GNDT_HD void query_points(const QueryView& Q, const float* xyz, uint32_t sf, uint64_t i0, uint64_t step, uint64_t n, uint32_t* row_out,
                          float* h_out, uint32_t* state_out) {
    float px[ILP], py[ILP], pz[ILP];
    QueryKey k[ILP];
    uint32_t slot[ILP], c[ILP], ncol[ILP];
    uint64_t skey[ILP];
    uint32_t sval[ILP];
    QueryBest b[ILP];
#pragma unroll
    for (int j = 0; j < ILP; ++j) {                 // 1. the points
        const uint64_t i = i0 + (uint64_t)j * step;
        px[j] = py[j] = pz[j] = 0.f;
        if (i < n) { const float* p = xyz + i * sf; px[j] = p[0]; py[j] = p[1]; pz[j] = p[2]; }
    }
#pragma unroll
    for (int j = 0; j < ILP; ++j) {                 // 2. keys, and the first probe of the column index
        k[j] = query_key<MODE>(Q, px[j], py[j], pz[j]);
        k[j].ok = k[j].ok && i0 + (uint64_t)j * step < n;
        slot[j] = query_slot(Q, k[j]);
        skey[j] = Q.V.ctab_key[slot[j]];
        sval[j] = Q.V.ctab_val[slot[j]];
    }
#pragma unroll
    for (int j = 0; j < ILP; ++j) {                 // 3. the column's first row and its node count
        c[j] = query_column(Q, k[j], skey[j], sval[j]);
        ncol[j] = c[j] != kNoColumn ? Q.V.row_ncol[c[j]] : 0u;
    }
#pragma unroll
    for (int j = 0; j < ILP; ++j) {                 // 4. the column's rows: the first chunk of every query, then what is left
        b[j].row = kNoRow; b[j].d = 0.f; b[j].sz = 0;
        query_chunk<MODE>(Q, c[j], ncol[j], 0u, k[j], pz[j], b[j]);
    }
#pragma unroll
    for (int j = 0; j < ILP; ++j) query_rest<MODE>(Q, c[j], ncol[j], k[j], pz[j], b[j]);
    uint32_t hb[ILP], st[ILP];
#pragma unroll
    for (int j = 0; j < ILP; ++j) {                 // 5. the answers (and what the cost map holds for them)
        hb[j] = 0x7F7FFFFFu; st[j] = 0u;             // FLT_MAX, untouched
        if (GATHER && b[j].row != kNoRow) { hb[j] = Q.h_bits[b[j].row]; st[j] = Q.state[b[j].row]; }
    }
#pragma unroll
    for (int j = 0; j < ILP; ++j) {
        const uint64_t i = i0 + (uint64_t)j * step;
        if (i < n) {
            row_out[i] = b[j].row;
            if (GATHER) {
                if (h_out) h_out[i] = bits_float(hb[j]);
                if (state_out) state_out[i] = st[j];
            }
        }
    }
}

// ---- raster export (include/gndt.h "raster export"): one pixel per column of an inclusive box of signed column indices ----------------
// Pixel (i, j) sits at j * width + i; i runs over the box's non-zero sx ascending, j over its non-zero sy ascending.  Per pixel: the
// column from (i, j) (integer arithmetic, no keying of a coordinate), one probe of the query's column index, the column's node count,
// the column's rows through the query's walk (query_chunk / query_rest), then the gathers of the selected row.
constexpr int kRasterLowest = 0, kRasterHighest = 1, kRasterNearestZ = 2;   // GNDT_RASTER_LOWEST / _HIGHEST / _NEAREST_Z
constexpr uint32_t kRasterSlope = 1u, kRasterCost = 2u;                       // gathers compiled in: mean z / rough; cost map h / state

// The i-th non-zero index >= lo on an axis (signed indices skip 0: pixels stay one grid_len apart, across the origin too)
GNDT_HD int raster_index(int lo, uint32_t i) {
    const int s = lo + (int)i;
    return lo <= 0 && s >= 0 ? s + 1 : s;
}

// Pixels of the axis [lo, hi]: its non-zero integers (0 when lo > hi)
GNDT_HD uint32_t raster_count(int lo, int hi) {
    if (lo > hi) return 0u;
    return (uint32_t)(hi - lo + 1) - (lo <= 0 && hi >= 0 ? 1u : 0u);
}

struct RasterOut {           // one pointer per layer, null = not written
    uint32_t* row;
    float *z, *rough;
    uint32_t* nodes;
    float* h;
    uint32_t* state;
};

// Pixel p (< width * height) of the box whose smallest indices are (sx_lo, sy_lo).  Q.V.rough is read with kRasterSlope, Q.h_bits and
// Q.state with kRasterCost.
template <int MODE, uint32_t GATHER>
GNDT_HD void raster_pixel(const QueryView& Q, int sx_lo, int sy_lo, uint32_t width, float z_ref, uint32_t p, const RasterOut& o) {
    constexpr int W = MODE == kRasterLowest ? kWalkLowest : MODE == kRasterHighest ? kWalkHighest : kQueryNearestSlope;
    const uint32_t j = p / width, i = p - j * width;
    QueryKey k;
    k.sx = raster_index(sx_lo, i); k.sy = raster_index(sy_lo, j); k.sz = 0; k.ok = true;
    const uint32_t slot = query_slot(Q, k);
    const uint64_t skey = Q.V.ctab_key[slot];
    const uint32_t sval = Q.V.ctab_val[slot];
    const uint32_t c = query_column(Q, k, skey, sval);
    const uint32_t ncol = c != kNoColumn ? Q.V.row_ncol[c] : 0u;
    QueryBest b;
    b.row = kNoRow; b.d = 0.f; b.sz = 0;
    query_chunk<W>(Q, c, ncol, 0u, k, z_ref, b);
    query_rest<W>(Q, c, ncol, k, z_ref, b);
    uint32_t zb = 0x7FC00000u, rb = 0x7FC00000u, hb = 0x7F7FFFFFu, st = 0u;     // quiet NaN, quiet NaN, FLT_MAX, untouched
    if (b.row != kNoRow) {
        if ((GATHER & kRasterSlope) && o.z) zb = float_bits(Q.V.mean[3 * (size_t)b.row + 2]);
        if ((GATHER & kRasterSlope) && o.rough) rb = float_bits(Q.V.rough[b.row]);
        if ((GATHER & kRasterCost) && o.h) hb = Q.h_bits[b.row];
        if ((GATHER & kRasterCost) && o.state) st = Q.state[b.row];
    }
    if (o.row) o.row[p] = b.row;
    if (o.nodes) o.nodes[p] = ncol;
    if ((GATHER & kRasterSlope) && o.z) o.z[p] = bits_float(zb);
    if ((GATHER & kRasterSlope) && o.rough) o.rough[p] = bits_float(rb);
    if ((GATHER & kRasterCost) && o.h) o.h[p] = bits_float(hb);
    if ((GATHER & kRasterCost) && o.state) o.state[p] = st;
}

#if defined(__HIPCC__)
// One thread: ILP queries per pass of a grid-stride loop (any n; the grid is sized to what the chip holds at once)
template <int ILP, int MODE, bool GATHER>
static __global__ void __launch_bounds__(256) k_query(QueryView Q, const float* __restrict__ xyz, uint32_t sf, uint64_t n,
                                                      uint32_t* __restrict__ row_out, float* __restrict__ h_out, uint32_t* __restrict__ state_out) {
    const uint64_t gsz = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i0 < n; i0 += gsz * ILP)
        query_points<ILP, MODE, GATHER>(Q, xyz, sf, i0, gsz, n, row_out, h_out, state_out);
}

// One thread per pixel, grid-stride beyond what the chip holds at once: a wave stores 64 consecutive pixels of every layer
template <int MODE, uint32_t GATHER>
static __global__ void __launch_bounds__(256) k_raster(QueryView Q, int sx_lo, int sy_lo, uint32_t width, uint32_t n, float z_ref, RasterOut o) {
    const uint32_t gsz = gridDim.x * blockDim.x;     // (n <= 2^31 and gsz <= 2^19: p + gsz does not wrap)
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < n; p += gsz) raster_pixel<MODE, GATHER>(Q, sx_lo, sy_lo, width, z_ref, p, o);
}
#endif

}  // namespace gndt
