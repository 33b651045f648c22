// Host build of the map consumers' per-element code for the CPU test tier, compiled with g++: the point queries' per-point function
// (gndt_query.hpp query_points, at every ILP the kernel is instantiated with) and the column index's probe (ctab_find); the raster
// export's pixel -> column index helper, axis pixel count and per-pixel function (raster_pixel, at every mode and gather mask k_raster
// is instantiated with); free-space clearing's walk of one ray (gndt_ray.hpp ray_begin / ray_next) and the passes of a batch of rays
// as the kernels count them in count-only mode (k_clear_extent, k_clear_protect, k_clear_walk one lane after another), with and
// without the extent skip.  Test infrastructure only (tests/host_emulation.py consumer_shim: test_query_host.py, test_raster_host.py,
// test_clear_host.py).
#include <stdint.h>

#include "gndt_ray.hpp"
#include "shim_map.hpp"

using namespace gndt;

extern "C" {

// The column index k_cost_columns builds, filled sequentially: (sx, sy) of every column's first row -> that row
void build_index(const int32_t* sx, const int32_t* sy, const uint32_t* row_ncol, uint64_t rows, uint64_t* ctab_key, uint32_t* ctab_val,
                 uint32_t ctab_size) {
    for (uint32_t i = 0; i < ctab_size; ++i) ctab_key[i] = kEmptyKey;
    const uint32_t mask = ctab_size - 1;
    for (uint64_t r = 0; r < rows; ++r) {
        if (row_ncol[r] == 0u) continue;
        const uint64_t key = column_pack(sx[r], sy[r]);
        uint32_t s = (uint32_t)mix64(key) & mask;
        while (ctab_key[s] != kEmptyKey) s = (s + 1) & mask;
        ctab_key[s] = key;
        ctab_val[s] = (uint32_t)r;
    }
}

// ---- point queries ----

// n queries (sf floats per point) as the kernel runs them: queries i, i + step, ... with step = the "grid" of `threads` threads
int qshim_query(int mode, int ilp, int gather, const float* xyz, uint32_t sf, uint64_t n, const ShimMap* m, uint64_t threads,
                uint32_t* row_out, float* h_out, uint32_t* state_out) {
    const QueryView Q = view_of(*m);
    const uint64_t step = threads;
#define QSHIM_RUN(ILP, MODE, G)                                                                                      \
    for (uint64_t t = 0; t < step; ++t)                                                                              \
        for (uint64_t i0 = t; i0 < n; i0 += step * ILP) query_points<ILP, MODE, G>(Q, xyz, sf, i0, step, n, row_out, h_out, state_out)
#define QSHIM_MODES(ILP)                                                                                             \
    if (mode == kQueryNode) { if (gather) { QSHIM_RUN(ILP, kQueryNode, true); } else { QSHIM_RUN(ILP, kQueryNode, false); } }     \
    else { if (gather) { QSHIM_RUN(ILP, kQueryNearestSlope, true); } else { QSHIM_RUN(ILP, kQueryNearestSlope, false); } }
    if (mode != kQueryNode && mode != kQueryNearestSlope) return 1;
    if (ilp == 1) { QSHIM_MODES(1) }
    else if (ilp == 2) { QSHIM_MODES(2) }
    else if (ilp == 4) { QSHIM_MODES(4) }
    else return 1;
    return 0;
}

// ctab_find itself (the probe the query falls back to when the first slot belongs to another column)
uint32_t qshim_ctab_find(const uint64_t* ctab_key, const uint32_t* ctab_val, uint32_t ctab_size, int32_t sx, int32_t sy) {
    CostView V{};
    V.ctab_key = ctab_key; V.ctab_val = ctab_val; V.ctab_mask = ctab_size - 1;
    return ctab_find(V, sx, sy);
}

// ---- raster export ----

int rshim_index(int32_t lo, uint32_t i) { return raster_index(lo, i); }

uint32_t rshim_count(int32_t lo, int32_t hi) { return raster_count(lo, hi); }

// Every pixel of a width x (n / width) image, as the kernel's threads run them (pixel p on its own); null layers are not written
int rshim_raster(int mode, uint32_t gather, int32_t sx_lo, int32_t sy_lo, uint32_t width, uint32_t n, float z_ref, const ShimMap* m,
                 uint32_t* row_out, float* z_out, float* rough_out, uint32_t* nodes_out, float* h_out, uint32_t* state_out) {
    const QueryView Q = view_of(*m);
    const RasterOut o{row_out, z_out, rough_out, nodes_out, h_out, state_out};
#define RSHIM_RUN(MODE, G) for (uint32_t p = 0; p < n; ++p) raster_pixel<MODE, G>(Q, sx_lo, sy_lo, width, z_ref, p, o)
#define RSHIM_GATHER(MODE)                                                         \
    if (gather == 0u) { RSHIM_RUN(MODE, 0u); }                                     \
    else if (gather == kRasterSlope) { RSHIM_RUN(MODE, kRasterSlope); }            \
    else if (gather == kRasterCost) { RSHIM_RUN(MODE, kRasterCost); }              \
    else if (gather == (kRasterSlope | kRasterCost)) { RSHIM_RUN(MODE, kRasterSlope | kRasterCost); } \
    else return 1;
    if (mode == kRasterLowest) { RSHIM_GATHER(kRasterLowest) }
    else if (mode == kRasterHighest) { RSHIM_GATHER(kRasterHighest) }
    else if (mode == kRasterNearestZ) { RSHIM_GATHER(kRasterNearestZ) }
    else return 1;
    return 0;
}

// ---- free-space clearing ----

static RayGrid grid_of(const float* map_origin, float grid_len, float z_len, const float* o, float max_range, float end_margin) {
    RayGrid G;
    G.ox = map_origin[0]; G.oy = map_origin[1]; G.oz = map_origin[2]; G.grid_len = grid_len; G.z_len = z_len;
    G.rx = o[0]; G.ry = o[1]; G.rz = o[2]; G.max_range = max_range; G.end_margin = end_margin;
    return G;
}

// The columns of one ray's walk: (sx, sy, lo, hi) per column into out (at most cap columns).  -> columns, -1 when the point is skipped.
int cshim_walk(const float* map_origin, float grid_len, float z_len, const float* o, const float* p, float max_range, float end_margin,
               int32_t* out, int32_t cap) {
    const RayGrid G = grid_of(map_origin, grid_len, z_len, o, max_range, end_margin);
    RayWalk w;
    if (!ray_begin(G, p[0], p[1], p[2], w)) return -1;
    RayColumn c;
    int k = 0;
    while (ray_next(G, w, c)) {
        if (k < cap) { out[4 * k] = c.sx; out[4 * k + 1] = c.sy; out[4 * k + 2] = c.lo; out[4 * k + 3] = c.hi; }
        ++k;
    }
    return k;
}

// Count-only passes of n rays (stride sf floats) against the rows and the column index (build_index)
//; stats = {rays, skipped}
void cshim_passes(const float* o, const float* xyz, uint64_t n, uint32_t sf, float max_range, float end_margin, int use_ext, const ShimMap* m,
                  LevelExtent* ext, uint32_t* passes, uint64_t* stats) {
    const QueryView Q = view_of(*m);
    const RayGrid G = grid_of(m->origin, m->grid_len, m->z_len, o, max_range, end_margin);
    const int32_t* sz = m->sz;
    for (uint64_t r = 0; r < m->n; ++r) { passes[r] = 0u; clear_extent_of(Q, (uint32_t)r, ext); }
    stats[0] = stats[1] = 0;
    for (uint64_t i = 0; i < n; ++i) {          // k_clear_protect
        const float* p = xyz + i * sf;
        RayWalk w;
        if (!ray_begin(G, p[0], p[1], p[2], w)) { ++stats[1]; continue; }
        ++stats[0];
        const uint32_t row = clear_node_row(Q, p[0], p[1], p[2]);
        if (row != kNoRow) passes[row] |= kClearProtected;
    }
    for (uint64_t i = 0; i < n; ++i) {          // k_clear_walk, count-only
        const float* p = xyz + i * sf;
        RayWalk w;
        if (!ray_begin(G, p[0], p[1], p[2], w)) continue;
        RayColumn rc;
        while (ray_next(G, w, rc)) {
            uint32_t ncol;
            const uint32_t c = use_ext ? clear_column<true>(Q, ext, rc, ncol) : clear_column<false>(Q, ext, rc, ncol);
            for (uint32_t t = c; t < c + ncol; ++t)
                if (sz[t] >= rc.lo && sz[t] <= rc.hi) ++passes[t];
        }
    }
}

}  // extern "C"
