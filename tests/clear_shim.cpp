// Host build of free-space clearing's code (grid_ndt_amd/csrc/gndt_ray.hpp) for the CPU test tier: the walk of one ray (ray_begin /
// ray_next, the kernel's own functions), and the passes of a batch of rays as the kernels count them in count-only mode (k_clear_extent,
// k_clear_protect, k_clear_walk one lane after another), with and without the extent skip.  Compiled with g++.  Test infrastructure only
// (tests/test_clear_host.py).
#include <stdint.h>

#include "gndt_ray.hpp"

using namespace gndt;

extern "C" {

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

// Count-only passes of n rays (stride sf floats) against the rows and the column index (tests/raster_shim.cpp's rshim_build_index
// layout); stats = {rays, skipped}
void cshim_passes(const float* map_origin, float grid_len, float z_len, const float* o, const float* xyz, uint64_t n, uint32_t sf,
                  float max_range, float end_margin, int use_ext, const int32_t* sx, const int32_t* sy, const int32_t* sz,
                  const uint32_t* row_ncol, uint64_t rows, const uint64_t* ctab_key, const uint32_t* ctab_val, uint32_t ctab_size,
                  LevelExtent* ext, uint32_t* passes, uint64_t* stats) {
    QueryView Q{};
    Q.V.sx = sx; Q.V.sy = sy; Q.V.sz = sz; Q.V.row_ncol = row_ncol;
    Q.V.ctab_key = ctab_key; Q.V.ctab_val = ctab_val; Q.V.ctab_mask = ctab_size - 1;
    Q.ox = map_origin[0]; Q.oy = map_origin[1]; Q.oz = map_origin[2]; Q.grid_len = grid_len; Q.z_len = z_len;
    const RayGrid G = grid_of(map_origin, grid_len, z_len, o, max_range, end_margin);
    for (uint64_t r = 0; r < rows; ++r) { passes[r] = 0u; clear_extent_of(Q, (uint32_t)r, ext); }
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

extern "C" {

// The column index k_cost_columns builds (tests/raster_shim.cpp's layout), filled sequentially
void cshim_build_index(const int32_t* sx, const int32_t* sy, const uint32_t* row_ncol, uint64_t rows, uint64_t* ctab_key, uint32_t* ctab_val,
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

}  // extern "C"
