// Host build of the raster export's code (grid_ndt_amd/csrc/gndt_query.hpp) for the CPU test tier: the pixel -> column index helper,
// the axis pixel count, and the kernel's own per-pixel function (raster_pixel, at every mode and gather mask k_raster is instantiated
// with), compiled with g++.  Test infrastructure only (tests/test_raster_host.py).
#include <stdint.h>

#include "gndt_query.hpp"

using namespace gndt;

extern "C" {

int rshim_index(int32_t lo, uint32_t i) { return raster_index(lo, i); }

uint32_t rshim_count(int32_t lo, int32_t hi) { return raster_count(lo, hi); }

// The column index k_cost_columns builds, filled sequentially: (sx, sy) of every column's first row -> that row
void rshim_build_index(const int32_t* sx, const int32_t* sy, const uint32_t* row_ncol, uint64_t rows, uint64_t* ctab_key, uint32_t* ctab_val,
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

// Every pixel of a width x (n / width) image, as the kernel's threads run them (pixel p on its own); null layers are not written
int rshim_raster(int mode, uint32_t gather, int32_t sx_lo, int32_t sy_lo, uint32_t width, uint32_t n, float z_ref, const int32_t* sx,
                 const int32_t* sy, const int32_t* sz, const float* mean, const float* rough, const uint32_t* flags, const uint32_t* row_ncol,
                 const uint64_t* ctab_key, const uint32_t* ctab_val, uint32_t ctab_size, const uint32_t* h_bits, const uint32_t* state,
                 uint32_t* row_out, float* z_out, float* rough_out, uint32_t* nodes_out, float* h_out, uint32_t* state_out) {
    QueryView Q{};
    Q.V.sx = sx; Q.V.sy = sy; Q.V.sz = sz; Q.V.mean = mean; Q.V.rough = rough; Q.V.flags = flags; Q.V.row_ncol = row_ncol;
    Q.V.ctab_key = ctab_key; Q.V.ctab_val = ctab_val; Q.V.ctab_mask = ctab_size - 1;
    Q.h_bits = h_bits; Q.state = state;
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

}  // extern "C"
