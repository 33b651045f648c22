// shim_map.hpp — the one struct a finished map crosses the C boundary in, for every host shim of the CPU test tier, and the view the
// shared headers read it through.  tests/host_emulation.py mirrors the struct (ShimMap there) and MapRows fills it; load_shim checks the
// mirror against shim_map_layout / shim_map_fields when it loads a shim, so a drift between the two declarations is a failed load.
// A null pointer stands for an array the caller's code does not read.  Test infrastructure only.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "gndt_query.hpp"

extern "C" struct ShimMap {
    uint64_t n;                             // rows
    const int32_t *sx, *sy, *sz;            // the row arrays, in CostView's order
    const float *mean, *normal, *rough;
    const uint32_t* flags;
    const uint32_t* count;                  // the scoring and cast shims' (ScoreView)
    const float* cov;
    const uint32_t* row_ncol;
    const uint64_t* ctab_key;               // the column index (consumer_shim.cpp build_index), ctab_size slots: a power of two
    const uint32_t* ctab_val;
    uint32_t ctab_size;
    const uint32_t *h_bits, *state;         // the cost map
    float origin[3], grid_len, z_len, slope_interval;
    int32_t demand_true;
};

// every field, in the struct's order
#define SHIM_MAP_FIELDS(X) \
    X(n) X(sx) X(sy) X(sz) X(mean) X(normal) X(rough) X(flags) X(count) X(cov) X(row_ncol) X(ctab_key) X(ctab_val) X(ctab_size) \
    X(h_bits) X(state) X(origin) X(grid_len) X(z_len) X(slope_interval) X(demand_true)

extern "C" {

// out[0] = sizeof(ShimMap), out[1 ...] = every field's offset and size (padding hides a width from the offsets alone), in the order of
// shim_map_fields; returns the words written (at most 64)
__attribute__((used)) inline uint32_t shim_map_layout(uint32_t* out) {
    uint32_t k = 0;
    out[k++] = (uint32_t)sizeof(ShimMap);
#define SHIM_MAP_OFFSET(f) out[k++] = (uint32_t)offsetof(ShimMap, f); out[k++] = (uint32_t)sizeof(ShimMap::f);
    SHIM_MAP_FIELDS(SHIM_MAP_OFFSET)
#undef SHIM_MAP_OFFSET
    return k;
}

// the fields' names, space separated
__attribute__((used)) inline const char* shim_map_fields() {
#define SHIM_MAP_NAME(f) #f " "
    return SHIM_MAP_FIELDS(SHIM_MAP_NAME);
#undef SHIM_MAP_NAME
}

}  // extern "C"

// The rows, the column index, the cost map and the grid as the kernels read them; the flood's tables (nbr, self, edges) stay null
inline gndt::QueryView view_of(const ShimMap& m) {
    gndt::QueryView Q{};
    gndt::CostView& V = Q.V;
    V.sx = m.sx; V.sy = m.sy; V.sz = m.sz;
    V.mean = m.mean; V.normal = m.normal; V.rough = m.rough; V.flags = m.flags;
    V.row_ncol = m.row_ncol;
    V.ctab_key = m.ctab_key; V.ctab_val = m.ctab_val; V.ctab_mask = m.ctab_size - 1;
    V.slope_interval = m.slope_interval; V.demand_true = m.demand_true;
    Q.h_bits = m.h_bits; Q.state = m.state;
    Q.ox = m.origin[0]; Q.oy = m.origin[1]; Q.oz = m.origin[2]; Q.grid_len = m.grid_len; Q.z_len = m.z_len;
    return Q;
}
