// Host build of the point-query code (grid_ndt_amd/csrc/gndt_query.hpp) for the CPU test tier: the kernel's own per-point function
// (query_points, at every ILP the kernel is instantiated with) and the column index's probe (ctab_find), compiled with g++.
// Test infrastructure only (tests/test_query_host.py).
#include <stdint.h>

#include "gndt_query.hpp"

using namespace gndt;

extern "C" {

// The column index k_cost_columns builds, filled sequentially: (sx, sy) of every column's first row -> that row
void qshim_build_index(const int32_t* sx, const int32_t* sy, const uint32_t* row_ncol, uint64_t rows, uint64_t* ctab_key, uint32_t* ctab_val,
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

// n queries (sf floats per point) as the kernel runs them: queries i, i + step, ... with step = the "grid" of `threads` threads
int qshim_query(int mode, int ilp, int gather, const float* xyz, uint32_t sf, uint64_t n, const int32_t* sx, const int32_t* sy, const int32_t* sz,
                const float* mean, const uint32_t* flags, const uint32_t* row_ncol, const uint64_t* ctab_key, const uint32_t* ctab_val,
                uint32_t ctab_size, const uint32_t* h_bits, const uint32_t* state, const float* origin, float grid_len, float z_len,
                uint64_t threads, uint32_t* row_out, float* h_out, uint32_t* state_out) {
    QueryView Q{};
    Q.V.sx = sx; Q.V.sy = sy; Q.V.sz = sz; Q.V.mean = mean; Q.V.flags = flags; Q.V.row_ncol = row_ncol;
    Q.V.ctab_key = ctab_key; Q.V.ctab_val = ctab_val; Q.V.ctab_mask = ctab_size - 1;
    Q.h_bits = h_bits; Q.state = state;
    Q.ox = origin[0]; Q.oy = origin[1]; Q.oz = origin[2]; Q.grid_len = grid_len; Q.z_len = z_len;
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

}  // extern "C"
