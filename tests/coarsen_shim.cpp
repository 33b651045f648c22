// Test-only host shim: grid_ndt_amd/csrc/gndt_coarsen.hpp's per-node arithmetic (what k_coarsen runs for every source node), compiled
// with g++ for the CPU test tier.  Not part of the product library.
#include <stdint.h>
#include "gndt_coarsen.hpp"

extern "C" {

int cshim_parent_index(int s, int f) { return gndt::parent_index(s, f); }

void cshim_parent_keys(const uint64_t* keys, uint64_t n, int fxy, int fz, uint64_t* out) {
    for (uint64_t i = 0; i < n; ++i) out[i] = gndt::parent_key(keys[i], fxy, fz);
}

// per node: delta (3) and the shifted statistics (9)
void cshim_coarsen(const uint64_t* keys, const uint32_t* count, const double* sums, uint64_t n, int fxy, int fz, const float o[3],
                   float grid_len, float z_len, float coarse_grid_len, float coarse_z_len, double* delta, double* out) {
    for (uint64_t i = 0; i < n; ++i) {
        gndt::coarsen_delta(keys[i], fxy, fz, o, grid_len, z_len, coarse_grid_len, coarse_z_len, delta + 3 * i);
        gndt::coarsen_sums(count[i], sums + 9 * i, delta + 3 * i, out + 9 * i);
    }
}

}  // extern "C"
