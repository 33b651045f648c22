// Test-only host shim: grid_ndt_amd/csrc/gndt_merge.hpp's per-node arithmetic (what k_merge_map runs for every source node), compiled
// with g++ for the CPU test tier.  Not part of the product library.
#include <stdint.h>
#include "gndt_merge.hpp"

extern "C" {

// per node: the destination key (ok 0: no key, key_out and out untouched) and the nine sums about the destination node's centre
void mshim_merge(const uint64_t* keys, const uint32_t* count, const double* sums, uint64_t n, const double pose[12], const float so[3],
                 float sgl, float szl, const float dorg[3], float dgl, float dzl, uint64_t* key_out, uint8_t* ok, double* out) {
    gndt::MergeParams P{};
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) P.R[3 * i + j] = pose[4 * i + j];
        P.t[i] = pose[4 * i + 3];
        P.so[i] = so[i];
        P.dorg[i] = dorg[i];
    }
    P.sgl = sgl; P.szl = szl; P.dgl = dgl; P.dzl = dzl;
    for (uint64_t i = 0; i < n; ++i) ok[i] = gndt::merge_node(keys[i], count[i], sums + 9 * i, P, key_out[i], out + 9 * i) ? 1 : 0;
}

}  // extern "C"
