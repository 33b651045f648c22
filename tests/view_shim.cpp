// Host build of view gain's per-ray code for the CPU test tier, compiled with g++ (tests/test_view_host.py through
// host_emulation.load_shim): view_one over the rays of every pose as k_view_gain's threads run it, one ray after another, with the
// kernel's mark on two bitmaps of the kernel's size (a plain OR in place of the LDS atomic) and the kernel's tallies and record.  Test
// infrastructure only.
#include <stdint.h>

#include <vector>

#include "gndt_view.hpp"
#include "shim_map.hpp"

using namespace gndt;

namespace {

struct PlainOr {
    uint32_t operator()(uint32_t* w, uint32_t m) const { const uint32_t before = *w; *w = before | m; return before; }
};

}  // namespace

extern "C" {

// out = {reach of (max_range, grid_len), words of one bitmap, LDS bytes of the launch, the largest reach a launch takes without a grant,
// the largest with one}
void viewshim_window(float max_range, float grid_len, uint64_t* out) {
    const uint32_t reach = view_reach(max_range, grid_len);
    out[0] = reach; out[1] = view_words(reach); out[2] = view_lds_bytes(reach);
    out[3] = view_max_reach(kViewLdsDefault); out[4] = view_max_reach(kViewLdsBytes);
}

// K poses (12 doubles each) x n directions (sd floats apart) against the rows and the column index; the parameters with the defaults
// filled in; info: K records of 48 bytes; row, range: [K, n] or null.  The bitmaps are cleared per pose, as the kernel clears them.
int viewshim_gain(const double* poses, uint32_t K, const float* dirs, uint32_t sd, uint32_t n, const ShimMap* m, uint32_t min_count, float max_range,
                  double min_range, void* info, uint32_t* row, float* range) {
    static_assert(sizeof(ViewInfo) == 48, "gndt_view_info");
    const ScoreView S{view_of(*m), m->count, m->cov};
    RayGrid G{};
    G.ox = m->origin[0]; G.oy = m->origin[1]; G.oz = m->origin[2]; G.grid_len = m->grid_len; G.z_len = m->z_len;
    G.max_range = max_range; G.end_margin = 0.f;
    CastParams P{};
    P.min_count = min_count; P.min_range = min_range;
    ViewRule F{};
    F.max_range = max_range;
    F.reach = view_reach(max_range, m->grid_len);
    if (view_words(F.reach) > (1ull << 28)) return 1;
    F.words = (uint32_t)view_words(F.reach);
    std::vector<uint32_t> bits(2 * (size_t)F.words);
    const PlainOr or_;
    for (uint32_t k = 0; k < K; ++k) {
        for (uint32_t& w : bits) w = 0u;
        const double* T = poses + 12 * (size_t)k;
        int lx0, ly0;
        const bool ok = view_origin(G, T, lx0, ly0);
        ViewTally t{};
        for (uint32_t i = 0; i < n; ++i)
            view_one(S, P, G, F, T, lx0, ly0, dirs, sd, i, bits.data(), bits.data() + F.words, or_, t, row ? row + (size_t)k * n : nullptr,
                     range ? range + (size_t)k * n : nullptr);
        view_record(t, ok, static_cast<ViewInfo*>(info)[k]);
    }
    return 0;
}

}  // extern "C"
