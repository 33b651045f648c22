// Host build of the surface patches' per-row code (grid_ndt_amd/csrc/gndt_patch.hpp: patch_mark, patch_link with the frontiers'
// union-find, patch_term / patch_fold, patch_moments, patch_fit) for the CPU test tier, compiled with g++: the passes of the kernels run
// one row after another, the link pass in any row order the caller names, with parent[x] <= x looked at after every union.  The list (the
// ordered compaction of the roots, a scan on the device) is a plain loop here; the ten sums are added in ascending row.  Test
// infrastructure only (tests/test_patch_host.py).
#include <stdint.h>

#include <vector>

#include "gndt_patch.hpp"
#include "shim_map.hpp"

using namespace gndt;

namespace {

ScoreView score_view_of(const ShimMap& m) {
    ScoreView S{};
    S.Q = view_of(m);
    S.count = m.count;
    S.cov = m.cov;
    return S;
}

// ints: {candidates, connectivity, boxed, sx_min, sx_max, sy_min, sy_max}; floats: {cos_min, max_offset, max_var, cos_level, sin_level}
PatchRule rule_of(const int32_t* ints, const float* floats) {
    return PatchRule{ints[0], (uint32_t)ints[1], floats[0], floats[1], floats[2], (double)floats[3], (double)floats[4],
                     ints[2], ints[3], ints[4], ints[5], ints[6]};
}

}  // namespace

extern "C" {

// out[i] = patch_links(a[i], b[i]) for k pairs of rows
void pshim_links(const int32_t* ints, const float* floats, const ShimMap* m, const uint32_t* a, const uint32_t* b, uint64_t k, uint8_t* out) {
    const ScoreView S = score_view_of(*m);
    const PatchRule F = rule_of(ints, floats);
    for (uint64_t i = 0; i < k; ++i) out[i] = patch_links(S.Q.V, F, a[i], b[i]) ? 1 : 0;
}

// order: the rows in the order the link pass takes them (null: ascending).  label [n], patches [cap], counts [4] as gndt_patches writes
// them.  Returns 0, or 1 + the row at which parent[x] <= x failed.
int64_t pshim_patches(const int32_t* ints, const float* floats, uint32_t min_size, const uint32_t* order, const ShimMap* m, uint32_t* label,
                      PatchRecord* patches, uint32_t cap, uint32_t* counts) {
    const ScoreView S = score_view_of(*m);
    const uint32_t n = (uint32_t)m->n;
    const PatchRule F = rule_of(ints, floats);
    using Ops = FrontierSerialOps;
    std::vector<uint32_t> parent(n), size_at(n, 0u);
    // mark
    for (uint32_t r = 0; r < n; ++r) parent[r] = patch_mark(S, F, r) ? r : kNoRow;
    // link
    int64_t bad = 0;
    const auto chain_ok = [&](uint32_t x) {
        for (uint32_t step = 0; step <= n; ++step) {
            const uint32_t p = parent[x];
            if (p > x) { if (!bad) bad = 1 + (int64_t)x; return; }
            if (p == x) return;
            x = p;
        }
        if (!bad) bad = 1 + (int64_t)x;           // a cycle
    };
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t r = order ? order[i] : i;
        if (parent[r] == kNoRow) continue;
        patch_link<Ops>(S, F, parent.data(), r, n, [&](uint32_t a, uint32_t t) { chain_ok(a); chain_ok(t); });
    }
    for (uint32_t r = 0; r < n; ++r)
        if (parent[r] != kNoRow && parent[r] > r && !bad) bad = 1 + (int64_t)r;
    if (bad) return bad;
    // flatten, and the roots' member counts
    for (uint32_t r = 0; r < n; ++r) {
        uint32_t root = kNoRow;
        if (parent[r] != kNoRow) {
            root = frontier_root<Ops>(parent.data(), r, n);
            parent[r] = root;
            ++size_at[root];
        }
        label[r] = root;
    }
    // the list: roots in row order, those with min_size members get the next place
    std::vector<double> moments((size_t)kPatchMoments * cap, 0.0);
    uint32_t listed = 0, rows = 0, roots = 0;
    for (uint32_t r = 0; r < n; ++r) {
        if (parent[r] == kNoRow) continue;
        ++rows;
        if (parent[r] != r) continue;
        ++roots;
        uint32_t at = kNoRow;
        if (size_at[r] >= min_size) {
            if (listed < cap) { at = listed; patches[listed] = patch_record_init(r, size_at[r]); }
            ++listed;
        }
        size_at[r] = at;
    }
    counts[0] = listed; counts[1] = rows; counts[2] = roots; counts[3] = 0u;
    // reduce: the integer fields and the ten sums
    for (uint32_t r = 0; r < n; ++r) {
        if (parent[r] == kNoRow) continue;
        const uint32_t at = size_at[parent[r]];
        if (at == kNoRow) continue;
        patch_fold<Ops>(patches + at, patch_term(S, r));
        double q[kPatchMoments];
        patch_moments(S, r, parent[r], q);
        for (int k = 0; k < kPatchMoments; ++k) moments[(size_t)kPatchMoments * at + k] += q[k];
    }
    // fit
    const uint32_t written = listed < cap ? listed : cap;
    for (uint32_t p = 0; p < written; ++p)
        patch_fit(F, moments.data() + (size_t)kPatchMoments * p, S.Q.V.mean + 3 * (size_t)patches[p].label, patches + p);
    return 0;
}

}  // extern "C"
