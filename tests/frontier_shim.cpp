// Host build of frontier extraction's per-row code (grid_ndt_amd/csrc/gndt_frontier.hpp: frontier_mark, frontier_link with its
// union-find, frontier_term / frontier_fold) for the CPU test tier, compiled with g++: the passes of the kernels run one row after
// another, the link pass in any row order the caller names, with parent[x] <= x looked at after every union.  The list (the ordered
// compaction of the roots, a scan on the device) is a plain loop here.  Test infrastructure only (tests/test_frontier_host.py).
#include <stdint.h>

#include <vector>

#include "gndt_frontier.hpp"
#include "shim_map.hpp"

using namespace gndt;

extern "C" {

int fshim_lin(int s) { return frontier_lin(s); }

// rule: {candidates, open_rule, level_reach, min_open, link_dz, boxed, sx_min, sx_max, sy_min, sy_max}; order: the rows in the order the
// link pass takes them (null: ascending).  label [n], open [n] (kFrontierNone for a row that is no frontier row), clusters [cap],
// counts [4] as gndt_frontiers writes them.  Returns 0, or 1 + the row at which parent[x] <= x failed.
int64_t fshim_frontiers(const int32_t* rule, uint32_t min_size, const uint32_t* order, const ShimMap* m, uint32_t* label, uint8_t* open,
                        FrontierRecord* clusters, uint32_t cap, uint32_t* counts) {
    const QueryView Q = view_of(*m);
    const uint32_t n = (uint32_t)m->n;
    const FrontierRule F{rule[0], rule[1], (uint32_t)rule[2], (uint32_t)rule[3], (uint32_t)rule[4], rule[5], rule[6], rule[7], rule[8], rule[9]};
    using Ops = FrontierSerialOps;
    std::vector<uint32_t> parent(n), size_at(n, 0u);
    // mark
    for (uint32_t r = 0; r < n; ++r) {
        const uint32_t o = frontier_mark(Q, F, r);
        parent[r] = o != kFrontierNone ? r : kNoRow;
        open[r] = (uint8_t)o;
    }
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
        frontier_link<Ops>(Q, F, parent.data(), r, n, [&](uint32_t a, uint32_t t) { chain_ok(a); chain_ok(t); });
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
    uint32_t listed = 0, rows = 0, roots = 0;
    for (uint32_t r = 0; r < n; ++r) {
        if (parent[r] == kNoRow) continue;
        ++rows;
        if (parent[r] != r) continue;
        ++roots;
        uint32_t at = kNoRow;
        if (size_at[r] >= min_size) {
            if (listed < cap) { at = listed; clusters[listed] = frontier_record_init(r, size_at[r]); }
            ++listed;
        }
        size_at[r] = at;
    }
    counts[0] = listed; counts[1] = rows; counts[2] = roots; counts[3] = 0u;
    // reduce
    for (uint32_t r = 0; r < n; ++r) {
        if (parent[r] == kNoRow) continue;
        const uint32_t at = size_at[parent[r]];
        if (at == kNoRow) continue;
        frontier_fold<Ops>(clusters + at, frontier_term(Q, F, r, open[r]));
    }
    return 0;
}

}  // extern "C"
