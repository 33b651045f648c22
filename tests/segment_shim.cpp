// Host build of scan segmentation's per-element code (grid_ndt_amd/csrc/gndt_segment.hpp: seg_class, the cell table's seg_join /
// seg_find, seg_link with the frontiers' union-find, seg_term / seg_fold) for the CPU test tier, compiled with g++: the passes of the
// kernels run one item after another, in any item order the caller names, with parent[x] <= x looked at after every union.  The list
// (the ordered compaction of the roots, a scan on the device) is a plain loop here.  Test infrastructure only
// (tests/test_segment_host.py).
#include <stdint.h>

#include <vector>

#include "gndt_segment.hpp"
#include "shim_map.hpp"

using namespace gndt;

extern "C" {

uint64_t gshim_table_slots(uint64_t n) { return seg_table_slots(n); }

uint32_t gshim_z_image(float f) { return seg_z_image(f); }

uint32_t gshim_z_bits(uint32_t image) { return seg_z_bits(image); }

// score: {cov_rel, cov_floor} as the library widens them; rule: {classes, min_points, connectivity, min_cluster_points,
// min_cluster_cells} with the defaults filled in; order: the items in the order every pass takes them (null: ascending).
// point_class [n], point_label [n], clusters [cap], counts [4] as gndt_segment_scan writes them; table: {occupied slots, slots,
// longest probe walk}.  Returns 0, 1 + the index at which parent[x] <= x failed, or -1: the table had no room.
int64_t gshim_segment(int nbh, const float* xyz, uint32_t sf, uint32_t n, const double* pose, const ShimMap* m, uint32_t min_count,
                      const double* score, float novel_d2, const uint32_t* rule, const uint32_t* order, uint8_t* point_class,
                      uint32_t* point_label, SegRecord* clusters, uint32_t cap, uint32_t* counts, uint32_t* table) {
    if (nbh != kScoreDirect1 && nbh != kScoreDirect7) return -2;
    const ScoreView S{view_of(*m), m->count, m->cov};
    ScoreParams P;
    P.min_count = min_count; P.cov_rel = score[0]; P.cov_floor = score[1]; P.max_d2 = 0.0;
    const SegRule R{novel_d2, rule[0], rule[1], rule[2], rule[3], rule[4]};
    using Ops = SegSerialOps;
    const uint64_t slots = seg_table_slots(n);
    std::vector<uint64_t> key(slots, kEmptyKey);
    std::vector<uint32_t> first(slots, 0xFFFFFFFFu), count(slots, 0u);
    const SegTable T{key.data(), first.data(), count.data(), (uint32_t)(slots - 1)};
    std::vector<uint32_t> slot_root(n, 0xDEADBEEFu), parent(n, 0xDEADBEEFu), cells_at(n, 0u), points_at(n, 0u);
    std::vector<uint8_t> cls_of(n, 0xEEu);
    std::vector<uint64_t> pkey(n, kEmptyKey);
    const auto item = [&](uint32_t j) { return order ? order[j] : j; };
    // classify
    for (uint32_t j = 0; j < n; ++j) {
        const uint32_t i = item(j);
        float qx, qy, qz;
        seg_transform(pose, xyz + (size_t)i * sf, qx, qy, qz);
        QueryKey k;
        const uint32_t cls = nbh == kScoreDirect1 ? seg_class<kScoreDirect1>(S, P, R.novel_d2, qx, qy, qz, k)
                                                  : seg_class<kScoreDirect7>(S, P, R.novel_d2, qx, qy, qz, k);
        cls_of[i] = (uint8_t)cls;
        if (point_class) point_class[i] = (uint8_t)cls;
        if (seg_is_novel(R, cls)) pkey[i] = pack_key(k.sx, k.sy, k.sz);
    }
    // insert
    for (uint32_t j = 0; j < n; ++j) {
        const uint32_t i = item(j);
        slot_root[i] = kNoRow;
        if (pkey[i] == kEmptyKey) continue;
        if ((slot_root[i] = seg_join<Ops>(T, pkey[i], i)) == kNoRow) return -1;
    }
    if (table) {
        uint32_t used = 0, walk = 0;
        for (uint64_t s = 0; s < slots; ++s) {
            if (key[s] == kEmptyKey) continue;
            ++used;
            const uint32_t home = (uint32_t)mix64(key[s]) & T.mask;
            const uint32_t d = ((uint32_t)s - home) & T.mask;
            if (d > walk) walk = d;
        }
        table[0] = used; table[1] = (uint32_t)slots; table[2] = walk;
    }
    // cells
    for (uint32_t j = 0; j < n; ++j) { const uint32_t i = item(j); parent[i] = seg_parent_init(T, R, i, slot_root[i]); }
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
    for (uint32_t j = 0; j < n; ++j) {
        const uint32_t i = item(j);
        if (parent[i] == kNoRow) continue;
        seg_link<Ops>(T, R, parent.data(), i, slot_root[i], n, [&](uint32_t a, uint32_t b) { chain_ok(a); chain_ok(b); });
    }
    for (uint32_t i = 0; i < n; ++i)
        if (parent[i] != kNoRow && parent[i] > i && !bad) bad = 1 + (int64_t)i;
    if (bad) return bad;
    // flatten: labels, the roots' cells and points
    for (uint32_t j = 0; j < n; ++j) {
        const uint32_t i = item(j);
        const uint32_t slot = slot_root[i];
        const uint32_t id = seg_cell_id(T, R, slot);
        uint32_t root = kNoRow;
        if (id != kNoRow) {
            root = frontier_root<Ops>(parent.data(), id, n);
            if (id == i) { ++cells_at[root]; points_at[root] += T.count[slot]; }
        }
        slot_root[i] = root;
        if (point_label) point_label[i] = root;
    }
    for (uint32_t i = 0; i < n; ++i)                               // (the device stores the root with the label; here after every walk)
        if (parent[i] != kNoRow) parent[i] = frontier_root<Ops>(parent.data(), i, n);
    // the list: roots in index order, those that pass the size filters get the next place
    uint32_t listed = 0, novel = 0, cells = 0, roots = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (seg_is_novel(R, cls_of[i])) ++novel;
        if (parent[i] == kNoRow) continue;
        ++cells;
        if (parent[i] != i) continue;
        ++roots;
        uint32_t at = kNoRow;
        if (points_at[i] >= R.min_cluster_points && cells_at[i] >= R.min_cluster_cells) {
            if (listed < cap) { at = listed; clusters[listed] = seg_record_init(i, cells_at[i]); }
            ++listed;
        }
        points_at[i] = at;
    }
    counts[0] = listed; counts[1] = novel; counts[2] = cells; counts[3] = roots;
    // reduce
    for (uint32_t j = 0; j < n; ++j) {
        const uint32_t i = item(j);
        if (slot_root[i] == kNoRow) continue;
        const uint32_t at = points_at[slot_root[i]];
        if (at == kNoRow) continue;
        float qx, qy, qz;
        seg_transform(pose, xyz + (size_t)i * sf, qx, qy, qz);
        seg_fold<Ops>(clusters + at, seg_term(query_key<kQueryNode>(S.Q, qx, qy, qz), qx, qy, qz, cls_of[i]));
    }
    for (uint32_t j = 0; j < (listed < cap ? listed : cap); ++j) seg_record_finish(clusters + j);
    return 0;
}

}  // extern "C"
