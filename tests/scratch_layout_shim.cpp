// Host build of the consumers' scratch layouts (grid_ndt_amd/csrc/gndt_scratch.hpp's Carver and the layout structs next to the kernels)
// for the CPU test tier, compiled with g++: every layout carved over a fake base that is never dereferenced, its pieces and its members
// reported as offsets.  Test infrastructure only (tests/test_scratch_layout_host.py; tests/cpp/scratch_layout_check.cpp includes this file
// for the sanitizer run).
#include <stdint.h>

#define GNDT_SCRATCH_LOG 1      // gndt_scratch.hpp: the carver notes every piece it hands out (this build only)
#include "gndt_obstacle.hpp"
#include "gndt_route_field.hpp"
#include "gndt_segment.hpp"
#include "gndt_walk.hpp"

namespace scratch_layouts {

constexpr int kLayouts = 7, kMostPieces = 16;

template <typename... P>
int put(const void** member, P*... p) {
    int k = 0;
    ((member[k++] = p), ...);
    return k;
}

// Layout `which` of sizes (n, a, b) carved from c: 0 clearance (n), 1 route field (n), 2 walk (n), 3 obstacle (n, a = n_boxes),
// 4 frontier (n, a = tiles), 5 segment (n, a = slots, b = tiles), 6 the obstacle field's marks (n = rows).  member[k]: the layout's
// k-th pointer in declaration order, the derived ones included.  Returns how many, -1 for an unknown layout.
inline int run(int which, uint64_t n, uint64_t a, uint64_t b, gndt::Carver& c, const void** member) {
    using namespace gndt;
    switch (which) {
    case 0: { ClearanceScratch S(c, n); return put(member, S.step, S.key[0], S.key[1], S.flags, S.tall); }
    case 1: { RouteScratch S(c, n); return put(member, S.first, S.rest, S.key, S.flags, S.w, S.more); }
    case 2: { WalkScratch S(c, n); return put(member, S.step, S.key0, S.flag, S.tall); }
    case 3: { ObstacleScratch S(c, n, a); return put(member, S.hdr, S.W, S.key[0], S.key[1], S.step, S.flags, S.covers, S.list, S.tall); }
    case 4: { FrontierScratch S(c, n, a); return put(member, S.parent, S.size_at, S.tile_cnt, S.open, S.slack); }
    case 5: { SegmentScratch S(c, n, a, b);
              return put(member, S.T.key, S.T.first, S.T.count, S.slot_root, S.parent, S.cells_at, S.points_at, S.tile_cnt, S.cls_of, S.slack); }
    case 6: { ObstacleMarks M{}; obstacle_carve_marks(c, n, M); return put(member, M.cover, M.cstamp, M.slot); }
    default: return -1;
    }
}

}  // namespace scratch_layouts

extern "C" {

uint64_t slshim_seg_slots(uint64_t n) { return gndt::seg_table_slots(n); }
uint32_t slshim_flag_words(int route) { return (uint32_t)(route ? gndt::kRouteFlagWords : gndt::kClrFlagWords); }

// pieces [16][4]: offset, element size, element alignment, count of every piece in the order taken; members [16]: offset of every
// pointer of the layout (scratch_layouts::run's order); counts [2]: how many of each; total: the bytes.  sizing != 0: over a null base
// (then every member must be null: members[k] = 0, and the total is what carve_scratch allocates).  Returns 0, -1: unknown layout.
int slshim_layout(int which, uint64_t n, uint64_t a, uint64_t b, int sizing, uint64_t* pieces, uint64_t* members, uint32_t* counts, uint64_t* total) {
    char* const base = sizing ? nullptr : reinterpret_cast<char*>(uintptr_t(1) << 40);      // a multiple of 256
    gndt::ScratchPiece log[scratch_layouts::kMostPieces];
    gndt::Carver c(base);
    c.log = log;
    const void* member[scratch_layouts::kMostPieces];
    const int k = scratch_layouts::run(which, n, a, b, c, member);
    if (k < 0 || c.pieces > (uint32_t)scratch_layouts::kMostPieces) return -1;
    for (uint32_t i = 0; i < c.pieces; ++i) {
        pieces[4 * i + 0] = log[i].offset; pieces[4 * i + 1] = log[i].elem; pieces[4 * i + 2] = log[i].align; pieces[4 * i + 3] = log[i].count;
    }
    for (int i = 0; i < k; ++i) members[i] = sizing ? (uint64_t)(uintptr_t)member[i] : (uint64_t)(static_cast<const char*>(member[i]) - base);
    counts[0] = c.pieces; counts[1] = (uint32_t)k;
    *total = c.pos;
    return 0;
}

}  // extern "C"
