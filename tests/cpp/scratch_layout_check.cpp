// Stand-alone sanitizer run of the consumers' scratch layouts (grid_ndt_amd/csrc/gndt_scratch.hpp and the layout structs next to the
// kernels): every layout at the sizes of tests/test_scratch_layout_host.py is sized over a null base, carved from a malloc of exactly
// that many bytes, and the first and the last byte of every piece and behind every member pointer are written.  A piece that is carved
// but not counted writes past the allocation.  Host code only, run on the CPU:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I grid_ndt_amd/csrc -o tests/cpp/scratch_layout_check
//       tests/cpp/scratch_layout_check.cpp && tests/cpp/scratch_layout_check
#include <cstdio>
#include <cstdlib>

#include "../scratch_layout_shim.cpp"

namespace {

constexpr uint64_t kNs[] = {0, 1, 3, 255, 256, 257, 9216, 9217, 20448, 20449};
constexpr uint64_t kBoxes[] = {0, 1, 3};
unsigned long long g_layouts = 0, g_bytes = 0;

int walk(int which, uint64_t n, uint64_t a = 0, uint64_t b = 0) {
    const void* member[scratch_layouts::kMostPieces];
    gndt::Carver sizer;
    if (scratch_layouts::run(which, n, a, b, sizer, member) < 0) return 1;
    char* const base = static_cast<char*>(std::malloc(sizer.pos ? sizer.pos : 1));
    if (!base) return 1;
    gndt::ScratchPiece log[scratch_layouts::kMostPieces];
    gndt::Carver c(base);
    c.log = log;
    const int k = scratch_layouts::run(which, n, a, b, c, member);
    int bad = c.pos != sizer.pos || c.pieces != sizer.pieces || c.pieces > (uint32_t)scratch_layouts::kMostPieces;
    for (uint32_t i = 0; i < c.pieces && !bad; ++i) {
        if (!log[i].count) continue;
        base[log[i].offset] = (char)i;
        base[log[i].offset + log[i].elem * log[i].count - 1] = (char)i;
    }
    // a member's array has at least one element wherever its piece has one: the segment pairs' second halves with n (or slots) elements
    for (int i = 0; i < k && !bad; ++i) {
        char* p = const_cast<char*>(static_cast<const char*>(member[i]));
        if (p >= base && p < base + c.pos) *p = (char)i;
        else if (p != base + c.pos) bad = 1;                 // (an empty array at the very end points one past: never written)
    }
    std::free(base);
    ++g_layouts; g_bytes += sizer.pos;
    if (bad) std::fprintf(stderr, "layout %d (%llu, %llu, %llu): sizes or members disagree\n", which, (unsigned long long)n, (unsigned long long)a, (unsigned long long)b);
    return bad;
}

}  // namespace

int main() {
    int bad = 0;
    for (const uint64_t n : kNs) {
        const uint64_t tiles = (n + 1023) / 1024;
        for (int which = 0; which < 3; ++which) bad |= walk(which, n);
        for (const uint64_t boxes : kBoxes) bad |= walk(3, n, boxes);
        bad |= walk(4, n, tiles);
        bad |= walk(5, n, gndt::seg_table_slots(n), tiles);
        bad |= walk(6, n + n / 4);
    }
    std::printf("%llu layouts carved, %llu bytes in all: %s\n", g_layouts, g_bytes, bad ? "FAILED" : "ok");
    return bad;
}
