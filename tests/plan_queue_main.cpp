// plan_queue_main.cpp — a stand-alone host program (its own main; built with -fsanitize=address,undefined by tests/test_plan_host.py
// and run as a subprocess, never loaded into Python, never on a GPU) that drives gndt_plan.hpp's open queue through a scene with a
// small first tier, so that the spill tier, the compaction at a full queue and the overflow guard all run under the sanitizers.
//
//   plan_queue_main <scene file>
// The scene file (written by the test): 8 uint64 {rows, table slots, starts, goal row, demand, 0, 0, 0}, 8 floats {origin xyz, grid_len,
// z_len, slope_interval, 0, 0}, 4 floats robot, then the arrays sx sy sz (i32) mean normal (3 f32) rough (f32) flags row_ncol (u32)
// ctab_key (u64) ctab_val (u32) h_bits (u32) starts (3 f32 each).
// Prints "same <queries>" when a 64-entry first tier (with the default spill, and with a spill just above the peak, which compacts at
// a full queue) gives the bytes of the 1024-entry tier, then "limit <n>" for a queue of 128 entries in all, and exits 0.
#include <cstdio>
#include <cstdlib>

#include "plan_shim.cpp"

namespace {
template <typename T>
std::vector<T> take(FILE* f, size_t count) {
    std::vector<T> v(count ? count : 1);
    if (count && std::fread(v.data(), sizeof(T), count, f) != count) { std::fprintf(stderr, "short scene file\n"); std::exit(2); }
    return v;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: plan_queue_main <scene file>\n"); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    const auto head = take<uint64_t>(f, 8);
    const auto fl = take<float>(f, 8);
    const auto robot = take<float>(f, 4);
    const uint64_t n = head[0], tsize = head[1], K = head[2];
    const auto sx = take<int32_t>(f, n), sy = take<int32_t>(f, n), sz = take<int32_t>(f, n);
    const auto mean = take<float>(f, 3 * n), normal = take<float>(f, 3 * n), rough = take<float>(f, n);
    const auto flags = take<uint32_t>(f, n), row_ncol = take<uint32_t>(f, n);
    const auto ctab_key = take<uint64_t>(f, tsize);
    const auto ctab_val = take<uint32_t>(f, tsize), h_bits = take<uint32_t>(f, n);
    const auto starts = take<float>(f, 3 * K);
    std::fclose(f);
    ShimMap m{};
    m.n = n;
    m.sx = sx.data(); m.sy = sy.data(); m.sz = sz.data(); m.mean = mean.data(); m.normal = normal.data(); m.rough = rough.data();
    m.flags = flags.data(); m.row_ncol = row_ncol.data();
    m.ctab_key = ctab_key.data(); m.ctab_val = ctab_val.data(); m.ctab_size = (uint32_t)tsize;
    m.h_bits = h_bits.data();
    m.origin[0] = fl[0]; m.origin[1] = fl[1]; m.origin[2] = fl[2]; m.grid_len = fl[3]; m.z_len = fl[4]; m.slope_interval = fl[5];
    m.demand_true = (int32_t)head[4];
    const uint32_t cap = (uint32_t)n;
    auto run = [&](uint32_t lds, uint32_t entries, std::vector<uint32_t>& route, std::vector<RouteInfo>& info) {
        route.assign((size_t)K * cap + 1, 0xDEADBEEFu);
        info.assign(K + 1, RouteInfo{});
        return planshim_routes(&m, robot.data(), (uint32_t)head[3], kQueryNode, starts.data(), 3u, K, 0u, lds, entries, route.data(), cap,
                               info.data(), nullptr);
    };
    std::vector<uint32_t> r0, r1;
    std::vector<RouteInfo> i0, i1;
    if (run(1024u, 0u, r0, i0)) return 1;
    uint32_t peak = 0;
    for (uint64_t k = 0; k < K; ++k) peak = i0[k].queue_peak > peak ? i0[k].queue_peak : peak;
    const uint32_t tight = peak + 1u;
    for (uint32_t entries : {0u, tight}) {
        if (run(64u, entries, r1, i1)) return 1;
        if (r0 != r1 || std::memcmp(i0.data(), i1.data(), K * sizeof(RouteInfo)) != 0) {
            std::printf("a 64-entry first tier (queue of %u entries) changed the answers\n", entries);
            return 1;
        }
    }
    std::printf("same %llu peak %u\n", (unsigned long long)K, peak);
    if (run(64u, 128u, r1, i1)) return 1;
    uint64_t limit = 0;
    for (uint64_t k = 0; k < K; ++k) {
        if (i1[k].status == kRouteLimit) { ++limit; continue; }
        if (std::memcmp(&i0[k], &i1[k], sizeof(RouteInfo)) != 0) { std::printf("query %llu differs under a 128-entry queue\n", (unsigned long long)k); return 1; }
    }
    std::printf("limit %llu\n", (unsigned long long)limit);
    return 0;
}
