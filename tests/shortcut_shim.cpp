// Host build of route shortcutting's per-route code (grid_ndt_amd/csrc/gndt_shortcut.hpp: shortcut_link, the group choice, the sums,
// shortcut_route) for the CPU test tier, compiled with g++: one route after another, the wavefront's collectives run lane after lane
// (ShortcutWaveHost).  Test infrastructure only (tests/test_shortcut_host.py).
#include <stdint.h>

#include "gndt_shortcut.hpp"
#include "shim_map.hpp"

using namespace gndt;

static_assert(sizeof(ShortcutInfo) == 48, "gndt_shortcut_info");

extern "C" {

// robot: {radius, reachable_height, max_rough, max_angle_deg}; rule: {window, checks, min_hops, max_links} (resolved).
// lengths: the uint32 at lengths + k * length_stride.  info [K] (48 bytes each), wp [K * wp_cap], path [K * path_cap] (or null with 0) as
// gndt_shortcut_routes writes them.  Returns 0.
int sshim_shortcut(const float* robot, const uint32_t* rule, const ShimMap* m, const uint32_t* hops, const uint32_t* routes, uint64_t K,
                   uint32_t route_cap, const char* lengths, uint64_t length_stride, uint32_t* wp, uint32_t wp_cap, uint32_t* path,
                   uint32_t path_cap, ShortcutInfo* info) {
    const QueryView Q = view_of(*m);
    const uint32_t n = (uint32_t)m->n;
    const Robot R{robot[0], robot[1], robot[2], robot[3]};
    const ShortcutRule P{rule[0], rule[3], WalkRule{kQueryNearestSlope, rule[1], rule[2], kWalkDefaultSteps}};
    for (uint64_t k = 0; k < K; ++k)
        shortcut_route<ShortcutWaveHost>(Q, R, P, hops, n, routes + k * route_cap, *reinterpret_cast<const uint32_t*>(lengths + k * length_stride),
                                         route_cap, wp + k * wp_cap, wp_cap, path ? path + k * path_cap : nullptr, path_cap, info[k]);
    return 0;
}

// One link on its own: 1 if Link(a, b) holds.
int sshim_link(const float* robot, const uint32_t* rule, const ShimMap* m, const uint32_t* hops, uint32_t a, uint32_t b) {
    const QueryView Q = view_of(*m);
    const uint32_t n = (uint32_t)m->n;
    const Robot R{robot[0], robot[1], robot[2], robot[3]};
    const ShortcutRule P{rule[0], rule[3], WalkRule{kQueryNearestSlope, rule[1], rule[2], kWalkDefaultSteps}};
    return shortcut_link<false>(Q, R, P, hops, n, a, b, nullptr) ? 1 : 0;
}

}  // extern "C"
