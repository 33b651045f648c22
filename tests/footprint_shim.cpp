// Host build of the footprint poses' per-pose code (grid_ndt_amd/csrc/gndt_footprint.hpp: foot_centre, foot_gather, the fold of the
// sums, foot_plane, foot_shape, foot_finish, the rows) for the CPU test tier, compiled with g++: one pose after another, the
// wavefront's 64 lanes run in turn and its collectives replayed in the kernel's order (FootWaveHost).  Test infrastructure only
// (tests/test_footprint_host.py, tests/test_gpu_footprint.py).
#include <stdint.h>

#include <memory>

#include "gndt_footprint.hpp"
#include "shim_map.hpp"

using namespace gndt;

static_assert(sizeof(FootInfo) == 64, "gndt_footprint_info");

extern "C" {

// robot: {radius, reachable_height, max_rough, max_angle_deg}; rule: {half_length^2, half_width^2, cos(max_angle_deg), min_cover} as
// the host forms them in fp64; frule: {max_dz, height}; urule: {min_cells (resolved), weight, n}.  poses: five floats at poses + k *
// stride.  info [K] (64 bytes each), rows [K * row_cap] (or null with 0) as gndt_footprint_poses writes them.  Returns 0.
int fshim_footprints(const float* robot, const double* rule, const float* frule, const uint32_t* urule, const ShimMap* m, const char* poses,
                     uint64_t K, uint64_t stride, uint32_t* rows, uint32_t row_cap, FootInfo* info) {
    const ScoreView S{view_of(*m), m->count, m->cov};
    const Robot R{robot[0], robot[1], robot[2], robot[3]};
    const FootRule F{rule[0], rule[1], rule[2], rule[3], frule[0], frule[1], R.reach, urule[0], urule[1], urule[2]};
    auto w = std::make_unique<FootWaveHost>();
    for (uint64_t k = 0; k < K; ++k)
        foot_pose(S, R, F, reinterpret_cast<const float*>(poses + k * stride), rows ? rows + k * row_cap : nullptr, row_cap, *w, info[k]);
    return 0;
}

}  // extern "C"
