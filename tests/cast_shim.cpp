// Host build of ray casting's per-ray code for the CPU test tier, compiled with g++ (tests/test_cast_host.py through
// host_emulation.load_shim): the walk of one ray from its own origin with every step's crossing parameter (gndt_ray.hpp ray_begin /
// ray_next), and cast_one over n rays as k_cast's lanes run it, one ray after another, with the kernel's tallies.  Test
// infrastructure only.
#include <stdint.h>

#include "gndt_cast.hpp"
#include "shim_map.hpp"

using namespace gndt;

namespace {

RayGrid grid_of(const float* map_origin, float grid_len, float z_len, float max_range) {
    RayGrid G{};
    G.ox = map_origin[0]; G.oy = map_origin[1]; G.oz = map_origin[2]; G.grid_len = grid_len; G.z_len = z_len;
    G.max_range = max_range; G.end_margin = 0.f;
    return G;
}

}  // namespace

extern "C" {

// The columns of one ray's walk: (sx, sy, lev_in, lev_out) per column into cols and (t_in, t_out) into ts, at most cap columns.
// -> columns, -1 when the ray is skipped.
int castshim_walk(const float* map_origin, float grid_len, float z_len, const float* o, const float* p, float max_range, int32_t* cols,
                  double* ts, int32_t cap) {
    const RayGrid G = grid_of(map_origin, grid_len, z_len, max_range);
    RayWalk w;
    if (!ray_begin(G, o[0], o[1], o[2], p[0], p[1], p[2], w)) return -1;
    RayColumn c;
    RayCross x;
    double t_in = 0.0;
    int k = 0;
    while (ray_next(G, w, c, x)) {
        if (k < cap) {
            cols[4 * k] = c.sx; cols[4 * k + 1] = c.sy; cols[4 * k + 2] = x.lev_in; cols[4 * k + 3] = x.lev_out;
            ts[2 * k] = t_in; ts[2 * k + 1] = x.t;
        }
        t_in = x.t;
        ++k;
    }
    return k;
}

// n rays (so floats between origins, 0 = one origin; se floats between ends) against the rows and the column index (consumer_shim's
// build_index); the parameters with the defaults filled in; stats = {rays, skipped, hits}
int castshim_cast(int mode, const float* origins, uint32_t so, const float* ends, uint32_t se, uint64_t n, const ShimMap* m, uint32_t min_count,
                  float max_range, double min_range, double cov_rel, double cov_floor, double max_d2, uint32_t* row, float* range, float* d2,
                  uint64_t* stats) {
    if (mode != kCastVoxel && mode != kCastNdt) return 1;
    const ScoreView S{view_of(*m), m->count, m->cov};
    const RayGrid G = grid_of(m->origin, m->grid_len, m->z_len, max_range);
    CastParams P;
    P.min_count = min_count; P.min_range = min_range; P.cov_rel = cov_rel; P.cov_floor = cov_floor; P.max_d2 = max_d2;
    const CastOut o{row, range, d2};
    stats[0] = stats[1] = stats[2] = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const int rc = mode == kCastVoxel ? cast_one<kCastVoxel>(S, P, G, origins, so, ends, se, i, o)
                                          : cast_one<kCastNdt>(S, P, G, origins, so, ends, se, i, o);
        if (rc == kCastSkipped) ++stats[1]; else ++stats[0];
        if (rc == kCastHit) ++stats[2];
    }
    return 0;
}

}  // extern "C"
