// gndt_api_score_maps.hip — map-to-map scoring (gndt_score_maps.hpp): the distribution-to-distribution NDT score of one map's nodes
// against another map for a batch of poses, and that score with its gradient and Hessian.
// Two readers' worth of gndt_api_score.hip: both maps finished, the destination's column index, kernels on the caller's stream,
// nothing awaited.  The partial sums live in the destination's scoring scratch (the records are the score's own).
#include <cmath>

#include "gndt_handle.hpp"
#include "gndt_score_maps.hpp"

using namespace gndt;
using namespace gndt_host;

static_assert(sizeof(ScoreRecord) == sizeof(gndt_pose_score) && sizeof(ScoreDerivRecord) == sizeof(gndt_pose_derivs),
              "the score's reduce kernels write the records of include/gndt.h");

namespace gndt_host {

namespace {

constexpr uint32_t kMaxPoses = 65535;                      // the grid's y limit
constexpr uint64_t kPartialBytes = 64ull << 20;            // partial sums of one launch: a batch of poses is split to stay below this

// GNDT_ERR_INVALID on both handles (the caller may ask either for the text)
int maps_refuse(gndt_handle* dst, gndt_handle* src, const std::string& msg) {
    src->err = msg;
    dst->err = msg;
    return GNDT_ERR_INVALID;
}

// Every GNDT_ERR_INVALID of include/gndt.h "map-to-map scoring" but the handles' state; R = the parameters with the defaults filled in
int maps_check_args(gndt_handle* dst, gndt_handle* src, const double* poses, uint32_t K, const gndt_score_params* p, const void* out,
                    bool per_node, ScoreParams& R) {
    if (src->device != dst->device) return maps_refuse(dst, src, "gndt_score_maps: the two handles are on different devices");
    if (!p) return maps_refuse(dst, src, "gndt_score_maps: null params");
    if (K && (!poses || !out)) return maps_refuse(dst, src, "gndt_score_maps: null poses or out");
    if (K > kMaxPoses) return maps_refuse(dst, src, "gndt_score_maps: more than 65535 poses in one call");
    if (p->neighbourhood != GNDT_SCORE_DIRECT1 && p->neighbourhood != GNDT_SCORE_DIRECT7)
        return maps_refuse(dst, src, "gndt_score_maps: unknown neighbourhood");
    if (per_node && p->point_pose >= K) return maps_refuse(dst, src, "gndt_score_maps: node_pose is not one of the K poses");
    const int32_t floor_count = std::max<int32_t>(std::max<int32_t>(dst->P.min_points, src->P.min_points), 3);
    if (p->min_count != 0 && p->min_count < floor_count)
        return maps_refuse(dst, src, "gndt_score_maps: min_count must be 0 or at least max(both min_points, 3) (smaller nodes keep zero statistics)");
    const float fl[3] = {p->cov_rel, p->cov_floor, p->max_d2};
    for (float v : fl)
        if (!std::isfinite(v) || v < 0.f) return maps_refuse(dst, src, "gndt_score_maps: cov_rel, cov_floor and max_d2 must be finite and >= 0");
    R.min_count = (uint32_t)(p->min_count ? p->min_count : floor_count);
    R.cov_rel = (double)(p->cov_rel != 0.f ? p->cov_rel : 0.01f);
    R.cov_floor = (double)(p->cov_floor != 0.f ? p->cov_floor : 1e-6f);
    R.max_d2 = (double)p->max_d2;
    return GNDT_OK;
}

// The handles' state, in the score's order: no capture, both maps finished (what gndt_sync finishes on either comes first), then the
// stream — the source's later work waits for it too — and the destination's column index.  *go: there is something to launch.
int maps_prepare(gndt_handle* dst, gndt_handle* src, uint32_t K, void* hip_stream, hipStream_t* s, bool* go) {
    *go = false;
    int rc = check_ready(dst);
    if (rc) return rc;
    if (src != dst && (rc = check_ready(src))) { dst->err = src->err; return rc; }
    *s = stream_of(dst, hip_stream);
    if ((rc = refuse_capture(dst, *s, "gndt_score_maps: a score is not recorded into a hipGraph"))) { src->err = dst->err; return rc; }
    if ((rc = finished_map(dst, "no finished build to score against", false))) { src->err = dst->err; return rc; }
    if (src != dst && (rc = finished_map(src, "no finished build to score", false))) { dst->err = src->err; return rc; }
    if (K == 0) return GNDT_OK;
    if ((rc = use_stream(dst, *s))) return rc;
    if (src != dst && (rc = use_stream(src, *s))) { dst->err = src->err; return rc; }
    *go = true;
    return GNDT_OK;
}

ScoreView maps_view(gndt_handle* h) {
    ScoreView S{};
    S.Q = query_view(h);
    S.count = h->out.count;
    S.cov = h->out.cov;
    return S;
}

MapsSource maps_source(gndt_handle* h) {
    MapsSource M{};
    M.count = h->out.count; M.mean = h->out.mean; M.cov = h->out.cov; M.flags = h->out.flags;
    return M;
}

template <int NBH>
void maps_launch(const ScoreView& D, const ScoreParams& R, const MapsSource& M, uint64_t n, const double* poses, uint32_t kc, uint32_t tiles,
                 bool nodewise, uint32_t node_pose, ScorePartial* partial, float* node_d2, uint32_t* node_row, hipStream_t s) {
    const dim3 grid(tiles, kc);
    if (nodewise)
        hipLaunchKernelGGL((k_score_maps<NBH, true>), grid, dim3(kScoreTile), 0, s, D, R, M, n, poses, node_pose, partial, node_d2, node_row);
    else
        hipLaunchKernelGGL((k_score_maps<NBH, false>), grid, dim3(kScoreTile), 0, s, D, R, M, n, poses, 0u, partial, (float*)nullptr,
                           (uint32_t*)nullptr);
}

// K >= 1 poses, n >= 1 source rows; waits for nothing.  Poses go in launches of as many as the partial sums' scratch takes: a
// pose's tiles and their order do not depend on the split.
int maps_run(gndt_handle* dst, gndt_handle* src, uint64_t n, const double* poses, uint32_t K, int32_t nbh, const ScoreParams& R,
             uint32_t node_pose, gndt_pose_score* out, float* node_d2, uint32_t* node_row, hipStream_t s) {
    const uint64_t tiles64 = (n + kScoreTile - 1) / kScoreTile;
    const uint32_t tiles = (uint32_t)tiles64;              // (rows are 32-bit: below 2^24 tiles)
    const uint64_t per_pose = tiles64 * sizeof(ScorePartial);
    const uint32_t chunk = (uint32_t)std::min<uint64_t>(K, std::max<uint64_t>(1, kPartialBytes / per_pose));
    const int rc = grow_scratch(dst, dst->score.partial, dst->score.partial_cap, per_pose * chunk);
    if (rc) return rc;
    ScorePartial* partial = static_cast<ScorePartial*>(dst->score.partial);
    const ScoreView D = maps_view(dst);
    const MapsSource M = maps_source(src);
    const bool per_node = node_d2 || node_row;
    for (uint32_t k0 = 0; k0 < K; k0 += chunk) {
        const uint32_t kc = std::min(chunk, K - k0);
        const bool nw = per_node && node_pose >= k0 && node_pose < k0 + kc;
        if (nbh == GNDT_SCORE_DIRECT1)
            maps_launch<kScoreDirect1>(D, R, M, n, poses + 12 * (size_t)k0, kc, tiles, nw, node_pose - k0, partial, node_d2, node_row, s);
        else
            maps_launch<kScoreDirect7>(D, R, M, n, poses + 12 * (size_t)k0, kc, tiles, nw, node_pose - k0, partial, node_d2, node_row, s);
        HIP_TRY(dst, hipGetLastError());
        hipLaunchKernelGGL(k_score_reduce, dim3(kc), dim3(kScoreReduceBlock), 0, s, partial, tiles, reinterpret_cast<ScoreRecord*>(out) + k0);
        HIP_TRY(dst, hipGetLastError());
    }
    return GNDT_OK;
}

// maps_run for the derivatives: k_score_maps_derivs, then the score derivatives' own two reduce kernels; the same 64 MiB bound
int maps_derivs_run(gndt_handle* dst, gndt_handle* src, uint64_t n, const double* poses, uint32_t K, int32_t nbh, const ScoreParams& R,
                    gndt_pose_derivs* out, hipStream_t s) {
    const uint64_t tiles64 = (n + kScoreTile - 1) / kScoreTile;
    const uint32_t tiles = (uint32_t)tiles64;
    const uint64_t per_pose = tiles64 * sizeof(ScoreDerivPartial);
    const uint32_t chunk = (uint32_t)std::min<uint64_t>(K, std::max<uint64_t>(1, kPartialBytes / (per_pose + sizeof(ScoreDerivWaves))));
    const uint64_t wave_bytes = (uint64_t)chunk * sizeof(ScoreDerivWaves);
    const int rc = grow_scratch(dst, dst->score.dpartial, dst->score.dpartial_cap, wave_bytes + per_pose * chunk);
    if (rc) return rc;
    ScoreDerivWaves* waves = static_cast<ScoreDerivWaves*>(dst->score.dpartial);
    ScoreDerivPartial* partial = reinterpret_cast<ScoreDerivPartial*>(static_cast<char*>(dst->score.dpartial) + wave_bytes);
    const ScoreView D = maps_view(dst);
    const MapsSource M = maps_source(src);
    for (uint32_t k0 = 0; k0 < K; k0 += chunk) {
        const uint32_t kc = std::min(chunk, K - k0);
        const dim3 grid(tiles, kc);
        if (nbh == GNDT_SCORE_DIRECT1)
            hipLaunchKernelGGL((k_score_maps_derivs<kScoreDirect1>), grid, dim3(kScoreTile), 0, s, D, R, M, n, poses + 12 * (size_t)k0, partial);
        else
            hipLaunchKernelGGL((k_score_maps_derivs<kScoreDirect7>), grid, dim3(kScoreTile), 0, s, D, R, M, n, poses + 12 * (size_t)k0, partial);
        HIP_TRY(dst, hipGetLastError());
        hipLaunchKernelGGL(k_score_derivs_reduce, dim3(kDerivReduceWaves, kc), dim3(64), 0, s, partial, tiles, waves);
        HIP_TRY(dst, hipGetLastError());
        hipLaunchKernelGGL(k_score_derivs_finish, dim3(kc), dim3(64), 0, s, waves, reinterpret_cast<ScoreDerivRecord*>(out) + k0);
        HIP_TRY(dst, hipGetLastError());
    }
    return GNDT_OK;
}

}  // namespace

}  // namespace gndt_host

extern "C" {

int gndt_score_maps_device(gndt_handle* dst, gndt_handle* src, const double* poses_dev, uint32_t K, const gndt_score_params* params,
                           gndt_pose_score* out_dev, float* node_d2_dev, uint32_t* node_row_dev, void* hip_stream) {
    if (!dst || !src) return GNDT_ERR_INVALID;
    ScoreParams R{};
    int rc = maps_check_args(dst, src, poses_dev, K, params, out_dev, node_d2_dev || node_row_dev, R);
    if (rc) return rc;
    hipStream_t s;
    bool go;
    if ((rc = maps_prepare(dst, src, K, hip_stream, &s, &go)) || !go) return rc;
    const uint64_t n = src->res_nodes;
    if (n == 0) {
        HIP_TRY(dst, hipMemsetAsync(out_dev, 0, (size_t)K * sizeof(gndt_pose_score), s));
        return GNDT_OK;
    }
    if ((rc = column_index(dst, s))) return rc;
    return maps_run(dst, src, n, poses_dev, K, params->neighbourhood, R, params->point_pose, out_dev, node_d2_dev, node_row_dev, s);
}

int gndt_score_maps_derivs_device(gndt_handle* dst, gndt_handle* src, const double* poses_dev, uint32_t K, const gndt_score_params* params,
                                  gndt_pose_derivs* out_dev, void* hip_stream) {
    if (!dst || !src) return GNDT_ERR_INVALID;
    ScoreParams R{};
    int rc = maps_check_args(dst, src, poses_dev, K, params, out_dev, false, R);
    if (rc) return rc;
    hipStream_t s;
    bool go;
    if ((rc = maps_prepare(dst, src, K, hip_stream, &s, &go)) || !go) return rc;
    const uint64_t n = src->res_nodes;
    if (n == 0) {
        HIP_TRY(dst, hipMemsetAsync(out_dev, 0, (size_t)K * sizeof(gndt_pose_derivs), s));
        return GNDT_OK;
    }
    if ((rc = column_index(dst, s))) return rc;
    return maps_derivs_run(dst, src, n, poses_dev, K, params->neighbourhood, R, out_dev, s);
}

}  // extern "C"
