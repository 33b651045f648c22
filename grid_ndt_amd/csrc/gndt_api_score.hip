// gndt_api_score.hip — scan scoring (gndt_score.hpp): the NDT match score of a scan against the finished grid for a batch of poses,
// and (gndt_score_derivs.hpp) that score with its gradient and Hessian with respect to a pose perturbation.
// A reader of the map like the point queries: finished_map, the map's column index, kernels on the caller's stream, nothing awaited.
#include <cmath>
#include <cstring>

#include "gndt_handle.hpp"
#include "gndt_score.hpp"
#include "gndt_score_derivs.hpp"

using namespace gndt;
using namespace gndt_host;

static_assert(sizeof(gndt_pose_score) == 32 && sizeof(ScoreRecord) == sizeof(gndt_pose_score), "k_score_reduce writes gndt_pose_score records");
static_assert(sizeof(ScorePartial) == 24, "the per-tile partial sums are 24 bytes");
static_assert(sizeof(gndt_pose_derivs) == 248 && sizeof(ScoreDerivRecord) == sizeof(gndt_pose_derivs), "k_score_derivs_finish writes gndt_pose_derivs records");
static_assert(sizeof(ScoreDerivPartial) == 240 && sizeof(ScoreDerivWaves) % 8 == 0, "the per-tile partial sums of the derivatives are 240 bytes");

namespace gndt_host {

void free_score(gndt_handle* h) {
    if (h->score.partial) (void)hipFree(h->score.partial);
    if (h->score.dpartial) (void)hipFree(h->score.dpartial);
    h->score = gndt_handle::Score{};
}

namespace {

constexpr uint32_t kMaxPoses = 65535;                      // the grid's y limit
constexpr uint64_t kPartialBytes = 64ull << 20;            // partial sums of one launch: a batch of poses is split to stay below this

// Arguments (every GNDT_ERR_INVALID of include/gndt.h but the handle's state) of a score or a derivatives call (`out`: its records;
// no per-point outputs: point_pose is not looked at); R = the parameters with the defaults filled in
int score_check_args(gndt_handle* h, const void* xyz, size_t n, size_t stride_bytes, const double* poses, uint32_t K,
                     const gndt_score_params* p, const void* out, const float* point_d2, const uint32_t* point_row, ScoreParams& R) {
    if (!p) { h->err = "gndt_score_poses: null params"; return GNDT_ERR_INVALID; }
    if (n && !xyz) { h->err = "gndt_score_poses: null points"; return GNDT_ERR_INVALID; }
    if (K && (!poses || !out)) { h->err = "gndt_score_poses: null poses or out"; return GNDT_ERR_INVALID; }
    if (K > kMaxPoses) { h->err = "gndt_score_poses: more than 65535 poses in one call"; return GNDT_ERR_INVALID; }
    if (stride_bytes != 12 && stride_bytes != 16) { h->err = "gndt_score_poses: stride_bytes must be 12 or 16"; return GNDT_ERR_INVALID; }
    if (p->neighbourhood != GNDT_SCORE_DIRECT1 && p->neighbourhood != GNDT_SCORE_DIRECT7) {
        h->err = "gndt_score_poses: unknown neighbourhood"; return GNDT_ERR_INVALID;
    }
    if ((point_d2 || point_row) && p->point_pose >= K) { h->err = "gndt_score_poses: point_pose is not one of the K poses"; return GNDT_ERR_INVALID; }
    const int32_t floor_count = std::max<int32_t>(h->P.min_points, 3);
    if (p->min_count != 0 && p->min_count < floor_count) {
        h->err = "gndt_score_poses: min_count must be 0 or at least max(min_points, 3) (smaller nodes keep zero statistics)";
        return GNDT_ERR_INVALID;
    }
    const float fl[3] = {p->cov_rel, p->cov_floor, p->max_d2};
    for (float v : fl)
        if (!std::isfinite(v) || v < 0.f) { h->err = "gndt_score_poses: cov_rel, cov_floor and max_d2 must be finite and >= 0"; return GNDT_ERR_INVALID; }
    R.min_count = (uint32_t)(p->min_count ? p->min_count : floor_count);
    R.cov_rel = (double)(p->cov_rel != 0.f ? p->cov_rel : 0.01f);
    R.cov_floor = (double)(p->cov_floor != 0.f ? p->cov_floor : 1e-6f);
    R.max_d2 = (double)p->max_d2;
    return GNDT_OK;
}

// The handle's state, in the queries' order: no capture, a finished map
int score_sync(gndt_handle* h, hipStream_t s) {
    const int rc = refuse_capture(h, s, "gndt_score_poses: a score is not recorded into a hipGraph");
    return rc ? rc : finished_map(h, "no finished build to score against", false);
}

ScoreView score_view(gndt_handle* h) {
    ScoreView S{};
    S.Q = query_view(h);
    S.count = h->out.count;
    S.cov = h->out.cov;
    return S;
}

template <int NBH>
void score_launch(const ScoreView& S, const ScoreParams& R, const float* xyz, uint32_t sf, uint64_t n, const double* poses, uint32_t kc,
                  uint32_t tiles, bool pointwise, uint32_t point_pose, ScorePartial* partial, float* point_d2, uint32_t* point_row,
                  hipStream_t s) {
    const dim3 grid(tiles, kc);
    if (pointwise)
        hipLaunchKernelGGL((k_score<NBH, true>), grid, dim3(kScoreTile), 0, s, S, R, xyz, sf, n, poses, point_pose, partial, point_d2, point_row);
    else
        hipLaunchKernelGGL((k_score<NBH, false>), grid, dim3(kScoreTile), 0, s, S, R, xyz, sf, n, poses, 0u, partial, (float*)nullptr,
                           (uint32_t*)nullptr);
}

// K >= 1 poses against n >= 1 points, everything on the device; waits for nothing.  Poses go in launches of as many as the partial
// sums' scratch takes: a pose's tiles and their order do not depend on the split.
int score_run(gndt_handle* h, const void* xyz_dev, size_t n, size_t stride_bytes, const double* poses, uint32_t K, int32_t nbh,
              const ScoreParams& R, uint32_t point_pose, gndt_pose_score* out, float* point_d2, uint32_t* point_row, hipStream_t s) {
    const uint64_t tiles64 = ((uint64_t)n + kScoreTile - 1) / kScoreTile;
    if (tiles64 > 0x7FFFFFFFull) { h->err = "gndt_score_poses: more than 2^39 points in one call"; return GNDT_ERR_INVALID; }
    const uint32_t tiles = (uint32_t)tiles64;
    const uint64_t per_pose = tiles64 * sizeof(ScorePartial);
    const uint32_t chunk = (uint32_t)std::min<uint64_t>(K, std::max<uint64_t>(1, kPartialBytes / per_pose));
    const int rc = grow_scratch(h, h->score.partial, h->score.partial_cap, per_pose * chunk);
    if (rc) return rc;
    ScorePartial* partial = static_cast<ScorePartial*>(h->score.partial);
    const ScoreView S = score_view(h);
    const float* xyz = static_cast<const float*>(xyz_dev);
    const uint32_t sf = (uint32_t)(stride_bytes / 4);
    const bool per_point = point_d2 || point_row;
    for (uint32_t k0 = 0; k0 < K; k0 += chunk) {
        const uint32_t kc = std::min(chunk, K - k0);
        const bool pw = per_point && point_pose >= k0 && point_pose < k0 + kc;
        if (nbh == GNDT_SCORE_DIRECT1)
            score_launch<kScoreDirect1>(S, R, xyz, sf, n, poses + 12 * (size_t)k0, kc, tiles, pw, point_pose - k0, partial, point_d2, point_row, s);
        else
            score_launch<kScoreDirect7>(S, R, xyz, sf, n, poses + 12 * (size_t)k0, kc, tiles, pw, point_pose - k0, partial, point_d2, point_row, s);
        HIP_TRY(h, hipGetLastError());
        hipLaunchKernelGGL(k_score_reduce, dim3(kc), dim3(kScoreReduceBlock), 0, s, partial, tiles, reinterpret_cast<ScoreRecord*>(out) + k0);
        HIP_TRY(h, hipGetLastError());
    }
    return GNDT_OK;
}

// score_run for the derivatives: k_score_derivs, the 16 waves of k_score_derivs_reduce per pose, k_score_derivs_finish.  The same
// 64 MiB bound on a launch's partial sums (the tiles' and the 16 waves'); a pose's tiles and their order do not depend on the split.
int score_derivs_run(gndt_handle* h, const void* xyz_dev, size_t n, size_t stride_bytes, const double* poses, uint32_t K, int32_t nbh,
                     const ScoreParams& R, gndt_pose_derivs* out, hipStream_t s) {
    const uint64_t tiles64 = ((uint64_t)n + kScoreTile - 1) / kScoreTile;
    if (tiles64 > 0x7FFFFFFFull) { h->err = "gndt_score_derivs: more than 2^39 points in one call"; return GNDT_ERR_INVALID; }
    const uint32_t tiles = (uint32_t)tiles64;
    const uint64_t per_pose = tiles64 * sizeof(ScoreDerivPartial);
    const uint32_t chunk = (uint32_t)std::min<uint64_t>(K, std::max<uint64_t>(1, kPartialBytes / (per_pose + sizeof(ScoreDerivWaves))));
    const uint64_t wave_bytes = (uint64_t)chunk * sizeof(ScoreDerivWaves);
    const int rc = grow_scratch(h, h->score.dpartial, h->score.dpartial_cap, wave_bytes + per_pose * chunk);
    if (rc) return rc;
    ScoreDerivWaves* waves = static_cast<ScoreDerivWaves*>(h->score.dpartial);
    ScoreDerivPartial* partial = reinterpret_cast<ScoreDerivPartial*>(static_cast<char*>(h->score.dpartial) + wave_bytes);
    const ScoreView S = score_view(h);
    const float* xyz = static_cast<const float*>(xyz_dev);
    const uint32_t sf = (uint32_t)(stride_bytes / 4);
    for (uint32_t k0 = 0; k0 < K; k0 += chunk) {
        const uint32_t kc = std::min(chunk, K - k0);
        const dim3 grid(tiles, kc);
        if (nbh == GNDT_SCORE_DIRECT1)
            hipLaunchKernelGGL((k_score_derivs<kScoreDirect1>), grid, dim3(kScoreTile), 0, s, S, R, xyz, sf, n, poses + 12 * (size_t)k0, partial);
        else
            hipLaunchKernelGGL((k_score_derivs<kScoreDirect7>), grid, dim3(kScoreTile), 0, s, S, R, xyz, sf, n, poses + 12 * (size_t)k0, partial);
        HIP_TRY(h, hipGetLastError());
        hipLaunchKernelGGL(k_score_derivs_reduce, dim3(kDerivReduceWaves, kc), dim3(64), 0, s, partial, tiles, waves);
        HIP_TRY(h, hipGetLastError());
        hipLaunchKernelGGL(k_score_derivs_finish, dim3(kc), dim3(64), 0, s, waves, reinterpret_cast<ScoreDerivRecord*>(out) + k0);
        HIP_TRY(h, hipGetLastError());
    }
    return GNDT_OK;
}

}  // namespace

}  // namespace gndt_host

extern "C" {

int gndt_score_poses_device(gndt_handle* h, const void* xyz_dev, size_t n, size_t stride_bytes, const double* poses_dev, uint32_t K,
                            const gndt_score_params* params, gndt_pose_score* out_dev, float* point_d2_dev, uint32_t* point_row_dev,
                            void* hip_stream) {
    int rc = check_ready(h);
    if (rc) return rc;
    ScoreParams R{};
    if ((rc = score_check_args(h, xyz_dev, n, stride_bytes, poses_dev, K, params, out_dev, point_d2_dev, point_row_dev, R))) return rc;
    const hipStream_t s = stream_of(h, hip_stream);
    if ((rc = score_sync(h, s)) || K == 0) return rc;
    if ((rc = use_stream(h, s))) return rc;
    if (n == 0) {
        HIP_TRY(h, hipMemsetAsync(out_dev, 0, (size_t)K * sizeof(gndt_pose_score), s));
        return GNDT_OK;
    }
    if ((rc = column_index(h, s))) return rc;
    return score_run(h, xyz_dev, n, stride_bytes, poses_dev, K, params->neighbourhood, R, params->point_pose, out_dev, point_d2_dev,
                     point_row_dev, s);
}

int gndt_score_poses(gndt_handle* h, const void* xyz_host, size_t n, size_t stride_bytes, const double* poses_host, uint32_t K,
                     const gndt_score_params* params, gndt_pose_score* out_host, float* point_d2_host, uint32_t* point_row_host) {
    int rc = check_ready(h);
    if (rc) return rc;
    ScoreParams R{};
    if ((rc = score_check_args(h, xyz_host, n, stride_bytes, poses_host, K, params, out_host, point_d2_host, point_row_host, R))) return rc;
    const hipStream_t s = h->own_stream;
    if ((rc = score_sync(h, s)) || K == 0) return rc;
    if (n == 0) {
        memset(out_host, 0, (size_t)K * sizeof(gndt_pose_score));
        return GNDT_OK;
    }
    if ((rc = use_stream(h, s)) || (rc = column_index(h, s))) return rc;
    IoPiece io[5] = {io_in(xyz_host, (uint64_t)n * stride_bytes),
                     io_in(poses_host, (uint64_t)K * 12 * sizeof(double)),
                     io_out(out_host, (uint64_t)K * sizeof(gndt_pose_score)),
                     io_out(point_d2_host, (uint64_t)n * 4),
                     io_out(point_row_host, (uint64_t)n * 4)};
    if ((rc = stage_in(h, io, s))) return rc;
    if ((rc = score_run(h, io[0].dev, n, stride_bytes, io[1].as<const double>(), K, params->neighbourhood, R, params->point_pose,
                        io[2].as<gndt_pose_score>(), io[3].as<float>(), io[4].as<uint32_t>(), s)))
        return rc;
    return stage_out(h, io, s);
}

int gndt_score_derivs_device(gndt_handle* h, const void* xyz_dev, size_t n, size_t stride_bytes, const double* poses_dev, uint32_t K,
                             const gndt_score_params* params, gndt_pose_derivs* out_dev, void* hip_stream) {
    int rc = check_ready(h);
    if (rc) return rc;
    ScoreParams R{};
    if ((rc = score_check_args(h, xyz_dev, n, stride_bytes, poses_dev, K, params, out_dev, nullptr, nullptr, R))) return rc;
    const hipStream_t s = stream_of(h, hip_stream);
    if ((rc = score_sync(h, s)) || K == 0) return rc;
    if ((rc = use_stream(h, s))) return rc;
    if (n == 0) {
        HIP_TRY(h, hipMemsetAsync(out_dev, 0, (size_t)K * sizeof(gndt_pose_derivs), s));
        return GNDT_OK;
    }
    if ((rc = column_index(h, s))) return rc;
    return score_derivs_run(h, xyz_dev, n, stride_bytes, poses_dev, K, params->neighbourhood, R, out_dev, s);
}

int gndt_score_derivs(gndt_handle* h, const void* xyz_host, size_t n, size_t stride_bytes, const double* poses_host, uint32_t K,
                      const gndt_score_params* params, gndt_pose_derivs* out_host) {
    int rc = check_ready(h);
    if (rc) return rc;
    ScoreParams R{};
    if ((rc = score_check_args(h, xyz_host, n, stride_bytes, poses_host, K, params, out_host, nullptr, nullptr, R))) return rc;
    const hipStream_t s = h->own_stream;
    if ((rc = score_sync(h, s)) || K == 0) return rc;
    if (n == 0) {
        memset(out_host, 0, (size_t)K * sizeof(gndt_pose_derivs));
        return GNDT_OK;
    }
    if ((rc = use_stream(h, s)) || (rc = column_index(h, s))) return rc;
    IoPiece io[3] = {io_in(xyz_host, (uint64_t)n * stride_bytes),
                     io_in(poses_host, (uint64_t)K * 12 * sizeof(double)),
                     io_out(out_host, (uint64_t)K * sizeof(gndt_pose_derivs))};
    if ((rc = stage_in(h, io, s))) return rc;
    if ((rc = score_derivs_run(h, io[0].dev, n, stride_bytes, io[1].as<const double>(), K, params->neighbourhood, R, io[2].as<gndt_pose_derivs>(), s)))
        return rc;
    return stage_out(h, io, s);
}

}  // extern "C"
