// gndt_api_cast.hip — ray casting (gndt_cast.hpp): the first map node along each ray of a batch, its row, range and d2.
// A reader of the map like the point queries: finished_map, the map's column index, one kernel on the caller's stream, nothing awaited
// unless the counters are asked for.
#include <cmath>

#include "gndt_handle.hpp"
#include "gndt_cast.hpp"

using namespace gndt;
using namespace gndt_host;

static_assert(sizeof(gndt_cast_params) == 32 && sizeof(gndt_cast_stats) == 24, "the ABI of include/gndt.h \"ray casting\"");

namespace gndt_host {

void free_cast(gndt_handle* h) {
    if (h->cast.d_stats) (void)hipFree(h->cast.d_stats);
    if (h->cast.h_stats) (void)hipHostFree(h->cast.h_stats);
    h->cast = gndt_handle::Cast{};
}

namespace {

constexpr uint64_t kMaxRays = 0x7FFFFFFFull;

// Arguments (every GNDT_ERR_INVALID of include/gndt.h but the handle's state); R = the parameters with the defaults filled in
int cast_check_args(gndt_handle* h, const void* origins, size_t origin_stride, const void* ends, size_t n, size_t end_stride,
                    const gndt_cast_params* p, const gndt_cast_out* out, CastParams& R) {
    if (!p || !out) { h->err = "gndt_cast_rays: null params or out"; return GNDT_ERR_INVALID; }
    if (!out->row && !out->range && !out->d2) { h->err = "gndt_cast_rays: no output asked for"; return GNDT_ERR_INVALID; }
    if (n && (!origins || !ends)) { h->err = "gndt_cast_rays: null origins or ends"; return GNDT_ERR_INVALID; }
    if (n > kMaxRays) { h->err = "gndt_cast_rays: more than 2^31 - 1 rays in one call"; return GNDT_ERR_INVALID; }
    if (origin_stride != 0 && origin_stride != 12 && origin_stride != 16) {
        h->err = "gndt_cast_rays: origin_stride_bytes must be 0, 12 or 16"; return GNDT_ERR_INVALID;
    }
    if (end_stride != 12 && end_stride != 16) { h->err = "gndt_cast_rays: end_stride_bytes must be 12 or 16"; return GNDT_ERR_INVALID; }
    if (p->mode != GNDT_CAST_VOXEL && p->mode != GNDT_CAST_NDT) { h->err = "gndt_cast_rays: unknown mode"; return GNDT_ERR_INVALID; }
    if (p->reserved != 0u) { h->err = "gndt_cast_rays: reserved must be 0"; return GNDT_ERR_INVALID; }
    const float fl[5] = {p->max_range, p->min_range, p->cov_rel, p->cov_floor, p->max_d2};
    for (float v : fl)
        if (!std::isfinite(v) || v < 0.f) {
            h->err = "gndt_cast_rays: max_range, min_range, cov_rel, cov_floor and max_d2 must be finite and >= 0"; return GNDT_ERR_INVALID;
        }
    if (p->mode == GNDT_CAST_VOXEL) {
        if (p->min_count < 0) { h->err = "gndt_cast_rays: min_count must be >= 0"; return GNDT_ERR_INVALID; }
        R.min_count = (uint32_t)(p->min_count ? p->min_count : 1);
    } else {
        const int32_t floor_count = std::max<int32_t>(h->P.min_points, 3);
        if (p->min_count != 0 && p->min_count < floor_count) {
            h->err = "gndt_cast_rays: in NDT mode min_count must be 0 or at least max(min_points, 3) (smaller nodes keep zero statistics)";
            return GNDT_ERR_INVALID;
        }
        R.min_count = (uint32_t)(p->min_count ? p->min_count : floor_count);
    }
    R.min_range = (double)p->min_range;
    R.cov_rel = (double)(p->cov_rel != 0.f ? p->cov_rel : 0.01f);
    R.cov_floor = (double)(p->cov_floor != 0.f ? p->cov_floor : 1e-6f);
    R.max_d2 = (double)p->max_d2;
    return GNDT_OK;
}

// The handle's state, in the queries' order: no capture, a finished map
int cast_sync(gndt_handle* h, hipStream_t s) {
    const int rc = refuse_capture(h, s, "gndt_cast_rays: a cast is not recorded into a hipGraph");
    return rc ? rc : finished_map(h, "no finished build to cast rays into", false);
}

void zero_stats(gndt_cast_stats* stats) {
    if (stats) { stats->rays = 0; stats->skipped = 0; stats->hits = 0; }
}

template <int MODE>
void cast_kernel(bool tally, int blocks, hipStream_t s, const ScoreView& S, const CastParams& R, const RayGrid& G, const float* origins,
                 uint32_t so, const float* ends, uint32_t se, uint64_t n, const CastOut& o, unsigned long long* d_stats) {
    if (tally) hipLaunchKernelGGL((k_cast<MODE, true>), dim3(blocks), dim3(256), 0, s, S, R, G, origins, so, ends, se, n, o, d_stats);
    else hipLaunchKernelGGL((k_cast<MODE, false>), dim3(blocks), dim3(256), 0, s, S, R, G, origins, so, ends, se, n, o, (unsigned long long*)nullptr);
}

// The kernel on the current map, everything on the device.  Waits for nothing.  tally: the counters are cleared before, counted by the
// kernel and copied to the pinned mirror behind it; without it the launch is the call's only stream operation.
int cast_launch(gndt_handle* h, const float* origins, uint32_t so, const float* ends, uint32_t se, uint64_t n, const gndt_cast_params* p,
                const CastParams& R, const CastOut& o, bool tally, hipStream_t s) {
    auto& c = h->cast;
    if (tally) {
        if (!c.d_stats) HIP_TRY(h, hipMalloc(&c.d_stats, 3 * sizeof(unsigned long long)));
        if (!c.h_stats) HIP_TRY(h, hipHostMalloc(&c.h_stats, 3 * sizeof(unsigned long long)));
        HIP_TRY(h, hipMemsetAsync(c.d_stats, 0, 3 * sizeof(unsigned long long), s));
    }
    ScoreView S{};
    S.Q = query_view(h);
    S.count = h->out.count;
    S.cov = h->out.cov;
    RayGrid G{};
    G.ox = h->origin[0]; G.oy = h->origin[1]; G.oz = h->origin[2]; G.grid_len = h->P.grid_len; G.z_len = h->P.z_len;
    G.max_range = p->max_range; G.end_margin = 0.f;
    const int blocks = grid_for(n, 256, 2048);
    if (p->mode == GNDT_CAST_VOXEL) cast_kernel<kCastVoxel>(tally, blocks, s, S, R, G, origins, so, ends, se, n, o, c.d_stats);
    else cast_kernel<kCastNdt>(tally, blocks, s, S, R, G, origins, so, ends, se, n, o, c.d_stats);
    HIP_TRY(h, hipGetLastError());
    if (tally) HIP_TRY(h, hipMemcpyAsync(c.h_stats, c.d_stats, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    return GNDT_OK;
}

void cast_stats_out(const gndt_handle* h, gndt_cast_stats* stats) {
    if (!stats) return;
    const unsigned long long* v = h->cast.h_stats;
    stats->rays = v[0]; stats->skipped = v[1]; stats->hits = v[2];
}

}  // namespace

}  // namespace gndt_host

extern "C" {

int gndt_cast_rays_device(gndt_handle* h, const void* origins_dev, size_t origin_stride_bytes, const void* ends_dev, size_t n,
                          size_t end_stride_bytes, const gndt_cast_params* params, const gndt_cast_out* out_dev, gndt_cast_stats* stats,
                          void* hip_stream) {
    int rc = check_ready(h);
    if (rc) return rc;
    CastParams R{};
    if ((rc = cast_check_args(h, origins_dev, origin_stride_bytes, ends_dev, n, end_stride_bytes, params, out_dev, R))) return rc;
    const hipStream_t s = stream_of(h, hip_stream);
    if ((rc = cast_sync(h, s))) return rc;
    zero_stats(stats);
    if (n == 0) return GNDT_OK;
    if ((rc = use_stream(h, s)) || (rc = column_index(h, s))) return rc;
    const CastOut o{out_dev->row, out_dev->range, out_dev->d2};
    if ((rc = cast_launch(h, static_cast<const float*>(origins_dev), (uint32_t)(origin_stride_bytes / 4), static_cast<const float*>(ends_dev),
                          (uint32_t)(end_stride_bytes / 4), n, params, R, o, stats != nullptr, s)))
        return rc;
    if (stats) HIP_TRY(h, hipStreamSynchronize(s));
    cast_stats_out(h, stats);
    return GNDT_OK;
}

int gndt_cast_rays(gndt_handle* h, const void* origins_host, size_t origin_stride_bytes, const void* ends_host, size_t n,
                   size_t end_stride_bytes, const gndt_cast_params* params, const gndt_cast_out* out_host, gndt_cast_stats* stats) {
    int rc = check_ready(h);
    if (rc) return rc;
    CastParams R{};
    if ((rc = cast_check_args(h, origins_host, origin_stride_bytes, ends_host, n, end_stride_bytes, params, out_host, R))) return rc;
    const hipStream_t s = h->own_stream;
    if ((rc = cast_sync(h, s))) return rc;
    zero_stats(stats);
    if (n == 0) return GNDT_OK;
    if ((rc = use_stream(h, s)) || (rc = column_index(h, s))) return rc;
    IoPiece io[5] = {io_in(origins_host, origin_stride_bytes ? (uint64_t)n * origin_stride_bytes : 12),
                     io_in(ends_host, (uint64_t)n * end_stride_bytes),
                     io_out(out_host->row, (uint64_t)n * 4),
                     io_out(out_host->range, (uint64_t)n * 4),
                     io_out(out_host->d2, (uint64_t)n * 4)};
    if ((rc = stage_in(h, io, s))) return rc;
    const CastOut o{io[2].as<uint32_t>(), io[3].as<float>(), io[4].as<float>()};
    if ((rc = cast_launch(h, io[0].as<const float>(), (uint32_t)(origin_stride_bytes / 4), io[1].as<const float>(), (uint32_t)(end_stride_bytes / 4), n,
                          params, R, o, stats != nullptr, s)))
        return rc;
    if ((rc = stage_out(h, io, s))) return rc;
    cast_stats_out(h, stats);                          // (from their pinned mirror)
    return GNDT_OK;
}

}  // extern "C"
