// gndt_api_view.hip — view gain (gndt_view.hpp): per pose of a batch, the distinct columns a fan of rays crosses before something stops
// them, split into those the map has and those it has not.  A reader of the map like ray casting: finished_map, the map's column index,
// one kernel on the caller's stream, nothing awaited.  The handle owns nothing for it: the two bitmaps of a pose live in the LDS of the
// workgroup that walks its rays.
#include <cmath>
#include <string>

#include "gndt_handle.hpp"
#include "gndt_view.hpp"

using namespace gndt;
using namespace gndt_host;

static_assert(sizeof(gndt_view_params) == 32 && sizeof(gndt_view_info) == 48 && sizeof(ViewInfo) == 48, "the ABI of include/gndt.h \"view gain\"");
static_assert(offsetof(gndt_view_info, steps) == offsetof(ViewInfo, steps) && offsetof(gndt_view_info, sum_uy) == offsetof(ViewInfo, sum_uy) &&
              offsetof(gndt_view_info, status) == offsetof(ViewInfo, status), "gndt_view.hpp's record is gndt.h's");
static_assert(kViewLdsTail == 1024u && kViewLdsDefault < kViewLdsBytes, "k_view_gain's tail holds every wave's tallies");

namespace gndt_host {

namespace {

constexpr uint64_t kMaxPoses = 0x7FFFFFFFull, kMaxDirs = 0x7FFFFFFFull;

// Arguments (every GNDT_ERR_INVALID of include/gndt.h but the handle's state and the window's size)
int view_check_args(gndt_handle* h, const void* poses, size_t K, const void* dirs, size_t n, size_t dir_stride, const gndt_view_params* p,
                    const gndt_view_info* info, CastParams& R) {
    if (!p) { h->err = "gndt_view_gain: null params"; return GNDT_ERR_INVALID; }
    if (K > kMaxPoses || n > kMaxDirs) { h->err = "gndt_view_gain: more than 2^31 - 1 poses or directions in one call"; return GNDT_ERR_INVALID; }
    if (K && n && (!poses || !dirs || !info)) { h->err = "gndt_view_gain: null poses, directions or info"; return GNDT_ERR_INVALID; }
    if (dir_stride != 12 && dir_stride != 16) { h->err = "gndt_view_gain: dir_stride_bytes must be 12 or 16"; return GNDT_ERR_INVALID; }
    if (!std::isfinite(p->max_range) || !(p->max_range > 0.f)) { h->err = "gndt_view_gain: max_range must be finite and > 0"; return GNDT_ERR_INVALID; }
    if (!std::isfinite(p->min_range) || p->min_range < 0.f) { h->err = "gndt_view_gain: min_range must be finite and >= 0"; return GNDT_ERR_INVALID; }
    if (p->min_count < 0) { h->err = "gndt_view_gain: min_count must be >= 0"; return GNDT_ERR_INVALID; }
    for (uint32_t r : p->reserved)
        if (r != 0u) { h->err = "gndt_view_gain: reserved must be 0"; return GNDT_ERR_INVALID; }
    R = CastParams{};
    R.min_count = (uint32_t)(p->min_count ? p->min_count : 1);
    R.min_range = (double)p->min_range;
    return GNDT_OK;
}

// The handle's state, in the cast's order: no capture, a finished map
int view_sync(gndt_handle* h, hipStream_t s) {
    const int rc = refuse_capture(h, s, "gndt_view_gain: a view gain call is not recorded into a hipGraph");
    return rc ? rc : finished_map(h, "no finished build to look into", false);
}

// The window of the call and the LDS its launch asks for: GNDT_ERR_INVALID when the two bitmaps do not fit what the kernel can be granted
int view_window(gndt_handle* h, const gndt_view_params* p, ViewRule& F, uint32_t& lds) {
    F = ViewRule{};
    F.max_range = p->max_range;
    F.reach = view_reach(p->max_range, h->P.grid_len);
    static LdsGrant grant;                             // k_view_gain's 160 KiB
    uint32_t room = kViewLdsDefault;
    if (view_lds_bytes(F.reach) > room && lds_granted(h, (const void*)&k_view_gain, kViewLdsBytes, grant)) room = kViewLdsBytes;
    if (view_lds_bytes(F.reach) > room) {
        h->err = "gndt_view_gain: max_range / grid_len gives a window of reach " + std::to_string(F.reach) + " columns, the largest whose two bitmaps fit the LDS of a workgroup is " +
                 std::to_string(view_max_reach(room)) + " (there is no global-memory tier): lower max_range, or look into a coarser map (gndt_coarsen_device)";
        return GNDT_ERR_INVALID;
    }
    F.words = (uint32_t)view_words(F.reach);
    lds = (uint32_t)view_lds_bytes(F.reach);
    return GNDT_OK;
}

// The kernel on the current map, everything on the device.  Waits for nothing.
int view_launch(gndt_handle* h, const double* poses, uint32_t K, const float* dirs, uint32_t sd, uint32_t n, const CastParams& R, const ViewRule& F,
                uint32_t lds, uint32_t* row, float* range, ViewInfo* info, hipStream_t s) {
    ScoreView S{};
    S.Q = query_view(h);
    S.count = h->out.count;
    S.cov = h->out.cov;
    RayGrid G{};
    G.ox = h->origin[0]; G.oy = h->origin[1]; G.oz = h->origin[2]; G.grid_len = h->P.grid_len; G.z_len = h->P.z_len;
    G.max_range = F.max_range; G.end_margin = 0.f;
    // threads: whole waves for the fan, at most the tuned block; workgroups: what 256 CUs hold of this window at once (LDS and the
    // CU's 2048 threads), grid-stride beyond
    const uint32_t cap = (uint32_t)tuning().view_threads;
    const uint32_t threads = std::min<uint32_t>(cap, (n + 63u) & ~63u);
    const uint32_t per_cu = std::max<uint32_t>(1u, std::min<uint32_t>(kViewLdsBytes / lds, 2048u / threads));
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(K, 256ull * per_cu);
    hipLaunchKernelGGL(k_view_gain, dim3(blocks), dim3(threads), lds, s, S, R, G, F, poses, K, dirs, sd, n, row, range, info);
    HIP_TRY(h, hipGetLastError());
    return GNDT_OK;
}

}  // namespace

}  // namespace gndt_host

extern "C" {

int gndt_view_gain_device(gndt_handle* h, const double* poses_dev, size_t K, const void* dirs_dev, size_t n, size_t dir_stride_bytes,
                          const gndt_view_params* params, gndt_view_info* info_dev, uint32_t* row_dev, float* range_dev, void* hip_stream) {
    int rc = check_ready(h);
    if (rc) return rc;
    CastParams R{};
    if ((rc = view_check_args(h, poses_dev, K, dirs_dev, n, dir_stride_bytes, params, info_dev, R))) return rc;
    if (misaligned(7u, {poses_dev, info_dev}) || misaligned(3u, {dirs_dev, row_dev, range_dev})) {
        h->err = "gndt_view_gain_device: poses_dev and info_dev must be aligned to 8 bytes, dirs_dev, row_dev and range_dev to 4";
        return GNDT_ERR_INVALID;
    }
    const hipStream_t s = stream_of(h, hip_stream);
    if ((rc = view_sync(h, s))) return rc;
    ViewRule F;
    uint32_t lds = 0;
    if ((rc = view_window(h, params, F, lds))) return rc;
    if (K == 0 || n == 0) return GNDT_OK;
    if ((rc = use_stream(h, s)) || (rc = column_index(h, s))) return rc;
    return view_launch(h, poses_dev, (uint32_t)K, static_cast<const float*>(dirs_dev), (uint32_t)(dir_stride_bytes / 4), (uint32_t)n, R, F, lds, row_dev,
                       range_dev, reinterpret_cast<ViewInfo*>(info_dev), s);
}

int gndt_view_gain(gndt_handle* h, const double* poses_host, size_t K, const void* dirs_host, size_t n, size_t dir_stride_bytes,
                   const gndt_view_params* params, gndt_view_info* info_host, uint32_t* row_host, float* range_host) {
    int rc = check_ready(h);
    if (rc) return rc;
    CastParams R{};
    if ((rc = view_check_args(h, poses_host, K, dirs_host, n, dir_stride_bytes, params, info_host, R))) return rc;
    const hipStream_t s = h->own_stream;
    if ((rc = view_sync(h, s))) return rc;
    ViewRule F;
    uint32_t lds = 0;
    if ((rc = view_window(h, params, F, lds))) return rc;
    if (K == 0 || n == 0) return GNDT_OK;
    if ((rc = use_stream(h, s)) || (rc = column_index(h, s))) return rc;
    IoPiece io[5] = {io_in(poses_host, (uint64_t)K * 12 * sizeof(double)),
                     io_in(dirs_host, (uint64_t)n * dir_stride_bytes),
                     io_out(info_host, (uint64_t)K * sizeof(ViewInfo)),
                     io_out(row_host, (uint64_t)K * n * 4),
                     io_out(range_host, (uint64_t)K * n * 4)};
    if ((rc = stage_in(h, io, s))) return rc;
    if ((rc = view_launch(h, io[0].as<const double>(), (uint32_t)K, io[1].as<const float>(), (uint32_t)(dir_stride_bytes / 4), (uint32_t)n, R, F, lds,
                          io[3].as<uint32_t>(), io[4].as<float>(), io[2].as<ViewInfo>(), s)))
        return rc;
    return stage_out(h, io, s);
}

}  // extern "C"
