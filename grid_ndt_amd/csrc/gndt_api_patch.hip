// gndt_api_patch.hip — surface patches (gndt_patch.hpp): the map's nodes grown into planes, each with its bounds, its members merged as
// Gaussians and the plane fitted to them.  A reader of the map like the frontiers: runs after the point queries' steps (query_sync) on
// the map's column index (column_index); launches on the caller's stream, nothing awaited.  The union-find's work memory and the listed
// patches' fp64 sums live in a scratch area of the handle.
#include "gndt_handle.hpp"
#include "gndt_patch.hpp"

using namespace gndt;
using namespace gndt_host;

static_assert(sizeof(gndt_patch_params) == 48 && sizeof(gndt_patch) == 128 && sizeof(PatchRecord) == 128, "the ABI of include/gndt.h \"surface patches\"");
static_assert(offsetof(gndt_patch, points) == offsetof(PatchRecord, points) && offsetof(gndt_patch, sx_min) == offsetof(PatchRecord, sx_min) &&
              offsetof(gndt_patch, sz_max) == offsetof(PatchRecord, sz_max) && offsetof(gndt_patch, sum_px) == offsetof(PatchRecord, sum_px) &&
              offsetof(gndt_patch, centroid) == offsetof(PatchRecord, centroid) && offsetof(gndt_patch, normal) == offsetof(PatchRecord, normal) &&
              offsetof(gndt_patch, var) == offsetof(PatchRecord, var) && offsetof(gndt_patch, kind) == offsetof(PatchRecord, kind), "PatchRecord is gndt_patch");
static_assert(GNDT_PATCH_NODES == kPatchNodes && GNDT_PATCH_SLOPES == kPatchSlopes && GNDT_PATCH_HORIZONTAL == kPatchHorizontal &&
              GNDT_PATCH_VERTICAL == kPatchVertical && GNDT_PATCH_INCLINED == kPatchInclined && GNDT_PATCH_SLOPES_ONLY == kPatchSlopesOnly,
              "gndt_patch.hpp's enums are gndt.h's");

namespace gndt_host {

namespace {

constexpr const char* kPatchCapture = "gndt_patches: a patch call is not recorded into a hipGraph";

bool threshold_ok(float v) { return std::isfinite(v) && v >= 0.f; }

// Arguments (every GNDT_ERR_INVALID of include/gndt.h but the handle's state) -> the rule the kernels apply
int patch_args(gndt_handle* h, const gndt_crop_box* box, const gndt_patch_params* p, const gndt_patch* patches, uint32_t patch_cap,
               const uint32_t* counts, PatchRule& F, uint32_t& min_size) {
    if (!p) { h->err = "gndt_patches: null params"; return GNDT_ERR_INVALID; }
    if (!counts) { h->err = "gndt_patches: null counts"; return GNDT_ERR_INVALID; }
    if (p->candidates != GNDT_PATCH_NODES && p->candidates != GNDT_PATCH_SLOPES) { h->err = "gndt_patches: unknown candidates"; return GNDT_ERR_INVALID; }
    if (p->connectivity > 3u) { h->err = "gndt_patches: connectivity > 3 (1, 2 or 3 axes may differ; 0 = 3)"; return GNDT_ERR_INVALID; }
    for (const float v : {p->cos_min, p->max_offset, p->max_var, p->cos_level, p->sin_level})
        if (!threshold_ok(v)) { h->err = "gndt_patches: a threshold is negative or not finite"; return GNDT_ERR_INVALID; }
    if (p->cos_min > 1.f || p->cos_level > 1.f) { h->err = "gndt_patches: cos_min or cos_level above 1"; return GNDT_ERR_INVALID; }
    for (uint32_t r : p->reserved)
        if (r != 0u) { h->err = "gndt_patches: reserved must be 0"; return GNDT_ERR_INVALID; }
    if ((patches == nullptr) != (patch_cap == 0u)) { h->err = "gndt_patches: patches is NULL exactly when patch_cap is 0"; return GNDT_ERR_INVALID; }
    if (box) {                                         // the frontiers' rules
        if (box->sx_min > box->sx_max || box->sy_min > box->sy_max) { h->err = "gndt_patches: empty box (min > max)"; return GNDT_ERR_INVALID; }
        for (const int32_t v : {box->sx_min, box->sx_max, box->sy_min, box->sy_max})
            if (v < -kMaxXY || v > kMaxXY) { h->err = "gndt_patches: box index beyond +-65535 (the codec's range)"; return GNDT_ERR_INVALID; }
        if (!raster_count(box->sx_min, box->sx_max) || !raster_count(box->sy_min, box->sy_max)) {
            h->err = "gndt_patches: no non-zero index on an axis (signed indices skip 0)";
            return GNDT_ERR_INVALID;
        }
    }
    F = PatchRule{p->candidates, p->connectivity ? p->connectivity : 3u, p->cos_min, p->max_offset, p->max_var, (double)p->cos_level,
                  (double)p->sin_level, box ? 1 : 0, box ? box->sx_min : 0, box ? box->sx_max : 0, box ? box->sy_min : 0, box ? box->sy_max : 0};
    min_size = std::max(p->min_size, 1u);
    return GNDT_OK;
}

// The handle's state (query_sync has run): the stream and the column index, then the passes of gndt_patch.hpp.  Nothing is awaited.
int patch_enqueue(gndt_handle* h, const PatchRule& F, uint32_t min_size, uint32_t* label, PatchRecord* patches, uint32_t patch_cap,
                  uint32_t* counts, hipStream_t s) {
    int rc = use_stream(h, s);
    if (rc) return rc;
    const uint64_t rows = h->res_nodes;
    if (rows == 0) {                                   // nothing that indexes rows
        HIP_TRY(h, hipMemsetAsync(counts, 0, 4 * sizeof(uint32_t), s));
        return GNDT_OK;
    }
    if ((rc = rows_fit_32(h, "gndt_patches")) || (rc = column_index(h, s))) return rc;
    const uint32_t n = (uint32_t)rows;
    const uint32_t tiles = (n + kCropTile - 1) / kCropTile;
    PatchScratch P;
    if ((rc = carve_scratch(h, h->patch, P, n, tiles, patch_cap))) return rc;
    ScoreView S{};
    S.Q = query_view(h);
    S.count = h->out.count;
    S.cov = h->out.cov;
    // the row passes: at most 2048 workgroups of 256 threads (what the chip holds at once), grid-stride beyond: the frontiers' launch
    const dim3 grid(grid_for(n, 256, 2048)), block(256);
    hipLaunchKernelGGL(k_patch_mark, grid, block, 0, s, S, F, n, P.parent, P.size_at);
    hipLaunchKernelGGL(k_patch_link, grid, block, 0, s, S, F, n, P.parent);
    hipLaunchKernelGGL(k_frontier_flatten, grid, block, 0, s, n, P.parent, P.size_at, label);
    hipLaunchKernelGGL(k_frontier_count, dim3(tiles), dim3(kCropT), 0, s, P.parent, P.size_at, n, min_size, P.tile_cnt);
    hipLaunchKernelGGL(k_frontier_scan, dim3(1), dim3(kCropScanT), 0, s, P.tile_cnt, tiles, counts);
    if (patch_cap) {                                   // (a count-only call stops here)
        hipLaunchKernelGGL(k_patch_rank, dim3(tiles), dim3(kCropT), 0, s, P.parent, P.size_at, n, min_size, P.tile_cnt, patches, P.moments, patch_cap);
        // the reductions: fewer, longer-lived workgroups (a wave carries a patch's integers over its trips, a workgroup sends a patch's
        // sums to memory once, behind its loop)
        const dim3 few(grid_for(n, 256, 512));
        hipLaunchKernelGGL(k_patch_reduce, few, block, 0, s, S, n, P.parent, P.size_at, patches);
        if (tuning().patch_lds) hipLaunchKernelGGL(k_patch_moments<true>, few, block, 0, s, S, n, P.parent, P.size_at, P.moments);
        else hipLaunchKernelGGL(k_patch_moments<false>, grid, block, 0, s, S, n, P.parent, P.size_at, P.moments);
        hipLaunchKernelGGL(k_patch_fit, dim3(grid_for(patch_cap, 64, 1024)), dim3(64), 0, s, S, F, counts, patch_cap, P.moments, patches);
    }
    HIP_TRY(h, hipGetLastError());
    return GNDT_OK;
}

}  // namespace

}  // namespace gndt_host

extern "C" {

int gndt_patches_device(gndt_handle* h, const gndt_crop_box* box, const gndt_patch_params* params, uint32_t* label_dev,
                        gndt_patch* patches_dev, uint32_t patch_cap, uint32_t* counts_dev, void* hip_stream) {
    int rc = check_ready(h);
    if (rc) return rc;
    PatchRule F;
    uint32_t min_size = 1;
    if ((rc = patch_args(h, box, params, patches_dev, patch_cap, counts_dev, F, min_size))) return rc;
    if (misaligned(7u, {patches_dev}) || misaligned(3u, {counts_dev, label_dev})) {
        h->err = "gndt_patches_device: patches_dev must be aligned as gndt_patch is (8 bytes), counts_dev and label_dev to 4";
        return GNDT_ERR_INVALID;
    }
    const hipStream_t s = stream_of(h, hip_stream);
    if ((rc = query_sync(h, false, s, kPatchCapture))) return rc;
    return patch_enqueue(h, F, min_size, label_dev, reinterpret_cast<PatchRecord*>(patches_dev), patch_cap, counts_dev, s);
}

int gndt_patches(gndt_handle* h, const gndt_crop_box* box, const gndt_patch_params* params, uint32_t* label_host,
                 gndt_patch* patches_host, uint32_t patch_cap, uint32_t* counts_host) {
    int rc = check_ready(h);
    if (rc) return rc;
    PatchRule F;
    uint32_t min_size = 1;
    if ((rc = patch_args(h, box, params, patches_host, patch_cap, counts_host, F, min_size))) return rc;
    const hipStream_t s = h->own_stream;
    // the steps that fix the row count first (staging is sized by it)
    if ((rc = query_sync(h, false, s, kPatchCapture))) return rc;
    const uint64_t rows = h->res_nodes;
    IoPiece io[3] = {io_out(counts_host, 4 * sizeof(uint32_t)),     // (first of the outputs: the counts come back before the rest)
                     io_out(label_host, rows * 4),
                     {nullptr, nullptr, (uint64_t)patch_cap * sizeof(gndt_patch)}};     // the patches: copied below
    if ((rc = stage_in(h, io, s))) return rc;
    if ((rc = patch_enqueue(h, F, min_size, io[1].as<uint32_t>(), io[2].as<PatchRecord>(), patch_cap, io[0].as<uint32_t>(), s))) return rc;
    if ((rc = stage_out(h, io, s))) return rc;
    // only the records the call wrote: what lies beyond them in the caller's array stays as it is
    const uint64_t written = std::min<uint64_t>(counts_host[0], patch_cap);
    if (written) HIP_TRY(h, hipMemcpy(patches_host, io[2].dev, written * sizeof(gndt_patch), hipMemcpyDeviceToHost));
    return GNDT_OK;
}

}  // extern "C"
