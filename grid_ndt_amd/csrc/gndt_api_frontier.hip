// gndt_api_frontier.hip — frontier extraction (gndt_frontier.hpp): the slopes at which the known map ends, clustered into connected
// components, with the row of each cluster that is cheapest to reach.  A reader of the map (and, under REACHED, of the cost map) like
// the rasters: runs after the point queries' steps (query_sync) on the map's column index (column_index); launches on the caller's
// stream, nothing awaited.  The union-find's work memory lives in a scratch area of the handle.
#include "gndt_handle.hpp"
#include "gndt_frontier.hpp"

using namespace gndt;
using namespace gndt_host;

static_assert(sizeof(gndt_frontier_params) == 32 && sizeof(gndt_frontier) == 64 && sizeof(FrontierRecord) == 64, "the ABI of include/gndt.h \"frontier extraction\"");
static_assert(offsetof(gndt_frontier, best_row) == offsetof(FrontierRecord, best) && offsetof(gndt_frontier, best_h) == offsetof(FrontierRecord, best) + 4 &&
              offsetof(gndt_frontier, sx_min) == offsetof(FrontierRecord, sx_min) && offsetof(gndt_frontier, sum_px) == offsetof(FrontierRecord, sum_px) &&
              offsetof(gndt_frontier, open_sides) == offsetof(FrontierRecord, open_sides), "FrontierRecord is gndt_frontier (little-endian: best_row below best_h)");
static_assert(GNDT_FRONTIER_REACHED == kFrontierReached && GNDT_FRONTIER_SLOPES == kFrontierSlopes && GNDT_FRONTIER_OPEN_COLUMN == kFrontierOpenColumn &&
              GNDT_FRONTIER_OPEN_LEVEL == kFrontierOpenLevel, "gndt_frontier.hpp's enums are gndt.h's");

namespace gndt_host {

namespace {

constexpr const char* kFrontierCapture = "gndt_frontiers: a frontier call is not recorded into a hipGraph";

// Arguments (every GNDT_ERR_INVALID of include/gndt.h but the handle's state) -> the rule the kernels apply
int frontier_args(gndt_handle* h, const gndt_crop_box* box, const gndt_frontier_params* p, const gndt_frontier* clusters, uint32_t cluster_cap,
                  const uint32_t* counts, FrontierRule& F, uint32_t& min_size) {
    if (!p) { h->err = "gndt_frontiers: null params"; return GNDT_ERR_INVALID; }
    if (!counts) { h->err = "gndt_frontiers: null counts"; return GNDT_ERR_INVALID; }
    if (p->candidates != GNDT_FRONTIER_REACHED && p->candidates != GNDT_FRONTIER_SLOPES) { h->err = "gndt_frontiers: unknown candidates"; return GNDT_ERR_INVALID; }
    if (p->open_rule != GNDT_FRONTIER_OPEN_COLUMN && p->open_rule != GNDT_FRONTIER_OPEN_LEVEL) { h->err = "gndt_frontiers: unknown open_rule"; return GNDT_ERR_INVALID; }
    if (p->min_open > 4u) { h->err = "gndt_frontiers: min_open > 4 (a column has four sides)"; return GNDT_ERR_INVALID; }
    for (uint32_t r : p->reserved)
        if (r != 0u) { h->err = "gndt_frontiers: reserved must be 0"; return GNDT_ERR_INVALID; }
    if ((clusters == nullptr) != (cluster_cap == 0u)) { h->err = "gndt_frontiers: clusters is NULL exactly when cluster_cap is 0"; return GNDT_ERR_INVALID; }
    if (box) {                                         // the raster's rules but its pixel limit: nothing here is sized by the box
        if (box->sx_min > box->sx_max || box->sy_min > box->sy_max) { h->err = "gndt_frontiers: empty box (min > max)"; return GNDT_ERR_INVALID; }
        for (const int32_t v : {box->sx_min, box->sx_max, box->sy_min, box->sy_max})
            if (v < -kMaxXY || v > kMaxXY) { h->err = "gndt_frontiers: box index beyond +-65535 (the codec's range)"; return GNDT_ERR_INVALID; }
        if (!raster_count(box->sx_min, box->sx_max) || !raster_count(box->sy_min, box->sy_max)) {
            h->err = "gndt_frontiers: no non-zero index on an axis (signed indices skip 0)";
            return GNDT_ERR_INVALID;
        }
    }
    F = FrontierRule{p->candidates, p->open_rule, p->level_reach, std::max(p->min_open, 1u), p->link_dz, box ? 1 : 0,
                     box ? box->sx_min : 0, box ? box->sx_max : 0, box ? box->sy_min : 0, box ? box->sy_max : 0};
    min_size = std::max(p->min_size, 1u);
    return GNDT_OK;
}

// The handle's state (query_sync has run, with the cost map under REACHED): the stream and the column index, then the passes of
// gndt_frontier.hpp.  Nothing is awaited.
int frontier_enqueue(gndt_handle* h, const FrontierRule& F, uint32_t min_size, uint32_t* label, FrontierRecord* clusters, uint32_t cluster_cap,
                     uint32_t* counts, hipStream_t s) {
    int rc = use_stream(h, s);
    if (rc) return rc;
    const uint64_t rows = h->res_nodes;
    if (rows == 0) {                                   // nothing that indexes rows
        HIP_TRY(h, hipMemsetAsync(counts, 0, 4 * sizeof(uint32_t), s));
        return GNDT_OK;
    }
    if ((rc = rows_fit_32(h, "gndt_frontiers")) || (rc = column_index(h, s))) return rc;
    const uint32_t n = (uint32_t)rows;
    const uint32_t tiles = (n + kCropTile - 1) / kCropTile;
    FrontierScratch S;
    if ((rc = carve_scratch(h, h->frontier, S, n, tiles))) return rc;
    const QueryView Q = query_view(h);
    // the row passes: at most 2048 workgroups of 256 threads (what the chip holds at once), grid-stride beyond: the raster's launch
    const dim3 grid(grid_for(n, 256, 2048)), block(256);
    hipLaunchKernelGGL(k_frontier_mark, grid, block, 0, s, Q, F, n, S.parent, S.open, S.size_at);
    hipLaunchKernelGGL(k_frontier_link, grid, block, 0, s, Q, F, n, S.parent);
    hipLaunchKernelGGL(k_frontier_flatten, grid, block, 0, s, n, S.parent, S.size_at, label);
    hipLaunchKernelGGL(k_frontier_count, dim3(tiles), dim3(kCropT), 0, s, S.parent, S.size_at, n, min_size, S.tile_cnt);
    hipLaunchKernelGGL(k_frontier_scan, dim3(1), dim3(kCropScanT), 0, s, S.tile_cnt, tiles, counts);
    if (cluster_cap) {                                 // (a count-only call stops here)
        hipLaunchKernelGGL(k_frontier_rank, dim3(tiles), dim3(kCropT), 0, s, S.parent, S.size_at, n, min_size, S.tile_cnt, clusters, cluster_cap);
        hipLaunchKernelGGL(k_frontier_reduce, grid, block, 0, s, Q, F, n, S.parent, S.size_at, S.open, clusters);
    }
    HIP_TRY(h, hipGetLastError());
    return GNDT_OK;
}

}  // namespace

}  // namespace gndt_host

extern "C" {

int gndt_frontiers_device(gndt_handle* h, const gndt_crop_box* box, const gndt_frontier_params* params, uint32_t* label_dev,
                          gndt_frontier* clusters_dev, uint32_t cluster_cap, uint32_t* counts_dev, void* hip_stream) {
    int rc = check_ready(h);
    if (rc) return rc;
    FrontierRule F;
    uint32_t min_size = 1;
    if ((rc = frontier_args(h, box, params, clusters_dev, cluster_cap, counts_dev, F, min_size))) return rc;
    if (misaligned(7u, {clusters_dev}) || misaligned(3u, {counts_dev, label_dev})) {
        h->err = "gndt_frontiers_device: clusters_dev must be aligned as gndt_frontier is (8 bytes), counts_dev and label_dev to 4";
        return GNDT_ERR_INVALID;
    }
    const hipStream_t s = stream_of(h, hip_stream);
    if ((rc = query_sync(h, F.candidates == kFrontierReached, s, kFrontierCapture))) return rc;
    return frontier_enqueue(h, F, min_size, label_dev, reinterpret_cast<FrontierRecord*>(clusters_dev), cluster_cap, counts_dev, s);
}

int gndt_frontiers(gndt_handle* h, const gndt_crop_box* box, const gndt_frontier_params* params, uint32_t* label_host,
                   gndt_frontier* clusters_host, uint32_t cluster_cap, uint32_t* counts_host) {
    int rc = check_ready(h);
    if (rc) return rc;
    FrontierRule F;
    uint32_t min_size = 1;
    if ((rc = frontier_args(h, box, params, clusters_host, cluster_cap, counts_host, F, min_size))) return rc;
    const hipStream_t s = h->own_stream;
    // the steps that fix the row count first (staging is sized by it)
    if ((rc = query_sync(h, F.candidates == kFrontierReached, s, kFrontierCapture))) return rc;
    const uint64_t rows = h->res_nodes;
    IoPiece io[3] = {io_out(counts_host, 4 * sizeof(uint32_t)),     // (first of the outputs: the counts come back before the rest)
                     io_out(label_host, rows * 4),
                     {nullptr, nullptr, (uint64_t)cluster_cap * sizeof(gndt_frontier)}};     // the clusters: copied below
    if ((rc = stage_in(h, io, s))) return rc;
    if ((rc = frontier_enqueue(h, F, min_size, io[1].as<uint32_t>(), io[2].as<FrontierRecord>(), cluster_cap, io[0].as<uint32_t>(), s))) return rc;
    if ((rc = stage_out(h, io, s))) return rc;
    // only the records the call wrote: what lies beyond them in the caller's array stays as it is
    const uint64_t written = std::min<uint64_t>(counts_host[0], cluster_cap);
    if (written) HIP_TRY(h, hipMemcpy(clusters_host, io[2].dev, written * sizeof(gndt_frontier), hipMemcpyDeviceToHost));
    return GNDT_OK;
}

}  // extern "C"
