// gndt_api_raster.hip — raster export (gndt_query.hpp k_raster): one pixel per column of a box of signed column indices, the slope of
// the column a consumer stands on (the reference's showBottom / showSlopeList, include/map2D.h:980-1284), with its row, height,
// roughness, node count and cost.  Runs after the point queries' steps (query_sync) on the map's column index (column_index).
#include "gndt_handle.hpp"
#include "gndt_query.hpp"

using namespace gndt;
using namespace gndt_host;

namespace gndt_host {

namespace {

// The image size of a box, or what is wrong with it (no handle needed: gndt_raster_shape)
const char* raster_box(const gndt_crop_box* box, uint32_t& width, uint32_t& height) {
    if (!box) return "gndt_raster: null box";
    if (box->sx_min > box->sx_max || box->sy_min > box->sy_max) return "gndt_raster: empty box (min > max)";
    for (const int32_t v : {box->sx_min, box->sx_max, box->sy_min, box->sy_max})
        if (v < -kMaxXY || v > kMaxXY) return "gndt_raster: box index beyond +-65535 (the codec's range)";
    width = raster_count(box->sx_min, box->sx_max);
    height = raster_count(box->sy_min, box->sy_max);
    if (!width || !height) return "gndt_raster: no non-zero index on an axis (signed indices skip 0)";
    if ((uint64_t)width * height > (1ull << 31)) return "gndt_raster: width * height > 2^31";
    return nullptr;
}

int raster_args(gndt_handle* h, const gndt_crop_box* box, int32_t mode, float z_ref, const gndt_raster_layers* L, uint32_t& width,
                uint32_t& height) {
    if (!L || !(L->row || L->z || L->rough || L->nodes || L->h || L->state)) { h->err = "gndt_raster: no layer requested"; return GNDT_ERR_INVALID; }
    if (mode != GNDT_RASTER_LOWEST && mode != GNDT_RASTER_HIGHEST && mode != GNDT_RASTER_NEAREST_Z) {
        h->err = "gndt_raster: unknown mode";
        return GNDT_ERR_INVALID;
    }
    if (mode == GNDT_RASTER_NEAREST_Z && !std::isfinite(z_ref)) { h->err = "gndt_raster: NEAREST_Z needs a finite z_ref"; return GNDT_ERR_INVALID; }
    if (const char* e = raster_box(box, width, height)) { h->err = e; return GNDT_ERR_INVALID; }
    return GNDT_OK;
}

template <int MODE, uint32_t GATHER>
void raster_launch(const QueryView& Q, const gndt_crop_box& B, uint32_t width, uint32_t n, float z_ref, const RasterOut& o, hipStream_t s) {
    // at most 2048 workgroups of 256 threads (what the chip holds at once), grid-stride beyond: the query's launch
    hipLaunchKernelGGL((k_raster<MODE, GATHER>), dim3(grid_for(n, 256, 2048)), dim3(256), 0, s, Q, (int)B.sx_min, (int)B.sy_min, width, n,
                       z_ref, o);
}

template <int MODE>
void raster_launch_gather(const QueryView& Q, const gndt_crop_box& B, uint32_t width, uint32_t n, float z_ref, const RasterOut& o,
                          hipStream_t s) {
    const uint32_t gather = (o.z || o.rough ? kRasterSlope : 0u) | (o.h || o.state ? kRasterCost : 0u);
    if (gather == 0u) raster_launch<MODE, 0u>(Q, B, width, n, z_ref, o, s);
    else if (gather == kRasterSlope) raster_launch<MODE, kRasterSlope>(Q, B, width, n, z_ref, o, s);
    else if (gather == kRasterCost) raster_launch<MODE, kRasterCost>(Q, B, width, n, z_ref, o, s);
    else raster_launch<MODE, kRasterSlope | kRasterCost>(Q, B, width, n, z_ref, o, s);
}

// Arguments checked: the queries' steps (capture, finished map, cost map, gndt_sync), the stream and the column index, then one kernel
int raster_enqueue(gndt_handle* h, const gndt_crop_box& B, int32_t mode, float z_ref, uint32_t width, uint32_t height,
                   const gndt_raster_layers& L, hipStream_t s) {
    int rc = query_sync(h, L.h || L.state, s, "gndt_raster: a raster is not recorded into a hipGraph");
    if (rc) return rc;
    if ((rc = use_stream(h, s)) || (rc = column_index(h, s))) return rc;
    const QueryView Q = query_view(h);
    const RasterOut o{L.row, L.z, L.rough, L.nodes, L.h, L.state};
    const uint32_t n = width * height;               // (<= 2^31: raster_box)
    if (mode == GNDT_RASTER_LOWEST) raster_launch_gather<kRasterLowest>(Q, B, width, n, z_ref, o, s);
    else if (mode == GNDT_RASTER_HIGHEST) raster_launch_gather<kRasterHighest>(Q, B, width, n, z_ref, o, s);
    else raster_launch_gather<kRasterNearestZ>(Q, B, width, n, z_ref, o, s);
    HIP_TRY(h, hipGetLastError());
    return GNDT_OK;
}

}  // namespace

}  // namespace gndt_host

extern "C" {

int gndt_raster_shape(const gndt_crop_box* box, uint32_t* width, uint32_t* height) {
    if (!width || !height) return GNDT_ERR_INVALID;
    uint32_t w = 0, ht = 0;
    if (raster_box(box, w, ht)) return GNDT_ERR_INVALID;
    *width = w;
    *height = ht;
    return GNDT_OK;
}

int gndt_raster_device(gndt_handle* h, const gndt_crop_box* box, int32_t mode, float z_ref, const gndt_raster_layers* out_dev,
                       void* hip_stream) {
    int rc = check_ready(h);
    if (rc) return rc;
    uint32_t width = 0, height = 0;
    if ((rc = raster_args(h, box, mode, z_ref, out_dev, width, height))) return rc;
    return raster_enqueue(h, *box, mode, z_ref, width, height, *out_dev, stream_of(h, hip_stream));
}

int gndt_raster(gndt_handle* h, const gndt_crop_box* box, int32_t mode, float z_ref, const gndt_raster_layers* out_host) {
    int rc = check_ready(h);
    if (rc) return rc;
    uint32_t width = 0, height = 0;
    if ((rc = raster_args(h, box, mode, z_ref, out_host, width, height))) return rc;
    const hipStream_t s = h->own_stream;
    // the requested layers in the handle's staging
    const uint64_t n = (uint64_t)width * height;
    IoPiece io[6] = {io_out(out_host->row, n * 4), io_out(out_host->z, n * 4),     io_out(out_host->rough, n * 4),
                     io_out(out_host->nodes, n * 4), io_out(out_host->h, n * 4), io_out(out_host->state, n * 4)};
    if ((rc = stage_in(h, io, s))) return rc;
    const gndt_raster_layers L{io[0].as<uint32_t>(), io[1].as<float>(), io[2].as<float>(), io[3].as<uint32_t>(), io[4].as<float>(), io[5].as<uint32_t>()};
    if ((rc = raster_enqueue(h, *box, mode, z_ref, width, height, L, s))) return rc;
    return stage_out(h, io, s);
}

}  // extern "C"
