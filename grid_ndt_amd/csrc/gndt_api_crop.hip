// gndt_api_crop.hip — region crop (gndt_crop.hpp): the columns a box of signed column indices drops leave the map, without the points.
#include "gndt_handle.hpp"
#include "gndt_crop.hpp"

using namespace gndt;
using namespace gndt_host;

namespace gndt_host {

namespace {
void release_rows(gndt_handle* h, OutView& v, uint32_t*& ncol) {
    for (const RowArray& a : row_arrays(v)) release_device(h, *a.p);
    release_device(h, ncol);
    v = OutView{};
    ncol = nullptr;
}
}  // namespace

void free_crop(gndt_handle* h) {
    auto& c = h->crop;
    for (const RowArray& a : row_arrays(c.spare))
        if (*a.p) (void)hipFree(*a.p);
    for (void* p : {(void*)c.spare_ncol, (void*)c.tiles})
        if (p) (void)hipFree(p);
    c = gndt_handle::Crop{};
}

namespace {

// The second set of result arrays, with the capacities of the first (after the swap the handle's capacities are what they were)
int ensure_spare(gndt_handle* h) {
    auto& c = h->crop;
    const uint64_t rows = h->out_cap, ncols = h->part.row_ncol_cap;
    if (c.spare.sx && c.spare_cap == rows && c.spare_ncol_cap == ncols) return GNDT_OK;
    release_rows(h, c.spare, c.spare_ncol);
    c.spare_cap = c.spare_ncol_cap = 0;
    const int rc = alloc_rows(h, c.spare, rows);
    if (rc) return rc;
    HIP_TRY(h, hipMalloc(&c.spare_ncol, ncols * 4));
    c.spare_cap = rows;  c.spare_ncol_cap = ncols;
    return GNDT_OK;
}

// Table-backed map: the dropped nodes leave the node table, in place (k_crop_table + k_stats_merge); the stream position stays.
int crop_table(gndt_handle* h, const CropBox& B, hipStream_t s) {
    const uint32_t C = h->h_cnt->num_nodes;          // (gndt_sync has just waited: the mirror holds the table's node count)
    if (!C) return GNDT_OK;
    int rc = ensure_stats_buffers(h, C);
    if (rc) return rc;
    hipLaunchKernelGGL(k_crop_table, dim3(grid_for(C)), dim3(kBlock), 0, s, h->node_slot, h->col_slot_of_node, h->keys, h->acc, h->col_keys,
                       h->col_first, h->col_cnt, h->col_head, h->cap, C, B, (const Counters*)h->d_cnt, h->st_key, h->st_sums, h->st_count,
                       h->st_first);
    HIP_TRY(h, hipGetLastError());
    if (h->ever_captured) {
        // A graph recorded before the crop may be replayed after it: it must find the table of its day, whole, not this one half way
        // through a finalisation (it is reported stale either way).  So such a handle takes a fresh table and retires the old one
        // (alloc_table: table_gen moves), as a table reallocation does.
        if ((rc = alloc_table(h, h->cap, s))) return rc;
    }
    hipLaunchKernelGGL(k_crop_table_restart, dim3(1), dim3(64), 0, s, h->d_cnt);
    HIP_TRY(h, hipGetLastError());
    hipLaunchKernelGGL(k_stats_merge, dim3(grid_for(C)), dim3(kBlock), 0, s, h->keys, h->acc, h->cap - 1, h->node_slot, h->index_of_slot,
                       h->st_key, h->st_sums, h->st_count, h->st_first, (uint64_t)C, h->d_cnt);
    HIP_TRY(h, hipGetLastError());
    // the staging rows, order arrays and column entries of the last finalisation are gone: the next update relabels every column
    h->incr_ok = false;
    h->table_dirty = true;
    return GNDT_OK;
}

// What the row compaction needs, allocated before anything of the map is touched
int crop_prepare(gndt_handle* h) {
    auto& c = h->crop;
    const uint64_t n = h->res_nodes;
    if (n == 0) return GNDT_OK;
    if (n > h->out_cap || n > h->part.row_ncol_cap || !h->part.row_ncol) { h->err = "gndt_crop: result rows without their column index"; return GNDT_ERR_INVALID; }
    int rc = ensure_spare(h);
    if (rc) return rc;
    const uint64_t tiles = (n + kCropTile - 1) / kCropTile;
    if ((rc = grow_scratch(h, c.tiles, c.tiles_cap, tiles * 4))) return rc;
    if (h->map_in_table && h->cap && h->h_cnt->num_nodes) return ensure_stats_buffers(h, h->h_cnt->num_nodes);
    return GNDT_OK;
}

// Every map: the kept rows, in order, into the second set of arrays, which then becomes the result (the first one the spare).
int crop_rows(gndt_handle* h, const CropBox& B, hipStream_t s) {
    auto& c = h->crop;
    const uint64_t n = h->res_nodes;
    if (n == 0) return GNDT_OK;
    const uint64_t tiles = (n + kCropTile - 1) / kCropTile;
    const uint32_t n32 = (uint32_t)n;
    hipLaunchKernelGGL(k_crop_count, dim3((uint32_t)tiles), dim3(kCropT), 0, s, (const int32_t*)h->out.sx, (const int32_t*)h->out.sy, n32, B, c.tiles);
    HIP_TRY(h, hipGetLastError());
    hipLaunchKernelGGL(k_crop_scan, dim3(1), dim3(kCropScanT), 0, s, c.tiles, (uint32_t)tiles, h->d_cnt);
    HIP_TRY(h, hipGetLastError());
    hipLaunchKernelGGL(k_crop_scatter, dim3((uint32_t)tiles), dim3(kCropT), 0, s, h->out, (const uint32_t*)h->part.row_ncol, c.spare, c.spare_ncol,
                       n32, B, (const uint32_t*)c.tiles, h->d_cnt, h->h_cnt);
    HIP_TRY(h, hipGetLastError());
    std::swap(h->out, c.spare);
    std::swap(h->part.row_ncol, c.spare_ncol);       // (equal capacities: ensure_spare)
    // A call recorded into a hipGraph before the crop writes its rows through the pointers of its day: its replay is reported as stale
    // (realloc_gen, gndt_sync).  Such a handle keeps the old arrays until gndt_destroy (Handle::retired) instead of reusing them.
    ++h->realloc_gen;
    if (h->ever_captured) { release_rows(h, c.spare, c.spare_ncol); c.spare_cap = c.spare_ncol_cap = 0; }
    return GNDT_OK;
}

}  // namespace

}  // namespace gndt_host

extern "C" {

int gndt_crop_box_from_world(const float origin[3], float grid_len, const float lo_xy[2], const float hi_xy[2], gndt_crop_box* out) {
    if (!origin || !lo_xy || !hi_xy || !out) return GNDT_ERR_INVALID;
    if (!(grid_len > 0.f) || !std::isfinite(grid_len)) return GNDT_ERR_INVALID;
    for (int a = 0; a < 2; ++a)
        if (!std::isfinite(origin[a]) || !std::isfinite(lo_xy[a]) || !std::isfinite(hi_xy[a]) || lo_xy[a] > hi_xy[a]) return GNDT_ERR_INVALID;
    // axis_index is monotone in the coordinate (IEEE subtract, divide, ceil; no index 0): the columns of [lo, hi] are those between the
    // indices of its ends.  Ends beyond the codec's range clamp to it (no node lies further out).
    bool ok = true;
    gndt_crop_box b;
    b.sx_min = axis_index(lo_xy[0], origin[0], grid_len, ok, kMaxXY);
    b.sx_max = axis_index(hi_xy[0], origin[0], grid_len, ok, kMaxXY);
    b.sy_min = axis_index(lo_xy[1], origin[1], grid_len, ok, kMaxXY);
    b.sy_max = axis_index(hi_xy[1], origin[1], grid_len, ok, kMaxXY);
    *out = b;
    return GNDT_OK;
}

int gndt_crop_device(gndt_handle* h, const gndt_crop_box* box, int32_t mode, void* hip_stream) {
    int rc = check_ready(h);
    if (rc) return rc;
    if (!box) { h->err = "gndt_crop: null box"; return GNDT_ERR_INVALID; }
    if (mode != GNDT_CROP_KEEP_INSIDE && mode != GNDT_CROP_DROP_INSIDE) { h->err = "gndt_crop: unknown mode"; return GNDT_ERR_INVALID; }
    if (box->sx_min > box->sx_max || box->sy_min > box->sy_max) { h->err = "gndt_crop: empty box (min > max)"; return GNDT_ERR_INVALID; }
    const hipStream_t s = stream_of(h, hip_stream);
    if ((rc = refuse_capture(h, s, "gndt_crop: a crop is not recorded into a hipGraph"))) return rc;
    // what gndt_sync finishes (a pending build, a deferred emit, a re-run) comes first; points outside the key range are only reported
    if ((rc = finished_map(h, "no finished build to crop", true))) return rc;
    if ((rc = use_stream(h, s))) return rc;
    const CropBox B{box->sx_min, box->sx_max, box->sy_min, box->sy_max, mode == GNDT_CROP_KEEP_INSIDE ? 1 : 0};
    if ((rc = crop_prepare(h))) return rc;
    if (h->map_in_table && h->cap) {
        if ((rc = crop_table(h, B, s))) return rc;
    } else if (h->table_dirty) {
        // the rows came through the node table without living there (an owner build's records): the table is emptied, so that the
        // node count the crop leaves in the counters never describes a table that holds more nodes
        if ((rc = do_reset(h, s))) return rc;
        h->results_valid = true;
    }
    if ((rc = crop_rows(h, B, s))) { h->results_valid = false; return rc; }
    // the map has changed: cost map and column index are stale, the next update takes the full finalisation, nothing deferred is left
    ++h->result_serial;
    h->incr_ok = false;
    h->emit_pending = false; h->deferred_captured = false; h->pending_words = 0;
    h->small_used = false; h->small_captured = false;
    if (h->part.h_pc) h->part.h_pc->capture_id = 0;  // (what the mirrors hold next is this call's: not a replay)
    h->pending.active = false;
    h->last_stream = s;
    return GNDT_OK;
}

int gndt_crop(gndt_handle* h, const gndt_crop_box* box, int32_t mode) {
    int rc = check_ready(h);
    if (rc) return rc;
    rc = gndt_crop_device(h, box, mode, h->own_stream);
    if (rc) return rc;
    return gndt_sync(h, nullptr, nullptr, nullptr);
}

}  // extern "C"
