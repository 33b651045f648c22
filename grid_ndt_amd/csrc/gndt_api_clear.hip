// gndt_api_clear.hip — free-space clearing (gndt_ray.hpp): the nodes that the rays from a sensor origin to its end points pass through
// leave the map, unless an end point lies in them.  By definition a clear is gndt_remove of every point ever added to the nodes that
// leave, so the tail is gndt_remove_device's (drop_dead_and_finalize).
#include "gndt_handle.hpp"
#include "gndt_query.hpp"
#include "gndt_ray.hpp"

using namespace gndt;
using namespace gndt_host;

namespace gndt_host {

void free_clear(gndt_handle* h) {
    auto& c = h->clear;
    void* ptrs[] = {c.passes, c.ext, c.d_stats};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    if (c.h_stats) (void)hipHostFree(c.h_stats);
    c = gndt_handle::Clear{};
}

namespace {

constexpr uint64_t kMaxRays = 0x7FFFFFFFull;     // a pass count fits bits 0-30 whatever the rays do

// Arguments (every GNDT_ERR_INVALID of include/gndt.h but the handle's state)
int clear_check_args(gndt_handle* h, const float* origin, const void* xyz, size_t n, size_t stride_bytes, const gndt_clear_params* p) {
    if (!origin || !p) { h->err = "gndt_clear_rays: null origin or params"; return GNDT_ERR_INVALID; }
    if (n && !xyz) { h->err = "gndt_clear_rays: null points"; return GNDT_ERR_INVALID; }
    if (n > kMaxRays) { h->err = "gndt_clear_rays: more than 2^31 - 1 points in one call"; return GNDT_ERR_INVALID; }
    if (stride_bytes != 12 && stride_bytes != 16) { h->err = "gndt_clear_rays: stride_bytes must be 12 or 16"; return GNDT_ERR_INVALID; }
    if (p->flags & ~(uint32_t)GNDT_CLEAR_COUNT_ONLY) { h->err = "gndt_clear_rays: unknown flags"; return GNDT_ERR_INVALID; }
    if (!std::isfinite(p->max_range) || p->max_range < 0.f) { h->err = "gndt_clear_rays: max_range must be finite and >= 0"; return GNDT_ERR_INVALID; }
    if (!std::isfinite(p->end_margin) || p->end_margin < 0.f) { h->err = "gndt_clear_rays: end_margin must be finite and >= 0"; return GNDT_ERR_INVALID; }
    if (p->min_passes == 0u) { h->err = "gndt_clear_rays: min_passes must be >= 1"; return GNDT_ERR_INVALID; }
    if (!std::isfinite(origin[0]) || !std::isfinite(origin[1]) || !std::isfinite(origin[2])) {
        h->err = "gndt_clear_rays: non-finite origin"; return GNDT_ERR_INVALID;
    }
    if (!point_key(origin[0], origin[1], origin[2], h->origin[0], h->origin[1], h->origin[2], h->P.grid_len, h->P.z_len).ok) {
        h->err = "gndt_clear_rays: the origin has no key (beyond the codec's range)"; return GNDT_ERR_INVALID;
    }
    return GNDT_OK;
}

// The handle's state, in crop's order: no capture, a finished map (points outside the key range are only reported), the node table
// when clearing
int clear_sync(gndt_handle* h, bool count_only, hipStream_t s) {
    int rc = refuse_capture(h, s, "gndt_clear_rays: a clear is not recorded into a hipGraph");
    if (!rc) rc = finished_map(h, "no finished build to clear", true);
    if (rc) return rc;
    if (!count_only && (!h->map_in_table || h->cap == 0)) {
        h->err = "gndt_clear_rays needs the additive node table (strategy ATOMIC / TILE or a map built by gndt_update*); "
                 "GNDT_CLEAR_COUNT_ONLY works on every map";
        return GNDT_ERR_INVALID;
    }
    return GNDT_OK;
}

// Per-row scratch (pass counts unless the caller's buffer takes them, level extents) and the counters
int clear_buffers(gndt_handle* h, uint64_t rows) {
    auto& c = h->clear;
    if (!c.d_stats) HIP_TRY(h, hipMalloc(&c.d_stats, 4 * sizeof(unsigned long long)));
    if (!c.h_stats) HIP_TRY(h, hipHostMalloc(&c.h_stats, 4 * sizeof(unsigned long long)));
    if (rows * sizeof(LevelExtent) > c.ext_cap) c.ext_serial = 0;      // (a new buffer holds no extents)
    const int rc = grow_scratch(h, c.passes, c.passes_cap, rows * 4);
    return rc ? rc : grow_scratch(h, c.ext, c.ext_cap, rows * sizeof(LevelExtent));
}

// Protect, walk, tally (and while clearing, kill) on the current map; the counters go to the pinned mirror.  Waits for nothing.
int clear_launch(gndt_handle* h, const float* origin, const float* xyz, uint64_t n, uint32_t sf, const gndt_clear_params* p,
                 uint32_t* passes, hipStream_t s) {
    auto& c = h->clear;
    const uint64_t rows = h->res_nodes;
    const bool clear = !(p->flags & GNDT_CLEAR_COUNT_ONLY);
    const bool ext = tuning().clear_extent;
    HIP_TRY(h, hipMemsetAsync(c.d_stats, 0, 4 * sizeof(unsigned long long), s));
    if (rows) HIP_TRY(h, hipMemsetAsync(passes, 0, rows * 4, s));
    const QueryView Q = query_view(h);
    LevelExtent* E = static_cast<LevelExtent*>(c.ext);
    // the extents: kept while the map is the one they were computed for (map_current)
    if (ext && rows && !map_current(h, c.ext_serial)) {
        hipLaunchKernelGGL(k_clear_extent, dim3(grid_for(rows, 256, 2048)), dim3(256), 0, s, Q, (uint32_t)rows, E);
        HIP_TRY(h, hipGetLastError());
        c.ext_serial = h->result_serial;
    }
    RayGrid G;
    G.ox = h->origin[0]; G.oy = h->origin[1]; G.oz = h->origin[2]; G.grid_len = h->P.grid_len; G.z_len = h->P.z_len;
    G.rx = origin[0]; G.ry = origin[1]; G.rz = origin[2]; G.max_range = p->max_range; G.end_margin = p->end_margin;
    const int blocks = grid_for(n, 256, 2048);
    hipLaunchKernelGGL(k_clear_protect, dim3(blocks), dim3(256), 0, s, Q, G, xyz, sf, n, passes, c.d_stats);
    if (rows) {
        if (clear && ext) hipLaunchKernelGGL((k_clear_walk<true, true>), dim3(blocks), dim3(256), 0, s, Q, G, xyz, sf, n, E, passes, p->min_passes);
        else if (clear) hipLaunchKernelGGL((k_clear_walk<true, false>), dim3(blocks), dim3(256), 0, s, Q, G, xyz, sf, n, E, passes, p->min_passes);
        else if (ext) hipLaunchKernelGGL((k_clear_walk<false, true>), dim3(blocks), dim3(256), 0, s, Q, G, xyz, sf, n, E, passes, p->min_passes);
        else hipLaunchKernelGGL((k_clear_walk<false, false>), dim3(blocks), dim3(256), 0, s, Q, G, xyz, sf, n, E, passes, p->min_passes);
        HIP_TRY(h, hipGetLastError());
        const int rblocks = grid_for(rows, 256, 2048);
        const uint32_t cap_mask = h->cap ? h->cap - 1 : 0u;
        if (clear)
            hipLaunchKernelGGL(k_clear_kill<true>, dim3(rblocks), dim3(256), 0, s, (const int32_t*)h->out.sx, (const int32_t*)h->out.sy,
                               (const int32_t*)h->out.sz, (uint32_t)rows, passes, p->min_passes, h->keys, h->acc, cap_mask, h->d_cnt, c.d_stats);
        else
            hipLaunchKernelGGL(k_clear_kill<false>, dim3(rblocks), dim3(256), 0, s, (const int32_t*)h->out.sx, (const int32_t*)h->out.sy,
                               (const int32_t*)h->out.sz, (uint32_t)rows, passes, p->min_passes, (const uint64_t*)nullptr, (NodeAcc*)nullptr,
                               0u, h->d_cnt, c.d_stats);
    }
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(c.h_stats, c.d_stats, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    return GNDT_OK;
}

void clear_stats_out(const gndt_handle* h, gndt_clear_stats* stats) {
    if (!stats) return;
    const unsigned long long* v = h->clear.h_stats;
    stats->rays = v[0]; stats->skipped = v[1]; stats->protected_rows = v[2]; stats->cleared = v[3];
}

// After a clearing launch: wait, and if nodes died, gndt_remove_device's tail; then the crop's lifetime bookkeeping
int clear_finish(gndt_handle* h, hipStream_t s) {
    int rc = fetch_counters(h, s);                     // (waits) deaths are only known on the device
    if (rc) return rc;
    if (h->clear.h_stats[3]) {
        h->pending.active = false;
        next_event_set(h);
        h->last_strategy = GNDT_STRATEGY_ATOMIC;
        h->incr_ok = false;                            // every row is redone
        h->results_valid = false;
        if ((rc = drop_dead_and_finalize(h, s))) return rc;
    }
    // the map is new: cost map, column index and row numbers are stale; a graph recorded before this call is reported stale when replayed
    ++h->result_serial;
    ++h->realloc_gen;
    h->last_stream = s;
    return GNDT_OK;
}

void zero_stats(gndt_clear_stats* stats) {
    if (stats) { stats->rays = 0; stats->skipped = 0; stats->protected_rows = 0; stats->cleared = 0; }
}

}  // namespace

}  // namespace gndt_host

extern "C" {

int gndt_clear_rays_device(gndt_handle* h, const float origin_xyz[3], const void* xyz_dev, size_t n, size_t stride_bytes,
                           const gndt_clear_params* p, uint32_t* passes_out_dev, gndt_clear_stats* stats, void* hip_stream) {
    int rc = check_ready(h);
    if (rc) return rc;
    if ((rc = clear_check_args(h, origin_xyz, xyz_dev, n, stride_bytes, p))) return rc;
    const hipStream_t s = stream_of(h, hip_stream);
    const bool count_only = (p->flags & GNDT_CLEAR_COUNT_ONLY) != 0;
    if ((rc = clear_sync(h, count_only, s))) return rc;
    zero_stats(stats);
    if (n == 0) return GNDT_OK;
    if ((rc = use_stream(h, s)) || (rc = column_index(h, s))) return rc;
    if ((rc = clear_buffers(h, h->res_nodes))) return rc;
    uint32_t* passes = passes_out_dev ? passes_out_dev : h->clear.passes;
    if ((rc = clear_launch(h, origin_xyz, static_cast<const float*>(xyz_dev), n, (uint32_t)(stride_bytes / 4), p, passes, s))) return rc;
    if (count_only) {
        if (stats) HIP_TRY(h, hipStreamSynchronize(s));
        clear_stats_out(h, stats);
        return GNDT_OK;
    }
    if ((rc = clear_finish(h, s))) return rc;
    clear_stats_out(h, stats);
    return GNDT_OK;
}

int gndt_clear_rays(gndt_handle* h, const float origin_xyz[3], const void* xyz_host, size_t n, size_t stride_bytes,
                    const gndt_clear_params* p, uint32_t* passes_out_host, gndt_clear_stats* stats) {
    int rc = check_ready(h);
    if (rc) return rc;
    if ((rc = clear_check_args(h, origin_xyz, xyz_host, n, stride_bytes, p))) return rc;
    const hipStream_t s = h->own_stream;
    const bool count_only = (p->flags & GNDT_CLEAR_COUNT_ONLY) != 0;
    if ((rc = clear_sync(h, count_only, s))) return rc;
    zero_stats(stats);
    if (n == 0) return GNDT_OK;
    if ((rc = use_stream(h, s)) || (rc = column_index(h, s))) return rc;
    const uint64_t rows = h->res_nodes;
    if ((rc = clear_buffers(h, rows))) return rc;
    auto& c = h->clear;
    IoPiece io[1] = {io_in(xyz_host, (uint64_t)n * stride_bytes)};
    if ((rc = stage_in(h, io, s))) return rc;
    if ((rc = clear_launch(h, origin_xyz, io[0].as<const float>(), n, (uint32_t)(stride_bytes / 4), p, c.passes, s))) return rc;
    // (the passes come from the handle's own array, the stats from their pinned mirror: neither is staged)
    if (passes_out_host && rows) HIP_TRY(h, hipMemcpyAsync(passes_out_host, c.passes, rows * 4, hipMemcpyDeviceToHost, s));
    if ((rc = stage_out(h, io, s))) return rc;
    if (!count_only && (rc = clear_finish(h, s))) return rc;
    clear_stats_out(h, stats);
    if (!count_only) return gndt_sync(h, nullptr, nullptr, nullptr);
    return GNDT_OK;
}

}  // extern "C"
