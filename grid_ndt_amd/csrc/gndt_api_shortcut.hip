// gndt_api_shortcut.hip — route shortcutting (gndt_shortcut.hpp): K slope-to-slope routes string-pulled into any-angle waypoints.  A
// reader of the map like the path walks: runs after the point queries' steps (query_sync) on the map's column index (column_index);
// one kernel on the caller's stream, nothing awaited; no cost map and no work memory of the handle's.
#include <string.h>

#include <vector>

#include "gndt_handle.hpp"
#include "gndt_shortcut.hpp"

using namespace gndt;
using namespace gndt_host;

static_assert(sizeof(gndt_shortcut_params) == 32 && sizeof(gndt_shortcut_info) == 48 && sizeof(ShortcutInfo) == 48,
              "the ABI of include/gndt.h \"route shortcutting\"");
static_assert(GNDT_SHORTCUT_OK == kShortcutOk && GNDT_SHORTCUT_EMPTY == kShortcutEmpty && GNDT_SHORTCUT_BAD_ROUTE == kShortcutBadRoute &&
              GNDT_SHORTCUT_LIMIT == kShortcutLimit, "gndt_shortcut.hpp's constants are gndt.h's");

namespace gndt_host {

namespace {

// Arguments (every GNDT_ERR_INVALID of include/gndt.h but the handle's state and the device pointers' alignment) -> the rule the kernel applies
int shortcut_args(gndt_handle* h, const uint32_t* routes, size_t K, uint32_t route_cap, const void* lengths, size_t stride,
                  const gndt_shortcut_params* p, const uint32_t* wp, const uint32_t* path, uint32_t path_cap, const gndt_shortcut_info* info,
                  ShortcutRule& F) {
    if (!p) { h->err = "gndt_shortcut_routes: null params"; return GNDT_ERR_INVALID; }
    if (!info) { h->err = "gndt_shortcut_routes: null info"; return GNDT_ERR_INVALID; }
    if (K && (!routes || !lengths)) { h->err = "gndt_shortcut_routes: null routes or lengths"; return GNDT_ERR_INVALID; }
    if (K >= (1ull << 31)) { h->err = "gndt_shortcut_routes: 2^31 or more routes in one call"; return GNDT_ERR_INVALID; }
    if (K && route_cap == 0u) { h->err = "gndt_shortcut_routes: route_cap is 0"; return GNDT_ERR_INVALID; }
    if (stride < 4 || (stride & 3u)) { h->err = "gndt_shortcut_routes: length_stride_bytes must be a multiple of 4, at least 4"; return GNDT_ERR_INVALID; }
    if (p->window > kShortcutMaxWindow) { h->err = "gndt_shortcut_routes: window > 256 (it bounds a lane's loop)"; return GNDT_ERR_INVALID; }
    if (p->checks & ~(uint32_t)GNDT_WALK_CHECK_OVERHEAD) { h->err = "gndt_shortcut_routes: unknown check bits"; return GNDT_ERR_INVALID; }
    if (p->max_links > kShortcutMaxLinks) { h->err = "gndt_shortcut_routes: max_links > 2^24"; return GNDT_ERR_INVALID; }
    for (uint32_t r : p->reserved)
        if (r != 0u) { h->err = "gndt_shortcut_routes: reserved must be 0"; return GNDT_ERR_INVALID; }
    if (!wp) { h->err = "gndt_shortcut_routes: null waypoint_rows"; return GNDT_ERR_INVALID; }
    if ((path == nullptr) != (path_cap == 0u)) { h->err = "gndt_shortcut_routes: path_rows is NULL exactly when path_cap is 0"; return GNDT_ERR_INVALID; }
    F = ShortcutRule{p->window ? p->window : kShortcutDefaultWindow, p->max_links ? p->max_links : kShortcutDefaultLinks,
                     WalkRule{kQueryNearestSlope, p->checks, p->min_hops, kWalkDefaultSteps}};
    return GNDT_OK;
}

// The handle's state (query_sync has run): the stream, the column index, the kernel.  Nothing is awaited.
int shortcut_enqueue(gndt_handle* h, const Robot& R, const ShortcutRule& F, const uint32_t* routes, uint64_t K, uint32_t route_cap,
                     const void* lengths, uint64_t stride, const uint32_t* hops, uint32_t* wp, uint32_t wp_cap, uint32_t* path, uint32_t path_cap,
                     ShortcutInfo* info, hipStream_t s) {
    int rc = use_stream(h, s);
    if (rc) return rc;
    const uint64_t n = h->res_nodes;
    if ((rc = rows_fit_32(h, "gndt_shortcut_routes")) || (rc = column_index(h, s))) return rc;
    const QueryView Q = query_view(h);
    // one route a wavefront: at most kShortcutMaxBlocks workgroups of kShortcutWaves (16 wavefronts on each of the 256 CUs), grid-stride beyond
    const dim3 grid(grid_for(K, kShortcutWaves, kShortcutMaxBlocks)), block(kShortcutThreads);
    hipLaunchKernelGGL(k_shortcut_routes, grid, block, 0, s, Q, R, F, (uint32_t)n, hops, routes, K, route_cap, static_cast<const char*>(lengths),
                       stride, wp, wp_cap, path, path_cap, info);
    HIP_TRY(h, hipGetLastError());
    return GNDT_OK;
}

constexpr const char* kShortcutCapture = "gndt_shortcut_routes: a shortcut call is not recorded into a hipGraph";

}  // namespace

}  // namespace gndt_host

extern "C" {

int gndt_shortcut_routes_device(gndt_handle* h, const uint32_t* route_rows_dev, size_t K, uint32_t route_cap, const void* lengths_dev,
                                size_t length_stride_bytes, const gndt_robot* robot, const gndt_shortcut_params* params, const uint32_t* hops_dev,
                                uint32_t* waypoint_rows_dev, uint32_t waypoint_cap, uint32_t* path_rows_dev, uint32_t path_cap,
                                gndt_shortcut_info* info_dev, void* hip_stream) {
    int rc = check_ready(h);
    if (rc) return rc;
    ShortcutRule F;
    if ((rc = shortcut_args(h, route_rows_dev, K, route_cap, lengths_dev, length_stride_bytes, params, waypoint_rows_dev, path_rows_dev, path_cap,
                            info_dev, F)))
        return rc;
    if (misaligned(15u, {info_dev}) || misaligned(3u, {route_rows_dev, lengths_dev, hops_dev, waypoint_rows_dev, path_rows_dev})) {
        h->err = "gndt_shortcut_routes_device: info_dev must be 16-byte aligned (it is written 16 bytes at a time), the other pointers 4-byte";
        return GNDT_ERR_INVALID;
    }
    const hipStream_t s = stream_of(h, hip_stream);
    if ((rc = query_sync(h, false, s, kShortcutCapture))) return rc;
    if (K == 0) return GNDT_OK;
    return shortcut_enqueue(h, robot_of(robot), F, route_rows_dev, K, route_cap, lengths_dev, length_stride_bytes, hops_dev, waypoint_rows_dev,
                            waypoint_cap, path_rows_dev, path_cap, reinterpret_cast<ShortcutInfo*>(info_dev), s);
}

int gndt_shortcut_routes(gndt_handle* h, const uint32_t* route_rows_host, size_t K, uint32_t route_cap, const void* lengths_host,
                         size_t length_stride_bytes, const gndt_robot* robot, const gndt_shortcut_params* params, const uint32_t* hops_host,
                         uint32_t* waypoint_rows_host, uint32_t waypoint_cap, uint32_t* path_rows_host, uint32_t path_cap,
                         gndt_shortcut_info* info_host) {
    int rc = check_ready(h);
    if (rc) return rc;
    ShortcutRule F;
    if ((rc = shortcut_args(h, route_rows_host, K, route_cap, lengths_host, length_stride_bytes, params, waypoint_rows_host, path_rows_host, path_cap,
                            info_host, F)))
        return rc;
    const hipStream_t s = h->own_stream;
    if ((rc = query_sync(h, false, s, kShortcutCapture))) return rc;
    if (K == 0) return GNDT_OK;
    std::vector<uint32_t> lengths(K);                    // the lengths out of their records, whatever their alignment
    for (size_t k = 0; k < K; ++k) memcpy(&lengths[k], static_cast<const char*>(lengths_host) + k * length_stride_bytes, 4);
    IoPiece io[6] = {io_in(route_rows_host, (uint64_t)K * route_cap * 4),
                     io_in(lengths.data(), (uint64_t)K * 4),
                     io_in(hops_host, h->res_nodes * 4),
                     io_out(waypoint_rows_host, (uint64_t)K * waypoint_cap * 4),
                     io_out(path_rows_host, (uint64_t)K * path_cap * 4),
                     io_out(info_host, (uint64_t)K * sizeof(ShortcutInfo))};
    if ((rc = stage_in(h, io, s))) return rc;
    // (a map without rows: hops has no entry and every route is a BAD_ROUTE)
    if ((rc = shortcut_enqueue(h, robot_of(robot), F, io[0].as<const uint32_t>(), K, route_cap, io[1].dev, 4, io[2].as<const uint32_t>(),
                               io[3].as<uint32_t>(), waypoint_cap, io[4].as<uint32_t>(), path_cap, io[5].as<ShortcutInfo>(), s)))
        return rc;
    return stage_out(h, io, s);                          // (awaits the stream: `lengths` lives until here)
}

}  // extern "C"
