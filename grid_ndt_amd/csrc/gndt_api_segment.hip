// gndt_api_segment.hip — scan segmentation (gndt_segment.hpp): the points of a scan that the map does not explain, clustered into
// connected components of grid cells.  A reader of the map like scan scoring: finished_map, the map's column index, kernels on the
// caller's stream, nothing awaited.  The call's cell table and the union-find's work memory live in a scratch area of the handle
// whose size is a function of the point count alone.
#include <cmath>
#include <cstring>

#include "gndt_handle.hpp"
#include "gndt_segment.hpp"

using namespace gndt;
using namespace gndt_host;

static_assert(sizeof(gndt_segment_params) == 48 && sizeof(gndt_scan_cluster) == 72 && sizeof(SegRecord) == 72, "the ABI of include/gndt.h \"scan segmentation\"");
static_assert(offsetof(gndt_scan_cluster, sx_min) == offsetof(SegRecord, sx_min) && offsetof(gndt_scan_cluster, sum_x) == offsetof(SegRecord, sum_x) &&
              offsetof(gndt_scan_cluster, z_lo) == offsetof(SegRecord, z_lo) && offsetof(gndt_scan_cluster, z_hi) == offsetof(SegRecord, z_hi),
              "SegRecord is gndt_scan_cluster");
static_assert(GNDT_SEG_UNKEYED == kSegUnkeyed && GNDT_SEG_EXPLAINED == kSegExplained && GNDT_SEG_OFF_SURFACE == kSegOffSurface &&
              GNDT_SEG_UNMAPPED == kSegUnmapped, "gndt_segment.hpp's classes are gndt.h's");

namespace gndt_host {

namespace {

constexpr uint64_t kSegMaxPoints = 1ull << 30;       // 2 n slots stay within 2^31

// Arguments (every GNDT_ERR_INVALID of include/gndt.h but the handle's state) -> the rules the kernels apply
int segment_args(gndt_handle* h, const void* xyz, size_t n, size_t stride_bytes, const gndt_segment_params* p, const void* clusters,
                 uint32_t cluster_cap, const uint32_t* counts, ScoreParams& P, SegRule& R) {
    if (!p) { h->err = "gndt_segment_scan: null params"; return GNDT_ERR_INVALID; }
    if (!counts) { h->err = "gndt_segment_scan: null counts"; return GNDT_ERR_INVALID; }
    if (n && !xyz) { h->err = "gndt_segment_scan: null points"; return GNDT_ERR_INVALID; }
    if ((uint64_t)n >= (1ull << 32)) { h->err = "gndt_segment_scan: point indices do not fit 32 bits (n >= 2^32)"; return GNDT_ERR_INVALID; }
    if (stride_bytes != 12 && stride_bytes != 16) { h->err = "gndt_segment_scan: stride_bytes must be 12 or 16"; return GNDT_ERR_INVALID; }
    if (p->neighbourhood != GNDT_SCORE_DIRECT1 && p->neighbourhood != GNDT_SCORE_DIRECT7) {
        h->err = "gndt_segment_scan: unknown neighbourhood"; return GNDT_ERR_INVALID;
    }
    if (p->connectivity != 0u && p->connectivity != 6u && p->connectivity != 26u) {
        h->err = "gndt_segment_scan: connectivity must be 26, 6 or 0 (= 26)"; return GNDT_ERR_INVALID;
    }
    const int32_t floor_count = std::max<int32_t>(h->P.min_points, 3);
    if (p->min_count != 0 && p->min_count < floor_count) {
        h->err = "gndt_segment_scan: min_count must be 0 or at least max(min_points, 3) (smaller nodes keep zero statistics)";
        return GNDT_ERR_INVALID;
    }
    for (float v : {p->cov_rel, p->cov_floor, p->novel_d2})
        if (!std::isfinite(v) || v < 0.f) { h->err = "gndt_segment_scan: cov_rel, cov_floor and novel_d2 must be finite and >= 0"; return GNDT_ERR_INVALID; }
    if (p->classes & ~((1u << GNDT_SEG_OFF_SURFACE) | (1u << GNDT_SEG_UNMAPPED))) {
        h->err = "gndt_segment_scan: classes may hold the bits of GNDT_SEG_OFF_SURFACE and GNDT_SEG_UNMAPPED only"; return GNDT_ERR_INVALID;
    }
    for (uint32_t r : p->reserved)
        if (r != 0u) { h->err = "gndt_segment_scan: reserved must be 0"; return GNDT_ERR_INVALID; }
    if ((clusters == nullptr) != (cluster_cap == 0u)) { h->err = "gndt_segment_scan: clusters is NULL exactly when cluster_cap is 0"; return GNDT_ERR_INVALID; }
    P.min_count = (uint32_t)(p->min_count ? p->min_count : floor_count);
    P.cov_rel = (double)(p->cov_rel != 0.f ? p->cov_rel : 0.01f);
    P.cov_floor = (double)(p->cov_floor != 0.f ? p->cov_floor : 1e-6f);
    P.max_d2 = 0.0;
    R.novel_d2 = p->novel_d2 != 0.f ? p->novel_d2 : 11.345f;
    R.classes = p->classes ? p->classes : (1u << GNDT_SEG_OFF_SURFACE) | (1u << GNDT_SEG_UNMAPPED);
    R.min_points = std::max(p->min_points, 1u);
    R.connectivity = p->connectivity ? p->connectivity : 26u;
    R.min_cluster_points = std::max(p->min_cluster_points, 1u);
    R.min_cluster_cells = std::max(p->min_cluster_cells, 1u);
    return GNDT_OK;
}

// The handle's state, in scan scoring's order: no capture, a finished map
int segment_sync(gndt_handle* h, hipStream_t s) {
    const int rc = refuse_capture(h, s, "gndt_segment_scan: a segmentation is not recorded into a hipGraph");
    return rc ? rc : finished_map(h, "no finished build to segment against", false);
}

// Arguments checked, the handle's state looked at, the stream taken (segment_sync, use_stream): the column index, the scratch and the
// passes of gndt_segment.hpp, everything on the device.  Nothing is awaited.
int segment_enqueue(gndt_handle* h, const void* xyz_dev, size_t n64, size_t stride_bytes, const double* pose, int32_t nbh, const ScoreParams& P,
                    const SegRule& R, uint8_t* point_class, uint32_t* point_label, SegRecord* clusters, uint32_t cluster_cap, uint32_t* counts,
                    hipStream_t s) {
    if (n64 == 0) {
        HIP_TRY(h, hipMemsetAsync(counts, 0, 4 * sizeof(uint32_t), s));
        return GNDT_OK;
    }
    if (n64 > kSegMaxPoints) { h->err = "gndt_segment_scan: more than 2^30 points in one call (the cell table would pass 2^31 slots)"; return GNDT_ERR_CAPACITY; }
    int rc = column_index(h, s);
    if (rc) return rc;
    const uint32_t n = (uint32_t)n64;
    const uint64_t slots = seg_table_slots(n);
    const uint32_t tiles = (n + kCropTile - 1) / kCropTile;
    SegmentScratch A;
    if ((rc = carve_scratch(h, h->segment, A, n, slots, tiles))) return rc;
    const SegTable T = A.T;
    HIP_TRY(h, hipMemsetAsync(T.key, 0xFF, slots * 12, s));             // key | first: kEmptyKey, and the identity of the minimum
    HIP_TRY(h, hipMemsetAsync(T.count, 0, slots * 4, s));
    HIP_TRY(h, hipMemsetAsync(A.cells_at, 0, (uint64_t)n * 8, s));       // A.cells_at | A.points_at
    ScoreView S{};
    S.Q = query_view(h);
    S.count = h->out.count;
    S.cov = h->out.cov;
    const float* xyz = static_cast<const float*>(xyz_dev);
    const uint32_t sf = (uint32_t)(stride_bytes / 4);
    // the point passes: at most 2048 workgroups of 256 threads (what the chip holds at once), grid-stride beyond
    const dim3 grid(grid_for(n, 256, 2048)), block(256);
    if (nbh == GNDT_SCORE_DIRECT1)
        hipLaunchKernelGGL((k_seg_classify<kScoreDirect1>), grid, block, 0, s, S, P, R, xyz, sf, n, pose, T, A.slot_root, A.cls_of, point_class);
    else
        hipLaunchKernelGGL((k_seg_classify<kScoreDirect7>), grid, block, 0, s, S, P, R, xyz, sf, n, pose, T, A.slot_root, A.cls_of, point_class);
    hipLaunchKernelGGL(k_seg_cells, grid, block, 0, s, T, R, n, A.slot_root, A.parent);
    hipLaunchKernelGGL(k_seg_link, grid, block, 0, s, T, R, n, A.slot_root, A.parent);
    hipLaunchKernelGGL(k_seg_flatten, grid, block, 0, s, T, R, n, A.parent, A.slot_root, A.cells_at, A.points_at, point_label);
    hipLaunchKernelGGL(k_seg_count, dim3(tiles), dim3(kCropT), 0, s, R, A.parent, A.cls_of, A.cells_at, A.points_at, n, A.tile_cnt);
    hipLaunchKernelGGL(k_seg_scan, dim3(1), dim3(kCropScanT), 0, s, A.tile_cnt, tiles, counts);
    if (cluster_cap) {                                 // (a count-only call stops here)
        hipLaunchKernelGGL(k_seg_rank, dim3(tiles), dim3(kCropT), 0, s, R, A.parent, A.cls_of, A.cells_at, A.points_at, n, A.tile_cnt, clusters, cluster_cap);
        hipLaunchKernelGGL(k_seg_reduce, grid, block, 0, s, S.Q, xyz, sf, n, pose, A.slot_root, A.points_at, A.cls_of, clusters);
        hipLaunchKernelGGL(k_seg_finish, dim3(grid_for(cluster_cap, 256, 256)), block, 0, s, clusters, cluster_cap, counts);
    }
    HIP_TRY(h, hipGetLastError());
    return GNDT_OK;
}

}  // namespace

}  // namespace gndt_host

extern "C" {

int gndt_segment_scan_device(gndt_handle* h, const void* xyz_dev, size_t n, size_t stride_bytes, const double* pose_dev,
                             const gndt_segment_params* params, uint8_t* point_class_dev, uint32_t* point_label_dev,
                             gndt_scan_cluster* clusters_dev, uint32_t cluster_cap, uint32_t* counts_dev, void* hip_stream) {
    int rc = check_ready(h);
    if (rc) return rc;
    ScoreParams P{};
    SegRule R{};
    if ((rc = segment_args(h, xyz_dev, n, stride_bytes, params, clusters_dev, cluster_cap, counts_dev, P, R))) return rc;
    if (misaligned(7u, {clusters_dev, pose_dev}) || misaligned(3u, {counts_dev, point_label_dev, xyz_dev})) {
        h->err = "gndt_segment_scan_device: clusters_dev and pose_dev must be aligned to 8 bytes, counts_dev, point_label_dev and xyz_dev to 4";
        return GNDT_ERR_INVALID;
    }
    const hipStream_t s = stream_of(h, hip_stream);
    if ((rc = segment_sync(h, s)) || (rc = use_stream(h, s))) return rc;
    return segment_enqueue(h, xyz_dev, n, stride_bytes, pose_dev, params->neighbourhood, P, R, point_class_dev, point_label_dev,
                           reinterpret_cast<SegRecord*>(clusters_dev), cluster_cap, counts_dev, s);
}

int gndt_segment_scan(gndt_handle* h, const void* xyz_host, size_t n, size_t stride_bytes, const double* pose_host,
                      const gndt_segment_params* params, uint8_t* point_class_host, uint32_t* point_label_host,
                      gndt_scan_cluster* clusters_host, uint32_t cluster_cap, uint32_t* counts_host) {
    int rc = check_ready(h);
    if (rc) return rc;
    ScoreParams P{};
    SegRule R{};
    if ((rc = segment_args(h, xyz_host, n, stride_bytes, params, clusters_host, cluster_cap, counts_host, P, R))) return rc;
    const hipStream_t s = h->own_stream;
    if ((rc = segment_sync(h, s)) || (rc = use_stream(h, s))) return rc;
    if (n > kSegMaxPoints) { h->err = "gndt_segment_scan: more than 2^30 points in one call (the cell table would pass 2^31 slots)"; return GNDT_ERR_CAPACITY; }
    IoPiece io[6] = {io_in(xyz_host, (uint64_t)n * stride_bytes),
                     io_in(pose_host, 12 * sizeof(double)),
                     io_out(counts_host, 4 * sizeof(uint32_t)),     // (first of the outputs: the counts come back before the rest)
                     io_out(point_class_host, (uint64_t)n),
                     io_out(point_label_host, (uint64_t)n * 4),
                     {nullptr, nullptr, (uint64_t)cluster_cap * sizeof(gndt_scan_cluster)}};     // the clusters: copied below
    if ((rc = stage_in(h, io, s))) return rc;
    if ((rc = segment_enqueue(h, io[0].dev, n, stride_bytes, io[1].as<const double>(), params->neighbourhood, P, R, io[3].as<uint8_t>(),
                              io[4].as<uint32_t>(), io[5].as<SegRecord>(), cluster_cap, io[2].as<uint32_t>(), s)))
        return rc;
    if ((rc = stage_out(h, io, s))) return rc;
    // only the records the call wrote: what lies beyond them in the caller's array stays as it is
    const uint64_t written = std::min<uint64_t>(counts_host[0], cluster_cap);
    if (written) HIP_TRY(h, hipMemcpy(clusters_host, io[5].dev, written * sizeof(gndt_scan_cluster), hipMemcpyDeviceToHost));
    return GNDT_OK;
}

}  // extern "C"
