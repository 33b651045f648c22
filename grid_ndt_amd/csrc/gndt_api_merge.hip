// gndt_api_merge.hip — map merge (gndt_merge.hpp): the source's node table, moved by a pose, is added into the destination's.  By
// definition the destination ends as after gndt_stats_merge_device of the moved statistics + gndt_finalize_device, so the head and the
// tail of the call ARE those entry points (stats_merge_head, gndt_finalize_device), as gndt_api_coarsen.hip's are.
#include <cmath>

#include "gndt_handle.hpp"
#include "gndt_merge.hpp"

using namespace gndt;
using namespace gndt_host;

static_assert(sizeof(gndt_merge_params) == 8 && sizeof(gndt_merge_stats) == 48, "the ABI of include/gndt.h \"map merge\"");

namespace gndt_host {

void free_merge(gndt_handle* h) {
    if (h->merge.d_stats) (void)hipFree(h->merge.d_stats);
    if (h->merge.h_stats) (void)hipHostFree(h->merge.h_stats);
    h->merge = gndt_handle::Merge{};
}

namespace {

// GNDT_ERR_INVALID on both handles (the caller may ask either for the text)
int merge_refuse(gndt_handle* dst, gndt_handle* src, const std::string& msg) {
    src->err = msg;
    dst->err = msg;
    return GNDT_ERR_INVALID;
}

}  // namespace

}  // namespace gndt_host

extern "C" {

int gndt_merge_map_device(gndt_handle* dst, gndt_handle* src, const double pose[12], const gndt_merge_params* params,
                          gndt_merge_stats* stats, void* hip_stream) {
    if (!src || !dst) return GNDT_ERR_INVALID;
    if (src == dst) { dst->err = "gndt_merge_map: source and destination are the same handle"; return GNDT_ERR_INVALID; }
    if (src->device != dst->device) return merge_refuse(dst, src, "gndt_merge_map: the two handles are on different devices");
    MergeParams P{};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 4; ++j) {
            const double v = pose ? pose[4 * i + j] : (i == j ? 1.0 : 0.0);
            if (!std::isfinite(v)) return merge_refuse(dst, src, "gndt_merge_map: the pose has a non-finite entry");
            if (j < 3) P.R[3 * i + j] = v; else P.t[i] = v;
        }
    if (params && params->reserved != 0u) return merge_refuse(dst, src, "gndt_merge_map: reserved must be 0");
    if (params && params->min_count < 0) return merge_refuse(dst, src, "gndt_merge_map: min_count must be >= 0");
    P.min_count = (uint32_t)(params && params->min_count ? params->min_count : 1);
    int rc = check_ready(src);
    if (rc) { dst->err = src->err; return rc; }
    if (!dst->origin_set) return merge_refuse(dst, src, "gndt_merge_map: the destination has no origin (gndt_set_origin)");
    dst->capturing = false;
    if ((rc = refuse_capture(dst, stream_of(dst, hip_stream), "gndt_merge_map: a merge is not recorded into a hipGraph"))) {
        src->err = dst->err;
        return rc;
    }
    // what gndt_sync finishes on either handle (a pending build, a deferred emit, a re-run) comes first; points outside the key range
    // are only reported.  The source's stream is idle from here on, and nothing below enqueues on it.
    if ((rc = finished_map(src, "no finished build to merge", true))) { dst->err = src->err; return rc; }
    if (!src->map_in_table || src->cap == 0)
        return merge_refuse(dst, src, "gndt_merge_map needs the source's additive node table: build it with strategy ATOMIC / TILE or through gndt_update*");
    rc = gndt_sync(dst, nullptr, nullptr, nullptr);
    if (rc && rc != GNDT_ERR_KEY_RANGE) { src->err = dst->err; return rc; }
    // (gndt_sync has just waited: the source's mirror holds its table's node count and stream position)
    const uint32_t C = std::min(src->h_cnt->num_nodes, src->cap);
    const uint64_t src_pos = std::max<uint64_t>(src->stream_pos, src->h_cnt->stream_pos);

    // what the destination holds now (its stream is idle: gndt_sync has just waited), before anything of it is touched
    if ((rc = fetch_counters(dst, dst->last_stream))) { src->err = dst->err; return rc; }
    const uint64_t base = std::max<uint64_t>(dst->stream_pos, dst->h_cnt->stream_pos);
    const uint64_t nodes_before = dst->h_cnt->num_nodes;
    if (base + src_pos > 0xFFFFFFFEull)
        return merge_refuse(dst, src, "gndt_merge_map: the two point streams together exceed 2^32 - 2 points (point indices are 32-bit)");

    // ---- the destination: gndt_stats_merge_device's head (room for one new node per source node) ----
    hipStream_t s;
    if ((rc = stats_merge_head(dst, C, hip_stream, &s))) { src->err = dst->err; return rc; }
    auto& m = dst->merge;
    if (!m.d_stats) HIP_TRY(dst, hipMalloc(&m.d_stats, kMergeStats * sizeof(unsigned long long)));
    if (!m.h_stats) HIP_TRY(dst, hipHostMalloc(&m.h_stats, kMergeStats * sizeof(unsigned long long)));
    HIP_TRY(dst, hipMemsetAsync(m.d_stats, 0, kMergeStats * sizeof(unsigned long long), s));
    for (int k = 0; k < 3; ++k) { P.so[k] = src->origin[k]; P.dorg[k] = dst->origin[k]; }
    P.sgl = src->P.grid_len; P.szl = src->P.z_len;
    P.dgl = dst->P.grid_len; P.dzl = dst->P.z_len;
    P.base = (uint32_t)base;
    P.new_pos = (uint32_t)(base + src_pos);
    dst->last_strategy = GNDT_STRATEGY_ATOMIC;
    if (C) {
        hipLaunchKernelGGL(k_merge_map, dim3(grid_for(C)), dim3(kBlock), 0, s, (const uint64_t*)src->keys, (const NodeAcc*)src->acc,
                           (const uint32_t*)src->node_slot, src->cap - 1, (const Counters*)src->d_cnt, P, dst->keys, dst->acc, dst->cap - 1,
                           dst->node_slot, dst->index_of_slot, dst->d_cnt, m.d_stats);
        HIP_TRY(dst, hipGetLastError());
        dst->table_dirty = true;
    } else {
        hipLaunchKernelGGL(k_raise_stream, dim3(1), dim3(64), 0, s, dst->d_cnt, P.new_pos);
        HIP_TRY(dst, hipGetLastError());
    }
    dst->incr_ok = false;
    dst->results_valid = false;
    HIP_TRY(dst, hipMemcpyAsync(m.h_stats, m.d_stats, kMergeStats * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    // (waits: the source's table is free again when this returns, and the tallies and the exact node count are known)
    if ((rc = fetch_counters(dst, s))) return rc;
    dst->stream_pos = base + src_pos;
    dst->nodes_bound = dst->h_cnt->num_nodes;
    if (stats) {
        stats->source_nodes = m.h_stats[0]; stats->below_min_count = m.h_stats[1]; stats->skipped = m.h_stats[2];
        stats->merged_nodes = m.h_stats[3]; stats->merged_points = m.h_stats[4];
        stats->new_nodes = dst->h_cnt->num_nodes - nodes_before;
    }
    if (dst->h_cnt->err_table_full) { dst->err = "node table full: raise gndt_params.max_nodes_hint"; return GNDT_ERR_CAPACITY; }
    // the map is new: a graph recorded before this call is reported stale when replayed (as after a crop or a clear)
    ++dst->realloc_gen;
    return gndt_finalize_device(dst, hip_stream);
}

}  // extern "C"
