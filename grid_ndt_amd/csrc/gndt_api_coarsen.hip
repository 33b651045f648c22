// gndt_api_coarsen.hip — map pyramids (gndt_coarsen.hpp): the destination handle becomes the map a build of the source's point stream
// at factor times the cell lengths would give, from the source's node table.  By definition the destination ends as after gndt_reset +
// gndt_stats_merge_device of the parents' statistics + gndt_finalize_device, so the head and the tail of the call ARE those entry points.
#include "gndt_handle.hpp"
#include "gndt_coarsen.hpp"

using namespace gndt;
using namespace gndt_host;

namespace {

bool coarsen_factor_ok(uint32_t f) { return f >= 1u && f <= 1024u && (f & (f - 1u)) == 0u; }

// GNDT_ERR_INVALID on both handles (the caller may ask either for the text)
int coarsen_refuse(gndt_handle* src, gndt_handle* dst, const std::string& msg) {
    src->err = msg;
    dst->err = msg;
    return GNDT_ERR_INVALID;
}

}  // namespace

extern "C" {

int gndt_coarsen_device(gndt_handle* src, gndt_handle* dst, uint32_t factor_xy, uint32_t factor_z, void* hip_stream) {
    if (!src || !dst) return GNDT_ERR_INVALID;
    if (src == dst) { src->err = "gndt_coarsen: source and destination are the same handle"; return GNDT_ERR_INVALID; }
    if (src->device != dst->device) return coarsen_refuse(src, dst, "gndt_coarsen: the two handles are on different devices");
    if (!coarsen_factor_ok(factor_xy) || !coarsen_factor_ok(factor_z))
        return coarsen_refuse(src, dst, "gndt_coarsen: a factor must be a power of two in 1 .. 1024");
    if (dst->P.grid_len != (float)factor_xy * src->P.grid_len || dst->P.z_len != (float)factor_z * src->P.z_len)
        return coarsen_refuse(src, dst, "gndt_coarsen: the destination's grid_len / z_len must be factor_xy / factor_z times the source's");
    int rc = check_ready(src);
    if (rc) { dst->err = src->err; return rc; }
    dst->capturing = false;
    const hipStream_t s = stream_of(dst, hip_stream);
    if ((rc = refuse_capture(dst, s, "gndt_coarsen: a coarsen is not recorded into a hipGraph"))) { src->err = dst->err; return rc; }
    // what gndt_sync finishes on the source (a pending build, a deferred emit, a re-run) comes first; points outside the key range are
    // only reported.  The source's stream is idle from here on, and nothing below enqueues on it.
    if ((rc = finished_map(src, "no finished build to coarsen", true))) { dst->err = src->err; return rc; }
    if (!src->map_in_table || src->cap == 0)
        return coarsen_refuse(src, dst, "gndt_coarsen needs the additive node table: build with strategy ATOMIC / TILE or through gndt_update*");
    // (gndt_sync has just waited: the mirror holds the table's node count and stream position; the kernel reads the device's own)
    const uint32_t C = std::min(src->h_cnt->num_nodes, src->cap);
    const uint64_t src_pos = std::min<uint64_t>(std::max<uint64_t>(src->stream_pos, src->h_cnt->stream_pos), 0xFFFFFFFEull);

    // ---- the destination: gndt_reset, the source's origin, room for every parent (at most one per source node) ----
    if ((rc = gndt_reset(dst, hip_stream))) return rc;
    if (memcmp(dst->origin, src->origin, sizeof(dst->origin)) != 0) dst->part.blk_state = 0;
    memcpy(dst->origin, src->origin, sizeof(dst->origin));
    dst->origin_set = true;
    if ((rc = reserve_table(dst, dst->P.max_nodes_hint ? std::max<uint64_t>(dst->P.max_nodes_hint, C) : C, s))) return rc;
    if (C) {
        CoarsenParams P;
        for (int k = 0; k < 3; ++k) P.o[k] = src->origin[k];
        P.grid_len = src->P.grid_len; P.z_len = src->P.z_len;
        P.coarse_grid_len = dst->P.grid_len; P.coarse_z_len = dst->P.z_len;
        P.fxy = (int)factor_xy; P.fz = (int)factor_z;
        hipLaunchKernelGGL(k_coarsen, dim3(grid_for(C)), dim3(kBlock), 0, s, (const uint64_t*)src->keys, (const NodeAcc*)src->acc,
                           (const uint32_t*)src->node_slot, src->cap - 1, (const Counters*)src->d_cnt, P, (uint32_t)src_pos, dst->keys,
                           dst->acc, dst->cap - 1, dst->node_slot, dst->index_of_slot, dst->d_cnt);
        HIP_TRY(dst, hipGetLastError());
        dst->incr_ok = false;
        dst->table_dirty = true;
        dst->results_valid = false;
    } else {
        hipLaunchKernelGGL(k_raise_stream, dim3(1), dim3(64), 0, s, dst->d_cnt, (uint32_t)src_pos);
        HIP_TRY(dst, hipGetLastError());
    }
    // (waits: the source's table is free again when this returns, and the parents' exact number is known)
    if ((rc = fetch_counters(dst, s))) return rc;
    dst->stream_pos = std::max<uint64_t>(src_pos, dst->h_cnt->stream_pos);
    dst->nodes_bound = dst->h_cnt->num_nodes;
    if (dst->h_cnt->err_table_full) { dst->err = "node table full: raise gndt_params.max_nodes_hint"; return GNDT_ERR_CAPACITY; }
    return gndt_finalize_device(dst, hip_stream);
}

}  // extern "C"
