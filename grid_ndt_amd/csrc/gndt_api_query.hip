// gndt_api_query.hip — batched point queries against the finished grid (gndt_query.hpp): the lookup of computeCost's goal
// (include/map2D.h:1291-1306) and findRoute's start / goal (include/GlobalPlan.h:56-61) for n points at once.
#include "gndt_handle.hpp"
#include "gndt_query.hpp"

using namespace gndt;
using namespace gndt_host;

namespace gndt_host {

// What a query or a raster does before its kernel (the rules of include/gndt.h "point queries", stated once for both): no capture,
// a finished map (gndt_sync first finishes a pending build, a deferred emit, a re-run), a cost map of the current grid when gathered.
int query_sync(gndt_handle* h, bool gather, hipStream_t s, const char* capture_err) {
    int rc = refuse_capture(h, s, capture_err);
    if (!rc) rc = finished_map(h, "no finished build to query (the lookups run on the map create2DMap made, receiver.cpp:160, 171)", false);
    if (!rc && gather) rc = cost_map_check(h);
    return rc;
}

// The rows, the column index and the cost map as every consumer's kernels read them
QueryView query_view(gndt_handle* h) {
    QueryView Q{};
    CostView& V = Q.V;
    V.sx = h->out.sx; V.sy = h->out.sy; V.sz = h->out.sz;
    V.mean = h->out.mean; V.normal = h->out.normal; V.rough = h->out.rough; V.flags = h->out.flags;
    V.row_ncol = h->part.row_ncol;
    V.ctab_key = h->index.key; V.ctab_val = h->index.val; V.ctab_mask = h->index.mask;
    V.slope_interval = h->P.slope_interval; V.demand_true = h->P.demand == GNDT_DEMAND_TRUE ? 1 : 0;
    Q.h_bits = h->cost.h_bits; Q.state = h->cost.state;
    Q.ox = h->origin[0]; Q.oy = h->origin[1]; Q.oz = h->origin[2];
    Q.grid_len = h->P.grid_len; Q.z_len = h->P.z_len;
    return Q;
}

namespace {

// Arguments, the finished map, the cost map when asked for (n == 0 stops there), the stream; then the map's column index.
int query_prepare(gndt_handle* h, const void* xyz, size_t n, size_t stride_bytes, int32_t mode, const uint32_t* row_out, bool gather,
                  hipStream_t s) {
    if (n && !xyz) { h->err = "gndt_query: null points"; return GNDT_ERR_INVALID; }
    if (n && !row_out) { h->err = "gndt_query: null row_out"; return GNDT_ERR_INVALID; }
    if (mode != GNDT_QUERY_NODE && mode != GNDT_QUERY_NEAREST_SLOPE) { h->err = "gndt_query: unknown mode"; return GNDT_ERR_INVALID; }
    if (stride_bytes != 12 && stride_bytes != 16) { h->err = "gndt_query: stride_bytes must be 12 or 16"; return GNDT_ERR_INVALID; }
    int rc = query_sync(h, gather, s, "gndt_query: a query is not recorded into a hipGraph");
    if (rc || n == 0) return rc;
    if ((rc = use_stream(h, s))) return rc;
    return column_index(h, s);
}

template <int ILP, int MODE, bool GATHER>
void query_launch(const QueryView& Q, const float* xyz, uint32_t sf, uint64_t n, uint32_t* row_out, float* h_out, uint32_t* state_out,
                  hipStream_t s) {
    // at most 2048 workgroups of 256 threads (32 waves on each of the 256 CUs: what the chip holds at once), grid-stride beyond
    const int blocks = grid_for((n + ILP - 1) / ILP, 256, 2048);
    hipLaunchKernelGGL((k_query<ILP, MODE, GATHER>), dim3(blocks), dim3(256), 0, s, Q, xyz, sf, (uint64_t)n, row_out, h_out, state_out);
}

template <int MODE, bool GATHER>
void query_launch_ilp(int ilp, const QueryView& Q, const float* xyz, uint32_t sf, uint64_t n, uint32_t* row_out, float* h_out,
                      uint32_t* state_out, hipStream_t s) {
    if (ilp == 4) query_launch<4, MODE, GATHER>(Q, xyz, sf, n, row_out, h_out, state_out, s);
    else if (ilp == 2) query_launch<2, MODE, GATHER>(Q, xyz, sf, n, row_out, h_out, state_out, s);
    else query_launch<1, MODE, GATHER>(Q, xyz, sf, n, row_out, h_out, state_out, s);
}

int query_run(gndt_handle* h, const void* xyz_dev, size_t n, size_t stride_bytes, int32_t mode, uint32_t* row_out, float* h_out,
              uint32_t* state_out, hipStream_t s) {
    const QueryView Q = query_view(h);
    const float* xyz = static_cast<const float*>(xyz_dev);
    const uint32_t sf = (uint32_t)(stride_bytes / 4);
    const int ilp = tuning().query_ilp;
    const bool gather = h_out || state_out;
    if (mode == GNDT_QUERY_NODE) {
        if (gather) query_launch_ilp<kQueryNode, true>(ilp, Q, xyz, sf, n, row_out, h_out, state_out, s);
        else query_launch_ilp<kQueryNode, false>(ilp, Q, xyz, sf, n, row_out, nullptr, nullptr, s);
    } else {
        if (gather) query_launch_ilp<kQueryNearestSlope, true>(ilp, Q, xyz, sf, n, row_out, h_out, state_out, s);
        else query_launch_ilp<kQueryNearestSlope, false>(ilp, Q, xyz, sf, n, row_out, nullptr, nullptr, s);
    }
    HIP_TRY(h, hipGetLastError());
    return GNDT_OK;
}

}  // namespace

}  // namespace gndt_host

extern "C" {

int gndt_query_device(gndt_handle* h, const void* xyz_dev, size_t n, size_t stride_bytes, int32_t mode, uint32_t* row_out, float* h_out,
                      uint32_t* state_out, void* hip_stream) {
    int rc = check_ready(h);
    if (rc) return rc;
    const hipStream_t s = stream_of(h, hip_stream);
    rc = query_prepare(h, xyz_dev, n, stride_bytes, mode, row_out, h_out || state_out, s);
    if (rc || n == 0) return rc;
    return query_run(h, xyz_dev, n, stride_bytes, mode, row_out, h_out, state_out, s);
}

int gndt_query(gndt_handle* h, const void* xyz_host, size_t n, size_t stride_bytes, int32_t mode, uint32_t* row_out, float* h_out,
               uint32_t* state_out) {
    int rc = check_ready(h);
    if (rc) return rc;
    const hipStream_t s = h->own_stream;
    rc = query_prepare(h, xyz_host, n, stride_bytes, mode, row_out, h_out || state_out, s);
    if (rc || n == 0) return rc;
    IoPiece io[4] = {io_in(xyz_host, (uint64_t)n * stride_bytes),
                     io_out(row_out, (uint64_t)n * 4),
                     io_out(h_out, (uint64_t)n * 4),
                     io_out(state_out, (uint64_t)n * 4)};
    if ((rc = stage_in(h, io, s))) return rc;
    if ((rc = query_run(h, io[0].dev, n, stride_bytes, mode, io[1].as<uint32_t>(), io[2].as<float>(), io[3].as<uint32_t>(), s))) return rc;
    return stage_out(h, io, s);
}

}  // extern "C"
