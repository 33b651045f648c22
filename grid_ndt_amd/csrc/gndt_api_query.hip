// gndt_api_query.hip — batched point queries against the finished grid (gndt_query.hpp): the lookup of computeCost's goal
// (include/map2D.h:1291-1306) and findRoute's start / goal (include/GlobalPlan.h:56-61) for n points at once.
#include "gndt_handle.hpp"
#include "gndt_query.hpp"

using namespace gndt;
using namespace gndt_host;

namespace gndt_host {

void free_query(gndt_handle* h) {
    auto& q = h->query;
    void* ptrs[] = {q.ctab_key, q.ctab_val, q.d_cc, q.in, q.rows, q.h_bits, q.state};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    q = gndt_handle::Query{};
}

// What a query or a raster does before its kernel (the rules of include/gndt.h "point queries", stated once for both): no capture,
// a finished map (gndt_sync first finishes a pending build, a deferred emit, a re-run), a cost map of the current grid when gathered.
int query_sync(gndt_handle* h, bool gather, hipStream_t s, const char* capture_err) {
    {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        (void)hipStreamIsCapturing(s, &cap);
        if (cap != hipStreamCaptureStatusNone) { h->err = capture_err; return GNDT_ERR_INVALID; }
    }
    { const int prc = partition_resolve(h); if (prc) return prc; }
    if (!h->results_valid) { h->err = "no finished build to query (the lookups run on the map create2DMap made, receiver.cpp:160, 171)"; return GNDT_ERR_INVALID; }
    int rc = gndt_sync(h, nullptr, nullptr, nullptr);
    if (rc) return rc;
    if (gather && (h->cost.serial == 0 || h->cost.serial != h->result_serial)) {
        h->err = "no cost map for the current grid (call gndt_compute_cost after the build)";
        return GNDT_ERR_INVALID;
    }
    return GNDT_OK;
}

// The stream, then the column index for the current map (h->query: ctab_key / ctab_val / ctab_mask)
int query_index(gndt_handle* h, hipStream_t s) {
    int rc = use_stream(h, s);
    if (rc) return rc;
    // The column index: kept while the map is the one it was built for.  Not on a handle that has recorded a hipGraph: a replay rewrites
    // the map without the host's serial moving (gndt_compute_cost keeps its tables under the same rule).
    auto& q = h->query;
    const uint64_t rows = h->res_nodes, K = h->res_columns;
    const uint32_t tsize = pow2_ceil(std::max<uint64_t>(1024, 2 * K));     // the flood's rule (gndt_compute_cost): load <= 1/2
    if (q.serial && q.serial == h->result_serial && !h->ever_captured && q.ctab_mask == tsize - 1) return GNDT_OK;
    q.serial = 0;
    if (!q.d_cc) HIP_TRY(h, hipMalloc(&q.d_cc, sizeof(CostCounters)));
    if (tsize > q.ctab_cap) {
        if (q.ctab_key) (void)hipFree(q.ctab_key);
        if (q.ctab_val) (void)hipFree(q.ctab_val);
        q.ctab_key = nullptr; q.ctab_val = nullptr; q.ctab_cap = 0;
        HIP_TRY(h, hipMalloc(&q.ctab_key, (size_t)tsize * 8));
        HIP_TRY(h, hipMalloc(&q.ctab_val, (size_t)tsize * 4));
        q.ctab_cap = tsize;
    }
    q.ctab_mask = tsize - 1;
    // (k_cost_clear with no rows: the table's keys and the scratch counters; k_cost_columns' range_error is the flood's bound, not ours)
    hipLaunchKernelGGL(k_cost_clear, dim3(grid_for(tsize)), dim3(256), 0, s, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, q.ctab_key, tsize, q.d_cc);
    if (rows)
        hipLaunchKernelGGL(k_cost_columns, dim3(grid_for(rows)), dim3(256), 0, s, h->out.sx, h->out.sy, h->part.row_ncol, (uint32_t)rows,
                           q.ctab_key, q.ctab_val, q.ctab_mask, q.d_cc);
    HIP_TRY(h, hipGetLastError());
    q.serial = h->result_serial;
    return GNDT_OK;
}

// The rows, the column index and the cost map as the query kernels read them
QueryView query_view(gndt_handle* h) {
    QueryView Q{};
    Q.V.sx = h->out.sx; Q.V.sy = h->out.sy; Q.V.sz = h->out.sz;
    Q.V.mean = h->out.mean; Q.V.flags = h->out.flags; Q.V.rough = h->out.rough;
    Q.V.row_ncol = h->part.row_ncol;
    Q.V.ctab_key = h->query.ctab_key; Q.V.ctab_val = h->query.ctab_val; Q.V.ctab_mask = h->query.ctab_mask;
    Q.h_bits = h->cost.h_bits; Q.state = h->cost.state;
    Q.ox = h->origin[0]; Q.oy = h->origin[1]; Q.oz = h->origin[2];
    Q.grid_len = h->P.grid_len; Q.z_len = h->P.z_len;
    return Q;
}

namespace {

// A query buffer of `bytes` (the query's own: never recorded into a graph, so plainly freed — not retired)
template <typename T>
int query_alloc(gndt_handle* h, T*& p, uint64_t bytes) {
    if (p) (void)hipFree(p);
    p = nullptr;
    HIP_TRY(h, hipMalloc(&p, bytes));
    return GNDT_OK;
}

// Arguments, the finished map, the cost map when asked for (n == 0 stops there), the stream; then the column index for the current map.
int query_prepare(gndt_handle* h, const void* xyz, size_t n, size_t stride_bytes, int32_t mode, const uint32_t* row_out, bool gather,
                  hipStream_t s) {
    if (n && !xyz) { h->err = "gndt_query: null points"; return GNDT_ERR_INVALID; }
    if (n && !row_out) { h->err = "gndt_query: null row_out"; return GNDT_ERR_INVALID; }
    if (mode != GNDT_QUERY_NODE && mode != GNDT_QUERY_NEAREST_SLOPE) { h->err = "gndt_query: unknown mode"; return GNDT_ERR_INVALID; }
    if (stride_bytes != 12 && stride_bytes != 16) { h->err = "gndt_query: stride_bytes must be 12 or 16"; return GNDT_ERR_INVALID; }
    const int rc = query_sync(h, gather, s, "gndt_query: a query is not recorded into a hipGraph");
    if (rc || n == 0) return rc;
    return query_index(h, s);
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
    auto& q = h->query;
    const uint64_t in_bytes = (uint64_t)n * stride_bytes, out_bytes = (uint64_t)n * 4;
    if (in_bytes > q.in_cap) {
        q.in_cap = 0;
        if ((rc = query_alloc(h, q.in, in_bytes))) return rc;
        q.in_cap = in_bytes;
    }
    if (out_bytes > q.out_cap) {
        q.out_cap = 0;
        if ((rc = query_alloc(h, q.rows, out_bytes)) || (rc = query_alloc(h, q.h_bits, out_bytes)) || (rc = query_alloc(h, q.state, out_bytes)))
            return rc;
        q.out_cap = out_bytes;
    }
    HIP_TRY(h, hipMemcpyAsync(q.in, xyz_host, in_bytes, hipMemcpyHostToDevice, s));
    rc = query_run(h, q.in, n, stride_bytes, mode, q.rows, h_out ? reinterpret_cast<float*>(q.h_bits) : nullptr, state_out ? q.state : nullptr, s);
    if (rc) return rc;
    HIP_TRY(h, hipMemcpyAsync(row_out, q.rows, out_bytes, hipMemcpyDeviceToHost, s));
    if (h_out) HIP_TRY(h, hipMemcpyAsync(h_out, q.h_bits, out_bytes, hipMemcpyDeviceToHost, s));
    if (state_out) HIP_TRY(h, hipMemcpyAsync(state_out, q.state, out_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    return GNDT_OK;
}

}  // extern "C"
