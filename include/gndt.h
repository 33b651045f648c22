/* gndt.h — C ABI of the MI355X-native NDT grid builder (libgndt.so).
 *
 * This is the drop-in boundary for ONE path of daysun/grid_ndt: the two statements of
 * chatterCallback that build the map,
 *     for (i = 1 .. n-1) uniformDivision(points[i], false);     src/receiver.cpp:150-154
 *     map2D.create2DMap(demand);                                 src/receiver.cpp:160
 * i.e. point -> (xy Morton key, z level) binning (include/map2D.h:950-976, src/receiver.cpp:41-93),
 * the per-node mean / un-normalised scatter (map2D.h:611-627), the min-eigenpair that gives roughness
 * and normal (map2D.h:110-133) and the order-dependent slope label (map2D.h:66-108, 630-643).
 *
 * The reference has no FFI of its own (the path is a free function plus methods of a header-only
 * class working on a global `daysun::TwoDmap map2D`, receiver.cpp:35), so the entry points below are
 * what a binding for this path would need; each names the reference statement it replaces.
 * Plain pointers and sizes only; no C++ or torch types cross this boundary; nothing throws.
 *
 * Conventions kept from the reference:
 *   - point 0 of a cloud is the ORIGIN and is not binned (receiver.cpp:145, 150): call
 *     gndt_set_origin(h, &cloud[0]) and pass cloud+1, n-1 to gndt_build*.
 *   - inputs hold no NaN/Inf (the publisher strips them, src/publisher.cpp:24-26).
 *   - errors are status codes (the reference returns bool + prints, map2D.h:602-604).
 *   - one caller per handle at a time (ros::spin() is single-threaded, receiver.cpp:283).
 */
#ifndef GNDT_H
#define GNDT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gndt_handle gndt_handle;

enum {
    GNDT_OK = 0,
    GNDT_ERR_INVALID = 1,      /* bad argument / call order */
    GNDT_ERR_NO_DEVICE = 2,    /* no usable HIP device: the product path never falls back to the CPU */
    GNDT_ERR_HIP = 3,          /* a HIP runtime call failed; see gndt_last_error */
    GNDT_ERR_KEY_RANGE = 4,    /* |nx| or |ny| > 65535 (countMorton wraps, Stopwatch.h:102-110) or |nz| >= 2^21 */
    GNDT_ERR_CAPACITY = 5,     /* node table full and growth disabled */
    GNDT_ERR_NOMEM = 6,
    GNDT_ERR_PEER = 7          /* sharded builds: another rank of the communicator reported a failure; every rank left the
                                  collective sequence at the same point (this rank's own input was fine) */
};

enum { GNDT_DEMAND_SLOPE = 0, GNDT_DEMAND_TRUE = 1 };   /* create2DMap(demand), map2D.h:630, 644 */

/* gndt_cells.flags */
enum {
    GNDT_FLAG_HAS_STATS = 1u,  /* node reached min_points: mean/cov/N are set (map2D.h:611) */
    GNDT_FLAG_SLOPE = 2u,      /* a Slope object exists for the node (map2D.h:632 / :648) */
    GNDT_FLAG_DOWN = 4u        /* Slope::down (map2D.h:636) */
};

/* accumulate strategy (how points reach the per-node sufficient statistics) */
enum {
    GNDT_STRATEGY_AUTO = 0,
    GNDT_STRATEGY_ATOMIC = 1,     /* one pass, wave-aggregated fp64 atomics into the HBM node table */
    GNDT_STRATEGY_PARTITION = 2,  /* partition by column hash, then LDS-resident accumulation; large builds use the
                                     two-level partition without counting passes and fall back to the exact one */
    GNDT_STRATEGY_PARTITION_EXACT = 3,      /* always the single-level counting partition (histogram + offsets + scatter) */
    GNDT_STRATEGY_PARTITION_TWO_LEVEL = 4,  /* the two-level partition whatever the size (PARTITION picks it from 2^20 points) */
    GNDT_STRATEGY_PARTITION_ONE_LEVEL = 6,  /* (reported by gndt_last_strategy only) small clouds: one tile-sort level writes the
                                             * buckets directly; PARTITION / AUTO pick it when the cloud needs at most 512 buckets */
    GNDT_STRATEGY_PARTITION_BLOCKED = 7,    /* (reported by gndt_last_strategy only) the two partition levels with SPATIAL blocks of 512 nodes as
                                             * buckets and a bucket kernel that addresses its table directly (no index, no search): taken by AUTO /
                                             * PARTITION for clouds whose map is a dense, evenly filled box of bounded height (what the previous
                                             * build on the handle found), abandoned — the build re-run with hashed buckets — when a cloud outgrows it */
    GNDT_STRATEGY_TILE = 5        /* one pass for clouds that keep their scan order: contiguous ranges of the cloud, node table
                                     privatised in LDS per workgroup, ONE partial per distinct node and flush into the HBM node
                                     table (gndt_tile.hpp).  AUTO takes it when a sample of the cloud shows enough points per
                                     partial (gndt_locality_sample); like ATOMIC it keeps additive state (updates, statistics) */
};

typedef struct {
    float grid_len;         /* TwoDmap::gridLen  (setLen, map2D.h:493)   */
    float z_len;            /* TwoDmap::zLen     (setZLen, map2D.h:496)  */
    float slope_interval;   /* setInterval, map2D.h:499 */
    int32_t demand;         /* GNDT_DEMAND_* */
    int32_t min_points;     /* MINPOINTSIZE = 3, map2D.h:28 */
    int32_t device_id;      /* HIP device ordinal */
    int32_t strategy;       /* GNDT_STRATEGY_* */
    uint64_t max_points_hint;  /* largest batch expected (0 = grow on demand) */
    uint64_t max_nodes_hint;   /* occupied (xy,z) nodes expected (0 = derive from the batch size) */
} gndt_params;

/* Structure-of-arrays view of the finished map: one entry per occupied (xy,z) node — every OcNode of
 * map_xy, including those with fewer than min_points points (they keep zero mean/cov, map2D.h:54-56).
 * Order: columns in first-seen order (= morton_list, receiver.cpp:70), nodes of a column in
 * first-seen order (= insertion order among equal keys of the multimap, receiver.cpp:88).
 * 76 bytes per node.  Pointers are device or host memory depending on the call that filled them. */
typedef struct {
    uint64_t num_nodes;
    uint64_t num_columns;    /* = morton_list.size() */
    uint64_t num_slopes;
    int32_t* sx;             /* signed x index: +nx in quadrants A,B (px > ox), -nx in C,D */
    int32_t* sy;             /* signed y index: +ny in quadrants A,C (py > oy), -ny in B,D */
    int32_t* sz;             /* morton_z: signed z level, never 0 (map2D.h:963-973) */
    uint32_t* count;         /* points binned into the node */
    uint32_t* first_idx;     /* index (in the accumulated stream) of the node's first point */
    float* mean;             /* [num_nodes][3] OcNode::xyz_centroid / Slope::mean */
    float* cov;              /* [num_nodes][6] upper triangle xx,xy,xz,yy,yz,zz of covariance_matrix (un-normalised) */
    float* rough;            /* Slope::rough: min eigenvalue (0 -> 0.01, map2D.h:131) */
    float* normal;           /* [num_nodes][3] Slope::normal: its eigenvector, unit length, sign free */
    uint32_t* flags;         /* GNDT_FLAG_* */
} gndt_cells;

/* Per-node sufficient statistics (cell-local coordinates), the additive state exchanged between GPUs.
 * v = p - centre(node); centre is a pure function of (key, origin, grid_len, z_len). */
typedef struct {
    uint64_t num_nodes;
    uint64_t* key;           /* packed (sx,sy,sz), see gndt_pack_key */
    double* sums;            /* [num_nodes][9]: Sum v (3), Sum v v^T upper triangle (6) */
    uint32_t* count;
    uint32_t* first_idx;
} gndt_stats;

/* ---- lifetime ------------------------------------------------------------------------------- */
/* `TwoDmap map2D(res, zres)` + setInterval (receiver.cpp:35, 267-269) */
int gndt_create(const gndt_params* params, gndt_handle** out);
void gndt_destroy(gndt_handle* h);
const char* gndt_last_error(const gndt_handle* h);   /* h may be NULL: last error of a failed create */

/* `map2D.setCloudFirst(points[0])` (receiver.cpp:145, map2D.h:490) */
int gndt_set_origin(gndt_handle* h, const float origin_xyz[3]);
/* The origin in use (gndt_build_cloud takes it from the first valid point of the cloud). */
int gndt_get_origin(const gndt_handle* h, float origin_xyz[3]);

/* ---- build: replaces receiver.cpp:150-154 + :160 --------------------------------------------- */
/* Host memory in (e.g. pcl::PointCloud<PointXYZ>::points.data()+1, stride 16).  Synchronous. */
int gndt_build(gndt_handle* h, const void* xyz_host, size_t n, size_t stride_bytes);
/* Device memory in; all work is enqueued on `hip_stream` (a hipStream_t, may be NULL = the handle's own
 * NON-BLOCKING stream: work the caller has on the null stream is not ordered with it — a caller that fills its input on the
 * null stream passes hipStreamLegacy, the null stream's explicit name, instead).  stride_bytes is 12 (packed) or 16 (PointXYZ).
 * Partition strategies: the call returns once everything is enqueued.  The device-side overflow flags are read by
 * the next call that needs the result (gndt_sync, gndt_export*, gndt_compute_cost, ...), which waits for the
 * stream and, if a table or region was too small, re-runs the build with more room — so `xyz_dev` must stay valid
 * and unchanged until then (a later gndt_build* / gndt_reset on the handle abandons the pending build instead).
 * A PARTITION build captured in a hipGraph and replayed is not watched by the host: if the replayed cloud needs more room than
 * the captured one (LDS tables, partition regions, staging rows), gndt_sync reports GNDT_ERR_CAPACITY — build that cloud
 * eagerly, then capture again.
 * Strategies ATOMIC and TILE wait for the stream once before returning (and grow the table themselves) — except on a stream
 * under hipGraph capture, where they are recorded once for the table as it stands and a replay that outgrows it reports
 * GNDT_ERR_CAPACITY at gndt_sync.  AUTO picks per cloud (ATOMIC below 65 536 points; above, TILE when a sample of the
 * cloud shows dense scan-ordered cells, PARTITION otherwise); under capture it keeps the choice of the last eager build. */
int gndt_build_device(gndt_handle* h, const void* xyz_dev, size_t n, size_t stride_bytes, void* hip_stream);
/* Allocate NOW every buffer a build / update of up to max_points points and max_nodes nodes (0: max_points / 4) can ask for,
 * whatever the strategy and whatever a re-run with more room would want.  After it such a build allocates nothing: it can be
 * captured into a hipGraph on a FRESH handle (no eager warm-up), and no replay finds its buffers moved.  Without it a captured
 * call that has to grow a buffer fails with GNDT_ERR_CAPACITY before touching the allocator (allocating on a capturing stream
 * would invalidate the capture — and, on this runtime, every later capture of the process).  Waits for the handle's stream.
 * On a handle that holds a map the map stays: the node table and the result rows keep their contents when they grow; where the
 * column order's buffers had to move, the rows of a map in the table are made again from it before the call returns, and the next
 * gndt_update* relabels every column. */
int gndt_reserve(gndt_handle* h, uint64_t max_points, uint64_t max_nodes);
/* The reference builds ONE map per process (receiver.cpp:137-160): what its user sees is the FIRST build of a process, not the
 * steady state.  HIP resolves a kernel's code at its first launch and every buffer is allocated on first use; on a 200 k-point frame
 * that made the first build 0.4-1.0 ms against 0.05 ms for the next one.  gndt_warmup takes both out of the first build:
 *   1. it runs a synthetic cloud of `expected_points` points (0: params.max_points_hint, else 200 000; at most 4 M) through every
 *      strategy family a build on this handle can take — AUTO's locality sample, the partition pipeline at that size, its exact
 *      fallback, ATOMIC, TILE, an incremental update, the export and a cost flood — on a TEMPORARY handle with this handle's
 *      parameters, device and stream, so that the kernels' code is loaded (process-wide, per device) and this handle's state
 *      stays that of a fresh handle;
 *   2. if params.max_points_hint (or expected_points) is set, it calls gndt_reserve(h, that, params.max_nodes_hint).
 * Waits for the device.  Not under stream capture.  Costs 5-40 ms, once; calling it again is cheap (the code is loaded). */
int gndt_warmup(gndt_handle* h, uint64_t expected_points);

/* Incremental add (the intent of changeCallback/change2DMap, receiver.cpp:179-212, map2D.h:672-822;
 * semantics defined in SURVEY.md Appendix A.7): after update(F1) .. update(Fk) the map equals
 * build(F1 || .. || Fk).  first_idx continues counting across calls.  Needs a handle of strategy ATOMIC (the node
 * table keeps the additive state).  gndt_update_device never waits for the host: every size it needs lives on the
 * device, so once the buffers exist (one eager frame, or max_nodes_hint + max_points_hint) the call can be captured
 * in a hipGraph and replayed per frame; table / row / index overflow is reported by gndt_sync.
 * Point indices (first_idx) are 32-bit: a map holds at most 2^32 - 2 points between two gndt_reset calls (about an hour of
 * a 10 Hz, 131 072-point stream); the next update then fails with GNDT_ERR_INVALID instead of wrapping. */
int gndt_update(gndt_handle* h, const void* xyz_host, size_t n, size_t stride_bytes);
int gndt_update_device(gndt_handle* h, const void* xyz_dev, size_t n, size_t stride_bytes, void* hip_stream);
/* Stream-friendly mode (off by default).  The dense rows in the reference's order move whenever a column in front of them grows, so
 * producing them costs O(map) per frame however little the frame touched.  With deferred emit on, gndt_update* relabels the touched
 * columns and stops — O(touched) — and the rows are ordered and emitted by the next call that READS the map (gndt_sync,
 * gndt_export*, gndt_compute_cost): a node that integrates frames at 10 Hz and plans once a second pays for the dense form once a
 * second.  Results are those of the default mode (tests: a 100-frame stream equals one build of its points in both). */
int gndt_set_deferred_emit(gndt_handle* h, int on);

/* Incremental delete: the intent of del2DMap (include/map2D.h:826-915; its caller delCallback is commented out at
 * src/receiver.cpp:214-248, and the shipped merge formula is inconsistent: SURVEY row a10), DEFINED here as the inverse of
 * gndt_update: the given points — which must have been added before, with the same coordinates — leave their nodes.
 *   - counts and the additive statistics are exactly those of the stream without the points (sums up to fp64 rounding);
 *   - a node whose last point leaves is deleted (map2D.h:861-873) and takes its slope with it;
 *   - a node that falls below min_points keeps its key and count but no statistics, like a node that never reached them;
 *   - every surviving node KEEPS its first-seen index, i.e. its place in the order — the reference's containers do not
 *     re-sort either (multimap::erase, morton_list untouched).  The result therefore equals a fresh build of the remaining
 *     points whenever no surviving node lost its first point; otherwise the order (and with it the order-dependent slope
 *     label, map2D.h:66-108) is that of the ORIGINAL stream.
 * Needs the additive state (strategy ATOMIC / TILE or a map built by gndt_update*).  A point that was never added is an
 * error (GNDT_ERR_INVALID) and leaves the handle to be reset.  Waits for the device (the node table is compacted when
 * nodes died); every row is re-finalised. */
int gndt_remove(gndt_handle* h, const void* xyz_host, size_t n, size_t stride_bytes);
int gndt_remove_device(gndt_handle* h, const void* xyz_dev, size_t n, size_t stride_bytes, void* hip_stream);

/* Split form of build for a cloud sharded over several GPUs:
 *   accumulate (binning + sufficient statistics only)  ->  [exchange stats]  ->  finalize.
 * `first_idx_base` is the global index of xyz_dev[0] so that first-seen order is global. */
int gndt_reset(gndt_handle* h, void* hip_stream);
int gndt_accumulate_device(gndt_handle* h, const void* xyz_dev, size_t n, size_t stride_bytes,
                           uint64_t first_idx_base, void* hip_stream);
int gndt_finalize_device(gndt_handle* h, void* hip_stream);

/* ---- results --------------------------------------------------------------------------------- */
/* Waits for the handle's pending work, reports counts and any deferred device-side error. */
int gndt_sync(gndt_handle* h, uint64_t* num_nodes, uint64_t* num_columns, uint64_t* num_slopes);
/* Device-resident SoA of the last build/finalize; valid until the next build/update/remove/crop/clear/destroy. */
int gndt_export_device(gndt_handle* h, gndt_cells* out);
/* Copies into caller-allocated host arrays sized from gndt_sync's num_nodes (NULL arrays skipped). */
int gndt_export(gndt_handle* h, gndt_cells* out_host);
/* The same rows in host memory the HANDLE owns (pinned, one D2H pass, no copy into caller arrays): the pointers stored in *out
 * stay valid until the next gndt_export_host / gndt_destroy on the handle.  What gndt_compat::TwoDmap reads the map from
 * (the reference's containers are filled from it, or — lazy mode — the consumers are served from it directly). */
int gndt_export_host(gndt_handle* h, gndt_cells* out);

/* ---- statistics exchange (multi-GPU; additive over any partition of the points) --------------- */
/* Device-resident compact list of this handle's occupied nodes. */
int gndt_stats_export_device(gndt_handle* h, gndt_stats* out, void* hip_stream);
/* Adds `in` (device memory) into the handle's table: sums add, counts add, first_idx takes the min. */
int gndt_stats_merge_device(gndt_handle* h, const gndt_stats* in, void* hip_stream);

/* One global map from a cloud sharded over several GPUs, without the node table:
 *   gndt_shard_stats_device   this rank's shard -> compact statistics of its occupied nodes (the counting
 *                             partition + LDS bucket pipeline of a normal build, statistics out instead of rows);
 *                             `first_idx_base` = global index of xyz_dev[0].  Returns with `out` filled.
 *   [exchange: union of keys, sum of sums/counts, min of first_idx — grid_ndt_amd/dist.py over RCCL]
 *   gndt_finalize_stats_device  the merged statistics -> the map.  `in` must hold every node once, SORTED BY KEY
 *                             (any total order of the packed keys: a column's nodes are then adjacent);
 *                             `total_points` = number of points of the whole cloud (first_idx < total_points). */
int gndt_shard_stats_device(gndt_handle* h, const void* xyz_dev, size_t n, size_t stride_bytes, uint64_t first_idx_base,
                            gndt_stats* out, void* hip_stream);
int gndt_finalize_stats_device(gndt_handle* h, const gndt_stats* in, uint64_t total_points, void* hip_stream);

/* The whole sharded build behind the C ABI, RCCL called from C++ (resolved with dlopen: single-GPU users do not need it):
 * one process per GPU, every rank calls gndt_build_global_device with ITS contiguous range of the cloud; on return every
 * rank's handle holds the map of the whole cloud (origin = the global cloud's point 0 on every rank).
 *   shard -> statistics | all-gather of the occupied keys -> canonical order | ONE packed all-reduce (9 sums + count, fp64)
 *   + one min all-reduce (first-seen) | finalize from the reduced statistics.
 * The communicator: rank 0 calls gndt_comm_unique_id and hands the 128 bytes to the other ranks by its own means (a file,
 * MPI, torch.distributed ...); every rank then calls gndt_comm_create. */
#define GNDT_COMM_ID_BYTES 128
typedef struct gndt_comm gndt_comm;
typedef struct {
    float shard_ms, exchange_ms, finalize_ms;     /* device time of the three stages (HIP events on the stream) */
    uint32_t ranks;
    uint64_t local_nodes, global_nodes, bytes_reduced;
} gndt_exchange_times;
int gndt_comm_unique_id(char id_out[GNDT_COMM_ID_BYTES]);
int gndt_comm_create(const char id[GNDT_COMM_ID_BYTES], int32_t rank, int32_t world, int32_t device_id, gndt_comm** out);
/* `world` communicators whose ranks are THREADS of this process (one handle and one calling thread per rank, any devices
 * that can copy to each other — normally one): gndt_build_owned_device then hands the runs over with device copies and host
 * barriers instead of RCCL.  One GPU can play a whole node (the tests do), and a process that drives several handles from
 * several threads needs no RCCL.  Every rank must make every call; destroy each communicator. */
int gndt_comm_create_threads(int32_t world, int32_t device_id, gndt_comm** out /* [world] */);
void gndt_comm_destroy(gndt_comm* c);
const char* gndt_comm_last_error(void);
/* One tiny, VERIFIED round of every collective the sharded builds use — all-gather, the all-to-all of runs (ncclSend / ncclRecv in
 * one group), reduce-scatter, all-reduce (f64 sum, u32 min) — on communicator `c`, all ranks calling together.  ok_mask: bit 0
 * all-gather, 1 send/recv, 2 reduce-scatter, 3 all-reduce; times include the host copies that carry the test data.  Returns GNDT_OK
 * only if every primitive gave the right answer on this rank (GNDT_ERR_PEER and gndt_last_error(h) name the wrong one).  Run it
 * once before the first sharded build of a job: that build is otherwise the first test of the transport. */
typedef struct {
    float all_gather_ms, exchange_ms, reduce_scatter_ms, all_reduce_ms;
    uint32_t ok_mask, ranks;
} gndt_comm_selftest_report;
int gndt_comm_selftest(gndt_handle* h, gndt_comm* c, gndt_comm_selftest_report* out, void* hip_stream);
/* first_idx_base = index of shard[0] in the whole cloud's binned points; total_points = binned points of the whole cloud.
 * `times` may be NULL (it makes the call wait for the stream). */
int gndt_build_global_device(gndt_handle* h, gndt_comm* c, const void* shard_xyz_dev, size_t n, size_t stride_bytes,
                             uint64_t first_idx_base, uint64_t total_points, gndt_exchange_times* times, void* hip_stream);

/* ---- owner-partitioned build of a sharded cloud: the POINTS travel, statistics do not ----------------------------
 * No reference counterpart (the reference is single-process).  Every column of the grid has an owner rank (a hash of its
 * xy cell); each rank sends every point to the owner of its column (all-to-all, 16 B per point, consecutive identical points
 * folded into weighted records first), builds the columns it owns with the ordinary pipeline — statistics, labels and rows
 * are final — and learns, from an all-gather of 8 B per column, which row each of its rows has in the map of the WHOLE
 * cloud.  The map stays sharded by owner:
 *     gndt_export* on the handle   = this rank's columns, in the reference's order among themselves
 *     global_row[r]                = the row that local row r has in the single-process map of the whole cloud
 * so the union of all ranks' rows scattered by global_row IS that map (tests/test_gpu_owner.py assembles it and compares it
 * with the oracle).  Per rank a build moves (W-1)/W of its points out and as many in; gndt_build_global_device moves 84 B per
 * node of the global map through an all-reduce and leaves the whole map on every rank.
 *
 * gndt_build_owned_device does all of it over RCCL.  The four steps are also exported one by one for hosts that bring their
 * own transport (MPI, a ROS bridge) and for the single-GPU tests that play W ranks on one device:
 *   gndt_owner_split_device    shard -> records grouped by owner: rank r's run is counts_host[r] records of 16 bytes starting
 *                              offsets_host[r] records into *records_dev (the runs need not be adjacent; valid until the
 *                              next call on the handle); waits for the stream
 *   gndt_build_records_device  the records a rank owns (runs of all ranks, concatenated in any order) -> its map; like
 *                              gndt_build_device it is launched, not awaited.  total_points = binned points of the whole cloud
 *   gndt_owned_columns_device  (first-seen index << 32 | node count) per column of the local map; waits
 *   gndt_owned_global_rows_device  everybody's pairs (any order, entries of ~0 are skipped) -> global_row of every local row
 *                              (device pointer, valid until the next build), node / column count of the whole map; waits */
typedef struct gndt_owned_info {
    uint64_t owned_points;          /* records this rank received (weighted records count once) */
    uint64_t local_nodes, local_columns;
    uint64_t global_nodes, global_columns, global_slopes;
    uint64_t bytes_sent, bytes_received;   /* over the links (the run a rank keeps for itself is not counted) */
    float split_ms, exchange_ms, build_ms, order_ms;   /* device time of the stages (HIP events on the stream) */
    uint32_t ranks;
} gndt_owned_info;
/* owner rank of the columns (sx[i], sy[i]) among `world` ranks: the hash gndt_owner_split_device uses (host helper, no GPU) */
int gndt_owner_of_columns(const int32_t* sx, const int32_t* sy, size_t n, uint32_t world, uint32_t* owner_out);
/* Optional, before the split — locality-aware ownership (gndt_build_owned_device does it by itself): a contiguous range of a
 * scan-ordered cloud covers a patch of ground, so a block of 32 x 32 columns is given to the rank that already holds most
 * of its points and those points never cross a link.
 *   gndt_owner_sample_device  65 536 evenly spaced points of the shard -> a fixed-size message (device pointer, 32-bit words)
 *   gndt_owner_map_device     the messages of ALL ranks, concatenated in rank order -> the block table kept on the handle and
 *                             used by gndt_owner_split_device calls for the same `world` until replaced.  Every rank must
 *                             build it from the same messages (it then holds the same table); columns of blocks the
 *                             samples missed, or of a block holding more than 1/(4 world) of the cloud, go by the hash.
 * Without these two calls (or with world > 16) ownership is gndt_owner_of_columns' hash. */
int gndt_owner_sample_device(gndt_handle* h, const void* shard_xyz_dev, size_t n, size_t stride_bytes, const uint32_t** msg_dev,
                             uint64_t* msg_words, void* hip_stream);
int gndt_owner_map_device(gndt_handle* h, const uint32_t* all_msgs_dev, uint32_t world, void* hip_stream);
int gndt_owner_split_device(gndt_handle* h, const void* shard_xyz_dev, size_t n, size_t stride_bytes, uint64_t first_idx_base,
                            uint64_t total_points, uint32_t world, const void** records_dev, uint64_t* counts_host,
                            uint64_t* offsets_host, void* hip_stream);
int gndt_build_records_device(gndt_handle* h, const void* records_dev, size_t n_records, uint64_t total_points, void* hip_stream);
/* The same from TWO segments, so that the run a rank keeps for itself need not be copied next to what it receives: the
 * second segment must be preceded, in its own allocation, by room for the n_first records of the first (only small builds,
 * which partition one array, fill that room). */
int gndt_build_records2_device(gndt_handle* h, const void* first_dev, size_t n_first, void* second_dev, size_t n_second,
                               uint64_t total_points, void* hip_stream);
int gndt_owned_columns_device(gndt_handle* h, const uint64_t** pairs_dev, uint64_t* n_pairs, void* hip_stream);
int gndt_owned_global_rows_device(gndt_handle* h, const uint64_t* all_pairs_dev, uint64_t n_all, uint64_t total_points,
                                  const uint32_t** global_row_dev, uint64_t* global_nodes, uint64_t* global_columns, void* hip_stream);
int gndt_build_owned_device(gndt_handle* h, gndt_comm* c, const void* shard_xyz_dev, size_t n, size_t stride_bytes,
                            uint64_t first_idx_base, uint64_t total_points, const uint32_t** global_row_dev,
                            gndt_owned_info* info, void* hip_stream);
/* Errors inside the collective sequence of gndt_build_owned_device / gndt_build_global_device: a rank that fails on its own
 * (bad input, a point outside the key range, a build that does not fit) still takes part in the collectives that follow, its
 * error code travelling with the messages that are exchanged anyway; every rank that sees a non-zero code leaves at the same
 * point — the failing rank with its own error, the others with GNDT_ERR_PEER — so no rank is left waiting.  Not reportable
 * this way, hence fatal for the group like the loss of a rank: a failing collective, and memory exhaustion for the exchange
 * buffers themselves.
 *
 * ---- one map for the consumers (src/receiver.cpp:171-175 runs computeCost and the planner on ONE map)
 * After gndt_build_owned_device the map is sharded by column owner.  gndt_gather_owned_map_device moves the finished rows —
 * 84 bytes each: the 76-byte row of gndt_cells, the column index the cost map uses, and the row's place in the map of the
 * whole cloud — to rank `root` (ncclSend / ncclRecv) or, with root < 0, to every rank (one padded all-gather), and scatters
 * them by that place into the handle's result arrays: the handle then HOLDS THE WHOLE MAP, in the reference's order, and
 * gndt_sync / gndt_export* / gndt_compute_cost / gndt_compat::TwoDmap work on it as after a single-GPU build.  Ranks other
 * than `root` keep the columns they own.  All ranks of the communicator call it, after a successful gndt_build_owned_device,
 * ONCE per build (a second call fails with GNDT_ERR_INVALID on every rank, before any collective).
 * For hosts with their own transport the two device steps are exported:
 *   gndt_owned_pack_rows_device   this rank's rows as packed records (GNDT_PACKED_ROW_WORDS 32-bit words each; device pointer
 *                                 valid until the next call on the handle)
 *   gndt_adopt_rows_device        packed records of ANY number of ranks (padding records, last word 0xFFFFFFFF, are skipped)
 *                                 -> the handle's result rows; fails with GNDT_ERR_INVALID unless exactly total_nodes rows
 *                                 arrive. */
#define GNDT_PACKED_ROW_WORDS 21
int gndt_gather_owned_map_device(gndt_handle* h, gndt_comm* c, int32_t root, void* hip_stream);
int gndt_owned_pack_rows_device(gndt_handle* h, const uint32_t** rows_dev, uint64_t* n_rows, void* hip_stream);
int gndt_adopt_rows_device(gndt_handle* h, const uint32_t* rows_dev, uint64_t n_rows, uint64_t total_nodes, uint64_t total_columns,
                           uint64_t total_slopes, void* hip_stream);

/* ---- cost map over the finished grid -------------------------------------
 * gndt_compute_cost replaces TwoDmap::computeCost (include/map2D.h:1285-1397; called at receiver.cpp:171
 * right after create2DMap): the FIFO flood from the goal slope with CollisionCheck (:351-411; the 3D variants
 * :414-474 when the handle's demand is "true") and AccessibleNeighbors (:530-588).  It fills, per result row,
 *   h      Slope::h  (FLT_MAX where the row has no Slope, was never reached, or collided and was not relaxed again)
 *   state  0 = untouched, 1 = traversable (the reference's `traversability` list), 2 = closed (collision)
 * bit-identical to the reference's sequential flood on the same grid (DESIGN.md "Cost map").
 * The call returns when the flood is complete.  Column indices must not exceed 32767 (mortonToXY's range,
 * Stopwatch.h:171-189).  The flood builds or reuses the map's column index, which point queries, rasters and clears share.  `robot` NULL = RobotSphere(0.25) with robot.h:38-46's thresholds. */
typedef struct gndt_robot {
    float radius;            /* RobotSphere::r            receiver.cpp:33  */
    float reachable_height;  /* getReachableHeight() 0.15  robot.h:38-39   */
    float max_rough;         /* getRough() 100             robot.h:40-43   */
    float max_angle_deg;     /* getAngle() 30              robot.h:44-46   */
} gndt_robot;

typedef struct gndt_cost_stats {
    int32_t goal_status;     /* 0 flood ran; 1 no cell at the goal (reference: nothing happens); 2 no slope at the
                                goal's level ("Goal position wrong", map2D.h:1304-1306) */
    uint32_t ring;           /* n = (ceil(2r/gridLen)-1)/2, the collision ring depth (map2D.h:1310) */
    uint32_t levels;         /* layers of the flood */
    uint32_t ring_store;     /* 0: no collision ring (robot no wider than a cell); 1: the rings' verdicts came from `ring` rounds of
                                neighbour propagation over the whole map before the flood (no ring is listed, no capacity) */
    uint64_t traversable;    /* traversability.size() (map2D.h:1382) */
    uint64_t closed;         /* slopes closed by a collision */
    uint64_t check_pushes;   /* checkList.size() (map2D.h:1383) */
} gndt_cost_stats;

int gndt_compute_cost(gndt_handle* h, const float goal_xyz[3], const gndt_robot* robot, void* hip_stream);
/* Device-resident h (fp32) and state (u32) per result row; valid until the next build/update/crop/compute_cost. */
int gndt_cost_export_device(gndt_handle* h, const float** h_dev, const uint32_t** state_dev, gndt_cost_stats* stats);
/* Copies into caller-allocated host arrays of num_nodes elements (NULL arrays skipped). */
int gndt_cost_export(gndt_handle* h, float* h_out, uint32_t* state_out, gndt_cost_stats* stats);

/* ---- route planning: A* routes to the flood's goal for a batch of starts ---------------------------------
 * gndt_plan_routes* replaces AstarPlanar::findRoute (include/GlobalPlan.h:49-166; receiver.cpp:172-176, right after computeCost) for K
 * starts at once, on the device, against the current cost map.  Per start the route is what findRoute returns on a FRESH map (every
 * slope g = f = FLT_MAX, no father, an empty queue and closed list) whose Slope::h is the cost map — slope for slope, with the
 * reference's quirks (DESIGN.md §4.3j "Route planning" lists them).  Queries of a batch are independent of each other and of earlier calls.
 *   start   the row GNDT_QUERY_NODE finds for the point, if it has GNDT_FLAG_SLOPE (GlobalPlan.h:56-64); start_mode
 *           GNDT_QUERY_NEAREST_SLOPE uses that rule instead.  None: status GNDT_ROUTE_NO_START (a non-finite coordinate, a key out of
 *           range, no such node, a node without a slope).
 *   goal    the slope the last gndt_compute_cost seeded.  If that flood's goal_status was not 0, every query gets GNDT_ROUTE_NO_GOAL
 *           and no search runs.
 *   robot   the last flood's (AccessibleNeighbors comand 2.5; 4, which also evaluates Slope::countUp, on a demand-"true" handle).
 * Per query, gndt_route_info: status; length, the slopes of the route (start and goal included; 0 without a route); start_row;
 * expansions, the slopes popped and expanded (a slope popped again through a stale second queue entry counts again); queue_peak, the
 * most entries the open queue held; cost, g of the goal (FLT_MAX without a route); h_start, the cost map's h at the start (FLT_MAX
 * without one).  route_rows[k * route_cap ..]: the route of query k as rows of gndt_cells, START FIRST, GOAL LAST; a route longer than
 * route_cap writes its first route_cap rows (the caller sees length > route_cap), unused entries are GNDT_NO_ROW.  route_rows may be
 * NULL with route_cap 0: only the info is written.
 * The guard: a query that has expanded max_expansions slopes (0 = 4 * num_slopes + 1024) without popping the goal ends with
 * GNDT_ROUTE_LIMIT and no route — the loop's bound is not obvious and the device is shared.  So does a query whose open queue holds
 * more than 2 * num_slopes + 1024 live entries at once (its LDS and spill tiers together; the reference's queue is bounded by nothing
 * but its expansions, which the guard bounds).
 * Per-query state (g, f, father, closed per row; the queue's spill) lives in a scratch area the handle owns and grows: 16 bytes a row
 * and 8 a queue entry per query.  Queries that do not fit params->scratch_bytes (0 = 256 MiB) together run in consecutive launches on
 * the same stream; GNDT_ERR_CAPACITY if a single query does not fit.
 * Needs a cost map of the current grid (the condition of gndt_cost_export) and the tables its flood kept, which a handle that has
 * recorded a hipGraph does not keep.  The map, h and state are not modified.  Like queries and casts the call is enqueued and not
 * awaited (gndt_plan_routes: synchronous), returns GNDT_OK and launches nothing for K == 0, and has no CPU path.
 * GNDT_ERR_INVALID: a null handle or params, null starts or info with K > 0, K >= 2^31, a stride other than 12 / 16, an unknown
 * start_mode, a non-zero reserved word, route_rows NULL with route_cap > 0 or the reverse (K > 0), no finished build, no current cost map (none,
 * or made stale by a build / update / remove / crop since), the flood's tables not kept, a stream under hipGraph capture. */
enum { GNDT_ROUTE_FOUND = 0, GNDT_ROUTE_NO_START = 1, GNDT_ROUTE_NO_ROUTE = 2, GNDT_ROUTE_LIMIT = 3, GNDT_ROUTE_NO_GOAL = 4 };
typedef struct gndt_plan_params {
    int32_t start_mode;       /* GNDT_QUERY_NODE (0, the reference's lookup) or GNDT_QUERY_NEAREST_SLOPE */
    uint32_t max_expansions;  /* 0 = 4 * num_slopes + 1024 */
    uint64_t scratch_bytes;   /* 0 = 256 MiB */
    uint32_t reserved[4];     /* 0 */
} gndt_plan_params;           /* zeros = defaults */
typedef struct gndt_route_info {
    int32_t status;
    uint32_t length, start_row, expansions, queue_peak;
    float cost, h_start;
    uint32_t reserved;
} gndt_route_info;            /* 32 bytes */
/* Device memory in and out: starts (stride 12 or 16), route_rows [K * route_cap], info [K]; enqueued on `hip_stream` (NULL = the
 * handle's stream) and not awaited.  info_dev must be 16-byte aligned (the kernel writes a record as two 16-byte stores; what hipMalloc
 * returns is): GNDT_ERR_INVALID otherwise.  The host entry point below takes any alignment. */
int gndt_plan_routes_device(gndt_handle* h, const void* starts_dev, size_t K, size_t stride_bytes, const gndt_plan_params* params,
                            uint32_t* route_rows_dev, uint32_t route_cap, gndt_route_info* info_dev, void* hip_stream);
/* Host memory in and out; returns when the answers are in place. */
int gndt_plan_routes(gndt_handle* h, const void* starts_host, size_t K, size_t stride_bytes, const gndt_plan_params* params,
                     uint32_t* route_rows_host, uint32_t route_cap, gndt_route_info* info_host);

/* ---- point queries against the finished grid --------------------------------------------------------
 * The lookup the reference writes out wherever a consumer needs the slope at a position:
 *     transMortonXYZ(p) -> map_cell.find(morton_xy) -> map_slope.find(morton_z)
 * (the goal of computeCost, map2D.h:1291-1306; start and goal of AstarPlanar::findRoute, GlobalPlan.h:56-61), for n points at once,
 * on the device, against the rows gndt_export* hands out.  Per point the answer is a row number (gndt_cells order) or GNDT_NO_ROW.
 *   GNDT_QUERY_NODE           the row whose (sx, sy, sz) is point_key(p): the key the build gives the point (transMortonXYZ,
 *                             map2D.h:950-976, from the handle's origin, grid_len and z_len).  ANY node counts — also one below
 *                             min_points or without a slope: map_xy's view.  The reference's goal / start lookup (map2D.h:1293-1306,
 *                             GlobalPlan.h:56-61: map_cell.find, then map_slope.find(morton_z)) is "a NODE row whose flags have
 *                             GNDT_FLAG_SLOPE": a row without that flag is the reference's "Goal position wrong".
 *   GNDT_QUERY_NEAREST_SLOPE  only the column (sx, sy) is keyed (z only has to be finite): among its rows with GNDT_FLAG_SLOPE the
 *                             one with the least fabsf(mean_z - p.z) in fp32, a tie going to the smaller sz; GNDT_NO_ROW if the column
 *                             has no slope.  The slope under a robot whose pose z need not fall into the slope's level (the reference
 *                             needs it to: findRoute finds no start otherwise, hence receiver.cpp:257-266's hand-tuned pos / goal).
 * A point with no answer is a normal question, not an error: GNDT_NO_ROW for a non-finite coordinate (tested before keying), a key
 * outside the codec's range (|nx|, |ny| > 65535; in NODE mode also |nz| >= 2^21) and a column or node the map does not hold.
 * h_out / state_out may be NULL; when given they receive the cost map's h / state of the row (FLT_MAX / 0 for GNDT_NO_ROW) and need
 * a cost map of the current grid (the condition of gndt_cost_export).
 * GNDT_ERR_INVALID: null handle, null xyz or row_out with n > 0, unknown mode, stride other than 12 / 16, no finished build, h_out /
 * state_out without a current cost map, a stream under hipGraph capture (queries are not recorded).  There is no CPU path: without a
 * device the call fails like every compute entry point.  n == 0 returns GNDT_OK and launches nothing.
 * Order: the call first finishes what gndt_compute_cost finishes (a pending build, a deferred emit, a re-run: gndt_sync), then builds
 * or reuses the map's column index, which the flood, rasters and clears share — rebuilt after every build / update / remove, and on
 * every call on a handle that has recorded a hipGraph (a replay rewrites the map unseen) — and enqueues one kernel.  Row numbers stay valid until the next build, update, remove,
 * crop or reset.  A sharded map answers from the rows this rank holds. */
enum { GNDT_QUERY_NODE = 0, GNDT_QUERY_NEAREST_SLOPE = 1 };
#define GNDT_NO_ROW 0xFFFFFFFFu
/* Device memory in and out (stride 12 or 16, like gndt_build_device); enqueued on `hip_stream` (NULL = the handle's stream, the rules
 * of gndt_build_device) and not awaited: the outputs are valid once that stream reaches them. */
int gndt_query_device(gndt_handle* h, const void* xyz_dev, size_t n, size_t stride_bytes, int32_t mode,
                      uint32_t* row_out, float* h_out, uint32_t* state_out, void* hip_stream);
/* Host memory in and out; synchronous. */
int gndt_query(gndt_handle* h, const void* xyz_host, size_t n, size_t stride_bytes, int32_t mode,
               uint32_t* row_out, float* h_out, uint32_t* state_out);

/* ---- region crop: whole columns leave the map, without their points -------------------------------------------------------
 * A rolling window around a robot (keep the columns inside a box) or an area cleared for re-mapping (drop the columns inside it).
 * The region is an inclusive box of SIGNED column indices (gndt_cells.sx / sy).  Signed indices skip 0 and point_key's axis index is
 * monotone in the coordinate, so an index range is a contiguous strip of the world.  min > max on either axis is GNDT_ERR_INVALID.
 *   GNDT_CROP_KEEP_INSIDE   every node whose (sx, sy) lies OUTSIDE the box leaves the map (the rolling window)
 *   GNDT_CROP_DROP_INSIDE   every node whose (sx, sy) lies INSIDE the box leaves the map
 * A node leaves with everything it has (count, statistics, slope, labels), whether or not it reached min_points or holds a slope.
 * Labels only look at nodes of their own column (isSlope, map2D.h:66-108), so every surviving row is BIT-IDENTICAL in all eleven
 * gndt_cells fields and keeps its place relative to the other survivors: the export after the crop is the export before it, filtered
 * by (sx, sy); num_nodes, num_columns and num_slopes are recounted.  No row is finalised again.
 * The stream position is kept: the next gndt_update* numbers its points after everything ever added, and a dropped column that
 * receives points again is a new column (first_idx = that of its new first point).  Hence, by definition,
 *     crop(R)  ==  gndt_remove of every point added so far that lies in a column R drops.
 * Any map the handle holds rows for can be cropped, whatever built it.  A map held in the node table (strategies ATOMIC / TILE, maps
 * built by gndt_update*) leaves the table as well, so updates and removes go on afterwards; the next update then re-finalises every
 * column (as after gndt_remove).  A PARTITION-built map is cropped as rows only.  A sharded map crops the rows this rank holds.
 * Order and lifetime:
 *   - the call first finishes what gndt_sync finishes (a pending build, a deferred emit, a re-run);
 *   - the map is new: the cost map is invalid until the next gndt_compute_cost (gndt_cost_export* refuse it, as after an update), the
 *     map's column index is rebuilt, and device pointers from gndt_export_device and row numbers from gndt_query* are invalid;
 *   - a stream under hipGraph capture is refused (GNDT_ERR_INVALID: a crop is not recorded);
 *   - a graph recorded before a crop and replayed after it is reported stale by gndt_sync (GNDT_ERR_CAPACITY, as after a buffer
 *     reallocation): the crop moves the result arrays.  Capture again after the crop.
 * gndt_crop_device enqueues its kernels on `hip_stream` (NULL = the handle's stream, the rules of gndt_build_device) and returns; the
 * counts are read by the next gndt_sync.  It waits for the device only to finish pending work (the gndt_sync above).  gndt_crop is
 * the same followed by gndt_sync. */
enum { GNDT_CROP_KEEP_INSIDE = 0, GNDT_CROP_DROP_INSIDE = 1 };
typedef struct { int32_t sx_min, sx_max, sy_min, sy_max; } gndt_crop_box;
int gndt_crop_device(gndt_handle* h, const gndt_crop_box* box, int32_t mode, void* hip_stream);
int gndt_crop(gndt_handle* h, const gndt_crop_box* box, int32_t mode);
/* Host helper, no handle, no GPU: the box of the columns that hold at least one point of the world rectangle [lo, hi] (inclusive), as the
 * codec keys them — the IEEE fp32 axis index (gndt_trans_morton_xyz's arithmetic) of lo and of hi on each axis; exact at lattice
 * multiples (a point on a cell border belongs to the cell the codec gives it).  Ends beyond the codec's range (|index| > 65535) clamp
 * to it.  GNDT_ERR_INVALID: a null pointer, grid_len not > 0, a non-finite value, lo > hi on an axis. */
int gndt_crop_box_from_world(const float origin[3], float grid_len, const float lo_xy[2], const float hi_xy[2], gndt_crop_box* out);

/* ---- raster export: one pixel per column of a box, the slope a consumer stands on -------------------------------------------
 * The map over a window as a 2-D image (an occupancy grid, a costmap layer, an elevation map, a bird's-eye-view tensor), the
 * reference's showBottom / showSlopeList (map2D.h:980-1284: one cell per column, coloured by its slope's height), without exporting
 * every row.  The region is a gndt_crop_box (a world rectangle reaches it through gndt_crop_box_from_world).
 * Geometry: signed indices skip 0, so the image is `width` x `height`, the non-zero integers of [sx_min, sx_max] x [sy_min, sy_max].
 * Pixel (i, j) sits at j * width + i; i runs over those sx ascending, j over those sy ascending (row-major, row 0 at the smallest y:
 * the nav_msgs/OccupancyGrid convention).  Pixels are grid_len apart everywhere, across the origin too: the centre of column s is
 * origin + sign(s) * (|s| - 0.5) * grid_len.
 * Selection, among the rows of the pixel's column that have GNDT_FLAG_SLOPE:
 *   GNDT_RASTER_LOWEST     the least sz (the reference's bottom: the ground under a bridge)
 *   GNDT_RASTER_HIGHEST    the greatest sz (the deck)
 *   GNDT_RASTER_NEAREST_Z  the least fabsf(mean_z - z_ref) in fp32, a tie going to the smaller sz: GNDT_QUERY_NEAREST_SLOPE's rule
 *                          (the same code), for every pixel at once
 * A column without a slope gives an empty pixel (row GNDT_NO_ROW, z and rough quiet NaN, h FLT_MAX, state 0); its `nodes` layer still
 * counts the column's nodes, so "observed, nothing to stand on" (nodes > 0) stays apart from "never observed" (nodes == 0).  A box
 * that covers no column of the map is not an error: every pixel is empty.
 * GNDT_ERR_INVALID: a null handle or box, every layer pointer NULL, an unknown mode, a non-finite z_ref with NEAREST_Z, min > max on an
 * axis, an index beyond +-65535, an axis without a non-zero index ([0, 0]), width * height > 2^31, no finished build, h or state
 * without a cost map of the current grid (the rule of gndt_cost_export), a stream under hipGraph capture (a raster is not recorded).
 * Order and lifetime are the point queries': the call first finishes what gndt_sync finishes (a pending build, a deferred emit, a
 * re-run), then builds or reuses the map's column index (the one the queries and the flood use, under the same rule).  Row numbers stay valid until the
 * next build, update, remove, crop or reset.  A sharded map rasterises the rows this rank holds. */
enum { GNDT_RASTER_LOWEST = 0, GNDT_RASTER_HIGHEST = 1, GNDT_RASTER_NEAREST_Z = 2 };
typedef struct {
    uint32_t* row;    /* selected slope's row (gndt_cells order), GNDT_NO_ROW where none      */
    float*    z;      /* its mean z;                          quiet NaN where none           */
    float*    rough;  /* its Slope::rough;                    quiet NaN where none           */
    uint32_t* nodes;  /* the column's node count (any node);  0 = column not in the map      */
    float*    h;      /* cost map h of the row;               FLT_MAX where none             */
    uint32_t* state;  /* cost map state of the row;           0 where none                   */
} gndt_raster_layers;  /* every pointer optional (NULL = not written); at least one non-NULL; each width * height elements */
/* Host, no handle, no GPU: the image size of a box.  GNDT_ERR_INVALID for the box errors above (and null pointers). */
int gndt_raster_shape(const gndt_crop_box* box, uint32_t* width, uint32_t* height);
/* Device layers; enqueued on `hip_stream` (NULL = the handle's stream, the rules of gndt_build_device) and not awaited. */
int gndt_raster_device(gndt_handle* h, const gndt_crop_box* box, int32_t mode, float z_ref, const gndt_raster_layers* out_dev,
                       void* hip_stream);
/* Host layers, through a device scratch the handle owns and grows; synchronous. */
int gndt_raster(gndt_handle* h, const gndt_crop_box* box, int32_t mode, float z_ref, const gndt_raster_layers* out_host);

/* ---- frontier extraction: the slopes where the known map ends, clustered on the device --------------------------------------
 * What an explorer, a coverage planner or a "map is complete" check asks between a flood and a planning call: where does the map end,
 * and which of those places can the robot drive to?  The answer is a list of clusters whose best rows are ready to be planned to
 * (gndt_plan_routes*, start_mode GNDT_QUERY_NEAREST_SLOPE at the rows' column centres).  The map cannot tell "unknown" from "seen
 * empty": a frontier here is where the map ends.  Every definition is integer or bit-pattern arithmetic: the answer is exact and does
 * not depend on the order threads work in.  lin(s) = s > 0 ? s - 1 : s is the position of a signed index on a line without the hole
 * at 0 (signed indices skip 0 on all three axes).
 *   candidate     a row with GNDT_FLAG_SLOPE, inside `box` (NULL = the whole map), and
 *                   GNDT_FRONTIER_REACHED  with cost-map state 1 (the flood expanded it); needs a cost map of the current grid (the
 *                                          rule of gndt_cost_export);
 *                   GNDT_FRONTIER_SLOPES   nothing more; no cost map is read and best_h is FLT_MAX.
 *   open side     one of the row's four neighbour columns (sx -+ 1, sy), (sx, sy -+ 1), stepping over 0, that
 *                   GNDT_FRONTIER_OPEN_COLUMN  is not in the map (an index beyond the codec's +-65535 is not);
 *                   GNDT_FRONTIER_OPEN_LEVEL   is not in the map or holds no node (ANY node: map_xy's view) with
 *                                              |lin(sz_n) - lin(sz)| <= level_reach: on a two-storey map the deck's edge over the
 *                                              ground is then a frontier of the deck.
 *   frontier row  a candidate with at least min_open (1..4; 0 = 1) open sides.
 *   link          two frontier rows whose columns are 8-adjacent (|lin(sx_a) - lin(sx_b)| <= 1 and |lin(sy_a) - lin(sy_b)| <= 1, not
 *                 the same column) with |lin(sz_a) - lin(sz_b)| <= link_dz.  Two slopes of one column are never linked directly.
 *   cluster       a connected component of the links; its label is its smallest member row.
 * Outputs: clusters[] holds the clusters with at least min_size members in ascending label, the first cluster_cap of them (nothing is
 * written beyond those); counts[0] is how many there are — it may exceed cluster_cap, so the caller sees the truncation and can call
 * again (cluster_cap 0 with clusters NULL only counts) — counts[1] the frontier rows, counts[2] the clusters of any size, counts[3] 0.
 * label[row] (optional, num_nodes entries) is the row's cluster label, GNDT_NO_ROW for a row that is no frontier row; min_size does not
 * filter it.  A cluster's record: its label and size, the member with the least cost-map h (a tie going to the smaller row; under
 * SLOPES that is the label) and that h, the bounds of its columns' signed indices, the sums of lin(sx), lin(sy), lin(sz) over its
 * members (centroid = sum / size; a column's centre is origin + (lin(s) + 0.5) * grid_len) and the sum of its members' open sides.
 * Order and lifetime are the point queries': the call first finishes what gndt_sync finishes, builds or reuses the map's column
 * index and enqueues its kernels on `hip_stream` (NULL = the handle's stream), not awaited; gndt_frontiers is synchronous.  Row
 * numbers stay valid until the next build, update, remove, crop or reset.  The map, h and state are not modified.  Work memory (9 bytes
 * a row) belongs to the handle and grows with the map.  A map without rows gives four zero counts.  There is no CPU path.
 * A sharded map answers from the rows this rank holds: the borders between ranks therefore look open.
 * GNDT_ERR_INVALID: a null handle, params or counts, unknown candidates / open_rule, min_open > 4, a non-zero reserved word, a bad box
 * (the raster's rules but its pixel limit: min > max on an axis, an index beyond +-65535, an axis without a non-zero index), clusters
 * NULL with cluster_cap > 0 or the reverse, a device pointer not aligned as its type is, no finished build, REACHED without a current
 * cost map, a stream under hipGraph capture (the call is not recorded). */
enum { GNDT_FRONTIER_REACHED = 0, GNDT_FRONTIER_SLOPES = 1 };
enum { GNDT_FRONTIER_OPEN_COLUMN = 0, GNDT_FRONTIER_OPEN_LEVEL = 1 };
typedef struct gndt_frontier_params {
    int32_t  candidates;     /* GNDT_FRONTIER_REACHED / _SLOPES */
    int32_t  open_rule;      /* GNDT_FRONTIER_OPEN_COLUMN / _OPEN_LEVEL */
    uint32_t level_reach;    /* OPEN_LEVEL only */
    uint32_t min_open;       /* 0 = 1 */
    uint32_t link_dz;        /* levels, as given (0 = same level only) */
    uint32_t min_size;       /* clusters with fewer members are left out of the list; 0 = 1 */
    uint32_t reserved[2];    /* 0 */
} gndt_frontier_params;
typedef struct gndt_frontier {      /* 64 bytes */
    uint32_t label, size;            /* smallest member row; members */
    uint32_t best_row; float best_h; /* the member with the least cost-map h, a tie going to the smaller row */
    int32_t  sx_min, sx_max, sy_min, sy_max;
    int64_t  sum_px, sum_py, sum_pz; /* sums of lin(sx), lin(sy), lin(sz) over the members */
    uint32_t open_sides;             /* sum of the members' open sides */
    uint32_t reserved;
} gndt_frontier;
/* Device memory out: label_dev [num_nodes] or NULL, clusters_dev [cluster_cap], counts_dev [4]. */
int gndt_frontiers_device(gndt_handle* h, const gndt_crop_box* box, const gndt_frontier_params* params,
                          uint32_t* label_dev /* [num_nodes] or NULL */, gndt_frontier* clusters_dev, uint32_t cluster_cap,
                          uint32_t* counts_dev /* [4] */, void* hip_stream);
/* Host memory out, through a device scratch the handle owns and grows; returns when the answers are in place. */
int gndt_frontiers(gndt_handle* h, const gndt_crop_box* box, const gndt_frontier_params* params,
                   uint32_t* label_host, gndt_frontier* clusters_host, uint32_t cluster_cap, uint32_t* counts_host);

/* ---- surface patches: map nodes grouped into planes, on the device ------------------------------------------------------------
 * What the map is made of: this floor, that wall, this ramp, the deck above the ground.  Every node carries the normal and the
 * thickness of a local plane; region growing over them turns 800 k rows into a few hundred records — to publish, log and compare; to
 * say which rows are wall, floor or inclined; to hand plane pairs to a check of a registration; to name the drivable surface as one
 * object with an extent and a tilt.  lin(s) = s > 0 ? s - 1 : s, as in the frontiers.
 * Rounding: every fp32 operation below is ONE rounded operation in the order written, no fused multiply-add (numpy float32 gives the
 * same bits).
 *   candidate   a row inside `box` (NULL = the whole map; the frontiers' box rules) that has GNDT_FLAG_HAS_STATS, under
 *               GNDT_PATCH_SLOPES also GNDT_FLAG_SLOPE (GNDT_PATCH_NODES: nothing more), and rough <= max_var * (float)count (one fp32
 *               multiply).  rough is the STORED value — the least eigenvalue of the node's scatter, the reference's 0 -> 0.01
 *               included: a perfectly flat node is a candidate whenever max_var * count >= 0.01.  A node that has statistics but no
 *               slope (demand "slope": a node with another one of its column close above it) stores no normal and rough 0: under
 *               GNDT_PATCH_NODES it is a candidate that links to nothing (c = 0) and ends as a patch of one.  Maps built with demand
 *               "true" give every node with statistics its normal: build so where walls — stacks of nodes — are to become patches.
 *   adjacent    rows a != b with |lin(sx_a) - lin(sx_b)|, |lin(sy_a) - lin(sy_b)| and |lin(sz_a) - lin(sz_b)| all <= 1 and at most
 *               `connectivity` axes differing: 1, 2 or 3 for the 6-, 18- or 26-neighbourhood; 0 = 3.  Unlike the frontiers, two nodes
 *               of one column that are one level apart ARE adjacent: a wall is a stack.
 *   link        two adjacent candidates with normals n, means m (fp32, as stored) for which both tests pass:
 *                 c = (nax*nbx + nay*nby) + naz*nbz                     fabsf(c) >= cos_min          (normals are sign free)
 *                 d = m_b - m_a componentwise;  ea = fabsf((nax*dx + nay*dy) + naz*dz),  eb = fabsf((nbx*dx + nby*dy) + nbz*dz)
 *                                                                       ea <= max_offset and eb <= max_offset
 *               fp32 subtraction is exactly antisymmetric, so the rule is symmetric to the bit.
 *   patch       a connected component of the links; its label is its smallest member row.  A candidate without a link is a patch of
 *               one.  This is single-link growing: a gently curved surface chains into ONE patch — the record's var shows it.
 * Outputs (the frontiers' conventions): patches[] holds the patches with at least min_size members in ascending label, the first
 * patch_cap of them (nothing is written beyond those); counts[0] is how many such patches exist — it may exceed patch_cap (patch_cap 0
 * with patches NULL only counts) — counts[1] the candidates, counts[2] the patches of any size, counts[3] 0.  label[row] (optional,
 * num_nodes entries) is the row's patch label, GNDT_NO_ROW for a row that is no candidate; min_size does not filter it.
 * A patch's record: label, nodes (members), points (the sum of their counts), the bounds of their signed indices on the three axes, the
 * sums of lin(sx), lin(sy), lin(sz), and the plane of the members merged as Gaussians: with r the label row's mean as fp64,
 * d_i = mean_i - r, N = Sum count_i, S1 = Sum count_i d_i and S2 = Sum (scatter_i + count_i d_i d_i^T) — scatter_i the node's stored cov,
 * moved by the moment match of the map pyramids (gndt_coarsen_device) —
 *   C = S2 - S1 S1^T / N     centroid = r + S1 / N     normal = the unit eigenvector of C's least eigenvalue (the build's fp64 solver),
 *   its first non-zero component in the order z, y, x positive     var = max(lambda_min, 0) / N (m^2: the patch's thickness)
 *   kind: GNDT_PATCH_HORIZONTAL |normal_z| >= cos_level, GNDT_PATCH_VERTICAL |normal_z| <= sin_level (tested in that order),
 *         GNDT_PATCH_INCLINED neither; GNDT_PATCH_SLOPES_ONLY every member has GNDT_FLAG_SLOPE (an integer tally).
 * What is exact: labels, counts and every integer field (kind's SLOPES_ONLY bit included), whatever order threads work in.  The fp64 sums
 * are accumulated with atomics, so centroid, normal, var and the three orientation bits of kind are reproducible only to fp64 rounding
 * from run to run — the standard the build's own node statistics have; no bits are promised for them.
 * Order and lifetime are the frontiers': the call first finishes what gndt_sync finishes, builds or reuses the map's column index and
 * enqueues its kernels on `hip_stream` (NULL = the handle's stream), not awaited; gndt_patches is synchronous.  Row numbers stay valid
 * until the next build, update, remove, crop or reset.  The map is not modified; no cost map is read.  Work memory (8 bytes a row and 80
 * a listed patch) belongs to the handle and grows with the map.  A map without rows gives four zero counts.  There is no CPU path.
 * A sharded map answers from the rows this rank holds: a plane that crosses ranks is one patch per rank.
 * GNDT_ERR_INVALID: a null handle, params or counts, unknown candidates, connectivity > 3, a threshold (cos_min, max_offset, max_var,
 * cos_level, sin_level) that is negative or not finite, cos_min or cos_level above 1, a non-zero reserved word, a bad box (the frontiers'
 * rules), patches NULL with patch_cap > 0 or the reverse, a device pointer not aligned as its type is, no finished build, a stream under
 * hipGraph capture (the call is not recorded). */
enum { GNDT_PATCH_NODES = 0, GNDT_PATCH_SLOPES = 1 };
enum { GNDT_PATCH_HORIZONTAL = 1, GNDT_PATCH_VERTICAL = 2, GNDT_PATCH_INCLINED = 4, GNDT_PATCH_SLOPES_ONLY = 8 };
typedef struct gndt_patch_params {
    int32_t  candidates;     /* GNDT_PATCH_NODES / _SLOPES */
    uint32_t connectivity;   /* axes that may differ between adjacent rows: 1, 2 or 3; 0 = 3 */
    float    cos_min;        /* least |cosine| between linked normals, 0 .. 1 */
    float    max_offset;     /* m: most a linked node's mean may lie off the other's plane */
    float    max_var;        /* m^2: a candidate's rough / count at most */
    float    cos_level;      /* |normal_z| from which a patch is HORIZONTAL, 0 .. 1 */
    float    sin_level;      /* |normal_z| up to which a patch is VERTICAL */
    uint32_t min_size;       /* patches with fewer members are left out of the list; 0 = 1 */
    uint32_t reserved[4];    /* 0 */
} gndt_patch_params;
typedef struct gndt_patch {            /* 128 bytes */
    uint32_t label, nodes;  uint64_t points;                 /* smallest member row; members; sum of their counts */
    int32_t  sx_min, sx_max, sy_min, sy_max, sz_min, sz_max;
    int64_t  sum_px, sum_py, sum_pz;                          /* sums of lin(s) over the members */
    double   centroid[3], normal[3], var;                     /* the members merged as Gaussians */
    uint32_t kind, reserved;
} gndt_patch;
/* Device memory out: label_dev [num_nodes] or NULL, patches_dev [patch_cap], counts_dev [4]. */
int gndt_patches_device(gndt_handle* h, const gndt_crop_box* box, const gndt_patch_params* params,
                        uint32_t* label_dev /* [num_nodes] or NULL */, gndt_patch* patches_dev, uint32_t patch_cap,
                        uint32_t* counts_dev /* [4] */, void* hip_stream);
/* Host memory out, through a device scratch the handle owns and grows; returns when the answers are in place. */
int gndt_patches(gndt_handle* h, const gndt_crop_box* box, const gndt_patch_params* params,
                 uint32_t* label_host, gndt_patch* patches_host, uint32_t patch_cap, uint32_t* counts_host);

/* ---- clearance field: hops to the nearest barrier for every slope ------------------------------------------------------------
 * What a planner asks after "can the robot stand here" (the flood's CollisionCheck) and "what does it cost to reach the goal from
 * here" (h): how far is this slope from the nearest place the robot cannot go?  The answer is an inflation layer for a costmap, a
 * direction to push trajectories away from, a way to rank a narrow passage against a wide one, and one field for robots of several
 * widths.  Every definition is integer arithmetic except the flood's three gates, which are the flood's own code: the answer is exact
 * and does not depend on the order threads work in.
 *   side          (q, k): slope q (a row with GNDT_FLAG_SLOPE) towards its k-th neighbour column in the flood's order — (sx, sy - 1),
 *                 (sx, sy + 1), (sx + 1, sy), (sx - 1, sy), stepping over index 0.  A side is
 *                   open      the column is not in the map (an index beyond the codec's +-65535 is not);
 *                   passable  at least one row t of the column has GNDT_FLAG_SLOPE and passes the flood's gates seen from q (the
 *                             roughness of t, the angle between the normals, |mean_z(t) - mean_z(q)| <= reachable_height): those
 *                             rows are the steps of q through the side;
 *                   blocked   the column is in the map and no row passes: a wall, a kerb, a step up or down, rubble.
 *   source        a slope for which a condition selected in params->sources (a bit mask, 0 = GNDT_CLEARANCE_BLOCKED) holds:
 *                   GNDT_CLEARANCE_BLOCKED   at least one blocked side;
 *                   GNDT_CLEARANCE_OPEN      at least one open side: the map's edge counts as a barrier;
 *                   GNDT_CLEARANCE_OVERHEAD  the next slope above in its own cell lies within 2 radius and more than reachable_height
 *                                            above it (CollisionCheck's last test; the only use of robot->radius).
 *   hops(q)       the length of the shortest walk q -> p1 -> ... -> s along steps that ends in a source s; 0 for a source.  The graph
 *                 is directed (the roughness gate looks only at the destination).  GNDT_CLEARANCE_BEYOND for a slope without such a
 *                 walk of at most max_hops steps (0 = 32; above 1024 is refused: it bounds the launches of a call, and the device is
 *                 shared) and for every row without a slope.
 *   nearest(q)    the smallest row among the sources exactly hops(q) steps from q; GNDT_NO_ROW where hops is BEYOND.  The pair is the
 *                 fixed point of key(q) = min(key(q), min over steps p of key(p) + 2^32) with key = hops << 32 | source row, which
 *                 rounds over all rows at once reach exactly.
 *   sides(q)      one byte: bits 0-3 the blocked sides, bits 4-7 the open sides, in the order above; 0xFF for a row without a slope.
 *   counts[4]     the sources, the slopes with finite hops, the largest finite hops, 0.
 * hops, nearest and sides have num_nodes entries; each may be NULL (it is then not written), but not all three.  `robot` NULL = the
 * flood's defaults.  Order and lifetime are the frontier call's: the call first finishes what gndt_sync finishes, builds or reuses the
 * map's column index and enqueues its kernels on `hip_stream` (NULL = the handle's stream), not awaited — one launch per hop, of
 * which those behind the last hop that changed anything return at once; a map of up to 9216 rows takes every hop in one launch of one
 * workgroup.  gndt_clearance is synchronous.  The map, h and state are not modified and no cost map is needed.  Work memory (49 bytes a
 * row) belongs to the handle and grows with the map.  A map without rows gives four zero counts.  There is no CPU path.  A sharded
 * map answers from the rows this rank holds: the borders between ranks therefore look open.
 * GNDT_ERR_INVALID: a null handle, params or counts, hops, nearest and sides all NULL, unknown source bits, max_hops > 1024, a
 * non-zero reserved word, hops_dev, nearest_dev or counts_dev not aligned to 4 bytes, no finished build, a stream under hipGraph
 * capture (the call is not recorded). */
#define GNDT_CLEARANCE_BEYOND 0xFFFFFFFFu
enum { GNDT_CLEARANCE_BLOCKED = 1, GNDT_CLEARANCE_OPEN = 2, GNDT_CLEARANCE_OVERHEAD = 4 };
typedef struct gndt_clearance_params { uint32_t sources, max_hops, reserved[6]; } gndt_clearance_params;  /* zeros = defaults */
/* Device memory out: hops_dev, nearest_dev [num_nodes] (uint32), sides_dev [num_nodes] (bytes), each or NULL; counts_dev [4]. */
int gndt_clearance_device(gndt_handle* h, const gndt_robot* robot, const gndt_clearance_params* params,
                          uint32_t* hops_dev, uint32_t* nearest_dev, uint8_t* sides_dev, uint32_t* counts_dev /* [4] */, void* hip_stream);
/* Host memory out, through a device scratch the handle owns and grows; returns when the answers are in place. */
int gndt_clearance(gndt_handle* h, const gndt_robot* robot, const gndt_clearance_params* params,
                   uint32_t* hops_host, uint32_t* nearest_host, uint8_t* sides_host, uint32_t* counts_host);

/* ---- path walks: candidate trajectories driven over the map's slopes ----------------------------------------------------------
 * What a local planner asks between a global route and the wheels — a DWA arc fan, MPPI rollouts, "does the route of a second ago
 * still hold after the last update": can the robot step from slope to slope along this polyline under the flood's gates, where does
 * it stop if not and why, how long, steep and rough is the drive, how close does it come to a barrier.  One call takes K paths of T
 * waypoints each: floats x, y, z at stride 12 or 16, path-major (waypoint [k * T + j] is the j-th of path k).  `robot` NULL = the
 * flood's defaults.  Per path, in this order:
 *   1. start     waypoint 0 through the point queries' own lookup selects the start row: params->start_mode 0 or
 *                GNDT_WALK_START_NEAREST_SLOPE (= GNDT_QUERY_NEAREST_SLOPE's value and rule), or GNDT_WALK_START_NODE
 *                (GNDT_QUERY_NODE's lookup — that enum's value is 0, which here has to mean "the default" — and the row must have
 *                GNDT_FLAG_SLOPE).  No row: status GNDT_WALK_NO_START (waypoints 0, both rows GNDT_NO_ROW).  q = that row; the checks
 *                of 4 apply to it.
 *   2. segments  for j = 1 .. T-1: a waypoint whose x or y is not finite ends the path normally (a terminator: one call holds paths
 *                of different lengths).  A finite waypoint that point_key cannot key — with waypoint 0's z, which every point of the
 *                path is given — ends it with GNDT_WALK_LEFT_MAP.  Otherwise the segment from waypoint j-1 to waypoint j is crossed
 *                column by column in the column sequence of the ray walk ("free-space clearing": max_range = end_margin = 0, its
 *                levels ignored): |dx| + |dy| unit steps, each across the lattice plane the segment meets first, fp64, a tie
 *                stepping x.  Consecutive segments join in one column, since both key the same float point.  Every column change is
 *                a step through one side k of q in the flood's order (the clearance field's sides; no index 0).
 *   3. a step    through side k: among the rows t of that neighbour column that have GNDT_FLAG_SLOPE and pass the flood's gates seen
 *                from q (the clearance field's "steps of q through the side") the one with the least fabsf(mean_z(t) - mean_z(q))
 *                in fp32, a tie going to the smaller row.  The column is not in the map (an index beyond +-65535 is not):
 *                GNDT_WALK_LEFT_MAP; it is and offers no step: GNDT_WALK_BLOCKED; both with stop_side = k and end_row the last
 *                slope stood on.
 *   4. checks    on every slope stood on, the start included, each optional: with GNDT_WALK_CHECK_OVERHEAD in params->checks the
 *                next slope above in its own cell within 2 radius and more than reachable_height above (CollisionCheck's last
 *                test, the clearance field's OVERHEAD) gives GNDT_WALK_OVERHEAD; with hops_dev != NULL, hops_dev[t] <
 *                params->min_hops gives GNDT_WALK_TOO_CLOSE (overhead is tested first).  hops_dev is a gndt_clearance* `hops` output
 *                OF THIS MAP AS IT IS NOW, num_nodes entries: the caller vouches for that — after an update, a crop or a clear the
 *                field has to be computed again, and a stale or shorter array is read out of bounds.  hops_min is the least value
 *                seen whether or not min_hops is set, GNDT_CLEARANCE_BEYOND without hops_dev.  The slope that fails a check has
 *                been entered: it is end_row, counts in steps and in the sums and maxima.
 *   5. guard     a path that has taken params->max_steps steps (0 = 65536; above 2^20 is refused: it bounds a lane's loop, and the
 *                device is shared) and needs another ends with GNDT_WALK_LIMIT; one that needs exactly max_steps is DONE.
 *   6. sums      in walk order, so that one thread's sequential arithmetic reproduces them: length = the sum of TravelCost(mean(q),
 *                mean(t)) (the flood's: fp32 differences, squares and root in fp64, rounded to fp32) over the steps, added in fp64
 *                and rounded to fp32 once; climb = the sum of fabsf(mean_z(t) - mean_z(q)) the same way; rough_max the largest
 *                `rough` over the slopes stood on (0 without a start).
 * waypoints counts the waypoints whose column was reached, the start included.  rows_dev (optional, NULL together with row_cap 0)
 * receives per path row_cap entries: the slopes stood on, start first, GNDT_NO_ROW behind them; a longer walk writes its first row_cap
 * rows and the caller sees steps + 1 > row_cap.  info is written 16 bytes at a time: info_dev must be aligned to 16 bytes.
 * Order and lifetime are the clearance call's: the call first finishes what gndt_sync finishes, builds or reuses the map's column
 * index and enqueues its kernel on `hip_stream` (NULL = the handle's stream), not awaited; gndt_walk_paths is synchronous and takes
 * host memory of any alignment.  The map, h and state are not modified and no cost map is needed.  K == 0 or T == 0 returns GNDT_OK
 * and launches nothing.  There is no CPU path.  A sharded map answers from the rows this rank holds.  Work memory (41 bytes a row)
 * belongs to the handle and is used only when a call reads its steps from a table made once per call: on a map of up to 2048 rows
 * per waypoint of a path (GNDT_DEBUG_WALK_STEP_TABLE); the answer does not depend on it.
 * GNDT_ERR_INVALID: a null handle, params or info, null paths with K and T non-zero, K * T >= 2^31, a stride other than 12 or 16, an
 * unknown start_mode or check bit, max_steps > 2^20, a non-zero reserved word, rows NULL with row_cap != 0 or the reverse, info_dev
 * not aligned to 16 bytes or paths_dev, hops_dev, rows_dev not to 4, no finished build, a stream under hipGraph capture. */
enum { GNDT_WALK_DONE = 0, GNDT_WALK_NO_START = 1, GNDT_WALK_BLOCKED = 2, GNDT_WALK_LEFT_MAP = 3, GNDT_WALK_OVERHEAD = 4,
       GNDT_WALK_TOO_CLOSE = 5, GNDT_WALK_LIMIT = 6 };
enum { GNDT_WALK_START_NEAREST_SLOPE = 1, GNDT_WALK_START_NODE = 2 };
#define GNDT_WALK_CHECK_OVERHEAD 1u
#define GNDT_WALK_NO_SIDE 0xFFFFFFFFu
typedef struct gndt_walk_params {
    int32_t start_mode;       /* 0 = GNDT_WALK_START_NEAREST_SLOPE */
    uint32_t checks;          /* GNDT_WALK_CHECK_* bits */
    uint32_t min_hops;        /* with hops: a slope with fewer hops ends the path (0: none does) */
    uint32_t max_steps;       /* 0 = 65536 */
    uint32_t reserved[4];     /* 0 */
} gndt_walk_params;           /* 32 bytes; zeros = defaults */
typedef struct gndt_walk_info {
    int32_t status;           /* GNDT_WALK_* */
    uint32_t stop_side;       /* 0..3 for BLOCKED and a LEFT_MAP of a step, else GNDT_WALK_NO_SIDE */
    uint32_t steps;           /* column changes taken */
    uint32_t waypoints;       /* waypoints whose column was reached, the start included */
    uint32_t start_row, end_row;
    float length, climb;
    float rough_max;
    uint32_t hops_min;
    uint32_t reserved[2];
} gndt_walk_info;             /* 48 bytes */
/* Device memory in and out. */
int gndt_walk_paths_device(gndt_handle* h, const void* paths_dev, size_t K, size_t T, size_t stride_bytes, const gndt_robot* robot,
                           const gndt_walk_params* params, const uint32_t* hops_dev /* [num_nodes] or NULL */,
                           uint32_t* rows_dev /* [K * row_cap] or NULL */, uint32_t row_cap, gndt_walk_info* info_dev /* [K] */,
                           void* hip_stream);
/* Host memory in and out, through a device scratch the handle owns and grows; returns when the answers are in place. */
int gndt_walk_paths(gndt_handle* h, const void* paths_host, size_t K, size_t T, size_t stride_bytes, const gndt_robot* robot,
                    const gndt_walk_params* params, const uint32_t* hops_host, uint32_t* rows_host, uint32_t row_cap,
                    gndt_walk_info* info_host);

/* ---- route shortcutting: any-angle waypoints from slope-to-slope routes ---------------------------------------------------------
 * What gndt_plan_routes* returns is a staircase of 4-neighbour slopes, one waypoint a cell.  A controller wants it string-pulled: only
 * the waypoints between which the robot can drive straight, and no corner cut closer to a barrier than the caller allows.  One call
 * takes K routes in the layout gndt_plan_routes* writes: route_rows[k * route_cap + i], start first; its length n_k is the uint32 at
 * lengths + k * length_stride_bytes (stride sizeof(gndt_route_info) with &info[0].length of a plan call, stride 4 for a plain array).
 * A route need not come from the planner: any sequence of slope rows is one.  `robot` NULL = the flood's defaults.
 * Link(a, b) for two rows:
 *   1. both rows are < num_nodes and have GNDT_FLAG_SLOPE;
 *   2. P_a, P_b: the centres of their columns, per axis (float)((double)o + sign(s) * (|s| - 0.5) * (double)grid_len) (no index 0);
 *   3. both points take z = mean_z(a); the levels are ignored, as in the walks;
 *   4. point_key of either point does not give back that row's column: the link fails;
 *   5. the columns are more than `window` unit steps apart (|dlx| + |dly| in lattice cells): the link fails untested;
 *   6. otherwise the link is the path walk ("path walks" 2 - 4) of the two-waypoint polyline P_a -> P_b: the ray walk's column
 *      sequence, the step through a side, the checks on every slope stood on, a included (GNDT_WALK_CHECK_OVERHEAD in
 *      params->checks; hops_dev with params->min_hops, under the walk call's conditions on hops_dev) —
 *   7. except that the walk STARTS STANDING ON ROW a, not on what the start lookup finds;
 *   8. the link HOLDS iff the walk ends GNDT_WALK_DONE ON ROW b (b's column reached on another storey is not enough).
 * Per route with rows r[0 .. n):
 *   1. out = [r[0]], anchor a = 0.
 *   2. while a < n - 1: the candidates are j in (a, min(a + window, n - 1)], in groups of 64 counted from the anchor: a+1 .. a+64,
 *      a+65 .. a+128, ...
 *   3. the groups are evaluated from the farthest down; the first group in which a link r[a] -> r[j] holds ends the search;
 *   4. the next anchor is the largest j of that group whose link holds;
 *   5. no link holds in any group: the next anchor is a + 1, a FALLBACK LINK — the route's own step, kept untested, so the output
 *      is never worse than the input;
 *   6. links_tested counts the candidates of the groups evaluated (the group order is part of the definition);
 *   7. before a group is evaluated, links_tested plus its size is checked against max_links: if it would exceed it the route ends
 *      with GNDT_SHORTCUT_LIMIT and the rows from a + 1 on are appended as fallback links (the output is still a route).
 * waypoint_rows[k * waypoint_cap ..]: the anchors, start first and goal last, GNDT_NO_ROW behind them; a longer answer writes its
 * first waypoint_cap rows and `waypoints` says so.  path_rows (optional: NULL exactly when path_cap is 0) [k * path_cap ..]: every
 * slope stood on along the accepted links, in order, each junction once; a fallback link contributes r[a + 1]; cut and filled the
 * same way.  Where every link is a 4-neighbour step this is again a slope-to-slope route.
 * gndt_shortcut_info, written 16 bytes at a time: status — GNDT_SHORTCUT_OK; _EMPTY for n = 0; _BAD_ROUTE for n > route_cap or a row
 * that is out of range (GNDT_NO_ROW is), or holds no slope: nothing is tested and nothing but the GNDT_NO_ROW tails is written, the
 * counts and sums are 0 but length_in; _LIMIT — length_in = n; waypoints; path_slopes; links_tested; fallback_links; cost_in, the sum
 * of TravelCost over consecutive input rows, and cost_out, the same sum over consecutive path rows whether or not they are written,
 * both added in order in fp64 and rounded to fp32 once; hops_min over the path's slopes, GNDT_CLEARANCE_BEYOND without hops_dev.
 * Order, lifetime and refusals follow the walk call's: after what gndt_sync finishes, on the map's column index, enqueued on
 * `hip_stream` (NULL = the handle's stream) and not awaited; gndt_shortcut_routes is synchronous and takes host memory of any
 * alignment.  No cost map is needed; the map, h and state are not modified.  K == 0 returns GNDT_OK and launches nothing.  There is no
 * CPU path.  GNDT_ERR_INVALID: a null handle, params or info, null routes or lengths with K > 0, K >= 2^31, route_cap 0 with K > 0, a
 * stride below 4 or not a multiple of 4, window > 256 (with n anchors, window / 64 groups and up to `window` steps a lane the worst
 * case grows with window^2 n, and the device is shared), unknown check bits, max_links > 2^24, a non-zero reserved word,
 * waypoint_rows NULL, path_rows NULL with path_cap != 0 or the reverse, info_dev not aligned to 16 bytes or another device pointer not
 * to 4, no finished build, a stream under hipGraph capture. */
enum { GNDT_SHORTCUT_OK = 0, GNDT_SHORTCUT_EMPTY = 1, GNDT_SHORTCUT_BAD_ROUTE = 2, GNDT_SHORTCUT_LIMIT = 3 };
typedef struct gndt_shortcut_params {
    uint32_t window;          /* candidates looked at behind an anchor, and the most unit steps of a link; 0 = 64, at most 256 */
    uint32_t checks;          /* GNDT_WALK_CHECK_* bits */
    uint32_t min_hops;        /* with hops: a slope with fewer hops fails the link (0: none does) */
    uint32_t max_links;       /* 0 = 2^20, at most 2^24 */
    uint32_t reserved[4];     /* 0 */
} gndt_shortcut_params;       /* 32 bytes; zeros = defaults */
typedef struct gndt_shortcut_info {
    int32_t status;           /* GNDT_SHORTCUT_* */
    uint32_t length_in, waypoints, path_slopes;
    uint32_t links_tested, fallback_links;
    float cost_in, cost_out;
    uint32_t hops_min;
    uint32_t reserved[3];     /* 0 */
} gndt_shortcut_info;         /* 48 bytes */
/* Device memory in and out. */
int gndt_shortcut_routes_device(gndt_handle* h, const uint32_t* route_rows_dev, size_t K, uint32_t route_cap,
                                const void* lengths_dev, size_t length_stride_bytes,
                                const gndt_robot* robot, const gndt_shortcut_params* params, const uint32_t* hops_dev /* [num_nodes] or NULL */,
                                uint32_t* waypoint_rows_dev /* [K * waypoint_cap] */, uint32_t waypoint_cap,
                                uint32_t* path_rows_dev /* [K * path_cap] or NULL */, uint32_t path_cap,
                                gndt_shortcut_info* info_dev /* [K] */, void* hip_stream);
/* Host memory in and out, through a device scratch the handle owns and grows; returns when the answers are in place. */
int gndt_shortcut_routes(gndt_handle* h, const uint32_t* route_rows_host, size_t K, uint32_t route_cap,
                         const void* lengths_host, size_t length_stride_bytes,
                         const gndt_robot* robot, const gndt_shortcut_params* params, const uint32_t* hops_host,
                         uint32_t* waypoint_rows_host, uint32_t waypoint_cap, uint32_t* path_rows_host, uint32_t path_cap,
                         gndt_shortcut_info* info_host);

/* ---- footprint poses: fitted plane, tilt, step and headroom under a rectangular vehicle ----------------------------------------
 * A vehicle is not a point.  Standing at (x, y) with a heading it asks what surface its footprint rests on, how far that surface
 * tilts along and across the heading, whether a kerb or a hole lies under it, how much of it stands on unknown ground, and what
 * hangs over it.  Every slope of the map is a Gaussian (count, mean, scatter); the Gaussians under a rectangle merge in closed form
 * and the smallest eigenpair of the merged scatter is the supporting plane.  One call takes K poses: five floats x, y, z, hx, hy at
 * poses + k * stride_bytes (any multiple of 4 from 20 up).  (hx, hy) is the heading as a VECTOR of any non-zero length, not an
 * angle: which column lies under the vehicle is then decided by + and x in fp64 alone (the library is built without contraction),
 * and no sine or cosine of any libm enters an answer.  The rectangle reaches half_length along the heading and half_width across
 * it, both ways.  `robot` NULL = the flood's defaults; only reachable_height and max_angle_deg are read.  Per pose, in this order:
 *   1. pose      a non-finite field, or hx == hy == 0: status GNDT_FOOT_BAD_POSE.
 *   2. centre    the row GNDT_QUERY_NEAREST_SLOPE finds for (x, y, z) (the point queries' own lookup).  None: GNDT_FOOT_NO_GROUND.
 *                z0 = its mean z (fp32), (cx, cy) = its column.
 *   3. box       n = ceil(sqrt(half_length^2 + half_width^2) / grid_len), formed once on the host in fp64 from the floats widened
 *                (n >= 1; n > 15 is refused: (2n + 1)^2 <= 1024 bounds a lane's loop and a wavefront's table).  The box is the
 *                (2n + 1)^2 columns around (cx, cy): per axis the n non-zero signed indices below the centre's, the centre's and
 *                the n above (signed indices skip 0, as the raster export steps them).  Box position p = j (2n + 1) + i, i over
 *                x ascending, j over y ascending; the centre column is p = n (2n + 1) + n.
 *   4. inside    with the column's centre per axis o + sign(s) (|s| - 0.5) grid_len in fp64 (o and grid_len widened), all in fp64:
 *                dx = centre_x - x, dy = centre_y - y, u = dx hx + dy hy, v = dy hx - dx hy, hh = hx hx + hy hy; the column is
 *                under the vehicle iff u u <= (half_length half_length) hh and v v <= (half_width half_width) hh.  The centre
 *                column is under the vehicle whatever the rounding.  `cells` counts the columns under the vehicle.
 *   5. support   a column under the vehicle whose index lies beyond +-65535, or that holds no node, is `unknown`.  Otherwise, among
 *                its rows with GNDT_FLAG_SLOPE and fabsf(mean_z - z0) <= max_dz in fp32 (all of them when max_dz is 0), the one
 *                with the least fabsf(mean_z - z0), a tie going to the smaller sz (the query's rule), is its support; a column
 *                with no such row is a `gap`.  The centre column's support is the centre row.  `support`, `gaps` and `unknown`
 *                count these; cells = support + gaps + unknown.
 *   6. merge     over the supports, in fp64, about the point (x, y, z0): d = mean - (x, y, z0) (each float widened first),
 *                w = 1 (GNDT_FOOT_WEIGHT_CELL) or count (GNDT_FOOT_WEIGHT_COUNT), s = w / count;
 *                W = sum w;  M_a = sum (w d_a);  Q_ab = sum ((w d_a) d_b + s cov_ab), cov the row's un-normalised scatter;
 *                dbar_a = M_a / W;  S_ab = Q_ab - (W dbar_a) dbar_b.
 *                THE ORDER OF EVERY SUM is fixed by box position alone — never by arrival, by K, or by where the pose sits in the
 *                batch: 64 partial sums l = 0 .. 63, each starting from +0 and adding the terms of the supports at positions
 *                p = l, l + 64, l + 128, ... in ascending p; then six rounds offset = 32, 16, 8, 4, 2, 1 in each of which every
 *                partial l becomes partial[l] + partial[l ^ offset] (all 64 at once); the sum is partial 0.
 *                support < min_cells (0 = 3): status GNDT_FOOT_SPARSE, the counts and centre_row are reported, flags and every
 *                float field are 0.
 *   7. plane     (lambda, nrm) = the smallest eigenpair of S (the build's solver without its fp32 trigonometric start value:
 *                only +, x, / and sqrt in fp64, so that a host run of the same code returns the device's bits), nrm negated if
 *                nrm_z < 0.
 *                rms = sqrt(max(lambda, 0) / W);  z = (z0 + dbar_z) + (nrm_x dbar_x + nrm_y dbar_y) / nrm_z, the plane's height at
 *                (x, y);  with rh = sqrt(hh), f = (hx / rh, hy / rh):  along = -(nrm_x f_x + nrm_y f_y) / nrm_z,
 *                across = -(nrm_y f_x - nrm_x f_y) / nrm_z — rise per metre along the heading and to its left; fp64, rounded to
 *                fp32 once.  The library takes no arctangent: pitch = atan(along), roll = atan(across) are the caller's.
 *                nrm_z == 0: z = z0 + dbar_z, along = across = 0 (and GNDT_FOOT_TILT is set by 9).
 *   8. shape     step_max: the largest fabsf(mean_z(a) - mean_z(b)) in fp32 over the supports a, b of two 4-adjacent box columns
 *                that both have one (0 if none).  bump_max: the largest |(nrm_x e_x + nrm_y e_y) + nrm_z e_z| over the supports,
 *                e = d - dbar, fp64, rounded once.  headroom: over the rows t of the support columns with GNDT_FLAG_HAS_STATS and
 *                mean_z(t) > mean_z(support) + reachable_height (fp32), the least of mean_z(t) - zp, zp the plane's height at the
 *                column's centre, (z0 + dbar_z) - (nrm_x (ex - dbar_x) + nrm_y (ey - dbar_y)) / nrm_z with (ex, ey) = (dx, dy) of
 *                4 (z0 + dbar_z where nrm_z == 0); fp64, rounded once; FLT_MAX if there is none.
 *   9. verdict   bits in `flags`: GNDT_FOOT_TILT nrm_z < cos(max_angle_deg) (the cosine formed once on the host in fp64);
 *                GNDT_FOOT_STEP step_max > reachable_height; GNDT_FOOT_COVER support < min_cover * cells in fp64; GNDT_FOOT_LOW
 *                height > 0 and headroom < height.  Status GNDT_FOOT_OK with flags 0 means "stands here".
 * rows_dev (optional, NULL together with row_cap 0) receives per pose row_cap entries: the supports in box order, GNDT_NO_ROW behind
 * them (all GNDT_NO_ROW for BAD_POSE and NO_GROUND); more supports than row_cap write the first row_cap and the caller sees
 * support > row_cap.  info is written 16 bytes at a time: info_dev must be aligned to 16 bytes.  A box holds at most 961 columns, so
 * the four counts are 16-bit.  Order, lifetime and refusals are the walk call's: the call first finishes what gndt_sync finishes,
 * builds or reuses the map's column index and enqueues its kernel on `hip_stream` (NULL = the handle's stream), not awaited;
 * gndt_footprint_poses is synchronous and takes host memory of any alignment.  The map, h and state are only read and no cost map
 * is needed.  K == 0 returns GNDT_OK and launches nothing.  There is no CPU path.  A sharded map answers from the rows this rank
 * holds.  GNDT_ERR_INVALID: a null handle, params or info, null poses with K > 0, K * 1024 >= 2^31, a stride below 20 or not a
 * multiple of 4, a half extent that is not finite or not greater than 0, a box beyond n = 15, max_dz, height or min_cover negative
 * or not finite, an unknown weight, a non-zero reserved word, rows NULL with row_cap != 0 or the reverse, info_dev not aligned to 16
 * bytes or poses_dev, rows_dev not to 4, no finished build, a stream under hipGraph capture. */
enum { GNDT_FOOT_OK = 0, GNDT_FOOT_BAD_POSE = 1, GNDT_FOOT_NO_GROUND = 2, GNDT_FOOT_SPARSE = 3 };
enum { GNDT_FOOT_WEIGHT_CELL = 0, GNDT_FOOT_WEIGHT_COUNT = 1 };
#define GNDT_FOOT_TILT 1u
#define GNDT_FOOT_STEP 2u
#define GNDT_FOOT_COVER 4u
#define GNDT_FOOT_LOW 8u
typedef struct gndt_footprint_params {
    float half_length;        /* metres along the heading, each way; finite, > 0 */
    float half_width;         /* metres across the heading, each way; finite, > 0 */
    float max_dz;             /* supports lie within this of the centre slope's mean z; 0 = no band */
    float height;             /* the vehicle's height for GNDT_FOOT_LOW; 0 = no headroom verdict */
    uint32_t min_cells;       /* fewer supports: GNDT_FOOT_SPARSE; 0 = 3 */
    float min_cover;          /* share of `cells` that must be supports, for GNDT_FOOT_COVER; 0 = none */
    uint32_t weight;          /* GNDT_FOOT_WEIGHT_* */
    uint32_t reserved[5];     /* 0 */
} gndt_footprint_params;      /* 48 bytes; zeros = defaults (the half extents have none) */
typedef struct gndt_footprint_info {
    int32_t status;           /* GNDT_FOOT_OK / _BAD_POSE / _NO_GROUND / _SPARSE */
    uint32_t flags;           /* GNDT_FOOT_TILT | _STEP | _COVER | _LOW */
    uint32_t centre_row;      /* GNDT_NO_ROW without a centre */
    uint16_t cells, support;  /* columns under the vehicle; those with a support */
    uint16_t gaps, unknown;   /* those in the map without a support; those not in the map */
    float z;                  /* the plane's height at (x, y) */
    float normal[3];          /* unit, normal[2] >= 0 */
    float along, across;      /* rise per metre */
    float rms;
    float step_max, bump_max, headroom;
    uint32_t reserved;        /* 0 */
} gndt_footprint_info;        /* 64 bytes */
/* Device memory in and out. */
int gndt_footprint_poses_device(gndt_handle* h, const void* poses_dev, size_t K, size_t stride_bytes, const gndt_robot* robot,
                                const gndt_footprint_params* params, uint32_t* rows_dev /* [K * row_cap] or NULL */, uint32_t row_cap,
                                gndt_footprint_info* info_dev /* [K] */, void* hip_stream);
/* Host memory in and out, through a device scratch the handle owns and grows; returns when the answers are in place. */
int gndt_footprint_poses(gndt_handle* h, const void* poses_host, size_t K, size_t stride_bytes, const gndt_robot* robot,
                         const gndt_footprint_params* params, uint32_t* rows_host, uint32_t row_cap, gndt_footprint_info* info_host);

/* ---- free-space clearing: nodes that sensor rays pass through leave the map -------------------------------------------------
 * What was seen once and is gone now — a person, a car, an open door — leaves nodes that change its columns' labels (isSlope,
 * map2D.h:66-108) and that the cost flood routes around for as long as the map lives (the reference's changeCallback only adds).
 * One call takes a sensor origin o (finite and keyed by the codec) and n end points p_i in map coordinates (stride 12 or 16, like
 * gndt_build_device).  Every finite end point whose key is in the codec's range defines one ray (stats.rays); the others are skipped
 * (stats.skipped).
 * The walk of a ray is a DEFINITION, not an approximation (tests restate it in numpy, bit for bit):
 *   - cut point: e = o + d * min(1, max_range / |d|, max(0, |d| - end_margin) / |d|), d = p - o, all in fp64 (e = p when nothing
 *     is cut; max_range = 0: no limit).  A ray with |d| = 0 walks only the origin's voxel.
 *   - first and last column: the codec's (sx, sy) of o and of e (point_key / axis_index in fp32, exactly as the build keys points).
 *   - steps: exactly |dx| + |dy| unit steps between them, measured in lattice cells (signed indices skip 0: positive index s is the
 *     cell between the planes s - 1 and s, negative index s the cell between s and s + 1, in grid_len from the map origin).  Each step
 *     crosses the lattice plane the segment meets first: crossing parameter t = (o_axis + k * grid_len - o_ray) / d_axis in fp64,
 *     clamped to [0, 1], with o_axis the map origin and d_axis the uncut direction; an axis whose index has reached the last column's
 *     is not stepped again; a tie steps x first.
 *   - levels: in every column the ray walks every level between its level at the column's entry and at its exit, inclusive (0 skipped):
 *     the first column's entry level is the codec's sz of o, the last column's exit level the codec's sz of e, a crossing's level is the
 *     codec's rule in fp64 at the ray's z there: sign(z - oz) * max(1, ceil(|z - oz| / z_len)).  Both ends' voxels are walked.
 * A node is PASSED by a ray when the walk visits its (sx, sy, sz).  A node is PROTECTED when the GNDT_QUERY_NODE lookup of some ray's
 * UNCUT end point p_i names it (something was seen in it in this call; the query's own code).
 * Clearing: a node leaves the map when its passes are >= min_passes and it is not protected — with everything it has, with or without
 * statistics or a slope.  By definition
 *     clear  ==  gndt_remove of every point ever added to the nodes that leave,
 * so survivors keep first_idx and their place in the order, the stream position stays, every row is re-finalised (the labels of the
 * touched columns change as isSlope says they must), and a cleared node that receives points again is a new node.  Clearing needs the
 * additive node table, as gndt_remove does (strategy ATOMIC / TILE or a map built by gndt_update*); otherwise GNDT_ERR_INVALID and the
 * map is unchanged.
 * GNDT_CLEAR_COUNT_ONLY: the same walk, and nothing changes — a dry run, and a read-only "which parts of the map does this scan see
 * through" query.  It works on every map that has rows (PARTITION-built and sharded ones: the rows this rank holds), as queries do.
 * passes_out (optional, num_nodes u32, indexed by the rows as they were BEFORE the call): bits 0-30 the pass count, bit 31
 * (GNDT_CLEAR_PROTECTED) a protected row.  Count-only: exact counts (n < 2^31, so they cannot saturate).  While clearing the kernel
 * stops adding to a row once it has min_passes, and adds nothing to a protected row: the count of a row that is not protected is
 * min(exact, min_passes), that of a protected row 0.
 * stats (optional): rays, skipped points, protected rows, nodes cleared (0 in count-only mode).
 * GNDT_ERR_INVALID: null handle, origin or params, null points with n > 0, n >= 2^31, a non-finite origin or one without a key, a
 * negative or non-finite max_range / end_margin, min_passes == 0, unknown flags, a stride other than 12 / 16, no finished build, a
 * stream under hipGraph capture (a clear is not recorded), clearing without the node table.  There is no CPU path: without a device
 * the call fails like every compute entry point.  n == 0 returns GNDT_OK and changes nothing.
 * Order and lifetime are gndt_crop's:
 *   - the call first finishes what gndt_sync finishes (a pending build, a deferred emit, a re-run), then builds or reuses the map's
 *     column index (the one the point queries and the flood use);
 *   - clearing makes a new map: the cost map is invalid until the next gndt_compute_cost (gndt_cost_export* refuse it), the column
 *     index is rebuilt, device pointers from gndt_export_device and row numbers from gndt_query* are invalid, and a graph recorded before
 *     the clear and replayed after it is reported stale by gndt_sync (GNDT_ERR_CAPACITY).  Capture again after the clear.
 * Clearing waits for the device, as gndt_remove does: deaths are only known there.  A count-only gndt_clear_rays_device is enqueued on
 * `hip_stream` (NULL = the handle's stream, the rules of gndt_build_device) and not awaited unless `stats` is non-NULL.
 * gndt_clear_rays takes host points and a host passes_out and is synchronous. */
enum { GNDT_CLEAR_COUNT_ONLY = 1 };
#define GNDT_CLEAR_PROTECTED 0x80000000u
typedef struct gndt_clear_params {
    float max_range;      /* > 0: walk at most this far from the origin; 0 = no limit            */
    float end_margin;     /* >= 0: the last end_margin metres before an end point are not walked */
    uint32_t min_passes;  /* >= 1 */
    uint32_t flags;       /* GNDT_CLEAR_* */
} gndt_clear_params;
typedef struct gndt_clear_stats {
    uint64_t rays, skipped, protected_rows, cleared;   /* cleared = 0 in count-only mode */
} gndt_clear_stats;
int gndt_clear_rays_device(gndt_handle* h, const float origin_xyz[3], const void* xyz_dev, size_t n, size_t stride_bytes,
                           const gndt_clear_params* p, uint32_t* passes_out_dev, gndt_clear_stats* stats, void* hip_stream);
int gndt_clear_rays(gndt_handle* h, const float origin_xyz[3], const void* xyz_host, size_t n, size_t stride_bytes,
                    const gndt_clear_params* p, uint32_t* passes_out_host, gndt_clear_stats* stats);

/* ---- scan scoring: how well a scan fits the map at each of K poses -----------------------------------------------------------
 * The map is a grid of normal distributions (count, mean, scatter per node); this call reads it as one: the NDT match score of n scan
 * points (fp32, stride 12 or 16, like gndt_build_device) for K poses, each a row-major 3 x 4 double matrix [R | t] (nothing checks that
 * R is a rotation).  No optimiser, no derivatives: the sum a localisation health check, a particle filter's weighting step, a pose
 * search or a registration loop is built on.
 * The score is a DEFINITION (tests restate it in numpy).  For pose k and point p = (x, y, z):
 *   1. transform, in fp64, in this order, rounded once to fp32 per coordinate: q_i = (float)(((R_i0 x + R_i1 y) + R_i2 z) + t_i).
 *      Everything after this step sees only the fp32 q: scoring cloud P at pose T and scoring fl32(T P) at the identity are the same
 *      computation.
 *   2. key: q's key as GNDT_QUERY_NODE keys a point (finite, and all three axes in the codec's range).  No key: the point contributes
 *      nothing for this pose (not an error).
 *   3. candidates: GNDT_SCORE_DIRECT1 the node with that key; GNDT_SCORE_DIRECT7 also its six face neighbours, by the index rules of the
 *      cost flood, which skip 0: (sx -+ 1, sy, sz), (sx, sy -+ 1, sz), (sx, sy, level above / below sz).  A neighbour index beyond the
 *      codec's range (|sx|, |sy| > 65535, |sz| >= 2^21) is no candidate.  A candidate counts when the map holds it and its
 *      count >= min_count.
 *   4. term of a candidate with c = count, mean m and scatter S (gndt_cells.cov, un-normalised), in fp64 from the rows' fp32 values:
 *      C = S / (c - 1); eps = max(cov_rel * (C_xx + C_yy + C_zz) / 3, cov_floor); A = C + eps I; d = q - m; d2 = d^T A^-1 d by the
 *      adjugate (cofactors, one division by the determinant; grid_ndt_amd/csrc/gndt_score.hpp states the evaluation order);
 *      term = exp(-d2 / 2).  With max_d2 > 0 a candidate whose d2 > max_d2 does not count.
 *   5. per pose: score = the sum of the terms, d2_sum = the sum of their d2, terms = how many, matched = how many points had at least
 *      one.
 *   6. per point, optional, for the one pose `point_pose`: the least d2 among the point's terms as fp32 (+inf: none) and that node's row
 *      (GNDT_NO_ROW: none; equal d2: the lower row) — which points of the scan disagree with the map.
 * Parameters, 0 = default: min_count = max(the handle's min_points, 3); cov_rel = 0.01f; cov_floor = 1e-6f (m^2); max_d2 = 0 is no
 * gate.  eps is therefore always positive and A never singular; with cov_rel = 0.01 the condition number of A is at most 301 whatever
 * the node's shape (a rank-1 node of three collinear points included).
 * Results are reproducible to the bit: sums are formed per thread, then in a fixed tree per tile of 256 points, then over a pose's
 * tiles in tile order — no floating-point atomics.  Pose k of a batch has exactly the bits a single-pose call of that pose gives, on
 * any stream, at either stride.
 * Order and lifetime are the point queries': the call first finishes what gndt_sync finishes (a pending build, a deferred emit, a
 * re-run), then builds or reuses the map's column index, then enqueues its kernels on `hip_stream` (NULL = the handle's stream, the
 * rules of gndt_build_device) and does not wait.  The map is not modified.  Row numbers stay valid until the next build, update, remove,
 * crop, clear or reset.  A sharded map answers from the rows this rank holds (the caller adds the ranks' records).  There is no CPU
 * path.  n == 0 with K > 0 writes K zeroed records; K == 0 returns GNDT_OK and launches nothing.
 * GNDT_ERR_INVALID: null handle or params, null points with n > 0, null poses or out with K > 0, K > 65535, a stride other than 12 / 16,
 * an unknown neighbourhood, point_pose >= K when a per-point output is asked for, min_count of 1 or 2 or below the handle's min_points
 * (such nodes keep zero statistics), a negative or non-finite cov_rel, cov_floor or max_d2, no finished build, a stream under hipGraph
 * capture (a score is not recorded). */
enum { GNDT_SCORE_DIRECT1 = 1, GNDT_SCORE_DIRECT7 = 7 };
typedef struct gndt_score_params {
    int32_t neighbourhood;   /* GNDT_SCORE_DIRECT1 / GNDT_SCORE_DIRECT7                          */
    int32_t min_count;       /* 0 = max(min_points, 3)                                           */
    float cov_rel;           /* 0 = 0.01                                                         */
    float cov_floor;         /* 0 = 1e-6 (m^2)                                                   */
    float max_d2;            /* > 0: candidates beyond this d2 do not count; 0 = no gate         */
    uint32_t point_pose;     /* the pose the per-point outputs are written for (< K)             */
} gndt_score_params;
typedef struct gndt_pose_score {
    double score, d2_sum;
    uint64_t matched, terms;
} gndt_pose_score;           /* 32 bytes */
/* Device points, poses ([K][12] doubles), records ([K]) and per-point outputs ([n] each, either may be NULL). */
int gndt_score_poses_device(gndt_handle* h, const void* xyz_dev, size_t n, size_t stride_bytes, const double* poses_dev, uint32_t K,
                            const gndt_score_params* params, gndt_pose_score* out_dev, float* point_d2_dev, uint32_t* point_row_dev,
                            void* hip_stream);
/* The same with host memory, through a device scratch the handle owns and grows; synchronous. */
int gndt_score_poses(gndt_handle* h, const void* xyz_host, size_t n, size_t stride_bytes, const double* poses_host, uint32_t K,
                     const gndt_score_params* params, gndt_pose_score* out_host, float* point_d2_host, uint32_t* point_row_host);

/* ---- scan segmentation: the points of a scan that the map does not explain, clustered into objects ---------------------------------
 * What a robot asks of every frame next to "how well does it fit" (scan scoring): what in this scan is NOT in the map, and where are
 * those things — a person, a parked car, a pallet that was not there when the map was made.  The answer is a list of clusters (boxes for
 * gndt_walk_paths / gndt_footprint_poses obstacles), a label per point (the points not to gndt_update the map with) and four counts (a
 * localisation health signal).  Everything after the classification is integer arithmetic: the answer is exact and does not depend on
 * the order threads work in.  lin(s) = s > 0 ? s - 1 : s, as in "frontier extraction": signed indices skip 0 on all three axes.
 * A DEFINITION (tests restate it in numpy).  For point i = (x, y, z) of n (fp32, stride 12 or 16):
 *   1. transform and key: steps 1 and 2 of "scan scoring" — q = fl32(T p) for the one pose `pose` ([12] doubles; NULL = the identity,
 *      q = p), then q's GNDT_QUERY_NODE key (sx, sy, sz).  A point without a key has class GNDT_SEG_UNKEYED.
 *   2. class: candidates and terms are steps 3 and 4 of "scan scoring" with this call's neighbourhood, min_count, cov_rel, cov_floor
 *      (the same defaults) and max_d2 = 0.  d2_i = the least d2 of the point's counting candidates, rounded to fp32 — the very number
 *      gndt_score_poses* reports per point (+inf: no candidate counts).
 *        GNDT_SEG_EXPLAINED    d2_i <= novel_d2           (novel_d2 0 = 11.345f, the 0.99 quantile of chi^2 with 3 degrees of freedom)
 *        GNDT_SEG_OFF_SURFACE  candidates count, but d2_i > novel_d2
 *        GNDT_SEG_UNMAPPED     no candidate counts
 *      A point is NOVEL when `classes` (a mask of 1u << class; 0 = OFF_SURFACE | UNMAPPED) holds its class.
 *   3. cell: a novel point's cell is its key in the map's grid.  A NOVEL CELL is a cell with at least min_points novel points (0 = 1);
 *      its id is the smallest index of its novel points.
 *   4. link: two different novel cells a, b are linked under connectivity 26 (0 = 26) when |lin(s_a) - lin(s_b)| <= 1 on all three
 *      axes, under 6 when the three differences add up to 1.  An index beyond the codec's range (|sx|, |sy| > 65535, |sz| >= 2^21) does
 *      not exist.
 *   5. cluster: a connected component of the links; its label is the smallest id of its cells: the smallest index of its points.
 *   6. record (gndt_scan_cluster): label; cells; off_surface / unmapped, the cluster's points by class (points = their sum: the novel
 *      points of its cells); the bounds of its cells' signed indices; sum_x / _y / _z, each the sum over its points of
 *      llrint((double)q * 1024.0) (round to nearest even; integer, so exact in any order: centroid = sum / points / 1024); z_lo / z_hi,
 *      the least and greatest q_z of its points (compared through the order-preserving integer image of the float: -0 below +0).
 * Outputs: clusters[] holds the clusters with at least min_cluster_points points and min_cluster_cells cells (0 = 1 for both) in
 * ascending label, the first cluster_cap of them (nothing is written behind those); counts[0] is how many there are — it may exceed
 * cluster_cap (cluster_cap 0 with clusters NULL only counts) — counts[1] the novel points, counts[2] the novel cells, counts[3] the
 * clusters of any size.  point_class[i] (optional) is the class of step 2; point_label[i] (optional) the label of the point's cluster,
 * GNDT_NO_ROW for a point that is not novel or whose cell has fewer than min_points; the cluster-size filters do not filter labels.
 * Order and lifetime are scan scoring's and the frontiers': the call first finishes what gndt_sync finishes, builds or reuses the map's
 * column index and enqueues its kernels on `hip_stream` (NULL = the handle's stream), not awaited; gndt_segment_scan is synchronous.  The
 * map is not modified.  Work memory belongs to the handle and grows; its size is a function of n alone, so nothing waits for the host:
 * a table of the smallest power of two >= max(2 n, 1024) slots of 16 bytes for the cells (n cells in n points stay at or below half
 * load) and 17 bytes a point, 81 bytes a point at the most.  n == 0 writes four zero counts.  A sharded map answers from the rows this
 * rank holds.  There is no CPU path.
 * GNDT_ERR_INVALID: a null handle, params or counts, null points with n > 0, n >= 2^32, a stride other than 12 / 16, an unknown
 * neighbourhood or connectivity, min_count of 1 or 2 or below the handle's min_points, a negative or non-finite cov_rel, cov_floor or
 * novel_d2, a `classes` bit other than OFF_SURFACE's and UNMAPPED's, a non-zero reserved word, clusters NULL with cluster_cap > 0 or the
 * reverse, a device pointer not aligned as its type is, no finished build, a stream under hipGraph capture (the call is not recorded).
 * GNDT_ERR_CAPACITY: n > 2^30 (the cell table would pass 2^31 slots). */
enum { GNDT_SEG_UNKEYED = 0, GNDT_SEG_EXPLAINED = 1, GNDT_SEG_OFF_SURFACE = 2, GNDT_SEG_UNMAPPED = 3 };
typedef struct gndt_segment_params {
    int32_t  neighbourhood;        /* GNDT_SCORE_DIRECT1 / GNDT_SCORE_DIRECT7                              */
    int32_t  min_count;            /* 0 = max(min_points of the handle, 3)                                 */
    float    cov_rel;              /* 0 = 0.01                                                             */
    float    cov_floor;            /* 0 = 1e-6 (m^2)                                                       */
    float    novel_d2;             /* 0 = 11.345                                                           */
    uint32_t classes;              /* mask of 1u << class; 0 = OFF_SURFACE | UNMAPPED                      */
    uint32_t min_points;           /* novel points that make a cell novel; 0 = 1                           */
    uint32_t connectivity;         /* 26 or 6; 0 = 26                                                      */
    uint32_t min_cluster_points;   /* clusters with fewer points are left out of the list; 0 = 1           */
    uint32_t min_cluster_cells;    /* ... or with fewer cells; 0 = 1                                       */
    uint32_t reserved[2];          /* 0 */
} gndt_segment_params;             /* 48 bytes */
typedef struct gndt_scan_cluster { /* 72 bytes */
    uint32_t label, cells, off_surface, unmapped;
    int32_t  sx_min, sx_max, sy_min, sy_max, sz_min, sz_max;
    int64_t  sum_x, sum_y, sum_z;
    float    z_lo, z_hi;
} gndt_scan_cluster;
/* Device points, pose ([12] doubles or NULL), per-point outputs ([n] each, either may be NULL), clusters ([cluster_cap]), counts ([4]). */
int gndt_segment_scan_device(gndt_handle* h, const void* xyz_dev, size_t n, size_t stride_bytes, const double* pose_dev,
                             const gndt_segment_params* params, uint8_t* point_class_dev, uint32_t* point_label_dev,
                             gndt_scan_cluster* clusters_dev, uint32_t cluster_cap, uint32_t* counts_dev /* [4] */, void* hip_stream);
/* The same with host memory, through a device scratch the handle owns and grows; synchronous. */
int gndt_segment_scan(gndt_handle* h, const void* xyz_host, size_t n, size_t stride_bytes, const double* pose_host,
                      const gndt_segment_params* params, uint8_t* point_class_host, uint32_t* point_label_host,
                      gndt_scan_cluster* clusters_host, uint32_t cluster_cap, uint32_t* counts_host);

/* ---- obstacle field: hops to transient obstacles for every slope ----------------------------------------------------------------
 * What gndt_walk_paths* and gndt_shortcut_routes* take as `hops` when the barrier is not in the map: a list of boxes of signed cell
 * indices — the clusters gndt_segment_scan* has just found, a keep-out zone, a virtual wall, another robot's announced footprint —
 * turned into "0 on the slopes a box stands on, 1, 2, ... on the slopes that many steps away", optionally already minimised with a
 * gndt_clearance* field.  The map is not changed: next frame the pallet has moved on and so has the field.  This is a DEFINITION:
 * only the flood's three gates are floating point (the clearance field's steps), everything else is integer arithmetic, so the answer
 * is exact and does not depend on the order threads work in.  lin(s) = s > 0 ? s - 1 : s; all sums are taken in 64 bits.
 *   1. boxes      box b is six int32 sx_min, sx_max, sy_min, sy_max, sz_min, sz_max read at boxes + b * box_stride_bytes (a multiple
 *                 of 4, at least 24; the pointer 4-aligned): &clusters[0].sx_min with stride sizeof(gndt_scan_cluster) reads
 *                 segmentation's records where they lie.  B = n_boxes, with n_boxes_dev min(*n_boxes_dev, n_boxes) read on the device
 *                 (segmentation's counts[0] may exceed its list's capacity).  A box with min > max on any axis is VOID.
 *   2. window     K = inflate + max_hops.  On x the window of a box that is not void is the set of indices that exist (non-zero,
 *                 |s| <= 65535) with lin in [lin(sx_min) - K, lin(sx_max) + K]; the same on y; w_b is the product of the two counts
 *                 (it may be 0) and W_b the inclusive prefix sum of w over the boxes that are not void, in index order.  Box b is
 *                 ADMITTED when it is not void and W_b <= max_columns; every other box that is not void is DROPPED: it covers
 *                 nothing and is counted — the caller reads the count and splits the box or raises the budget.
 *   3. covered    a row q with GNDT_FLAG_SLOPE is covered by an admitted box b when lin(sx_min) - inflate <= lin(sx_q) <=
 *                 lin(sx_max) + inflate, the same on y, lin(sz_min) <= lin(sz_q) + levels_above and lin(sz_max) >= lin(sz_q) -
 *                 levels_below (the robot's body in levels: an obstacle on a bridge does not block the ground under it).
 *   4. in reach   a slope whose column lies in an admitted box's window (z plays no part).
 *   5. field      steps are the clearance field's (a directed graph).  hops(q) is the length of the shortest walk from q along steps
 *                 to a covered slope, 0 on a covered slope, GNDT_CLEARANCE_BEYOND beyond max_hops (0 = 8; above 1024 is refused) and
 *                 for a row without a slope.  obstacle(q) is the smallest box index among the boxes covering the covered slopes
 *                 exactly hops(q) steps from q, GNDT_NO_ROW where hops is BEYOND: the clearance key hops << 32 | index under an
 *                 unsigned minimum.  A walk of at most max_hops steps to a slope covered by b never leaves b's window (a step moves
 *                 one column along one axis, over the missing index 0 too), so the search visits the rows in reach only.
 *   6. outputs    hops[q] = min(base_hops[q], hops(q)) with a base (base_hops_dev == hops_dev is allowed), obstacle[q] ignores the
 *                 base; both have num_nodes entries, every entry is written; either may be NULL, not both.  counts[8]: the covered
 *                 slopes, the slopes with finite obstacle hops, the largest finite obstacle hops, B, the admitted boxes that cover at
 *                 least one slope, the slopes in reach, the dropped boxes, 0.
 * B == 0 or a map without rows writes the base (or BEYOND / NO_ROW) and counts that are zero except counts[3].  `robot` NULL = the
 * flood's defaults.  Order and lifetime are the clearance call's: the call first finishes what gndt_sync finishes, builds or reuses the
 * map's column index and enqueues its kernels on `hip_stream` (NULL = the handle's stream), not awaited — B, the prefix sums and the
 * list of rows in reach stay on the device, one launch per hop, of which those behind the last hop that changed anything return at
 * once.  Only the fill of the two outputs passes over the map; the marking pass takes one thread per column of the admitted windows
 * (at most max_columns: 0 = 2^24, above 2^28 is refused), the steps and the hops the rows of the columns in reach.
 * gndt_obstacle_field is synchronous.  Neither the map nor the cost map is modified and no cost map is needed.  Work memory belongs to
 * the handle and grows: room for 53 bytes per row of a column in reach, reserved for every row of the map (a window may hold them
 * all); 16 bytes a map row of marks that are stamped per call, so never cleared; 12 bytes a box.  There is no CPU path.  A sharded map
 * answers from the rows this rank holds.
 * GNDT_ERR_INVALID: a null handle, params, boxes (with n_boxes > 0) or counts, hops and obstacle both NULL, a stride below 24 or not a
 * multiple of 4, boxes or a device pointer not aligned to 4 bytes, n_boxes > 2^20, inflate > 1024, max_hops > 1024, max_columns >
 * 2^28, a non-zero reserved word, no finished build, a stream under hipGraph capture (the call is not recorded). */
typedef struct gndt_obstacle_params {
    uint32_t inflate;        /* columns added round a box on x and y (Chebyshev, in lin space); above 1024 is refused */
    uint32_t max_hops;       /* 0 = 8; above 1024 is refused */
    uint32_t levels_above;   /* the robot's body: levels above a slope's own that an obstacle blocks it from */
    uint32_t levels_below;   /* ... and below */
    uint64_t max_columns;    /* budget for the windows' columns of one call; 0 = 2^24; above 2^28 is refused */
    uint32_t reserved[2];    /* 0 */
} gndt_obstacle_params;      /* 32 bytes */
/* Device boxes, n_boxes_dev (one uint32 or NULL), base_hops_dev ([num_nodes] or NULL), hops_dev, obstacle_dev ([num_nodes], either or NULL), counts_dev ([8]). */
int gndt_obstacle_field_device(gndt_handle* h, const gndt_robot* robot, const void* boxes_dev, uint32_t n_boxes, size_t box_stride_bytes,
                               const uint32_t* n_boxes_dev, const gndt_obstacle_params* params, const uint32_t* base_hops_dev,
                               uint32_t* hops_dev, uint32_t* obstacle_dev, uint32_t* counts_dev /* [8] */, void* hip_stream);
/* The same with host memory, through a device scratch the handle owns and grows; synchronous. */
int gndt_obstacle_field(gndt_handle* h, const gndt_robot* robot, const void* boxes_host, uint32_t n_boxes, size_t box_stride_bytes,
                        const gndt_obstacle_params* params, const uint32_t* base_hops_host, uint32_t* hops_host, uint32_t* obstacle_host,
                        uint32_t* counts_host);

/* ---- route field: cost-to-go to a set of goals for every slope, keeping clear of obstacles, and the routes it gives ----------------
 * A navigation function.  What the flood's h is not: the LEAST cost to reach ANY of G goals along the steps a robot can take, never
 * entering a slope the caller's `hops` field (a gndt_clearance* or gndt_obstacle_field* output) forbids, with the slope to step to
 * next.  One field serves every start, any number of robots and every re-plan until the map or the obstacles change: cost[row] is a
 * rollout's h_end, and following `next` from a start is a route in the layout gndt_plan_routes* writes and gndt_shortcut_routes*
 * takes.  Every definition is fp32 arithmetic in a stated order under an unsigned minimum: the answer is exact and does not depend on
 * the order threads work in.
 *   graph         the clearance field's: the steps of slope q through side k are the rows t of that neighbour column that have
 *                 GNDT_FLAG_SLOPE and pass the flood's gates seen from q.  Directed.  `robot` NULL = the flood's defaults.
 *   entering      a step q -> t may be taken only if t may be entered.  A row t may NOT be entered when hops_dev != NULL and
 *                 hops_dev[t] < min_hops (the caller vouches for hops_dev exactly as for the walks: num_nodes entries OF THIS MAP AS IT
 *                 IS NOW), or when GNDT_WALK_CHECK_OVERHEAD is set in `checks` and the clearance field's OVERHEAD predicate holds for t.
 *                 A slope that may not be entered still gets a field value from its own steps: a robot that finds itself inside the
 *                 inflated zone is shown the way out, but no route passes through it.
 *   step cost     c(q, t) = fl(TravelCost(mean q, mean t) * w(t)), fp32, never contracted; TravelCost is the flood's (fp32 differences,
 *                 squares and root in fp64, rounded once).  w(t) = 1 without hops or when hops[t] >= soft_hops (soft_hops 0: no
 *                 penalty), else fl(1.0f + fl(soft_weight * (float)(soft_hops - hops[t]))).  soft_weight must be finite and >= 0.
 *   goals         G rows (uint32) with optional goal_cost[G] (fp32; NULL = zeros; -0 counts as 0).  A goal is IGNORED, and counted,
 *                 when its row is out of range, has no slope or may not be entered, or when its cost is not finite or is negative.
 *                 The same row given twice keeps its least cost; every accepted entry counts.
 *   field         cost(q) is the least, over walks q -> ... -> g along steps that end on an accepted goal, of the value accumulated
 *                 from the goal backwards: v(g) = goal_cost(g), v(p) = fl(c(p, next) + v(next)).  It is the fixed point, reached from
 *                 above, of
 *                     key(q) = min(seed(q), min over steps t of q that may be entered of bits(fl(c(q, t) + cost(t))) << 32 | t)
 *                 under an unsigned 64-bit minimum, seed = bits(goal_cost) << 32 | GNDT_NO_ROW on an accepted goal and all ones
 *                 elsewhere.  next(q) is the low word: the smallest row among the steps that give the least cost, GNDT_NO_ROW on a
 *                 goal that nothing improves.  fl(a + c) is monotone in a, so every relaxation order reaches the same fixed point.  A
 *                 candidate whose sum is not below FLT_MAX is discarded, and with max_cost > 0 one above max_cost (a seed is no
 *                 candidate).  cost is FLT_MAX and next GNDT_NO_ROW where there is no walk and on rows without a slope.
 *   sweeps        a sweep relaxes every slope at least once; one that changes nothing proves the fixed point, and the launches behind
 *                 it return at once, as the clearance rounds do.  max_rounds bounds the sweeps of a call (0 = 1024; above 4096 is
 *                 refused: it bounds the launches of a call, and the device is shared).  If the deepest least-cost walk has L steps,
 *                 L + 1 sweeps always suffice.
 *   counts[8]     0 accepted goals, 1 ignored goals, 2 slopes with a finite cost, 3 the bits of the largest finite cost, 4 converged
 *                 (1 or 0), 5 the sweeps that changed something (diagnostic: not part of the definition), 6 and 7 zero.
 *   not converged counts[4] == 0: the outputs are still usable, and this is all that is promised: every finite cost is >= the fixed
 *                 point's; following `next` from any row with a finite cost reaches an accepted goal without repeating a row; the
 *                 cost recomputed along that chain from the goal backwards is <= the stored one.
 * cost and next have num_nodes entries and every entry is written; either may be NULL, not both.  Order, lifetime and refusals are the
 * clearance call's: the call first finishes what gndt_sync finishes, builds or reuses the map's column index and enqueues its kernels
 * on `hip_stream` (NULL = the handle's stream), not awaited — one launch per sweep, the keys relaxed in place; a map of up to 20 448
 * rows takes every sweep in one launch of one workgroup, its keys in LDS (GNDT_DEBUG_ROUTE_FIELD_ONE_WORKGROUP).  gndt_route_field is
 * synchronous, through the handle's scratch.  G == 0 or a map without rows writes FLT_MAX / GNDT_NO_ROW and counts that are zero but for
 * counts[4] = 1.  The map, h and state are not modified and no cost map is needed.  Work memory (77 bytes a row: per side the first
 * step with its cost and the rest of its steps, the key, the weight, one byte) belongs to the handle and grows with the map.  There
 * is no CPU path.  A sharded map answers from the rows this rank holds.
 * GNDT_ERR_INVALID: a null handle, params or counts, cost and next both NULL, null goals with G > 0, G > 2^20, an unknown check bit,
 * soft_weight or max_cost not finite or negative, max_rounds > 4096, a non-zero reserved word, a device pointer not aligned to 4
 * bytes, no finished build, a stream under hipGraph capture (the call is not recorded). */
typedef struct gndt_route_field_params {
    uint32_t checks;         /* GNDT_WALK_CHECK_* bits */
    uint32_t min_hops;       /* with hops: a slope with fewer hops may not be entered (0: every slope may) */
    uint32_t soft_hops;      /* with hops: a slope with fewer hops costs more to enter (0: none does) */
    float soft_weight;       /* ... by this much per hop it lacks; finite, >= 0 */
    float max_cost;          /* > 0: candidates above it are discarded; 0: none is */
    uint32_t max_rounds;     /* 0 = 1024; above 4096 is refused */
    uint32_t reserved[2];    /* 0 */
} gndt_route_field_params;   /* 32 bytes; zeros = defaults */
/* Device memory in and out: goals_dev [G] (uint32), goal_cost_dev [G] (fp32) or NULL, hops_dev [num_nodes] or NULL, cost_dev (fp32)
 * and next_dev (uint32) [num_nodes], either or NULL; counts_dev [8]. */
int gndt_route_field_device(gndt_handle* h, const gndt_robot* robot, const gndt_route_field_params* params, const uint32_t* goals_dev,
                            uint32_t G, const float* goal_cost_dev, const uint32_t* hops_dev, float* cost_dev, uint32_t* next_dev,
                            uint32_t* counts_dev /* [8] */, void* hip_stream);
/* The same with host memory, through a device scratch the handle owns and grows; returns when the answers are in place. */
int gndt_route_field(gndt_handle* h, const gndt_robot* robot, const gndt_route_field_params* params, const uint32_t* goals_host, uint32_t G,
                     const float* goal_cost_host, const uint32_t* hops_host, float* cost_host, uint32_t* next_host, uint32_t* counts_host);

/* gndt_descend_routes*: K starts become routes by following `next` of a route field of this map as it is now (cost and next, both
 * num_nodes entries: the caller vouches for that as for hops), in the layout gndt_plan_routes* writes: route_rows[k * route_cap ..]
 * start first, goal last, GNDT_NO_ROW behind (a route longer than route_cap writes its first route_cap rows and the caller sees length
 * > route_cap; route_rows may be NULL with route_cap 0), one gndt_route_info per start.  Starts are floats x, y, z at stride 12 or
 * 16; start_mode is the walks' (0 = GNDT_WALK_START_NEAREST_SLOPE).  status:
 *   GNDT_ROUTE_NO_START  the lookup finds no slope (length 0, start_row GNDT_NO_ROW, cost and h_start FLT_MAX);
 *   GNDT_ROUTE_NO_ROUTE  cost[start_row] is FLT_MAX (length 0);
 *   GNDT_ROUTE_LIMIT     the chain needs more than max_steps steps (0 = 65536; above 2^20 is refused: it bounds a lane's loop, and the
 *                        device is shared), or meets a `next` entry that is neither GNDT_NO_ROW nor < num_nodes: no route (length 0,
 *                        every entry GNDT_NO_ROW, cost FLT_MAX); a chain of exactly max_steps steps is FOUND;
 *   GNDT_ROUTE_FOUND     otherwise: length counts start and goal, cost = h_start = cost[start_row].
 * expansions is the steps followed, queue_peak 0.  The kernel reads nothing outside num_nodes entries of the two arrays.  The guard also
 * covers the one pathology of fp32: a step cost below half an ulp of the cost-to-go is absorbed, fl(c + a) == a, and the smallest-row
 * tie-break can then point two slopes at each other.  That needs two means a fraction of a millimetre apart in neighbouring cells at
 * costs of metres; such a chain ends with GNDT_ROUTE_LIMIT instead of spinning.
 * One lane a start; enqueued on `hip_stream` after what gndt_sync finishes and the column index, not awaited; info_dev must be aligned
 * to 16 bytes (two 16-byte stores a record).  gndt_descend_routes is synchronous and takes host memory of any alignment.  K == 0
 * returns GNDT_OK and launches nothing.  There is no CPU path.
 * GNDT_ERR_INVALID: a null handle, params, cost, next or info, null starts with K > 0, K >= 2^31, a stride other than 12 or 16, an
 * unknown start_mode, max_steps > 2^20, a non-zero reserved word, route_rows NULL with route_cap != 0 or the reverse, info_dev not
 * aligned to 16 bytes or another device pointer not to 4, no finished build, a stream under hipGraph capture. */
typedef struct gndt_descend_params {
    int32_t start_mode;      /* 0 = GNDT_WALK_START_NEAREST_SLOPE, or GNDT_WALK_START_NODE */
    uint32_t max_steps;      /* 0 = 65536 */
    uint32_t reserved[6];    /* 0 */
} gndt_descend_params;       /* 32 bytes; zeros = defaults */
int gndt_descend_routes_device(gndt_handle* h, const void* starts_dev, size_t K, size_t stride_bytes, const gndt_descend_params* params,
                               const float* cost_dev, const uint32_t* next_dev, uint32_t* route_rows_dev, uint32_t route_cap,
                               gndt_route_info* info_dev, void* hip_stream);
int gndt_descend_routes(gndt_handle* h, const void* starts_host, size_t K, size_t stride_bytes, const gndt_descend_params* params,
                        const float* cost_host, const uint32_t* next_host, uint32_t* route_rows_host, uint32_t route_cap,
                        gndt_route_info* info_host);

/* ---- scan score derivatives:the score of a pose with its gradient and Hessian, for K poses ------------------------------------
 * What a registration step needs of "scan scoring": score, gradient g (6) and full Hessian H (6 x 6, not the Gauss-Newton part only)
 * of the score with respect to a pose perturbation.  No optimiser here either (grid_ndt_amd/registration.py drives one from Python).
 * Steps 1 to 4 of "scan scoring" hold unchanged — the transform q = fl32(T p), the key, the candidates, min_count, cov_rel, cov_floor,
 * max_d2 and the arithmetic of A, its cofactors c_ij, det, d, u and d2 — with the same gndt_score_params (point_pose is ignored).
 * The derivative is a DEFINITION as the score is (tests restate it in numpy), that of the FROZEN sum: every point keeps the candidate
 * set found at the pose itself and q is treated as a real vector (neither the fp32 rounding nor the cell boundaries are
 * differentiated).  The perturbation xi = (v, w), v, w in R^3, acts on the left, translation first:
 *     q(xi) = Exp([w]x) q + v              (T <- [Exp(w) R | Exp(w) t + v])
 * so at xi = 0: dq/dv_a = e_a, dq/dw_a = e_a x q, d2q/dw_a dw_b = (e_a q_b + e_b q_a) / 2 - delta_ab q, every other second derivative
 * zero.  With B = adj(A) / det, ub = B d and e = exp(-d2 / 2) of a counted candidate, and per point the two sums over its counted
 * candidates in the candidates' order
 *     w3 = sum e ub  (3 values)            M = sum e (ub ub^T - B)  (symmetric, 6 values)
 * a pose's results are sums over the points:
 *     score = sum e                        g_v = - sum w3                       g_w = - sum q x w3
 *     H = sum J^T M J - [0 0; 0 N],        J = [I | -[q]x] (3 x 6),             N_ab = (w3_a q_b + w3_b q_a) / 2 - delta_ab (w3 . q)
 * g is the gradient of the score (which a registration maximises), H its Hessian; a point without a counted candidate adds nothing.
 * grid_ndt_amd/csrc/gndt_score_derivs.hpp states the evaluation order of ub, B, the nine per-point sums and their expansion into the
 * 6 + 21 values.
 * The record: score, d2_sum, matched and terms have EXACTLY the bits gndt_score_poses gives for the same arguments (the same tile of
 * 256 points, the same tree); g in the order of xi; H's upper triangle row-major (H_00 .. H_05, H_11 .. H_15, ... H_55).  All 31 values
 * are reproducible to the bit like the score: no floating-point atomics; pose k of a batch has the bits of a single-pose call, on any
 * stream, at either stride.
 * Order, lifetime, stream rules, the sharded-map remark, the empty cases and every GNDT_ERR_INVALID are gndt_score_poses' (there are no
 * per-point outputs, so point_pose is never refused).  There is no CPU path. */
typedef struct gndt_pose_derivs {
    double score, d2_sum;
    uint64_t matched, terms;
    double g[6];             /* d score / d (v, w)                                               */
    double H[21];            /* upper triangle of d2 score / d xi d xi, row-major                 */
} gndt_pose_derivs;          /* 248 bytes, 8-byte fields only */
/* Device points, poses ([K][12] doubles) and records ([K]). */
int gndt_score_derivs_device(gndt_handle* h, const void* xyz_dev, size_t n, size_t stride_bytes, const double* poses_dev, uint32_t K,
                             const gndt_score_params* params, gndt_pose_derivs* out_dev, void* hip_stream);
/* The same with host memory, through a device scratch the handle owns and grows; synchronous. */
int gndt_score_derivs(gndt_handle* h, const void* xyz_host, size_t n, size_t stride_bytes, const double* poses_host, uint32_t K,
                      const gndt_score_params* params, gndt_pose_derivs* out_host);

/* ---- ray casting: the first map node along each ray of a batch, and how far away it is ----------------------------------------
 * The expected range of a beam from a pose (a particle filter's beam model; gndt_score_poses is the likelihood-field model), line of
 * sight and visibility, synthetic scans and depth images, and "does this return lie in front of the map or behind it" before
 * gndt_clear_rays.  Ray i has an origin o_i and an end point p_i, both fp32 in map coordinates, d = p - o in fp64.
 * A ray is SKIPPED when o_i or p_i has a non-finite coordinate or no key in the codec's range: not an error, counted in stats.skipped.
 * The answer is a DEFINITION (tests restate it in numpy, bit for bit):
 *   - walk: "free-space clearing"'s walk from o_i to the cut point e = o + d * min(1, max_range / |d|) (max_range = 0: no limit; there
 *     is no end_margin): the same columns, |dx| + |dy| steps, tie rule, fp64 crossing parameters and level range per column.
 *   - interval of a column visit, in units of the uncut d: t_in = 0 in the first column, otherwise the crossing parameter of the step
 *     that entered the column; t_out = the crossing parameter of the step that leaves it, in the last column the cut factor
 *     f = min(1, max_range / |d|); t_hi = max(t_in, t_out).
 *   - order of levels: inside a column the levels are visited from the entry level towards the exit level, level 0 skipped.
 *   - GNDT_CAST_VOXEL: a candidate is a row of the column with sz in the level range and count >= min_count (0 = 1; any value >= 1).
 *     Its level the entry level: t_hit = t_in.  Otherwise t_z = the crossing of the z-plane through which the ray enters that level, by
 *     the walk's crossing rule on the z axis (lattice plane k of z_len from the map origin, clamped to [0, 1], 1 for d_z = 0): going up
 *     k is the level's lower plane, going down its upper plane; t_hit = min(max(t_in, t_z), t_hi).  d2 is 0.
 *   - GNDT_CAST_NDT: a candidate also needs statistics: min_count 0 = max(min_points, 3), values below that are refused as in "scan
 *     scoring".  A and its cofactors c_ij are exactly scoring's, from count, cov, cov_rel and cov_floor with the same defaults.  The
 *     point of the line o + t d with the least Mahalanobis distance to the node: w_i = (c_i0 d_x + c_i1 d_y) + c_i2 d_z, g = mean - o,
 *     t_line = ((g_x w_x + g_y w_y) + g_z w_z) / ((d_x w_x + d_y w_y) + d_z w_z), 0 for |d| = 0;
 *     t_hit = min(max(t_line, t_in), t_hi) (a NaN t_line takes t_in); q = o + t_hit d per coordinate in fp64; d2 is the score's d2 of
 *     q - mean with q kept in fp64.  With max_d2 > 0 a candidate whose d2 > max_d2 does not stop the ray (0: no gate).
 *   - selection: range = t_hit * |d| (|d| the fp64 square root the walk uses).  A candidate with range < min_range (fp64 comparison)
 *     does not count: a sensor that sits inside a mapped voxel.  The ray's answer is the first counting candidate in walk order:
 *     columns in walk order, levels in visit order inside a column.
 * Everything is + - x /, sqrt and ceil in fp64, no product fused with a sum, no exp, no floating-point atomics: the same bits in every
 * run, on every stream, at every stride (grid_ndt_amd/csrc/gndt_cast.hpp states the evaluation order).
 * Outputs per ray (each of the three arrays may be NULL, not all of them):
 *     hit       row = the hit row      range = (float)range     d2 = 0 (VOXEL) / (float)d2 (NDT)
 *     miss      row = GNDT_NO_ROW      range = +inf             d2 = +inf
 *     skipped   row = GNDT_NO_ROW      range = NaN              d2 = NaN
 * stats (optional): rays (not skipped), skipped, hits.  Asking for it makes the call wait.
 * origin_stride_bytes is 0, 12 or 16; with 0 every ray starts at the one origin at `origins`.  end_stride_bytes is 12 or 16.
 * Order, lifetime and stream rules are the point queries': the call first finishes what gndt_sync finishes, then builds or reuses the
 * map's column index, then enqueues one kernel on `hip_stream` (NULL = the handle's stream, the rules of gndt_build_device) and does not
 * wait unless `stats` is given.  The map is not modified.  It works on every map that has rows (PARTITION-built ones too: the node
 * table is not needed); a sharded map answers from the rows this rank holds.  There is no CPU path.  n == 0 returns GNDT_OK, launches
 * nothing and zeroes stats.
 * GNDT_ERR_INVALID: null handle, params or out, all three output pointers null, null origins or ends with n > 0, n >= 2^31, a stride
 * other than the above, an unknown mode, a negative or non-finite max_range, min_range, cov_rel, cov_floor or max_d2, a negative
 * min_count, in NDT mode a min_count of 1 or 2 or below the handle's min_points, reserved != 0, no finished build, a stream under
 * hipGraph capture (a cast is not recorded). */
enum { GNDT_CAST_VOXEL = 0, GNDT_CAST_NDT = 1 };
typedef struct gndt_cast_params {
    int32_t mode;            /* GNDT_CAST_VOXEL / GNDT_CAST_NDT                                   */
    int32_t min_count;       /* 0 = 1 (VOXEL) / max(min_points, 3) (NDT)                          */
    float max_range;         /* > 0: walk at most this far from the origin; 0 = no limit          */
    float min_range;         /* >= 0: candidates nearer than this do not count                    */
    float cov_rel;           /* NDT: 0 = 0.01                                                     */
    float cov_floor;         /* NDT: 0 = 1e-6 (m^2)                                               */
    float max_d2;            /* NDT, > 0: candidates beyond this d2 do not stop the ray; 0 = none */
    uint32_t reserved;       /* 0                                                                 */
} gndt_cast_params;          /* 32 bytes */
typedef struct gndt_cast_out {
    uint32_t* row;           /* [n] each, NULL = not written (not all three)                      */
    float* range;
    float* d2;
} gndt_cast_out;
typedef struct gndt_cast_stats {
    uint64_t rays, skipped, hits;
} gndt_cast_stats;
/* Device origins and ends; `out_dev` holds device pointers. */
int gndt_cast_rays_device(gndt_handle* h, const void* origins_dev, size_t origin_stride_bytes, const void* ends_dev, size_t n,
                          size_t end_stride_bytes, const gndt_cast_params* params, const gndt_cast_out* out_dev, gndt_cast_stats* stats,
                          void* hip_stream);
/* The same with host memory, through a device scratch the handle owns and grows; synchronous. */
int gndt_cast_rays(gndt_handle* h, const void* origins_host, size_t origin_stride_bytes, const void* ends_host, size_t n,
                   size_t end_stride_bytes, const gndt_cast_params* params, const gndt_cast_out* out_host, gndt_cast_stats* stats);

/* ---- view gain: the unknown columns a sensor would see from each of K poses ---------------------------------------------------
 * What a next-best-view planner divides by the cost of getting there: gndt_frontiers* gives candidate places, gndt_route_field* the cost
 * to reach them, and this call how much a sensor standing there would learn.  For each of K poses a fan of N rays is walked through
 * the map, and the DISTINCT columns the rays cross before something stops them are counted, split into columns the map has and columns
 * it has not.  It cannot be composed from gndt_cast_rays*: a cast says where a ray stopped, not which columns it crossed, and the rays
 * of a fan cross the same columns many times over near the sensor, so the walk has to mark a set.
 * "Unknown" is GNDT_FRONTIER_OPEN_COLUMN's rule: the map cannot tell a column nobody has looked at from one that was seen empty, so a
 * column that is not in the map is unknown.
 * The answer is a DEFINITION (tests/view_ref.py restates it with sets of columns):
 *   - inputs: K poses, fp64 [K, 12], row-major 3 x 4 [R | t], map <- sensor (the layout gndt_score_poses* takes); N directions (x, y, z)
 *     in the sensor frame, fp32 at dir_stride_bytes 12 or 16, shared by all poses; max_range is the struct's float, widened.
 *   - ray (k, i): origin o = float32(t); end e_a = float32(t_a + max_range * ((R_a0 x + R_a1 y) + R_a2 z)), formed in fp64 in exactly
 *     this order, no product fused with a sum.  The walk is "ray casting"'s in GNDT_CAST_VOXEL mode with its max_range set to
 *     max_range, min_count (0 = 1) and min_range as there: the columns of the walk in order, until a column holds a counting candidate
 *     (the hit) or the cut point's column has been given.  A ray whose origin or end is not finite or has no key is SKIPPED.
 *   - sets: every column the walk of a ray that is not skipped is given, up to and including the column of its hit, is SEEN by pose k.  A
 *     seen column that is not in the map is UNKNOWN, every other seen column is KNOWN.
 *   - the record of pose k (gndt_view_info): rays (not skipped), skipped, hits; unknown and known, the DISTINCT columns of either kind;
 *     status 0, or 1 when the pose's origin is not finite or has no key (every ray is then skipped); steps, the column visits summed over
 *     the rays (the call's work); sum_ux and sum_uy, the sums of c(sx) and c(sy) over the distinct unknown columns, c(s) = s > 0 ? s - 1 : s
 *     the contiguous cell index: sum / unknown is where the unknown lies, the direction to turn the sensor to.
 *   Everything is integer arithmetic over a set: the record does not depend on the order of the directions or of the threads, and
 *   directions given several times change only rays, skipped, hits and steps.
 *   - per ray, optional (row and range, [K, N], each may be NULL): the cast's row and range of that ray, bit for bit what
 *     gndt_cast_rays* in VOXEL mode gives for the same origins and ends (GNDT_NO_ROW and +inf for a miss, GNDT_NO_ROW and NaN skipped).
 * Window and limit: with reach = ceil(max_range / grid_len) + 1, every column a ray of pose k can be given lies within `reach` columns of
 * the origin's column on both axes (the cut point lies within max_range of the origin and the walk stays between the two columns; the
 * one is for the float32 rounding of the cut point).  The two sets of a pose are two bitmaps of W * W bits, W = 2 reach + 1, held in the
 * LDS of the one workgroup that walks the pose's rays.  A call whose bitmaps do not fit the LDS a workgroup can be granted (reach 403
 * on a gfx950 CU's 160 KiB) returns GNDT_ERR_INVALID and names the largest reach it takes: lower max_range or look into a coarser map
 * (gndt_coarsen_device).  There is no global-memory tier for larger windows.
 * Order, lifetime and stream rules are the cast's: the call first finishes what gndt_sync finishes, then builds or reuses the map's
 * column index, then enqueues one kernel on `hip_stream` (NULL = the handle's stream) and waits for nothing.  The map is not modified.
 * There is no CPU path.  K == 0 or N == 0 returns GNDT_OK, launches nothing and writes nothing.
 * GNDT_ERR_INVALID: null handle or params, null poses, directions or info with K > 0 and N > 0, K or N >= 2^31, a stride other than
 * 12 or 16, max_range not finite or not > 0, min_range negative or not finite, a negative min_count, reserved != 0, a window beyond
 * the limit above, (device entry point) poses_dev or info_dev not aligned to 8 bytes or another pointer not to 4, no finished build, a
 * stream under hipGraph capture (the call is not recorded). */
typedef struct gndt_view_params {
    float max_range;         /* > 0, finite: the length of every ray                              */
    float min_range;         /* >= 0: candidates nearer than this do not stop a ray               */
    int32_t min_count;       /* 0 = 1: a node stops a ray from this many points on                */
    uint32_t reserved[5];    /* 0                                                                 */
} gndt_view_params;          /* 32 bytes */
typedef struct gndt_view_info {
    uint32_t rays, skipped, hits;
    uint32_t unknown;        /* distinct seen columns that are not in the map                     */
    uint32_t known;          /* distinct seen columns that are                                    */
    uint32_t status;         /* 0; 1: the origin is not finite or has no key                      */
    uint64_t steps;          /* column visits, summed over the rays                               */
    int64_t sum_ux, sum_uy;  /* sums of the unknown columns' contiguous cell indices              */
} gndt_view_info;            /* 48 bytes */
/* Device poses, directions and outputs (info_dev [K]; row_dev, range_dev [K, N] or NULL). */
int gndt_view_gain_device(gndt_handle* h, const double* poses_dev, size_t K, const void* dirs_dev, size_t n, size_t dir_stride_bytes,
                          const gndt_view_params* params, gndt_view_info* info_dev, uint32_t* row_dev, float* range_dev, void* hip_stream);
/* The same with host memory of any alignment, through a device scratch the handle owns and grows; synchronous. */
int gndt_view_gain(gndt_handle* h, const double* poses_host, size_t K, const void* dirs_host, size_t n, size_t dir_stride_bytes,
                   const gndt_view_params* params, gndt_view_info* info_host, uint32_t* row_host, float* range_host);

/* ---- map pyramids: a coarser map of the same point stream, from the map alone --------------------------------------------------
 * The scan score has a basin of less than a cell (grid_ndt_amd/registration.py); coarse-to-fine registration needs the same cloud at
 * 2x, 4x ... the cell lengths, and a map grown by gndt_update*, cropped or cleared no longer has its points.  It does not need them:
 * for a power-of-two factor f the coarse index of a point is a function of its fine index s (there is no index 0),
 *     parent(s, f) = sign(s) * ceil(|s| / f)
 * (fl32(|d| / (f L)) = fl32(|d| / L) / f exactly, and ceil(x / f) = ceil(ceil(x) / f) for x > 0), and a node's additive statistics
 * (count, Sum v, Sum v v^T about its centre c) move to the parent's centre c' = c - d by
 *     Sum v' = Sum v + n d,        Sum v' v'^T_ab = Sum v v^T_ab + d_a Sum v_b + d_b Sum v_a + n d_a d_b
 * (grid_ndt_amd/csrc/gndt_coarsen.hpp states the evaluation order).  Parents add their children's statistics and counts and take the
 * least first-seen index.  The result is the map a build of the same stream on a handle at f times the lengths gives: keys, counts,
 * first-seen indices, order and labels exactly, statistics up to the rounding of the fp64 sums (whose order is not fixed: the adds are
 * floating-point atomics, as the ATOMIC build's are).
 * gndt_coarsen_device(src, dst, factor_xy, factor_z) resets `dst` (a map it held is gone), gives it `src`'s origin, fills its node table
 * from `src`'s in one pass and finalises it with dst's own demand, slope_interval and min_points: afterwards `dst` is in the state of
 * gndt_reset + gndt_stats_merge_device + gndt_finalize_device, and its stream position is `src`'s — a frame then given to gndt_update*
 * on both handles keeps `dst` the coarse build of the whole stream.  Factors (1, 1) make a clone.
 * `src` is only read: the call first finishes what gndt_sync(src) finishes (a pending build, a deferred emit, a re-run), then leaves its
 * rows, its column index and a current cost map valid and its export bit-identical.  The kernel and the finalisation are enqueued on
 * `hip_stream` (NULL = dst's stream, the rules of gndt_build_device); the call waits for the kernel, as gndt_stats_merge_device does.
 * GNDT_ERR_INVALID, with `dst` unchanged: a null handle, src == dst, handles on different devices, a factor that is not a power of two
 * in 1 .. 1024, dst.grid_len != (float)(factor_xy * src.grid_len) or dst.z_len != (float)(factor_z * src.z_len) (exact fp32), no
 * finished build in `src`, a `src` whose map is not in the additive node table (a PARTITION build; strategy ATOMIC / TILE or a map built
 * by gndt_update* is, as for gndt_remove), a stream under hipGraph capture (a coarsen is not recorded).  A destination table that is
 * too small for the parents reports GNDT_ERR_CAPACITY, as elsewhere.  There is no CPU path. */
int gndt_coarsen_device(gndt_handle* src, gndt_handle* dst, uint32_t factor_xy, uint32_t factor_z, void* hip_stream);

/* ---- map merge: one map folded into another under a rigid transform, from the maps alone ---------------------------------------
 * A registration returns the pose at which a submap, another robot's map or an earlier session's map fits the map being localised
 * against; the merge uses it.  A source node is a Gaussian with a count: it is moved by the pose, the destination node its mean falls
 * into is found, and its moment-matched statistics are added there (the standard NDT map-fusion step).  No point is needed, and a node
 * is kept whole: one that straddles destination cells is not split (DESIGN.md 4.3h says what that costs).
 * The answer is a definition.  Everything is fp64, no product is fused with a sum (grid_ndt_amd/csrc/gndt_merge.hpp states the
 * evaluation order).  For every live source node (count >= 1, count >= min_count) with key k, count n, s1 = Sum v (3 values) and
 * s2 = Sum v v^T (6 values, xx xy xz yy yz zz) about its centre c = axis centre of k at the SOURCE's origin and lengths:
 *   1. source mean          mu_a = s1_a / (double)n,      m_a = c_a + mu_a
 *   2. central scatter      S_ab = s2_ab - s1_a * mu_b
 *   3. moved mean           m'_i = ((R_i0 m_x + R_i1 m_y) + R_i2 m_z) + t_i                       (the shape of scan scoring's step 1)
 *   4. destination key      the codec's key of ((float)m'_x, (float)m'_y, (float)m'_z) at the DESTINATION's origin, grid_len and z_len;
 *                           a non-finite coordinate or a key outside the codec's range: the node does not travel and is counted in
 *                           `skipped` (not an error)
 *   5. rotated scatter      W_ib = (R_i0 S_0b + R_i1 S_1b) + R_i2 S_2b   (S symmetric),   S'_ij = (W_i0 R_j0 + W_i1 R_j1) + W_i2 R_j2, i <= j
 *                           (nothing checks that R is a rotation: any affine map moves the Gaussian this way)
 *   6. destination centre   c' = axis centre of the destination key
 *   7. statistics about c'  u_a = m'_a - c'_a (the fp64 m', not its fp32 rounding),  nu_a = (double)n * u_a:
 *                           out[a] = nu_a,      out[3+ab] = S'_ab + nu_a * u_b
 *   8. into the table       the nine sums add and the count adds; the first-seen index takes the minimum with base + first, base =
 *                           the destination's stream position before the call
 * The destination's stream position becomes base + the source's, whether or not any node travelled.  So a merge under the identity
 * between handles of equal origin and lengths equals gndt_update* of the source's point stream whenever every source node's points
 * share the cell of their mean: the merged part orders after everything the destination held, in the source's own order.  The order
 * of the floating-point adds into one destination node is not fixed (atomics, as in the ATOMIC build and the coarsen).
 * Afterwards `dst` is in the state of gndt_stats_merge_device + gndt_finalize_device: every row re-finalised with dst's demand,
 * slope_interval and min_points, the cost map invalid, the column index rebuilt, device pointers from gndt_export_device and row
 * numbers from gndt_query* invalid; a graph recorded before the merge and replayed after it is reported stale by gndt_sync
 * (GNDT_ERR_CAPACITY, as after a crop or a clear); gndt_update* / gndt_remove* go on afterwards.  The destination may be empty (fresh, or
 * after gndt_reset, with an origin) and may differ from the source in lengths, origin, demand and min_points.
 * `src` is only read: the call first finishes what gndt_sync(src) and gndt_sync(dst) finish, then leaves src's rows, column index and a
 * current cost map valid and its export bit-identical.  `pose` is host memory, row-major 3 x 4 [R | t], dst <- src; NULL = identity.
 * The kernel and the finalisation are enqueued on `hip_stream` (NULL = dst's stream, the rules of gndt_build_device); the call waits for
 * the kernel, as gndt_coarsen_device does, so `stats` (optional) costs nothing extra: source_nodes (live: count >= 1), merged_nodes and
 * merged_points (what travelled), below_min_count, skipped, new_nodes (the destination's node count after minus before).
 * GNDT_ERR_INVALID, with `dst`'s map unchanged and the text on both handles: a null handle, src == dst, handles on different devices, a
 * non-finite pose entry, reserved != 0, a negative min_count, no finished build in `src`, a `src` whose map is not in the additive node
 * table (the rule of gndt_coarsen_device), a `dst` without an origin, a `dst` that holds a PARTITION-built map (the rule of
 * gndt_stats_merge_device: call gndt_reset first), base + the source's stream position > 2^32 - 2, a stream under hipGraph capture (a
 * merge is not recorded).  A destination table that cannot be grown reports GNDT_ERR_CAPACITY or GNDT_ERR_NOMEM, as elsewhere.  A
 * sharded map merges into the rows' owner only if the caller arranges it: the call treats `dst` as one map.  There is no CPU path. */
typedef struct gndt_merge_params {
    int32_t min_count;       /* source nodes with fewer points stay behind; 0 = 1                */
    uint32_t reserved;       /* 0                                                                 */
} gndt_merge_params;         /* 8 bytes */
typedef struct gndt_merge_stats {
    uint64_t source_nodes, merged_nodes, merged_points, below_min_count, skipped, new_nodes;
} gndt_merge_stats;
int gndt_merge_map_device(gndt_handle* dst, gndt_handle* src, const double pose[12], const gndt_merge_params* params,
                          gndt_merge_stats* stats, void* hip_stream);

/* ---- map-to-map scoring: how well one map's nodes fit another map at each of K poses, with derivatives ------------------------
 * Distribution-to-distribution NDT (Stoyanov et al., IJRR 2012): every source node is scored as a Gaussian against the destination
 * Gaussians it lands on; the covariance of the difference is the sum of the two covariances, the source's rotated by the pose.  What
 * a registration of a submap, another robot's map or an earlier session's map needs when the points are gone (a map grown by
 * gndt_update*, cropped, cleared or merged), and per source node the nearest destination Gaussian and its distance: what is in this
 * submap that the map does not explain.
 * Two handles on one device: `dst` is the map scored against, `src` supplies the nodes; both are only read and src == dst is allowed.
 * K poses, each row-major 3 x 4 doubles [R | t], dst <- src (nothing checks that R is a rotation).
 * The score is a DEFINITION (tests restate it in numpy).  A source row COUNTS when it has statistics (GNDT_FLAG_HAS_STATS) and its
 * count >= min_count; the same min_count gates the destination candidates.  For pose k and counted source row r with count c_s, mean
 * m_s (fp32) and scatter S_s (fp32, gndt_cells.cov, un-normalised):
 *   1. q = fl32(T m_s): "scan scoring"'s step 1 to the bit, and its steps 2 and 3 give q's key and the candidates in `dst`
 *      (GNDT_SCORE_DIRECT1 / GNDT_SCORE_DIRECT7, the same candidate order).
 *   2. source covariance, fp64: C_s = S_s * (1 / (c_s - 1)) entry-wise; Sigma = R C_s R^T in the shape of "map merge"'s step 5:
 *      W_ib = (R_i0 C_0b + R_i1 C_1b) + R_i2 C_2b, Sigma_ij = (W_i0 R_j0 + W_i1 R_j1) + W_i2 R_j2, i <= j.
 *   3. per counted candidate with c_d, m_d, S_d: C_d = S_d * (1 / (c_d - 1)), P = Sigma + C_d (six values);
 *      eps = max(cov_rel * (((P_xx + P_yy) + P_zz) / 3), cov_floor), A = P + eps I; cofactors, det, d = q - m_d, u and d2 exactly in
 *      "scan scoring"'s order; term = exp(-d2 / 2); with max_d2 > 0 a candidate whose d2 > max_d2 does not count.  With cov_rel = 0.01
 *      the condition number of A is at most 301; with Sigma = 0 the term has scan scoring's bits.
 *   4. per pose: score, d2_sum, terms, and matched = counted source rows with at least one term (a gndt_pose_score).
 *   5. per source row, optional, for the one pose `point_pose` of the parameters (read as the node pose): the least d2 as fp32 and
 *      that destination row; +inf / GNDT_NO_ROW when the row has no term (equal d2: the lower row); NaN / GNDT_NO_ROW for a source row
 *      that does not count.
 * Derivatives are those of the FROZEN sum, as in "scan score derivatives": the candidate set found at the pose is kept, eps is kept, q
 * is a real vector.  The left perturbation xi = (v, w) acts on both moments:
 *     q(xi) = Exp([w]x) q + v,        A(xi) = Exp([w]x) Sigma Exp([w]x)^T + C_d + eps I.
 * With G_a = [e_a]x, B = A^-1, ub = B d, e = exp(-d2 / 2) and a = 0 .. 5: d_a = e_a (translations), e_a x q (rotations); A_a = 0
 * (translations), G_a Sigma + Sigma G_a^T (rotations); r_a = d_a - A_a ub; phi_a = 2 ub . d_a - ub^T A_a ub;
 * phi_ab = 2 r_a^T B r_b, plus for two rotations 2 ub . (G_ab q) - ub^T A_ab ub with G_ab = (G_a G_b + G_b G_a) / 2 (so
 * G_ab q = (e_a q_b + e_b q_a) / 2 - delta_ab q) and A_ab = G_a Sigma G_b^T + G_b Sigma G_a^T + G_ab Sigma + Sigma G_ab^T; then
 *     g_a = sum over the pairs of -e phi_a / 2,        H_ab = sum over the pairs of e (phi_a phi_b / 4 - phi_ab / 2).
 * grid_ndt_amd/csrc/gndt_score_maps.hpp states the evaluation order of Sigma, P, r_a, phi_a, phi_ab and the 6 + 21 values.  The record
 * is gndt_pose_derivs; its first four fields are EXACTLY the bits the score-only call gives.
 * Parameters are gndt_score_params with "scan scoring"'s defaults, except min_count: 0 = max(dst's min_points, src's min_points, 3),
 * and a value of 1 or 2 or below either handle's min_points is refused.
 * Reproducible to the bit by the score's rules: one thread per (source row, pose), the rows in row order, every row, counted or not,
 * keeping its slot (the tile of row r is r / 256), the score's fixed tree per tile, a pose's tiles in tile order, no floating-point
 * atomics; pose k of a batch has the bits of a single-pose call, on any stream.
 * Order and lifetime are gndt_score_poses_device's: the call first finishes what gndt_sync finishes on both handles, builds or reuses
 * dst's column index, enqueues on `hip_stream` (NULL = dst's stream) and does not wait; later work on either handle is ordered behind
 * it.  It works on every map that has rows (PARTITION-built ones too); a sharded map answers from the rows this rank holds.  There is
 * no CPU path and no host-memory variant: both maps live on the device.  No source rows with K > 0 writes K zeroed records; K == 0
 * launches nothing.
 * GNDT_ERR_INVALID: a null handle or params, handles on different devices, null poses or out with K > 0, K > 65535, an unknown
 * neighbourhood, point_pose >= K when a per-node output is asked for, the min_count rule above, a negative or non-finite cov_rel,
 * cov_floor or max_d2, no finished build in either handle, a stream under hipGraph capture (a score is not recorded; the capture
 * goes on). */
/* Device poses ([K][12] doubles), records ([K]) and per-node outputs ([src's rows] each, either may be NULL). */
int gndt_score_maps_device(gndt_handle* dst, gndt_handle* src, const double* poses_dev, uint32_t K, const gndt_score_params* params,
                           gndt_pose_score* out_dev, float* node_d2_dev, uint32_t* node_row_dev, void* hip_stream);
int gndt_score_maps_derivs_device(gndt_handle* dst, gndt_handle* src, const double* poses_dev, uint32_t K, const gndt_score_params* params,
                                  gndt_pose_derivs* out_dev, void* hip_stream);

/* ---- input side ---------------------------------------------------------
 * Where x, y, z sit inside one raw point record: sensor_msgs::PointCloud2 fields / point_step, the records of a
 * binary .pcd, or pcl::PointXYZ itself (step 16, offsets 0, 4, 8).  Offsets are multiples of 4. */
typedef struct gndt_point_layout {
    uint32_t point_step, offset_x, offset_y, offset_z;
} gndt_point_layout;

/* A .pcd file as pcl::io::loadPCDFile reads it (src/publisher.cpp:19): header + payload.  `DATA binary` payloads are
 * returned as they are in the file (binary_compressed ones after LZF decompression and re-interleaving) (`layout` says where x, y, z are), `DATA ascii` as packed xyz.  Host-only. */
typedef struct gndt_pcd {
    uint64_t num_points;
    gndt_point_layout layout;
    int32_t data_kind;          /* 0 ascii (converted to packed xyz), 1 binary, 2 binary_compressed (decompressed, records rebuilt) */
    int32_t reserved;
    void* data;                 /* num_points * layout.point_step bytes, released by gndt_pcd_free */
} gndt_pcd;
int gndt_pcd_read(const char* path, gndt_pcd* out, char err[256]);
void gndt_pcd_free(gndt_pcd* pcd);

/* Raw records on the device -> packed fp32 xyz on the device ([n][3], caller-allocated), rows with a non-finite
 * coordinate dropped, order kept: pcl::fromPCLPointCloud2 (receiver.cpp:140-143) + pcl::removeNaNFromPointCloud
 * (publisher.cpp:24-26).  *n_valid (host) = rows written; the call returns when it is known. */
int gndt_pack_points_device(gndt_handle* h, const void* raw_dev, size_t n, const gndt_point_layout* layout,
                            float* xyz_out_dev, uint64_t* n_valid, void* hip_stream);
/* chatterCallback in one call (receiver.cpp:137-160): raw host records -> device, NaN strip, origin := the first
 * valid point (receiver.cpp:145), build of the rest.  Returns like gndt_build. */
int gndt_build_cloud(gndt_handle* h, const void* raw_host, size_t n, const gndt_point_layout* layout);

/* ---- host key codec (consumers call transMortonXYZ on pos/goal: map2D.h:1071,1293; GlobalPlan.h:56) */
/* `transMortonXYZ` (map2D.h:950-976): quadrant letter, 1-based indices, signed z level and the
 * map key string (letter + decimal Morton, <= 12 chars + NUL). */
int gndt_trans_morton_xyz(const float origin[3], float grid_len, float z_len, const float p[3],
                          char* quadrant, int32_t* nx, int32_t* ny, int32_t* sz, char key_out[16]);
/* `countMorton` (Stopwatch.h:116-147), decimal string of the 32-bit interleave. */
int gndt_count_morton(int32_t a, int32_t b, char out[16]);
/* `mortonToXY` (Stopwatch.h:171-189). */
int gndt_morton_to_xy(int32_t morton, int32_t* a, int32_t* b);
/* Packed 64-bit node key used by gndt_stats: bits 63..43 sx+2^20, 42..22 sy+2^20, 21..0 sz+2^21. */
uint64_t gndt_pack_key(int32_t sx, int32_t sy, int32_t sz);
void gndt_unpack_key(uint64_t key, int32_t* sx, int32_t* sy, int32_t* sz);

/* ---- phase timing (bench.py / profiling) ------------------------------------------------------ */
/* With profiling on, build/accumulate/finalize record HIP events on the launch stream around each
 * phase; gndt_get_phase_times waits for them and returns milliseconds (-1 = phase did not run).
 * Phase names depend on the strategy the last build used (gndt_last_strategy):
 *   ATOMIC:    [0] clear  [1] accumulate  [2] columns  [3] rows  [4] bitmap_scan  [5] rank
 *              [6] column_scan  [7] dest  [8] emit   (bitmap_scan = prefix of the per-word column weights; rank and
 *              column_scan are empty since the ordering needs neither: kept so that phase indices stay put)
 *   PARTITION_EXACT: [0] clear  [1] hist  [2] offsets  [3] scatter  [4] bucket_build  [5] bitmap_scan
 *              [6] rank  [7] column_scan  [8] dest  [9] emit
 *   PARTITION (two-level): as PARTITION_EXACT with [1] level1  [2] (unused)  [3] level2 */
#define GNDT_NUM_PHASES 10
/* enable: 0 off, 1 events around every phase, 2 only around the dominant phase of the strategy in use
 * (bucket_build / accumulate): two events per build instead of eleven. */
int gndt_set_profiling(gndt_handle* h, int enable);
int gndt_get_phase_times(gndt_handle* h, double ms_out[GNDT_NUM_PHASES]);
/* GNDT_STRATEGY_ATOMIC, _PARTITION (two-level, hashed buckets), _PARTITION_BLOCKED (two-level, spatial blocks as buckets), _PARTITION_ONE_LEVEL,
 * _PARTITION_EXACT or _TILE: what the last build actually ran (AUTO resolves, and PARTITION falls back to ATOMIC when a bucket does not
 * fit in LDS). */
/* The measurement AUTO bases that choice on, for logs and tuning: `tiles` tiles of 2048 consecutive points spread over the
 * cloud; *points_per_partial = points looked at / distinct nodes met per tile.  Waits for the result. */
int gndt_locality_sample(gndt_handle* h, const void* xyz_dev, size_t n, size_t stride_bytes, uint32_t tiles, double* points_per_partial,
                         void* hip_stream);
int gndt_last_strategy(const gndt_handle* h);
/* Diagnostic (not for timed runs): after gndt_debug_enable_stamps(1) the bucket kernel
 * stamps the shader clock at its phase boundaries; this returns the mean cycles per bucket of
 * [0] clear [1] accumulate [2] columns [3] labels [4] order [5] emit, then the accumulate phase split into
 * [6] load wait [7] classify [8] scan+scatter [9] reduce (first chunk), and the bucket count. */
int gndt_debug_bucket_phases(gndt_handle* h, double cycles_out[10], uint32_t* buckets_out);
/* How many times this handle has re-run a PARTITION build because an LDS table, a partition region or the staging rows were
 * too small (each is a whole extra build).  A build is launched without waiting and its flags are only looked at by the call
 * that needs the result: a benchmark that enqueues builds back to back should check that this does not move. */
int gndt_debug_retry_count(gndt_handle* h, uint64_t* retries);
/* Switch the stamps on or off for the builds that follow (process-wide). */
int gndt_debug_enable_stamps(int on);
/* The library reads NO environment variable: what used to be GNDT_VERBOSE / GNDT_TILE_RATIO / GNDT_COST_WG (rounds 1-5) is set
 * here, process-wide, for the calls that follow.  Returns GNDT_ERR_INVALID for an unknown option or a value out of range.
 *   GNDT_DEBUG_VERBOSE            value != 0: one stderr line per resolved partition build (fullest region, flags, re-runs, second
 *                                 pass, node sketch) and per locality sample                                        default 0
 *   GNDT_DEBUG_TILE_RATIO         points per partial from which strategy AUTO takes TILE (tools/calibrate_tile.py sweeps it);
 *                                 value >= 1                                                                        default 48
 *   GNDT_DEBUG_COST_ONE_WORKGROUP value == 0: gndt_compute_cost launches every layer on its own, the one-workgroup kernel that walks
 *                                 the narrow layers is not used (tests run the flood both ways)                     default 1
 *   GNDT_DEBUG_QUERY_ILP          independent queries one thread of gndt_query* works on at once: 1, 2 or 4       default 1
 *   GNDT_DEBUG_CLEAR_EXTENT       value == 1: gndt_clear_rays* read the rows of a walked column only if the column's level extent
 *                                 meets the ray's level range (tools/measure_clear.py A/Bs the two; same results)  default 0
 *   GNDT_DEBUG_PLAN_LDS_ENTRIES   entries of a planning query's open queue held in LDS, a multiple of 64 in 64 .. 1024; what does
 *                                 not fit spills to the query's scratch (tests cap it so that a small map spills)  default 1024
 *   GNDT_DEBUG_POISON_BYTE        the -DGNDT_POISON build only (a regular build answers GNDT_ERR_INVALID): the byte every device and
 *                                 pinned host allocation that follows is filled with before it is handed out, an integer in
 *                                 0 .. 255.  0xA5 breaks indices, counts and flags; 0x7F also breaks floating-point reads
 *                                 (3.40e38 as a float) and is none of the library's sentinels (tests run both)      default 0xA5
 *   GNDT_DEBUG_CLEARANCE_ONE_WORKGROUP value == 0: gndt_clearance* launch every hop on its own, the one-workgroup kernel that holds a
 *                                 small map's keys in LDS is not used (tests run the field both ways)               default 1
 *   GNDT_DEBUG_OBSTACLE_TALLY     value != 0: the marking pass of gndt_obstacle_field* keeps the tallies gndt_debug_obstacle_marks
 *                                 reads (a few atomics a wavefront)                                                    default 0
 *   GNDT_DEBUG_WALK_STEP_TABLE    value == 1: gndt_walk_paths* first make a per-side steps table of the whole map (the clearance
 *                                 field's first pass) and read every step of every walk from it; 0: a walk finds its steps itself,
 *                                 gates included (tests run the walks both ways); 2: the table for a map of up to 2048 rows per
 *                                 waypoint of a path (num_nodes <= 2048 T), where it was measured faster          default 2
 *   GNDT_DEBUG_BLOCKED_MIN_POINTS points from which a build may take BLOCKED buckets (GNDT_STRATEGY_PARTITION_BLOCKED), an integer in
 *                                 65 536 .. 1 048 576.  A tuning choice of the host, not a limit of the kernel: tests lower it and ask
 *                                 for GNDT_STRATEGY_PARTITION_TWO_LEVEL to reach the blocked kernel with small clouds  default 1 048 576
 *   GNDT_DEBUG_COLUMN_DEST        value == 0: a BLOCKED build that orders and emits in two kernels finds its rows' places from the staged
 *                                 nodes (ord_cf / ord_idx, as every other build does) instead of from the bucket kernel's column
 *                                 table; same map either way (tests build both and compare)                          default 1
 *   GNDT_DEBUG_PLACE_EMIT_WORDS   PARTITION builds of clouds with up to this many column-order bitmap words (32 points each) order and
 *                                 emit in ONE kernel, larger ones in two; an integer in 0 .. 2^24, 0 = always two kernels (tests send
 *                                 small clouds through the two kernels of a production-size build)                   default 16 384
 *   GNDT_DEBUG_ROUTE_FIELD_ONE_WORKGROUP value == 0: gndt_route_field* launch every sweep on its own, the one-workgroup kernel that holds a
 *                                 small map's keys in LDS is not used (tests run the field both ways)               default 1
 *   GNDT_DEBUG_VIEW_THREADS       threads of a gndt_view_gain* workgroup at most, a multiple of 64 in 64 .. 1024 (a fan of fewer rays
 *                                 takes fewer); the records do not depend on it (tests run several)                 default 1024
 *   GNDT_DEBUG_PATCH_LDS          value == 0: the moment pass of gndt_patches* sends every wavefront's sums to memory itself instead of
 *                                 combining a workgroup's waves in LDS first (tools/measure_patches.py A/Bs the two; the same
 *                                 integer fields, plane fields equal to fp64 rounding)                              default 1 */
#define GNDT_DEBUG_VERBOSE 1
#define GNDT_DEBUG_TILE_RATIO 2
#define GNDT_DEBUG_COST_ONE_WORKGROUP 3
#define GNDT_DEBUG_QUERY_ILP 4
#define GNDT_DEBUG_CLEAR_EXTENT 5
#define GNDT_DEBUG_PLAN_LDS_ENTRIES 6
#define GNDT_DEBUG_POISON_BYTE 7
#define GNDT_DEBUG_CLEARANCE_ONE_WORKGROUP 8
#define GNDT_DEBUG_WALK_STEP_TABLE 9
#define GNDT_DEBUG_BLOCKED_MIN_POINTS 10
#define GNDT_DEBUG_COLUMN_DEST 11
#define GNDT_DEBUG_PLACE_EMIT_WORDS 12
#define GNDT_DEBUG_OBSTACLE_TALLY 13
#define GNDT_DEBUG_ROUTE_FIELD_ONE_WORKGROUP 14
#define GNDT_DEBUG_VIEW_THREADS 15
#define GNDT_DEBUG_PATCH_LDS 16
int gndt_debug_set_option(int option, double value);
/* The -DGNDT_POISON build only (a regular build returns GNDT_ERR_INVALID and writes nothing): the bytes of device memory and of pinned
 * host memory this process has filled with the poison byte so far.  Tests prove with it that a poisoned run was one. */
int gndt_debug_poisoned_bytes(uint64_t* device_bytes, uint64_t* host_bytes);
/* The bucket kernel finds a node through a 21-bit fingerprint of its key and confirms it with the key itself; a bucket in
 * which a fingerprint named the wrong node (~1 in 10^4) is accumulated a second time with every probe confirmed.  Tests narrow
 * the fingerprint (0 .. 21 bits, process-wide, for the builds that follow) so that this happens in every bucket;
 * gndt_debug_fp_clashes: buckets of the last resolved PARTITION build that took the second pass. */
int gndt_debug_set_fp_bits(int bits);
int gndt_debug_fp_clashes(gndt_handle* h, uint64_t* buckets);
/* Buckets of the last resolved PARTITION build whose 512-slot LDS table overflowed and that were done again by the bucket kernel's
 * second pass (1024-slot tables, those buckets only) instead of the whole build being re-run (gndt_debug_retry_count). */
int gndt_debug_second_pass_buckets(gndt_handle* h, uint64_t* buckets);
/* The block layout the handle holds for BLOCKED buckets (GNDT_STRATEGY_PARTITION_BLOCKED), as the last resolved build decided it; waits
 * for nothing and changes nothing.  out[0] = state (0: not looked at yet, 1: the next cloud of this size takes blocked buckets, -1: it
 * does not), out[1..3] = smallest contiguous index of the box on x, y, z (c = s > 0 ? s - 1 : s of a signed index s; the block of margin
 * and the level padding included), out[4..6] = log2 of a block's extent in columns along x, columns along y and levels (they sum to 9),
 * out[7..8] = blocks along x and y, out[9] = buckets (out[7] * out[8]).  out[1..9] mean something only while out[0] == 1. */
int gndt_debug_block_layout(gndt_handle* h, int32_t out[10]);
/* What the marking pass of the handle's last gndt_obstacle_field* call did (tools/measure_obstacle.py); waits for the handle's last
 * stream.  out[0] = columns of the admitted windows (one thread each), out[1] = rows of the worklist (every row of a column in reach),
 * out[2] = index probes that found a column, out[3] = columns put on the worklist (one atomic pair each), out[4] = 64-bit minima sent for
 * covered slopes (a thread that reads a cover word already at or below its own sends none).  out[2..4] are kept only while
 * GNDT_DEBUG_OBSTACLE_TALLY is set.  Zeros before the first call. */
int gndt_debug_obstacle_marks(gndt_handle* h, uint64_t out[5]);
/* Tests of the sharded builds: the next allocation at `site` on this handle fails once, as if the device were out of memory —
 * 1: the receive buffer of gndt_build_owned_device's exchange, 2: its column-pair buffers, 3: the buffers of
 * gndt_gather_owned_map_device, 4: the fixed-size message buffers of a communicator's first owned build (0: none).  Every rank
 * of the build must then return — the failing one GNDT_ERR_NOMEM, the others GNDT_ERR_PEER — instead of waiting in a collective. */
int gndt_debug_fail_next_alloc(gndt_handle* h, int site);

/* Library / device information for logs: returns 0 and fills what it can. */
int gndt_device_info(int32_t device_id, char name_out[128], int32_t* compute_units, uint64_t* hbm_bytes);

#ifdef __cplusplus
}
#endif
#endif /* GNDT_H */
