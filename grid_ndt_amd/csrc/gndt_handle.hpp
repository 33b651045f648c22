// gndt_handle.hpp — the handle behind include/gndt.h and the host-side helpers its translation units share.
// Host code only owns memory, orders launches on a HIP stream and maps errors to status codes; the entry points are
// grouped by what they drive:
//   gndt_api_core.hip   handle life cycle, origin, sync / export, profiling, shared buffers
//   gndt_api_table.hip  strategy ATOMIC: the HBM node table (accumulate, update, finalize, statistics export / merge)
//   gndt_api_build.hip  strategy PARTITION: launch, pending-build resolution, gndt_build*
//   gndt_api_dist.hip   one global map from a sharded cloud (shard statistics, exchange, finalize from statistics)
//   gndt_api_cost.hip   cost-map flood over the finished grid
//   gndt_api_query.hip  batched point queries against the finished grid
//   gndt_api_crop.hip   region crop: the columns outside (or inside) a box leave the map
//   gndt_api_clear.hip  free-space clearing: nodes that sensor rays pass through leave the map
//   gndt_api_score.hip  scan scoring and its derivatives
//   gndt_api_plan.hip   route planning: A* routes to the flood's goal for a batch of starts
//   gndt_api_frontier.hip  frontier extraction: the slopes where the map ends, clustered
//   gndt_api_segment.hip   scan segmentation: the points of a scan the map does not explain, clustered
//   gndt_api_patch.hip     surface patches: the map's nodes grown into planes over their normals and means
//   gndt_api_clearance.hip  clearance field: per slope the steps to the nearest barrier, and where it is
//   gndt_api_route_field.hip route field: per slope the least cost to a set of goals and the step to take, routes by descent
//   gndt_api_obstacle.hip   obstacle field: per slope the steps to the nearest slope a box of the caller's list stands on
//   gndt_api_view.hip       view gain: per pose the distinct unknown and known columns a fan of rays crosses (the handle owns nothing for it)
//   gndt_api_walk.hip       path walks: candidate polylines driven over the map's slopes under the flood's gates
//   gndt_api_coarsen.hip  map pyramids: a coarser map of the same stream from the node table
//   gndt_api_merge.hip  map merge: one map's node table folded into another's under a rigid transform
//   gndt_api_io.hip     input side (record unpack + NaN strip, gndt_build_cloud)
// The consumers' per-call scratch areas are carved by gndt_scratch.hpp's Carver from the layout structs next to their kernels
// (carve_scratch below); their host-pointer entry points stage their arrays through stage_in / stage_out.
// There is NO CPU fallback: without a HIP device every compute entry point fails with GNDT_ERR_NO_DEVICE.
#pragma once
#include <algorithm>
#include <array>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "gndt.h"

namespace gndt { struct QueryView; }   // gndt_query.hpp

// Debug build (-DGNDT_POISON, grid_ndt_amd/csrc/libgndt_poison.so): every device allocation and every pinned host allocation is
// filled with one byte before it is handed out.  A fresh process gets zeroed pages from hipMalloc and hipHostMalloc, which hides
// reads of memory the library never initialised; a process that has freed and reallocated for a while does not (tools/fuzz_graph.py
// found two such reads only after ~100 handles).  The byte is gndt_debug_set_option(GNDT_DEBUG_POISON_BYTE, .): 0xA5 by default (as a
// uint32 2 779 096 485: breaks indices, counts and flags, but reads as the float -2.87e-16, which a sum that starts from it survives),
// 0x7F for the floating-point reads (3.40e38 as a float, 1.38e306 as a double, 2 139 062 143 as an int; none of the library's
// sentinels).  gndt_debug_poisoned_bytes counts what has been filled.  tests/test_gpu_poisoned.py runs the consumers' tests under both.
#ifdef GNDT_POISON
namespace gndt_host {
inline std::atomic<int> g_poison_byte{0xA5};
inline std::atomic<unsigned long long> g_poisoned_device{0}, g_poisoned_host{0};
inline hipError_t poison_malloc(void** p, size_t bytes) {
    const hipError_t e = (hipMalloc)(p, bytes);
    if (e == hipSuccess && bytes) { (void)hipMemset(*p, g_poison_byte.load(), bytes); (void)hipDeviceSynchronize(); g_poisoned_device += bytes; }
    return e;
}
inline hipError_t poison_host_malloc(void** p, size_t bytes) {
    const hipError_t e = (hipHostMalloc)(p, bytes);
    if (e == hipSuccess && bytes) { std::memset(*p, g_poison_byte.load(), bytes); g_poisoned_host += bytes; }
    return e;
}
}  // namespace gndt_host
#define hipMalloc(p, bytes) gndt_host::poison_malloc((void**)(p), (bytes))
#define hipHostMalloc(p, bytes) gndt_host::poison_host_malloc((void**)(p), (bytes))
#endif
#include "gndt_kernels.hpp"
#include "gndt_partition.hpp"
#include "gndt_cost.hpp"
#include "gndt_scratch.hpp"

using namespace gndt;   // host translation units of libgndt only: nothing else includes this header

struct gndt_handle {
    gndt_params P{};
    float origin[3] = {0, 0, 0};
    bool origin_set = false;
    int device = 0;
    hipStream_t own_stream = nullptr;
    bool stream_borrowed = false;      // gndt_warmup's temporary handles run on the stream of the handle they warm up (never destroyed by them)
    hipStream_t last_stream = nullptr;
    hipEvent_t xstream_ev = nullptr;   // orders work on a new stream behind what the previous one still runs (use_stream)
    // A build recorded into a hipGraph keeps the device pointers of its day.  Once a stream of this handle has been seen under
    // capture, buffers that are outgrown are not freed but RETIRED (kept until gndt_destroy): a replay of the old graph then writes
    // into memory that is still the handle's — its result is reported as stale (realloc_gen), but it cannot fault or corrupt
    // someone else's allocation (round 5, tools/fuzz_graph.py: "write access to a read-only page" 60 s into the first seed that
    // put eager table-family builds between the replays).
    bool ever_captured = false;  std::vector<void*> retired;
    uint32_t table_gen = 0;            // allocations of the node table so far (Counters::table_gen on the device)
    // Calls recorded into a hipGraph: each gets an id that the last kernel of the recorded work stores into the host's mirror of the
    // flags (PartCounters::capture_id) — so the call that next waits for the stream can tell that what it finds on the device is a
    // REPLAY (the host saw none of it), of which recorded call, and whether that call's buffers are still the handle's.
    struct CaptureRec { uint32_t id = 0; uint64_t realloc_gen = 0; uint32_t table_gen = 0; bool partition = false; bool two_level = false, one_level = false; };
    CaptureRec captures[32];           // (a ring: a handle with more than 32 live graphs reports the oldest ones as stale)
    uint32_t capture_seq = 0, cur_capture_id = 0;
    uint32_t replay_seen = 0;          // the capture id the last gndt_sync found in the mirror (0: the host's own call)
    uint64_t realloc_gen = 0;          // bumped whenever a device buffer of this handle is freed / reallocated: a build recorded into a hipGraph
                                       //   before that writes through the old pointers when replayed — noticed and reported (Pending::captured_gen)
    bool capturing = false;            // the stream of the call in progress is under hipGraph capture (use_stream): nothing may allocate,
                                       //   free or wait — such a call would not only fail, it INVALIDATES the capture (GNDT_NO_CAPTURE)

    // A device area that a consumer owns, grows on demand (grow_scratch) and never records into a graph; freed by free_scratch
    struct Scratch { void* p = nullptr;  uint64_t bytes = 0; };

    // node table
    uint32_t cap = 0;  // slots, power of two
    uint64_t* keys = nullptr;
    NodeAcc* acc = nullptr;
    uint64_t* col_keys = nullptr;
    uint32_t* col_first = nullptr;
    SlotAux* aux = nullptr;
    // node list + ordering buffers (cap entries each)
    uint32_t* node_slot = nullptr;
    uint32_t* col_slot_of_node = nullptr;
    uint32_t* col_cnt = nullptr;
    uint32_t* col_head = nullptr;
    uint32_t* node_next = nullptr;
    void* ninfo = nullptr;          // gndt::NodeInfo[cap]: per node {first-seen, z level, mean z, flags} for the column walks (gndt_table.hpp)
    // incremental updates: slot -> node index, touch marks, the lists of touched nodes / columns
    uint32_t *index_of_slot = nullptr, *touch_epoch = nullptr, *col_epoch = nullptr, *touched = nullptr, *touched_cols = nullptr;
    bool incr_ok = false;       // the persistent staging rows / order of the table path describe the current map

    Counters* d_cnt = nullptr;
    Counters* h_cnt = nullptr;  // pinned

    // results
    uint64_t out_cap = 0;
    OutView out{};
    uint64_t res_nodes = 0, res_columns = 0, res_slopes = 0;
    bool results_valid = false;

    // stats export buffers
    uint64_t st_cap = 0;
    uint64_t* st_key = nullptr;
    double* st_sums = nullptr;
    uint32_t* st_count = nullptr;
    uint32_t* st_first = nullptr;

    // staging for host input
    void* stage = nullptr;
    size_t stage_bytes = 0;
    void* exp_host = nullptr;  uint64_t exp_rows = 0;   // gndt_export_host: pinned mirror of the result arrays
    void* bounce[2] = {nullptr, nullptr};          // pinned bounce buffers for large pageable inputs (stage_host_input)
    hipEvent_t bounce_ev[2] = {nullptr, nullptr};
    // gndt_build_cloud: packed xyz of the unpacked, NaN-stripped cloud; pinned word for the valid count
    float* packed = nullptr;
    uint64_t packed_cap = 0;
    uint32_t* d_nvalid = nullptr;
    uint32_t* h_nvalid = nullptr;

    uint64_t stream_pos = 0;    // points accumulated since the last reset (host mirror of the device-side first_idx base)
    uint64_t nodes_bound = 0;   // host-side upper bound of the nodes in the table (no sync needed to size buffers)
    bool table_dirty = false;   // table holds nodes
    // small maps (k_small_finalize, gndt_table.hpp): the node count the last resolved table-path build had; cleared when the
    // one-workgroup finalisation met a map that was not small; whether its last launch was recorded under hipGraph capture
    uint32_t table_nodes_seen = 0;  bool small_ok = true;  bool small_captured = false;  bool small_used = false;
    // deferred-emit mode (gndt_set_deferred_emit): gndt_update* relabels the touched columns and stops; the rows in the reference's
    // dense order are produced by the next call that READS the map.  emit_pending: frames have been added since the rows were emitted
    bool defer_emit = false;  bool emit_pending = false;  uint64_t pending_words = 0;
    bool deferred_captured = false;    // the last deferred frame was recorded under hipGraph capture: replays add frames the host does not see

    // strategy PARTITION buffers (gndt_partition.hpp)
    struct Part {
        uint64_t rec_cap = 0;      float4* recs = nullptr;
        // two-level partition: level-1 regions, cursors of both levels, record ranges of the fine buckets
        uint64_t rec1_cap = 0;     float4* recs1 = nullptr;
        uint64_t cur_cap = 0;      uint32_t *cursors = nullptr, *range_lo = nullptr, *range_hi = nullptr, *range_cap = nullptr;
        // (range_hi doubles as the bucket kernel's retry list: buckets whose 512-slot table overflowed, done again with 1024 slots)
        bool retry_pass = true;    // launch that second pass behind the bucket kernel (first builds, captured builds, clouds that needed it)
        uint32_t retry_seen = 0;   // buckets the last resolved build sent through it
        int two_level_failures = 0;   // builds whose regions overflowed although sized from the sample
        bool one_level_ok = true;  // cleared when a bucket of the one-level tile partition (small clouds) overflowed its fixed room
        bool two_level_ok = true;  // cleared when the regions a cloud needs are too large: exact path from then on
        double fill1_ratio = 0.0;   // fullest level-1 region / mean seen on this handle (0 = unknown)
        uint64_t hist_cap = 0;     uint32_t* hist = nullptr;
        uint32_t bucket_cap = 0;   uint32_t* totals = nullptr; uint32_t* bucket_base = nullptr;
        uint64_t stage_cap = 0;    StageRow* stage = nullptr;    // stage_cap: staging rows the order arrays below can hold ...
        uint64_t stage_rows_cap = 0;                             // ... and how many StageRow records `stage` holds (the table / TILE / statistics paths;
                                                                 //     the PARTITION strategies stage RawNode records in `raw` instead and never grow it)
        RawNode* raw = nullptr;  uint64_t raw_cap = 0;          // k_bucket_direct's staging rows (dense, a column's rows adjacent)
        uint32_t *ord_cf = nullptr, *ord_idx = nullptr, *inv = nullptr;
        uint32_t* row_of = nullptr;        // [stage_cap] row of every staged node (table path: the incremental finalisation emits in place)
        uint32_t* row_ncol = nullptr; uint64_t row_ncol_cap = 0;     // per result row: its column's node count on the column's first row, else 0
        // column order (gndt_partition.hpp ColumnOrder): per bitmap word, and per point index for ncol_at
        uint64_t words_init = 0;   // bitmap / word_weight words the table path's column order has initialised
        uint64_t word_cap = 0;     uint32_t *bitmap = nullptr, *word_weight = nullptr, *word_base = nullptr, *bsum_words = nullptr,
                                            *ncol_at = nullptr;
        PartCounters* d_pc = nullptr;
        // Round 6: what level 1 needs zeroed BEFORE it starts (the cursors, the partition counters) exists twice; the level-1 kernel of a
        // build zeroes the set the NEXT build takes (and this build's bitmap / Counters, which nothing reads before the bucket kernel),
        // so that an eager build is not preceded by a k_part_clear launch (~4.5 us of a 49 us frame).  Not for handles that ever
        // recorded a hipGraph: a replay uses the set it was recorded with, unseen by the host.
        uint32_t* cursors_alt = nullptr;
        PartCounters* d_pc_alt = nullptr;
        bool alt_clean = false;         // cursors_alt / d_pc_alt are zero (a level-1 kernel launched on this stream left them so)
        PartCounters* h_pc = nullptr;   // pinned
        unsigned long long* dbg = nullptr;  uint32_t dbg_buckets = 0;   // diagnostic phase stamps (gndt_debug_enable_stamps)
        uint32_t last_buckets = 0;
        uint64_t nodes_learned = 0;   // node count of the last successful PARTITION build (+20 %)
        // blocked buckets (gndt_blocked.hpp): 0 = not looked at yet, 1 = the map of the last build is a dense box: the next builds of
        // clouds of that size take them, -1 = no (or a blocked build failed)
        int blk_state = 0;  uint64_t blk_n = 0;  BlockMap blk_map{};  uint32_t blk_buckets = 0;
        uint32_t* d_extent = nullptr;  uint32_t* h_extent = nullptr;      // k_key_extent's seven words and their pinned mirror
        // the blocked kernel's column table (gndt_blocked.hpp, col_tab): blk_buckets << (shx + shy) 16-byte records, one per column of every
        // block, written whole by every blocked build that the per-column ordering pass follows (k_order_dest_table); sized by
        // partition_launch for the layout blocked_decide fixed (a blocked build is never recorded into a hipGraph: it may allocate)
        uint4* col_tab = nullptr;  uint64_t col_tab_cap = 0;
        int good_slots = 0; uint64_t good_est = 0, good_n = 0;   // table size / estimate that worked last time
        int good_load = 0;          //   ... and the table load (percent) if it had to be lowered (0: the default)
        int load_pct = 60;          // average LDS-table load (percent) the bucket count aims at
        // how the last PARTITION attempt of this handle was sized: a build RECORDED into a hipGraph right after it is sized the same
        // way (what the eager build allocated is then enough — what it has learnt since, e.g. "more buckets next time", would ask
        // for buffers a capture cannot allocate)
        uint64_t last_n = 0, last_est = 0, last_stage_want = 0, last_rows_floor = 0;  int last_attempt = 0, last_load = 0;
        double pair_ratio = -1.0;   // share of the last resolved build's records that sat next to one of their own node inside a bucket (< 0: unknown)
        uint64_t retries_total = 0; // builds re-run because a table / region / staging area was too small (gndt_debug_retry_count)
    } part;
    // cost-map flood over the finished grid (gndt_cost.hpp)
    struct Cost {
        uint64_t node_cap = 0;     uint32_t *h_bits = nullptr, *state = nullptr, *f[2] = {nullptr, nullptr};
        uint32_t* nbr = nullptr;       // per-flood tables, node_cap rows each: neighbour columns (8 words), own column + collision verdict (2), ring step masks (4), ring extremes (4)
        CostEdge* edges = nullptr;     // node_cap x 4 records: what a slope does to each of its neighbour cells (gndt_cost.hpp)
        CostCounters* d_cc = nullptr;   // (also counts the column index's builds: its column range bound, cost_counters)
        CostCounters* h_cc = nullptr;   // pinned
        uint64_t serial = 0;            // result_serial the flood was computed for (0 = none)
        uint64_t tables_serial = 0;     // result_serial the per-map-and-robot tables (nbr / self / edges, ring verdicts) belong to (0 = none) ...
        float tables_robot[4] = {0, 0, 0, 0};   // ... and the robot they were worked out for: the next goal on the same map reuses them
        int ring_n = 0, ring_store = 0;
    } cost;
    // the map's column index, (sx, sy) -> first row (gndt_cost.hpp k_cost_columns): one per map, built by whichever of the flood, a
    // query, a raster or a clear needs it first (column_index); keys (8 B a slot), then values (4 B a slot) in one buffer
    struct ColumnIndex {
        void* buf = nullptr;  uint64_t bytes = 0;
        uint64_t* key = nullptr;  uint32_t* val = nullptr;  uint32_t mask = 0;
        uint64_t serial = 0;            // result_serial the index was built for (0 = none)
    } index;
    // device staging of the host-pointer consumers (gndt_query, gndt_raster, gndt_clear_rays, ...: stage_in), grown on demand
    void* io = nullptr;  uint64_t io_cap = 0;     // bytes
    // region crop (gndt_crop.hpp): the second set of result arrays the kept rows are compacted into (then swapped with out / row_ncol:
    // same capacities), and the per-tile counts of the scan
    struct Crop {
        OutView spare{};  uint32_t* spare_ncol = nullptr;  uint64_t spare_cap = 0, spare_ncol_cap = 0;
        uint32_t* tiles = nullptr;  uint64_t tiles_cap = 0;     // bytes
    } crop;
    // free-space clearing (gndt_ray.hpp): per-row pass counts and protection bits, the per-column level extents (at each column's first
    // row) and the call's counters {rays, skipped, protected rows}; grown on demand
    struct Clear {
        uint32_t* passes = nullptr;  uint64_t passes_cap = 0;  void* ext = nullptr;  uint64_t ext_cap = 0;   // bytes; ext: gndt::LevelExtent[rows]
        uint64_t ext_serial = 0;        // result_serial the extents were computed for (0 = none)
        unsigned long long* d_stats = nullptr;  unsigned long long* h_stats = nullptr;   // [3], device and pinned
    } clear;
    // scan scoring (gndt_score.hpp): the per-tile partial sums of the poses one launch takes, grown on demand
    struct Score {
        void* partial = nullptr;  uint64_t partial_cap = 0;   // bytes; gndt::ScorePartial[poses of a launch][tiles]
        // scan score derivatives (gndt_score_derivs.hpp): ScoreDerivWaves[poses of a launch], then ScoreDerivPartial[poses][tiles]
        void* dpartial = nullptr; uint64_t dpartial_cap = 0;
    } score;
    // ray casting (gndt_cast.hpp): the call's counters {rays, skipped, hits}, device and pinned
    struct Cast {
        unsigned long long* d_stats = nullptr;  unsigned long long* h_stats = nullptr;
    } cast;
    // route planning (gndt_plan.hpp): the queries' per-row state and queue spill, one slot per query of a launch; stamp: the last
    // launch's (a row's state counts only with the launch's stamp, so nothing is cleared between launches); slot_bytes / rows: the
    // layout the stamps in the area belong to
    struct Plan {
        Scratch scratch;
        uint32_t stamp = 0;  uint64_t slot_bytes = 0, rows = 0;
    } plan;
    // frontier extraction (gndt_frontier.hpp): per row its parent in the union-find (4 B), its root's member count, then place in the
    // list (4 B) and its open sides (1 B), and three counts per tile of rows; grown on demand
    Scratch frontier;
    // surface patches (gndt_patch.hpp): per listed patch its ten fp64 sums (80 B), per row its parent in the union-find (4 B) and its
    // root's member count, then place in the list (4 B), and three counts per tile of rows; grown on demand
    Scratch patch;
    // scan segmentation (gndt_segment.hpp): the call's cell table (16 B a slot, the smallest power of two >= 2 n slots), per point its
    // cell's slot, then root (4 B), its parent in the union-find (4 B), its root's cells and points, then place (8 B) and its class
    // (1 B), and four counts per tile of points; grown on demand
    Scratch segment;
    // clearance field (gndt_clearance.hpp): per row the steps table of its four sides (32 B), two key arrays for the rounds' ping-pong
    // (16 B) and its tall-column bits (1 B), and one flag word per round; grown on demand
    Scratch clearance;
    // obstacle field (gndt_obstacle.hpp).  marks: per map row a column stamp and its first worklist place (4 B each) and the stamped cover
    // word (8 B), set to "never" when allocated and when the stamp would wrap, never cleared between calls: a call's stamp is marks_stamp
    // after it.  scratch: per row the worklist (4 B), the steps of its four sides (32 B), two key arrays (16 B) and the tall-column bits
    // (1 B), per box its prefix sum (8 B) and its covers-a-slope word (4 B), the header and one flag word per round; grown on demand
    struct Obstacle {
        void* marks = nullptr;  uint64_t marks_bytes = 0, marks_rows = 0;  uint32_t stamp = 0;
        Scratch scratch;
    } obstacle;
    // route field (gndt_route_field.hpp): per row the first step of its four sides with its cost (32 B), the rest of their steps (32 B),
    // the key the sweeps relax in place (8 B), the weight of entering it (4 B) and its "more" bits (1 B), and one flag word per sweep;
    // grown on demand
    Scratch route_field;
    // path walks (gndt_walk.hpp), the table variant only: per row the steps table of its four sides (32 B) and what else
    // k_clearance_steps writes (a round-0 key, 8 B, and the tall-column bits, 1 B); made again by every call that takes it
    Scratch walk;
    // map merge (gndt_merge.hpp): the call's tallies, device and pinned
    struct Merge {
        unsigned long long* d_stats = nullptr;  unsigned long long* h_stats = nullptr;
    } merge;
    // statistics exchange of a sharded build (gndt_exchange.hpp, gndt_api_dist.hip)
    struct Exchange {
        unsigned long long* d_counts = nullptr; uint64_t counts_cap = 0; unsigned long long* h_counts = nullptr;
        uint64_t *keys_in = nullptr, *keys_all = nullptr, *keys_sorted = nullptr, *canon = nullptr;
        uint64_t keys_in_cap = 0, keys_all_cap = 0, keys_sorted_cap = 0, canon_cap = 0;
        unsigned int* d_unique = nullptr;  uint32_t* d_missing = nullptr;
        char* scratch = nullptr; uint64_t scratch_cap = 0;
        double* packed = nullptr; uint64_t packed_cap = 0;  uint32_t* pfirst = nullptr; uint64_t pfirst_cap = 0;
        double* r_sums = nullptr; uint64_t r_sums_cap = 0;  uint32_t* r_count = nullptr; uint64_t r_count_cap = 0;
        double* red_tmp = nullptr; uint64_t red_tmp_cap = 0;      // thread ranks: where an in-place all-reduce is summed up
        // owner-partitioned build (gndt_build_owned_device): records grouped by owner, the records this rank owns, its
        // columns as (first-seen index, node count) pairs, everybody's pairs, the global row of every local row
        float4* send_recs = nullptr; uint64_t send_cap = 0;  float4* own_recs = nullptr; uint64_t own_cap = 0;
        uint32_t* d_matrix = nullptr; uint64_t matrix_cap = 0;  uint32_t* h_matrix = nullptr;     // [W x W] send counts
        gndt::Counters* d_split_cnt = nullptr;  gndt::Counters* h_split_cnt = nullptr;
        unsigned long long* pairs = nullptr; uint64_t pairs_cap = 0;  unsigned long long* pairs_all = nullptr; uint64_t pairs_all_cap = 0;
        uint32_t* d_npairs = nullptr;  uint32_t* global_row = nullptr; uint64_t global_row_cap = 0;
        unsigned long long* gw = nullptr; uint64_t gw_cap = 0;                                   // bitmap word + weight, packed (k_pairs_note)
        unsigned long long* d_colmsg = nullptr;  unsigned long long* h_colmsg = nullptr;         // [2 x ranks] column count, build failed
        unsigned long long* d_totals = nullptr;  unsigned long long* h_totals = nullptr;          // [4] nodes, columns, slopes, points
        hipEvent_t ev[5] = {};          // stage stamps of the sharded builds (created once, reused)
        uint32_t* h_bad = nullptr;      // pinned: the "pair beyond the index range" counter comes back here
        uint64_t send_off[1025] = {}, send_cnt[1025] = {};   // host: start and length of every owner's run in send_recs (after the split)
        bool split_one_pass = false;  uint64_t split_cap = 0;   // one-pass split: run r at r * split_cap
        // the assembled map (gndt_gather_owned_map_device): this rank's rows packed for travel, everybody's rows, the adopt tally
        uint32_t* grec = nullptr; uint64_t grec_cap = 0;  uint32_t* grec_all = nullptr; uint64_t grec_all_cap = 0;
        uint32_t* d_tally = nullptr;  uint32_t* h_tally = nullptr;
        uint64_t owned_serial = 0;  uint32_t owned_world = 0;   // result_serial / ranks of the owned build global_row describes (0: none)
        bool gathered = false;                                  // gndt_gather_owned_map_device has run for that build (every rank: once per build)
        uint32_t* d_status = nullptr;                           // scratch word for the status kernels
        // agreement rounds (gndt_api_dist.hip `agree`): one word per rank, device and pinned; allocated with the handle, so that a
        // rank can ALWAYS say "I cannot go on" — whatever else it failed to allocate
        unsigned long long* d_agree = nullptr;  unsigned long long* h_agree = nullptr;
        int inject_site = 0;                                    // tests: the allocation site that fails next (gndt_debug_fail_next_alloc)
        // sliced global rows: the first row of every pair of this rank, everybody's pair places, this rank's, slice totals / rows
        uint32_t* row_of_pair = nullptr; uint64_t row_of_pair_cap = 0;  uint32_t* place_all = nullptr; uint64_t place_all_cap = 0;
        uint32_t* place_mine = nullptr; uint64_t place_mine_cap = 0;  unsigned long long* d_slice = nullptr;   // [2 mine | 2W all | W rows]
        // locality-aware ownership (gndt_exchange.hpp): this rank's sample message, everybody's, the block table
        uint32_t* owner_msg = nullptr;  uint32_t* owner_msgs_all = nullptr; uint64_t owner_msgs_cap = 0;
        uint32_t* bkey = nullptr;  uint32_t* bcnt = nullptr; uint64_t bcnt_cap = 0;  uint8_t* bown = nullptr;  uint32_t* d_owner_full = nullptr;
        uint32_t owner_map_world = 0;   // ranks the block table in bkey / bown was made for (0: none — hash ownership)
    } exch;
    uint64_t result_serial = 0;         // bumped whenever a build / finalize produces new result rows
    int last_strategy = GNDT_STRATEGY_ATOMIC;
    // strategy AUTO: what the locality sample said last time, for which cloud size, and how many builds ago
    int tile_choice = -1;  uint64_t tile_choice_n = 0;  int tile_choice_age = 0;  double tile_ratio_seen = 0.0;
    unsigned long long* d_sample = nullptr;  unsigned long long* h_sample = nullptr;   // k_tile_sample's counters {points, nodes, ticket} and the pinned words its last workgroup fills
    // a locality sample whose answer has not been looked at yet (round 6: a build on a handle that already has room for any answer does
    // not wait for it — the build it rides in front of takes the handle's last choice, the next one finds the answer)
    bool sample_pending = false;  uint64_t sample_n = 0;  hipEvent_t sample_ev = nullptr;
    uint32_t* d_sketch = nullptr;  uint32_t* h_sketch = nullptr;                        // k_node_sketch's HyperLogLog registers (pinned copy)
    bool map_in_table = true;   // false after a PARTITION build: the HBM node table does not hold the map

    // optional phase timing (bench / profiling): events recorded on the launch stream
    int prof = 0;               // 0 off, 1 every phase, 2 only the dominant phase of the strategy in use
    // one event set per build in a ring, so that back-to-back (un-synchronised) builds can all be timed
    static constexpr int kEvSets = 32;
    hipEvent_t ev[kEvSets][GNDT_NUM_PHASES + 1] = {};
    bool ev_recorded[kEvSets][GNDT_NUM_PHASES + 1] = {};
    int ev_set = 0;

    // A PARTITION build is launched without waiting for it; its overflow flags are looked at (and the build
    // re-run with more room if they are set) by the next call that needs the result.
    struct Pending {
        bool active = false;
        const void* xyz = nullptr; size_t n = 0, stride = 0;
        hipStream_t s = nullptr;
        int attempt = 0, bslots = 0;
        int load_pct = 0;               // average LDS-table load this build aims at (0: the handle's default)
        uint64_t nodes_est = 0, stage_want = 0, est0 = 0;   // est0: the estimate the first attempt used
        uint64_t rows_floor = 0;        // staging rows THIS build asks for whatever the handle already has (stage_want also covers what it has)
        bool est_reliable = false;      //   ... and whether it came from a hint / an earlier build rather than the n / 4 guess
        bool two_level = false;         // this attempt used the two-level partition
        bool one_level = false;         //   ... the one-level tile partition (small clouds)
        bool retry_pass = false;        //   ... and the bucket kernel's second pass behind the first (overflowing 512-slot tables done again with 1024)
        double mean1 = 0.0;             // its mean level-1 region fill (to turn the fullest region into a ratio)
        bool stats_only = false;        // gndt_shard_stats_device: statistics out, no labels / ordering / rows
        bool blocked = false;           // this attempt used blocked buckets (gndt_blocked.hpp)
        bool no_block = false;          //   ... a blocked attempt of this build failed: hashed buckets from here on
        uint64_t captured_gen = 0;      // Handle::realloc_gen when this build was recorded (captured builds only)
        bool captured = false;          // launched on a stream under hipGraph capture: it runs when the graph is replayed, with the
                                        //   buffers it was recorded with — never re-run here with more room (new buffers: the graph holds the old)
        bool replay_failed = false;     // the last replay of this build ran out of room (results_valid is false because of that, and only that)
        uint64_t done_serial = 0;       // result_serial when this build was resolved: while the handle still shows that serial, the map
                                        //   on the device can only have been replaced by a REPLAY of this build (hipGraph)
        gndt::GridParams gp{};          // origin and grid parameters AS THEY WERE when the build was launched: a retry
                                        // re-runs the same build even if the handle's origin has moved on since
        uint32_t first_base = 0;        // global index of xyz[0] (shards of a global cloud)
        bool records = false;           // the input is 16-B records {x, y, z, index word} (owner-partitioned build): the index
        uint64_t index_range = 0;       //   word is taken as it is; point indices then run over [0, index_range) (0: n)
        const void* xyz2 = nullptr; size_t n2 = 0;   // records only: a second segment, PRECEDED in its allocation by room for the
                                        //   first one (the exact partition reads one array: the first segment is copied in front)
    } pending;

    std::string err;
};

namespace gndt_host {
using namespace gndt;

// What a process can set about the library, and nothing else: a field of Tuning is set by a gndt_debug_* call (process-wide, for the
// calls that follow), by one of the -D macros of DESIGN §4.5 (A/B builds) or by tuning_force_*.  The library reads no environment variable.
// Choices that lost their knob are constants here or at the place they decide, each with the measurement that set it.
// (Folded into constants in round 4, each after losing its A/B: level-1 cursor replicas (1), workgroups of the counting partition
//  (256), incremental updates through the tile kernel (by strategy), every rank ordering all columns instead of its slice (no).)
constexpr int kPartWgs = 256;    // workgroups of the exact counting partition
constexpr int kBucketLoad = 60;        // average LDS-table load (percent) that sizes the bucket count
constexpr int kBucketLoadLarge = 75;   // the same from 2 M points on (the chip is full either way: fuller tables, fewer buckets; 85 / 92 with the second pass behind them: noise, r05 §4)
constexpr uint32_t kL1Wgs = 2048;      // level-1 workgroups (512 are resident: 2048 of them, ~1.2 tiles each, 69 us against 75 with 1024 and 72 with 512 on the bench scene, r05 §5)
struct Tuning {
    // set at build time (-D, each with its A/B in profiles/r06_ablation.txt) ...
#ifndef GNDT_BUCKET_POINTS
#define GNDT_BUCKET_POINTS 0
#endif
    int bucket_points = GNDT_BUCKET_POINTS;       // points per bucket (0 = derived: 700 .. 3600 with the cloud's size)
#ifndef GNDT_PLACE_EMIT_WORDS
#define GNDT_PLACE_EMIT_WORDS 16384
#endif
    int place_emit_words = GNDT_PLACE_EMIT_WORDS;    // PARTITION builds of clouds with up to this many bitmap words (32 points each): ordering + emit as one kernel
                                                     //   in scatter form (gndt_partition.hpp k_place_emit_rows; 0: never)
#ifndef GNDT_BLOCKED
#define GNDT_BLOCKED 1
#endif
    int blocked = GNDT_BLOCKED;  // clouds whose map is a dense, evenly filled box: spatial blocks as buckets, directly addressed tables (round 6)
#ifndef GNDT_THREE_WGS
#define GNDT_THREE_WGS 1
#endif
    int bucket_three_wgs = GNDT_THREE_WGS;    // clouds without locality: the bucket kernel with one record per thread at three workgroups per CU (round 6)
#ifndef GNDT_FOLD_CLEAR
#define GNDT_FOLD_CLEAR 1
#endif
    int fold_clear = GNDT_FOLD_CLEAR;    // eager PARTITION builds: no k_part_clear launch — level 1 prepares the next build's cursors / counters (Part::cursors_alt)
    int fp_bits = 21;            // bits of the bucket kernel's index fingerprint (tests narrow it through gndt_debug_set_fp_bits to force clashes)
    // ... and what gndt_debug_set_option / gndt_debug_enable_stamps can set (process-wide)
    double tile_ratio = 48.0;    // GNDT_DEBUG_TILE_RATIO   AUTO takes strategy TILE from this many points per partial on (sampled; the
                                 //                         measured crossover, profiles/r02_tile_calibration.json; tools/calibrate_tile.py sweeps it)
    bool stamps = false;         // gndt_debug_enable_stamps: in-kernel phase stamps of the bucket kernel
    bool verbose = false;        // GNDT_DEBUG_VERBOSE      stderr line per resolved two-level build
    bool cost_one_workgroup = true;   // GNDT_DEBUG_COST_ONE_WORKGROUP   0: every layer of the flood its own launch
    int query_ilp = 1;           // GNDT_DEBUG_QUERY_ILP           queries a thread of k_query works on at once (1, 2 or 4)
    int plan_lds_entries = 1024; // GNDT_DEBUG_PLAN_LDS_ENTRIES    entries of a planning query's open queue kept in LDS (64 .. 1024; the rest spills)
    bool clearance_one_workgroup = true;   // GNDT_DEBUG_CLEARANCE_ONE_WORKGROUP   0: every round of the clearance field its own launch
    bool obstacle_tally = false;           // GNDT_DEBUG_OBSTACLE_TALLY            1: the obstacle field's marking pass keeps the tallies gndt_debug_obstacle_marks reads
    bool route_field_one_workgroup = true; // GNDT_DEBUG_ROUTE_FIELD_ONE_WORKGROUP 0: every sweep of the route field its own launch
    bool patch_lds = true;                 // GNDT_DEBUG_PATCH_LDS                 0: the patches' moment pass sends every wave's sums to memory itself
    int view_threads = 1024;               // GNDT_DEBUG_VIEW_THREADS              threads of a view gain workgroup at most (64 .. 1024, whole waves; same records at every value)
    int walk_step_table = 2;               // GNDT_DEBUG_WALK_STEP_TABLE          gndt_walk_paths*: 0 the steps found on the walk, 1 read from a per-call table, 2 by the map's size
    bool clear_extent = false;   // GNDT_DEBUG_CLEAR_EXTENT        the ray walk reads a column's rows only if its level extent meets the ray's
                                 //   level range (lost its A/B on the S4 frame: walk 1057 against 958 µs)
    uint32_t blocked_min_points = 1u << 20;   // GNDT_DEBUG_BLOCKED_MIN_POINTS   points from which a build may take BLOCKED buckets (65 536 .. 2^20; tests lower it)
    bool column_dest = true;     // GNDT_DEBUG_COLUMN_DEST         BLOCKED builds that end in the two-kernel tail: the ordering pass runs over the
                                 //   bucket kernel's column table (k_order_dest_table); 0: over the staged nodes (k_order_dest_columns, ord_cf / ord_idx)
                                 // GNDT_DEBUG_PLACE_EMIT_WORDS sets place_emit_words (above)
};
const Tuning& tuning();
void tuning_force_stamps(bool on);   // bench.py --stamps flips this after the timed run
void tuning_force_fp_bits(int bits); // tests: narrow the fingerprint so that clashes happen
int tuning_set_option(int option, double value);

#define HIP_TRY(h, expr)                                                                                 \
    do {                                                                                                 \
        hipError_t e__ = (expr);                                                                         \
        if (e__ != hipSuccess) {                                                                         \
            (h)->err = std::string(#expr) + ": " + hipGetErrorString(e__);                               \
            return GNDT_ERR_HIP;                                                                         \
        }                                                                                                \
    } while (0)

// Allocating, freeing or waiting while a stream of the process is being captured makes HIP refuse the call AND invalidate the
// capture (hipErrorStreamCaptureInvalidated at hipStreamEndCapture; round 3's fuzz: one such capture and every later capture of
// the process was refused).  Code that is about to do one of these asks first and reports GNDT_ERR_CAPACITY — a clean error the
// caller answers with gndt_reserve() (or an eager build of the same size) before capturing.
#define GNDT_NO_CAPTURE(h, what)                                                                                              \
    do {                                                                                                                      \
        {   /* asked of the stream itself: entry points that enqueue nothing (gndt_sync, gndt_export*) do not pass use_stream, and a flag left by the last captured call would refuse them */ \
            hipStreamCaptureStatus c__ = hipStreamCaptureStatusNone;                                                          \
            (void)hipStreamIsCapturing((h)->last_stream, &c__);                                                               \
            (h)->capturing = c__ != hipStreamCaptureStatusNone;                                                               \
        }                                                                                                                     \
        if ((h)->capturing) {                                                                                                 \
            (h)->err = std::string(what) + " must be (re)allocated or waited for, which a stream under hipGraph capture cannot do: "  \
                       "call gndt_reserve(max_points, max_nodes) — or build a cloud of this size eagerly — before capturing";  \
            return GNDT_ERR_CAPACITY;                                                                                         \
        }                                                                                                                     \
    } while (0)

inline void mark(gndt_handle* h, int i, hipStream_t s) {
    if (!h->prof || !h->ev[h->ev_set][i]) return;
    if (h->prof == 2) {   // the bucket kernel sits between marks 4 and 5, k_accumulate between 1 and 2
        const int lo = h->last_strategy != GNDT_STRATEGY_ATOMIC ? 4 : 1;
        if (i != lo && i != lo + 1) return;
    }
    (void)hipEventRecord(h->ev[h->ev_set][i], s);
    h->ev_recorded[h->ev_set][i] = true;
}

// a new build / update starts: next event set of the ring
inline void next_event_set(gndt_handle* h) {
    if (!h->prof) return;
    h->ev_set = (h->ev_set + 1) % gndt_handle::kEvSets;
    for (auto& r : h->ev_recorded[h->ev_set]) r = false;
}

inline int grid_for(uint64_t work, int block = kBlock, int max_blocks = 256 * 8) {
    uint64_t b = (work + block - 1) / block;
    if (b < 1) b = 1;
    if (b > (uint64_t)max_blocks) b = max_blocks;
    return (int)b;
}

inline uint32_t pow2_ceil(uint64_t v) {
    uint64_t p = 1024;
    while (p < v && p < (1ull << 31)) p <<= 1;
    return (uint32_t)p;
}

inline GridParams grid_params(const gndt_handle* h) {
    GridParams g{};            // (blk.on = 0: buckets by column hash; partition_launch fills the block map in when it takes the blocked build)
    g.ox = h->origin[0]; g.oy = h->origin[1]; g.oz = h->origin[2];
    g.grid_len = h->P.grid_len; g.z_len = h->P.z_len; g.slope_interval = h->P.slope_interval;
    g.demand = h->P.demand; g.min_points = h->P.min_points;
    g.inv_grid = 1.0f / g.grid_len; g.inv_z = 1.0f / g.z_len;     // correctly rounded on the host
    return g;
}

// slots wanted for `nodes` occupied entries (load factor <= 1/2)
inline uint32_t cap_for_nodes(uint64_t nodes) { return pow2_ceil(std::max<uint64_t>(2048, nodes * 2)); }

// NULL = the handle's own stream; hipStreamLegacy (the null stream by its explicit name) = the null stream handle itself,
// which every HIP call accepts (some do not accept the named constant)
inline hipStream_t stream_of(gndt_handle* h, void* hip_stream) {
    if (!hip_stream) return h->own_stream;
    return (hipStream_t)hip_stream == hipStreamLegacy ? (hipStream_t) nullptr : (hipStream_t)hip_stream;
}

// a device buffer of the handle goes out of use (see Handle::retired)
inline void release_device(gndt_handle* h, void* p, bool bump = true) {     // (bump = false: the node table, which has a generation of its own)
    if (!p) return;
    if (bump) ++h->realloc_gen;
    if (h->ever_captured) h->retired.push_back(p); else (void)hipFree(p);
}

// A device buffer that a consumer owns and never records into a graph, grown to `bytes` on demand and plainly freed.  (Not grow_buf:
// that one retires the old buffer and bumps realloc_gen, which would report unrelated recorded graphs as stale.)
template <typename T>
int grow_scratch(gndt_handle* h, T*& p, uint64_t& cap, uint64_t bytes) {
    if (bytes <= cap) return GNDT_OK;
    if (p) (void)hipFree(p);
    p = nullptr; cap = 0;
    HIP_TRY(h, hipMalloc(&p, bytes));
    cap = bytes;
    return GNDT_OK;
}

inline void free_scratch(gndt_handle::Scratch& a) { if (a.p) (void)hipFree(a.p);  a = gndt_handle::Scratch{}; }

// A consumer's per-call scratch: LAYOUT (a layout struct over gndt_scratch.hpp's Carver) run over a null base for the bytes, the area
// grown to them, the pieces carved from it.  What is carved is what was counted.
template <typename LAYOUT, typename... SIZES>
int carve_scratch(gndt_handle* h, gndt_handle::Scratch& a, LAYOUT& out, SIZES... sizes) {
    Carver sizer;
    (void)LAYOUT(sizer, sizes...);
    const int rc = grow_scratch(h, a.p, a.bytes, sizer.pos);
    if (rc) return rc;
    Carver c(a.p);
    out = LAYOUT(c, sizes...);
    return GNDT_OK;
}

// The row numbers of a finished map as the consumers' 32-bit words (kNoRow excepted)
inline int rows_fit_32(gndt_handle* h, const char* entry) {
    if (h->res_nodes < 0xFFFFFFFFull) return GNDT_OK;
    h->err = std::string(entry) + ": row numbers do not fit 32 bits";
    return GNDT_ERR_CAPACITY;
}

// one of the pointers has a bit of `mask` set (null is aligned)
inline bool misaligned(uintptr_t mask, std::initializer_list<const void*> ptrs) {
    return std::any_of(ptrs.begin(), ptrs.end(), [mask](const void* p) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; });
}

// A cache of the map (the column index, the clear's level extents, the flood's per-map tables) is current while the map is the one it
// was made for — never on a handle that has recorded a hipGraph: a replay rewrites the map without the host's serial moving
inline bool map_current(const gndt_handle* h, uint64_t serial) { return serial && serial == h->result_serial && !h->ever_captured; }

// The ten result-row arrays of an OutView or a gndt_cells (the same fields) and the bytes a row takes in each: 76 in all
struct RowArray { void** p; size_t elem; };
template <typename V>
std::array<RowArray, 10> row_arrays(V& v) {
    return {{{(void**)&v.sx, 4}, {(void**)&v.sy, 4}, {(void**)&v.sz, 4}, {(void**)&v.count, 4}, {(void**)&v.first_idx, 4},
             {(void**)&v.mean, 12}, {(void**)&v.cov, 24}, {(void**)&v.rough, 4}, {(void**)&v.normal, 12}, {(void**)&v.flags, 4}}};
}

template <typename T>
int grow_buf(gndt_handle* h, T*& p, uint64_t& cap, uint64_t want) {
    if (want <= cap) return GNDT_OK;
    GNDT_NO_CAPTURE(h, "a work buffer");
    // Once a graph has been recorded an outgrown buffer is kept until gndt_destroy (release_device): a handle whose eager clouds
    // grow slowly would keep the sum of all earlier sizes.  Growing by half bounds what is retired to twice the final size.
    if (h->ever_captured && cap) want = std::max<uint64_t>(want, cap + cap / 2);
    release_device(h, p);
    p = nullptr; cap = 0;
    HIP_TRY(h, hipMalloc(&p, want * sizeof(T)));
    cap = want;
    return GNDT_OK;
}

// "a cloud of this size": within a quarter of `of`, either way (the blocked box, AUTO's locality sample, the warm-up)
inline bool within_quarter(uint64_t n, uint64_t of) { return n <= of + of / 4 && n + n / 4 >= of; }

// One launch of k_part2_level1 (gndt_partition.hpp) by name.  What is left at its default is what a launch without it passes.
struct Level1Launch {
    const float* in = nullptr;  uint64_t n = 0;  int stride_floats = 4;   // the input: points of 3 or 4 floats, or 16-byte records
    uint32_t first_base = 0;    // global index of in[0]
    GridParams gp{};
    uint32_t B = 0, F1 = 0, F2_shift = 0;       // buckets (ranks), level-1 regions, log2 of the level-2 fan-out
    uint32_t replicas = 1;      // sub-regions per region (cursor replicas)
    bool fan512 = false;        // more than 256 regions: the LDS arrays of the large fan-out
    bool small_tiles = false;   // points only: tiles of kTilePerSmall points per thread
    uint32_t* cursor1 = nullptr;  uint32_t cap1 = 0;  int cursor_shift = 0;      // the regions' fills, a region's room, the cursors' spacing (log2 words)
    uint32_t* est2 = nullptr;   // the sample votes
    float4* recs1 = nullptr;    // the output records
    Counters* cnt = nullptr;  PartCounters* pc = nullptr;
    uint32_t compress = 0;
    OwnerMap owner{nullptr, nullptr, 0u, nullptr};
    uint32_t *range_lo = nullptr, *range_cap = nullptr;  uint64_t rec_cap = 0;   // the buckets' layout, written by the last workgroup to finish (null: none)
    FoldClear fold{};
    dim3 grid{1};
};
// What the input is decides which instantiations a translation unit carries: Points <3|4, 256|512> and the same with kTilePerSmall,
// Records <4, 256|512, true>, OwnerSplit <3|4, 256, false, true> (gndt_api_dist.hip; at most 256 ranks).
enum class Level1Input { Points, Records, OwnerSplit };
template <int SF, int FAN, auto... MORE>      // (MORE: IDXW, OWNER, PER1 — the kernel's own defaults where left out)
void enqueue_level1(const Level1Launch& a, hipStream_t s) {      // (the one place that knows the kernel's argument order)
    hipLaunchKernelGGL((k_part2_level1<SF, FAN, MORE...>), a.grid, dim3(kTileThreads), 0, s, a.in, a.n, a.first_base, a.gp, a.B, a.F1, a.F2_shift,
                       a.replicas, a.cursor1, a.cap1, a.est2, a.recs1, a.cnt, a.pc, a.compress, a.owner, a.range_lo, a.range_cap, a.rec_cap, a.fold, a.cursor_shift);
}
template <Level1Input IN>
void launch_level1(const Level1Launch& a, hipStream_t s) {
    const bool f3 = a.stride_floats == 3, wide = a.fan512;
    if constexpr (IN == Level1Input::OwnerSplit) {
        if (f3) enqueue_level1<3, 256, false, true>(a, s); else enqueue_level1<4, 256, false, true>(a, s);
    } else if constexpr (IN == Level1Input::Records) {
        if (wide) enqueue_level1<4, 512, true>(a, s); else enqueue_level1<4, 256, true>(a, s);
    } else if (a.small_tiles) {
        if (f3) { if (wide) enqueue_level1<3, 512, false, false, kTilePerSmall>(a, s); else enqueue_level1<3, 256, false, false, kTilePerSmall>(a, s); }
        else { if (wide) enqueue_level1<4, 512, false, false, kTilePerSmall>(a, s); else enqueue_level1<4, 256, false, false, kTilePerSmall>(a, s); }
    } else {
        if (f3) { if (wide) enqueue_level1<3, 512>(a, s); else enqueue_level1<3, 256>(a, s); }
        else { if (wide) enqueue_level1<4, 512>(a, s); else enqueue_level1<4, 256>(a, s); }
    }
}

// ---- gndt_api_core.hip: shared buffers ----
int create_handle(const gndt_params* params, gndt_handle** out, hipStream_t borrowed_stream);   // gndt_create's body
int check_ready(gndt_handle* h);
// A finished map for a consumer: a pending build resolved, results_valid (else no_map_err), gndt_sync; with key_range_ok a
// GNDT_ERR_KEY_RANGE of the build does not stop the caller (crop, clear)
int finished_map(gndt_handle* h, const char* no_map_err, bool key_range_ok);
int refuse_capture(gndt_handle* h, hipStream_t s, const char* msg);   // GNDT_ERR_INVALID with msg when s is under hipGraph capture
int alloc_rows(gndt_handle* h, OutView& v, uint64_t rows);            // the ten result-row arrays, `rows` rows each
// One array of a host-pointer entry point: `bytes` of staging at dev (stage_in sets it), filled from `in` before the kernels and copied
// to `out` behind them (either may be null: an output, an input, or room that the entry point copies from itself)
struct IoPiece {
    const void* in;  void* out;  uint64_t bytes;
    void* dev = nullptr;
    template <typename T> T* as() const { return static_cast<T*>(dev); }
};
// an input / an output of the caller's; null: not passed, so no room and a null kernel argument
inline IoPiece io_in(const void* host, uint64_t bytes) { return IoPiece{host, nullptr, host ? bytes : 0}; }
inline IoPiece io_out(void* host, uint64_t bytes) { return IoPiece{nullptr, host, host ? bytes : 0}; }
// the host-pointer consumers' staging (h->io): every piece's dev, 256-byte aligned (null where its bytes are 0)
int stage_pieces(gndt_handle* h, IoPiece* pieces, int count);
int stage_in(gndt_handle* h, IoPiece* pieces, int count, hipStream_t s);          // staged; every piece with `in` and bytes copied in, in order
int stage_out(gndt_handle* h, const IoPiece* pieces, int count, hipStream_t s);   // every piece with `out` and bytes copied out, in order; the stream awaited
template <int N> int stage_in(gndt_handle* h, IoPiece (&pieces)[N], hipStream_t s) { return stage_in(h, pieces, N, s); }
template <int N> int stage_out(gndt_handle* h, const IoPiece (&pieces)[N], hipStream_t s) { return stage_out(h, pieces, N, s); }
// More dynamic LDS than the default has to be asked for once per device (the attribute belongs to the function ON the current device,
// which check_ready has made the handle's).  `grant` is the asking kernel's own (static storage).  A refusal clears the sticky error
// and is final: the caller launches per round from then on.  Devices outside 0-63 are never granted.
struct LdsGrant { std::atomic<int> state[64]; };        // per device: 0 not asked yet, 1 granted, 2 refused
bool lds_granted(const gndt_handle* h, const void* kernel, uint32_t bytes, LdsGrant& grant);
int use_stream(gndt_handle* h, hipStream_t s);     // work moves to stream s: it waits for what the handle's last stream still runs
int ensure_out(gndt_handle* h, uint64_t n);
int ensure_stats_buffers(gndt_handle* h, uint64_t n);
int ensure_stage(gndt_handle* h, uint64_t nodes, bool rows = true);   // rows = false: the order arrays only (PARTITION: RawNode records, ensure_raw)
int ensure_raw(gndt_handle* h, uint64_t records);
int ensure_words(gndt_handle* h, uint64_t words);
int ensure_part_counters(gndt_handle* h);
int ensure_cursors(gndt_handle* h, uint64_t buckets);   // gndt_api_build.hip
int fetch_counters(gndt_handle* h, hipStream_t s);   // read the device counters (synchronises the stream)
int stage_host_input(gndt_handle* h, const void* xyz_host, size_t n, size_t stride_bytes, hipStream_t s);
void free_part(gndt_handle* h);
// ---- gndt_api_table.hip ----
void free_table(gndt_handle* h);
int alloc_table(gndt_handle* h, uint32_t cap, hipStream_t s);
int do_reset(gndt_handle* h, hipStream_t s);
int zero_device_now(gndt_handle* h, void* p, size_t bytes);
int partition_recheck_after_replay(gndt_handle* h);
int reserve_table(gndt_handle* h, uint64_t nodes, hipStream_t s);
int stats_merge_head(gndt_handle* h, uint64_t nodes, void* hip_stream, hipStream_t* s);   // gndt_stats_merge_device up to its kernel: room for `nodes` more
int drop_dead_and_finalize(gndt_handle* h, hipStream_t s);   // gndt_remove* / gndt_clear_rays*: drop the nodes left empty, re-finalise every row
int table_refinalize(gndt_handle* h);      // the regular finalisation after the small-map one gave up (gndt_sync)
int table_emit_pending(gndt_handle* h);    // deferred-emit mode: the ordering + emit pass the frames since the last read left out (gndt_sync)
int build_atomic(gndt_handle* h, const void* xyz_dev, size_t n, size_t stride_bytes, hipStream_t s, bool tile = false,
                 const gndt_handle::Pending* rec = nullptr);
int locality_sample(gndt_handle* h, const void* xyz_dev, size_t n, size_t stride_bytes, uint32_t tiles, double* ratio, hipStream_t s);
int locality_sample_begin(gndt_handle* h, const void* xyz_dev, size_t n, size_t stride_bytes, uint32_t tiles, hipStream_t s);   // launched, not awaited
int ensure_sample_buffers(gndt_handle* h);
bool locality_sample_take(gndt_handle* h, bool wait, double* ratio);                                                          // its answer, if there is one
int sketch_nodes(gndt_handle* h, const void* xyz_dev, size_t n, size_t stride_bytes, hipStream_t s, uint64_t* estimate);   // HyperLogLog over the node keys (waits)
// ---- gndt_api_build.hip ----
// tab_end: the table path's end-of-frame bookkeeping (k_tab_end + `advance` points of stream position) done by k_emit_rows
// partial: incremental finalisation — only rows from the first changed column on are placed and gathered again, touched rows in
//          front of it are emitted where they are (k_order_dest / k_emit_rows, gndt_partition.hpp)
int launch_order_and_emit(gndt_handle* h, uint64_t words, int m0, hipStream_t s, bool grouped = false, bool counters_to_host = false,
                          bool tab_end = false, uint32_t advance = 0, bool partial = false, uint32_t col_records = 0);
int partition_launch(gndt_handle* h, gndt_handle::Pending& P);
int partition_begin(gndt_handle* h, const void* xyz_dev, size_t n, size_t stride_bytes, hipStream_t s, bool records = false, uint64_t index_range = 0,
                    const void* records2 = nullptr, size_t n2 = 0);
int partition_resolve(gndt_handle* h);
// ---- gndt_api_cost.hip ----
void free_cost(gndt_handle* h);
int cost_counters(gndt_handle* h);        // h->cost.d_cc and its pinned mirror h_cc, allocated together by whoever comes first
int cost_map_check(gndt_handle* h);       // GNDT_ERR_INVALID unless the flood's cost map is the current map's
// The map's column index (h->index), built on stream s unless it is current (the caller has passed use_stream, the flood excepted).
// flood: the flood's one k_cost_clear, which also resets its h array (and clears no table when the index is current)
int column_index(gndt_handle* h, hipStream_t s, bool flood = false);
// ---- gndt_api_query.hip ----
// the steps before a query's or a raster's kernel: no capture, a finished map, the cost map when gathered; and the view of rows,
// index and cost map the kernels read
int query_sync(gndt_handle* h, bool gather, hipStream_t s, const char* capture_err);
gndt::QueryView query_view(gndt_handle* h);     // every field the handle supplies; the flood's tables (V.nbr, V.self, V.edges) are null
// The robot of a call: the caller's, or the flood's defaults (receiver.cpp:33, robot.h:38-46)
inline gndt::Robot robot_of(const gndt_robot* robot) {
    if (!robot) return gndt::Robot{0.25f, 0.15f, 100.f, 30.f};
    return gndt::Robot{robot->radius, robot->reachable_height, robot->max_rough, robot->max_angle_deg};
}
// ---- gndt_api_crop.hip ----
void free_crop(gndt_handle* h);
// ---- gndt_api_clear.hip ----
void free_clear(gndt_handle* h);
// ---- gndt_api_score.hip ----
void free_score(gndt_handle* h);
// ---- gndt_api_cast.hip ----
void free_cast(gndt_handle* h);
// ---- gndt_api_merge.hip ----
void free_merge(gndt_handle* h);
// ---- gndt_api_obstacle.hip ----
void free_obstacle(gndt_handle* h);        // (the marks beside the scratch)

}  // namespace gndt_host
