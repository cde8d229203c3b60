// hmk_ctx.h -- the context behind the C ABI and what the translation units of libhammock_hip.so's host side share:
// hmk_api.cpp (the extern "C" entry points: argument checks, locking, dispatch), hmk_common.cpp (errors, device, the grow-only
// buffers and their owners, streams), hmk_sizing.h (the sizing rules, pure functions), hmk_plan.cpp (the neighbour passes' planner),
// hmk_pass.cpp (launching the passes; the pair and block probes), hmk_cluster.cpp (the single-device clustering calls, CSR pipeline,
// row hand-over, second-loop driver), hmk_multi.cpp (the same calls on several devices), and one file per further call
// (hmk_search.cpp ... hmk_components.cpp, hmk_align.cpp, hmk_survey.cpp, hmk_separation.cpp, hmk_sweep.cpp, hmk_representatives.cpp, hmk_density.cpp, hmk_profile.cpp, hmk_scan.cpp, hmk_orders.cpp; hmk_levels.cpp: what the threshold-range calls among them share; hmk_slots.cpp: what the calls over given clusters share).  Not part of the public ABI.
#ifndef HMK_CTX_H
#define HMK_CTX_H
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <future>
#include <memory>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <numeric>
#include <string>
#include <tuple>
#include <thread>
#include <vector>

#include "hmk_internal.h"
#include "hmk_kernels.h"
#include "hmk_sizing.h"

using namespace hmk;

namespace hmk { namespace impl {

struct Group {
    int path;
    int nw;
    int lbk;  // column-length capacity of the kernel instantiation
    uint32_t base, count;
    uint32_t band;  // the first `band` tiles of the group touch a "band" row (caller index < Plan::band_rows)
    uint64_t work;  // cells its tiles add (pairs x cells per pair): what the launches of a forked pass are balanced by (hmk_pass.cpp)
};

// grow-only device storage (one hipMalloc per buffer and context, not per call): the greedy tail's scratch sb[] and a few named ones
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    template <class T> T *as() const { return (T *)p; }
    void release();   // (hmk_common.cpp, as the other owners': a failed free does not stay behind as the thread's last error)
};
// pinned host block, grow-only
struct PinnedBuf {
    void *p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes, size_t keep);   // the first `keep` bytes survive a reallocation
    void release();
};
// The internal edge buffer of a context: HMK_EDGE_SHARDS segments of seg_cap() entries and the segments' counts.  What the
// host-buffer entry points, the clustering calls and the searches score into.
struct EdgeBuffer {
    uint64_t *d = nullptr;
    uint64_t cap = 0;
    unsigned long long *counts = nullptr;
    int reserve(hmk_ctx *ctx, uint64_t want);   // grow-only (and the counts at first use); the error goes to ctx
    uint64_t seg_cap() const { return cap / HMK_EDGE_SHARDS; }
    EdgeSegs segs() const { return shard_segments(d, seg_cap(), counts); }
    int fetch(hmk_ctx *ctx, const unsigned long long n[HMK_EDGE_SHARDS], uint64_t *host_out) const;   // the segments' entries, back to back
    void release();
};
inline uint64_t total_of(const unsigned long long counts[HMK_EDGE_SHARDS]) { return std::accumulate(counts, counts + HMK_EDGE_SHARDS, (uint64_t)0); }
inline uint64_t max_of(const unsigned long long counts[HMK_EDGE_SHARDS]) { return *std::max_element(counts, counts + HMK_EDGE_SHARDS); }
enum {
    SB_DEG, SB_CURSOR, SB_START, SB_SCAN, SB_RANGE, SB_ADJ, SB_PART, SB_PARTSCR,   // full CSR (+ the bucketed lower sections)
    SB_BDEG, SB_BCURSOR, SB_BSTART, SB_BSCAN, SB_BRANGE, SB_BADJ, SB_BCOUNTS,     // band CSR (first rows only)
    SB_BNCNT, SB_BNUP, SB_BNSTART, SB_BFTOP, SB_BFMORE, SB_FDEG, SB_FSTART, SB_FADJ, SB_TRCNT, SB_TRSTART,   // the band prepared for phase 1 (BandPack)
    SB_COF, SB_BITMAP, SB_USIZE, SB_LEFT, SB_CNT, SB_CSTART, SB_OVER, SB_SCAN2, SB_CAND,             // pre-check of the second loop
    SB_JOINED, SB_CSIZE, SB_CID, SB_SEQSZ, SB_STATUS, SB_CHOICE, SB_FIRST, SB_ACTIVE, SB_DIRTY, SB_SUBS2, SB_RETRY, SB_PRECNT, SB_ACCEPTED, SB_JSLOT, SB_LCOUNT, SB_SUBSTART, SB_SUBS,   // device-side second loop
    SB_PEER, SB_PEERCNT, SB_PEERBAND, SB_PEERDEG,   // multi-device calls: the inbox of edge blocks from the other devices + their counts, band blocks (peers: compacted; root: gathered), degree slices
    SB_ROUTE, SB_ROUTECNT,                          // ... this device's edges dealt into one block per owning device; counts / offsets / cursors
    SB_REPL,                                        // ... (in a peer's context, on the ROOT's device) the peer's piece copied to the root: no peer access, or HMK_MULTI_REPLICATE
    SB_SEARCH_OUT, SB_SEARCH_CNT, SB_SEARCH_START, SB_SEARCH_SCAN, SB_SEARCH_HITS,   // query-vs-reference search (hmk_search.cpp): edges / keys,
                                                                                     // per-query counts + cursors, run starts, scan scratch, best-k
                                                                                     // (the assignment, hmk_assign.cpp, uses them too)
    SB_ASSIGN_CL,                                   // the assignment's clusters: member -> rank, members per rank, slot of each rank
    SB_MATCH_CL,                                    // the match's clusters (hmk_match.cpp): SB_ASSIGN_CL's + query member -> query slot, members per query slot
    SB_MATCH_REC,                                   // ... per query member its feasible (rank, min score) records
    SB_MATCH_SCR,                                   // ... feasible counts per query member, per query slot counts + cursors + long runs, run starts
    SB_MERGE_CL,                                    // the merge's clusters (hmk_merge.cpp): slot starts, members by slot, member -> slot
    SB_MERGE_LEN, SB_MERGE_MSTART,                  // ... row lengths in that order, their prefix sums
    SB_MERGE_TMP,                                   // ... per slot its feasible (slot, min score) records, at the slot's run offset
    SB_MERGE_CNT, SB_MERGE_OSTART, SB_MERGE_SCR, SB_MERGE_SCAN,   // ... feasible counts, their prefix sums, long-run list, scan scratch
    SB_LINK_TAB, SB_LINK_OUT,                       // the linkage inside given clusters (hmk_linkage.cpp): members by slot + work prefix sums; accumulators
    SB_SPLIT_SCORES,                                // the split of given clusters (hmk_split.cpp): the slots' dense triangles of int16 scores
    SB_CC_PARENT, SB_CC_SIZE,                       // connected components (hmk_components.cpp): the union-find's parent[n], members per root
    SB_CC_STATE, SB_CC_RUNS,                        // ... the levels' results, histogram and run offsets (CcState); the edges' (x, m) by level
    SB_ALIGN_SLOT, SB_ALIGN_MEMB,                   // the alignment of given clusters (hmk_align.cpp; tables in SB_LINK_TAB): per slot key, extent; per member sum, score, shift
    SB_SURVEY_ACC, SB_SURVEY_ROWS,                  // the score survey (hmk_survey.cpp): bins, counters, score range; per row key, best score, best index, degree
    SB_SEP_TAB, SB_SEP_REC, SB_SEP_OUT,             // the separation of given clusters (hmk_separation.cpp): partner order + slot tables; per (segment, member) records; per member outputs
    SB_SWEEP_RUNS, SB_SWEEP_STATE,                  // the greedy sweep (hmk_sweep.cpp): the pass's whole edges by level, the top level first; histogram, run offsets, prefixes, flag (SweepState)
    SB_REP_STATE, SB_REP_VERT, SB_REP_LIVE,         // the representatives (hmk_representatives.cpp): the level's counters (RepState); the per-vertex arrays (RepVertex); the two live-edge buffers
    SB_DEN_STATE, SB_DEN_VERT, SB_DEN_ROWS,         // density clustering (hmk_density.cpp): one record per level and the flag (DenState); the per-vertex arrays (DenVertex); the requested rows of a batch of levels
    SB_PROF_IN, SB_PROF_COLS, SB_PROF_OUT,          // the profile of given clusters (hmk_profile.cpp; tables in SB_LINK_TAB): tables and inputs per member and slot; per column ic, counts, flags; per member KLDs, per slot conserved count, first, last
    SB_SCAN_TRES, SB_SCAN_TOFF,                     // the scan along targets (hmk_scan.cpp): the targets' residues and offsets
    SB_SCAN_PLAN, SB_SCAN_TAB, SB_SCAN_SIZES,       // ... query list, runs and chunks of a call; the runs' tables; the sequences' sizes
    SB_SCAN_HITS, SB_SCAN_CNT,                      // ... the window hits; the pass's and the reduction's counters
    SB_SCAN_HASH, SB_SCAN_PAIRS, SB_SCAN_COV,       // ... pair mode's table of (pair, best window) and its records; the two coverage arrays
    SB_ORD_EDGES, SB_ORD_STATE, SB_ORD_POS,         // the greedy clusterings under many orders (hmk_orders.cpp): the pass's edges renamed into one order; sums, counters, flag (OrdersState); the order's inverse permutation
    SB_ORD_IDS, SB_ORD_SUPPORT, SB_ORD_PARTNERS,    // ... the valid orders' cluster ids, transposed; the support edges; partners ever [n], always [n]
    SB_N
};

// The library's environment switches (INTEGRATION.md lists them: every one is a test or diagnostic aid, none is needed for a
// result or for speed).  Read ONCE per entry-point call (refresh_switches, under the context's lock) -- never from a launch loop
// or a worker thread.
struct Switches {
    bool greedy_timing = false;   // HMK_GREEDY_TIMING: a clustering call's timeline, the plan's and the merge's phases on stderr
    bool no_band = false;         // HMK_NO_BAND: no band hand-over, phase 1 waits for the whole pass
    bool no_rows_kernel = false;  // HMK_NO_ROWS_KERNEL: the shift-packed tier (k_neighbors.hip) for every class
    int key_sort = 2;             // HMK_NO_KEY_SORT: 0, caller order and no key body; HMK_KEY_SORT_KEYS=1: the first key only (A/B runs)
    bool no_row_shared = false;   // HMK_NO_ROW_SHARED: no row group of a key-sorted plan takes the row-shared bodies (A/B runs)
    int key_row_pairs = -1;       // HMK_KEY_ROW_PAIRS=0|1: a key-sorted plan never / always takes 16-row tiles (-1: the planner's size rule)
    bool no_row_run_share = false;   // HMK_NO_ROW_RUN_SHARE: no 16-row tile's second group takes its merged cells from the first (A/B runs)
    bool no_tile_tables = false;  // HMK_NO_TILE_TABLES: every tile of a key-sorted plan builds its table in LDS, none copies the plan's (A/B runs)
    bool adj_8byte = false;       // HMK_ADJ_8BYTE: 8-byte adjacency entries even where 4 bytes hold every score
    bool local_literal = false;   // HMK_LOCAL_LITERAL: LocalAlignmentScorer through the literal DP
    bool local_signed = false;    // HMK_LOCAL_SIGNED: the signed tagged-max form (what gap_open = 0 runs) for every penalty
    bool local_no_pk = false;     // HMK_LOCAL_NO_PK: one column sequence per lane in the tagged-max DP
    bool multi_replicate = false; // HMK_MULTI_REPLICATE: a multi-device root copies the peers' finished adjacency pieces to itself instead of
                                  // reading them in place (what a machine without peer access between two of its devices runs)
    bool multi_force_copies = false;   // HMK_MULTI_FORCE_COPIES: contexts of one call that share a device exchange through copies and inboxes,
                                  // as distinct devices do (tests: the exchange's slot, offset and capacity arithmetic on one GPU)
    int second_loop = 0;          // HMK_SECOND_LOOP=device|host: 1 / 2 force that implementation of the second loop (0: the default choice)
    int phase1_threads = 0, phase1_window = 0;        // HMK_PHASE1_THREADS, HMK_PHASE1_WINDOW (GreedyOptions)
    int host_band_rows = 0, host_band_far_t = 0;      // HMK_PHASE1_HOST_BAND=rows[,far_t] (GreedyOptions)
    int loop_chain = -1;          // HMK_LOOP_CHAIN=0|1: chained joins never / from the first round (-1: from round 256 on)
    int loop_passes = 0;          // HMK_LOOP_PASSES: first/accept passes per round of the device-side loop (0: by cluster count)
    int precheck = 0;             // HMK_PRECHECK=two_passes|one_stage: 1 = count + fill passes, 2 = full-size tables for every row at once
    int late_buffers_delay_ms = 0;   // HMK_LATE_BUFFERS_DELAY_MS: hmk_reserve's buffer thread sleeps first (a host where device memory is slow to get)
    int csr_bucket_shift = 0;     // HMK_CSR_BUCKET_SHIFT: rows per bucket = 2^shift in the CSR's dealing pass (the wide buckets of n > 2^21)
    uint64_t edge_guess = 0;      // HMK_EDGE_GUESS: first edge-buffer capacity (forces the overflow / retry path)
    int test_grid_cap = 0;        // HMK_TEST_GRID_CAP=n, n >= 1: the grid-stride launches of hmk_grid.h get at most n workgroups (0: their own grids)
    int test_separation_segment = 0;   // HMK_TEST_SEPARATION_SEGMENT=n, n >= 1: the separation call's segments are n places long (0: sizing::separation_segments)
    bool no_scan_packed = false;  // HMK_NO_SCAN_PACKED: hmk_scan_shifted scores every class with the literal form (tests/test_scan.py)
    int profile_large_min = 0;    // HMK_PROFILE_LARGE_MIN=n, n >= 2: hmk_cluster_profile counts slots of n members or more in LDS (0: PROFILE_LARGE_MIN, hmk_profile.h)
    void read();
};

// the device copies every plan has (hmk_plan.cpp: upload_plan)
struct PlanArrays {
    uint8_t *d_res_sorted = nullptr;
    uint32_t *d_perm = nullptr;
    bool perm_identity = false;
    TileClass *d_classes = nullptr;
    Tile *d_tiles = nullptr;
};

struct Plan : PlanArrays {
    bool valid = false;
    int X = 0, p = 0, thr = 0;
    uint32_t part = 0, n_parts = 1;
    uint32_t band_rows = 0;   // tiles touching caller indices below this come first in every group (0: no band)
    int64_t band_req = 0;     // what the caller asked for (the plan may have had to drop the band)
    int lbmax = 12, lpad = 16;
    bool exact = false;       // the shift-packed length-12 kernel (k_neighbors_swar; only with HMK_NO_ROWS_KERNEL)
    bool rows_exact = false;  // one length for all and a row-packed instantiation for exactly that length
    bool no_rows_kernel = false;   // the switch this plan was built under (part of the cache key)
    int key_sort = 2;              // ... and this one: keys the plan sorts by (0: none; else rows_keyed shapes only)
    bool row_shared = true;        // ... and HMK_NO_ROW_SHARED (false: no tile is flagged row-shared)
    int key_row_pairs = -1;        // ... and HMK_KEY_ROW_PAIRS
    bool row_run_share = true;     // ... and HMK_NO_ROW_RUN_SHARE (false: no tile is flagged run-shared)
    bool tile_tables = true;       // ... and HMK_NO_TILE_TABLES (false: no tile is flagged ROWS_TILE_TABLE, the group records' tables stay unwritten)
    bool key_pairs = false;        // the plan is key-sorted with 16-row tiles: two row groups per column set-up (k_neighbors_rows.h)
    uint32_t paired_tiles = 0, run_shared_tiles = 0;   // tiles of a paired plan; those flagged ROWS_RUN_SHARED (hmk_neighbors_last_plan_shared)
    uint32_t table_tiles = 0;      // tiles flagged ROWS_TILE_TABLE, and the bytes of their tables inside d_keytab (hmk_neighbors_last_plan_tables)
    uint64_t table_bytes = 0;
    uint32_t *d_keyrun = nullptr;  // NeighborParams::keyrun / keytab (null: the plan is not key-sorted); keytab holds the tile tables too
    uint32_t *d_keytab = nullptr;
    uint32_t cols_per_tile = 16384;
    uint8_t *d_mb = nullptr;
    std::vector<Group> groups;
    hmk_neighbor_stats stats{};
    uint64_t band_pairs = 0;   // pairs inside the band tiles (of stats.pairs_scored)
    uint32_t q0 = 0, q1 = 0, r0 = 0, r1 = 0;   // a search plan (build_plan_search): its query and reference ranges
};

struct PlanLocal : PlanArrays {
    bool valid = false;
    uint32_t part = 0, n_parts = 1;
    bool triangle = false;   // unordered pairs only (a symmetric GlobalAlignmentScorer pass): classes la <= lb, column > row on la == lb
    uint32_t n_tiles = 0;
    uint64_t pairs = 0;
    uint32_t q0 = 0, q1 = 0, r0 = 0, r1 = 0;   // a search plan (build_plan_local_search): its query and reference ranges
};

} }  // namespace hmk::impl
using namespace hmk::impl;

struct hmk_ctx {
    int32_t M[HMK_ALPHABET * HMK_ALPHABET];
    bool symmetric = true;
    int min_m = 0, max_m = 0;
    int device = -1;
    bool has_device = false;
    int java_hashset = 8;   // hmk_set_java_hashset: whose HashSet iteration order clinkage emulates
    Switches sw;            // this call's environment switches (refresh_switches)

    uint32_t n = 0;
    std::vector<uint8_t> res;
    std::vector<uint32_t> off;
    std::vector<int32_t> sizes;
    bool has_sizes = false;
    // hmk_greedy_orders (hmk_orders.cpp): while one order's tail runs, Cluster.size() per row IN THAT ORDER -- what the tail reads
    // instead of `sizes` (tail_sizes below).  Null outside such a tail; `sizes` itself is never touched.
    const int32_t *sizes_view = nullptr;
    std::vector<uint8_t> len;
    int min_len = 0, max_len = 0;

    // hmk_set_targets: the second resident set (hmk_scan.cpp); the device copy (SB_SCAN_TRES / SB_SCAN_TOFF) is made at the first scan
    uint32_t n_targets = 0;
    std::vector<uint8_t> tres;
    std::vector<uint64_t> toff;
    bool targets_on_device = false;

    DevBuf d_res32, d_len;   // uint8: the probes' padded residues and lengths (ensure_res32)
    DevBuf d_M;              // int32: the matrix

    Plan plan;
    PlanLocal plan_local;
    PlanLocal plan_global;         // hmk_neighbors_global under a symmetric matrix: the triangle (every other global pass takes the local plans)
    Plan plan_search;              // the query-vs-reference searches' plans: cached apart from the all-vs-all ones, so that
    PlanLocal plan_local_search;   // searches and clustering calls on one context do not rebuild each other's
    Plan plan_assign;              // the assignments' plans (hmk_assign.cpp: members = the search's queries): cached apart too
    PlanLocal plan_local_assign;
    Plan plan_match;               // the cluster matches' plans (hmk_match.cpp: the assignment's rectangle): cached apart too
    PlanLocal plan_local_match;
    Plan plan_continue;            // hmk_greedy_continue (hmk_continue.cpp): members x new (a rectangle) and new x new (a triangle)
    Plan plan_continue_tri;
    Plan plan_merge;               // hmk_clinkage_merge / hmk_cluster_pairs_shifted (hmk_merge.cpp): the triangle inside the members' range
    EdgeBuffer edges;
    // side streams of the neighbour pass: the per-class launches of a mixed-length plan overlap their tails
    static constexpr int N_SIDE = 3;     // streams a mixed-length pass's launches are dealt to (hmk_pass.cpp)
    hipStream_t side[N_SIDE] = {nullptr};
    hipEvent_t ev_fork = nullptr, ev_join[N_SIDE] = {nullptr};
    hipStream_t copy_stream = nullptr;   // band CSR + device-to-host copies of adjacency rows (hmk_greedy_cluster)
    DevBuf d_rows_scratch;               // uint32: deg[n], cursor[n], misfit of hmk_pack_rows_dev

    double last_kernel_ms = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // greedy tail: own stream + events, grow-only device scratch, pinned host staging (all made once per context)
    hipStream_t gstream = nullptr;
    hipEvent_t ev_t0 = nullptr, ev_band = nullptr, ev_edges = nullptr, ev_csr = nullptr, ev_bandcsr = nullptr;
    DevBuf sb[SB_N];
    PinnedBuf h_start;   // uint64 start[n + 1], then uint32 up[n]
    PinnedBuf h_stage;   // what the merge uploads after phase 1 (cluster_of, sizes, leftovers, ...)
    PinnedBuf h_adj;     // adjacency rows fetched so far
    PinnedBuf h_merge;   // the cluster-level lists of hmk_merge.cpp (k_merge_compact stores them here)
    PinnedBuf h_split;   // the score triangles of hmk_split.cpp, copied back in one piece
    unsigned long long *h_loop = nullptr;    // pinned, coherent: progress word of the device-side second loop (written by k_loop_apply)
    unsigned long long *h_counts = nullptr;  // pinned: final segment counts [HMK_EDGE_SHARDS], band snapshot [HMK_EDGE_SHARDS], misc (HC_* below)
    hmk_greedy_phases phases{};

    // hmk_create_multi: this context is the root (devices[0]); one sub-context per further device, each with its own
    // copy of the sequences, its plan (shard d of n) and its edge buffer.  Empty for a single-device context.
    std::vector<hmk_ctx *> peers;
    // the stream this device's blocks travel to the other devices on (multi-device calls; a stream of this device)
    hipStream_t xfer_stream = nullptr;
    bool peer_loads_ok = true;   // (a peer:) the root's kernels may read this device's memory in place
    uint64_t inbox_entries = 0;  // entries per sender an overflowing block grew this device's inbox to (grow-only, like the buffer: the next call needs no retry)

    // hmk_reserve sizes the two buffers a clustering call needs LAST (adjacency, bucket records: 2 x 11 GB at 10^6) on its own
    // thread: on some hosts a fresh 11 GB of device memory takes 0.3-1.5 s to get, and a call has 0.27 s of scoring to do
    // before it writes to them.  Whoever touches SB_ADJ / SB_PART joins this first (ensure_buf does).
    std::future<hipError_t> late_buffers;

    bool wedged = false;   // a clustering call gave a stalled device up: nothing waits for it any more (calls fail with HMK_ERR_DEVICE)
    std::string err;
    mutable std::mutex mu;
};

namespace hmk { namespace impl {

extern thread_local std::string g_last_error;
int fail(hmk_ctx *ctx, int code, const std::string &msg);
// what a failed HIP call becomes: its status, and fail() with that status and "<what>: <HIP's text>"
inline int hip_status(hipError_t e) { return e == hipErrorOutOfMemory ? HMK_ERR_OOM : HMK_ERR_DEVICE; }
inline int fail_hip(hmk_ctx *ctx, const std::string &what, hipError_t e) { return fail(ctx, hip_status(e), what + ": " + hipGetErrorString(e)); }

#define HIPCHK(ctx, expr)                                        \
    do {                                                         \
        hipError_t e_ = (expr);                                  \
        if (e_ != hipSuccess) return fail_hip(ctx, #expr, e_);   \
    } while (0)

// a HIP call whose failure is not this call's business (teardown): the error must not stay behind as the thread's last one
#define HMK_QUIET(call) do { if ((call) != hipSuccess) (void)hipGetLastError(); } while (0)

// which: LAUNCH_ALL, or only the band tiles of the plan (LAUNCH_BAND: also zeroes the counts) / only the others
// (LAUNCH_REST: appends to the counts of the band launch).  A plan without a band (every search plan: Group::band = 0) launched with
// LAUNCH_REST runs ALL its tiles and appends to the counts already there (hmk_continue.cpp's second pass)
enum { LAUNCH_ALL = 0, LAUNCH_BAND = 1, LAUNCH_REST = 2 };

constexpr int ST_RETRY_OVERFLOW = 1000;   // internal: an edge segment overflowed, grow the buffer and score again
// layout of the small pinned block hmk_ctx::h_counts (64-bit words)
enum { HC_COUNTS = 0, HC_BAND = HMK_EDGE_SHARDS, HC_PEER = 2 * HMK_EDGE_SHARDS, HC_RANGE = HC_PEER + 32, HC_MISC = HC_RANGE + 8, HC_TOTAL = HC_MISC + 8, HC_WORDS = HC_TOTAL + 16 };

// (HMK_GREEDY_TIMING: what the grow-only buffers cost a call, i.e. the first call of a context)
extern thread_local double g_alloc_ms;
extern thread_local int g_allocs;
struct AllocTimer {
    const char *what;
    size_t bytes;
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    AllocTimer(const char *w, size_t b) : what(w), bytes(b) {}
    ~AllocTimer() {
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
        g_alloc_ms += ms;
        g_allocs++;
        static const bool timing = getenv("HMK_GREEDY_TIMING") != nullptr;   // (a destructor without a context: read once per process)
        if (timing && ms > 5.0) std::fprintf(stderr, "[hmk] %s of %.1f MB took %.1f ms\n", what, (double)bytes / 1048576.0, ms);
    }
};

// Where the edges of one greedy call are, and what is already known about them.  Everything the caller enqueued
// (scoring, snapshots) is on ctx->gstream; ev_edges has been recorded there after the last edge was written.
struct EdgeSource {
    EdgeSegs segs{};
    bool symmetric = true;
    bool check_overflow = false;       // segs are the HMK_EDGE_SHARDS segments of a neighbour pass: h_counts[0..16) receives
    uint64_t seg_cap = 0;              // their counts (copied on gstream before ev_edges); a count above seg_cap = overflow
    bool format_known = false;         // adjacency entry format decided without looking at the edges
    bool packed = false;
    int base = 0;
    uint64_t adj_bound = 0;            // upper bound of the adjacency entries (format_known only)
    uint64_t total_known = 0;          // exact number of edges, if known (else 0)
    uint32_t band_rows = 0;            // rows [0, band_rows) are complete in band_segs once ev_band has passed
    EdgeSegs band_segs{};
    bool deg_fused = false;            // the neighbour kernel counted the rows' degrees while it wrote the edges (SB_DEG, zeroed before the pass)
    bool deg_split = false;            // ... as upper counts [0, n) and lower counts [n, 2n) instead of totals
    // Multi-device calls: the adjacency is built in PIECES, piece d = the rows [d * rows_per, (d + 1) * rows_per) on device d, by that
    // device's worker (hmk_multi.cpp): `segs` is not used; before_full says when every piece's CSR has been built, precheck_pieces runs
    // the second loop's pre-check on every device for the leftovers whose rows it holds.
    struct Piece { hmk_ctx *c; uint32_t r0, r1; };
    std::vector<Piece> pieces;         // empty: one piece, the whole graph on this context
    uint32_t rows_per = 0;
    uint64_t total_edges = 0;          // (pieces: set by before_full) edges of all devices: the pieces' entries must add up to twice that
    std::function<bool(const struct PreIn &, unsigned long long *total)> precheck_pieces;   // -> every piece fits; *total = candidate entries
    hmk_clinkage_stats *clink = nullptr;   // non-null: run the clinkage nearest-neighbour chain instead of the greedy merge
    // multi-device calls: the peers' blocks arrive while the calling thread is already inside cluster_on_device.
    //   before_band  blocks until every peer's band block is on its way to the root and makes the copy stream wait for them;
    //                non-zero: no band hand-over in this call (phase 1 then waits for the full graph)
    //   before_full  blocks until every device's piece of the adjacency is complete (its size in the device's h_counts[HC_TOTAL]);
    //                HMK_OK, ST_RETRY_OVERFLOW or an error code (the text is in the context)
    std::function<int()> before_band, before_full;
};

// The source of one segment: the first `total` entries of `edges`, d_count = that number in device memory (a buffer without an edge:
// a count of 0 in a segment of room 1).  packed: null, or -- where the caller knows the adjacency format without looking at the
// edges -- whether an entry fits 4 bytes over `base`.
inline EdgeSource one_segment_source(const uint64_t *edges, const unsigned long long *d_count, uint64_t total, bool symmetric,
                                     const bool *packed = nullptr, int base = 0) {
    EdgeSource src;
    src.symmetric = symmetric;
    src.segs.n = 1;
    src.segs.s[0] = EdgeSeg{edges, d_count, std::max<uint64_t>(total, 1)};
    src.total_known = total;
    if (packed) {
        src.format_known = true;
        src.packed = *packed;
        src.base = base;
        src.adj_bound = (symmetric ? 2 : 1) * total;
    }
    return src;
}

// Two events that time a stretch of a stream, destroyed with the pair.
struct EventPair {
    hipEvent_t a = nullptr, b = nullptr;
    EventPair() = default;
    EventPair(const EventPair &) = delete;
    EventPair &operator=(const EventPair &) = delete;
    ~EventPair() {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
    }
    hipError_t create() {
        const hipError_t e = hipEventCreate(&a);
        return e == hipSuccess ? hipEventCreate(&b) : e;
    }
    hipError_t start(hipStream_t s) { return hipEventRecord(a, s); }
    hipError_t stop(hipStream_t s) { return hipEventRecord(b, s); }
    hipError_t elapsed(float *ms) const { return hipEventElapsedTime(ms, a, b); }   // (once b has passed)
};

// Cluster.size() per row as the clustering tail reads it: the context's sizes, or the permuted view of the order whose tail is
// running (hmk_ctx::sizes_view); null: every sequence counts once
inline const int32_t *tail_sizes(const hmk_ctx *ctx) { return ctx->sizes_view ? ctx->sizes_view : ctx->has_sizes ? ctx->sizes.data() : nullptr; }
// ---- hmk_common.cpp
void refresh_switches(hmk_ctx *ctx);              // the root's and its peers' (under the context's lock, once per entry-point call)
GreedyOptions greedy_options(const hmk_ctx *ctx);
int need_device(hmk_ctx *ctx);
int ensure_res32(hmk_ctx *ctx);
hipError_t ensure_buf_now(hmk_ctx *ctx, int which, size_t bytes);
bool late_buffers_pending(hmk_ctx *ctx);
hipError_t join_late_buffers(hmk_ctx *ctx);
hipError_t ensure_buf(hmk_ctx *ctx, int which, size_t bytes);
template <class T> T *buf(hmk_ctx *ctx, int which) { return (T *)ctx->sb[which].p; }
int greedy_streams(hmk_ctx *ctx);   // streams, events and pinned blocks of the clustering calls
bool csr_by_bucket(bool symmetric, bool packed);
// The CSR and pre-check buffers of one piece of the adjacency on c's device: a single device's whole graph, or a multi-device call's
// piece.  Entries of the adjacency = (symmetric ? 2 : 1) * adj_records; 0 records: that buffer is sized elsewhere (hmk_reserve's thread).
hipError_t ensure_piece_buffers(hmk_ctx *c, uint32_t n, bool packed, bool symmetric, uint64_t adj_records, uint64_t bucket_records);
int reserve_tail_buffers(hmk_ctx *ctx, uint32_t n, bool packed, uint32_t r1, bool full = false, bool late_on_a_thread = false);
// whether this context's adjacency entries fit 4 bytes at these parameters (sizing::adjacency_packed)
inline bool adjacency_packed(const hmk_ctx *ctx, int max_shift, int shift_penalty, int threshold) {
    return sizing::adjacency_packed(ctx->max_len, ctx->min_len, ctx->max_m, shift_penalty, max_shift, threshold, ctx->sw.adj_8byte);
}
// ---- hmk_plan.cpp
void free_plan(Plan &pl);
void free_plan_local(PlanLocal &pl);
void free_plans(hmk_ctx *ctx);   // every plan slot of the context
void classify(const hmk_ctx *ctx, int la, int lb, int X, int p, int thr, TileClass *out, long long row_bound = -1,
              long long *u8_row_limit = nullptr);
// key_sort_ok: a plain single-part pass (no band, no degree counters) that may take the key-sorted order
int build_plan(hmk_ctx *ctx, int X, int p, int thr, uint32_t part, uint32_t n_parts, int64_t band_rows = -1, bool key_sort_ok = false);
// all ordered pairs of the set (LocalAlignmentScorer; GlobalAlignmentScorer under an asymmetric matrix), or (triangle) every
// unordered pair once, into the plan slot `pl`
int build_plan_local(hmk_ctx *ctx, PlanLocal &pl, uint32_t part, uint32_t n_parts, bool triangle = false);
// the rectangle queries [q0, q1) x references [r0, r1) (disjoint, non-empty) into the plan slot `pl` (the search's, the
// assignment's, ... own)
int build_plan_search(hmk_ctx *ctx, Plan &pl, int X, int p, int thr, uint32_t q0, uint32_t q1, uint32_t r0, uint32_t r1);
int build_plan_local_search(hmk_ctx *ctx, PlanLocal &pl, uint32_t q0, uint32_t q1, uint32_t r0, uint32_t r1);
// the triangle of the pairs inside [q0, q1) (symmetric matrices; hmk_continue.cpp's new x new) into the plan slot `pl`
int build_plan_triangle(hmk_ctx *ctx, Plan &pl, int X, int p, int thr, uint32_t q0, uint32_t q1);
// the parameter checks of a shifted rectangle (the shift against both ranges, threshold and int16 limits)
int check_shifted(hmk_ctx *ctx, int X, int p, int thr, uint32_t q0, uint32_t q1, uint32_t r0, uint32_t r1);
// ---- hmk_assign.cpp
// the clusters' argument checks of the assignment and the continuation (`what` names the call in the range message):
// members[c] = slot c's members, size[c] = its Cluster.size()
int check_clusters(hmk_ctx *ctx, const char *what, uint32_t q0, uint32_t q1, uint32_t r0, uint32_t r1, const uint32_t *member_cluster,
                   const int32_t *cluster_id, uint32_t n_clusters, std::vector<uint32_t> &members, std::vector<int64_t> &size);
// The host's order of the clusters: size() descending, then cluster_id ascending -- the tie-breaks of the ranking after the
// score.  rank_of[slot], slot_of_rank[rank], members_of_rank[rank].
struct ClusterOrder {
    std::vector<uint32_t> rank_of, slot_of_rank, members_of_rank;
};
// the assignment's argument checks (k, then check_clusters) before the device is looked at (a host-only context answers them
// too); fills `order`.  hmk_match.cpp makes them too.
int check_assign(hmk_ctx *ctx, const char *what, uint32_t q0, uint32_t q1, uint32_t r0, uint32_t r1, const uint32_t *member_cluster,
                 const int32_t *cluster_id, uint32_t n_clusters, uint32_t k, ClusterOrder *order);
// the pass of the rectangle members [r0, r1) x new [q0, q1) into ctx->edges in the plan slot pl (shifted) / pll (local: `local`),
// with the members as the search's queries (seq1); -> the shards' counts, their total; *S = the pass's stats (symmetric kept
// for the local scorer), kernel_ms = the pass
int cluster_pass(hmk_ctx *ctx, bool local, Plan &pl, PlanLocal &pll, int a, int b, int thr, uint32_t q0, uint32_t q1, uint32_t r0, uint32_t r1,
                 unsigned long long counts[HMK_EDGE_SHARDS], uint64_t *total, hmk_neighbor_stats *S);
// ---- hmk_pass.cpp
int neighbors_dev_locked(hmk_ctx *ctx, int X, int p, int thr, uint32_t part, uint32_t n_parts, void *d_edges,
                         uint64_t capacity, void *d_counts, hipStream_t stream, int which = LAUNCH_ALL,
                         int64_t band_rows = -1, uint32_t *d_deg = nullptr, uint32_t *d_deg_lo = nullptr);
int launch_plan(hmk_ctx *ctx, const Plan &pl, int X, int p, int thr, void *d_edges, uint64_t capacity, void *d_counts,
                hipStream_t stream, int which = LAUNCH_ALL, uint32_t *d_deg = nullptr, uint32_t *d_deg_lo = nullptr);
bool local_enc(const hmk_ctx *ctx, int gap_open, int gap_extend);
bool local_literal(const hmk_ctx *ctx, int gap_open, int gap_extend);
int check_local_fits(hmk_ctx *ctx, int gap_open, int gap_extend, int thr);
// the gapped scorers of the PlanLocal passes (launch_pairs' numbering)
enum { SCORER_LOCAL = 1, SCORER_GLOBAL = 2 };
// GlobalAlignmentScorer's argument checks (made before the device is looked at): -127 <= gap_open <= gap_extend <= 0, the
// threshold within [-30000, 30000], 32 * max(0, max M) <= 32767
int check_global_fits(hmk_ctx *ctx, int gap_open, int gap_extend, int thr);
int launch_plan_local(hmk_ctx *ctx, const PlanLocal &pl, int scorer, int gap_open, int gap_extend, int thr, uint64_t *d_edges, uint64_t capacity,
                      unsigned long long *d_counts, hipStream_t stream);
int neighbors_internal(hmk_ctx *ctx, int X, int p, int thr, uint32_t part, uint32_t n_parts, uint64_t want_cap,
                       unsigned long long counts[HMK_EDGE_SHARDS], double *kernel_ms);
int neighbors_local_dev_locked(hmk_ctx *ctx, int gap_open, int gap_extend, int thr, uint32_t part, uint32_t n_parts,
                               uint64_t *d_edges, uint64_t capacity, unsigned long long *d_counts, hipStream_t stream);
void timer_start(hmk_ctx *ctx);
void timer_stop(hmk_ctx *ctx);
int check_pairs(hmk_ctx *ctx, const uint32_t *i, const uint32_t *j, uint64_t n_pairs, bool shifted, int X);
int score_pairs(hmk_ctx *ctx, int scorer, const uint32_t *i, const uint32_t *j, uint64_t n_pairs, int a, int b,
                int32_t *out, int32_t *out_shift = nullptr);
int score_block(hmk_ctx *ctx, int scorer, uint32_t r0, uint32_t r1, uint32_t c0, uint32_t c1, int a, int b,
                int32_t *out);
// ---- hmk_cluster.cpp
// What the second loop's pre-check needs of the host (pinned, read-only while the pieces run): cluster_of | usize | leftover in one block
struct PreIn {
    uint32_t n = 0, nl = 0, ncl = 0;
    bool packed = true;
    const char *h_block = nullptr;       // pinned: cluster_of int32[n], usize int32[ncl], leftover uint32[nl]
    size_t b_cof = 0, b_us = 0, b_left = 0;
    unsigned long long region_cap = 0;   // entries per region of the candidate buffer (HMK_PRE_REGIONS regions)
    int first_slots = 128;               // table size of the first stage
    bool two_stage = true;
};
// CSR of the rows [r0, r1) from `segs` on c's device, enqueued on q (counts or the fused counters, scan, scatter); records c->ev_csr;
// the piece's entry count lands in c->h_counts[HC_TOTAL], the score range / invalid edges in c->h_counts + HC_RANGE
hipError_t piece_enqueue_csr(hmk_ctx *c, const EdgeSegs &segs, bool symmetric, bool packed, int base, uint32_t n, uint32_t r0, uint32_t r1,
                             bool deg_fused, bool deg_split, hipStream_t q);
// the pre-check of one piece (k_greedy_precheck, single pass with region counters): upload on c's copy stream, kernels on q behind the piece's
// CSR, counters back, q synchronised.  -> 0: fits (entries in *total), 1: a region overran (count + fill passes needed), -1: failed / a row
// overflowed its tables (the host's pre-check)
int piece_precheck(hmk_ctx *c, const PreIn &in, uint32_t r0, uint32_t r1, uint32_t region_base, uint32_t region_count, hipStream_t q,
                   bool upload, unsigned long long *total);
hipError_t piece_precheck_upload(hmk_ctx *c, const PreIn &in);   // (the upload alone, on c's copy stream: records c->ev_bandcsr)
// What the device-side second loop needs besides the pre-check's candidate lists and the uploaded leftover list (SB_LEFT)
struct LoopIn {
    uint32_t n = 0, nl = 0, ncl = 0;
    uint32_t cand_total = 0;                          // candidate entries (< 2^31)
    bool packed = true;                               // the CSR's entry format
    const std::vector<int64_t> *csize = nullptr;      // Cluster.size() per slot
    const std::vector<int32_t> *cids = nullptr;       // Java id per slot
    const std::vector<EdgeSource::Piece> *pieces = nullptr;   // where the joiners' rows live (one piece: this context's CSR)
    uint32_t rows_per = 0;                            // (several pieces: rows per piece)
};
// The rounds of k_loop_* on S until one joins nobody: join_slot[q] = the slot leftover q joins or -1.  false: did not run to the
// end (the caller falls back); *stall_err is set when the device stalled and the context was given up (ctx->wedged).
bool device_second_loop(hmk_ctx *ctx, hipStream_t S, const LoopIn &in, std::vector<int32_t> &join_slot, uint32_t *rounds,
                        std::string *stall_err);
int cluster_on_device(hmk_ctx *ctx, const EdgeSource &src, int max_clusters, int32_t *cluster_id, int32_t *result_order,
                      int32_t *member_rank, hmk_greedy_stats *stats, std::chrono::steady_clock::time_point t0);
// the bodies of hmk_greedy_cluster / hmk_clinkage_cluster on one device, behind the entry points' argument checks (t_entry: the call's
// start, for HMK_GREEDY_TIMING)
int greedy_cluster_single(hmk_ctx *ctx, int max_shift, int shift_penalty, int threshold, int max_clusters, int32_t *cluster_id,
                          int32_t *result_order, int32_t *member_rank, hmk_greedy_stats *stats, std::chrono::steady_clock::time_point t_entry);
int clinkage_cluster_single(hmk_ctx *ctx, int max_shift, int shift_penalty, int threshold, int32_t *cluster_id, int32_t *result_order,
                            int32_t *member_rank, hmk_clinkage_stats *stats);
// ---- hmk_multi.cpp (the same two on a context of several devices)
int greedy_cluster_multi(hmk_ctx *ctx, int max_shift, int shift_penalty, int threshold, int max_clusters, int32_t *cluster_id,
                         int32_t *result_order, int32_t *member_rank, hmk_greedy_stats *stats, hmk_clinkage_stats *clink = nullptr);

// A pass into the context's edge buffer, grown until every segment fits: reserve, launch, time, read the counts, check the fit.
template <typename LaunchFn>
int neighbors_grow(hmk_ctx *ctx, uint64_t want_cap, unsigned long long counts[HMK_EDGE_SHARDS], double *kernel_ms,
                   LaunchFn launch) {
    int st = need_device(ctx);
    if (st) return st;
    uint64_t cap = std::max<uint64_t>(want_cap, (uint64_t)1 << 20);
    cap = (cap + HMK_EDGE_SHARDS - 1) / HMK_EDGE_SHARDS * HMK_EDGE_SHARDS;
    EventPair ev;
    HIPCHK(ctx, ev.create());
    auto attempt = [&]() -> int {
        int r = ctx->edges.reserve(ctx, cap);
        if (r) return r;
        HIPCHK(ctx, ev.start(nullptr));
        r = launch(ctx->edges.d, ctx->edges.cap, ctx->edges.counts);
        if (r) return r;
        HIPCHK(ctx, ev.stop(nullptr));
        HIPCHK(ctx, hipEventSynchronize(ev.b));
        float ms = 0;
        HIPCHK(ctx, ev.elapsed(&ms));
        if (kernel_ms) *kernel_ms = ms;
        HIPCHK(ctx, hipMemcpy(counts, ctx->edges.counts, HMK_EDGE_SHARDS * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        if (max_of(counts) <= ctx->edges.seg_cap()) return HMK_OK;
        cap = sizing::edge_capacity_after_overflow(max_of(counts));   // a segment overflowed: grow and rescore
        if (ctx->sw.greedy_timing)
            std::fprintf(stderr, "[hmk] an edge segment overflowed (%llu entries for %llu): %llu entries next, scoring again\n",
                         (unsigned long long)max_of(counts), (unsigned long long)ctx->edges.seg_cap(), (unsigned long long)cap);
        return ST_RETRY_OVERFLOW;
    };
    st = ST_RETRY_OVERFLOW;
    for (int k = 0; k < 4 && st == ST_RETRY_OVERFLOW; k++) st = attempt();
    if (st == ST_RETRY_OVERFLOW) return fail(ctx, HMK_ERR_DEVICE, "internal edge buffer kept overflowing");
    return st;
}

} }  // namespace hmk::impl
#endif
