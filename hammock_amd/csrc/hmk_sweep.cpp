// hmk_sweep.cpp -- the greedy clusterings at every threshold of a range from ONE scoring pass (hmk_greedy_sweep*).
// Replaces one LimitedGreedySequenceClusterer(scorer, t, maxClusters).cluster(sequences) per threshold t
// (LimitedGreedySequenceClusterer.java:22,39-69), each of which scores the whole pair space again.
//   pass      hmk_neighbors_shifted's (neighbors_internal: the all-vs-all plan slot, the same kernels) at `threshold` into the context's
//             edge buffer, grown until it fits;
//   deal      k_sweep_hist, k_sweep_scan, k_sweep_deal: the whole edges in one run per level min(score, threshold_hi) - threshold,
//             the top level first (SB_SWEEP_RUNS), so that the edges with score >= t are the prefix [0, prefix[t - threshold]);
//             no host synchronisation between the three, prefix[] and the flag come back in one copy;
//   tails     per level the clustering tail as it is (cluster_on_device) on an EdgeSource of one segment: that prefix.
// hmk_greedy_sweep_from_edges is the same answer on the host: the edges sorted by level by counting, hmk_greedy_from_edges's merge per
// prefix -- the second implementation the device path is tested against, and what a host-only context runs.
#include "hmk_ctx.h"
#include "hmk_sweep.h"

namespace hmk { namespace impl {

namespace {

struct SweepOut {
    int32_t *cluster_id, *result_order, *member_rank;   // each [n_levels][n] or null
    hmk_greedy_level *levels;
    hmk_greedy_sweep_stats *stats;
};

// the argument checks all three entry points make before the device is looked at
int check_sweep(hmk_ctx *ctx, int thr, int thr_hi, const SweepOut &o) {
    if (thr_hi < thr) return fail(ctx, HMK_ERR_BAD_ARG, "threshold_hi is below threshold");
    if ((long long)thr_hi - thr > (long long)SWEEP_MAX_LEVELS - 1) return fail(ctx, HMK_ERR_BAD_ARG, "at most 256 levels per call: threshold_hi - threshold <= 255");
    if (thr_hi > 32767) return fail(ctx, HMK_ERR_BAD_ARG, "threshold_hi is above 32767, the highest score an edge holds");
    if (ctx->n && !o.levels && !o.cluster_id && !o.result_order && !o.member_rank)
        return fail(ctx, HMK_ERR_BAD_ARG, "null outputs (levels, cluster_id, result_order and member_rank)");
    return HMK_OK;
}

// no sequences: cluster() of an empty list returns an empty list at every threshold
int empty_set(uint32_t nl, const SweepOut &o) {
    if (o.levels) std::fill(o.levels, o.levels + nl, hmk_greedy_level{});
    if (o.stats) {
        *o.stats = hmk_greedy_sweep_stats{};
        o.stats->n_levels = nl;
    }
    return HMK_OK;
}

// One level's outputs behind its clustering: st = what the clustering returned (HMK_OK or HMK_ERR_REFERENCE_WOULD_CRASH), ids = its
// cluster ids (the caller's row or the call's scratch).  A level where the reference would throw keeps the failure and -1 rows.
void finish_level(uint32_t n, uint32_t l, const SweepOut &o, int st, const hmk_greedy_stats &gs, uint64_t n_edges, const int32_t *ids, double ms,
                  std::vector<uint32_t> &members) {
    const bool crash = st == HMK_ERR_REFERENCE_WOULD_CRASH;
    if (crash)
        for (int32_t *rows : {o.cluster_id, o.result_order, o.member_rank})
            if (rows) std::fill(rows + (size_t)l * n, rows + (size_t)(l + 1) * n, -1);
    if (!o.levels) return;
    hmk_greedy_level &L = o.levels[l];
    L = hmk_greedy_level{};
    L.n_edges = n_edges;
    L.status = st;
    L.crash_case = gs.crash_case;
    L.crash_index = gs.crash_index;
    L.phase1_stop_index = gs.phase1_stop_index;
    L.phase1_clusters = gs.phase1_clusters;
    L.phase1_orphans = gs.phase1_orphans;
    L.n_result_clusters = gs.n_result_clusters;
    L.n_multi = gs.n_multi;
    L.tail_ms = ms;
    if (crash) return;
    members.assign(n, 0);   // a cluster's id is its seed's index
    for (uint32_t k = 0; k < n; k++)
        if ((uint32_t)ids[k] < n) members[(uint32_t)ids[k]]++;
    for (uint32_t c = 0; c < n; c++) {
        L.n_singletons += members[c] == 1;
        L.largest = std::max(L.largest, members[c]);
    }
}

// a level's rows before its clustering writes them: what a clustering leaves alone (result_order behind the returned clusters) is -1
int32_t *level_row(int32_t *rows, uint32_t l, uint32_t n) {
    if (!rows) return nullptr;
    std::fill(rows + (size_t)l * n, rows + (size_t)(l + 1) * n, -1);
    return rows + (size_t)l * n;
}

void set_runs(SweepEdges &E, const uint64_t *base, uint64_t stride, uint32_t n_runs, const unsigned long long *count) {
    E = SweepEdges{};
    E.base = base;
    E.stride = stride;
    E.n_runs = n_runs;
    for (uint32_t s = 0; s < n_runs; s++) {
        E.count[s] = count[s];
        E.chunk_start[s + 1] = E.chunk_start[s] + (uint32_t)((count[s] + SWEEP_CHUNK - 1) / SWEEP_CHUNK);
    }
}

// The device side behind the edges: E names them (packed, on this context's device), total = their number.  X, p: the scoring
// parameters the adjacency format follows from (scored = true), else the tail reads the format off each level's scores.
int sweep_on_device(hmk_ctx *ctx, const SweepEdges &E, uint64_t total, bool symmetric, bool scored, int X, int p, int thr, int thr_hi, int max_clusters,
                    const SweepOut &o, hmk_greedy_sweep_stats &S) {
    const uint32_t n = ctx->n, nl = (uint32_t)(thr_hi - thr) + 1;
    int st = greedy_streams(ctx);
    if (st) return st;
    hipStream_t Q = ctx->gstream;
    HIPCHK(ctx, ensure_buf(ctx, SB_SWEEP_STATE, sizeof(SweepState)));
    HIPCHK(ctx, ensure_buf(ctx, SB_SWEEP_RUNS, std::max<uint64_t>(total, 1) * sizeof(uint64_t)));
    SweepState *state = buf<SweepState>(ctx, SB_SWEEP_STATE);
    uint64_t *dealt = buf<uint64_t>(ctx, SB_SWEEP_RUNS);
    struct { unsigned long long prefix[SWEEP_MAX_LEVELS], flag; } back;
    static_assert(offsetof(SweepState, flag) == offsetof(SweepState, prefix) + sizeof(back.prefix), "prefix and flag are read in one copy");
    hipEvent_t e0 = nullptr, e1 = nullptr;
    HIPCHK(ctx, hipEventCreate(&e0));
    hipError_t e = hipEventCreate(&e1);
    if (e == hipSuccess) e = hipEventRecord(e0, Q);
    if (e == hipSuccess) e = hipMemsetAsync(state, 0, sizeof(SweepState), Q);
    if (e == hipSuccess) e = launch_sweep_hist(E, n, thr, thr_hi, state, Q);
    if (e == hipSuccess) e = launch_sweep_scan(nl, state, Q);
    if (e == hipSuccess) e = launch_sweep_deal(E, n, thr, thr_hi, state, dealt, Q);
    if (e == hipSuccess) e = hipEventRecord(e1, Q);
    if (e == hipSuccess) e = hipMemcpyAsync(&back, state->prefix, sizeof(back), hipMemcpyDeviceToHost, Q);
    if (e == hipSuccess) e = hipStreamSynchronize(Q);
    float ms = 0;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (e != hipSuccess) return fail(ctx, e == hipErrorOutOfMemory ? HMK_ERR_OOM : HMK_ERR_DEVICE, std::string("greedy sweep: ") + hipGetErrorString(e));
    if (back.flag) return fail(ctx, HMK_ERR_BAD_ARG, "edge list references a sequence outside [0, n) or a self pair");
    if (back.prefix[0] > total) return fail(ctx, HMK_ERR_DEVICE, "greedy sweep: more edges dealt than given");
    S.deal_ms = ms;
    S.n_edges = back.prefix[0];
    S.n_levels = nl;
    // the tails, from the top level (the shortest prefix) down: each takes the first prefix[l] entries of the dealt buffer as one
    // segment whose count is prefix[l] itself, in device memory
    std::vector<int32_t> ids(o.cluster_id ? 0 : n);
    std::vector<uint32_t> members;
    for (uint32_t l = nl; l-- > 0;) {
        const auto t0 = std::chrono::steady_clock::now();
        const int t = thr + (int)l;
        const uint64_t m = back.prefix[l];
        EdgeSource src;
        src.symmetric = symmetric;
        src.segs.n = 1;
        src.segs.s[0] = EdgeSeg{dealt, &state->prefix[l], std::max<uint64_t>(m, 1)};   // (a level without an edge: a count of 0 in a segment of room 1)
        src.total_known = m;
        if (scored) {
            src.format_known = true;
            src.packed = adjacency_packed(ctx, X, p, t);
            src.base = t;
            src.adj_bound = (symmetric ? 2 : 1) * m;
        }
        ctx->phases = hmk_greedy_phases{};
        HIPCHK(ctx, hipEventRecord(ctx->ev_t0, Q));
        HIPCHK(ctx, hipEventRecord(ctx->ev_edges, Q));
        hmk_greedy_stats gs{};
        int32_t *cid = o.cluster_id ? level_row(o.cluster_id, l, n) : ids.data();
        st = cluster_on_device(ctx, src, max_clusters, cid, level_row(o.result_order, l, n), level_row(o.member_rank, l, n), &gs, t0);
        if (st == ST_RETRY_OVERFLOW) return fail(ctx, HMK_ERR_DEVICE, "greedy sweep: a level's segment overflowed");
        if (st != HMK_OK && st != HMK_ERR_REFERENCE_WOULD_CRASH) return st;
        finish_level(n, l, o, st, gs, m, cid, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(), members);
    }
    return HMK_OK;
}

int greedy_sweep(hmk_ctx *ctx, int X, int p, int thr, int thr_hi, int max_clusters, const SweepOut &o) {
    if (!ctx) return fail(nullptr, HMK_ERR_BAD_ARG, "null context");
    std::lock_guard<std::mutex> lock(ctx->mu);
    refresh_switches(ctx);
    int st = check_sweep(ctx, thr, thr_hi, o);
    if (st) return st;
    const uint32_t n = ctx->n, nl = (uint32_t)(thr_hi - thr) + 1;
    if (n == 0) return empty_set(nl, o);
    st = need_device(ctx);
    if (st) return st;
    hmk_greedy_sweep_stats S{};
    unsigned long long counts[HMK_EDGE_SHARDS];
    double ms = 0;
    st = neighbors_internal(ctx, X, p, thr, 0, 1, sizing::edge_capacity_guess(ctx->symmetric, n, 1, ctx->sw.edge_guess, ctx->edges.cap), counts, &ms);
    if (st) return st;
    S.kernel_ms = ms;
    S.pairs_scored = ctx->plan.stats.pairs_scored;
    SweepEdges E;
    set_runs(E, ctx->edges.d, ctx->edges.seg_cap(), HMK_EDGE_SHARDS, counts);
    st = sweep_on_device(ctx, E, total_of(counts), ctx->symmetric, true, X, p, thr, thr_hi, max_clusters, o, S);
    if (st == HMK_OK && o.stats) *o.stats = S;
    return st;
}

int greedy_sweep_from_edges_dev(hmk_ctx *ctx, const void *d_edges, uint64_t n_edges, bool symmetric, int thr, int thr_hi, int max_clusters,
                                const SweepOut &o) {
    if (!ctx) return fail(nullptr, HMK_ERR_BAD_ARG, "null context");
    std::lock_guard<std::mutex> lock(ctx->mu);
    refresh_switches(ctx);
    int st = check_sweep(ctx, thr, thr_hi, o);
    if (st) return st;
    if (n_edges && !d_edges) return fail(ctx, HMK_ERR_BAD_ARG, "null edge buffer");
    if (n_edges > ((uint64_t)1 << 41)) return fail(ctx, HMK_ERR_BAD_ARG, "more than 2^41 edges");   // (chunks are counted in 32 bits)
    const uint32_t nl = (uint32_t)(thr_hi - thr) + 1;
    if (ctx->n == 0) return empty_set(nl, o);
    st = need_device(ctx);
    if (st) return st;
    // the caller's block may have been written on any stream of its own: wait for the device
    HIPCHK(ctx, hipDeviceSynchronize());
    hmk_greedy_sweep_stats S{};
    SweepEdges E;
    const unsigned long long cnt = n_edges;
    set_runs(E, (const uint64_t *)d_edges, 0, 1, &cnt);
    st = sweep_on_device(ctx, E, n_edges, symmetric, false, 0, 0, thr, thr_hi, max_clusters, o, S);
    if (st == HMK_OK && o.stats) *o.stats = S;
    return st;
}

// The edges sorted by level, descending, by counting; hmk_greedy_from_edges's merge on every prefix.
int greedy_sweep_from_edges(hmk_ctx *ctx, const uint64_t *edges, uint64_t n_edges, bool symmetric, int thr, int thr_hi, int max_clusters,
                            const SweepOut &o) {
    if (!ctx) return fail(nullptr, HMK_ERR_BAD_ARG, "null context");
    std::lock_guard<std::mutex> lock(ctx->mu);
    refresh_switches(ctx);
    int st = check_sweep(ctx, thr, thr_hi, o);
    if (st) return st;
    if (n_edges && !edges) return fail(ctx, HMK_ERR_BAD_ARG, "null edge list");
    const uint32_t n = ctx->n, nl = (uint32_t)(thr_hi - thr) + 1;
    if (n == 0) return empty_set(nl, o);
    std::vector<uint64_t> start((size_t)nl + 1, 0);   // runs by level, the highest level first: run of level l at start[nl - 1 - l]
    // (in 64 bits: `threshold` is any int here, and score - threshold must not wrap for an edge far below it)
    auto level_of = [&](uint64_t e) -> long long { return (long long)std::min((int)HMK_EDGE_SCORE(e), thr_hi) - thr; };
    for (uint64_t k = 0; k < n_edges; k++) {
        const uint32_t x = HMK_EDGE_X(edges[k]), m = HMK_EDGE_M(edges[k]);
        if (x >= n || m >= n || x == m) return fail(ctx, HMK_ERR_BAD_ARG, "edge list references a sequence outside [0, n) or a self pair");
        const long long l = level_of(edges[k]);
        if (l >= 0) start[nl - (uint32_t)l]++;
    }
    for (uint32_t r = 0; r < nl; r++) start[r + 1] += start[r];
    std::vector<uint64_t> sorted(start[nl]);
    {
        std::vector<uint64_t> at(start.begin(), start.end() - 1);
        for (uint64_t k = 0; k < n_edges; k++) {
            const long long l = level_of(edges[k]);
            if (l >= 0) sorted[at[nl - 1 - (uint32_t)l]++] = edges[k];
        }
    }
    std::vector<int32_t> ids(o.cluster_id ? 0 : n);
    std::vector<uint32_t> members;
    const GreedyOptions opt = greedy_options(ctx);
    for (uint32_t l = nl; l-- > 0;) {
        const auto t0 = std::chrono::steady_clock::now();
        const uint64_t m = start[nl - l];   // the edges of the levels >= l
        hmk_greedy_stats gs{};
        std::string err;
        int32_t *cid = o.cluster_id ? level_row(o.cluster_id, l, n) : ids.data();
        st = greedy_from_edges(n, ctx->has_sizes ? ctx->sizes.data() : nullptr, sorted.data(), m, symmetric, thr + (int)l, max_clusters, cid,
                               level_row(o.result_order, l, n), level_row(o.member_rank, l, n), &gs, &err, opt);
        if (st != HMK_OK && st != HMK_ERR_REFERENCE_WOULD_CRASH) return fail(ctx, st, err);
        finish_level(n, l, o, st, gs, m, cid, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(), members);
    }
    if (o.stats) {
        *o.stats = hmk_greedy_sweep_stats{};
        o.stats->n_edges = start[nl];
        o.stats->n_levels = nl;
    }
    return HMK_OK;
}

}  // namespace

} }  // namespace hmk::impl

extern "C" {

int hmk_greedy_sweep(hmk_ctx *ctx, int max_shift, int shift_penalty, int threshold, int threshold_hi, int max_clusters, int32_t *cluster_id,
                     int32_t *result_order, int32_t *member_rank, hmk_greedy_level *levels, hmk_greedy_sweep_stats *stats) {
    return greedy_sweep(ctx, max_shift, shift_penalty, threshold, threshold_hi, max_clusters, SweepOut{cluster_id, result_order, member_rank, levels, stats});
}

int hmk_greedy_sweep_from_edges(hmk_ctx *ctx, const uint64_t *edges, uint64_t n_edges, int symmetric, int threshold, int threshold_hi,
                                int max_clusters, int32_t *cluster_id, int32_t *result_order, int32_t *member_rank, hmk_greedy_level *levels,
                                hmk_greedy_sweep_stats *stats) {
    return greedy_sweep_from_edges(ctx, edges, n_edges, symmetric != 0, threshold, threshold_hi, max_clusters,
                                   SweepOut{cluster_id, result_order, member_rank, levels, stats});
}

int hmk_greedy_sweep_from_edges_dev(hmk_ctx *ctx, const void *d_edges, uint64_t n_edges, int symmetric, int threshold, int threshold_hi,
                                    int max_clusters, int32_t *cluster_id, int32_t *result_order, int32_t *member_rank,
                                    hmk_greedy_level *levels, hmk_greedy_sweep_stats *stats) {
    return greedy_sweep_from_edges_dev(ctx, d_edges, n_edges, symmetric != 0, threshold, threshold_hi, max_clusters,
                                       SweepOut{cluster_id, result_order, member_rank, levels, stats});
}

}  // extern "C"
