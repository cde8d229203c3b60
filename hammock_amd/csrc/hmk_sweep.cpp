// hmk_sweep.cpp -- the greedy clusterings at every threshold of a range from ONE scoring pass (hmk_greedy_sweep*).
// Replaces one LimitedGreedySequenceClusterer(scorer, t, maxClusters).cluster(sequences) per threshold t
// (LimitedGreedySequenceClusterer.java:22,39-69), each of which scores the whole pair space again.
//   pass      pass_edge_runs (hmk_levels.cpp): hmk_neighbors_shifted's (neighbors_internal: the all-vs-all plan slot, the same kernels) at
//             `threshold` into the context's edge buffer, grown until it fits;
//   deal      deal_by_level (hmk_levels.cpp): k_sweep_hist, k_sweep_scan, k_sweep_deal put the whole edges in one run per level
//             min(score, threshold_hi) - threshold, the top level first (SB_SWEEP_RUNS), so that the edges with score >= t are the
//             prefix [0, prefix[t - threshold]);
//   tails     per level the clustering tail as it is (cluster_on_device) on an EdgeSource of one segment: that prefix.
// hmk_greedy_sweep_from_edges is the same answer on the host: the edges sorted by level by counting, hmk_greedy_from_edges's merge per
// prefix -- the second implementation the device path is tested against, and what a host-only context runs.
#include "hmk_levels.h"

namespace hmk { namespace impl {

namespace {

struct SweepOut {
    int32_t *cluster_id, *result_order, *member_rank;   // each [n_levels][n] or null
    hmk_greedy_level *levels;
    hmk_greedy_sweep_stats *stats;
};

// the argument checks all three entry points make before the device is looked at
int check_sweep(hmk_ctx *ctx, int thr, int thr_hi, const SweepOut &o) {
    const int st = check_level_range(ctx, thr, thr_hi, true);
    if (st) return st;
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

// The device side behind the edges: E names them (packed, on this context's device), total = their number.  X, p: the scoring
// parameters the adjacency format follows from (scored = true), else the tail reads the format off each level's scores.
int sweep_on_device(hmk_ctx *ctx, const EdgeRuns &E, uint64_t total, bool symmetric, bool scored, int X, int p, int thr, int thr_hi, int max_clusters,
                    const SweepOut &o, hmk_greedy_sweep_stats &S) {
    const uint32_t n = ctx->n, nl = (uint32_t)(thr_hi - thr) + 1;
    int st = greedy_streams(ctx);
    if (st) return st;
    hipStream_t Q = ctx->gstream;
    EventPair ev;   // around the deal's kernels
    HIPCHK(ctx, ev.create());
    LevelPrefix back;
    const uint64_t *dealt = nullptr;
    SweepState *state = nullptr;
    st = deal_by_level(ctx, "greedy sweep", Q, E, total, thr, thr_hi, &ev, &back, &dealt, &state);
    if (st) return st;
    float ms = 0;
    HIPCHK(ctx, ev.elapsed(&ms));
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
        const bool packed = scored && adjacency_packed(ctx, X, p, t);
        const EdgeSource src = one_segment_source(dealt, &state->prefix[l], m, symmetric, scored ? &packed : nullptr, t);
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
    PassRuns P;
    st = pass_edge_runs(ctx, X, p, thr, ctx->symmetric, &P);
    if (st) return st;
    S.kernel_ms = P.kernel_ms;
    S.pairs_scored = P.pairs_scored;
    st = sweep_on_device(ctx, P.E, P.total, ctx->symmetric, true, X, p, thr, thr_hi, max_clusters, o, S);
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
    st = check_edges_dev(ctx, d_edges, n_edges);
    if (st) return st;
    const uint32_t nl = (uint32_t)(thr_hi - thr) + 1;
    if (ctx->n == 0) return empty_set(nl, o);
    st = need_device(ctx);
    if (st) return st;
    // the caller's block may have been written on any stream of its own: wait for the device
    HIPCHK(ctx, hipDeviceSynchronize());
    hmk_greedy_sweep_stats S{};
    const unsigned long long cnt = n_edges;
    st = sweep_on_device(ctx, edge_runs((const uint64_t *)d_edges, 0, 1, &cnt), n_edges, symmetric, false, 0, 0, thr, thr_hi, max_clusters, o, S);
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
