// hmk_search.cpp -- query-vs-reference search: queries [q0, q1) against references [r0, r1) of the hmk_set_sequences set, two
// disjoint ranges, with any of the three scorers.  The passes over the rectangle's plans (hmk_plan.cpp: build_plan_search, build_plan_local_search), the query-side
// orientation and best-k selection on the device (k_search.hip), the extern "C" entry points.
#include "hmk_ctx.h"

namespace hmk { namespace impl {

namespace {

enum { SEARCH_SHIFTED = 0, SEARCH_LOCAL = SCORER_LOCAL, SEARCH_GLOBAL = SCORER_GLOBAL };   // (the gapped ones: launch_plan_local's numbering)

// the argument checks every search makes before it looks at the device (a host-only context answers them too)
int check_ranges(hmk_ctx *ctx, uint32_t q0, uint32_t q1, uint32_t r0, uint32_t r1) {
    if (q0 > q1 || r0 > r1 || q1 > ctx->n || r1 > ctx->n)
        return fail(ctx, HMK_ERR_BAD_ARG, "search ranges must lie within [0, n) with q0 <= q1 and r0 <= r1 (n = " + std::to_string(ctx->n) + ")");
    if (q0 < q1 && r0 < r1 && q0 < r1 && r0 < q1) return fail(ctx, HMK_ERR_BAD_ARG, "the query and reference ranges overlap");
    return HMK_OK;
}

// the search pass into the context's edge buffer (grown until every segment fits); counts and the kernels' device time
int search_pass(hmk_ctx *ctx, int scorer, int a, int b, int thr, uint32_t q0, uint32_t q1, uint32_t r0, uint32_t r1, uint64_t want_cap,
                unsigned long long counts[HMK_EDGE_SHARDS], double *ms, hmk_neighbor_stats *stats) {
    int st = scorer == SEARCH_SHIFTED ? build_plan_search(ctx, ctx->plan_search, a, b, thr, q0, q1, r0, r1)
                                      : build_plan_local_search(ctx, ctx->plan_local_search, q0, q1, r0, r1);
    if (st) return st;
    st = neighbors_grow(ctx, want_cap, counts, ms, [&](uint64_t *d_edges, uint64_t cap, unsigned long long *d_counts) {
        return scorer == SEARCH_SHIFTED ? launch_plan(ctx, ctx->plan_search, a, b, thr, d_edges, cap, d_counts, nullptr)
                                        : launch_plan_local(ctx, ctx->plan_local_search, scorer, a, b, thr, d_edges, cap, d_counts, nullptr);
    });
    if (st) return st;
    const uint64_t total = total_of(counts);
    if (scorer == SEARCH_SHIFTED) {
        *stats = ctx->plan_search.stats;
    } else {
        *stats = hmk_neighbor_stats{};
        stats->pairs_scored = ctx->plan_local_search.pairs;
        stats->n_tiles = ctx->plan_local_search.n_tiles;
    }
    stats->n_edges = total;
    stats->kernel_ms = *ms;
    return HMK_OK;
}

int search_edges(hmk_ctx *ctx, int scorer, uint32_t q0, uint32_t q1, uint32_t r0, uint32_t r1, int a, int b, int thr, uint64_t *edges,
                 uint64_t capacity, uint64_t *n_edges, hmk_neighbor_stats *stats) {
    if (!ctx) return fail(nullptr, HMK_ERR_BAD_ARG, "null context");
    std::lock_guard<std::mutex> lock(ctx->mu);
    refresh_switches(ctx);
    if (!n_edges) return fail(ctx, HMK_ERR_BAD_ARG, "n_edges must not be null");
    if (capacity && !edges) return fail(ctx, HMK_ERR_BAD_ARG, "null edge buffer");
    int st = check_ranges(ctx, q0, q1, r0, r1);
    if (st) return st;
    *n_edges = 0;
    if (scorer == SEARCH_GLOBAL) st = check_global_fits(ctx, a, b, thr);   // (before the device is looked at, like the ranges)
    if (st) return st;
    st = need_device(ctx);
    if (st) return st;
    hmk_neighbor_stats S{};
    S.symmetric = scorer == SEARCH_SHIFTED && ctx->symmetric;
    if (q0 == q1 || r0 == r1) {
        if (stats) *stats = S;
        return HMK_OK;
    }
    st = scorer == SEARCH_SHIFTED ? check_shifted(ctx, a, b, thr, q0, q1, r0, r1) : scorer == SEARCH_LOCAL ? check_local_fits(ctx, a, b, thr) : HMK_OK;
    if (st) return st;
    unsigned long long counts[HMK_EDGE_SHARDS];
    double ms = 0;
    st = search_pass(ctx, scorer, a, b, thr, q0, q1, r0, r1, capacity, counts, &ms, &S);
    if (st) return st;
    const uint64_t total = S.n_edges;
    *n_edges = total;
    if (stats) *stats = S;
    if (total > capacity) return fail(ctx, HMK_ERR_CAPACITY, "edge buffer too small: " + std::to_string(total) + " needed");
    if (total == 0) return HMK_OK;
    HIPCHK(ctx, ensure_buf(ctx, SB_SEARCH_OUT, total * sizeof(uint64_t)));
    uint64_t *d_out = buf<uint64_t>(ctx, SB_SEARCH_OUT);
    HIPCHK(ctx, launch_search_compact(ctx->edges.d, ctx->edges.seg_cap(), ctx->edges.counts, max_of(counts), q0, q1 - q0, d_out, total, nullptr));
    HIPCHK(ctx, hipMemcpy(edges, d_out, total * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return HMK_OK;
}

}  // namespace

} }  // namespace hmk::impl

extern "C" {

int hmk_search_shifted(hmk_ctx *ctx, uint32_t q0, uint32_t q1, uint32_t r0, uint32_t r1, int max_shift, int shift_penalty, int threshold,
                       uint64_t *edges, uint64_t capacity, uint64_t *n_edges, hmk_neighbor_stats *stats) {
    return search_edges(ctx, SEARCH_SHIFTED, q0, q1, r0, r1, max_shift, shift_penalty, threshold, edges, capacity, n_edges, stats);
}

int hmk_search_local(hmk_ctx *ctx, uint32_t q0, uint32_t q1, uint32_t r0, uint32_t r1, int gap_open, int gap_extend, int threshold,
                     uint64_t *edges, uint64_t capacity, uint64_t *n_edges, hmk_neighbor_stats *stats) {
    return search_edges(ctx, SEARCH_LOCAL, q0, q1, r0, r1, gap_open, gap_extend, threshold, edges, capacity, n_edges, stats);
}

int hmk_search_global(hmk_ctx *ctx, uint32_t q0, uint32_t q1, uint32_t r0, uint32_t r1, int gap_open, int gap_extend, int threshold,
                      uint64_t *edges, uint64_t capacity, uint64_t *n_edges, hmk_neighbor_stats *stats) {
    return search_edges(ctx, SEARCH_GLOBAL, q0, q1, r0, r1, gap_open, gap_extend, threshold, edges, capacity, n_edges, stats);
}

int hmk_search_best_shifted(hmk_ctx *ctx, uint32_t q0, uint32_t q1, uint32_t r0, uint32_t r1, int max_shift, int shift_penalty,
                            int threshold, uint32_t k, uint32_t *hit_index, int32_t *hit_score, uint32_t *n_hits,
                            hmk_neighbor_stats *stats) {
    if (!ctx) return fail(nullptr, HMK_ERR_BAD_ARG, "null context");
    std::lock_guard<std::mutex> lock(ctx->mu);
    refresh_switches(ctx);
    if (k < 1 || k > 32) return fail(ctx, HMK_ERR_BAD_ARG, "k must be 1..32");
    int st = check_ranges(ctx, q0, q1, r0, r1);
    if (st) return st;
    const uint32_t nq = q1 - q0;
    if (nq && (!hit_index || !hit_score || !n_hits)) return fail(ctx, HMK_ERR_BAD_ARG, "null output buffer");
    st = need_device(ctx);
    if (st) return st;
    hmk_neighbor_stats S{};
    S.symmetric = ctx->symmetric;
    if (nq == 0 || r0 == r1) {
        for (uint64_t t = 0; t < (uint64_t)nq * k; t++) { hit_index[t] = 0xFFFFFFFFu; hit_score[t] = INT32_MIN; }
        for (uint32_t q = 0; q < nq; q++) n_hits[q] = 0;
        if (stats) *stats = S;
        return HMK_OK;
    }
    st = check_shifted(ctx, max_shift, shift_penalty, threshold, q0, q1, r0, r1);
    if (st) return st;
    unsigned long long counts[HMK_EDGE_SHARDS];
    double ms = 0;
    st = search_pass(ctx, SEARCH_SHIFTED, max_shift, shift_penalty, threshold, q0, q1, r0, r1, 0, counts, &ms, &S);
    if (st) return st;
    const uint64_t total = S.n_edges;
    if (total > 0xFFFFFFFFull) return fail(ctx, HMK_ERR_OOM, "more than 2^32 - 1 hits above the threshold: raise the threshold");
    const uint64_t nk = (uint64_t)nq * k;
    HIPCHK(ctx, ensure_buf(ctx, SB_SEARCH_CNT, (size_t)2 * nq * 4));
    HIPCHK(ctx, ensure_buf(ctx, SB_SEARCH_START, ((size_t)nq + 1) * 4));
    HIPCHK(ctx, ensure_buf(ctx, SB_SEARCH_SCAN, scan_scratch_bytes(nq)));
    HIPCHK(ctx, ensure_buf(ctx, SB_SEARCH_OUT, std::max<uint64_t>(total, 1) * sizeof(uint64_t)));
    HIPCHK(ctx, ensure_buf(ctx, SB_SEARCH_HITS, nk * 8 + (size_t)nq * 4));
    uint32_t *d_index = buf<uint32_t>(ctx, SB_SEARCH_HITS);
    int32_t *d_score = (int32_t *)(d_index + nk);
    uint32_t *d_nhits = d_index + 2 * nk;
    EventPair ev;
    HIPCHK(ctx, ev.create());
    hipError_t e = ev.start(nullptr);
    if (e == hipSuccess)
        e = launch_search_best(ctx->edges.d, ctx->edges.seg_cap(), ctx->edges.counts, max_of(counts), q0, nq, k, buf<uint32_t>(ctx, SB_SEARCH_CNT),
                               buf<uint32_t>(ctx, SB_SEARCH_START), buf<uint64_t>(ctx, SB_SEARCH_SCAN), buf<uint64_t>(ctx, SB_SEARCH_OUT),
                               std::max<uint64_t>(total, 1), d_index, d_score, d_nhits, nullptr);
    if (e == hipSuccess) e = ev.stop(nullptr);
    if (e == hipSuccess) e = hipEventSynchronize(ev.b);
    float sel_ms = 0;
    if (e == hipSuccess) e = ev.elapsed(&sel_ms);
    if (e != hipSuccess) return fail_hip(ctx, "best-k selection", e);
    HIPCHK(ctx, hipMemcpy(hit_index, d_index, nk * 4, hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(hit_score, d_score, nk * 4, hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(n_hits, d_nhits, (size_t)nq * 4, hipMemcpyDeviceToHost));
    S.kernel_ms = ms + sel_ms;
    if (stats) *stats = S;
    return HMK_OK;
}

}  // extern "C"
