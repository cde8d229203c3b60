// hmk_levels.cpp -- the steps the threshold-range calls share (hmk_levels.h): where a call's edges lie, the range and caller-block
// checks, the neighbour pass into the context's edge buffer, the edges dealt by level (k_sweep.hip).
#include "hmk_levels.h"

namespace hmk { namespace impl {

EdgeRuns edge_runs(const uint64_t *base, uint64_t stride, uint32_t n_runs, const unsigned long long *count) {
    EdgeRuns E{};
    E.base = base;
    E.stride = stride;
    E.n_runs = n_runs;
    for (uint32_t s = 0; s < n_runs; s++) {
        E.count[s] = count[s];
        E.chunk_start[s + 1] = E.chunk_start[s] + (uint32_t)((count[s] + EDGE_RUN_CHUNK - 1) / EDGE_RUN_CHUNK);
    }
    return E;
}

int check_level_range(hmk_ctx *ctx, int thr, int thr_hi, bool scores_fit_int16) {
    if (thr_hi < thr) return fail(ctx, HMK_ERR_BAD_ARG, "threshold_hi is below threshold");
    if ((long long)thr_hi - thr > (long long)SWEEP_MAX_LEVELS - 1) return fail(ctx, HMK_ERR_BAD_ARG, "at most 256 levels per call: threshold_hi - threshold <= 255");
    if (scores_fit_int16 && thr_hi > 32767) return fail(ctx, HMK_ERR_BAD_ARG, "threshold_hi is above 32767, the highest score an edge holds");
    return HMK_OK;
}

int check_edges_dev(hmk_ctx *ctx, const void *d_edges, uint64_t n_edges) {
    if (n_edges && !d_edges) return fail(ctx, HMK_ERR_BAD_ARG, "null edge buffer");
    if (n_edges > ((uint64_t)1 << 41)) return fail(ctx, HMK_ERR_BAD_ARG, "more than 2^41 edges");   // (chunks are counted in 32 bits)
    return HMK_OK;
}

int pass_edge_runs(hmk_ctx *ctx, int X, int p, int thr, bool symmetric, PassRuns *out) {
    unsigned long long counts[HMK_EDGE_SHARDS];
    double ms = 0;
    const int st = neighbors_internal(ctx, X, p, thr, 0, 1, sizing::edge_capacity_guess(symmetric, ctx->n, 1, ctx->sw.edge_guess, ctx->edges.cap), counts, &ms);
    if (st) return st;
    out->E = edge_runs(ctx->edges.d, ctx->edges.seg_cap(), HMK_EDGE_SHARDS, counts);
    out->total = total_of(counts);
    out->pairs_scored = ctx->plan.stats.pairs_scored;
    out->kernel_ms = ms;
    return HMK_OK;
}

int deal_by_level(hmk_ctx *ctx, const char *what, hipStream_t Q, const EdgeRuns &E, uint64_t total, int thr, int thr_hi, EventPair *timed,
                  LevelPrefix *back, const uint64_t **dealt, SweepState **state) {
    const uint32_t n = ctx->n, nl = (uint32_t)(thr_hi - thr) + 1;
    HIPCHK(ctx, ensure_buf(ctx, SB_SWEEP_STATE, sizeof(SweepState)));
    HIPCHK(ctx, ensure_buf(ctx, SB_SWEEP_RUNS, std::max<uint64_t>(total, 1) * sizeof(uint64_t)));
    SweepState *st = buf<SweepState>(ctx, SB_SWEEP_STATE);
    uint64_t *runs = buf<uint64_t>(ctx, SB_SWEEP_RUNS);
    hipError_t e = timed ? timed->start(Q) : hipSuccess;
    if (e == hipSuccess) e = hipMemsetAsync(st, 0, sizeof(SweepState), Q);
    if (e == hipSuccess) e = launch_sweep_hist(E, n, thr, thr_hi, st, Q);
    if (e == hipSuccess) e = launch_sweep_scan(nl, st, Q);
    if (e == hipSuccess) e = launch_sweep_deal(E, n, thr, thr_hi, st, runs, Q);
    if (e == hipSuccess && timed) e = timed->stop(Q);
    if (e == hipSuccess) e = hipMemcpyAsync(back, st->prefix, sizeof(LevelPrefix), hipMemcpyDeviceToHost, Q);
    if (e == hipSuccess) e = hipStreamSynchronize(Q);
    if (e != hipSuccess) return fail_hip(ctx, what, e);
    if (back->flag) return fail(ctx, HMK_ERR_BAD_ARG, "edge list references a sequence outside [0, n) or a self pair");
    if (back->prefix[0] > total) return fail(ctx, HMK_ERR_DEVICE, std::string(what) + ": more edges dealt than given");
    *dealt = runs;
    if (state) *state = st;
    return HMK_OK;
}

} }  // namespace hmk::impl
