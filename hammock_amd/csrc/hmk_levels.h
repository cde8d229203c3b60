// hmk_levels.h -- what the calls that answer "at one threshold or a range of them" from one neighbour pass share on the host
// (hmk_components.cpp, hmk_sweep.cpp, hmk_representatives.cpp, hmk_density.cpp, hmk_orders.cpp): plain functions, each entry point
// still lists its own steps.  Not part of the public ABI.
#ifndef HMK_LEVELS_H
#define HMK_LEVELS_H
#include "hmk_ctx.h"
#include "hmk_sweep.h"

namespace hmk { namespace impl {

// the runs at base + s * stride with their counts (in host memory), and the chunks before each
EdgeRuns edge_runs(const uint64_t *base, uint64_t stride, uint32_t n_runs, const unsigned long long *count);

// threshold ... threshold_hi is a range of 1 to SWEEP_MAX_LEVELS levels; scores_fit_int16: and threshold_hi is a score an edge can hold
int check_level_range(hmk_ctx *ctx, int thr, int thr_hi, bool scores_fit_int16);
// a caller's device block of n_edges packed edges: not null, and its chunks can be counted in 32 bits
int check_edges_dev(hmk_ctx *ctx, const void *d_edges, uint64_t n_edges);

// The neighbour pass at `thr` into the context's edge buffer (neighbors_internal: the all-vs-all plan slot, grown until it fits).
// symmetric: what the first capacity guess assumes of the matrix.  -> the runs over ctx->edges, their total, the pass's numbers.
struct PassRuns {
    EdgeRuns E;
    uint64_t total, pairs_scored;
    double kernel_ms;
};
int pass_edge_runs(hmk_ctx *ctx, int X, int p, int thr, bool symmetric, PassRuns *out);

// What the deal brings back in one copy: prefix[l] = the edges with score >= thr + l, flag as SweepState's.
struct LevelPrefix {
    unsigned long long prefix[SWEEP_MAX_LEVELS], flag;
};
static_assert(offsetof(SweepState, flag) == offsetof(SweepState, prefix) + sizeof(LevelPrefix::prefix), "prefix and flag are read in one copy");

// The whole edges E (total of them) dealt by level min(score, thr_hi) - thr, the top level first, on Q: k_sweep_hist, k_sweep_scan,
// k_sweep_deal into SB_SWEEP_RUNS with no host synchronisation between them, prefix[] and the flag back in one copy, Q synchronised.
// The edges with score >= thr + l are then dealt[0 .. back->prefix[l]), i.e. edge_runs(*dealt, 0, 1, &back->prefix[l]), and
// &(*state)->prefix[l] is their number in device memory (state: null where the caller does not need it).  timed: null, or two
// events recorded around the zeroing and the three kernels (not the copy).  what: the call's name in the error texts.
int deal_by_level(hmk_ctx *ctx, const char *what, hipStream_t Q, const EdgeRuns &E, uint64_t total, int thr, int thr_hi, EventPair *timed,
                  LevelPrefix *back, const uint64_t **dealt, SweepState **state = nullptr);

} }  // namespace hmk::impl
#endif
