// hmk_components.cpp -- connected components of the thresholded neighbour graph, at one threshold or a range (hmk_components_*).
//   pass      pass_edge_runs (hmk_levels.cpp): hmk_neighbors_shifted's (neighbors_internal: the all-vs-all plan slot, the same kernels) at
//             `threshold` into the context's edge buffer, grown until it fits;
//   levels    k_cc_hist, k_cc_scan, k_cc_partition: the edges' (x, m) in one run per level min(score, threshold_hi) - threshold (SB_CC_RUNS);
//             a single-level call that wants no `levels` skips them and unites straight from the pass's segments;
//   union     one k_cc_union launch per level from threshold_hi down, k_cc_flatten and k_cc_sizes behind each: no host
//             synchronisation between levels, the levels' numbers gather in a device block (SB_CC_STATE);
//   copy      that block and parent[] (= component at `threshold`) at the end.
// hmk_components_from_edges is the same answer by a sequential union-find on the host: the second implementation the device path is
// tested against, and what a host-only context runs.
#include "hmk_levels.h"
#include "hmk_components.h"

namespace hmk { namespace impl {

namespace {

// the argument checks all three entry points make before the device is looked at
int check_components(hmk_ctx *ctx, int thr, int thr_hi, const uint32_t *component, const hmk_component_level *levels) {
    static_assert(CC_MAX_LEVELS == SWEEP_MAX_LEVELS, "check_level_range checks the levels of both");
    const int st = check_level_range(ctx, thr, thr_hi, false);   // (no edge is dealt whole here: threshold_hi may lie above every score)
    if (st) return st;
    if (ctx->n && !component && !levels) return fail(ctx, HMK_ERR_BAD_ARG, "null outputs (component and levels)");
    return HMK_OK;
}

void fill_stats(hmk_components_stats *S, const hmk_component_level *lv, uint32_t n_levels) {
    S->n_levels = n_levels;
    S->n_edges = lv[0].n_edges;
    S->n_components = lv[0].n_components;
    S->n_singletons = lv[0].n_singletons;
    S->largest = lv[0].largest;
}

// The device side behind the edges: E names them (packed, on this context's device), total = their number.
int components_on_device(hmk_ctx *ctx, const EdgeRuns &E, uint64_t total, int thr, int thr_hi, uint32_t *component, hmk_component_level *levels,
                         hmk_components_stats *S) {
    const uint32_t n = ctx->n, nl = (uint32_t)(thr_hi - thr) + 1;
    const bool direct = nl == 1 && !levels;   // one level and only its labels wanted: no histogram, no partition
    HIPCHK(ctx, ensure_buf(ctx, SB_CC_PARENT, (size_t)n * sizeof(uint32_t)));
    HIPCHK(ctx, ensure_buf(ctx, SB_CC_SIZE, (size_t)n * sizeof(uint32_t)));
    HIPCHK(ctx, ensure_buf(ctx, SB_CC_STATE, sizeof(CcState)));
    if (!direct && total) HIPCHK(ctx, ensure_buf(ctx, SB_CC_RUNS, (size_t)total * sizeof(uint64_t)));
    uint32_t *parent = buf<uint32_t>(ctx, SB_CC_PARENT), *size = buf<uint32_t>(ctx, SB_CC_SIZE);
    CcState *st = buf<CcState>(ctx, SB_CC_STATE);
    uint64_t *runs = buf<uint64_t>(ctx, SB_CC_RUNS);
    hipStream_t Q = nullptr;
    EventPair ev;
    HIPCHK(ctx, ev.create());
    hipError_t e = ev.start(Q);
    if (e == hipSuccess) e = hipMemsetAsync(st, 0, sizeof(CcState), Q);
    if (e == hipSuccess) e = launch_cc_init(parent, size, n, Q);
    if (e == hipSuccess && !direct && total) {
        e = launch_cc_hist(E, n, thr, thr_hi, st, Q);
        if (e == hipSuccess) e = launch_cc_scan(nl, st, Q);
        if (e == hipSuccess) e = launch_cc_partition(E, n, thr, thr_hi, st, runs, Q);
    }
    for (uint32_t l = nl; l-- > 0 && e == hipSuccess;) {
        e = direct ? launch_cc_union_edges(E, n, thr, parent, st, Q) : launch_cc_union(runs, total, l, parent, st, Q);
        if (e == hipSuccess) e = launch_cc_flatten(parent, size, n, Q);
        if (e == hipSuccess) e = launch_cc_sizes(size, n, l, st, Q);
    }
    if (e == hipSuccess) e = ev.stop(Q);
    std::vector<hmk_component_level> lv(nl);
    if (e == hipSuccess) e = hipMemcpy(lv.data(), st->levels, nl * sizeof(hmk_component_level), hipMemcpyDeviceToHost);
    const bool bad = e == hipSuccess && lv[0].reserved != 0;
    if (e == hipSuccess && !bad && component) e = hipMemcpy(component, parent, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost);
    float ms = 0;
    if (e == hipSuccess) e = ev.elapsed(&ms);
    if (e != hipSuccess) return fail_hip(ctx, "components", e);
    if (bad) return fail(ctx, HMK_ERR_BAD_ARG, "edge list references a sequence outside [0, n) or a self pair");
    // the device counted each level's hooks: components at t = n - the hooks of the levels >= t
    uint32_t hooks = 0;
    for (uint32_t l = nl; l-- > 0;) {
        hooks += lv[l].n_components;
        lv[l].n_components = n - hooks;
        lv[l].reserved = 0;
    }
    S->components_ms = ms;
    fill_stats(S, lv.data(), nl);
    if (levels) std::copy(lv.begin(), lv.end(), levels);
    return HMK_OK;
}

int components_shifted(hmk_ctx *ctx, int X, int p, int thr, int thr_hi, uint32_t *component, hmk_component_level *levels,
                       hmk_components_stats *stats) {
    if (!ctx) return fail(nullptr, HMK_ERR_BAD_ARG, "null context");
    std::lock_guard<std::mutex> lock(ctx->mu);
    refresh_switches(ctx);
    hmk_components_stats S{};
    int st = check_components(ctx, thr, thr_hi, component, levels);
    if (st) return st;
    if (!ctx->symmetric)
        return fail(ctx, HMK_ERR_BAD_ARG, "components need a symmetric scoring matrix: a ~ b must not depend on which of the two is seq1");
    st = need_device(ctx);
    if (st) return st;
    const uint32_t n = ctx->n, nl = (uint32_t)(thr_hi - thr) + 1;
    if (n == 0) {
        if (levels) std::fill(levels, levels + nl, hmk_component_level{});
        S.n_levels = nl;
        if (stats) *stats = S;
        return HMK_OK;
    }
    PassRuns P;
    st = pass_edge_runs(ctx, X, p, thr, true, &P);
    if (st) return st;
    S.kernel_ms = P.kernel_ms;
    S.pairs_scored = P.pairs_scored;
    st = components_on_device(ctx, P.E, P.total, thr, thr_hi, component, levels, &S);
    if (st == HMK_OK && stats) *stats = S;
    return st;
}

int components_from_edges_dev(hmk_ctx *ctx, const void *d_edges, uint64_t n_edges, int thr, int thr_hi, uint32_t *component,
                              hmk_component_level *levels, hmk_components_stats *stats) {
    if (!ctx) return fail(nullptr, HMK_ERR_BAD_ARG, "null context");
    std::lock_guard<std::mutex> lock(ctx->mu);
    refresh_switches(ctx);
    hmk_components_stats S{};
    int st = check_components(ctx, thr, thr_hi, component, levels);
    if (st) return st;
    st = check_edges_dev(ctx, d_edges, n_edges);
    if (st) return st;
    st = need_device(ctx);
    if (st) return st;
    const uint32_t nl = (uint32_t)(thr_hi - thr) + 1;
    if (ctx->n == 0) {
        if (levels) std::fill(levels, levels + nl, hmk_component_level{});
        S.n_levels = nl;
        if (stats) *stats = S;
        return HMK_OK;
    }
    // the caller's block may have been written on any stream of its own: wait for the device
    HIPCHK(ctx, hipDeviceSynchronize());
    const unsigned long long cnt = n_edges;
    st = components_on_device(ctx, edge_runs((const uint64_t *)d_edges, 0, 1, &cnt), n_edges, thr, thr_hi, component, levels, &S);
    if (st == HMK_OK && stats) *stats = S;
    return st;
}

// Sequential union-find: the edges sorted by level, descending, by counting; a root is its tree's smallest index and carries the
// tree's size, so components, singletons and the largest component follow each hook in O(1).
int components_from_edges(hmk_ctx *ctx, const uint64_t *edges, uint64_t n_edges, int thr, int thr_hi, uint32_t *component,
                          hmk_component_level *levels, hmk_components_stats *stats) {
    if (!ctx) return fail(nullptr, HMK_ERR_BAD_ARG, "null context");
    std::lock_guard<std::mutex> lock(ctx->mu);
    refresh_switches(ctx);
    hmk_components_stats S{};
    const int st = check_components(ctx, thr, thr_hi, component, levels);
    if (st) return st;
    if (n_edges && !edges) return fail(ctx, HMK_ERR_BAD_ARG, "null edge list");
    const uint32_t n = ctx->n, nl = (uint32_t)(thr_hi - thr) + 1;
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
            if (l >= 0) sorted[at[nl - 1 - (uint32_t)l]++] = (uint64_t)HMK_EDGE_X(edges[k]) << 32 | HMK_EDGE_M(edges[k]);
        }
    }
    std::vector<uint32_t> parent(n), size(n, 1);
    std::iota(parent.begin(), parent.end(), 0u);
    auto find = [&](uint32_t v) {
        while (parent[v] != v) {
            parent[v] = parent[parent[v]];
            v = parent[v];
        }
        return v;
    };
    std::vector<hmk_component_level> lv(nl);
    uint32_t comps = n, singles = n, largest = n ? 1 : 0;
    for (uint32_t r = 0; r < nl; r++) {
        for (uint64_t k = start[r]; k < start[r + 1]; k++) {
            uint32_t a = find((uint32_t)(sorted[k] >> 32)), b = find((uint32_t)sorted[k]);
            if (a == b) continue;
            if (a > b) std::swap(a, b);
            singles -= (size[a] == 1) + (size[b] == 1);
            parent[b] = a;
            size[a] += size[b];
            largest = std::max(largest, size[a]);
            comps--;
        }
        lv[nl - 1 - r] = hmk_component_level{start[r + 1], comps, singles, largest, 0};
    }
    if (component)
        for (uint32_t v = 0; v < n; v++) component[v] = find(v);
    fill_stats(&S, lv.data(), nl);
    if (levels) std::copy(lv.begin(), lv.end(), levels);
    if (stats) *stats = S;
    return HMK_OK;
}

}  // namespace

} }  // namespace hmk::impl

extern "C" {

int hmk_components_shifted(hmk_ctx *ctx, int max_shift, int shift_penalty, int threshold, int threshold_hi, uint32_t *component,
                           hmk_component_level *levels, hmk_components_stats *stats) {
    return components_shifted(ctx, max_shift, shift_penalty, threshold, threshold_hi, component, levels, stats);
}

int hmk_components_from_edges(hmk_ctx *ctx, const uint64_t *edges, uint64_t n_edges, int threshold, int threshold_hi, uint32_t *component,
                              hmk_component_level *levels, hmk_components_stats *stats) {
    return components_from_edges(ctx, edges, n_edges, threshold, threshold_hi, component, levels, stats);
}

int hmk_components_from_edges_dev(hmk_ctx *ctx, const void *d_edges, uint64_t n_edges, int threshold, int threshold_hi, uint32_t *component,
                                  hmk_component_level *levels, hmk_components_stats *stats) {
    return components_from_edges_dev(ctx, d_edges, n_edges, threshold, threshold_hi, component, levels, stats);
}

}  // extern "C"
