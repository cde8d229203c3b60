// hmk_density.cpp -- density clustering of the uploaded set at one threshold or a range (hmk_density_*): DBSCAN on the neighbour
// graph {score >= t}, made independent of any order.  degree(i) = the edges that touch i; i is core iff degree(i) >= min_neighbors;
// clusters are the connected components of the core vertices under core-core edges, named by their smallest core index; a non-core
// vertex next to a core one is border and joins the cluster of its anchor, the core neighbour with the largest score (among equal
// scores the smallest index); everything else is noise.
//   pass      pass_edge_runs (hmk_levels.cpp): hmk_neighbors_shifted's (neighbors_internal: the all-vs-all plan slot, the same kernels) at
//             `threshold` into the context's edge buffer, grown until it fits;
//   deal      a range only: k_sweep_hist, k_sweep_scan, k_sweep_deal through deal_by_level (hmk_levels.cpp; SB_SWEEP_STATE, SB_SWEEP_RUNS): the edges
//             with score >= t are the prefix [0, prefix[t - threshold]) of one buffer, and level l's own run is [prefix[l + 1], prefix[l]).
//             A single level reads the pass's segments directly;
//   levels    from the top down, k_den_degree, k_den_core, k_den_link, k_den_labels, k_den_sizes per level (k_density.hip), every level
//             with a record of its own in the device block, so nothing waits for the host between levels;
//   rows      the labels kernel writes the requested rows into SB_DEN_ROWS, as many levels as sizing::density_rows_per_batch allows;
//             a batch comes back with one copy per requested array.  The levels' block comes back last.
// hmk_density_from_edges is the definition written plainly on the host: the second implementation the device path is tested against,
// and what a host-only context runs.
#include "hmk_levels.h"
#include "hmk_density.h"

namespace hmk { namespace impl {

namespace {

struct DenOut {
    uint32_t *cluster, *anchor, *degree;   // each [n_levels][n] or null
    hmk_density_level *levels;
    hmk_density_stats *stats;
};

// the argument checks all three entry points make before the device is looked at
int check_density(hmk_ctx *ctx, int thr, int thr_hi, int min_neighbors, const DenOut &o) {
    if (min_neighbors < 0) return fail(ctx, HMK_ERR_BAD_ARG, "min_neighbors is negative");
    const int st = check_level_range(ctx, thr, thr_hi, true);
    if (st) return st;
    if (ctx->n && !o.levels && !o.cluster && !o.anchor && !o.degree) return fail(ctx, HMK_ERR_BAD_ARG, "null outputs (levels, cluster, anchor and degree)");
    return HMK_OK;
}

int empty_set(uint32_t nl, int min_neighbors, const DenOut &o) {
    if (o.levels) std::fill(o.levels, o.levels + nl, hmk_density_level{});
    if (o.stats) {
        *o.stats = hmk_density_stats{};
        o.stats->n_levels = nl;
        o.stats->min_neighbors = (uint32_t)min_neighbors;
    }
    return HMK_OK;
}

void fill_stats(hmk_density_stats &S, const std::vector<hmk_density_level> &lv, int min_neighbors) {
    S.n_levels = (uint32_t)lv.size();
    S.min_neighbors = (uint32_t)min_neighbors;
    S.n_edges = lv[0].n_edges;
    S.n_core = lv[0].n_core;
    S.n_border = lv[0].n_border;
    S.n_noise = lv[0].n_noise;
    S.n_clusters = lv[0].n_clusters;
    S.largest = lv[0].largest;
}

// The device side behind the edges: src names them (packed, on this context's device), total = their number.
int density_on_device(hmk_ctx *ctx, const EdgeRuns &src, uint64_t total, int thr, int thr_hi, int min_neighbors, const DenOut &o, hmk_density_stats &S) {
    const uint32_t n = ctx->n, nl = (uint32_t)(thr_hi - thr) + 1;
    int st = greedy_streams(ctx);
    if (st) return st;
    hipStream_t Q = ctx->gstream;
    EventPair ev;
    HIPCHK(ctx, ev.create());
    HIPCHK(ctx, ev.start(Q));
    // a range: the whole edges by level, the top level first (the sweep's kernels and buffers)
    LevelPrefix back{};
    const uint64_t *dealt = nullptr;
    if (nl > 1) {
        st = deal_by_level(ctx, "density", Q, src, total, thr, thr_hi, nullptr, &back, &dealt);
        if (st) return st;
    }
    uint32_t *const host_rows[3] = {o.cluster, o.anchor, o.degree};
    const uint32_t n_arrays = (o.cluster ? 1u : 0u) + (o.anchor ? 1u : 0u) + (o.degree ? 1u : 0u);
    const uint32_t per_batch = sizing::density_rows_per_batch(n, n_arrays, nl);   // levels whose rows wait on the device for one copy
    HIPCHK(ctx, ensure_buf(ctx, SB_DEN_STATE, sizeof(DenState)));
    HIPCHK(ctx, ensure_buf(ctx, SB_DEN_VERT, den_vertex_bytes(n)));
    HIPCHK(ctx, ensure_buf(ctx, SB_DEN_ROWS, sizing::density_rows_bytes(n, n_arrays, per_batch)));
    DenState *dst = buf<DenState>(ctx, SB_DEN_STATE);
    const DenVertex V = den_vertex_arrays(buf<void>(ctx, SB_DEN_VERT), n);
    uint32_t *rows = buf<uint32_t>(ctx, SB_DEN_ROWS);
    uint32_t *dev_rows[3] = {nullptr, nullptr, nullptr};   // each requested array's rows of the batch at hand
    for (uint32_t a = 0, k = 0; a < 3; a++)
        if (host_rows[a]) dev_rows[a] = rows + (size_t)k++ * per_batch * n;
    const size_t state_bytes = offsetof(DenState, level) + (size_t)nl * sizeof(DenLevel);
    hipError_t e = hipMemsetAsync(dst, 0, state_bytes, Q);
    if (e == hipSuccess) e = launch_den_init(V, n, Q);
    uint32_t batch_hi = nl - 1;   // the batch at hand holds the levels batch_lo ... batch_hi, level l in slot l - batch_lo
    for (uint32_t l = nl; e == hipSuccess && l-- > 0;) {
        const uint32_t batch_lo = batch_hi + 1 >= per_batch ? batch_hi + 1 - per_batch : 0, slot = l - batch_lo;
        DenEdges D;
        D.E = nl > 1 ? edge_runs(dealt, 0, 1, &back.prefix[l]) : src;
        D.own_start = nl > 1 && l + 1 < nl ? back.prefix[l + 1] : 0;
        e = launch_den_degree(D, n, thr, V, dst, l, Q);
        if (e == hipSuccess) e = launch_den_core(n, (uint32_t)min_neighbors, V, dst, l, Q);
        if (e == hipSuccess) e = launch_den_link(D, n, thr, V, dst, l, Q);
        if (e == hipSuccess)
            e = launch_den_labels(n, V, dev_rows[0] ? dev_rows[0] + (size_t)slot * n : nullptr, dev_rows[1] ? dev_rows[1] + (size_t)slot * n : nullptr,
                                  dev_rows[2] ? dev_rows[2] + (size_t)slot * n : nullptr, dst, l, Q);
        if (e == hipSuccess) e = launch_den_sizes(n, V, dst, l, Q);
        if (l == batch_lo) {   // the batch is full: its rows go home, the next one starts below it
            for (uint32_t a = 0; a < 3 && e == hipSuccess; a++)
                if (host_rows[a])
                    e = hipMemcpyAsync(host_rows[a] + (size_t)batch_lo * n, dev_rows[a], (size_t)(batch_hi - batch_lo + 1) * n * 4, hipMemcpyDeviceToHost, Q);
            batch_hi = batch_lo - 1;   // (wraps behind level 0: the loop ends there)
        }
    }
    std::vector<unsigned char> block(state_bytes);
    if (e == hipSuccess) e = hipMemcpyAsync(block.data(), dst, state_bytes, hipMemcpyDeviceToHost, Q);
    if (e == hipSuccess) e = hipStreamSynchronize(Q);
    if (e != hipSuccess) return fail_hip(ctx, "density", e);
    const DenState *hb = (const DenState *)block.data();
    if (hb->flag) return fail(ctx, HMK_ERR_BAD_ARG, "edge list references a sequence outside [0, n) or a self pair");
    std::vector<hmk_density_level> lv(nl);
    for (uint32_t l = 0; l < nl; l++) {
        const DenLevel &d = hb->level[l];
        lv[l].n_edges = nl > 1 ? back.prefix[l] : d.n_edges;
        lv[l].n_core = d.n_core;
        lv[l].n_border = d.n_border;
        lv[l].n_noise = d.n_noise;
        lv[l].n_clusters = d.n_clusters;
        lv[l].largest = d.largest;
        if (ctx->sw.greedy_timing)
            std::fprintf(stderr, "[hmk density] threshold %d: %u vertices turned core, the link step looked at %llu of %llu edges\n", thr + (int)l, d.new_core,
                         d.looked, (unsigned long long)lv[l].n_edges);
    }
    HIPCHK(ctx, ev.stop(Q));
    HIPCHK(ctx, hipEventSynchronize(ev.b));
    float ms = 0;
    HIPCHK(ctx, ev.elapsed(&ms));
    S.density_ms = ms;
    fill_stats(S, lv, min_neighbors);
    if (o.levels) std::copy(lv.begin(), lv.end(), o.levels);
    return HMK_OK;
}

int density_shifted(hmk_ctx *ctx, int X, int p, int thr, int thr_hi, int min_neighbors, const DenOut &o) {
    if (!ctx) return fail(nullptr, HMK_ERR_BAD_ARG, "null context");
    std::lock_guard<std::mutex> lock(ctx->mu);
    refresh_switches(ctx);
    int st = check_density(ctx, thr, thr_hi, min_neighbors, o);
    if (st) return st;
    if (!ctx->symmetric)
        return fail(ctx, HMK_ERR_BAD_ARG, "density clustering needs a symmetric scoring matrix: a ~ b must not depend on which of the two is seq1");
    const uint32_t n = ctx->n, nl = (uint32_t)(thr_hi - thr) + 1;
    if (n == 0) return empty_set(nl, min_neighbors, o);
    st = need_device(ctx);
    if (st) return st;
    hmk_density_stats S{};
    PassRuns P;
    st = pass_edge_runs(ctx, X, p, thr, true, &P);
    if (st) return st;
    S.kernel_ms = P.kernel_ms;
    S.pairs_scored = P.pairs_scored;
    st = density_on_device(ctx, P.E, P.total, thr, thr_hi, min_neighbors, o, S);
    if (st == HMK_OK && o.stats) *o.stats = S;
    return st;
}

int density_from_edges_dev(hmk_ctx *ctx, const void *d_edges, uint64_t n_edges, int thr, int thr_hi, int min_neighbors, const DenOut &o) {
    if (!ctx) return fail(nullptr, HMK_ERR_BAD_ARG, "null context");
    std::lock_guard<std::mutex> lock(ctx->mu);
    refresh_switches(ctx);
    int st = check_density(ctx, thr, thr_hi, min_neighbors, o);
    if (st) return st;
    st = check_edges_dev(ctx, d_edges, n_edges);
    if (st) return st;
    const uint32_t nl = (uint32_t)(thr_hi - thr) + 1;
    if (ctx->n == 0) return empty_set(nl, min_neighbors, o);
    st = need_device(ctx);
    if (st) return st;
    // the caller's block may have been written on any stream of its own: wait for the device
    HIPCHK(ctx, hipDeviceSynchronize());
    hmk_density_stats S{};
    const unsigned long long cnt = n_edges;
    st = density_on_device(ctx, edge_runs((const uint64_t *)d_edges, 0, 1, &cnt), n_edges, thr, thr_hi, min_neighbors, o, S);
    if (st == HMK_OK && o.stats) *o.stats = S;
    return st;
}

// The definition, level by level: the degrees by counting, a sequential union-find over the core-core edges (the larger root under
// the smaller, so a root is its tree's smallest member), one pass over the edges for the anchors.
int density_from_edges(hmk_ctx *ctx, const uint64_t *edges, uint64_t n_edges, int thr, int thr_hi, int min_neighbors, const DenOut &o) {
    if (!ctx) return fail(nullptr, HMK_ERR_BAD_ARG, "null context");
    std::lock_guard<std::mutex> lock(ctx->mu);
    refresh_switches(ctx);
    const int st = check_density(ctx, thr, thr_hi, min_neighbors, o);
    if (st) return st;
    if (n_edges && !edges) return fail(ctx, HMK_ERR_BAD_ARG, "null edge list");
    const uint32_t n = ctx->n, nl = (uint32_t)(thr_hi - thr) + 1;
    for (uint64_t k = 0; k < n_edges; k++) {
        const uint32_t x = HMK_EDGE_X(edges[k]), m = HMK_EDGE_M(edges[k]);
        if (x >= n || m >= n || x == m) return fail(ctx, HMK_ERR_BAD_ARG, "edge list references a sequence outside [0, n) or a self pair");
    }
    if (n == 0) return empty_set(nl, min_neighbors, o);
    std::vector<hmk_density_level> lv(nl);
    std::vector<uint32_t> deg(n), parent(n), cluster(n), anchor(n), members(n);
    std::vector<uint64_t> key(n);
    auto find = [&](uint32_t v) {
        while (parent[v] != v) {
            parent[v] = parent[parent[v]];
            v = parent[v];
        }
        return v;
    };
    for (uint32_t l = 0; l < nl; l++) {
        const int t = thr + (int)l;
        hmk_density_level &L = lv[l];
        L = hmk_density_level{};
        std::fill(deg.begin(), deg.end(), 0u);
        for (uint64_t k = 0; k < n_edges; k++) {
            if (HMK_EDGE_SCORE(edges[k]) < t) continue;
            L.n_edges++;
            deg[HMK_EDGE_X(edges[k])]++;
            deg[HMK_EDGE_M(edges[k])]++;
        }
        auto core = [&](uint32_t v) { return deg[v] >= (uint32_t)min_neighbors; };
        for (uint32_t i = 0; i < n; i++) {
            parent[i] = i;
            key[i] = 0;
        }
        for (uint64_t k = 0; k < n_edges; k++) {
            const int32_t sc = HMK_EDGE_SCORE(edges[k]);
            if (sc < t) continue;
            const uint32_t x = HMK_EDGE_X(edges[k]), m = HMK_EDGE_M(edges[k]);
            if (core(x) && core(m)) {
                const uint32_t a = find(x), b = find(m);
                if (a != b) parent[std::max(a, b)] = std::min(a, b);
            } else if (core(x) || core(m)) {
                const uint32_t c = core(x) ? x : m, b = core(x) ? m : x;   // the core end, the other end
                key[b] = std::max(key[b], (uint64_t)(uint32_t)(sc + 32768) << 32 | (0xFFFFFFFFu - c));
            }
        }
        std::fill(members.begin(), members.end(), 0u);
        for (uint32_t i = 0; i < n; i++) {
            if (core(i)) {
                anchor[i] = i;
                cluster[i] = find(i);
                L.n_core++;
                L.n_clusters += cluster[i] == i ? 1u : 0u;
            } else if (key[i]) {
                anchor[i] = 0xFFFFFFFFu - (uint32_t)key[i];
                cluster[i] = find(anchor[i]);
                L.n_border++;
            } else {
                anchor[i] = cluster[i] = HMK_DENSITY_NOISE;
                L.n_noise++;
            }
            if (cluster[i] != HMK_DENSITY_NOISE) L.largest = std::max(L.largest, ++members[cluster[i]]);
        }
        if (o.cluster) std::copy(cluster.begin(), cluster.end(), o.cluster + (size_t)l * n);
        if (o.anchor) std::copy(anchor.begin(), anchor.end(), o.anchor + (size_t)l * n);
        if (o.degree) std::copy(deg.begin(), deg.end(), o.degree + (size_t)l * n);
    }
    hmk_density_stats S{};
    fill_stats(S, lv, min_neighbors);
    if (o.levels) std::copy(lv.begin(), lv.end(), o.levels);
    if (o.stats) *o.stats = S;
    return HMK_OK;
}

}  // namespace

} }  // namespace hmk::impl

extern "C" {

int hmk_density_shifted(hmk_ctx *ctx, int max_shift, int shift_penalty, int threshold, int threshold_hi, int min_neighbors, uint32_t *cluster,
                        uint32_t *anchor, uint32_t *degree, hmk_density_level *levels, hmk_density_stats *stats) {
    return density_shifted(ctx, max_shift, shift_penalty, threshold, threshold_hi, min_neighbors, DenOut{cluster, anchor, degree, levels, stats});
}

int hmk_density_from_edges(hmk_ctx *ctx, const uint64_t *edges, uint64_t n_edges, int threshold, int threshold_hi, int min_neighbors, uint32_t *cluster,
                           uint32_t *anchor, uint32_t *degree, hmk_density_level *levels, hmk_density_stats *stats) {
    return density_from_edges(ctx, edges, n_edges, threshold, threshold_hi, min_neighbors, DenOut{cluster, anchor, degree, levels, stats});
}

int hmk_density_from_edges_dev(hmk_ctx *ctx, const void *d_edges, uint64_t n_edges, int threshold, int threshold_hi, int min_neighbors, uint32_t *cluster,
                               uint32_t *anchor, uint32_t *degree, hmk_density_level *levels, hmk_density_stats *stats) {
    return density_from_edges_dev(ctx, d_edges, n_edges, threshold, threshold_hi, min_neighbors, DenOut{cluster, anchor, degree, levels, stats});
}

}  // extern "C"
