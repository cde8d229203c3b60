// hmk_representatives.cpp -- the representatives of the uploaded set at one threshold or a range (hmk_representatives_*): i is a
// representative iff no representative r < i is its neighbour in {score >= t} -- the greedy incremental selection of CD-HIT and
// UCLUST, on the graph the lexicographically first maximal independent set -- and for every other sequence the representatives next
// to it (covered_by: the smallest index, nearest: the largest score).
//   pass      pass_edge_runs (hmk_levels.cpp): hmk_neighbors_shifted's (neighbors_internal: the all-vs-all plan slot, the same kernels) at
//             `threshold` into the context's edge buffer, grown until it fits;
//   deal      a range only: k_sweep_hist, k_sweep_scan, k_sweep_deal through deal_by_level (hmk_levels.cpp; SB_SWEEP_STATE, SB_SWEEP_RUNS): the edges
//             with score >= t are the prefix [0, prefix[t - threshold]) of one buffer.  A single level reads the pass's segments directly;
//   rounds    per level k_rep_mark* / k_rep_decide until a round leaves no vertex undecided: the host watches the progress word the
//             decision kernel stores into pinned memory and keeps one round in the queue beside the running one (the pattern of
//             device_second_loop, hmk_cluster.cpp), no synchronisation between rounds;
//   assign    k_rep_assign over the level's edges, k_rep_finish over the vertices; the level's arrays and counters come back, the
//             groups' sizes are counted on the host from `nearest`.
// hmk_representatives_from_edges is the definition written plainly on the host: the second implementation the device path is tested
// against, and what a host-only context runs.
#include "hmk_levels.h"
#include "hmk_representatives.h"

namespace hmk { namespace impl {

namespace {

struct RepOut {
    uint32_t *covered_by, *nearest;   // each [n_levels][n] or null
    int32_t *nearest_score;
    hmk_representative_level *levels;
    hmk_representatives_stats *stats;
};

// the argument checks all three entry points make before the device is looked at
int check_representatives(hmk_ctx *ctx, int thr, int thr_hi, const RepOut &o) {
    const int st = check_level_range(ctx, thr, thr_hi, true);
    if (st) return st;
    if (ctx->n && !o.levels && !o.covered_by && !o.nearest && !o.nearest_score)
        return fail(ctx, HMK_ERR_BAD_ARG, "null outputs (levels, covered_by, nearest and nearest_score)");
    return HMK_OK;
}

int empty_set(uint32_t nl, const RepOut &o) {
    if (o.levels) std::fill(o.levels, o.levels + nl, hmk_representative_level{});
    if (o.stats) {
        *o.stats = hmk_representatives_stats{};
        o.stats->n_levels = nl;
    }
    return HMK_OK;
}

// the level's record; `largest` from the groups by nearest
hmk_representative_level level_record(uint32_t n, uint64_t n_edges, uint32_t n_rep, uint32_t n_isolated, uint32_t n_rounds, const uint32_t *nearest,
                                      std::vector<uint32_t> &members) {
    hmk_representative_level L{};
    L.n_edges = n_edges;
    L.n_representatives = n_rep;
    L.n_isolated = n_isolated;
    L.n_rounds = n_rounds;
    members.assign(n, 0);
    for (uint32_t i = 0; i < n; i++)
        if (nearest[i] < n) L.largest = std::max(L.largest, ++members[nearest[i]]);
    return L;
}

void fill_stats(hmk_representatives_stats &S, const std::vector<hmk_representative_level> &lv) {
    S.n_levels = (uint32_t)lv.size();
    S.n_edges = lv[0].n_edges;
    S.n_representatives = lv[0].n_representatives;
    S.n_isolated = lv[0].n_isolated;
    S.largest = lv[0].largest;
    S.rounds_total = 0;
    for (const hmk_representative_level &L : lv) S.rounds_total += L.n_rounds;
}

double ms_since(std::chrono::steady_clock::time_point a) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count();
}

// One level on the device: E = its edges (those with score >= t count), room = an upper bound of their number.  -> the level's block
// in *back, its arrays in the caller's rows (nearest_row is never null).
int level_on_device(hmk_ctx *ctx, hipStream_t Q, const EdgeRuns &E, uint64_t room, int t, const RepVertex &V, RepState *st, uint64_t *live0,
                    uint64_t *live1, uint64_t cap, uint32_t *covered_row, uint32_t *nearest_row, int32_t *score_row, RepState *back) {
    const uint32_t n = ctx->n;
    volatile unsigned long long *word = ctx->h_loop;
    word[0] = 0;   // (the stream is drained: no kernel of an earlier level or call stores there any more)
    word[1] = 0;
    hipError_t r = hipMemsetAsync(st, 0, sizeof(RepState), Q);
    if (r == hipSuccess) r = launch_rep_init(V, n, Q);
    // Every round decides at least the smallest undecided vertex, so n rounds always suffice.  The host keeps enqueuing rounds while it
    // watches the word (round << 32 | vertices left undecided), at most LOOKAHEAD rounds ahead of the device; a round enqueued after
    // the end finds no live edge and no undecided vertex.
    const uint32_t LOOKAHEAD = 2;
    uint32_t rounds = 0, last_seen = 0;
    bool done = false, stalled = false;
    auto t_progress = std::chrono::steady_clock::now();
    while (r == hipSuccess && !done && rounds <= n + 8) {
        rounds++;
        r = rounds <= 2 ? launch_rep_mark_first(rounds, E, n, t, V, st, live0, cap, Q) : launch_rep_mark(rounds, room, V, st, live0, live1, cap, Q);
        if (r == hipSuccess) r = launch_rep_decide(rounds, n, V, st, ctx->h_loop, Q);
        if (r != hipSuccess) break;
        for (uint32_t spins = 0;; spins++) {
            const unsigned long long w = word[0];
            const uint32_t seen = (uint32_t)(w >> 32);   // rounds the device has finished
            if (seen && (uint32_t)w == 0) { done = true; break; }
            if (rounds - seen < LOOKAHEAD) break;
            if (seen != last_seen) {
                last_seen = seen;
                t_progress = std::chrono::steady_clock::now();
            } else if ((spins & 1023u) == 1023u && ms_since(t_progress) > 60e3) { stalled = true; break; }
            std::this_thread::yield();
        }
        if (stalled) break;
    }
    if (stalled) {   // as device_second_loop: ten more seconds for the queue to drain, then the context is given up
        const auto t_drain = std::chrono::steady_clock::now();
        hipError_t q = hipStreamQuery(Q);
        while (q == hipErrorNotReady && ms_since(t_drain) < 10e3) {
            std::this_thread::sleep_for(std::chrono::milliseconds(5));
            q = hipStreamQuery(Q);
        }
        if (q == hipErrorNotReady) ctx->wedged = true;
        return fail(ctx, HMK_ERR_DEVICE, "representatives: the device made no progress for 60 s inside the rounds");
    }
    if (r == hipSuccess) r = launch_rep_assign(E, n, t, V, Q);
    if (r == hipSuccess) r = launch_rep_finish(n, V, st, Q);
    if (r == hipSuccess) r = hipMemcpyAsync(back, st, sizeof(RepState), hipMemcpyDeviceToHost, Q);
    if (r == hipSuccess && covered_row) r = hipMemcpyAsync(covered_row, V.covered_by, (size_t)n * 4, hipMemcpyDeviceToHost, Q);
    if (r == hipSuccess) r = hipMemcpyAsync(nearest_row, V.nearest, (size_t)n * 4, hipMemcpyDeviceToHost, Q);
    if (r == hipSuccess && score_row) r = hipMemcpyAsync(score_row, V.nearest_score, (size_t)n * 4, hipMemcpyDeviceToHost, Q);
    if (r == hipSuccess) r = hipStreamSynchronize(Q);
    if (r != hipSuccess) return fail_hip(ctx, "representatives", r);
    if (back->flag) return fail(ctx, HMK_ERR_BAD_ARG, "edge list references a sequence outside [0, n) or a self pair");
    if (back->rounds == 0) return fail(ctx, HMK_ERR_DEVICE, "representatives: the rounds did not come to an end");
    if (ctx->sw.greedy_timing) {
        std::string line;
        for (uint32_t k = 0; k < std::min(back->rounds, REP_TRACE); k++) line += " " + std::to_string(back->trace[k]);
        std::fprintf(stderr, "[hmk representatives] threshold %d: %u rounds, live edges behind each:%s\n", t, back->rounds, line.c_str());
    }
    return HMK_OK;
}

// The device side behind the edges: src names them (packed, on this context's device), total = their number.
int select_on_device(hmk_ctx *ctx, const EdgeRuns &src, uint64_t total, int thr, int thr_hi, const RepOut &o, hmk_representatives_stats &S) {
    const uint32_t n = ctx->n, nl = (uint32_t)(thr_hi - thr) + 1;
    int st = greedy_streams(ctx);
    if (st) return st;
    if (!ctx->h_loop) return fail(ctx, HMK_ERR_DEVICE, "no coherent pinned block for the rounds' progress word");
    hipStream_t Q = ctx->gstream;
    EventPair ev;
    HIPCHK(ctx, ev.create());
    HIPCHK(ctx, ev.start(Q));
    // a range: the whole edges by level, the top level first (the sweep's kernels and buffers)
    LevelPrefix back{};
    const uint64_t *dealt = nullptr;
    if (nl > 1) {
        st = deal_by_level(ctx, "representatives", Q, src, total, thr, thr_hi, nullptr, &back, &dealt);
        if (st) return st;
    }
    const uint64_t cap = std::max<uint64_t>(nl > 1 ? back.prefix[0] : total, 1);   // no level has more edges, no round keeps more
    HIPCHK(ctx, ensure_buf(ctx, SB_REP_STATE, sizeof(RepState)));
    HIPCHK(ctx, ensure_buf(ctx, SB_REP_VERT, rep_vertex_bytes(n)));
    HIPCHK(ctx, ensure_buf(ctx, SB_REP_LIVE, 2 * cap * sizeof(uint64_t)));
    RepState *rst = buf<RepState>(ctx, SB_REP_STATE);
    const RepVertex V = rep_vertex_arrays(buf<void>(ctx, SB_REP_VERT), n);
    uint64_t *live0 = buf<uint64_t>(ctx, SB_REP_LIVE), *live1 = live0 + cap;
    std::vector<hmk_representative_level> lv(nl);
    std::vector<uint32_t> near_scratch(o.nearest ? 0 : n), members;
    for (uint32_t l = nl; l-- > 0;) {
        const EdgeRuns E = nl > 1 ? edge_runs(dealt, 0, 1, &back.prefix[l]) : src;
        const uint64_t room = nl > 1 ? back.prefix[l] : total;
        uint32_t *near_row = o.nearest ? o.nearest + (size_t)l * n : near_scratch.data();
        RepState rb{};
        st = level_on_device(ctx, Q, E, room, thr + (int)l, V, rst, live0, live1, cap, o.covered_by ? o.covered_by + (size_t)l * n : nullptr, near_row,
                             o.nearest_score ? o.nearest_score + (size_t)l * n : nullptr, &rb);
        if (st) return st;
        lv[l] = level_record(n, nl > 1 ? back.prefix[l] : rb.n_edges, rb.n_rep, rb.n_isolated, rb.rounds, near_row, members);
    }
    HIPCHK(ctx, ev.stop(Q));
    HIPCHK(ctx, hipEventSynchronize(ev.b));
    float ms = 0;
    HIPCHK(ctx, ev.elapsed(&ms));
    S.select_ms = ms;
    fill_stats(S, lv);
    if (o.levels) std::copy(lv.begin(), lv.end(), o.levels);
    return HMK_OK;
}

int representatives_shifted(hmk_ctx *ctx, int X, int p, int thr, int thr_hi, const RepOut &o) {
    if (!ctx) return fail(nullptr, HMK_ERR_BAD_ARG, "null context");
    std::lock_guard<std::mutex> lock(ctx->mu);
    refresh_switches(ctx);
    int st = check_representatives(ctx, thr, thr_hi, o);
    if (st) return st;
    if (!ctx->symmetric)
        return fail(ctx, HMK_ERR_BAD_ARG, "representatives need a symmetric scoring matrix: a ~ b must not depend on which of the two is seq1");
    const uint32_t n = ctx->n, nl = (uint32_t)(thr_hi - thr) + 1;
    if (n == 0) return empty_set(nl, o);
    st = need_device(ctx);
    if (st) return st;
    hmk_representatives_stats S{};
    PassRuns P;
    st = pass_edge_runs(ctx, X, p, thr, true, &P);
    if (st) return st;
    S.kernel_ms = P.kernel_ms;
    S.pairs_scored = P.pairs_scored;
    st = select_on_device(ctx, P.E, P.total, thr, thr_hi, o, S);
    if (st == HMK_OK && o.stats) *o.stats = S;
    return st;
}

int representatives_from_edges_dev(hmk_ctx *ctx, const void *d_edges, uint64_t n_edges, int thr, int thr_hi, const RepOut &o) {
    if (!ctx) return fail(nullptr, HMK_ERR_BAD_ARG, "null context");
    std::lock_guard<std::mutex> lock(ctx->mu);
    refresh_switches(ctx);
    int st = check_representatives(ctx, thr, thr_hi, o);
    if (st) return st;
    st = check_edges_dev(ctx, d_edges, n_edges);
    if (st) return st;
    const uint32_t nl = (uint32_t)(thr_hi - thr) + 1;
    if (ctx->n == 0) return empty_set(nl, o);
    st = need_device(ctx);
    if (st) return st;
    // the caller's block may have been written on any stream of its own: wait for the device
    HIPCHK(ctx, hipDeviceSynchronize());
    hmk_representatives_stats S{};
    const unsigned long long cnt = n_edges;
    st = select_on_device(ctx, edge_runs((const uint64_t *)d_edges, 0, 1, &cnt), n_edges, thr, thr_hi, o, S);
    if (st == HMK_OK && o.stats) *o.stats = S;
    return st;
}

// The definition: the smaller neighbours of every vertex by counting, one walk in index order per level, one pass over the edges for
// covered_by and nearest.
int representatives_from_edges(hmk_ctx *ctx, const uint64_t *edges, uint64_t n_edges, int thr, int thr_hi, const RepOut &o) {
    if (!ctx) return fail(nullptr, HMK_ERR_BAD_ARG, "null context");
    std::lock_guard<std::mutex> lock(ctx->mu);
    refresh_switches(ctx);
    const int st = check_representatives(ctx, thr, thr_hi, o);
    if (st) return st;
    if (n_edges && !edges) return fail(ctx, HMK_ERR_BAD_ARG, "null edge list");
    const uint32_t n = ctx->n, nl = (uint32_t)(thr_hi - thr) + 1;
    std::vector<uint64_t> start((size_t)n + 1, 0);   // the smaller neighbours of i: lower[start[i] .. start[i + 1])
    for (uint64_t k = 0; k < n_edges; k++) {
        const uint32_t x = HMK_EDGE_X(edges[k]), m = HMK_EDGE_M(edges[k]);
        if (x >= n || m >= n || x == m) return fail(ctx, HMK_ERR_BAD_ARG, "edge list references a sequence outside [0, n) or a self pair");
        if (HMK_EDGE_SCORE(edges[k]) >= thr) start[std::max(x, m) + 1]++;
    }
    if (n == 0) return empty_set(nl, o);
    for (uint32_t i = 0; i < n; i++) start[i + 1] += start[i];
    struct Lower { uint32_t lo; int32_t score; };
    std::vector<Lower> lower(start[n]);
    {
        std::vector<uint64_t> at(start.begin(), start.end() - 1);
        for (uint64_t k = 0; k < n_edges; k++) {
            const uint32_t x = HMK_EDGE_X(edges[k]), m = HMK_EDGE_M(edges[k]);
            const int32_t sc = HMK_EDGE_SCORE(edges[k]);
            if (sc >= thr) lower[at[std::max(x, m)]++] = Lower{std::min(x, m), sc};
        }
    }
    std::vector<hmk_representative_level> lv(nl);
    std::vector<uint8_t> rep(n), touched(n);
    std::vector<uint32_t> cov(n), near(n), members;
    std::vector<int32_t> best(n);
    for (uint32_t l = 0; l < nl; l++) {
        const int t = thr + (int)l;
        for (uint32_t i = 0; i < n; i++) {
            rep[i] = 1;
            for (uint64_t k = start[i]; k < start[i + 1] && rep[i]; k++)
                if (lower[k].score >= t && rep[lower[k].lo]) rep[i] = 0;
        }
        uint32_t n_rep = 0, n_isolated = n;
        for (uint32_t i = 0; i < n; i++) {
            n_rep += rep[i];
            touched[i] = 0;
            cov[i] = near[i] = rep[i] ? i : 0xFFFFFFFFu;
            best[i] = rep[i] ? INT32_MAX : INT32_MIN;
        }
        uint64_t m_edges = 0;
        for (uint64_t k = 0; k < n_edges; k++) {
            const uint32_t x = HMK_EDGE_X(edges[k]), m = HMK_EDGE_M(edges[k]);
            const int32_t sc = HMK_EDGE_SCORE(edges[k]);
            if (sc < t) continue;
            m_edges++;
            for (uint32_t v : {x, m})
                if (!touched[v]) { touched[v] = 1; n_isolated--; }
            if (rep[x] == rep[m]) continue;   // (never both: the walk saw this edge)
            const uint32_t a = rep[x] ? x : m, b = rep[x] ? m : x;   // the representative, the other end
            cov[b] = std::min(cov[b], a);
            if (sc > best[b] || (sc == best[b] && a < near[b])) { best[b] = sc; near[b] = a; }
        }
        if (o.covered_by) std::copy(cov.begin(), cov.end(), o.covered_by + (size_t)l * n);
        if (o.nearest) std::copy(near.begin(), near.end(), o.nearest + (size_t)l * n);
        if (o.nearest_score) std::copy(best.begin(), best.end(), o.nearest_score + (size_t)l * n);
        lv[l] = level_record(n, m_edges, n_rep, n_isolated, 0, near.data(), members);
    }
    hmk_representatives_stats S{};
    fill_stats(S, lv);
    if (o.levels) std::copy(lv.begin(), lv.end(), o.levels);
    if (o.stats) *o.stats = S;
    return HMK_OK;
}

}  // namespace

} }  // namespace hmk::impl

extern "C" {

int hmk_representatives_shifted(hmk_ctx *ctx, int max_shift, int shift_penalty, int threshold, int threshold_hi, uint32_t *covered_by,
                                uint32_t *nearest, int32_t *nearest_score, hmk_representative_level *levels, hmk_representatives_stats *stats) {
    return representatives_shifted(ctx, max_shift, shift_penalty, threshold, threshold_hi, RepOut{covered_by, nearest, nearest_score, levels, stats});
}

int hmk_representatives_from_edges(hmk_ctx *ctx, const uint64_t *edges, uint64_t n_edges, int threshold, int threshold_hi, uint32_t *covered_by,
                                   uint32_t *nearest, int32_t *nearest_score, hmk_representative_level *levels, hmk_representatives_stats *stats) {
    return representatives_from_edges(ctx, edges, n_edges, threshold, threshold_hi, RepOut{covered_by, nearest, nearest_score, levels, stats});
}

int hmk_representatives_from_edges_dev(hmk_ctx *ctx, const void *d_edges, uint64_t n_edges, int threshold, int threshold_hi, uint32_t *covered_by,
                                       uint32_t *nearest, int32_t *nearest_score, hmk_representative_level *levels,
                                       hmk_representatives_stats *stats) {
    return representatives_from_edges_dev(ctx, d_edges, n_edges, threshold, threshold_hi, RepOut{covered_by, nearest, nearest_score, levels, stats});
}

}  // extern "C"
