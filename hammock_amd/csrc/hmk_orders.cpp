// hmk_orders.cpp -- the greedy clustering of the uploaded set under MANY orders from ONE scoring pass, and what makes several
// clusterings useful: the co-clustering support of every neighbouring pair, the stability of each sequence's company, the consensus
// clusters (hmk_greedy_orders*).  Replaces one LimitedGreedySequenceClusterer(scorer, threshold, maxClusters).cluster(list k)
// (LimitedGreedySequenceClusterer.java:22,39-69) per order k, list k = the set as UniqueSequence.sortSequences would hand it over
// under another -R: the scores do not depend on the order, only the tail does.
//   pass      pass_edge_runs (hmk_levels.cpp): hmk_neighbors_shifted's (neighbors_internal: the all-vs-all plan slot, the same kernels) at
//             `threshold` into the context's edge buffer, grown until it fits;
//   relabel   per order k_orders_relabel: the edges renamed to the order's positions (SB_ORD_EDGES), the 16 score bits copied;
//   tail      per order the clustering tail as it is (cluster_on_device) on an EdgeSource of one segment, with Cluster.size() read
//             through the order's permuted view (hmk_ctx::sizes_view); the rows mapped back to uploaded indices on the host;
//   support   once, k_orders_support over the ORIGINAL edges with the valid orders' cluster ids transposed (SB_ORD_IDS);
//   consensus k_components.hip's union-find (hmk_cc_device.h) straight over the support edges at min_support, flatten, count.
// hmk_greedy_orders_from_edges is the same answer on the host: relabel, hmk_greedy_from_edges's merge per order, supports by a loop,
// a sequential union-find -- the second implementation the device path is tested against, and what a host-only context runs.
#include "hmk_levels.h"
#include "hmk_components.h"
#include "hmk_orders.h"

namespace hmk { namespace impl {

namespace {

struct OrdersOut {
    int32_t *cluster_id, *result_order, *member_rank;   // each [n_orders][n] or null
    hmk_greedy_order *per_order;                         // [n_orders] or null
    uint32_t *partners_always, *partners_ever, *consensus;   // [n] each or null
    uint64_t *support_edges;
    uint64_t capacity;
    uint64_t *n_support_edges;
    hmk_greedy_orders_stats *stats;
};

// the argument checks both entry points make before the device is looked at
int check_orders(hmk_ctx *ctx, const uint32_t *orders, uint32_t n_orders, uint32_t min_support, const OrdersOut &o) {
    if (n_orders < 1 || n_orders > ORDERS_MAX) return fail(ctx, HMK_ERR_BAD_ARG, "n_orders must be within 1 .. 256");
    if (!orders) return fail(ctx, HMK_ERR_BAD_ARG, "null orders");
    if (!o.stats) return fail(ctx, HMK_ERR_BAD_ARG, "null stats");
    if (min_support > n_orders) return fail(ctx, HMK_ERR_BAD_ARG, "min_support is above n_orders");
    if (!o.support_edges && o.capacity) return fail(ctx, HMK_ERR_BAD_ARG, "null support_edges with a capacity");
    const uint32_t n = ctx->n;
    if (n && !o.cluster_id && !o.result_order && !o.member_rank && !o.per_order && !o.partners_always && !o.partners_ever && !o.consensus &&
        !o.support_edges)
        return fail(ctx, HMK_ERR_BAD_ARG, "null outputs (the rows, per_order, the partner counts, consensus and support_edges)");
    std::vector<uint8_t> seen(n);
    for (uint32_t k = 0; k < n_orders; k++) {
        std::fill(seen.begin(), seen.end(), 0);
        for (uint32_t pos = 0; pos < n; pos++) {
            const uint32_t i = orders[(size_t)k * n + pos];
            if (i >= n || seen[i]) return fail(ctx, HMK_ERR_BAD_ARG, "order " + std::to_string(k) + " is not a permutation of [0, n)");
            seen[i] = 1;
        }
    }
    if (!ctx->symmetric)
        return fail(ctx, HMK_ERR_BAD_ARG, "orders need a symmetric scoring matrix: the pass scores one orientation of a pair, and which "
                                          "of the two is seq1 would depend on the order");
    return HMK_OK;
}

// no sequences: cluster() of an empty list returns an empty list in every order
int empty_set(uint32_t n_orders, const OrdersOut &o) {
    if (o.per_order) std::fill(o.per_order, o.per_order + n_orders, hmk_greedy_order{});
    *o.stats = hmk_greedy_orders_stats{};
    o.stats->n_orders = o.stats->n_valid = n_orders;
    if (o.n_support_edges) *o.n_support_edges = 0;
    return HMK_OK;
}

// What a call gathers over its orders, on either path.
struct OrdersRun {
    uint32_t n = 0, n_orders = 0;
    std::vector<int32_t> ids_own;        // the cluster ids of every order where the caller wants no cluster_id rows
    int32_t *ids = nullptr;              // [n_orders][n], by uploaded index
    std::vector<hmk_greedy_order> ord;   // [n_orders]
    std::vector<uint32_t> valid;         // the orders in which the reference does not throw, ascending
    std::vector<uint32_t> pos, members;  // scratch: an order's inverse permutation; members per seed
    std::vector<int32_t> psz, r_id, r_order, r_rank;   // scratch: the order's sizes and its rows by position

    void init(const hmk_ctx *ctx, uint32_t k_orders, const OrdersOut &o) {
        n = ctx->n;
        n_orders = k_orders;
        if (!o.cluster_id) ids_own.resize((size_t)n_orders * n);
        ids = o.cluster_id ? o.cluster_id : ids_own.data();
        ord.assign(n_orders, hmk_greedy_order{});
        pos.resize(n);
        r_id.resize(n);
        r_order.resize(n);
        r_rank.resize(n);
        if (ctx->has_sizes) psz.resize(n);
    }
    // order k's inverse permutation and sizes; the position rows as a clustering leaves them alone: -1
    void begin(const hmk_ctx *ctx, const uint32_t *order) {
        for (uint32_t p = 0; p < n; p++) {
            pos[order[p]] = p;
            if (ctx->has_sizes) psz[p] = ctx->sizes[order[p]];
        }
        std::fill(r_order.begin(), r_order.end(), -1);
    }
    // Order k's rows behind its clustering (st: HMK_OK or HMK_ERR_REFERENCE_WOULD_CRASH), mapped back to uploaded indices: a cluster
    // is named by the uploaded index of its seed.  An order where the reference would throw keeps the failure and -1 rows.
    void finish(uint32_t k, const uint32_t *order, const OrdersOut &o, int st, const hmk_greedy_stats &gs, double ms) {
        const bool crash = st == HMK_ERR_REFERENCE_WOULD_CRASH;
        hmk_greedy_order &L = ord[k];
        L.status = st;
        L.crash_case = gs.crash_case;
        L.crash_index = gs.crash_index;
        L.phase1_stop_index = gs.phase1_stop_index;
        L.phase1_clusters = gs.phase1_clusters;
        L.phase1_orphans = gs.phase1_orphans;
        L.n_result_clusters = gs.n_result_clusters;
        L.n_multi = gs.n_multi;
        L.tail_ms = ms;
        int32_t *cid = ids + (size_t)k * n;
        int32_t *ro = o.result_order ? o.result_order + (size_t)k * n : nullptr, *mr = o.member_rank ? o.member_rank + (size_t)k * n : nullptr;
        if (crash) {
            std::fill(cid, cid + n, -1);
            if (ro) std::fill(ro, ro + n, -1);
            if (mr) std::fill(mr, mr + n, -1);
            return;
        }
        valid.push_back(k);
        members.assign(n, 0);
        for (uint32_t p = 0; p < n; p++) {
            const uint32_t seed = order[(uint32_t)r_id[p]];
            cid[order[p]] = (int32_t)seed;
            members[seed]++;
            if (mr) mr[order[p]] = r_rank[p];
            if (ro) ro[p] = r_order[p] >= 0 ? (int32_t)order[(uint32_t)r_order[p]] : -1;
        }
        for (uint32_t c = 0; c < n; c++) {
            L.n_singletons += members[c] == 1;
            L.largest = std::max(L.largest, members[c]);
        }
    }
    // an upper bound of the pairs with support >= 1: the pairs inside one cluster, summed over the valid orders
    uint64_t pairs_bound() {
        uint64_t sum = 0;
        for (uint32_t k : valid) {
            members.assign(n, 0);
            for (uint32_t i = 0; i < n; i++) members[(uint32_t)ids[(size_t)k * n + i]]++;
            for (uint32_t c = 0; c < n; c++) sum += (uint64_t)members[c] * (members[c] ? members[c] - 1 : 0) / 2;
        }
        return sum;
    }
    // the valid orders' cluster ids transposed: [n][n_valid]
    std::vector<int32_t> transposed() const {
        const size_t nv = valid.size();
        std::vector<int32_t> t((size_t)n * nv);
        for (size_t v = 0; v < nv; v++) {
            const int32_t *row = ids + (size_t)valid[v] * n;
            for (uint32_t i = 0; i < n; i++) t[(size_t)i * nv + v] = row[i];
        }
        return t;
    }
};

// what the consensus of a call without a valid order is: every sequence alone, nobody has a partner
void no_valid_order(uint32_t n, const OrdersOut &o, hmk_greedy_orders_stats &S) {
    for (uint32_t i = 0; i < n; i++) {
        if (o.partners_always) o.partners_always[i] = 0;
        if (o.partners_ever) o.partners_ever[i] = 0;
        if (o.consensus) o.consensus[i] = i;
    }
    S.n_consensus = S.n_consensus_singletons = n;
    S.consensus_largest = n ? 1 : 0;
}

// the outputs every exit of a finished call writes; HMK_ERR_CAPACITY when the support edges did not fit
int deliver(hmk_ctx *ctx, const OrdersRun &R, const OrdersOut &o, const hmk_greedy_orders_stats &S) {
    if (o.per_order) std::copy(R.ord.begin(), R.ord.end(), o.per_order);
    *o.stats = S;
    if (o.n_support_edges) *o.n_support_edges = S.pairs_ever;
    if (o.support_edges && S.pairs_ever > o.capacity)
        return fail(ctx, HMK_ERR_CAPACITY, "support edge buffer too small: " + std::to_string(S.pairs_ever) + " needed");
    return HMK_OK;
}

// the tail's sizes are the running order's while this lives; the context's own are what they were on every exit path
struct SizesView {
    hmk_ctx *ctx;
    explicit SizesView(hmk_ctx *c) : ctx(c) {}
    ~SizesView() { ctx->sizes_view = nullptr; }
};

int greedy_orders(hmk_ctx *ctx, int X, int p, int thr, int max_clusters, const uint32_t *orders, uint32_t n_orders, uint32_t min_support,
                  const OrdersOut &o) {
    if (!ctx) return fail(nullptr, HMK_ERR_BAD_ARG, "null context");
    std::lock_guard<std::mutex> lock(ctx->mu);
    refresh_switches(ctx);
    int st = check_orders(ctx, orders, n_orders, min_support, o);
    if (st) return st;
    const uint32_t n = ctx->n;
    if (n == 0) return empty_set(n_orders, o);
    st = need_device(ctx);
    if (st) return st;
    hmk_greedy_orders_stats S{};
    S.n_orders = n_orders;
    PassRuns P;
    st = pass_edge_runs(ctx, X, p, thr, true, &P);
    if (st) return st;
    S.kernel_ms = P.kernel_ms;
    S.pairs_scored = P.pairs_scored;
    const EdgeRuns &E = P.E;
    const uint64_t total = P.total;
    S.n_edges = total;
    OrderRuns runs{};   // the runs back to back in the renamed buffer
    for (uint32_t s = 1; s < E.n_runs; s++) runs.off[s] = runs.off[s - 1] + E.count[s - 1];
    st = greedy_streams(ctx);
    if (st) return st;
    hipStream_t Q = ctx->gstream;
    HIPCHK(ctx, ensure_buf(ctx, SB_ORD_STATE, sizeof(OrdersState)));
    HIPCHK(ctx, ensure_buf(ctx, SB_ORD_EDGES, std::max<uint64_t>(total, 1) * sizeof(uint64_t)));
    HIPCHK(ctx, ensure_buf(ctx, SB_ORD_POS, (size_t)n * sizeof(uint32_t)));
    OrdersState *state = buf<OrdersState>(ctx, SB_ORD_STATE);
    uint64_t *renamed = buf<uint64_t>(ctx, SB_ORD_EDGES);
    uint32_t *d_pos = buf<uint32_t>(ctx, SB_ORD_POS);
    const unsigned long long total_word = total;
    HIPCHK(ctx, hipMemsetAsync(state, 0, sizeof(OrdersState), Q));
    HIPCHK(ctx, hipMemcpyAsync(&state->total, &total_word, sizeof(total_word), hipMemcpyHostToDevice, Q));
    HIPCHK(ctx, hipStreamSynchronize(Q));
    EventPair ev;
    HIPCHK(ctx, ev.create());

    OrdersRun R;
    R.init(ctx, n_orders, o);
    SizesView view(ctx);
    for (uint32_t k = 0; k < n_orders; k++) {
        const auto t0 = std::chrono::steady_clock::now();
        const uint32_t *order = orders + (size_t)k * n;
        R.begin(ctx, order);
        HIPCHK(ctx, hipMemcpyAsync(d_pos, R.pos.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, Q));
        HIPCHK(ctx, ev.start(Q));
        HIPCHK(ctx, launch_orders_relabel(E, runs, n, d_pos, renamed, state, Q));
        HIPCHK(ctx, ev.stop(Q));
        // the tail takes the renamed edges as one segment whose count is the state's `total`, in device memory
        const bool packed = adjacency_packed(ctx, X, p, thr);
        const EdgeSource src = one_segment_source(renamed, &state->total, total, true, &packed, thr);
        ctx->phases = hmk_greedy_phases{};
        HIPCHK(ctx, hipEventRecord(ctx->ev_t0, Q));
        HIPCHK(ctx, hipEventRecord(ctx->ev_edges, Q));
        ctx->sizes_view = ctx->has_sizes ? R.psz.data() : nullptr;
        hmk_greedy_stats gs{};
        st = cluster_on_device(ctx, src, max_clusters, R.r_id.data(), R.r_order.data(), R.r_rank.data(), &gs, t0);
        ctx->sizes_view = nullptr;
        if (st == ST_RETRY_OVERFLOW) return fail(ctx, HMK_ERR_DEVICE, "greedy orders: an order's segment overflowed");
        if (st != HMK_OK && st != HMK_ERR_REFERENCE_WOULD_CRASH) return st;
        float ms = 0;
        HIPCHK(ctx, hipEventSynchronize(ev.b));
        HIPCHK(ctx, ev.elapsed(&ms));
        S.relabel_ms += ms;
        R.finish(k, order, o, st, gs, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    const uint32_t nv = (uint32_t)R.valid.size();
    S.n_valid = nv;
    if (nv == 0) {
        no_valid_order(n, o, S);
        return deliver(ctx, R, o, S);
    }

    // ---- support and consensus
    const uint32_t level = min_support ? std::min(min_support, nv) : nv;   // (a level above n_valid: no pair reaches it -- as n_valid + 1 would)
    const bool unreachable = min_support > nv;
    const uint64_t room = std::min<uint64_t>(total, R.pairs_bound());
    const std::vector<int32_t> idsT = R.transposed();
    HIPCHK(ctx, ensure_buf(ctx, SB_ORD_IDS, idsT.size() * sizeof(int32_t)));
    HIPCHK(ctx, ensure_buf(ctx, SB_ORD_SUPPORT, std::max<uint64_t>(room, 1) * sizeof(uint64_t)));
    HIPCHK(ctx, ensure_buf(ctx, SB_ORD_PARTNERS, (size_t)n * 2 * sizeof(uint32_t)));
    HIPCHK(ctx, ensure_buf(ctx, SB_CC_PARENT, (size_t)n * sizeof(uint32_t)));
    HIPCHK(ctx, ensure_buf(ctx, SB_CC_SIZE, (size_t)n * sizeof(uint32_t)));
    HIPCHK(ctx, ensure_buf(ctx, SB_CC_STATE, sizeof(CcState)));
    int32_t *d_ids = buf<int32_t>(ctx, SB_ORD_IDS);
    uint64_t *d_support = buf<uint64_t>(ctx, SB_ORD_SUPPORT);
    uint32_t *d_ever = buf<uint32_t>(ctx, SB_ORD_PARTNERS), *d_always = d_ever + n;
    uint32_t *parent = buf<uint32_t>(ctx, SB_CC_PARENT), *size = buf<uint32_t>(ctx, SB_CC_SIZE);
    CcState *cc = buf<CcState>(ctx, SB_CC_STATE);
    struct { unsigned long long n_support, n_always, total, flag; } back;
    static_assert(offsetof(OrdersState, flag) == offsetof(OrdersState, n_support) + 3 * sizeof(unsigned long long), "the counters and the flag are read in one copy");
    HIPCHK(ctx, hipMemcpyAsync(d_ids, idsT.data(), idsT.size() * sizeof(int32_t), hipMemcpyHostToDevice, Q));
    HIPCHK(ctx, ev.start(Q));
    HIPCHK(ctx, hipMemsetAsync(d_ever, 0, (size_t)n * 2 * sizeof(uint32_t), Q));
    HIPCHK(ctx, hipMemsetAsync(cc, 0, sizeof(CcState), Q));
    HIPCHK(ctx, launch_cc_init(parent, size, n, Q));
    HIPCHK(ctx, launch_orders_support(E, n, d_ids, nv, d_support, room, d_ever, d_always, state, Q));
    HIPCHK(ctx, hipMemcpyAsync(&back, &state->n_support, sizeof(back), hipMemcpyDeviceToHost, Q));
    HIPCHK(ctx, hipStreamSynchronize(Q));
    if (back.flag) return fail(ctx, HMK_ERR_DEVICE, "greedy orders: the pass left an edge outside [0, n) or a self pair");
    if (back.n_support > room) return fail(ctx, HMK_ERR_DEVICE, "greedy orders: more support edges than pairs inside clusters");
    // the consensus: the support edges are HMK_EDGE_* edges with the support as their score -- k_components.hip's single-level union at
    // `level`, flatten, count (the host knows their number now)
    const unsigned long long n_united = unreachable ? 0 : back.n_support;
    HIPCHK(ctx, launch_cc_union_edges(edge_runs(d_support, 0, 1, &n_united), n, (int)level, parent, cc, Q));
    HIPCHK(ctx, launch_cc_flatten(parent, size, n, Q));
    HIPCHK(ctx, launch_cc_sizes(size, n, 0, cc, Q));
    HIPCHK(ctx, ev.stop(Q));
    hmk_component_level lv{};
    std::vector<unsigned long long> sums((size_t)2 * ORDERS_MAX);
    HIPCHK(ctx, hipMemcpyAsync(&lv, &cc->levels[0], sizeof(lv), hipMemcpyDeviceToHost, Q));
    HIPCHK(ctx, hipMemcpyAsync(sums.data(), state->together, sums.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, Q));
    static_assert(offsetof(OrdersState, with_first) == ORDERS_MAX * sizeof(unsigned long long), "together and with_first are read in one copy");
    if (o.consensus) HIPCHK(ctx, hipMemcpyAsync(o.consensus, parent, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, Q));
    if (o.partners_ever) HIPCHK(ctx, hipMemcpyAsync(o.partners_ever, d_ever, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, Q));
    if (o.partners_always) HIPCHK(ctx, hipMemcpyAsync(o.partners_always, d_always, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, Q));
    if (o.support_edges && back.n_support <= o.capacity && back.n_support)
        HIPCHK(ctx, hipMemcpyAsync(o.support_edges, d_support, back.n_support * sizeof(uint64_t), hipMemcpyDeviceToHost, Q));
    HIPCHK(ctx, hipStreamSynchronize(Q));
    float ms = 0;
    HIPCHK(ctx, ev.elapsed(&ms));
    S.support_ms = ms;
    if (lv.reserved) return fail(ctx, HMK_ERR_DEVICE, "greedy orders: a support edge outside [0, n) or a self pair");
    for (uint32_t v = 0; v < nv; v++) {
        R.ord[R.valid[v]].pairs_together = sums[v];
        R.ord[R.valid[v]].pairs_with_first = sums[ORDERS_MAX + v];
    }
    S.pairs_ever = back.n_support;
    S.pairs_always = back.n_always;
    S.n_consensus = n - lv.n_components;   // (the device counted the hooks)
    S.n_consensus_singletons = lv.n_singletons;
    S.consensus_largest = lv.largest;
    return deliver(ctx, R, o, S);
}

// Plain host code: relabel, hmk_greedy_from_edges's merge per order, supports by a loop, a sequential union-find.
int greedy_orders_from_edges(hmk_ctx *ctx, const uint64_t *edges, uint64_t n_edges, int thr, int max_clusters, const uint32_t *orders,
                             uint32_t n_orders, uint32_t min_support, const OrdersOut &o) {
    if (!ctx) return fail(nullptr, HMK_ERR_BAD_ARG, "null context");
    std::lock_guard<std::mutex> lock(ctx->mu);
    refresh_switches(ctx);
    int st = check_orders(ctx, orders, n_orders, min_support, o);
    if (st) return st;
    if (n_edges && !edges) return fail(ctx, HMK_ERR_BAD_ARG, "null edge list");
    const uint32_t n = ctx->n;
    std::vector<uint64_t> kept;   // the edges at or above the threshold, x < m
    for (uint64_t e = 0; e < n_edges; e++) {
        const uint32_t x = HMK_EDGE_X(edges[e]), m = HMK_EDGE_M(edges[e]);
        if (x >= n || m >= n || x == m) return fail(ctx, HMK_ERR_BAD_ARG, "edge list references a sequence outside [0, n) or a self pair");
        if (HMK_EDGE_SCORE(edges[e]) < thr) continue;
        kept.push_back((uint64_t)std::min(x, m) << 40 | (uint64_t)std::max(x, m) << 16 | (edges[e] & 0xFFFFull));
    }
    if (n == 0) return empty_set(n_orders, o);
    hmk_greedy_orders_stats S{};
    S.n_orders = n_orders;
    S.n_edges = kept.size();
    OrdersRun R;
    R.init(ctx, n_orders, o);
    std::vector<uint64_t> renamed(kept.size());
    const GreedyOptions opt = greedy_options(ctx);
    for (uint32_t k = 0; k < n_orders; k++) {
        const auto t0 = std::chrono::steady_clock::now();
        const uint32_t *order = orders + (size_t)k * n;
        R.begin(ctx, order);
        for (size_t e = 0; e < kept.size(); e++) {
            const uint32_t a = R.pos[HMK_EDGE_X(kept[e])], b = R.pos[HMK_EDGE_M(kept[e])];
            renamed[e] = (uint64_t)std::min(a, b) << 40 | (uint64_t)std::max(a, b) << 16 | (kept[e] & 0xFFFFull);
        }
        hmk_greedy_stats gs{};
        std::string err;
        st = greedy_from_edges(n, ctx->has_sizes ? R.psz.data() : nullptr, renamed.data(), renamed.size(), true, thr, max_clusters, R.r_id.data(),
                               R.r_order.data(), R.r_rank.data(), &gs, &err, opt);
        if (st != HMK_OK && st != HMK_ERR_REFERENCE_WOULD_CRASH) return fail(ctx, st, err);
        R.finish(k, order, o, st, gs, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    const uint32_t nv = (uint32_t)R.valid.size();
    S.n_valid = nv;
    if (nv == 0) {
        no_valid_order(n, o, S);
        return deliver(ctx, R, o, S);
    }
    const uint32_t level = min_support ? min_support : nv;
    std::vector<uint32_t> parent(n), ever(n, 0), always(n, 0);
    std::iota(parent.begin(), parent.end(), 0u);
    auto find = [&](uint32_t v) {
        while (parent[v] != v) {
            parent[v] = parent[parent[v]];
            v = parent[v];
        }
        return v;
    };
    const int32_t *first = R.ids + (size_t)R.valid[0] * n;
    for (uint64_t w : kept) {
        const uint32_t x = HMK_EDGE_X(w), m = HMK_EDGE_M(w);
        uint32_t sup = 0;
        for (uint32_t k : R.valid) {
            const int32_t *row = R.ids + (size_t)k * n;
            if (row[x] != row[m]) continue;
            sup++;
            R.ord[k].pairs_together++;
            if (first[x] == first[m]) R.ord[k].pairs_with_first++;
        }
        if (!sup) continue;
        if (o.support_edges && S.pairs_ever < o.capacity) o.support_edges[S.pairs_ever] = (uint64_t)x << 40 | (uint64_t)m << 16 | sup;
        S.pairs_ever++;
        ever[x]++;
        ever[m]++;
        if (sup == nv) {
            S.pairs_always++;
            always[x]++;
            always[m]++;
        }
        if (sup >= level) {
            uint32_t a = find(x), b = find(m);
            if (a == b) continue;
            if (a > b) std::swap(a, b);
            parent[b] = a;   // a root is its tree's smallest index
        }
    }
    std::vector<uint32_t> members(n, 0);
    for (uint32_t v = 0; v < n; v++) {
        const uint32_t r = find(v);
        members[r]++;
        if (o.consensus) o.consensus[v] = r;
    }
    for (uint32_t c = 0; c < n; c++) {
        S.n_consensus += members[c] > 0;
        S.n_consensus_singletons += members[c] == 1;
        S.consensus_largest = std::max(S.consensus_largest, members[c]);
    }
    if (o.partners_ever) std::copy(ever.begin(), ever.end(), o.partners_ever);
    if (o.partners_always) std::copy(always.begin(), always.end(), o.partners_always);
    return deliver(ctx, R, o, S);
}

}  // namespace

} }  // namespace hmk::impl

extern "C" {

int hmk_greedy_orders(hmk_ctx *ctx, int max_shift, int shift_penalty, int threshold, int max_clusters, const uint32_t *orders, uint32_t n_orders,
                      uint32_t min_support, int32_t *cluster_id, int32_t *result_order, int32_t *member_rank, hmk_greedy_order *per_order,
                      uint32_t *partners_always, uint32_t *partners_ever, uint32_t *consensus, uint64_t *support_edges, uint64_t capacity,
                      uint64_t *n_support_edges, hmk_greedy_orders_stats *stats) {
    return greedy_orders(ctx, max_shift, shift_penalty, threshold, max_clusters, orders, n_orders, min_support,
                         OrdersOut{cluster_id, result_order, member_rank, per_order, partners_always, partners_ever, consensus, support_edges, capacity,
                                   n_support_edges, stats});
}

int hmk_greedy_orders_from_edges(hmk_ctx *ctx, const uint64_t *edges, uint64_t n_edges, int threshold, int max_clusters, const uint32_t *orders,
                                 uint32_t n_orders, uint32_t min_support, int32_t *cluster_id, int32_t *result_order, int32_t *member_rank,
                                 hmk_greedy_order *per_order, uint32_t *partners_always, uint32_t *partners_ever, uint32_t *consensus,
                                 uint64_t *support_edges, uint64_t capacity, uint64_t *n_support_edges, hmk_greedy_orders_stats *stats) {
    return greedy_orders_from_edges(ctx, edges, n_edges, threshold, max_clusters, orders, n_orders, min_support,
                                    OrdersOut{cluster_id, result_order, member_rank, per_order, partners_always, partners_ever, consensus,
                                              support_edges, capacity, n_support_edges, stats});
}

}  // extern "C"
