// hmk_assign.cpp -- assignment of new sequences [q0, q1) to the existing clusters of the members [r0, r1) of the hmk_set_sequences
// set (NearestClusterRunner / findNearestClusterParallel, ClinkageSequenceClusterer.java:137-177, 243-294, with
// ClinkageClusterScorer.java:30-49).  The pass is the search's rectangle (hmk_plan.cpp) with the members on the side the planner
// emits as m = seq1, in the assignment's own plan slots; the aggregation per (new sequence, cluster) and the best-k selection run
// on the device (k_assign.hip); the extern "C" entry points.
#include "hmk_ctx.h"

namespace hmk { namespace impl {

namespace {

enum { ASSIGN_SHIFTED = 0, ASSIGN_LOCAL = 1 };

}  // namespace

// the checks of the clusters' description that the assignment and hmk_greedy_continue (hmk_continue.cpp) make before the device is
// looked at (a host-only context answers them too): members[c] = slot c's members, size[c] = its Cluster.size()
int check_clusters(hmk_ctx *ctx, const char *what, uint32_t q0, uint32_t q1, uint32_t r0, uint32_t r1, const uint32_t *member_cluster,
                   const int32_t *cluster_id, uint32_t n_clusters, std::vector<uint32_t> &members, std::vector<int64_t> &size) {
    if (q0 > q1 || r0 > r1 || q1 > ctx->n || r1 > ctx->n)
        return fail(ctx, HMK_ERR_BAD_ARG, std::string(what) + " ranges must lie within [0, n) with q0 <= q1 and r0 <= r1 (n = " + std::to_string(ctx->n) + ")");
    if (q0 < q1 && r0 < r1 && q0 < r1 && r0 < q1) return fail(ctx, HMK_ERR_BAD_ARG, "the new-sequence and member ranges overlap");
    const uint32_t nm = r1 - r0;
    if (nm && !member_cluster) return fail(ctx, HMK_ERR_BAD_ARG, "null member_cluster");
    if (n_clusters && !cluster_id) return fail(ctx, HMK_ERR_BAD_ARG, "null cluster_id");
    members.assign(n_clusters, 0);
    size.assign(n_clusters, 0);
    for (uint32_t i = 0; i < nm; i++) {
        const uint32_t c = member_cluster[i];
        if (c >= n_clusters)
            return fail(ctx, HMK_ERR_BAD_ARG, "member_cluster[" + std::to_string(i) + "] = " + std::to_string(c) + " is not a slot below n_clusters = " +
                                                  std::to_string(n_clusters));
        members[c]++;
        size[c] += ctx->has_sizes ? ctx->sizes[r0 + i] : 1;   // Cluster.size(): the members' UniqueSequence.size() (Cluster.java:156-158)
    }
    for (uint32_t c = 0; c < n_clusters; c++)
        if (!members[c]) return fail(ctx, HMK_ERR_BAD_ARG, "cluster slot " + std::to_string(c) + " has no member");
    {
        std::vector<int32_t> ids(cluster_id, cluster_id + n_clusters);
        std::sort(ids.begin(), ids.end());
        for (uint32_t c = 1; c < n_clusters; c++)
            if (ids[c] == ids[c - 1]) return fail(ctx, HMK_ERR_BAD_ARG, "cluster_id " + std::to_string(ids[c]) + " is given to two slots");
    }
    return HMK_OK;
}

int check_assign(hmk_ctx *ctx, const char *what, uint32_t q0, uint32_t q1, uint32_t r0, uint32_t r1, const uint32_t *member_cluster,
                 const int32_t *cluster_id, uint32_t n_clusters, uint32_t k, ClusterOrder *order) {
    if (k < 1 || k > 32) return fail(ctx, HMK_ERR_BAD_ARG, "k must be 1..32");
    std::vector<uint32_t> members;
    std::vector<int64_t> size;
    const int st = check_clusters(ctx, what, q0, q1, r0, r1, member_cluster, cluster_id, n_clusters, members, size);
    if (st) return st;
    order->slot_of_rank.resize(n_clusters);
    for (uint32_t c = 0; c < n_clusters; c++) order->slot_of_rank[c] = c;
    std::sort(order->slot_of_rank.begin(), order->slot_of_rank.end(), [&](uint32_t a, uint32_t b) {
        if (size[a] != size[b]) return size[a] > size[b];
        return cluster_id[a] < cluster_id[b];
    });
    order->rank_of.resize(n_clusters);
    order->members_of_rank.resize(n_clusters);
    for (uint32_t r = 0; r < n_clusters; r++) {
        order->rank_of[order->slot_of_rank[r]] = r;
        order->members_of_rank[r] = members[order->slot_of_rank[r]];
    }
    return HMK_OK;
}

// the pass of the rectangle members [r0, r1) x new [q0, q1) into ctx->edges, the members as the search's queries, which every
// tier emits as m = seq1 (hmk_plan.cpp), in the plan slots `pl` / `pll`; -> the shards' counts, their total, the stats
// (kernel_ms = the pass)
int cluster_pass(hmk_ctx *ctx, bool local, Plan &pl, PlanLocal &pll, int a, int b, int thr, uint32_t q0, uint32_t q1, uint32_t r0, uint32_t r1,
                 unsigned long long counts[HMK_EDGE_SHARDS], uint64_t *total, hmk_neighbor_stats *S) {
    int st = !local ? build_plan_search(ctx, pl, a, b, thr, r0, r1, q0, q1) : build_plan_local_search(ctx, pll, r0, r1, q0, q1);
    if (st) return st;
    double ms = 0;
    st = neighbors_grow(ctx, 0, counts, &ms, [&](uint64_t *d_edges, uint64_t cap, unsigned long long *d_counts) {
        return !local ? launch_plan(ctx, pl, a, b, thr, d_edges, cap, d_counts, nullptr)
                      : launch_plan_local(ctx, pll, SCORER_LOCAL, a, b, thr, d_edges, cap, d_counts, nullptr);
    });
    if (st) return st;
    *total = total_of(counts);
    if (!local) {
        *S = pl.stats;
    } else {
        S->pairs_scored = pll.pairs;
        S->n_tiles = pll.n_tiles;
    }
    S->n_edges = *total;
    S->kernel_ms = ms;
    return HMK_OK;
}

namespace {

int assign(hmk_ctx *ctx, int scorer, uint32_t q0, uint32_t q1, uint32_t r0, uint32_t r1, const uint32_t *member_cluster, const int32_t *cluster_id,
           uint32_t n_clusters, int a, int b, int thr, uint32_t k, uint32_t *best_cluster, int32_t *best_score, uint32_t *n_feasible,
           hmk_neighbor_stats *stats) {
    if (!ctx) return fail(nullptr, HMK_ERR_BAD_ARG, "null context");
    std::lock_guard<std::mutex> lock(ctx->mu);
    refresh_switches(ctx);
    ClusterOrder order;
    int st = check_assign(ctx, "assignment", q0, q1, r0, r1, member_cluster, cluster_id, n_clusters, k, &order);
    if (st) return st;
    const uint32_t nq = q1 - q0, nm = r1 - r0;
    if (nq && (!best_cluster || !best_score || !n_feasible)) return fail(ctx, HMK_ERR_BAD_ARG, "null output buffer");
    st = need_device(ctx);
    if (st) return st;
    hmk_neighbor_stats S{};
    S.symmetric = scorer == ASSIGN_SHIFTED && ctx->symmetric;
    if (nq == 0 || nm == 0) {
        for (uint64_t t = 0; t < (uint64_t)nq * k; t++) { best_cluster[t] = 0xFFFFFFFFu; best_score[t] = INT32_MIN; }
        for (uint32_t q = 0; q < nq; q++) n_feasible[q] = 0;
        if (stats) *stats = S;
        return HMK_OK;
    }
    st = scorer == ASSIGN_SHIFTED ? check_shifted(ctx, a, b, thr, q0, q1, r0, r1) : check_local_fits(ctx, a, b, thr);
    if (st) return st;

    // the clusters, once per call: member -> rank | members per rank | slot of each rank
    std::vector<uint32_t> cl((size_t)nm + 2 * (size_t)n_clusters);
    for (uint32_t i = 0; i < nm; i++) cl[i] = order.rank_of[member_cluster[i]];
    std::memcpy(cl.data() + nm, order.members_of_rank.data(), (size_t)n_clusters * 4);
    std::memcpy(cl.data() + nm + n_clusters, order.slot_of_rank.data(), (size_t)n_clusters * 4);
    HIPCHK(ctx, ensure_buf(ctx, SB_ASSIGN_CL, cl.size() * 4));
    uint32_t *d_cl = buf<uint32_t>(ctx, SB_ASSIGN_CL);
    HIPCHK(ctx, hipMemcpy(d_cl, cl.data(), cl.size() * 4, hipMemcpyHostToDevice));

    unsigned long long counts[HMK_EDGE_SHARDS];
    uint64_t total = 0;
    st = cluster_pass(ctx, scorer == ASSIGN_LOCAL, ctx->plan_assign, ctx->plan_local_assign, a, b, thr, q0, q1, r0, r1, counts, &total, &S);
    if (st) return st;
    const double ms = S.kernel_ms;
    if (total > 0xFFFFFFFFull) return fail(ctx, HMK_ERR_OOM, "more than 2^32 - 1 member hits above the threshold: raise the threshold");

    const uint64_t nk = (uint64_t)nq * k;
    HIPCHK(ctx, ensure_buf(ctx, SB_SEARCH_CNT, ((size_t)3 * nq + 1) * 4));
    HIPCHK(ctx, ensure_buf(ctx, SB_SEARCH_START, ((size_t)nq + 1) * 4));
    HIPCHK(ctx, ensure_buf(ctx, SB_SEARCH_SCAN, scan_scratch_bytes(nq)));
    HIPCHK(ctx, ensure_buf(ctx, SB_SEARCH_OUT, std::max<uint64_t>(total, 1) * sizeof(uint64_t)));
    HIPCHK(ctx, ensure_buf(ctx, SB_SEARCH_HITS, nk * 8 + (size_t)nq * 4));
    uint32_t *d_best = buf<uint32_t>(ctx, SB_SEARCH_HITS);
    int32_t *d_score = (int32_t *)(d_best + nk);
    uint32_t *d_nfeas = d_best + 2 * nk;
    EventPair ev;
    HIPCHK(ctx, ev.create());
    hipError_t e = ev.start(nullptr);
    if (e == hipSuccess)
        e = launch_assign(ctx->edges.d, ctx->edges.seg_cap(), ctx->edges.counts, max_of(counts), total, q0, nq, r0, nm, k, d_cl,
                          d_cl + nm, d_cl + nm + n_clusters, buf<uint32_t>(ctx, SB_SEARCH_CNT), buf<uint32_t>(ctx, SB_SEARCH_START),
                          buf<uint64_t>(ctx, SB_SEARCH_SCAN), buf<uint64_t>(ctx, SB_SEARCH_OUT), std::max<uint64_t>(total, 1), d_best, d_score,
                          d_nfeas, nullptr);
    if (e == hipSuccess) e = ev.stop(nullptr);
    if (e == hipSuccess) e = hipEventSynchronize(ev.b);
    float sel_ms = 0;
    if (e == hipSuccess) e = ev.elapsed(&sel_ms);
    if (e != hipSuccess) return fail_hip(ctx, "assignment", e);
    HIPCHK(ctx, hipMemcpy(best_cluster, d_best, nk * 4, hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(best_score, d_score, nk * 4, hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(n_feasible, d_nfeas, (size_t)nq * 4, hipMemcpyDeviceToHost));
    S.kernel_ms = ms + sel_ms;
    if (stats) *stats = S;
    return HMK_OK;
}

}  // namespace

} }  // namespace hmk::impl

extern "C" {

int hmk_assign_shifted(hmk_ctx *ctx, uint32_t q0, uint32_t q1, uint32_t r0, uint32_t r1, const uint32_t *member_cluster, const int32_t *cluster_id,
                       uint32_t n_clusters, int max_shift, int shift_penalty, int threshold, uint32_t k, uint32_t *best_cluster, int32_t *best_score,
                       uint32_t *n_feasible, hmk_neighbor_stats *stats) {
    return assign(ctx, ASSIGN_SHIFTED, q0, q1, r0, r1, member_cluster, cluster_id, n_clusters, max_shift, shift_penalty, threshold, k, best_cluster,
                  best_score, n_feasible, stats);
}

int hmk_assign_local(hmk_ctx *ctx, uint32_t q0, uint32_t q1, uint32_t r0, uint32_t r1, const uint32_t *member_cluster, const int32_t *cluster_id,
                     uint32_t n_clusters, int gap_open, int gap_extend, int threshold, uint32_t k, uint32_t *best_cluster, int32_t *best_score,
                     uint32_t *n_feasible, hmk_neighbor_stats *stats) {
    return assign(ctx, ASSIGN_LOCAL, q0, q1, r0, r1, member_cluster, cluster_id, n_clusters, gap_open, gap_extend, threshold, k, best_cluster,
                  best_score, n_feasible, stats);
}

}  // extern "C"
