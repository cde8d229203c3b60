// hmk_match.cpp -- match of query clusters (sequences [q0, q1) in query slots) to the existing clusters of the members [r0, r1)
// of the hmk_set_sequences set: ClinkageClusterScorer.clusterScore(existing cluster, query cluster) (ClinkageClusterScorer.java
// :30-49) ranked as findNearestClusterParallel ranks it (ClinkageSequenceClusterer.java:137-177, 258-293), for every query cluster
// at once.  The pass is the assignment's rectangle (hmk_assign.cpp) in the match's own plan slots; the two-level aggregation and
// the best-k selection run on the device (k_match.hip); the extern "C" entry points.
#include "hmk_ctx.h"

namespace hmk { namespace impl {

namespace {

enum { MATCH_SHIFTED = 0, MATCH_LOCAL = 1 };

// the query side's checks (after the assignment's): query_members[b] = members of query slot b
int check_queries(hmk_ctx *ctx, uint32_t nq, const uint32_t *query_cluster, uint32_t n_query_clusters, std::vector<uint32_t> &query_members) {
    if (nq && !query_cluster) return fail(ctx, HMK_ERR_BAD_ARG, "null query_cluster");
    query_members.assign(n_query_clusters, 0);
    for (uint32_t i = 0; i < nq; i++) {
        const uint32_t b = query_cluster[i];
        if (b >= n_query_clusters)
            return fail(ctx, HMK_ERR_BAD_ARG, "query_cluster[" + std::to_string(i) + "] = " + std::to_string(b) +
                                                  " is not a slot below n_query_clusters = " + std::to_string(n_query_clusters));
        query_members[b]++;
    }
    for (uint32_t b = 0; b < n_query_clusters; b++)
        if (!query_members[b]) return fail(ctx, HMK_ERR_BAD_ARG, "query cluster slot " + std::to_string(b) + " has no member");
    return HMK_OK;
}

int match(hmk_ctx *ctx, int scorer, uint32_t q0, uint32_t q1, const uint32_t *query_cluster, uint32_t n_query_clusters, uint32_t r0, uint32_t r1,
          const uint32_t *member_cluster, const int32_t *cluster_id, uint32_t n_clusters, int a, int b, int thr, uint32_t k, uint32_t *best_cluster,
          int32_t *best_score, uint32_t *n_feasible, hmk_neighbor_stats *stats) {
    if (!ctx) return fail(nullptr, HMK_ERR_BAD_ARG, "null context");
    std::lock_guard<std::mutex> lock(ctx->mu);
    refresh_switches(ctx);
    ClusterOrder order;
    int st = check_assign(ctx, "match", q0, q1, r0, r1, member_cluster, cluster_id, n_clusters, k, &order);
    if (st) return st;
    const uint32_t nq = q1 - q0, nm = r1 - r0, nb = n_query_clusters;
    std::vector<uint32_t> query_members;
    st = check_queries(ctx, nq, query_cluster, nb, query_members);
    if (st) return st;
    if (nb && (!best_cluster || !best_score || !n_feasible)) return fail(ctx, HMK_ERR_BAD_ARG, "null output buffer");
    st = need_device(ctx);
    if (st) return st;
    hmk_neighbor_stats S{};
    S.symmetric = scorer == MATCH_SHIFTED && ctx->symmetric;
    if (nq == 0 || nm == 0) {
        for (uint64_t t = 0; t < (uint64_t)nb * k; t++) { best_cluster[t] = 0xFFFFFFFFu; best_score[t] = INT32_MIN; }
        for (uint32_t c = 0; c < nb; c++) n_feasible[c] = 0;
        if (stats) *stats = S;
        return HMK_OK;
    }
    st = scorer == MATCH_SHIFTED ? check_shifted(ctx, a, b, thr, q0, q1, r0, r1) : check_local_fits(ctx, a, b, thr);
    if (st) return st;

    // the clusters, once per call: member -> rank | members per rank | slot of each rank | query member -> query slot | members
    // per query slot
    std::vector<uint32_t> cl((size_t)nm + 2 * (size_t)n_clusters + nq + nb);
    uint32_t *h = cl.data();
    for (uint32_t i = 0; i < nm; i++) h[i] = order.rank_of[member_cluster[i]];
    std::memcpy(h + nm, order.members_of_rank.data(), (size_t)n_clusters * 4);
    std::memcpy(h + nm + n_clusters, order.slot_of_rank.data(), (size_t)n_clusters * 4);
    std::memcpy(h + nm + 2 * (size_t)n_clusters, query_cluster, (size_t)nq * 4);
    std::memcpy(h + nm + 2 * (size_t)n_clusters + nq, query_members.data(), (size_t)nb * 4);
    HIPCHK(ctx, ensure_buf(ctx, SB_MATCH_CL, cl.size() * 4));
    uint32_t *d_cl = buf<uint32_t>(ctx, SB_MATCH_CL);
    HIPCHK(ctx, hipMemcpy(d_cl, cl.data(), cl.size() * 4, hipMemcpyHostToDevice));

    unsigned long long counts[HMK_EDGE_SHARDS];
    uint64_t total = 0;
    st = cluster_pass(ctx, scorer == MATCH_LOCAL, ctx->plan_match, ctx->plan_local_match, a, b, thr, q0, q1, r0, r1, counts, &total, &S);
    if (st) return st;
    const double ms = S.kernel_ms;
    if (total > 0xFFFFFFFFull) return fail(ctx, HMK_ERR_OOM, "more than 2^32 - 1 member hits above the threshold: raise the threshold");

    const uint64_t nk = (uint64_t)nb * k, cap = std::max<uint64_t>(total, 1);
    HIPCHK(ctx, ensure_buf(ctx, SB_SEARCH_CNT, ((size_t)3 * nq + 1) * 4));
    HIPCHK(ctx, ensure_buf(ctx, SB_SEARCH_START, ((size_t)nq + 1) * 4));
    HIPCHK(ctx, ensure_buf(ctx, SB_SEARCH_SCAN, scan_scratch_bytes(std::max(nq, nb))));
    HIPCHK(ctx, ensure_buf(ctx, SB_SEARCH_OUT, cap * sizeof(uint64_t)));
    HIPCHK(ctx, ensure_buf(ctx, SB_MATCH_REC, cap * sizeof(uint64_t)));
    HIPCHK(ctx, ensure_buf(ctx, SB_MATCH_SCR, ((size_t)nq + 4 * (size_t)nb + 2) * 4));
    HIPCHK(ctx, ensure_buf(ctx, SB_SEARCH_HITS, nk * 8 + (size_t)nb * 4));
    uint32_t *d_best = buf<uint32_t>(ctx, SB_SEARCH_HITS);
    int32_t *d_score = (int32_t *)(d_best + nk);
    uint32_t *d_nfeas = d_best + 2 * nk;
    uint32_t *d_scr2 = buf<uint32_t>(ctx, SB_MATCH_SCR);
    EventPair ev;
    HIPCHK(ctx, ev.create());
    hipError_t e = ev.start(nullptr);
    if (e == hipSuccess)
        e = launch_match(ctx->edges.d, ctx->edges.seg_cap(), ctx->edges.counts, max_of(counts), total, q0, nq, r0, nm, nb, k, d_cl, d_cl + nm,
                         d_cl + nm + n_clusters, d_cl + nm + 2 * (size_t)n_clusters, d_cl + nm + 2 * (size_t)n_clusters + nq,
                         buf<uint32_t>(ctx, SB_SEARCH_CNT), buf<uint32_t>(ctx, SB_SEARCH_START), buf<uint64_t>(ctx, SB_SEARCH_SCAN),
                         buf<uint64_t>(ctx, SB_SEARCH_OUT), buf<uint64_t>(ctx, SB_MATCH_REC), cap, d_scr2, d_scr2 + nq + 3 * (size_t)nb + 1,
                         d_best, d_score, d_nfeas, nullptr);
    if (e == hipSuccess) e = ev.stop(nullptr);
    if (e == hipSuccess) e = hipEventSynchronize(ev.b);
    float sel_ms = 0;
    if (e == hipSuccess) e = ev.elapsed(&sel_ms);
    if (e != hipSuccess) return fail_hip(ctx, "match", e);
    HIPCHK(ctx, hipMemcpy(best_cluster, d_best, nk * 4, hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(best_score, d_score, nk * 4, hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(n_feasible, d_nfeas, (size_t)nb * 4, hipMemcpyDeviceToHost));
    S.kernel_ms = ms + sel_ms;
    if (stats) *stats = S;
    return HMK_OK;
}

}  // namespace

} }  // namespace hmk::impl

extern "C" {

int hmk_match_clusters_shifted(hmk_ctx *ctx, uint32_t q0, uint32_t q1, const uint32_t *query_cluster, uint32_t n_query_clusters, uint32_t r0,
                               uint32_t r1, const uint32_t *member_cluster, const int32_t *cluster_id, uint32_t n_clusters, int max_shift,
                               int shift_penalty, int threshold, uint32_t k, uint32_t *best_cluster, int32_t *best_score, uint32_t *n_feasible,
                               hmk_neighbor_stats *stats) {
    return match(ctx, MATCH_SHIFTED, q0, q1, query_cluster, n_query_clusters, r0, r1, member_cluster, cluster_id, n_clusters, max_shift,
                 shift_penalty, threshold, k, best_cluster, best_score, n_feasible, stats);
}

int hmk_match_clusters_local(hmk_ctx *ctx, uint32_t q0, uint32_t q1, const uint32_t *query_cluster, uint32_t n_query_clusters, uint32_t r0,
                             uint32_t r1, const uint32_t *member_cluster, const int32_t *cluster_id, uint32_t n_clusters, int gap_open,
                             int gap_extend, int threshold, uint32_t k, uint32_t *best_cluster, int32_t *best_score, uint32_t *n_feasible,
                             hmk_neighbor_stats *stats) {
    return match(ctx, MATCH_LOCAL, q0, q1, query_cluster, n_query_clusters, r0, r1, member_cluster, cluster_id, n_clusters, gap_open, gap_extend,
                 threshold, k, best_cluster, best_score, n_feasible, stats);
}

}  // extern "C"
