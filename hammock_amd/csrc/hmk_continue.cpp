// hmk_continue.cpp -- continuing a greedy clustering with new sequences: the second loop of LimitedGreedySequenceClusterer.cluster
// (LimitedGreedySequenceClusterer.java:59-67) with actualClusters = given clusters and actualSequences = the new sequences [q0, q1)
// of the hmk_set_sequences set.  Scoring: members x new (the search's rectangle, hmk_plan.cpp) and new x new (its triangle) into
// one edge list; the CSR of the new rows (piece_enqueue_csr), the pre-check (piece_precheck) and the rounds (device_second_loop) of
// hmk_cluster.cpp; the extern "C" entry point.
#include "hmk_ctx.h"

namespace hmk { namespace impl {

namespace {

// The candidate lists on the host, for a call whose device pre-check overflowed its tables (a new sequence next to more than
// ~45,000 clusters, k_greedy_precheck): the new rows come to the host, every cluster all of whose members are neighbours of a row
// is listed with the lowest score (the greedy's host pre-check, hmk_greedy.cpp), and the lists go back in the layout of the two-pass
// pre-check (cand_start = prefix sums).
template <class NbrT>
int host_precheck(hmk_ctx *ctx, uint32_t q0, uint32_t q1, const std::vector<int32_t> &cluster_of, const std::vector<uint32_t> &members,
                  uint32_t *cand_total) {
    const uint32_t nq = q1 - q0, ncl = (uint32_t)members.size();
    std::vector<uint64_t> start((size_t)nq + 1);
    HIPCHK(ctx, hipMemcpy(start.data(), buf<uint64_t>(ctx, SB_START) + q0, ((size_t)nq + 1) * 8, hipMemcpyDeviceToHost));
    std::vector<NbrT> adj(std::max<uint64_t>(start[nq] - start[0], 1));
    if (start[nq] > start[0])
        HIPCHK(ctx, hipMemcpy(adj.data(), buf<NbrT>(ctx, SB_ADJ) + start[0], (start[nq] - start[0]) * sizeof(NbrT), hipMemcpyDeviceToHost));
    std::vector<uint32_t> cstart((size_t)nq + 1, 0), cnt(std::max<uint32_t>(nq, 1), 0);
    std::vector<GreedyCand> cand;
    std::vector<uint32_t> c2(ncl, 0);
    std::vector<int32_t> m2(ncl, 0), seen;
    for (uint32_t q = 0; q < nq; q++) {
        seen.clear();
        for (uint64_t e = start[q] - start[0]; e < start[q + 1] - start[0]; e++) {
            const int32_t c = cluster_of[adj[e].id()];
            if (c < 0) continue;
            if (c2[c]++ == 0) { seen.push_back(c); m2[c] = adj[e].score(); }
            else m2[c] = std::min(m2[c], adj[e].score());
        }
        cstart[q] = (uint32_t)cand.size();
        for (int32_t c : seen) {
            if (c2[c] == members[c]) cand.push_back(GreedyCand{c, m2[c], 0});
            c2[c] = 0;
        }
        cnt[q] = (uint32_t)cand.size() - cstart[q];
        if (cand.size() > 0x7FFFFFFFu) return fail(ctx, HMK_ERR_OOM, "more than 2^31 - 1 candidate entries");
    }
    cstart[nq] = (uint32_t)cand.size();
    HIPCHK(ctx, ensure_buf(ctx, SB_CAND, std::max<size_t>(cand.size(), 1) * sizeof(GreedyCand)));
    if (!cand.empty()) HIPCHK(ctx, hipMemcpy(buf<void>(ctx, SB_CAND), cand.data(), cand.size() * sizeof(GreedyCand), hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemcpy(buf<void>(ctx, SB_CSTART), cstart.data(), ((size_t)nq + 1) * 4, hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemcpy(buf<void>(ctx, SB_CNT), cnt.data(), (size_t)nq * 4, hipMemcpyHostToDevice));
    *cand_total = (uint32_t)cand.size();
    return HMK_OK;
}

int greedy_continue(hmk_ctx *ctx, uint32_t q0, uint32_t q1, uint32_t r0, uint32_t r1, const uint32_t *member_cluster, const int32_t *cluster_id,
                    uint32_t n_clusters, int X, int p, int thr, int32_t *joined, int32_t *member_rank, hmk_continue_stats *stats) {
    if (!ctx) return fail(nullptr, HMK_ERR_BAD_ARG, "null context");
    std::lock_guard<std::mutex> lock(ctx->mu);
    refresh_switches(ctx);
    std::vector<uint32_t> members;
    std::vector<int64_t> csize;
    int st = check_clusters(ctx, "continuation", q0, q1, r0, r1, member_cluster, cluster_id, n_clusters, members, csize);
    if (st) return st;
    const uint32_t nq = q1 - q0, n = ctx->n;
    if (nq && (!joined || !member_rank)) return fail(ctx, HMK_ERR_BAD_ARG, "null output buffer");
    if (!ctx->symmetric)
        return fail(ctx, HMK_ERR_BAD_ARG, "hmk_greedy_continue needs a symmetric matrix: its device loop reads a pair's score from either end");
    st = need_device(ctx);
    if (st) return st;
    hmk_continue_stats S{};
    for (uint32_t q = 0; q < nq; q++) { joined[q] = -1; member_rank[q] = -1; }
    if (nq == 0 || n_clusters == 0) {   // (no candidates: every new sequence stays alone, :63-65)
        if (stats) *stats = S;
        return HMK_OK;
    }
    st = check_shifted(ctx, X, p, thr, q0, q1, r0, r1);
    if (st) return st;
    st = greedy_streams(ctx);
    if (st) return st;
    if (!ctx->h_loop) return fail(ctx, HMK_ERR_DEVICE, "no coherent pinned block for the device loop's progress word");

    // ---- the two passes into one edge list: members x new (members = the rectangle's queries, as the assignment has them), then
    // new x new (the triangle, appended to the counts of the first launch).  Members x members is never scored.
    st = build_plan_search(ctx, ctx->plan_continue, X, p, thr, r0, r1, q0, q1);
    if (st) return st;
    const bool tri = nq >= 2;
    if (tri) {
        st = build_plan_triangle(ctx, ctx->plan_continue_tri, X, p, thr, q0, q1);
        if (st) return st;
    }
    unsigned long long counts[HMK_EDGE_SHARDS];
    double ms = 0;
    st = neighbors_grow(ctx, 0, counts, &ms, [&](uint64_t *d_edges, uint64_t cap, unsigned long long *d_counts) {
        int r = launch_plan(ctx, ctx->plan_continue, X, p, thr, d_edges, cap, d_counts, nullptr);
        // (LAUNCH_REST on a plan without a band: every tile, no reset of the counts -- the triangle's edges go behind the rectangle's)
        if (r == HMK_OK && tri) r = launch_plan(ctx, ctx->plan_continue_tri, X, p, thr, d_edges, cap, d_counts, nullptr, LAUNCH_REST);
        return r;
    });
    if (st) return st;
    S.n_edges += total_of(counts);
    S.pairs_scored = ctx->plan_continue.stats.pairs_scored + (tri ? ctx->plan_continue_tri.stats.pairs_scored : 0);
    S.kernel_ms = ms;

    // ---- CSR of the new rows.  The rounds read only a joiner's upper section (k_loop_apply): the later new sequences have larger
    // ids whichever side of the members the new range lies on, so the caller's layout serves as it is.
    const auto tl = std::chrono::steady_clock::now();
    hipStream_t Q = ctx->gstream;
    const bool packed = adjacency_packed(ctx, X, p, thr);   // (4-byte entries m << 8 | score - threshold, as hmk_greedy_cluster)
    hipError_t e = piece_enqueue_csr(ctx, ctx->edges.segs(), true, packed, thr, n, q0, q1, false, false, Q);
    if (e == hipSuccess) e = hipStreamSynchronize(Q);
    if (e != hipSuccess) return fail_hip(ctx, "continuation CSR", e);
    if (((const int *)(ctx->h_counts + HC_RANGE))[2] != 0) return fail(ctx, HMK_ERR_DEVICE, "continuation CSR: an edge names a sequence outside [0, n)");
    const uint64_t entries = ctx->h_counts[HC_TOTAL];

    // ---- pre-check: per new sequence the clusters all of whose members are its neighbours (k_greedy_precheck, one pass)
    std::vector<int32_t> cluster_of(n, -1);
    for (uint32_t i = 0; i < r1 - r0; i++) cluster_of[r0 + i] = (int32_t)member_cluster[i];
    PreIn in;
    in.n = n; in.nl = nq; in.ncl = n_clusters; in.packed = packed;
    in.b_cof = (size_t)n * 4; in.b_us = (size_t)n_clusters * 4; in.b_left = (size_t)nq * 4;
    HIPCHK(ctx, ctx->h_stage.ensure(HMK_PRE_REGIONS * sizeof(unsigned long long) + in.b_cof + in.b_us + in.b_left + 64, 0));
    {
        char *hs = (char *)ctx->h_stage.p + HMK_PRE_REGIONS * sizeof(unsigned long long);   // (the block starts with the region counters)
        std::memcpy(hs, cluster_of.data(), in.b_cof);
        int32_t *us = (int32_t *)(hs + in.b_cof);
        for (uint32_t c = 0; c < n_clusters; c++) us[c] = (int32_t)members[c];
        uint32_t *left = (uint32_t *)(hs + in.b_cof + in.b_us);
        for (uint32_t q = 0; q < nq; q++) left[q] = q0 + q;
        in.h_block = hs;
    }
    // small tables first when the new rows see few clustered neighbours (the estimate of hmk_cluster.cpp: ~5 x the clusters of a row)
    const double est = (double)entries / nq * (double)(r1 - r0) / (double)((r1 - r0) + nq);
    in.first_slots = est <= 24.0 ? 128 : 512;
    in.two_stage = est <= 100.0 && ctx->sw.precheck != 2;
    const size_t want = std::max<size_t>({ctx->sb[SB_CAND].cap / sizeof(GreedyCand), (size_t)nq * 24, (size_t)HMK_PRE_REGIONS * 64});   // entries
    // entry indices stay below 2^31 (cand_start[] is uint32, the k_loop_* subscriber records keep 31 bits): regions of at most
    // 2^31 / HMK_PRE_REGIONS entries
    constexpr unsigned long long REGION_MAX = 0x7FFFFFFFull / HMK_PRE_REGIONS;
    in.region_cap = std::min<unsigned long long>(want / HMK_PRE_REGIONS, REGION_MAX);
    unsigned long long total = 0;
    ((uint32_t *)(ctx->h_counts + HC_MISC))[0] = 0;   // (the tables' overflow count lands here)
    int fit = piece_precheck(ctx, in, 0, n, 0, HMK_PRE_REGIONS, Q, true, &total);
    if (fit == 1) {   // a region overran: once more with room for the fullest one (the region counters are the block's first words)
        unsigned long long fullest = 0;
        for (uint32_t g = 0; g < HMK_PRE_REGIONS; g++) fullest = std::max(fullest, ((const unsigned long long *)ctx->h_stage.p)[g]);
        if (fullest <= REGION_MAX) {
            in.region_cap = fullest;
            fit = piece_precheck(ctx, in, 0, n, 0, HMK_PRE_REGIONS, Q, false, &total);
        }
    }
    uint32_t cand_total = 0;
    if (fit == 0) {
        cand_total = (uint32_t)total;   // (< 2^31: every entry lies below HMK_PRE_REGIONS x region_cap)
    } else if (fit == 1 || ((const uint32_t *)(ctx->h_counts + HC_MISC))[0] != 0) {
        // a region still overran (the second stage's rows reach the regions in no fixed order) or a row overflowed its tables: the
        // host's lists
        S.host_precheck = 1;
        st = packed ? host_precheck<NbrPacked>(ctx, q0, q1, cluster_of, members, &cand_total)
                    : host_precheck<Nbr>(ctx, q0, q1, cluster_of, members, &cand_total);
        if (st) return st;
    } else {
        return fail(ctx, HMK_ERR_DEVICE, "continuation pre-check failed: " + std::string(hipGetErrorString(hipGetLastError())));
    }

    // ---- the loop (k_loop_* rounds, hmk_greedy_cluster's): the slots' size() and ids, the new sequences as the leftovers
    std::vector<int32_t> cids(cluster_id, cluster_id + n_clusters);
    const std::vector<EdgeSource::Piece> pieces{EdgeSource::Piece{ctx, 0, n}};
    LoopIn li;
    li.n = n; li.nl = nq; li.ncl = n_clusters; li.cand_total = cand_total; li.packed = packed;
    li.csize = &csize; li.cids = &cids; li.pieces = &pieces;
    std::vector<int32_t> join_slot;
    std::string stall;
    const bool done = device_second_loop(ctx, Q, li, join_slot, &S.loop_rounds, &stall);
    if (!stall.empty()) return fail(ctx, HMK_ERR_DEVICE, stall);
    if (!ctx->wedged) {
        e = hipStreamSynchronize(Q);   // (the round enqueued past the last one)
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->copy_stream);
        if (!done && e == hipSuccess) e = hipErrorUnknown;
        if (e != hipSuccess) return fail(ctx, HMK_ERR_DEVICE, std::string("continuation loop: ") + hipGetErrorString(e));
    }
    // :61-62 in loop order: the joiner's place in Cluster.getSequences()
    std::vector<uint32_t> added(n_clusters, 0);
    for (uint32_t q = 0; q < nq; q++) {
        const int32_t c = join_slot[q];
        if (c < 0) continue;
        joined[q] = c;
        member_rank[q] = (int32_t)(members[c] + added[c]++);
        S.n_joined++;
    }
    S.loop_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tl).count();
    if (stats) *stats = S;
    return HMK_OK;
}

}  // namespace

} }  // namespace hmk::impl

extern "C" {

int hmk_greedy_continue(hmk_ctx *ctx, uint32_t q0, uint32_t q1, uint32_t r0, uint32_t r1, const uint32_t *member_cluster,
                        const int32_t *cluster_id, uint32_t n_clusters, int max_shift, int shift_penalty, int threshold, int32_t *joined,
                        int32_t *member_rank, hmk_continue_stats *stats) {
    return greedy_continue(ctx, q0, q1, r0, r1, member_cluster, cluster_id, n_clusters, max_shift, shift_penalty, threshold, joined,
                           member_rank, stats);
}

}  // extern "C"
