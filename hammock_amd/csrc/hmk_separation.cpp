// hmk_separation.cpp -- the separation of given clusters: per member the sum of its ShiftedScorer scores against the rest of its own
// slot and against the nearest other slot (the largest mean, compared exactly), and whether the member sits closer to that slot than
// to its own: the average-linkage statistic behind a silhouette.
//   tables   on the host, O(members + clusters): the members sorted by slot (the partner order every walk follows), the slot of
//            every place and of every member, the slots' first places; one upload;
//   kernels  k_separation.hip on the clustering stream: the walk (blocks of members x segments of the partner order, a record per
//            member and segment), the merge of a member's records;
//   results  one copy of the per-member block; the per-slot sums and counts are formed from it on the host, O(members).
// No sum per (member, slot) exists anywhere: the scratch is O(members x segments + clusters) with at most 64 segments
// (sizing::separation_segments), so no clustering ends in HMK_ERR_CAPACITY.
#include "hmk_ctx.h"
#include "hmk_separation.h"
#include "hmk_slots.h"

namespace hmk { namespace impl {

namespace {

int cluster_separation(hmk_ctx *ctx, uint32_t r0, uint32_t r1, const uint32_t *member_cluster, uint32_t n_clusters, int X, int p, int64_t *own_sum,
                       int64_t *near_sum, uint32_t *near_cluster, uint8_t *misplaced, uint32_t *cluster_misplaced, int64_t *cluster_own_sum,
                       hmk_separation_stats *stats) {
    if (!ctx) return fail(nullptr, HMK_ERR_BAD_ARG, "null context");
    std::lock_guard<std::mutex> lock(ctx->mu);
    refresh_switches(ctx);
    std::vector<uint32_t> members;
    int st = check_slots(ctx, "separation", r0, r1, member_cluster, n_clusters, members);
    if (st) return st;
    const uint32_t nm = r1 - r0;
    if (nm && (!own_sum || !near_sum || !near_cluster)) return fail(ctx, HMK_ERR_BAD_ARG, "null output (own_sum, near_sum, near_cluster)");
    if (!stats) return fail(ctx, HMK_ERR_BAD_ARG, "stats must not be null");
    if (!ctx->symmetric)
        return fail(ctx, HMK_ERR_BAD_ARG, "the separation of clusters needs a symmetric scoring matrix: a member's sum of scores must not "
                                          "depend on which sequence of a pair comes first");
    st = need_device(ctx);
    if (st) return st;
    hmk_separation_stats S{};
    if (nm == 0) {   // (check_clusters: then there is no slot either) nothing is written
        *stats = S;
        return HMK_OK;
    }
    st = check_link_scores(ctx, X, p, 0, r0, r1);   // (nothing is thresholded: 0 passes the threshold's own range check)
    if (st) return st;
    S.n_multi = count_slots(members).n_multi;
    S.pairs_scored = (uint64_t)nm * (nm - 1);
    const sizing::SeparationSegments segs = sizing::separation_segments(nm, (uint32_t)ctx->sw.test_separation_segment);
    S.n_segments = segs.count;

    // ord[nm] | pslot[nm] | mslot[nm] | cstart[ncl + 1]
    const size_t o_ord = 0, o_pslot = nm, o_mslot = 2 * (size_t)nm, o_cstart = 3 * (size_t)nm, words = o_cstart + n_clusters + 1;
    std::vector<uint32_t> h(words);
    {
        const SlotMembers M(nm, member_cluster, n_clusters, members);   // (index order inside every slot)
        std::copy(M.start.begin(), M.start.end(), h.begin() + o_cstart);
        for (uint32_t k = 0; k < nm; k++) {
            const uint32_t i = M.list[k], c = member_cluster[i];
            h[o_ord + k] = r0 + i;
            h[o_pslot + k] = c;
            h[o_mslot + i] = c;
        }
    }

    st = ensure_res32(ctx);
    if (st) return st;
    st = greedy_streams(ctx);
    if (st) return st;
    // records: own | head | tail | best_sum int64[segments x nm], best_size | best_slot uint32[segments x nm];
    // outputs: own_sum | near_sum int64[nm], near_cluster uint32[nm], misplaced uint8[nm]
    const size_t cells = (size_t)segs.count * nm, out_bytes = (size_t)nm * 21;
    HIPCHK(ctx, ensure_buf(ctx, SB_SEP_TAB, words * 4));
    HIPCHK(ctx, ensure_buf(ctx, SB_SEP_REC, cells * SEP_RECORD_BYTES));
    HIPCHK(ctx, ensure_buf(ctx, SB_SEP_OUT, out_bytes));
    HIPCHK(ctx, ctx->h_merge.ensure(out_bytes + 64, 0));
    const uint32_t *d_tab = buf<uint32_t>(ctx, SB_SEP_TAB);
    SepTables T;
    T.ord = d_tab + o_ord;
    T.pslot = d_tab + o_pslot;
    T.mslot = d_tab + o_mslot;
    T.cstart = d_tab + o_cstart;
    T.nm = nm;
    T.n_clusters = n_clusters;
    T.seg_len = segs.length;
    T.n_segments = segs.count;
    SepRecords rec;
    rec.own = buf<long long>(ctx, SB_SEP_REC);
    rec.head = rec.own + cells;
    rec.tail = rec.head + cells;
    rec.best_sum = rec.tail + cells;
    rec.best_size = reinterpret_cast<uint32_t *>(rec.best_sum + cells);
    rec.best_slot = rec.best_size + cells;
    SepOut out;
    out.own_sum = buf<long long>(ctx, SB_SEP_OUT);
    out.near_sum = out.own_sum + nm;
    out.near_cluster = reinterpret_cast<uint32_t *>(out.near_sum + nm);
    out.misplaced = reinterpret_cast<uint8_t *>(out.near_cluster + nm);
    const uint8_t *res32 = ctx->d_res32.as<uint8_t>(), *len = ctx->d_len.as<uint8_t>();
    const int32_t *d_M = ctx->d_M.as<int32_t>();
    char *h_out = (char *)ctx->h_merge.p;
    hipStream_t Q = ctx->gstream;
    EventPair ev;
    HIPCHK(ctx, ev.create());
    hipError_t e = hipMemcpyAsync(const_cast<uint32_t *>(d_tab), h.data(), words * 4, hipMemcpyHostToDevice, Q);
    if (e == hipSuccess) e = ev.start(Q);
    if (e == hipSuccess) e = launch_separation_walk(res32, len, d_M, T, r0, X, p, rec, Q);
    if (e == hipSuccess) e = launch_separation_merge(T, rec, out, Q);
    S.launches = 2;
    if (e == hipSuccess) e = ev.stop(Q);
    if (e == hipSuccess) e = hipMemcpyAsync(h_out, out.own_sum, out_bytes, hipMemcpyDeviceToHost, Q);
    if (e == hipSuccess) e = hipStreamSynchronize(Q);
    float ms = 0;
    if (e == hipSuccess) e = ev.elapsed(&ms);
    if (e != hipSuccess) return fail_hip(ctx, "cluster separation", e);
    S.kernel_ms = ms;

    const int64_t *h_own = (const int64_t *)h_out, *h_near = h_own + nm;
    const uint32_t *h_slot = (const uint32_t *)(h_near + nm);
    const uint8_t *h_mis = (const uint8_t *)(h_slot + nm);
    for (uint32_t i = 0; i < nm; i++) {
        const uint32_t c = h_slot[i];
        if (n_clusters == 1 ? c != 0xFFFFFFFFu : (c >= n_clusters || c == member_cluster[i]))
            return fail(ctx, HMK_ERR_DEVICE, "cluster separation: member " + std::to_string(r0 + i) + " came back without a nearest slot other than its own");
    }
    std::memcpy(own_sum, h_own, (size_t)nm * 8);
    std::memcpy(near_sum, h_near, (size_t)nm * 8);
    std::memcpy(near_cluster, h_slot, (size_t)nm * 4);
    if (misplaced) std::memcpy(misplaced, h_mis, nm);
    for (uint32_t c = 0; c < n_clusters; c++) {
        if (cluster_misplaced) cluster_misplaced[c] = 0;
        if (cluster_own_sum) cluster_own_sum[c] = 0;
    }
    for (uint32_t i = 0; i < nm; i++) {
        const uint32_t c = member_cluster[i];
        S.n_misplaced += h_mis[i];
        if (cluster_misplaced) cluster_misplaced[c] += h_mis[i];
        if (cluster_own_sum) cluster_own_sum[c] += h_own[i];
    }
    *stats = S;
    return HMK_OK;
}

}  // namespace

} }  // namespace hmk::impl

extern "C" {

int hmk_cluster_separation_shifted(hmk_ctx *ctx, uint32_t r0, uint32_t r1, const uint32_t *member_cluster, uint32_t n_clusters, int max_shift,
                                   int shift_penalty, int64_t *own_sum, int64_t *near_sum, uint32_t *near_cluster, uint8_t *misplaced,
                                   uint32_t *cluster_misplaced, int64_t *cluster_own_sum, hmk_separation_stats *stats) {
    return hmk::impl::cluster_separation(ctx, r0, r1, member_cluster, n_clusters, max_shift, shift_penalty, own_sum, near_sum, near_cluster,
                                         misplaced, cluster_misplaced, cluster_own_sum, stats);
}

}  // extern "C"
