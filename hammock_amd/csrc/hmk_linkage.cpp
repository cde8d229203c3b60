// hmk_linkage.cpp -- complete-linkage scores inside given clusters: per slot ClinkageClusterScorer.clusterScore without its early
// exit (ClinkageClusterScorer.java:30-49), applied to the pairs inside ONE cluster; the half of the question "is this clustering a
// fixed point of complete linkage" that hmk_cluster_pairs_shifted (hmk_merge.cpp, the pairs between clusters) leaves open.
//   tables   on the host, O(members + clusters) (hmk_slots.cpp: build_link_tables): the members by slot in index order, the small
//            slots' first, with the prefix sums the kernels decode their work from (pairs of the small slots, tiles of the large ones);
//   kernels  k_linkage.hip on the clustering stream: accumulators cleared, small slots flat, large slots tiled;
//   results  the accumulators back to the host, the slots' keys decoded there (O(clusters)).
// No pass, no edge buffer, no plan: nothing proportional to the number of pairs exists anywhere.
#include "hmk_ctx.h"
#include "hmk_linkage.h"

namespace hmk { namespace impl {

namespace {

int cluster_linkage(hmk_ctx *ctx, uint32_t r0, uint32_t r1, const uint32_t *member_cluster, uint32_t n_clusters, int X, int p, int thr,
                    int32_t *min_score, uint32_t *min_a, uint32_t *min_b, uint64_t *n_below, int32_t *member_min, uint32_t *member_below,
                    hmk_linkage_stats *stats) {
    if (!ctx) return fail(nullptr, HMK_ERR_BAD_ARG, "null context");
    std::lock_guard<std::mutex> lock(ctx->mu);
    refresh_switches(ctx);
    std::vector<uint32_t> members;
    int st = check_slots(ctx, "linkage", r0, r1, member_cluster, n_clusters, members);
    if (st) return st;
    if (n_clusters && (!min_score || !min_a || !min_b || !n_below)) return fail(ctx, HMK_ERR_BAD_ARG, "null output (min_score, min_a, min_b, n_below)");
    if ((member_min == nullptr) != (member_below == nullptr))
        return fail(ctx, HMK_ERR_BAD_ARG, "member_min and member_below are given together or not at all");
    if (!ctx->symmetric)
        return fail(ctx, HMK_ERR_BAD_ARG, "the linkage of a cluster needs a symmetric scoring matrix: the score of an unordered pair must not "
                                          "depend on which member comes first (ClinkageClusterScorer.java:30-49 scores each pair once)");
    st = need_device(ctx);
    if (st) return st;
    const uint32_t nm = r1 - r0;
    hmk_linkage_stats S{};
    for (uint32_t c = 0; c < n_clusters; c++) {
        min_score[c] = INT32_MAX;
        min_a[c] = min_b[c] = 0xFFFFFFFFu;
        n_below[c] = 0;
    }
    const SlotCounts counts = count_slots(members);
    S.n_multi = counts.n_multi;
    S.pairs_scored = counts.pairs;
    for (uint32_t i = 0; member_min && i < nm; i++) { member_min[i] = INT32_MAX; member_below[i] = 0; }
    if (nm) {
        st = check_link_scores(ctx, X, p, thr, r0, r1);
        if (st) return st;
    }
    if (S.n_multi == 0) {
        if (stats) *stats = S;
        return HMK_OK;
    }

    // ---- the tables: flat slots first, then the tiled ones; singletons take no part
    LinkTables T;
    build_link_tables(r0, nm, member_cluster, n_clusters, members, T);

    st = ensure_res32(ctx);
    if (st) return st;
    st = greedy_streams(ctx);
    if (st) return st;
    // the accumulators: key uint64[ncl] | below uint64[ncl] | member_min int32[nm] | member_below uint32[nm]
    const size_t out_bytes = (size_t)n_clusters * 16 + (member_min ? (size_t)nm * 8 : 0);
    LinkView V;
    st = reserve_link_tables(ctx, T, &V);
    if (st) return st;
    HIPCHK(ctx, ensure_buf(ctx, SB_LINK_OUT, out_bytes));
    HIPCHK(ctx, ctx->h_merge.ensure(out_bytes + 64, 0));
    uint64_t *d_key = buf<uint64_t>(ctx, SB_LINK_OUT);
    unsigned long long *d_below = reinterpret_cast<unsigned long long *>(d_key + n_clusters);
    int32_t *d_mmin = member_min ? reinterpret_cast<int32_t *>(d_below + n_clusters) : nullptr;
    uint32_t *d_mbelow = member_min ? reinterpret_cast<uint32_t *>(d_mmin + nm) : nullptr;
    const uint8_t *res32 = ctx->d_res32.as<uint8_t>(), *len = ctx->d_len.as<uint8_t>();
    const int32_t *d_M = ctx->d_M.as<int32_t>();
    hipStream_t Q = ctx->gstream;
    EventPair ev;
    HIPCHK(ctx, ev.create());
    hipError_t e = upload_link_tables(ctx, T, Q);
    if (e == hipSuccess) e = ev.start(Q);
    if (e == hipSuccess) e = launch_linkage_init(d_key, d_below, n_clusters, d_mmin, d_mbelow, nm, Q);
    if (e == hipSuccess) e = launch_linkage_flat(res32, len, d_M, V, r0, X, p, thr, d_key, d_below, d_mmin, d_mbelow, Q);
    if (e == hipSuccess) {
        e = launch_linkage_tiled(res32, len, d_M, V, r0, X, p, thr, d_key, d_below, d_mmin, d_mbelow, Q);
        S.launches = 1 + (V.flat_pairs ? 1 : 0) + (V.n_tiles ? 1 : 0);
    }
    if (e == hipSuccess) e = ev.stop(Q);
    if (e == hipSuccess) e = hipMemcpyAsync(ctx->h_merge.p, d_key, out_bytes, hipMemcpyDeviceToHost, Q);
    if (e == hipSuccess) e = hipStreamSynchronize(Q);
    float ms = 0;
    if (e == hipSuccess) e = ev.elapsed(&ms);
    if (e != hipSuccess) return fail_hip(ctx, "cluster linkage", e);
    S.kernel_ms = ms;

    const uint64_t *h_key = (const uint64_t *)ctx->h_merge.p, *h_below = h_key + n_clusters;
    for (uint32_t c = 0; c < n_clusters; c++) {
        if (members[c] < 2) continue;
        const uint64_t k = h_key[c];
        const uint32_t a = (uint32_t)(k >> 24) & 0xFFFFFFu, b = (uint32_t)k & 0xFFFFFFu;
        if (k == ~0ull || a >= b || a < r0 || b >= r1 || member_cluster[a - r0] != c || member_cluster[b - r0] != c)
            return fail(ctx, HMK_ERR_DEVICE, "cluster linkage: slot " + std::to_string(c) + " came back without a pair of its own members");
        min_score[c] = (int32_t)(uint32_t)(k >> 48) - 32768;
        min_a[c] = a;
        min_b[c] = b;
        n_below[c] = h_below[c];
        if (h_below[c]) S.n_violating++;
    }
    if (member_min) {
        std::memcpy(member_min, h_below + n_clusters, (size_t)nm * 4);
        std::memcpy(member_below, (const char *)(h_below + n_clusters) + (size_t)nm * 4, (size_t)nm * 4);
    }
    if (stats) *stats = S;
    return HMK_OK;
}

}  // namespace

} }  // namespace hmk::impl

extern "C" {

int hmk_cluster_linkage_shifted(hmk_ctx *ctx, uint32_t r0, uint32_t r1, const uint32_t *member_cluster, uint32_t n_clusters, int max_shift,
                                int shift_penalty, int threshold, int32_t *min_score, uint32_t *min_a, uint32_t *min_b, uint64_t *n_below,
                                int32_t *member_min, uint32_t *member_below, hmk_linkage_stats *stats) {
    return hmk::impl::cluster_linkage(ctx, r0, r1, member_cluster, n_clusters, max_shift, shift_penalty, threshold, min_score, min_a, min_b, n_below,
                                      member_min, member_below, stats);
}

}  // extern "C"
