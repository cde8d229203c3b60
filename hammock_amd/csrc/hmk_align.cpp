// hmk_align.cpp -- centre-star alignment of given clusters around their medoids, in the ungapped model of the scorer that formed them:
// per slot the member with the largest sum of ShiftedScorer scores against the others (the centre), per member scoreWithShift against
// that centre (ShiftedScorer.java:48-95), from whose shifts the aligned rows follow.  Not Clustal Omega's alignment
// (ClustalRunner.java:34-66): no gap ever stands inside a peptide.
//   tables   hmk_slots.cpp's (build_link_tables), O(members + clusters), one upload;
//   kernels  k_align.hip on the clustering stream: accumulators cleared, the members' sums (small slots flat, large slots tiled), the
//            slots' centres, every member against its centre; the centres stay on the device between the last two;
//   results  one copy of the per-slot block and one of the per-member block; keys decoded, columns and widths formed on the host,
//            O(members + clusters).
// Nothing proportional to the number of pairs exists anywhere.
#include "hmk_ctx.h"
#include "hmk_align.h"

namespace hmk { namespace impl {

namespace {

int cluster_align(hmk_ctx *ctx, uint32_t r0, uint32_t r1, const uint32_t *member_cluster, uint32_t n_clusters, int X, int p, uint32_t *center,
                  int64_t *center_sum, uint32_t *width, int64_t *member_sum, int32_t *center_score, int32_t *shift, uint32_t *column,
                  hmk_align_stats *stats) {
    if (!ctx) return fail(nullptr, HMK_ERR_BAD_ARG, "null context");
    std::lock_guard<std::mutex> lock(ctx->mu);
    refresh_switches(ctx);
    std::vector<uint32_t> members;
    int st = check_slots(ctx, "align", r0, r1, member_cluster, n_clusters, members);
    if (st) return st;
    const uint32_t nm = r1 - r0;
    if (n_clusters && (!center || !center_sum || !width)) return fail(ctx, HMK_ERR_BAD_ARG, "null output (center, center_sum, width)");
    if (nm && (!center_score || !shift || !column)) return fail(ctx, HMK_ERR_BAD_ARG, "null output (center_score, shift, column)");
    if (!ctx->symmetric)
        return fail(ctx, HMK_ERR_BAD_ARG, "the alignment of a cluster needs a symmetric scoring matrix: a member's sum of scores must not "
                                          "depend on which sequence of a pair comes first");
    st = need_device(ctx);
    if (st) return st;
    hmk_align_stats S{};
    if (nm == 0) {   // (check_clusters: then there is no slot either) nothing is written
        if (stats) *stats = S;
        return HMK_OK;
    }
    st = check_link_scores(ctx, X, p, 0, r0, r1);   // (nothing is thresholded: 0 passes the threshold's own range check)
    if (st) return st;

    // what the device does not touch: the slots of one member, each its own centre
    for (uint32_t i = 0; i < nm; i++) {
        const uint32_t c = member_cluster[i];
        center_score[i] = INT32_MAX;
        shift[i] = 0;
        column[i] = 0;
        if (member_sum) member_sum[i] = 0;
        if (members[c] == 1) {
            center[c] = r0 + i;
            center_sum[c] = 0;
            width[c] = ctx->len[r0 + i];
            S.max_width = std::max<uint32_t>(S.max_width, width[c]);
        }
    }
    const SlotCounts counts = count_slots(members);
    S.n_multi = counts.n_multi;
    S.pairs_scored = counts.pairs;
    for (const uint32_t s : members) S.pairs_scored += s >= 2 ? s - 1 : 0;   // (every member of such a slot but its centre, against the centre)
    if (S.n_multi == 0) {
        if (stats) *stats = S;
        return HMK_OK;
    }

    LinkTables T;
    build_link_tables(r0, nm, member_cluster, n_clusters, members, T);

    st = ensure_res32(ctx);
    if (st) return st;
    st = greedy_streams(ctx);
    if (st) return st;
    // per slot: key uint64[ncl] | min_shift int32[ncl] | max_end int32[ncl]; per member: sum int64[nm] | score int32[nm] | shift int32[nm]
    const size_t slot_bytes = (size_t)n_clusters * 16, memb_bytes = (size_t)nm * 16;
    const size_t memb_from = member_sum ? 0 : (size_t)nm * 8;   // (sums not wanted: they stay on the device)
    LinkView V;
    st = reserve_link_tables(ctx, T, &V);
    if (st) return st;
    HIPCHK(ctx, ensure_buf(ctx, SB_ALIGN_SLOT, slot_bytes));
    HIPCHK(ctx, ensure_buf(ctx, SB_ALIGN_MEMB, memb_bytes));
    HIPCHK(ctx, ctx->h_merge.ensure(slot_bytes + memb_bytes + 64, 0));
    AlignOut out;
    out.key = buf<uint64_t>(ctx, SB_ALIGN_SLOT);
    out.min_shift = reinterpret_cast<int32_t *>(out.key + n_clusters);
    out.max_end = out.min_shift + n_clusters;
    out.sum = buf<long long>(ctx, SB_ALIGN_MEMB);
    out.score = reinterpret_cast<int32_t *>(out.sum + nm);
    out.shift = out.score + nm;
    const AlignSlots slots{V.tab, V.fslot, V.fmstart, V.bslot, V.bmstart, V.nf, V.nb, V.nt};
    const uint8_t *res32 = ctx->d_res32.as<uint8_t>(), *len = ctx->d_len.as<uint8_t>();
    const int32_t *d_M = ctx->d_M.as<int32_t>();
    char *h_slot = (char *)ctx->h_merge.p, *h_memb = h_slot + slot_bytes;
    hipStream_t Q = ctx->gstream;
    EventPair ev;
    HIPCHK(ctx, ev.create());
    hipError_t e = upload_link_tables(ctx, T, Q);
    if (e == hipSuccess) e = ev.start(Q);
    if (e == hipSuccess) e = launch_align_init(out, n_clusters, nm, Q);
    if (e == hipSuccess) e = launch_align_sums_flat(res32, len, d_M, V, r0, X, p, out.sum, Q);
    if (e == hipSuccess) e = launch_align_sums_tiled(res32, len, d_M, V, r0, X, p, out.sum, Q);
    if (e == hipSuccess) e = launch_align_center(slots, r0, out.sum, out.key, Q);
    if (e == hipSuccess) e = launch_align_shift(res32, len, d_M, slots, r0, r1, X, p, out, Q);
    S.launches = 3 + (V.flat_pairs ? 1 : 0) + (V.n_tiles ? 1 : 0);
    if (e == hipSuccess) e = ev.stop(Q);
    if (e == hipSuccess) e = hipMemcpyAsync(h_slot, out.key, slot_bytes, hipMemcpyDeviceToHost, Q);
    if (e == hipSuccess) e = hipMemcpyAsync(h_memb + memb_from, (const char *)out.sum + memb_from, memb_bytes - memb_from, hipMemcpyDeviceToHost, Q);
    if (e == hipSuccess) e = hipStreamSynchronize(Q);
    float ms = 0;
    if (e == hipSuccess) e = ev.elapsed(&ms);
    if (e != hipSuccess) return fail_hip(ctx, "cluster align", e);
    S.kernel_ms = ms;

    const uint64_t *h_key = (const uint64_t *)h_slot;
    const int32_t *h_min = (const int32_t *)(h_key + n_clusters), *h_end = h_min + n_clusters;
    for (uint32_t c = 0; c < n_clusters; c++) {
        if (members[c] < 2) continue;
        const uint64_t k = h_key[c];
        const uint32_t z = 0xFFFFFFu - ((uint32_t)k & 0xFFFFFFu);
        if (k == 0 || z < r0 || z >= r1 || member_cluster[z - r0] != c || h_min[c] > 0 || h_end[c] <= h_min[c])
            return fail(ctx, HMK_ERR_DEVICE, "cluster align: slot " + std::to_string(c) + " came back without a centre among its own members");
        center[c] = z;
        center_sum[c] = (int64_t)(k >> 24) - ((int64_t)1 << 39);
        width[c] = (uint32_t)(h_end[c] - h_min[c]);
        S.max_width = std::max(S.max_width, width[c]);
    }
    const int32_t *h_score = (const int32_t *)(h_memb + (size_t)nm * 8), *h_shift = h_score + nm;
    if (member_sum) std::memcpy(member_sum, h_memb, (size_t)nm * 8);
    std::memcpy(center_score, h_score, (size_t)nm * 4);
    std::memcpy(shift, h_shift, (size_t)nm * 4);
    for (uint32_t i = 0; i < nm; i++) {
        const uint32_t c = member_cluster[i];
        if (members[c] >= 2) column[i] = (uint32_t)(h_shift[i] - h_min[c]);
    }
    if (stats) *stats = S;
    return HMK_OK;
}

}  // namespace

} }  // namespace hmk::impl

extern "C" {

int hmk_cluster_align_shifted(hmk_ctx *ctx, uint32_t r0, uint32_t r1, const uint32_t *member_cluster, uint32_t n_clusters, int max_shift,
                              int shift_penalty, uint32_t *center, int64_t *center_sum, uint32_t *width, int64_t *member_sum,
                              int32_t *center_score, int32_t *shift, uint32_t *column, hmk_align_stats *stats) {
    return hmk::impl::cluster_align(ctx, r0, r1, member_cluster, n_clusters, max_shift, shift_penalty, center, center_sum, width, member_sum,
                                    center_score, shift, column, stats);
}

}  // extern "C"
