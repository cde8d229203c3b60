// hmk_profile.cpp -- the profile of given clusters under a given placement: what the reference reads from a cluster's alignment
// (FileIOManager.getPositionLetterCounts / getInformationContents / defineMatchStates / checkConservedStates,
// FileIOManager.java:1172-1300, :1421-1439; Statistics.getClusterKlds / getPeptideKld / getCorrectedFrequencies,
// Statistics.java:207-300; the system means of Hammock.java:681-697), for every slot at once.
//   checks   on the host, before the device is looked at: the placement against HMK_PROFILE_MAX_WIDTH, the parameters, the residues;
//            the widths and the slots' column offsets are formed there too (O(members + clusters));
//   tables   hmk_slots.cpp's (build_link_tables) for the multi-member slots, and one block of the call's own: the frequency table,
//            per member slot and column, per slot size and column offset, the large slots' chunks; two uploads;
//   kernels  k_profile.hip on the clustering stream: accumulators cleared, counts (small slots, large slots), columns, match states,
//            KLDs; the masks stay on the device between them;
//   results  the requested per-column arrays straight to the caller, one copy of the per-slot block and one of the per-member
//            block; the means are summed on the host in member index order.
#include <cmath>

#include "hmk_ctx.h"
#include "hmk_profile.h"

static_assert(HMK_PROFILE_SYMBOLS == hmk::PROFILE_SYMBOLS && HMK_PROFILE_MAX_WIDTH == hmk::PROFILE_MAX_WIDTH, "hmk_profile.h restates the ABI's constants");

namespace hmk { namespace impl {

namespace {

bool positive(double v) { return std::isfinite(v) && v > 0; }

int cluster_profile(hmk_ctx *ctx, uint32_t r0, uint32_t r1, const uint32_t *member_cluster, uint32_t n_clusters, const uint32_t *column,
                    const hmk_profile_params *params, uint32_t *width, uint32_t *n_conserved, uint32_t *n_match, uint8_t *passes,
                    double *kld_match_mean, double *kld_all_mean, uint64_t *col_start, uint64_t col_capacity, uint32_t *counts, double *ic,
                    uint8_t *col_flags, double *kld_match, double *kld_all, hmk_profile_stats *stats) {
    if (!ctx) return fail(nullptr, HMK_ERR_BAD_ARG, "null context");
    std::lock_guard<std::mutex> lock(ctx->mu);
    refresh_switches(ctx);
    std::vector<uint32_t> members;
    int st = check_slots(ctx, "profile", r0, r1, member_cluster, n_clusters, members);
    if (st) return st;
    const uint32_t nm = r1 - r0;
    if (!params || !stats || !col_start) return fail(ctx, HMK_ERR_BAD_ARG, "null params, stats or col_start");
    if (n_clusters && (!width || !n_conserved || !n_match || !passes || !kld_match_mean || !kld_all_mean))
        return fail(ctx, HMK_ERR_BAD_ARG, "null output (width, n_conserved, n_match, passes, kld_match_mean, kld_all_mean)");
    if (nm && (!column || !kld_match || !kld_all)) return fail(ctx, HMK_ERR_BAD_ARG, "null column, kld_match or kld_all");
    const hmk_profile_params &P = *params;
    if (!std::isfinite(P.min_ic)) return fail(ctx, HMK_ERR_BAD_ARG, "min_ic is not finite");
    if (!(P.max_gap_proportion >= 0 && P.max_gap_proportion <= 1)) return fail(ctx, HMK_ERR_BAD_ARG, "max_gap_proportion outside [0, 1]");
    if (P.min_conserved_positions < 0) return fail(ctx, HMK_ERR_BAD_ARG, "negative min_conserved_positions");
    if (!positive(P.beta) || !positive(P.sigma) || !positive(P.scale)) return fail(ctx, HMK_ERR_BAD_ARG, "beta, sigma and scale must be finite and > 0");
    for (int e = 0; e < 400; e++)
        if (!positive(P.frequency[e]))
            return fail(ctx, HMK_ERR_BAD_ARG, "frequency[" + std::to_string(e / 20) + "][" + std::to_string(e % 20) + "] is not finite and > 0");
    for (int e = 0; e < 20; e++)
        if (!positive(P.background[e])) return fail(ctx, HMK_ERR_BAD_ARG, "background[" + std::to_string(e) + "] is not finite and > 0");
    for (uint32_t i = 0; i < nm; i++)
        if ((uint64_t)column[i] + ctx->len[r0 + i] > (uint64_t)HMK_PROFILE_MAX_WIDTH)
            return fail(ctx, HMK_ERR_BAD_ARG, "member " + std::to_string(r0 + i) + ": column + length = " +
                                              std::to_string((uint64_t)column[i] + ctx->len[r0 + i]) + " exceeds HMK_PROFILE_MAX_WIDTH");
    for (uint32_t i = 0; i < nm; i++) {
        const uint8_t *seq = ctx->res.data() + ctx->off[r0 + i];
        for (uint32_t k = 0; k < ctx->len[r0 + i]; k++)
            if (seq[k] >= PROFILE_RESIDUES)
                return fail(ctx, HMK_ERR_REFERENCE_WOULD_CRASH, "sequence " + std::to_string(r0 + i) + " holds a residue outside the 20 amino acids: "
                                                                "frequencyMatrix.get() is null for it (Statistics.java:286)");
    }

    // the widths and where every slot's columns begin
    hmk_profile_stats S{};
    for (uint32_t c = 0; c < n_clusters; c++) width[c] = 0;
    for (uint32_t i = 0; i < nm; i++) {
        uint32_t &w = width[member_cluster[i]];
        w = std::max<uint32_t>(w, column[i] + ctx->len[r0 + i]);
    }
    col_start[0] = 0;
    for (uint32_t c = 0; c < n_clusters; c++) col_start[c + 1] = col_start[c] + width[c];
    S.n_multi = count_slots(members).n_multi;
    S.omitted = n_clusters - S.n_multi;
    S.columns = col_start[n_clusters];
    S.system_kld_match = S.system_kld_all = std::nan("");
    if ((counts || ic || col_flags) && col_capacity < S.columns) {
        *stats = S;
        return fail(ctx, HMK_ERR_CAPACITY, "the per-column arrays hold " + std::to_string(col_capacity) + " columns, the slots have " +
                                           std::to_string(S.columns));
    }
    st = need_device(ctx);
    if (st) return st;
    if (nm == 0) {
        *stats = S;
        return HMK_OK;
    }
    if (S.columns >= ((uint64_t)1 << 32)) return fail(ctx, HMK_ERR_BAD_ARG, "2^32 columns or more");   // (n <= 2^24 keeps them below 96 * 2^24)

    LinkTables T;
    build_link_tables(r0, nm, member_cluster, n_clusters, members, T);
    const std::vector<uint32_t> &h = T.h;
    const uint32_t n_cols = (uint32_t)S.columns;

    // the call's own block: frequency | background (doubles), then mslot[nm] | column[nm] | size[ncl] | cstart[ncl + 1] | chunk[3 n_chunks]
    const uint32_t large_min = ctx->sw.profile_large_min >= 2 ? (uint32_t)ctx->sw.profile_large_min : PROFILE_LARGE_MIN;
    std::vector<uint32_t> chunk;
    auto add_chunks = [&](uint32_t slot, uint32_t place) {
        if (members[slot] < large_min) return;
        for (uint32_t b = 0; b < members[slot]; b += PROFILE_CHUNK) {
            chunk.push_back(place + b);
            chunk.push_back(std::min(PROFILE_CHUNK, members[slot] - b));
            chunk.push_back(slot);
        }
    };
    for (uint32_t f = 0; f < T.nf; f++) add_chunks(h[T.o_fslot + f], h[T.o_fmstart + f]);
    for (uint32_t g = 0; g < T.nb; g++) add_chunks(h[T.o_bslot + g], h[T.o_bmstart + g]);
    const uint32_t n_chunks = (uint32_t)(chunk.size() / 3);
    constexpr size_t FB_WORDS = 2 * 420;
    const size_t o_mslot = FB_WORDS, o_column = o_mslot + nm, o_size = o_column + nm, o_cstart = o_size + n_clusters,
                 o_chunk = o_cstart + n_clusters + 1, in_words = o_chunk + chunk.size();
    std::vector<uint32_t> hin(in_words);
    std::memcpy(hin.data(), P.frequency, 400 * sizeof(double));
    std::memcpy(hin.data() + 800, P.background, 20 * sizeof(double));
    for (uint32_t i = 0; i < nm; i++) {
        hin[o_mslot + i] = member_cluster[i];
        hin[o_column + i] = column[i];
        if (members[member_cluster[i]] < large_min) S.small_members++;
    }
    for (uint32_t c = 0; c < n_clusters; c++) { hin[o_size + c] = members[c]; hin[o_cstart + c] = (uint32_t)col_start[c]; }
    hin[o_cstart + n_clusters] = n_cols;
    std::copy(chunk.begin(), chunk.end(), hin.begin() + o_chunk);
    S.large_chunks = n_chunks;

    st = ensure_res32(ctx);
    if (st) return st;
    st = greedy_streams(ctx);
    if (st) return st;
    // per column: ic double[n_cols] | counts uint32[21 n_cols] | flags uint8[n_cols]
    // per member and slot: kld_match double[nm] | kld_all double[nm] | n_conserved uint32[ncl] | first uint32[ncl] | last uint32[ncl]
    const size_t col_bytes = (size_t)n_cols * (8 + 4 * PROFILE_SYMBOLS + 1), res_bytes = (size_t)nm * 16 + (size_t)n_clusters * 12;
    LinkView V;
    st = reserve_link_tables(ctx, T, &V);
    if (st) return st;
    HIPCHK(ctx, ensure_buf(ctx, SB_PROF_IN, in_words * 4));
    HIPCHK(ctx, ensure_buf(ctx, SB_PROF_COLS, col_bytes));
    HIPCHK(ctx, ensure_buf(ctx, SB_PROF_OUT, res_bytes));
    HIPCHK(ctx, ctx->h_merge.ensure(res_bytes + 64, 0));
    uint32_t *d_in = buf<uint32_t>(ctx, SB_PROF_IN);
    ProfileIn in;
    in.mslot = d_in + o_mslot;
    in.column = d_in + o_column;
    in.size = d_in + o_size;
    in.cstart = d_in + o_cstart;
    in.chunk = d_in + o_chunk;
    in.nm = nm;
    in.n_clusters = n_clusters;
    in.n_cols = n_cols;
    in.n_chunks = n_chunks;
    in.large_min = large_min;
    ProfileOut out;
    out.ic = buf<double>(ctx, SB_PROF_COLS);
    out.counts = reinterpret_cast<uint32_t *>(out.ic + n_cols);
    out.flags = reinterpret_cast<uint8_t *>(out.counts + (size_t)n_cols * PROFILE_SYMBOLS);
    out.kld_match = buf<double>(ctx, SB_PROF_OUT);
    out.kld_all = out.kld_match + nm;
    out.n_conserved = reinterpret_cast<uint32_t *>(out.kld_all + nm);
    out.first = out.n_conserved + n_clusters;
    out.last = out.first + n_clusters;
    ProfileParams K;
    K.min_ic = P.min_ic;
    K.max_gap_proportion = P.max_gap_proportion;
    K.beta = P.beta;
    K.sigma = P.sigma;
    K.scale = P.scale;
    K.allow_inner_gaps = P.allow_inner_gaps != 0;
    K.freq_bg = reinterpret_cast<const double *>(d_in);
    const uint8_t *res32 = ctx->d_res32.as<uint8_t>(), *len = ctx->d_len.as<uint8_t>();
    char *h_res = (char *)ctx->h_merge.p;
    hipStream_t Q = ctx->gstream;
    EventPair ev;
    HIPCHK(ctx, ev.create());
    hipError_t e = upload_link_tables(ctx, T, Q);
    if (e == hipSuccess) e = hipMemcpyAsync(d_in, hin.data(), in_words * 4, hipMemcpyHostToDevice, Q);
    if (e == hipSuccess) e = ev.start(Q);
    if (e == hipSuccess) e = launch_profile_init(in, out, Q);
    if (e == hipSuccess) e = launch_profile_counts_small(res32, len, r0, in, out.counts, Q);
    if (e == hipSuccess) e = launch_profile_counts_large(res32, len, V, r0, in, out.counts, Q);
    if (e == hipSuccess) e = launch_profile_columns(in, K, out, Q);
    if (e == hipSuccess) e = launch_profile_match(in, K, out, Q);
    if (e == hipSuccess) e = launch_profile_kld(res32, len, V, r0, in, K, out, Q);
    S.launches = 4 + (n_chunks ? 1 : 0) + (V.nt ? 1 : 0);
    if (e == hipSuccess) e = ev.stop(Q);
    if (e == hipSuccess) e = hipMemcpyAsync(h_res, out.kld_match, res_bytes, hipMemcpyDeviceToHost, Q);
    if (e == hipSuccess && ic) e = hipMemcpyAsync(ic, out.ic, (size_t)n_cols * 8, hipMemcpyDeviceToHost, Q);
    if (e == hipSuccess && counts) e = hipMemcpyAsync(counts, out.counts, (size_t)n_cols * PROFILE_SYMBOLS * 4, hipMemcpyDeviceToHost, Q);
    if (e == hipSuccess && col_flags) e = hipMemcpyAsync(col_flags, out.flags, n_cols, hipMemcpyDeviceToHost, Q);
    if (e == hipSuccess) e = hipStreamSynchronize(Q);
    float ms = 0;
    if (e == hipSuccess) e = ev.elapsed(&ms);
    if (e != hipSuccess) return fail_hip(ctx, "cluster profile", e);
    S.kernel_ms = ms;

    const double *h_match = (const double *)h_res, *h_all = h_match + nm;
    const uint32_t *h_cons = (const uint32_t *)(h_all + nm), *h_first = h_cons + n_clusters, *h_last = h_first + n_clusters;
    std::memcpy(kld_match, h_match, (size_t)nm * 8);
    std::memcpy(kld_all, h_all, (size_t)nm * 8);
    for (uint32_t c = 0; c < n_clusters; c++) {
        if (h_cons[c] > width[c] || (h_cons[c] && (h_first[c] > h_last[c] || h_last[c] >= width[c] || h_last[c] - h_first[c] + 1 < h_cons[c])))
            return fail(ctx, HMK_ERR_DEVICE, "cluster profile: slot " + std::to_string(c) + " came back with conserved columns outside its width");
        n_conserved[c] = h_cons[c];
        n_match[c] = (P.allow_inner_gaps || h_cons[c] == 0) ? h_cons[c] : h_last[c] - h_first[c] + 1;   // FileIOManager.java:1277-1297
        passes[c] = (int64_t)h_cons[c] >= (int64_t)P.min_conserved_positions;                            // :1180
        kld_match_mean[c] = kld_all_mean[c] = 0.0;
    }
    // the means, in member index order (Statistics.java:183, :196)
    double sys_match = 0.0, sys_all = 0.0;
    uint64_t sys_n = 0;
    for (uint32_t i = 0; i < nm; i++) {
        const uint32_t c = member_cluster[i];
        kld_match_mean[c] += kld_match[i];
        kld_all_mean[c] += kld_all[i];
        if (members[c] >= 2) { sys_match += kld_match[i]; sys_all += kld_all[i]; sys_n++; }
    }
    for (uint32_t c = 0; c < n_clusters; c++) {
        kld_match_mean[c] = kld_match_mean[c] / ((double)members[c] + 0.0);
        kld_all_mean[c] = kld_all_mean[c] / ((double)members[c] + 0.0);
    }
    S.system_kld_match = sys_match / ((double)sys_n + 0.0);   // (0.0 / 0.0 without a multi-member slot, as the reference's)
    S.system_kld_all = sys_all / ((double)sys_n + 0.0);
    *stats = S;
    return HMK_OK;
}

}  // namespace

} }  // namespace hmk::impl

extern "C" {

int hmk_cluster_profile(hmk_ctx *ctx, uint32_t r0, uint32_t r1, const uint32_t *member_cluster, uint32_t n_clusters, const uint32_t *column,
                        const hmk_profile_params *params, uint32_t *width, uint32_t *n_conserved, uint32_t *n_match, uint8_t *passes,
                        double *kld_match_mean, double *kld_all_mean, uint64_t *col_start, uint64_t col_capacity, uint32_t *counts, double *ic,
                        uint8_t *col_flags, double *kld_match, double *kld_all, hmk_profile_stats *stats) {
    return hmk::impl::cluster_profile(ctx, r0, r1, member_cluster, n_clusters, column, params, width, n_conserved, n_match, passes, kld_match_mean,
                                      kld_all_mean, col_start, col_capacity, counts, ic, col_flags, kld_match, kld_all, stats);
}

}  // extern "C"
