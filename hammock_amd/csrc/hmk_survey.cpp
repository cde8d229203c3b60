// hmk_survey.cpp -- the score survey of a pair space of the uploaded set: how many pairs score what (a histogram over a window of
// scores), each row's best partner and its number of partners at or above a threshold.  The pair space is the triangle inside one range
// (every unordered pair of distinct members, seq1 = the larger index: the orientation of hmk_cluster_linkage_shifted and of the
// neighbour edges) or the rectangle of two disjoint ranges (seq1 = the query, as hmk_search_shifted).
//   kernels  k_survey.hip on the clustering stream: accumulators cleared, every pair scored once by the literal scorer and reduced,
//            the rows' keys decoded;
//   results  one copy of the fixed block (bins, counters, score range) and one of the rows' block: O(bins + rows).
// No pass, no edge buffer, no plan: nothing proportional to the number of pairs exists anywhere, so no density ends in HMK_ERR_CAPACITY.
#include <atomic>

#include "hmk_ctx.h"
#include "hmk_slots.h"
#include "hmk_survey.h"

namespace hmk { namespace impl {

namespace {

std::atomic<int> g_hist_form{SURVEY_HIST_COPIES};

int score_survey(hmk_ctx *ctx, uint32_t q0, uint32_t q1, uint32_t r0, uint32_t r1, int X, int p, int thr, int score_lo, uint32_t n_bins,
                 uint64_t *hist, int32_t *best_score, uint32_t *best_index, uint32_t *degree, hmk_survey_stats *stats) {
    if (!ctx) return fail(nullptr, HMK_ERR_BAD_ARG, "null context");
    std::lock_guard<std::mutex> lock(ctx->mu);
    refresh_switches(ctx);
    if (q0 > q1 || r0 > r1 || q1 > ctx->n || r1 > ctx->n)
        return fail(ctx, HMK_ERR_BAD_ARG, "survey ranges must lie within [0, n) with q0 <= q1 and r0 <= r1 (n = " + std::to_string(ctx->n) + ")");
    const uint32_t nq = q1 - q0, nr = r1 - r0;
    const bool triangle = nq && q0 == r0 && q1 == r1;
    if (!triangle && nq && nr && q0 < r1 && r0 < q1)
        return fail(ctx, HMK_ERR_BAD_ARG, "the two ranges of a survey are the same range (a triangle) or disjoint (a rectangle): these overlap in part");
    if (n_bins > HMK_SURVEY_MAX_BINS) return fail(ctx, HMK_ERR_BAD_ARG, "n_bins above HMK_SURVEY_MAX_BINS (" + std::to_string(HMK_SURVEY_MAX_BINS) + ")");
    if ((hist == nullptr) != (n_bins == 0)) return fail(ctx, HMK_ERR_BAD_ARG, "hist is null if and only if n_bins is 0");
    const int row_ptrs = (best_score != nullptr) + (best_index != nullptr) + (degree != nullptr);
    if (row_ptrs != 0 && row_ptrs != 3) return fail(ctx, HMK_ERR_BAD_ARG, "best_score, best_index and degree are given together or not at all");
    const bool rows = row_ptrs == 3;
    if (!stats) return fail(ctx, HMK_ERR_BAD_ARG, "stats must not be null");
    const uint64_t pairs = triangle ? (uint64_t)nq * (nq - 1) / 2 : (uint64_t)nq * nr;
    if (pairs && !hist && !rows) return fail(ctx, HMK_ERR_BAD_ARG, "nothing to compute: neither a histogram nor the row outputs are wanted");
    if (triangle && !ctx->symmetric)
        return fail(ctx, HMK_ERR_BAD_ARG, "the survey of a triangle needs a symmetric scoring matrix: the score of an unordered pair must not "
                                          "depend on which member comes first");
    int st = need_device(ctx);
    if (st) return st;
    hmk_survey_stats S{};
    S.score_min = INT32_MAX;
    S.score_max = INT32_MIN;
    for (uint32_t k = 0; k < n_bins; k++) hist[k] = 0;
    for (uint32_t i = 0; rows && i < nq; i++) { best_score[i] = INT32_MIN; best_index[i] = 0xFFFFFFFFu; degree[i] = 0; }
    if (pairs == 0) {
        *stats = S;
        return HMK_OK;
    }
    // (nothing is range-checked against the threshold: 0 passes the threshold's own check)
    st = check_link_scores(ctx, X, p, 0, q0, q1);
    if (st == HMK_OK && !triangle) st = check_link_scores(ctx, X, p, 0, r0, r1);
    if (st) return st;
    // no score leaves [-32,768, 32,767] (check_link_scores): beyond +-100,000 a threshold or a window's start compares with every score as
    // +-100,000 does (n_bins <= 1,024), and the kernel's 32-bit differences cannot wrap
    const int thr_dev = std::max(-100000, std::min(100000, thr)), lo_dev = std::max(-100000, std::min(100000, score_lo));

    st = ensure_res32(ctx);
    if (st) return st;
    st = greedy_streams(ctx);
    if (st) return st;
    // fixed: hist uint64[MAX_BINS] | counts uint64[4] | range int32[2] (+ pad); rows: key uint64[nq] | best_score int32[nq] |
    // best_index uint32[nq] | degree uint32[nq]
    const size_t fixed_bytes = (size_t)(HMK_SURVEY_MAX_BINS + 4) * 8 + 16, row_bytes = rows ? (size_t)nq * 20 : 0;
    HIPCHK(ctx, ensure_buf(ctx, SB_SURVEY_ACC, fixed_bytes));
    if (rows) HIPCHK(ctx, ensure_buf(ctx, SB_SURVEY_ROWS, row_bytes));
    HIPCHK(ctx, ctx->h_merge.ensure(fixed_bytes + (size_t)nq * 12 + 64, 0));
    SurveyAcc acc{};
    acc.hist = buf<unsigned long long>(ctx, SB_SURVEY_ACC);
    acc.counts = acc.hist + HMK_SURVEY_MAX_BINS;
    acc.range = reinterpret_cast<int32_t *>(acc.counts + 4);
    if (rows) {
        acc.rowkey = buf<unsigned long long>(ctx, SB_SURVEY_ROWS);
        acc.best_score = reinterpret_cast<int32_t *>(acc.rowkey + nq);
        acc.best_index = reinterpret_cast<uint32_t *>(acc.best_score + nq);
        acc.degree = acc.best_index + nq;
    }
    const uint8_t *res32 = ctx->d_res32.as<uint8_t>(), *len = ctx->d_len.as<uint8_t>();
    const int32_t *d_M = ctx->d_M.as<int32_t>();
    char *h_fixed = (char *)ctx->h_merge.p, *h_rows = h_fixed + fixed_bytes;
    hipStream_t Q = ctx->gstream;
    EventPair ev;
    HIPCHK(ctx, ev.create());
    hipError_t e = ev.start(Q);
    if (e == hipSuccess) e = launch_survey_init(acc, n_bins, nq, Q);
    if (e == hipSuccess) e = launch_survey_tiled(res32, len, d_M, triangle, q0, nq, r0, nr, X, p, thr_dev, lo_dev, n_bins, g_hist_form.load(), acc, Q);
    if (e == hipSuccess) e = launch_survey_decode(acc, nq, Q);
    S.launches = rows ? 3 : 2;
    if (e == hipSuccess) e = ev.stop(Q);
    if (e == hipSuccess) e = hipMemcpyAsync(h_fixed, acc.hist, fixed_bytes, hipMemcpyDeviceToHost, Q);
    if (e == hipSuccess && rows) e = hipMemcpyAsync(h_rows, acc.best_score, (size_t)nq * 12, hipMemcpyDeviceToHost, Q);
    if (e == hipSuccess) e = hipStreamSynchronize(Q);
    float ms = 0;
    if (e == hipSuccess) e = ev.elapsed(&ms);
    if (e != hipSuccess) return fail_hip(ctx, "score survey", e);
    S.kernel_ms = ms;

    const uint64_t *h_hist = (const uint64_t *)h_fixed, *h_counts = h_hist + HMK_SURVEY_MAX_BINS;
    const int32_t *h_range = (const int32_t *)(h_counts + 4);
    if (n_bins) std::memcpy(hist, h_hist, (size_t)n_bins * 8);
    S.pairs_scored = pairs;
    S.n_below = n_bins ? h_counts[SURVEY_BELOW] : 0;
    S.n_above = n_bins ? h_counts[SURVEY_ABOVE] : 0;
    S.n_at_or_above = h_counts[SURVEY_AT_OR_ABOVE];
    S.score_min = h_range[0];
    S.score_max = h_range[1];
    if (S.score_min > S.score_max) return fail(ctx, HMK_ERR_DEVICE, "score survey: the pairs came back without a score");
    if (rows) {
        std::memcpy(best_score, h_rows, (size_t)nq * 4);
        std::memcpy(best_index, h_rows + (size_t)nq * 4, (size_t)nq * 4);
        std::memcpy(degree, h_rows + (size_t)nq * 8, (size_t)nq * 4);
    }
    *stats = S;
    return HMK_OK;
}

}  // namespace

} }  // namespace hmk::impl

extern "C" {

int hmk_score_survey_shifted(hmk_ctx *ctx, uint32_t q0, uint32_t q1, uint32_t r0, uint32_t r1, int max_shift, int shift_penalty, int threshold,
                             int score_lo, uint32_t n_bins, uint64_t *hist, int32_t *best_score, uint32_t *best_index, uint32_t *degree,
                             hmk_survey_stats *stats) {
    return hmk::impl::score_survey(ctx, q0, q1, r0, r1, max_shift, shift_penalty, threshold, score_lo, n_bins, hist, best_score, best_index, degree,
                                   stats);
}

// Not part of the ABI and not in the public header: the LDS histogram form (SURVEY_HIST_*) the following calls of this process run, for
// tools/bench_survey.py, which times both forms side by side.  -> the form that was set before.
int hmk_survey_hist_form_for_measurement(int form) {
    return hmk::impl::g_hist_form.exchange(form == hmk::SURVEY_HIST_WAVE ? hmk::SURVEY_HIST_WAVE : hmk::SURVEY_HIST_COPIES);
}

}  // extern "C"
