// hmk_traceback.cpp -- hmk_align_pairs_global: the gapped alignments of a pair list.  The checks, the chunks of 2^24 pairs and the
// timing are score_pairs' (hmk_pass.cpp); the kernel is k_traceback.hip.  21 bytes per pair come back: score, n_cols, gap1, gap2.
#include "hmk_ctx.h"
#include "hmk_traceback.h"

namespace hmk { namespace impl {

int align_pairs_global(hmk_ctx *ctx, const uint32_t *i, const uint32_t *j, uint64_t n_pairs, int gap_open, int gap_extend, int32_t *score,
                       uint8_t *n_cols, uint64_t *gap1, uint64_t *gap2) {
    std::lock_guard<std::mutex> lock(ctx->mu);
    refresh_switches(ctx);
    int st = check_global_fits(ctx, gap_open, gap_extend, 0);
    if (st) return st;
    st = need_device(ctx);
    if (st) return st;
    st = check_pairs(ctx, i, j, n_pairs, false, 0);
    if (st) return st;
    if (n_pairs && (!score || !n_cols || !gap1 || !gap2)) return fail(ctx, HMK_ERR_BAD_ARG, "null output (score, n_cols, gap1, gap2)");
    st = ensure_res32(ctx);
    if (st) return st;
    ctx->last_kernel_ms = 0;
    if (n_pairs == 0) return HMK_OK;
    const uint64_t ch = std::min<uint64_t>(1ull << 24, n_pairs);
    uint32_t *d_i = nullptr, *d_j = nullptr;
    int32_t *d_score = nullptr;
    uint8_t *d_cols = nullptr;
    unsigned long long *d_g1 = nullptr, *d_g2 = nullptr;
    hipError_t e = hipMalloc((void **)&d_i, ch * 4);
    if (e == hipSuccess) e = hipMalloc((void **)&d_j, ch * 4);
    if (e == hipSuccess) e = hipMalloc((void **)&d_score, ch * 4);
    if (e == hipSuccess) e = hipMalloc((void **)&d_cols, ch);
    if (e == hipSuccess) e = hipMalloc((void **)&d_g1, ch * 8);
    if (e == hipSuccess) e = hipMalloc((void **)&d_g2, ch * 8);
    for (uint64_t o = 0; o < n_pairs && e == hipSuccess; o += ch) {
        const uint64_t m = std::min(ch, n_pairs - o);
        e = hipMemcpy(d_i, i + o, m * 4, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(d_j, j + o, m * 4, hipMemcpyHostToDevice);
        const double acc = ctx->last_kernel_ms;   // (timer_start clears it: the chunks' times are summed)
        timer_start(ctx);
        if (e == hipSuccess)
            e = launch_traceback_global(ctx->max_len, ctx->d_res32.as<uint8_t>(), ctx->d_len.as<uint8_t>(), ctx->d_M.as<int32_t>(), d_i, d_j, m,
                                        gap_open, gap_extend, d_score, d_cols, d_g1, d_g2, nullptr);
        timer_stop(ctx);
        ctx->last_kernel_ms += acc;
        if (e == hipSuccess) e = hipMemcpy(score + o, d_score, m * 4, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(n_cols + o, d_cols, m, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(gap1 + o, d_g1, m * 8, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(gap2 + o, d_g2, m * 8, hipMemcpyDeviceToHost);
    }
    (void)hipFree(d_i);
    (void)hipFree(d_j);
    (void)hipFree(d_score);
    (void)hipFree(d_cols);
    (void)hipFree(d_g1);
    (void)hipFree(d_g2);
    if (e != hipSuccess) return fail(ctx, HMK_ERR_DEVICE, std::string("align_pairs_global: ") + hipGetErrorString(e));
    return HMK_OK;
}

} }  // namespace hmk::impl

extern "C" int hmk_align_pairs_global(hmk_ctx *ctx, const uint32_t *i, const uint32_t *j, uint64_t n_pairs, int gap_open, int gap_extend,
                                      int32_t *score, uint8_t *n_cols, uint64_t *gap1, uint64_t *gap2) {
    if (!ctx) return hmk::impl::fail(nullptr, HMK_ERR_BAD_ARG, "null context");
    return hmk::impl::align_pairs_global(ctx, i, j, n_pairs, gap_open, gap_extend, score, n_cols, gap1, gap2);
}
