// hmk_scan.cpp -- the scan of peptides along long targets: the second resident set (hmk_set_targets), the argument checks a
// host-only context answers, the work lists of a call (queries by length in runs of groups of 8, targets in chunks), which classes
// the byte-lane form takes (hmk_scan.h), the pass into a grow-only hit buffer, pair mode's reduction and the coverage (k_scan.hip),
// the extern "C" entry points.  DESIGN.md 5.25.
#include "hmk_ctx.h"
#include "hmk_scan.h"

namespace hmk { namespace impl {

namespace {

struct ScanWork {
    std::vector<uint32_t> qlist;
    std::vector<ScanRun> runs;
    std::vector<ScanChunk> chunks;
    uint32_t run0[HMK_MAX_LEN + 2] = {0};   // runs of length m: [run0[m], run0[m + 1])
    uint64_t table_entries = 0;
    uint64_t windows = 0, windows_packed = 0;
    uint64_t packed_of_len[HMK_MAX_LEN + 1] = {0};   // of windows_packed: by peptide length (a length without any needs no launch)
};

// the call's lists, and how many windows each form scores (the rule the kernels apply per (group, target): scan_bound_limit)
void build_work(const hmk_ctx *ctx, uint32_t q0, uint32_t q1, uint32_t t0, uint32_t t1, int X, int p, int thr, ScanWork &W) {
    const int bias = ctx->min_m < 0 ? -ctx->min_m : 0;
    std::vector<uint32_t> by_len[HMK_MAX_LEN + 1];
    for (uint32_t q = q0; q < q1; q++) by_len[ctx->len[q]].push_back(q);
    // per length: the groups' bounds, ascending, with the peptides they hold (for the counters)
    std::vector<std::pair<long long, uint32_t>> bounds[HMK_MAX_LEN + 1];
    uint64_t n_of_len[HMK_MAX_LEN + 1] = {0};
    for (int m = 1; m <= HMK_MAX_LEN; m++) {
        W.run0[m] = (uint32_t)W.runs.size();
        const std::vector<uint32_t> &L = by_len[m];
        n_of_len[m] = L.size();
        for (size_t f = 0; f < L.size(); f += SCAN_GROUP * SCAN_RUN_GROUPS) {
            ScanRun R{};
            R.first = (uint32_t)(W.qlist.size() + f);
            R.count = (uint32_t)std::min<size_t>(SCAN_GROUP * SCAN_RUN_GROUPS, L.size() - f);
            R.m = (uint32_t)m;
            R.table = (uint32_t)W.table_entries;
            W.table_entries += (uint64_t)SCAN_RUN_GROUPS * m * SCAN_COLUMNS;
            for (uint32_t g = 0; g * SCAN_GROUP < R.count; g++) {
                long long b = 0;
                const uint32_t in_group = std::min<uint32_t>(SCAN_GROUP, R.count - g * SCAN_GROUP);
                for (uint32_t k = 0; k < in_group; k++) {
                    const uint32_t q = L[f + g * SCAN_GROUP + k];
                    b = std::max(b, scan_row_bound(ctx->M, ctx->res.data() + ctx->off[q], m));
                }
                R.bound[g] = (int32_t)b;
                bounds[m].push_back({b, in_group});
            }
            W.runs.push_back(R);
        }
        W.qlist.insert(W.qlist.end(), L.begin(), L.end());
    }
    W.run0[HMK_MAX_LEN + 1] = (uint32_t)W.runs.size();
    std::vector<uint64_t> prefix[HMK_MAX_LEN + 1];   // peptides in the groups with the k smallest bounds
    for (int m = 1; m <= HMK_MAX_LEN; m++) {
        std::sort(bounds[m].begin(), bounds[m].end());
        prefix[m].assign(bounds[m].size() + 1, 0);
        for (size_t k = 0; k < bounds[m].size(); k++) prefix[m][k + 1] = prefix[m][k] + bounds[m][k].second;
    }
    for (uint32_t t = t0; t < t1; t++) {
        const uint64_t n = ctx->toff[t + 1] - ctx->toff[t];
        for (uint32_t w0 = 0; w0 < n + 2 * (uint64_t)X; w0 += SCAN_CHUNK) W.chunks.push_back({t, w0});   // (a length-1 peptide has n + 2X windows)
        for (int m = 1; m <= HMK_MAX_LEN; m++) {
            if (!n_of_len[m]) continue;
            const long long d = (long long)n - m;
            const uint64_t nwin = (uint64_t)(d + 2 * X + 1);
            W.windows += nwin * n_of_len[m];
            if (ctx->sw.no_scan_packed) continue;
            const long long limit = scan_bound_limit(m, X, p, thr, d, bias, ctx->max_m);
            if (limit < 0) continue;
            const size_t k = std::upper_bound(bounds[m].begin(), bounds[m].end(), std::make_pair(limit, 0xFFFFFFFFu)) - bounds[m].begin();
            W.windows_packed += nwin * prefix[m][k];
            W.packed_of_len[m] += nwin * prefix[m][k];
        }
    }
}

struct EventTimer {
    EventPair ev;   // (made at the first begin)
    double ms = 0;
    hipError_t begin() {
        const hipError_t e = ev.b ? hipSuccess : ev.create();
        return e == hipSuccess ? ev.start(nullptr) : e;
    }
    hipError_t end(bool add) {   // waits for the work; add: its time counts
        hipError_t e = ev.stop(nullptr);
        if (e == hipSuccess) e = hipEventSynchronize(ev.b);
        float t = 0;
        if (e == hipSuccess) e = ev.elapsed(&t);
        if (add) ms += t;
        return e;
    }
};

int scan_on_device(hmk_ctx *ctx, uint32_t q0, uint32_t q1, uint32_t t0, uint32_t t1, int X, int p, int thr, bool all_windows,
                   hmk_scan_hit *hits, uint64_t capacity, uint32_t *coverage_count, uint64_t *coverage_size, hmk_scan_stats &S) {
    ScanWork W;
    build_work(ctx, q0, q1, t0, t1, X, p, thr, W);
    S.windows_scored = W.windows;
    S.windows_packed = W.windows_packed;
    S.windows_literal = W.windows - W.windows_packed;
    S.n_tiles = (uint32_t)std::min<uint64_t>((uint64_t)W.chunks.size() * W.runs.size(), 0xFFFFFFFFu);
    if (W.table_entries > 0xFFFFFFFFull) return fail(ctx, HMK_ERR_OOM, "the query range needs more than 2^32 table entries: scan it in parts");
    if (W.chunks.size() > 0xFFFFFFFFull) return fail(ctx, HMK_ERR_OOM, "more than 2^32 - 1 target chunks: scan the targets in parts");

    int st = ensure_res32(ctx);
    if (st) return st;
    if (!ctx->targets_on_device) {
        HIPCHK(ctx, ensure_buf(ctx, SB_SCAN_TRES, std::max<size_t>(ctx->tres.size(), 1)));
        HIPCHK(ctx, ensure_buf(ctx, SB_SCAN_TOFF, ctx->toff.size() * sizeof(uint64_t)));
        if (!ctx->tres.empty()) HIPCHK(ctx, hipMemcpy(buf<void>(ctx, SB_SCAN_TRES), ctx->tres.data(), ctx->tres.size(), hipMemcpyHostToDevice));
        HIPCHK(ctx, hipMemcpy(buf<void>(ctx, SB_SCAN_TOFF), ctx->toff.data(), ctx->toff.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
        ctx->targets_on_device = true;
    }
    // the call's lists in one block: query list | runs | chunks (each 16-byte aligned)
    auto up16 = [](size_t b) { return (b + 15) / 16 * 16; };
    const size_t b_q = up16(W.qlist.size() * 4), b_r = up16(W.runs.size() * sizeof(ScanRun)), b_c = up16(W.chunks.size() * sizeof(ScanChunk));
    HIPCHK(ctx, ensure_buf(ctx, SB_SCAN_PLAN, b_q + b_r + b_c));
    char *d_plan = buf<char>(ctx, SB_SCAN_PLAN);
    HIPCHK(ctx, hipMemcpy(d_plan, W.qlist.data(), W.qlist.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemcpy(d_plan + b_q, W.runs.data(), W.runs.size() * sizeof(ScanRun), hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemcpy(d_plan + b_q + b_r, W.chunks.data(), W.chunks.size() * sizeof(ScanChunk), hipMemcpyHostToDevice));
    if (W.windows_packed) HIPCHK(ctx, ensure_buf(ctx, SB_SCAN_TAB, W.table_entries * 8));   // (the literal form reads no tables)
    HIPCHK(ctx, ensure_buf(ctx, SB_SCAN_CNT, 2 * sizeof(unsigned long long)));
    HIPCHK(ctx, ensure_buf(ctx, SB_SCAN_HITS, SCAN_FIRST_HITS * sizeof(hmk_scan_hit)));
    unsigned long long *d_cnt = buf<unsigned long long>(ctx, SB_SCAN_CNT);

    ScanParams P{};
    P.res32 = ctx->d_res32.as<uint8_t>();
    P.qlist = (const uint32_t *)d_plan;
    P.runs = (const ScanRun *)(d_plan + b_q);
    P.chunks = (const ScanChunk *)(d_plan + b_q + b_r);
    P.tres = buf<uint8_t>(ctx, SB_SCAN_TRES);
    P.toff = buf<uint64_t>(ctx, SB_SCAN_TOFF);
    P.M = ctx->d_M.as<int32_t>();
    P.tables = W.windows_packed ? buf<uint64_t>(ctx, SB_SCAN_TAB) : nullptr;
    P.count = d_cnt;
    P.n_runs = (uint32_t)W.runs.size();
    P.n_chunks = (uint32_t)W.chunks.size();
    P.X = X; P.p = p; P.thr = thr;
    P.bias = ctx->min_m < 0 ? -ctx->min_m : 0;
    P.max_m = ctx->max_m;
    P.no_packed = ctx->sw.no_scan_packed ? 1u : 0u;

    EventTimer T;
    // the pass, into a hit buffer that grows to what the pass before it needed
    unsigned long long found = 0;
    for (int attempt = 0;; attempt++) {
        P.hits = buf<hmk_scan_hit>(ctx, SB_SCAN_HITS);
        P.cap = ctx->sb[SB_SCAN_HITS].cap / sizeof(hmk_scan_hit);
        HIPCHK(ctx, hipMemset(d_cnt, 0, 2 * sizeof(unsigned long long)));
        HIPCHK(ctx, T.begin());   // (a pass that overflowed the buffer and is repeated counts too: kernel_ms and launches are what the call spent)
        if (S.windows_packed) {
            if (attempt == 0) {   // (the tables do not depend on the hit buffer)
                HIPCHK(ctx, launch_scan_tables(P, buf<uint64_t>(ctx, SB_SCAN_TAB), nullptr));
                S.launches++;
            }
            for (int m = SCAN_PACKED_MIN_LEN; m <= SCAN_PACKED_MAX_LEN; m++) {
                if (!W.packed_of_len[m]) continue;
                HIPCHK(ctx, launch_scan_packed(m, P, W.run0[m], W.run0[m + 1] - W.run0[m], nullptr));
                S.launches++;
            }
        }
        if (S.windows_literal) {
            HIPCHK(ctx, launch_scan_literal(P, nullptr));
            S.launches++;
        }
        HIPCHK(ctx, T.end(true));
        HIPCHK(ctx, hipMemcpy(&found, d_cnt, sizeof(found), hipMemcpyDeviceToHost));
        if (found <= P.cap) break;
        if (attempt == 2) return fail(ctx, HMK_ERR_DEVICE, "internal hit buffer kept overflowing");
        HIPCHK(ctx, ensure_buf(ctx, SB_SCAN_HITS, (size_t)found * sizeof(hmk_scan_hit)));
    }
    S.window_hits = found;

    const hmk_scan_hit *d_rec = P.hits;
    uint64_t n_rec = found;
    const uint32_t nt = t1 - t0;
    if (!all_windows && found) {
        uint64_t slots = 1024;
        while (slots < 2 * found) slots <<= 1;
        HIPCHK(ctx, ensure_buf(ctx, SB_SCAN_HASH, (size_t)slots * 16));
        HIPCHK(ctx, ensure_buf(ctx, SB_SCAN_PAIRS, (size_t)found * sizeof(hmk_scan_hit)));
        unsigned long long *keys = buf<unsigned long long>(ctx, SB_SCAN_HASH), *vals = keys + slots;
        HIPCHK(ctx, T.begin());
        HIPCHK(ctx, hipMemsetAsync(keys, 0, (size_t)slots * 16, nullptr));
        HIPCHK(ctx, launch_scan_pairs(P.hits, found, q0, t0, nt, X, keys, vals, slots, buf<hmk_scan_hit>(ctx, SB_SCAN_PAIRS), found, d_cnt + 1, nullptr));
        S.launches += 2;
        HIPCHK(ctx, T.end(true));
        unsigned long long pairs = 0;
        HIPCHK(ctx, hipMemcpy(&pairs, d_cnt + 1, sizeof(pairs), hipMemcpyDeviceToHost));
        if (pairs > found) return fail(ctx, HMK_ERR_DEVICE, "internal: more pairs than window hits");
        d_rec = buf<hmk_scan_hit>(ctx, SB_SCAN_PAIRS);
        n_rec = pairs;
    }
    S.n_hits = n_rec;
    S.kernel_ms = T.ms;
    if (n_rec > capacity) return fail(ctx, HMK_ERR_CAPACITY, "hit buffer too small: " + std::to_string(n_rec) + " needed");

    if (coverage_count || coverage_size) {
        const uint64_t total = ctx->toff[t1] - ctx->toff[t0];
        const size_t b_cc = up16((size_t)total * 4);
        HIPCHK(ctx, ensure_buf(ctx, SB_SCAN_COV, b_cc + (size_t)total * 8));
        uint32_t *d_cc = buf<uint32_t>(ctx, SB_SCAN_COV);
        unsigned long long *d_cs = (unsigned long long *)(buf<char>(ctx, SB_SCAN_COV) + b_cc);
        const int32_t *d_sizes = nullptr;
        if (ctx->has_sizes) {
            HIPCHK(ctx, ensure_buf(ctx, SB_SCAN_SIZES, (size_t)ctx->n * 4));
            HIPCHK(ctx, hipMemcpy(buf<void>(ctx, SB_SCAN_SIZES), ctx->sizes.data(), (size_t)ctx->n * 4, hipMemcpyHostToDevice));
            d_sizes = buf<int32_t>(ctx, SB_SCAN_SIZES);
        }
        HIPCHK(ctx, T.begin());
        HIPCHK(ctx, hipMemsetAsync(d_cc, 0, b_cc + (size_t)total * 8, nullptr));
        HIPCHK(ctx, launch_scan_coverage(d_rec, n_rec, ctx->d_len.as<uint8_t>(), d_sizes, P.toff, t0, nt, d_cc, d_cs, nullptr));
        S.launches += n_rec ? 2 : 1;
        HIPCHK(ctx, T.end(true));
        S.kernel_ms = T.ms;
        if (coverage_count) HIPCHK(ctx, hipMemcpy(coverage_count, d_cc, (size_t)total * 4, hipMemcpyDeviceToHost));
        if (coverage_size) HIPCHK(ctx, hipMemcpy(coverage_size, d_cs, (size_t)total * 8, hipMemcpyDeviceToHost));
    }
    if (n_rec) HIPCHK(ctx, hipMemcpy(hits, d_rec, (size_t)n_rec * sizeof(hmk_scan_hit), hipMemcpyDeviceToHost));
    return HMK_OK;
}

}  // namespace

} }  // namespace hmk::impl

extern "C" {

int hmk_set_targets(hmk_ctx *ctx, const uint8_t *residues, const uint64_t *offsets, uint32_t n_targets) {
    if (!ctx) return fail(nullptr, HMK_ERR_BAD_ARG, "null context");
    std::lock_guard<std::mutex> lock(ctx->mu);
    refresh_switches(ctx);
    if (n_targets && (!residues || !offsets)) return fail(ctx, HMK_ERR_BAD_ARG, "null target residues/offsets");
    if (n_targets && offsets[0] != 0) return fail(ctx, HMK_ERR_BAD_ARG, "target offsets[0] must be 0");
    for (uint32_t t = 0; t < n_targets; t++) {
        if (offsets[t + 1] < offsets[t]) return fail(ctx, HMK_ERR_BAD_ARG, "target offsets must ascend");
        const uint64_t l = offsets[t + 1] - offsets[t];
        if (l <= HMK_MAX_LEN)
            return fail(ctx, HMK_ERR_BAD_ARG, "target " + std::to_string(t) + " has " + std::to_string(l) + " residues: a target is longer than " +
                                                  std::to_string(HMK_MAX_LEN) + "; shorter ones are sequences (hmk_set_sequences, hmk_search_shifted)");
        if (l > HMK_TARGET_MAX_LEN)
            return fail(ctx, HMK_ERR_BAD_ARG, "target " + std::to_string(t) + " has " + std::to_string(l) + " residues: at most " +
                                                  std::to_string(HMK_TARGET_MAX_LEN) + " (cut it into overlapping pieces)");
        if (offsets[t + 1] > 0x7FFFFFFFull) return fail(ctx, HMK_ERR_BAD_ARG, "more than 2^31 - 1 target residues in all");
    }
    const uint64_t total = n_targets ? offsets[n_targets] : 0;
    for (uint64_t k = 0; k < total; k++)
        if (residues[k] >= HMK_ALPHABET) return fail(ctx, HMK_ERR_BAD_ARG, "target residue index >= 24");
    ctx->n_targets = n_targets;
    ctx->tres.assign(residues, residues + total);
    if (n_targets) ctx->toff.assign(offsets, offsets + n_targets + 1);
    else ctx->toff.assign(1, 0);
    ctx->targets_on_device = false;
    return HMK_OK;
}

int hmk_scan_shifted(hmk_ctx *ctx, uint32_t q0, uint32_t q1, uint32_t t0, uint32_t t1, int max_shift, int shift_penalty, int threshold,
                     uint32_t flags, hmk_scan_hit *hits, uint64_t capacity, uint32_t *coverage_count, uint64_t *coverage_size,
                     hmk_scan_stats *stats) {
    if (!ctx) return fail(nullptr, HMK_ERR_BAD_ARG, "null context");
    std::lock_guard<std::mutex> lock(ctx->mu);
    refresh_switches(ctx);
    if (!stats) return fail(ctx, HMK_ERR_BAD_ARG, "stats must not be null");
    *stats = hmk_scan_stats{};
    if (capacity && !hits) return fail(ctx, HMK_ERR_BAD_ARG, "null hit buffer");
    if (flags & ~HMK_SCAN_ALL_WINDOWS) return fail(ctx, HMK_ERR_BAD_ARG, "unknown flag bits");
    if (max_shift < 0) return fail(ctx, HMK_ERR_BAD_ARG, "max_shift must be >= 0");
    if (threshold < -30000 || threshold > 30000) return fail(ctx, HMK_ERR_BAD_ARG, "threshold outside [-30000, 30000]");
    {   // int32 window sums: the penalties of the longest target and 32 cells at the matrix's largest magnitude
        const long long absp = shift_penalty < 0 ? -(long long)shift_penalty : shift_penalty;
        const long long absm = std::max<long long>(std::llabs((long long)ctx->min_m), std::llabs((long long)ctx->max_m));
        if (absp * ((long long)HMK_TARGET_MAX_LEN + 2LL * max_shift) + 32 * absm >= (1LL << 30))
            return fail(ctx, HMK_ERR_BAD_ARG, "shift_penalty too large: window scores would not fit 2^30");
    }
    if (ctx->n == 0) return fail(ctx, HMK_ERR_NO_SEQUENCES, "no sequences set (hmk_set_sequences)");
    if (t1 > t0 && ctx->n_targets == 0) return fail(ctx, HMK_ERR_NO_SEQUENCES, "no targets set (hmk_set_targets)");
    if (q0 > q1 || q1 > ctx->n)
        return fail(ctx, HMK_ERR_BAD_ARG, "the query range must lie within [0, n) with q0 <= q1 (n = " + std::to_string(ctx->n) + ")");
    if (t0 > t1 || t1 > ctx->n_targets)
        return fail(ctx, HMK_ERR_BAD_ARG, "the target range must lie within [0, n_targets) with t0 <= t1 (n_targets = " +
                                              std::to_string(ctx->n_targets) + ")");
    if (q0 < q1) {
        int shortest = HMK_MAX_LEN;
        for (uint32_t q = q0; q < q1; q++) shortest = std::min<int>(shortest, ctx->len[q]);
        if (max_shift >= shortest)
            return fail(ctx, HMK_ERR_SHIFT_TOO_BIG, "Shift too big: " + std::to_string(shortest - 1) + " is maximum, but " +
                                                        std::to_string(max_shift) + " found");   // ShiftedScorer.java:59-62
    }
    const uint64_t cov_total = t0 < t1 ? ctx->toff[t1] - ctx->toff[t0] : 0;
    if (q0 == q1 || t0 == t1) {
        if (coverage_count) std::fill(coverage_count, coverage_count + cov_total, 0u);
        if (coverage_size) std::fill(coverage_size, coverage_size + cov_total, (uint64_t)0);
        return HMK_OK;
    }
    int st = need_device(ctx);
    if (st) return st;
    hmk_scan_stats S{};
    st = scan_on_device(ctx, q0, q1, t0, t1, max_shift, shift_penalty, threshold, (flags & HMK_SCAN_ALL_WINDOWS) != 0, hits, capacity,
                        coverage_count, coverage_size, S);
    *stats = S;
    return st;
}

}  // extern "C"
