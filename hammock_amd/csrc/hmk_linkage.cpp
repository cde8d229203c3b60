// hmk_linkage.cpp -- complete-linkage scores inside given clusters: per slot ClinkageClusterScorer.clusterScore without its early
// exit (ClinkageClusterScorer.java:30-49), applied to the pairs inside ONE cluster; the half of the question "is this clustering a
// fixed point of complete linkage" that hmk_cluster_pairs_shifted (hmk_merge.cpp, the pairs between clusters) leaves open.
//   tables   on the host, O(members + clusters): the members by slot in index order, the small slots' first, with the prefix sums
//            the kernels decode their work from (pairs of the small slots, tiles of the large ones);
//   kernels  k_linkage.hip on the clustering stream: accumulators cleared, small slots flat, large slots tiled;
//   results  the accumulators back to the host, the slots' keys decoded there (O(clusters)).
// No pass, no edge buffer, no plan: nothing proportional to the number of pairs exists anywhere.
#include "hmk_ctx.h"
#include "hmk_linkage.h"

namespace hmk {

void build_link_tables(uint32_t r0, uint32_t nm, const uint32_t *member_cluster, uint32_t n_clusters, const std::vector<uint32_t> &members,
                       LinkTables &T) {
    uint32_t nf = 0, nb = 0, flat_members = 0, big_members = 0;
    for (uint32_t c = 0; c < n_clusters; c++) {
        if (members[c] < 2) continue;
        if (members[c] <= (uint32_t)LINK_FLAT_MAX) { nf++; flat_members += members[c]; }
        else { nb++; big_members += members[c]; }
    }
    const size_t o_tab = 0, o_fslot = o_tab + flat_members + big_members, o_fmstart = o_fslot + nf, o_bslot = o_fmstart + nf + 1,
                 o_bmstart = o_bslot + nb, o_btstart = o_bmstart + nb + 1, o_fpstart = (o_btstart + nb + 1 + 1) & ~(size_t)1,
                 o_tbase = o_fpstart + 2 * ((size_t)nf + 1), words = o_tbase + 2 * ((size_t)nb + 1);
    std::vector<uint32_t> &h = T.h;
    h.assign(words, 0);
    std::vector<uint32_t> place(n_clusters, 0);   // where the slot's next member goes in tab
    unsigned long long *fpstart = reinterpret_cast<unsigned long long *>(h.data() + o_fpstart);
    unsigned long long *tbase = reinterpret_cast<unsigned long long *>(h.data() + o_tbase);
    uint32_t f = 0, g = 0, fm = 0, bm = flat_members;
    uint64_t tiles = 0;
    unsigned long long pairs = 0, big_pairs = 0;
    for (uint32_t c = 0; c < n_clusters; c++) {
        const uint32_t s = members[c];
        if (s < 2) continue;
        if (s <= (uint32_t)LINK_FLAT_MAX) {
            h[o_fslot + f] = c;
            h[o_fmstart + f] = fm;
            fpstart[f] = pairs;
            place[c] = fm;
            fm += s;
            pairs += (unsigned long long)s * (s - 1) / 2;
            f++;
        } else {
            const uint64_t t = ((uint64_t)s + LINK_TILE - 1) / LINK_TILE;
            h[o_bslot + g] = c;
            h[o_bmstart + g] = bm;
            h[o_btstart + g] = (uint32_t)tiles;
            tbase[g] = big_pairs;   // (the flat pair space is added below, once it is known)
            place[c] = bm;
            bm += s;
            tiles += t * (t + 1) / 2;
            big_pairs += (unsigned long long)s * (s - 1) / 2;
            g++;
        }
    }
    h[o_fmstart + nf] = fm;
    fpstart[nf] = pairs;
    h[o_bmstart + nb] = bm;
    h[o_btstart + nb] = (uint32_t)tiles;   // (n <= 2^24: at most 2^16 row blocks, 2^31 + 2^15 tiles)
    tbase[nb] = big_pairs;
    for (uint32_t k = 0; k <= nb; k++) tbase[k] += pairs;
    for (uint32_t i = 0; i < nm; i++) {
        const uint32_t c = member_cluster[i];
        if (members[c] >= 2) h[o_tab + place[c]++] = r0 + i;   // (index order inside every slot)
    }
    T.nf = nf; T.nb = nb; T.n_tiles = (uint32_t)tiles;
    T.o_tab = o_tab; T.o_fslot = o_fslot; T.o_fmstart = o_fmstart; T.o_bslot = o_bslot; T.o_bmstart = o_bmstart; T.o_btstart = o_btstart;
    T.o_fpstart = o_fpstart; T.o_tbase = o_tbase;
    T.flat_pairs = pairs;
    T.total_pairs = pairs + big_pairs;
}

namespace impl {

namespace {

int cluster_linkage(hmk_ctx *ctx, uint32_t r0, uint32_t r1, const uint32_t *member_cluster, uint32_t n_clusters, int X, int p, int thr,
                    int32_t *min_score, uint32_t *min_a, uint32_t *min_b, uint64_t *n_below, int32_t *member_min, uint32_t *member_below,
                    hmk_linkage_stats *stats) {
    if (!ctx) return fail(nullptr, HMK_ERR_BAD_ARG, "null context");
    std::lock_guard<std::mutex> lock(ctx->mu);
    refresh_switches(ctx);
    std::vector<uint32_t> members;
    std::vector<int64_t> size;
    {
        std::vector<int32_t> ids(n_clusters);
        for (uint32_t c = 0; c < n_clusters; c++) ids[c] = (int32_t)c + 1;
        const int st = check_clusters(ctx, "linkage", 0, 0, r0, r1, member_cluster, ids.data(), n_clusters, members, size);
        if (st) return st;
    }
    if (n_clusters && (!min_score || !min_a || !min_b || !n_below)) return fail(ctx, HMK_ERR_BAD_ARG, "null output (min_score, min_a, min_b, n_below)");
    if ((member_min == nullptr) != (member_below == nullptr))
        return fail(ctx, HMK_ERR_BAD_ARG, "member_min and member_below are given together or not at all");
    if (!ctx->symmetric)
        return fail(ctx, HMK_ERR_BAD_ARG, "the linkage of a cluster needs a symmetric scoring matrix: the score of an unordered pair must not "
                                          "depend on which member comes first (ClinkageClusterScorer.java:30-49 scores each pair once)");
    int st = need_device(ctx);
    if (st) return st;
    const uint32_t nm = r1 - r0;
    hmk_linkage_stats S{};
    for (uint32_t c = 0; c < n_clusters; c++) {
        min_score[c] = INT32_MAX;
        min_a[c] = min_b[c] = 0xFFFFFFFFu;
        n_below[c] = 0;
        if (members[c] >= 2) {
            S.n_multi++;
            S.pairs_scored += (uint64_t)members[c] * (members[c] - 1) / 2;
        }
    }
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
    const std::vector<uint32_t> &h = T.h;
    const size_t words = h.size(), o_tab = T.o_tab, o_fslot = T.o_fslot, o_fmstart = T.o_fmstart, o_bslot = T.o_bslot, o_bmstart = T.o_bmstart,
                 o_btstart = T.o_btstart, o_fpstart = T.o_fpstart;
    const uint32_t nf = T.nf, nb = T.nb, n_tiles = T.n_tiles;
    const unsigned long long flat_pairs = T.flat_pairs;

    st = ensure_res32(ctx);
    if (st) return st;
    st = greedy_streams(ctx);
    if (st) return st;
    // the accumulators: key uint64[ncl] | below uint64[ncl] | member_min int32[nm] | member_below uint32[nm]
    const size_t out_bytes = (size_t)n_clusters * 16 + (member_min ? (size_t)nm * 8 : 0);
    HIPCHK(ctx, ensure_buf(ctx, SB_LINK_TAB, words * 4));
    HIPCHK(ctx, ensure_buf(ctx, SB_LINK_OUT, out_bytes));
    HIPCHK(ctx, ctx->h_merge.ensure(out_bytes + 64, 0));
    uint32_t *d_tab = buf<uint32_t>(ctx, SB_LINK_TAB);
    uint64_t *d_key = buf<uint64_t>(ctx, SB_LINK_OUT);
    unsigned long long *d_below = reinterpret_cast<unsigned long long *>(d_key + n_clusters);
    int32_t *d_mmin = member_min ? reinterpret_cast<int32_t *>(d_below + n_clusters) : nullptr;
    uint32_t *d_mbelow = member_min ? reinterpret_cast<uint32_t *>(d_mmin + nm) : nullptr;
    const uint8_t *res32 = ctx->d_res32.as<uint8_t>(), *len = ctx->d_len.as<uint8_t>();
    const int32_t *d_M = ctx->d_M.as<int32_t>();
    hipStream_t Q = ctx->gstream;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    HIPCHK(ctx, hipEventCreate(&e0));
    hipError_t e = hipEventCreate(&e1);
    if (e == hipSuccess) e = hipMemcpyAsync(d_tab, h.data(), words * 4, hipMemcpyHostToDevice, Q);
    if (e == hipSuccess) e = hipEventRecord(e0, Q);
    if (e == hipSuccess) e = launch_linkage_init(d_key, d_below, n_clusters, d_mmin, d_mbelow, nm, Q);
    if (e == hipSuccess)
        e = launch_linkage_flat(res32, len, d_M, d_tab + o_tab, d_tab + o_fslot, d_tab + o_fmstart,
                                reinterpret_cast<const unsigned long long *>(d_tab + o_fpstart), nf, flat_pairs, r0, X, p, thr, d_key, d_below, d_mmin,
                                d_mbelow, Q);
    if (e == hipSuccess) {
        e = launch_linkage_tiled(res32, len, d_M, d_tab + o_tab, d_tab + o_bslot, d_tab + o_bmstart, d_tab + o_btstart, nb, n_tiles, r0, X, p, thr,
                                 d_key, d_below, d_mmin, d_mbelow, Q);
        S.launches = 1 + (flat_pairs ? 1 : 0) + (n_tiles ? 1 : 0);
    }
    if (e == hipSuccess) e = hipEventRecord(e1, Q);
    if (e == hipSuccess) e = hipMemcpyAsync(ctx->h_merge.p, d_key, out_bytes, hipMemcpyDeviceToHost, Q);
    if (e == hipSuccess) e = hipStreamSynchronize(Q);
    float ms = 0;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (e != hipSuccess) return fail(ctx, e == hipErrorOutOfMemory ? HMK_ERR_OOM : HMK_ERR_DEVICE, std::string("cluster linkage: ") + hipGetErrorString(e));
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

// the parameter checks of a scored call over the members [r0, r1): check_shifted, and scores and indices fit a slot's key
int check_link_scores(hmk_ctx *ctx, int X, int p, int thr, uint32_t r0, uint32_t r1) {
    const int st = check_shifted(ctx, X, p, thr, r0, r1, r0, r1);
    if (st) return st;
    // the slot keys carry score + 32768 in 16 bits and the indices in 24 each (as a packed edge does)
    const long long bottom = (long long)ctx->max_len * std::min(0, ctx->min_m) +
                             (long long)std::min(0, p) * ((ctx->max_len - ctx->min_len) + 2LL * X);
    if (bottom < -32768)
        return fail(ctx, HMK_ERR_BAD_ARG, "scores down to " + std::to_string(bottom) + " are possible with this matrix / shift penalty: "
                                          "they do not fit the int16 score of a slot's key");
    if (ctx->n > (1u << 24)) return fail(ctx, HMK_ERR_BAD_ARG, "more than 2^24 sequences: a slot's key holds 24-bit indices");
    return HMK_OK;
}

} }  // namespace hmk::impl

extern "C" {

int hmk_cluster_linkage_shifted(hmk_ctx *ctx, uint32_t r0, uint32_t r1, const uint32_t *member_cluster, uint32_t n_clusters, int max_shift,
                                int shift_penalty, int threshold, int32_t *min_score, uint32_t *min_a, uint32_t *min_b, uint64_t *n_below,
                                int32_t *member_min, uint32_t *member_below, hmk_linkage_stats *stats) {
    return cluster_linkage(ctx, r0, r1, member_cluster, n_clusters, max_shift, shift_penalty, threshold, min_score, min_a, min_b, n_below, member_min,
                           member_below, stats);
}

}  // extern "C"
