// hmk_slots.cpp -- what the calls over given clusters share on the host (hmk_slots.h).
#include "hmk_ctx.h"
#include "hmk_linkage.h"
#include "hmk_slots.h"

namespace hmk { namespace impl {

int check_slots(hmk_ctx *ctx, const char *what, uint32_t r0, uint32_t r1, const uint32_t *member_cluster, uint32_t n_clusters,
                std::vector<uint32_t> &members) {
    std::vector<int32_t> ids(n_clusters);
    for (uint32_t c = 0; c < n_clusters; c++) ids[c] = (int32_t)c + 1;
    std::vector<int64_t> size;
    return check_clusters(ctx, what, 0, 0, r0, r1, member_cluster, ids.data(), n_clusters, members, size);
}

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

SlotMembers::SlotMembers(uint32_t nm, const uint32_t *member_cluster, uint32_t n_clusters, const std::vector<uint32_t> &members)
    : start((size_t)n_clusters + 1, 0), list(nm) {
    for (uint32_t c = 0; c < n_clusters; c++) start[c + 1] = start[c] + members[c];
    std::vector<uint32_t> at(start.begin(), start.end() - 1);
    for (uint32_t i = 0; i < nm; i++) list[at[member_cluster[i]]++] = i;
}

SlotCounts count_slots(const std::vector<uint32_t> &members) {
    SlotCounts n{0, 0};
    for (const uint32_t s : members)
        if (s >= 2) {
            n.n_multi++;
            n.pairs += (uint64_t)s * (s - 1) / 2;
        }
    return n;
}

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

int reserve_link_tables(hmk_ctx *ctx, const LinkTables &T, LinkView *V) {
    const size_t words = T.h.size();
    HIPCHK(ctx, ensure_buf(ctx, SB_LINK_TAB, words * 4));
    const uint32_t *d_tab = buf<uint32_t>(ctx, SB_LINK_TAB);
    V->tab = d_tab + T.o_tab;
    V->fslot = d_tab + T.o_fslot;
    V->fmstart = d_tab + T.o_fmstart;
    V->bslot = d_tab + T.o_bslot;
    V->bmstart = d_tab + T.o_bmstart;
    V->btstart = d_tab + T.o_btstart;
    V->fpstart = reinterpret_cast<const unsigned long long *>(d_tab + T.o_fpstart);
    V->tbase = reinterpret_cast<const unsigned long long *>(d_tab + T.o_tbase);
    V->nf = T.nf;
    V->nb = T.nb;
    V->n_tiles = T.n_tiles;
    V->nt = T.h[T.o_bmstart + T.nb];
    V->flat_pairs = T.flat_pairs;
    return HMK_OK;
}

hipError_t upload_link_tables(hmk_ctx *ctx, const LinkTables &T, hipStream_t Q) {
    return hipMemcpyAsync(buf<uint32_t>(ctx, SB_LINK_TAB), T.h.data(), T.h.size() * 4, hipMemcpyHostToDevice, Q);
}

} }  // namespace hmk::impl
