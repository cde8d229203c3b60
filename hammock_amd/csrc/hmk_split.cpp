// hmk_split.cpp -- splitting given clusters by complete linkage: per slot ClinkageSequenceClusterer.cluster
// (ClinkageSequenceClusterer.java:43-124) on that slot's members alone, in index order.  The reverse of hmk_merge.cpp: that call runs
// the chain BETWEEN given clusters and never looks inside one, this one runs it INSIDE each given cluster and never looks between two.
//   tables   hmk_slots.cpp's (build_link_tables): the block-diagonal pair space, sum of s (s - 1) / 2 over the slots;
//   kernels  k_split.hip on the clustering stream: every score inside a slot as int16, a dense strict lower triangle per slot;
//   copy     the triangles to a pinned block in one piece;
//   chains   per slot its seeds -- one cluster per member, ids 1 ... s, the candidate lists read off the triangle row by row, which
//            leaves them sorted by place -- and the nearest-neighbour chain (hmk_clinkage.cpp), slots largest first on up to 8 threads.
// hmk_clinkage_split_from_edges builds the slots' candidate lists from a sequence-level edge list instead and shares everything
// behind them: the second implementation the device path is tested against, and what a host-only context runs.
#include "hmk_ctx.h"
#include "hmk_split.h"

#include <atomic>

namespace hmk { namespace impl {

namespace {

constexpr uint64_t SPLIT_MAX_PAIRS = 1ull << 30;   // int16 scores of one call: 2 GiB

struct SplitOut {
    uint32_t *split_cluster, *n_parts;
    int32_t *part_id, *member_rank, *part_order;
    uint32_t *part_start;
};

// fills the candidate lists of slot c (s >= 2 members, numbered by their place in the slot; each list sorted by place) -> its edges
using FillLists = std::function<uint64_t(uint32_t c, uint32_t s, std::vector<std::vector<ClinkCand>> &cand)>;

// The chains of all slots and every output.  Slots are independent: each writes its own members' entries and its own n_parts, so
// the result does not depend on how many threads take them; a failing slot does not stop the others, and the lowest one is reported.
int run_slots(hmk_ctx *ctx, uint32_t r0, uint32_t nm, const uint32_t *member_cluster, uint32_t n_clusters, const std::vector<uint32_t> &members,
              const SlotMembers &M, const FillLists &fill, const SplitOut &out, hmk_split_stats *S) {
    const auto t0 = std::chrono::steady_clock::now();
    const int hashset = ctx->java_hashset;
    const int32_t *sizes = ctx->has_sizes ? ctx->sizes.data() + r0 : nullptr;
    std::vector<uint32_t> jobs;
    for (uint32_t c = 0; c < n_clusters; c++) {
        if (members[c] >= 2) { jobs.push_back(c); continue; }
        out.n_parts[c] = members[c];
        if (members[c] == 0) continue;
        const uint32_t i = M.list[M.start[c]];   // a slot of one: the cluster of id 1, returned as it is
        out.split_cluster[i] = 0;
        if (out.part_id) out.part_id[i] = 1;
        if (out.member_rank) out.member_rank[i] = 0;
        if (out.part_order) out.part_order[M.start[c]] = 1;
    }
    std::stable_sort(jobs.begin(), jobs.end(), [&](uint32_t a, uint32_t b) { return members[a] > members[b]; });   // largest first
    struct Tally { uint64_t edges = 0, merges = 0; uint32_t bad_slot = 0xFFFFFFFFu; int bad_status = 0; std::string bad_text; };
    const unsigned T = (unsigned)std::max<size_t>(1, std::min<size_t>({8, usable_cpus(), jobs.size()}));
    std::vector<Tally> tally(T);
    std::atomic<size_t> next{0};
    auto work = [&](unsigned t) {
        Tally &tl = tally[t];
        std::vector<int32_t> cid, order, rank, pos;
        for (size_t k = next.fetch_add(1); k < jobs.size(); k = next.fetch_add(1)) {
            const uint32_t c = jobs[k], s = members[c];
            const uint32_t *mine = M.list.data() + M.start[c];
            ClinkSeeds seeds;   // :50-55 on the slot's members: one cluster per member, ids from 1 in list order
            seeds.n_clusters = seeds.n_members = s;
            seeds.id.resize(s);
            seeds.size.resize(s);
            seeds.mhead.resize(s);
            seeds.mtail.resize(s);
            seeds.mnext.assign(s, -1);
            seeds.cand.assign(s, std::vector<ClinkCand>());
            for (uint32_t m = 0; m < s; m++) {
                seeds.id[m] = (int32_t)m + 1;
                seeds.size[m] = sizes ? sizes[mine[m]] : 1;
                seeds.mhead[m] = seeds.mtail[m] = (int32_t)m;
            }
            tl.edges += fill(c, s, seeds.cand);
            cid.assign(s, 0);
            order.assign(s, 0);
            rank.assign(s, 0);
            hmk_clinkage_stats cs{};
            std::string err;
            const int st = clinkage_from_seeds(hashset, seeds, cid.data(), order.data(), rank.data(), &cs, &err);
            if (st) {
                if (c < tl.bad_slot) { tl.bad_slot = c; tl.bad_status = st; tl.bad_text = err; }
                out.n_parts[c] = 0;
                continue;
            }
            tl.merges += (uint64_t)cs.merges;
            const uint32_t parts = (uint32_t)cs.n_result_clusters;
            out.n_parts[c] = parts;
            pos.assign(2 * (size_t)s + 2, 0);   // ids reach s + 1 + (s - 1)
            for (uint32_t q = 0; q < parts; q++) pos[order[q]] = (int32_t)q;
            for (uint32_t m = 0; m < s; m++) {
                out.split_cluster[mine[m]] = (uint32_t)pos[cid[m]];   // the part's place in the slot's list; the slot's base comes afterwards
                if (out.part_id) out.part_id[mine[m]] = cid[m];
                if (out.member_rank) out.member_rank[mine[m]] = rank[m];
            }
            if (out.part_order) std::copy(order.begin(), order.begin() + parts, out.part_order + M.start[c]);
        }
    };
    {
        std::vector<std::thread> pool;
        for (unsigned t = 1; t < T; t++) pool.emplace_back(work, t);
        work(0);
        for (std::thread &th : pool) th.join();
    }
    const Tally *bad = nullptr;
    for (const Tally &tl : tally) {
        S->n_edges += tl.edges;
        S->merges += (uint32_t)tl.merges;
        if (tl.bad_status && (!bad || tl.bad_slot < bad->bad_slot)) bad = &tl;
    }
    S->chain_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (bad) {
        S->crash_slot = (int32_t)bad->bad_slot;
        return fail(ctx, bad->bad_status, "slot " + std::to_string(bad->bad_slot) + ": " + bad->bad_text);
    }
    // all parts numbered densely: slots in slot order, inside a slot its parts in list order
    std::vector<uint32_t> base((size_t)n_clusters + 1, 0);
    for (uint32_t c = 0; c < n_clusters; c++) {
        base[c + 1] = base[c] + out.n_parts[c];
        if (out.n_parts[c] > 1) S->n_split++;
    }
    for (uint32_t i = 0; i < nm; i++) out.split_cluster[i] += base[member_cluster[i]];
    S->n_result_clusters = base[n_clusters];
    if (out.part_start) std::copy(M.start.begin(), M.start.end(), out.part_start);
    return HMK_OK;
}

// the checks both entry points make before the device is looked at; members[c] as check_slots'
int check_split(hmk_ctx *ctx, uint32_t r0, uint32_t r1, const uint32_t *member_cluster, uint32_t n_clusters, const SplitOut &out,
                std::vector<uint32_t> &members, hmk_split_stats *S) {
    const int st = check_slots(ctx, "split", r0, r1, member_cluster, n_clusters, members);
    if (st) return st;
    if (r1 > r0 && (!out.split_cluster || !out.n_parts)) return fail(ctx, HMK_ERR_BAD_ARG, "null output (split_cluster, n_parts)");
    if ((out.part_order == nullptr) != (out.part_start == nullptr))
        return fail(ctx, HMK_ERR_BAD_ARG, "part_order and part_start are given together or not at all");
    if (!ctx->symmetric)
        return fail(ctx, HMK_ERR_BAD_ARG, "clinkage needs a symmetric scoring matrix: the reference caches cluster scores by unordered "
                                          "pair (CachedClusterScorer.java:43-53), so its result depends on the evaluation order otherwise");
    const SlotCounts counts = count_slots(members);
    S->n_multi = counts.n_multi;
    S->pairs_scored = counts.pairs;
    if (S->pairs_scored > SPLIT_MAX_PAIRS)
        return fail(ctx, HMK_ERR_BAD_ARG, std::to_string(S->pairs_scored) + " pairs inside the slots of this call, more than 2^30: pass fewer slots "
                                          "per call (slots are split independently of each other)");
    return HMK_OK;
}

int split(hmk_ctx *ctx, uint32_t r0, uint32_t r1, const uint32_t *member_cluster, uint32_t n_clusters, int X, int p, int thr, const SplitOut &out,
          hmk_split_stats *stats) {
    if (!ctx) return fail(nullptr, HMK_ERR_BAD_ARG, "null context");
    std::lock_guard<std::mutex> lock(ctx->mu);
    refresh_switches(ctx);
    hmk_split_stats S{};
    S.crash_slot = -1;
    std::vector<uint32_t> members;
    int st = check_split(ctx, r0, r1, member_cluster, n_clusters, out, members, &S);
    if (st) return st;
    const uint32_t nm = r1 - r0;
    if (nm) {   // scores travel as int16: both bounds (check_shifted: the highest; the lowest as the linkage call's)
        st = check_link_scores(ctx, X, p, thr, r0, r1);
        if (st) return st;
    }
    st = need_device(ctx);
    if (st) return st;
    if (nm == 0) {
        if (stats) *stats = S;
        return HMK_OK;
    }
    const SlotMembers M(nm, member_cluster, n_clusters, members);
    std::vector<uint64_t> tri_of(n_clusters, 0);   // where slot c's triangle begins in the score array
    const int16_t *scores = nullptr;
    if (S.n_multi) {
        LinkTables T;
        build_link_tables(r0, nm, member_cluster, n_clusters, members, T);
        for (uint32_t f = 0; f < T.nf; f++) tri_of[T.h[T.o_fslot + f]] = T.fpstart()[f];
        for (uint32_t g = 0; g < T.nb; g++) tri_of[T.h[T.o_bslot + g]] = T.tbase()[g];
        st = ensure_res32(ctx);
        if (st) return st;
        st = greedy_streams(ctx);
        if (st) return st;
        const size_t score_bytes = (size_t)T.total_pairs * sizeof(int16_t);
        LinkView V;
        st = reserve_link_tables(ctx, T, &V);
        if (st) return st;
        HIPCHK(ctx, ensure_buf(ctx, SB_SPLIT_SCORES, score_bytes));
        HIPCHK(ctx, ctx->h_split.ensure(score_bytes + 64, 0));
        int16_t *d_scores = buf<int16_t>(ctx, SB_SPLIT_SCORES);
        const uint8_t *res32 = ctx->d_res32.as<uint8_t>(), *len = ctx->d_len.as<uint8_t>();
        const int32_t *d_M = ctx->d_M.as<int32_t>();
        hipStream_t Q = ctx->gstream;
        EventPair kernels, copy;   // (the copy's stretch begins where the kernels' ends)
        HIPCHK(ctx, kernels.create());
        HIPCHK(ctx, copy.create());
        hipError_t e = upload_link_tables(ctx, T, Q);
        if (e == hipSuccess) e = kernels.start(Q);
        if (e == hipSuccess) e = launch_split_flat(res32, len, d_M, V, X, p, d_scores, Q);
        if (e == hipSuccess) e = launch_split_tiled(res32, len, d_M, V, X, p, d_scores, Q);
        if (e == hipSuccess) e = kernels.stop(Q);
        if (e == hipSuccess) e = copy.start(Q);
        if (e == hipSuccess) e = hipMemcpyAsync(ctx->h_split.p, d_scores, score_bytes, hipMemcpyDeviceToHost, Q);
        if (e == hipSuccess) e = copy.stop(Q);
        if (e == hipSuccess) e = hipStreamSynchronize(Q);
        float ms = 0, copy_ms = 0;
        if (e == hipSuccess) e = kernels.elapsed(&ms);
        if (e == hipSuccess) e = copy.elapsed(&copy_ms);
        if (e != hipSuccess) return fail_hip(ctx, "clinkage split", e);
        S.kernel_ms = ms;
        S.copy_ms = copy_ms;
        scores = (const int16_t *)ctx->h_split.p;
    }
    // row by row, i ascending: entry (i, j) goes to the end of list i and of list j, which leaves every list sorted by place
    const FillLists fill = [&](uint32_t c, uint32_t s, std::vector<std::vector<ClinkCand>> &cand) -> uint64_t {
        const int16_t *tri = scores + tri_of[c];
        std::vector<uint32_t> deg(s, 0);
        size_t q = 0;
        uint64_t edges = 0;
        for (uint32_t i = 1; i < s; i++)
            for (uint32_t j = 0; j < i; j++, q++)
                if (tri[q] >= thr) { deg[i]++; deg[j]++; edges++; }
        for (uint32_t m = 0; m < s; m++) cand[m].reserve(deg[m]);
        q = 0;
        for (uint32_t i = 1; i < s; i++)
            for (uint32_t j = 0; j < i; j++, q++)
                if (tri[q] >= thr) {
                    cand[i].push_back(ClinkCand{(int32_t)j, tri[q]});
                    cand[j].push_back(ClinkCand{(int32_t)i, tri[q]});
                }
        return edges;
    };
    st = run_slots(ctx, r0, nm, member_cluster, n_clusters, members, M, fill, out, &S);
    if (stats) *stats = S;
    return st;
}

int split_from_edges(hmk_ctx *ctx, const uint64_t *edges, uint64_t n_edges, uint32_t r0, uint32_t r1, const uint32_t *member_cluster,
                     uint32_t n_clusters, const SplitOut &out, hmk_split_stats *stats) {
    if (!ctx) return fail(nullptr, HMK_ERR_BAD_ARG, "null context");
    std::lock_guard<std::mutex> lock(ctx->mu);
    refresh_switches(ctx);
    hmk_split_stats S{};
    S.crash_slot = -1;
    std::vector<uint32_t> members;
    const int st0 = check_split(ctx, r0, r1, member_cluster, n_clusters, out, members, &S);
    if (st0) return st0;
    if (n_edges && !edges) return fail(ctx, HMK_ERR_BAD_ARG, "null edge list");
    S.pairs_scored = 0;   // (nothing is scored here)
    const uint32_t nm = r1 - r0;
    if (nm == 0) {
        if (stats) *stats = S;
        return HMK_OK;
    }
    const SlotMembers M(nm, member_cluster, n_clusters, members);
    std::vector<uint32_t> place(nm);   // the member's place inside its slot
    for (uint32_t c = 0; c < n_clusters; c++)
        for (uint32_t k = M.start[c]; k < M.start[c + 1]; k++) place[M.list[k]] = k - M.start[c];
    // the edges inside a slot, by slot: place of x << 40 | place of m << 16 | score
    std::vector<uint64_t> first((size_t)n_clusters + 1, 0);
    auto inside = [&](uint64_t e) {
        const uint32_t x = HMK_EDGE_X(e), m = HMK_EDGE_M(e);
        return x - r0 < nm && m - r0 < nm && x != m && member_cluster[x - r0] == member_cluster[m - r0];
    };
    for (uint64_t e = 0; e < n_edges; e++)
        if (inside(edges[e])) first[member_cluster[HMK_EDGE_X(edges[e]) - r0] + 1]++;
    for (uint32_t c = 0; c < n_clusters; c++) first[c + 1] += first[c];
    std::vector<uint64_t> rec(first[n_clusters]);
    {
        std::vector<uint64_t> at(first.begin(), first.end() - 1);
        for (uint64_t e = 0; e < n_edges; e++) {
            if (!inside(edges[e])) continue;
            const uint32_t x = HMK_EDGE_X(edges[e]) - r0, m = HMK_EDGE_M(edges[e]) - r0;
            rec[at[member_cluster[x]]++] = (uint64_t)place[x] << 40 | (uint64_t)place[m] << 16 | (edges[e] & 0xFFFFull);
        }
    }
    const FillLists fill = [&](uint32_t c, uint32_t, std::vector<std::vector<ClinkCand>> &cand) -> uint64_t {
        for (uint64_t q = first[c]; q < first[c + 1]; q++) {
            const int32_t a = (int32_t)HMK_EDGE_X(rec[q]), b = (int32_t)HMK_EDGE_M(rec[q]), sc = HMK_EDGE_SCORE(rec[q]);
            cand[a].push_back(ClinkCand{b, sc});
            cand[b].push_back(ClinkCand{a, sc});
        }
        for (std::vector<ClinkCand> &l : cand)
            std::sort(l.begin(), l.end(), [](const ClinkCand &u, const ClinkCand &v) { return u.ix < v.ix; });
        return first[c + 1] - first[c];
    };
    const int st = run_slots(ctx, r0, nm, member_cluster, n_clusters, members, M, fill, out, &S);
    if (stats) *stats = S;
    return st;
}

}  // namespace

} }  // namespace hmk::impl

extern "C" {

int hmk_clinkage_split(hmk_ctx *ctx, uint32_t r0, uint32_t r1, const uint32_t *member_cluster, uint32_t n_clusters, int max_shift, int shift_penalty,
                       int threshold, uint32_t *split_cluster, uint32_t *n_parts, int32_t *part_id, int32_t *member_rank, int32_t *part_order,
                       uint32_t *part_start, hmk_split_stats *stats) {
    return split(ctx, r0, r1, member_cluster, n_clusters, max_shift, shift_penalty, threshold,
                 SplitOut{split_cluster, n_parts, part_id, member_rank, part_order, part_start}, stats);
}

int hmk_clinkage_split_from_edges(hmk_ctx *ctx, const uint64_t *edges, uint64_t n_edges, uint32_t r0, uint32_t r1, const uint32_t *member_cluster,
                                  uint32_t n_clusters, uint32_t *split_cluster, uint32_t *n_parts, int32_t *part_id, int32_t *member_rank,
                                  int32_t *part_order, uint32_t *part_start, hmk_split_stats *stats) {
    return split_from_edges(ctx, edges, n_edges, r0, r1, member_cluster, n_clusters,
                            SplitOut{split_cluster, n_parts, part_id, member_rank, part_order, part_start}, stats);
}

}  // extern "C"
