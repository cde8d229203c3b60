// hmk_merge.cpp -- merging given clusters by complete linkage: ClinkageSequenceClusterer.cluster (ClinkageSequenceClusterer.java:43-124)
// with its seeding (:50-55) replaced by "activeClusters = the given clusters, in slot order".  The clusters are the members [r0, r1) of
// the hmk_set_sequences set in slots, as hmk_assign_shifted takes them.
//   pass    the triangle inside [r0, r1) (build_plan_triangle, in the merge's own plan slot) into the context's edge buffer;
//   CSR     of the range (piece_enqueue_csr), on the clustering stream;
//   graph   per cluster its feasible clusters and their complete-linkage scores (ClinkageClusterScorer.java:30-49), on the device
//           (k_merge.hip); the lists are stored into a pinned block by the device and sorted per cluster on the host (a list is short,
//           and the chain's seeding walks it anyway);
//   chain   the nearest-neighbour chain from seeds (hmk_clinkage.cpp) on the host.
// Only the cluster-level lists cross to the host.  hmk_clinkage_merge_from_edges builds the same lists on the host from a
// sequence-level edge list: the second implementation the device graph is tested against, and what a host-only context runs.
#include "hmk_ctx.h"
#include "hmk_slots.h"

#include <unordered_map>

namespace hmk { namespace impl {

namespace {

constexpr int32_t MAX_CLUSTER_ID = 1 << 30;

// the checks both entry points make before the device is looked at; members[c] / size[c] as check_clusters'.  cluster_id may be
// null (hmk_cluster_pairs_shifted has no ids, and reads no size)
int check_merge(hmk_ctx *ctx, uint32_t r0, uint32_t r1, const uint32_t *member_cluster, const int32_t *cluster_id, uint32_t n_clusters,
                std::vector<uint32_t> &members, std::vector<int64_t> &size) {
    int st = cluster_id ? check_clusters(ctx, "merge", 0, 0, r0, r1, member_cluster, cluster_id, n_clusters, members, size)
                        : check_slots(ctx, "merge", r0, r1, member_cluster, n_clusters, members);
    if (st) return st;
    if (cluster_id)
        for (uint32_t c = 0; c < n_clusters; c++)
            if (cluster_id[c] < 1 || cluster_id[c] > MAX_CLUSTER_ID)
                return fail(ctx, HMK_ERR_BAD_ARG, "cluster_id[" + std::to_string(c) + "] = " + std::to_string(cluster_id[c]) + " is outside [1, 2^30]");
    if (!ctx->symmetric)
        return fail(ctx, HMK_ERR_BAD_ARG, "clinkage needs a symmetric scoring matrix: the reference caches cluster scores by unordered "
                                          "pair (CachedClusterScorer.java:43-53), so its result depends on the evaluation order otherwise");
    uint64_t m1 = 0, m2 = 0;   // the two largest member counts: hits are counted in 32 bits
    for (uint32_t c = 0; c < n_clusters; c++) {
        if (members[c] > m1) { m2 = m1; m1 = members[c]; }
        else if (members[c] > m2) m2 = members[c];
    }
    if (m1 * m2 > 0xFFFFFFFFull)
        return fail(ctx, HMK_ERR_BAD_ARG, "two clusters with " + std::to_string(m1) + " and " + std::to_string(m2) + " members: 2^32 or more member pairs");
    return HMK_OK;
}

// the seeds without their candidate lists: ids, sizes, Cluster.getSequences() = the slot's members in index order
void seed_clusters(ClinkSeeds &S, uint32_t nm, const uint32_t *member_cluster, const int32_t *cluster_id, uint32_t n_clusters,
                   const std::vector<int64_t> &size) {
    S.n_clusters = n_clusters;
    S.n_members = nm;
    S.id.assign(cluster_id, cluster_id + n_clusters);
    S.size = size;
    S.mhead.assign(n_clusters, -1);
    S.mtail.assign(n_clusters, -1);
    S.mnext.assign(nm, -1);
    for (uint32_t i = 0; i < nm; i++) {
        const uint32_t c = member_cluster[i];
        if (S.mhead[c] < 0) S.mhead[c] = (int32_t)i; else S.mnext[S.mtail[c]] = (int32_t)i;
        S.mtail[c] = (int32_t)i;
    }
    S.cand.assign(n_clusters, std::vector<ClinkCand>());
}

// the seeds' candidate lists from the device's records (see merge): piece by piece, each sorted by candidate
int lists_from_records(hmk_ctx *ctx, const uint64_t *pinned, uint64_t n_rec, uint32_t n_clusters, std::vector<std::vector<ClinkCand>> &cand) {
    std::vector<uint64_t> rec(pinned, pinned + n_rec);
    std::vector<uint64_t> first((size_t)n_clusters + 1, 0);   // piece of slot a: rec[first[a] .. first[a + 1])
    for (uint64_t t = 0; t < n_rec; t++) {
        const uint32_t a = HMK_EDGE_X(rec[t]), b = HMK_EDGE_M(rec[t]);
        if (a >= n_clusters || b >= n_clusters || a == b || (t && a < HMK_EDGE_X(rec[t - 1])))
            return fail(ctx, HMK_ERR_DEVICE, "merge graph: a record names a slot that does not exist, or the pieces are out of order");
        first[a + 1]++;
    }
    for (uint32_t a = 0; a < n_clusters; a++) first[a + 1] += first[a];
    const unsigned T = n_rec >= (1u << 16) ? std::max(1u, std::min(8u, usable_cpus())) : 1u;
    auto work = [&](unsigned t) {
        // slots [lo, hi): an equal share of the records
        const uint32_t lo = (uint32_t)(std::lower_bound(first.begin(), first.end(), n_rec * t / T) - first.begin());
        const uint32_t hi = t + 1 == T ? n_clusters : (uint32_t)(std::lower_bound(first.begin(), first.end(), n_rec * (t + 1) / T) - first.begin());
        for (uint32_t a = std::min(lo, n_clusters); a < std::min(hi, n_clusters); a++) {
            std::sort(rec.begin() + first[a], rec.begin() + first[a + 1]);
            std::vector<ClinkCand> &l = cand[a];
            l.resize(first[a + 1] - first[a]);
            for (uint64_t q = first[a]; q < first[a + 1]; q++) l[q - first[a]] = ClinkCand{(int32_t)HMK_EDGE_M(rec[q]), HMK_EDGE_SCORE(rec[q])};
        }
    };
    std::vector<std::thread> pool;
    for (unsigned t = 1; t < T; t++) pool.emplace_back(work, t);
    work(0);
    for (std::thread &th : pool) th.join();
    return HMK_OK;
}

// the chain on the seeds (candidate lists sorted by slot), and the outputs per slot
int run_chain(hmk_ctx *ctx, ClinkSeeds &S, const uint32_t *member_cluster, int32_t *merged_id, int32_t *result_order, int32_t *member_rank,
              hmk_merge_stats *stats) {
    std::vector<int32_t> of_member(std::max<uint32_t>(S.n_members, 1));
    hmk_clinkage_stats cs{};
    std::string err;
    const uint32_t nm = S.n_members;
    const int st = clinkage_from_seeds(ctx->java_hashset, S, of_member.data(), result_order, member_rank, &cs, &err);
    stats->merges = cs.merges;
    stats->searches = cs.searches;
    stats->n_result_clusters = cs.n_result_clusters;
    stats->chain_ms = cs.chain_ms;
    if (st) return fail(ctx, st, err);
    for (uint32_t i = 0; i < nm; i++) merged_id[member_cluster[i]] = of_member[i];
    return HMK_OK;
}

// The device side: pass, CSR and cluster graph of the members [r0, r1) (nm >= 2, n_clusters >= 2).  Leaves *n_rec records
// a << 40 | b << 16 | score in ctx->h_merge -- every ordered pair of feasible clusters, or with upper_only those with a < b.
int device_graph(hmk_ctx *ctx, uint32_t r0, uint32_t r1, const uint32_t *member_cluster, uint32_t n_clusters, const std::vector<uint32_t> &members,
                 int X, int p, int thr, bool upper_only, hmk_merge_stats *S, uint64_t *n_rec) {
    const uint32_t nm = r1 - r0, n = ctx->n;
    *n_rec = 0;
    int st = check_shifted(ctx, X, p, thr, r0, r1, r0, r1);
    if (st) return st;
    st = greedy_streams(ctx);
    if (st) return st;
    st = build_plan_triangle(ctx, ctx->plan_merge, X, p, thr, r0, r1);
    if (st) return st;
    unsigned long long counts[HMK_EDGE_SHARDS];
    double ms = 0;
    st = neighbors_grow(ctx, 0, counts, &ms, [&](uint64_t *d_edges, uint64_t cap, unsigned long long *d_counts) {
        return launch_plan(ctx, ctx->plan_merge, X, p, thr, d_edges, cap, d_counts, nullptr);
    });
    if (st) return st;
    S->n_edges += total_of(counts);
    S->pairs_scored = ctx->plan_merge.stats.pairs_scored;
    S->kernel_ms = ms;
    if (2 * S->n_edges > 0xFFFFFFFFull) return fail(ctx, HMK_ERR_OOM, "more than 2^31 - 1 edges above the threshold: raise the threshold");

    // the clusters, once per call: slot starts | members by slot (absolute indices) | member -> slot
    std::vector<uint32_t> cl((size_t)n_clusters + 1 + 2 * (size_t)nm);
    uint32_t *cl_start = cl.data(), *cl_members = cl_start + n_clusters + 1, *cluster_of = cl_members + nm;
    cl_start[0] = 0;
    for (uint32_t c = 0; c < n_clusters; c++) cl_start[c + 1] = cl_start[c] + members[c];
    {
        std::vector<uint32_t> at(cl_start, cl_start + n_clusters);
        for (uint32_t i = 0; i < nm; i++) cl_members[at[member_cluster[i]]++] = r0 + i;
    }
    std::memcpy(cluster_of, member_cluster, (size_t)nm * 4);
    const uint64_t room = std::max<uint64_t>(2 * S->n_edges, 1);
    HIPCHK(ctx, ensure_buf(ctx, SB_MERGE_CL, cl.size() * 4));
    HIPCHK(ctx, ensure_buf(ctx, SB_MERGE_LEN, ((size_t)nm + 1) * 4));
    HIPCHK(ctx, ensure_buf(ctx, SB_MERGE_MSTART, ((size_t)nm + 1) * 4));
    HIPCHK(ctx, ensure_buf(ctx, SB_MERGE_TMP, room * sizeof(uint64_t)));
    HIPCHK(ctx, ensure_buf(ctx, SB_MERGE_CNT, (size_t)n_clusters * 4));
    HIPCHK(ctx, ensure_buf(ctx, SB_MERGE_OSTART, ((size_t)n_clusters + 1) * 4));
    HIPCHK(ctx, ensure_buf(ctx, SB_MERGE_SCR, ((size_t)n_clusters + 2) * 4));
    HIPCHK(ctx, ensure_buf(ctx, SB_MERGE_SCAN, scan_scratch_bytes(std::max(nm, n_clusters) + 1)));
    uint32_t *d_cl = buf<uint32_t>(ctx, SB_MERGE_CL);
    hipStream_t Q = ctx->gstream;
    HIPCHK(ctx, hipMemcpyAsync(d_cl, cl.data(), cl.size() * 4, hipMemcpyHostToDevice, Q));

    const bool packed = adjacency_packed(ctx, X, p, thr);   // (4-byte entries m << 8 | score - threshold, as hmk_greedy_cluster)
    const EdgeSegs segs = ctx->edges.segs();
    EventPair ev;
    HIPCHK(ctx, ev.create());
    hipError_t e = ev.start(Q);
    if (e == hipSuccess) e = piece_enqueue_csr(ctx, segs, true, packed, thr, n, r0, r1, false, false, Q);
    if (e == hipSuccess)
        e = launch_merge_graph(packed, buf<uint64_t>(ctx, SB_START), buf<void>(ctx, SB_ADJ), thr, r0, nm, n_clusters, d_cl, d_cl + n_clusters + 1,
                               d_cl + n_clusters + 1 + nm, upper_only, 2 * S->n_edges, buf<uint32_t>(ctx, SB_MERGE_LEN),
                               buf<uint32_t>(ctx, SB_MERGE_MSTART), buf<uint64_t>(ctx, SB_MERGE_TMP), buf<uint32_t>(ctx, SB_MERGE_CNT),
                               buf<uint32_t>(ctx, SB_MERGE_OSTART), buf<uint32_t>(ctx, SB_MERGE_SCR), buf<uint64_t>(ctx, SB_MERGE_SCAN), Q);
    uint32_t *h_total = (uint32_t *)(ctx->h_counts + HC_MISC) + 2;   // (the number of records)
    if (e == hipSuccess) e = hipMemcpyAsync(h_total, buf<uint32_t>(ctx, SB_MERGE_OSTART) + n_clusters, 4, hipMemcpyDeviceToHost, Q);
    if (e == hipSuccess) e = hipStreamSynchronize(Q);
    uint64_t total = 0;
    bool bad_edge = false;
    if (e == hipSuccess) {
        bad_edge = ((const int *)(ctx->h_counts + HC_RANGE))[2] != 0 || ctx->h_counts[HC_TOTAL] != 2 * S->n_edges;
        total = *h_total;
    }
    if (e == hipSuccess && !bad_edge && total) {
        // the lists to the host: stored by the device into the pinned block
        e = ctx->h_merge.ensure(total * sizeof(uint64_t) + 64, 0);
        uint64_t *d_out = nullptr;
        if (e == hipSuccess) e = hipHostGetDevicePointer((void **)&d_out, ctx->h_merge.p, 0);
        if (e == hipSuccess)
            e = launch_merge_compact(n_clusters, d_cl, buf<uint32_t>(ctx, SB_MERGE_MSTART), buf<uint64_t>(ctx, SB_MERGE_TMP), buf<uint32_t>(ctx, SB_MERGE_CNT),
                                     buf<uint32_t>(ctx, SB_MERGE_OSTART), thr, d_out, total, Q);
    }
    if (e == hipSuccess) e = ev.stop(Q);
    if (e == hipSuccess) e = hipEventSynchronize(ev.b);
    float gms = 0;
    if (e == hipSuccess) e = ev.elapsed(&gms);
    if (e != hipSuccess) return fail_hip(ctx, "merge graph", e);
    if (bad_edge) return fail(ctx, HMK_ERR_DEVICE, "merge CSR: an edge names a sequence outside the range, or the rows do not add up to the edges");
    S->graph_ms = gms;
    *n_rec = total;
    return HMK_OK;
}

int cluster_pairs(hmk_ctx *ctx, uint32_t r0, uint32_t r1, const uint32_t *member_cluster, uint32_t n_clusters, int X, int p, int thr, uint64_t *pairs,
                  uint64_t capacity, uint64_t *n_pairs, hmk_merge_stats *stats) {
    if (!ctx) return fail(nullptr, HMK_ERR_BAD_ARG, "null context");
    std::lock_guard<std::mutex> lock(ctx->mu);
    refresh_switches(ctx);
    std::vector<uint32_t> members;
    std::vector<int64_t> size;
    int st = check_merge(ctx, r0, r1, member_cluster, nullptr, n_clusters, members, size);
    if (st) return st;
    if (!n_pairs) return fail(ctx, HMK_ERR_BAD_ARG, "null n_pairs");
    st = need_device(ctx);
    if (st) return st;
    hmk_merge_stats S{};
    *n_pairs = 0;
    uint64_t n_rec = 0;
    if (n_clusters >= 2) {
        st = device_graph(ctx, r0, r1, member_cluster, n_clusters, members, X, p, thr, true, &S, &n_rec);
        if (st) return st;
    }
    S.cluster_pairs = n_rec;
    *n_pairs = n_rec;
    if (stats) *stats = S;
    if (n_rec > capacity) return fail(ctx, HMK_ERR_CAPACITY, "pair buffer too small: " + std::to_string(n_rec) + " cluster pairs");
    if (n_rec && !pairs) return fail(ctx, HMK_ERR_BAD_ARG, "null pair buffer");
    if (n_rec) std::memcpy(pairs, ctx->h_merge.p, n_rec * sizeof(uint64_t));
    return HMK_OK;
}

int merge_common_checks(hmk_ctx *ctx, uint32_t r0, uint32_t r1, const uint32_t *member_cluster, const int32_t *cluster_id, uint32_t n_clusters,
                        int32_t *merged_id, std::vector<uint32_t> &members, std::vector<int64_t> &size) {
    if (n_clusters && !cluster_id) return fail(ctx, HMK_ERR_BAD_ARG, "null cluster_id");
    int st = check_merge(ctx, r0, r1, member_cluster, cluster_id, n_clusters, members, size);
    if (st) return st;
    if (n_clusters == 0)
        return fail(ctx, HMK_ERR_REFERENCE_WOULD_CRASH,
                    "the reference throws NoSuchElementException here (ClinkageSequenceClusterer.java:118): no clusters");
    if (!merged_id) return fail(ctx, HMK_ERR_BAD_ARG, "null merged_id");
    return HMK_OK;
}

int merge(hmk_ctx *ctx, uint32_t r0, uint32_t r1, const uint32_t *member_cluster, const int32_t *cluster_id, uint32_t n_clusters, int X, int p, int thr,
          int32_t *merged_id, int32_t *result_order, int32_t *member_rank, hmk_merge_stats *stats) {
    if (!ctx) return fail(nullptr, HMK_ERR_BAD_ARG, "null context");
    std::lock_guard<std::mutex> lock(ctx->mu);
    refresh_switches(ctx);
    std::vector<uint32_t> members;
    std::vector<int64_t> size;
    int st = merge_common_checks(ctx, r0, r1, member_cluster, cluster_id, n_clusters, merged_id, members, size);
    if (st) return st;
    hmk_merge_stats local;
    if (!stats) stats = &local;
    *stats = hmk_merge_stats{};
    st = need_device(ctx);
    if (st) return st;
    const uint32_t nm = r1 - r0;
    uint64_t n_rec = 0;
    if (n_clusters >= 2) {
        st = device_graph(ctx, r0, r1, member_cluster, n_clusters, members, X, p, thr, false, stats, &n_rec);
        if (st) return st;
    }
    ClinkSeeds S;
    seed_clusters(S, nm, member_cluster, cluster_id, n_clusters, size);
    // the device stored slot a's records in one piece at its run start (a << 40 | b << 16 | score), in arbitrary order inside the piece: a
    // sort of the piece's 64-bit words is the sort by candidate, on the host (pieces are short, the words are in cache once copied,
    // and several threads take a share of the slots each)
    st = lists_from_records(ctx, (const uint64_t *)ctx->h_merge.p, n_rec, n_clusters, S.cand);
    if (st) return st;
    stats->cluster_pairs = n_rec / 2;
    return run_chain(ctx, S, member_cluster, merged_id, result_order, member_rank, stats);
}

int merge_from_edges(hmk_ctx *ctx, const uint64_t *edges, uint64_t n_edges, uint32_t r0, uint32_t r1, const uint32_t *member_cluster,
                     const int32_t *cluster_id, uint32_t n_clusters, int32_t *merged_id, int32_t *result_order, int32_t *member_rank,
                     hmk_merge_stats *stats) {
    if (!ctx) return fail(nullptr, HMK_ERR_BAD_ARG, "null context");
    std::lock_guard<std::mutex> lock(ctx->mu);
    refresh_switches(ctx);
    std::vector<uint32_t> members;
    std::vector<int64_t> size;
    int st = merge_common_checks(ctx, r0, r1, member_cluster, cluster_id, n_clusters, merged_id, members, size);
    if (st) return st;
    if (n_edges && !edges) return fail(ctx, HMK_ERR_BAD_ARG, "null edge list");
    hmk_merge_stats local;
    if (!stats) stats = &local;
    *stats = hmk_merge_stats{};
    const uint32_t nm = r1 - r0;
    // the cluster graph on the host: hits and minimum per unordered pair of slots
    struct Agg { uint64_t hits; int32_t mn; };
    std::unordered_map<uint64_t, Agg> agg;
    for (uint64_t e = 0; e < n_edges; e++) {
        const uint32_t x = HMK_EDGE_X(edges[e]), m = HMK_EDGE_M(edges[e]);
        if (x - r0 >= nm || m - r0 >= nm) continue;
        stats->n_edges++;
        uint32_t a = member_cluster[x - r0], b = member_cluster[m - r0];
        if (a == b) continue;
        if (a > b) std::swap(a, b);
        const int32_t sc = HMK_EDGE_SCORE(edges[e]);
        auto it = agg.find((uint64_t)a << 32 | b);
        if (it == agg.end()) agg.emplace((uint64_t)a << 32 | b, Agg{1, sc});
        else { it->second.hits++; it->second.mn = std::min(it->second.mn, sc); }
    }
    ClinkSeeds S;
    seed_clusters(S, nm, member_cluster, cluster_id, n_clusters, size);
    for (const auto &kv : agg) {
        const uint32_t a = (uint32_t)(kv.first >> 32), b = (uint32_t)kv.first;
        if (kv.second.hits != (uint64_t)members[a] * members[b]) continue;
        S.cand[a].push_back(ClinkCand{(int32_t)b, kv.second.mn});
        S.cand[b].push_back(ClinkCand{(int32_t)a, kv.second.mn});
        stats->cluster_pairs++;
    }
    for (std::vector<ClinkCand> &l : S.cand)
        std::sort(l.begin(), l.end(), [](const ClinkCand &a, const ClinkCand &b) { return a.ix < b.ix; });
    return run_chain(ctx, S, member_cluster, merged_id, result_order, member_rank, stats);
}

}  // namespace

} }  // namespace hmk::impl

extern "C" {

int hmk_cluster_pairs_shifted(hmk_ctx *ctx, uint32_t r0, uint32_t r1, const uint32_t *member_cluster, uint32_t n_clusters, int max_shift,
                              int shift_penalty, int threshold, uint64_t *pairs, uint64_t capacity, uint64_t *n_pairs, hmk_merge_stats *stats) {
    return cluster_pairs(ctx, r0, r1, member_cluster, n_clusters, max_shift, shift_penalty, threshold, pairs, capacity, n_pairs, stats);
}

int hmk_clinkage_merge(hmk_ctx *ctx, uint32_t r0, uint32_t r1, const uint32_t *member_cluster, const int32_t *cluster_id, uint32_t n_clusters,
                       int max_shift, int shift_penalty, int threshold, int32_t *merged_id, int32_t *result_order, int32_t *member_rank,
                       hmk_merge_stats *stats) {
    return merge(ctx, r0, r1, member_cluster, cluster_id, n_clusters, max_shift, shift_penalty, threshold, merged_id, result_order, member_rank,
                 stats);
}

int hmk_clinkage_merge_from_edges(hmk_ctx *ctx, const uint64_t *edges, uint64_t n_edges, uint32_t r0, uint32_t r1, const uint32_t *member_cluster,
                                  const int32_t *cluster_id, uint32_t n_clusters, int32_t *merged_id, int32_t *result_order, int32_t *member_rank,
                                  hmk_merge_stats *stats) {
    return merge_from_edges(ctx, edges, n_edges, r0, r1, member_cluster, cluster_id, n_clusters, merged_id, result_order, member_rank, stats);
}

}  // extern "C"
