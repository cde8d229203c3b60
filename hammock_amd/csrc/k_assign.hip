// k_assign.hip -- the device side of the assignment of new sequences to existing clusters (hmk_assign.cpp).  After the pass
// over members x new sequences: every edge's (cluster, score) record gathered into its new sequence's run (count, scan,
// scatter), then per new sequence the clusters of its run aggregated in an LDS open-addressing table (hits and minimum score
// per cluster, as k_greedy_precheck does), the clusters whose hits equal their member count kept as feasible, and the best k
// of them selected by (complete-linkage score, size, ~id).
// Clusters travel as their RANK in the host's (size descending, id ascending) order, so that one 64-bit key orders them:
// key = (min score + 32768) << 32 | (0xFFFFFFFF - rank), larger = better, never 0.
// Every store here is an ordinary vector store; the counters are vector atomics.
#include "hmk_device.h"
#include "k_assign_table.h"
#include "hmk_grid.h"

namespace hmk {

namespace {

// the new-sequence end (as x - q0) and the member end of a pass edge: the two ranges are disjoint, so whichever end lies in
// [q0, q0 + nq) is the new sequence (a symmetric pass emits (min, max) caller indices, an asymmetric or local one m = member)
__device__ __forceinline__ void edge_ends(uint64_t e, uint32_t q0, uint32_t nq, uint32_t *xq, uint32_t *m) {
    const uint32_t a = (uint32_t)(e >> 40), b = (uint32_t)(e >> 16) & 0xFFFFFFu;
    const bool a_new = a - q0 < nq;
    *xq = (a_new ? a : b) - q0;
    *m = a_new ? b : a;
}

// hits per new sequence (cnt: zeroed uint32[nq])
__global__ void __launch_bounds__(256)
k_assign_count(const uint64_t *__restrict__ edges, uint64_t cap_per_shard, const unsigned long long *__restrict__ counts, uint32_t q0,
               uint32_t nq, uint32_t *__restrict__ cnt) {
    const uint32_t shard = blockIdx.y;
    const uint64_t n = min((uint64_t)counts[shard], cap_per_shard);
    const uint64_t *seg = edges + (uint64_t)shard * cap_per_shard;
    for (uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (uint64_t)gridDim.x * 256) {
        uint32_t xq, m;
        edge_ends(seg[k], q0, nq, &xq, &m);
        if (xq < nq) atomicAdd(&cnt[xq], 1u);   // (always: every edge joins a member and a new sequence)
    }
}

// every hit as a record (member's cluster rank << 32 | score + 32768) into its new sequence's run rec[start[x] .. start[x + 1])
// (cursor: zeroed uint32[nq]; order inside a run arbitrary)
__global__ void __launch_bounds__(256)
k_assign_scatter(const uint64_t *__restrict__ edges, uint64_t cap_per_shard, const unsigned long long *__restrict__ counts, uint32_t q0,
                 uint32_t nq, uint32_t r0, uint32_t nm, const uint32_t *__restrict__ member_rank, const uint32_t *__restrict__ start,
                 uint32_t *__restrict__ cursor, uint64_t *__restrict__ rec, uint64_t rec_capacity) {
    const uint32_t shard = blockIdx.y;
    const uint64_t n = min((uint64_t)counts[shard], cap_per_shard);
    const uint64_t *seg = edges + (uint64_t)shard * cap_per_shard;
    for (uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (uint64_t)gridDim.x * 256) {
        const uint64_t e = seg[k];
        uint32_t xq, m;
        edge_ends(e, q0, nq, &xq, &m);
        if (xq >= nq || m - r0 >= nm) continue;   // (never, as above)
        const uint32_t score = (uint32_t)((int32_t)(int16_t)(e & 0xFFFFu) + 32768);
        const uint64_t pos = (uint64_t)start[xq] + atomicAdd(&cursor[xq], 1u);
        if (pos < rec_capacity) rec[pos] = ((uint64_t)member_rank[m - r0] << 32) | score;
    }
}

// one wave per new sequence whose run holds at most `long_run` records (4 waves per workgroup, grid-stride); the longer runs
// are listed in long_list[0 .. *long_count) for k_assign_block
__global__ void __launch_bounds__(256)
k_assign_wave(const uint32_t *__restrict__ start, const uint64_t *__restrict__ rec, uint32_t nq, uint32_t k, uint32_t long_run,
              const uint32_t *__restrict__ members_of_rank, const uint32_t *__restrict__ slot_of_rank, uint32_t *__restrict__ long_list,
              uint32_t *__restrict__ long_count, uint32_t *__restrict__ best_cluster, int32_t *__restrict__ best_score,
              uint32_t *__restrict__ n_feasible) {
    __shared__ int32_t keys_all[4 * WAVE_SLOTS];
    __shared__ uint32_t hits_all[4 * WAVE_SLOTS];
    __shared__ uint32_t mn_all[4 * WAVE_SLOTS];
    __shared__ uint16_t used_all[4 * WAVE_SLOTS];
    __shared__ uint32_t n_used_all[4];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const RunTable<64, WAVE_SLOTS> T{keys_all + wv * WAVE_SLOTS, hits_all + wv * WAVE_SLOTS, mn_all + wv * WAVE_SLOTS,
                                     used_all + wv * WAVE_SLOTS, n_used_all + wv, nullptr};
    T.init(lane);
    for (uint32_t q = blockIdx.x * 4 + wv; q < nq; q += gridDim.x * 4) {   // (wave-uniform)
        const uint32_t b = start[q], len = start[q + 1] - b;
        if (len > long_run) {
            if (lane == 0) long_list[atomicAdd(long_count, 1u)] = q;
            continue;
        }
        T.run(rec + b, len, members_of_rank, slot_of_rank, k, lane, best_cluster + (uint64_t)q * k, best_score + (uint64_t)q * k, n_feasible + q);
    }
}

// one workgroup per listed long run (grid-stride over the list)
__global__ void __launch_bounds__(256)
k_assign_block(const uint32_t *__restrict__ start, const uint64_t *__restrict__ rec, uint32_t k, const uint32_t *__restrict__ members_of_rank,
               const uint32_t *__restrict__ slot_of_rank, const uint32_t *__restrict__ long_list, const uint32_t *__restrict__ long_count,
               uint32_t *__restrict__ best_cluster, int32_t *__restrict__ best_score, uint32_t *__restrict__ n_feasible) {
    __shared__ int32_t keys[BLOCK_SLOTS];
    __shared__ uint32_t hits[BLOCK_SLOTS];
    __shared__ uint32_t mn[BLOCK_SLOTS];
    __shared__ uint16_t used[BLOCK_SLOTS];
    __shared__ uint32_t n_used;
    __shared__ uint64_t red[4];
    const RunTable<256, BLOCK_SLOTS> T{keys, hits, mn, used, &n_used, red};
    const uint32_t n_long = *long_count;
    if (blockIdx.x >= n_long) return;   // (uniform)
    T.init(threadIdx.x);
    for (uint32_t i = blockIdx.x; i < n_long; i += gridDim.x) {
        const uint32_t q = long_list[i];
        const uint32_t b = start[q], len = start[q + 1] - b;
        T.run(rec + b, len, members_of_rank, slot_of_rank, k, threadIdx.x, best_cluster + (uint64_t)q * k, best_score + (uint64_t)q * k,
              n_feasible + q);
    }
}

// workgroups per segment: from the longest segment's count (the host has the counts), ~2,048 edges each
uint32_t seg_grid_x(uint64_t max_count) {
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(128, (max_count + 2047) / 2048));
}

}  // namespace

hipError_t launch_assign_gather(const uint64_t *edges, uint64_t cap_per_shard, const unsigned long long *counts, uint64_t max_count, uint32_t q0,
                                uint32_t nq, uint32_t r0, uint32_t nm, const uint32_t *member_rank, uint32_t *scratch, uint32_t *start,
                                uint64_t *scan_scratch, uint64_t *rec, uint64_t rec_capacity, hipStream_t s) {
    uint32_t *cnt = scratch, *cursor = scratch + nq;
    hipError_t e = hipMemsetAsync(scratch, 0, ((size_t)2 * nq + 1) * sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    const uint32_t seg_x = seg_grid_x(max_count);
    const dim3 count_grid(capped_grid("k_assign_count", seg_x), HMK_EDGE_SHARDS), scatter_grid(capped_grid("k_assign_scatter", seg_x), HMK_EDGE_SHARDS);
    hipLaunchKernelGGL(k_assign_count, count_grid, dim3(256), 0, s, edges, cap_per_shard, counts, q0, nq, cnt);
    e = launch_scan_u32(cnt, start, nq, scan_scratch, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_assign_scatter, scatter_grid, dim3(256), 0, s, edges, cap_per_shard, counts, q0, nq, r0, nm, member_rank, start, cursor, rec,
                       rec_capacity);
    return hipGetLastError();
}

hipError_t launch_assign(const uint64_t *edges, uint64_t cap_per_shard, const unsigned long long *counts, uint64_t max_count, uint64_t total,
                         uint32_t q0, uint32_t nq, uint32_t r0, uint32_t nm, uint32_t k, const uint32_t *member_rank, const uint32_t *members_of_rank,
                         const uint32_t *slot_of_rank, uint32_t *scratch, uint32_t *start, uint64_t *scan_scratch, uint64_t *rec,
                         uint64_t rec_capacity, uint32_t *best_cluster, int32_t *best_score, uint32_t *n_feasible, hipStream_t s) {
    constexpr uint32_t LONG_RUN = 4096;   // longer runs: a workgroup each
    uint32_t *long_count = scratch + 2 * (size_t)nq, *long_list = long_count + 1;
    hipError_t e = launch_assign_gather(edges, cap_per_shard, counts, max_count, q0, nq, r0, nm, member_rank, scratch, start, scan_scratch, rec,
                                        rec_capacity, s);
    if (e != hipSuccess) return e;
    // a wave per new sequence, up to 8 workgroups per CU's worth (256 CUs), the rest grid-stride
    const uint32_t wave_grid = capped_grid("k_assign_wave", std::max(1u, std::min((nq + 3) / 4, 2048u)));
    hipLaunchKernelGGL(k_assign_wave, dim3(wave_grid), dim3(256), 0, s, start, rec, nq, k, LONG_RUN, members_of_rank, slot_of_rank, long_list,
                       long_count, best_cluster, best_score, n_feasible);
    // at most total / (LONG_RUN + 1) runs can be long: no workgroups for runs that cannot exist
    const uint64_t max_long = std::min<uint64_t>(nq, total / (LONG_RUN + 1));
    if (max_long)
        hipLaunchKernelGGL(k_assign_block, dim3(capped_grid("k_assign_block", (uint32_t)std::min<uint64_t>(max_long, 1024))), dim3(256), 0, s, start, rec, k,
                           members_of_rank, slot_of_rank, long_list, long_count, best_cluster, best_score, n_feasible);
    return hipGetLastError();
}

}  // namespace hmk
