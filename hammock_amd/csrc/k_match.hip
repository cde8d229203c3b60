// k_match.hip -- the device side of the match of query clusters to existing clusters (hmk_match.cpp).  After the pass over
// existing members x query members, in two levels built from the assignment's pieces (k_assign.hip, k_assign_table.h):
//   level 1, per query member x: the assignment's gather (every hit as a (cluster rank, score) record in x's run), the run
//            aggregated in the LDS table, and EVERY feasible (rank, min score) record of x written to a second buffer at x's
//            own run offsets (a feasible cluster has a hit, so they fit);
//   level 2, per query cluster b: its members' feasible records gathered into b's run (count, scan, copy), aggregated in the
//            same table (per rank: the members it is feasible for, the minimum of their minima), a rank feasible for b when
//            that number is b's member count, and the best k selected by the assignment's key.
// Every store here is an ordinary vector store; the counters are vector atomics.
#include "hmk_device.h"
#include "k_assign_table.h"
#include "hmk_grid.h"

namespace hmk {

namespace {

constexpr uint32_t LONG_RUN = 4096;   // longer runs: a workgroup each (both levels)

// level 1: one wave per query member whose run holds at most `long_run` records (4 waves per workgroup, grid-stride); the
// longer runs are listed in long_list[0 .. *long_count) for k_match_feasible_block.  feas: x's feasible records at start[x],
// n_feas[x]: how many
__global__ void __launch_bounds__(256)
k_match_feasible_wave(const uint32_t *__restrict__ start, const uint64_t *__restrict__ rec, uint32_t nq, uint32_t long_run,
                      const uint32_t *__restrict__ members_of_rank, uint32_t *__restrict__ long_list, uint32_t *__restrict__ long_count,
                      uint64_t *__restrict__ feas, uint32_t *__restrict__ n_feas) {
    __shared__ int32_t keys_all[4 * WAVE_SLOTS];
    __shared__ uint32_t hits_all[4 * WAVE_SLOTS];
    __shared__ uint32_t mn_all[4 * WAVE_SLOTS];
    __shared__ uint16_t used_all[4 * WAVE_SLOTS];
    __shared__ uint32_t n_used_all[4], n_out_all[4];
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
        T.run_all(rec + b, len, members_of_rank, lane, feas + b, n_out_all + wv, n_feas + q);
    }
}

// level 1: one workgroup per listed long run (grid-stride over the list)
__global__ void __launch_bounds__(256)
k_match_feasible_block(const uint32_t *__restrict__ start, const uint64_t *__restrict__ rec, const uint32_t *__restrict__ members_of_rank,
                       const uint32_t *__restrict__ long_list, const uint32_t *__restrict__ long_count, uint64_t *__restrict__ feas,
                       uint32_t *__restrict__ n_feas) {
    __shared__ int32_t keys[BLOCK_SLOTS];
    __shared__ uint32_t hits[BLOCK_SLOTS];
    __shared__ uint32_t mn[BLOCK_SLOTS];
    __shared__ uint16_t used[BLOCK_SLOTS];
    __shared__ uint32_t n_used, n_out;
    __shared__ uint64_t red[4];
    const RunTable<256, BLOCK_SLOTS> T{keys, hits, mn, used, &n_used, red};
    const uint32_t n_long = *long_count;
    if (blockIdx.x >= n_long) return;   // (uniform)
    T.init(threadIdx.x);
    for (uint32_t i = blockIdx.x; i < n_long; i += gridDim.x) {
        const uint32_t q = long_list[i];
        const uint32_t b = start[q], len = start[q + 1] - b;
        T.run_all(rec + b, len, members_of_rank, threadIdx.x, feas + b, &n_out, n_feas + q);
    }
}

// level 2: feasible records per query cluster (cnt: zeroed uint32[nb])
__global__ void __launch_bounds__(256)
k_match_count(const uint32_t *__restrict__ n_feas, const uint32_t *__restrict__ query_slot, uint32_t nq, uint32_t *__restrict__ cnt) {
    for (uint32_t q = blockIdx.x * 256 + threadIdx.x; q < nq; q += gridDim.x * 256) {
        const uint32_t n = n_feas[q];
        if (n) atomicAdd(&cnt[query_slot[q]], n);
    }
}

// level 2: every query member's feasible records copied into its cluster's run rec2[start2[b] .. start2[b + 1]), one wave per
// member (grid-stride); cursor: zeroed uint32[nb], order inside a run arbitrary
__global__ void __launch_bounds__(256)
k_match_copy(const uint32_t *__restrict__ start, const uint64_t *__restrict__ feas, const uint32_t *__restrict__ n_feas,
             const uint32_t *__restrict__ query_slot, uint32_t nq, const uint32_t *__restrict__ start2, uint32_t *__restrict__ cursor,
             uint64_t *__restrict__ rec2, uint64_t rec2_capacity) {
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    for (uint32_t q = blockIdx.x * 4 + wv; q < nq; q += gridDim.x * 4) {   // (wave-uniform)
        const uint32_t n = n_feas[q];
        if (n == 0) continue;
        const uint32_t b = query_slot[q];
        uint32_t at = 0;
        if (lane == 0) at = atomicAdd(&cursor[b], n);
        at = __shfl(at, 0, 64);
        const uint64_t dst = (uint64_t)start2[b] + at;
        const uint64_t *src = feas + start[q];
        for (uint32_t i = lane; i < n; i += 64)
            if (dst + i < rec2_capacity) rec2[dst + i] = src[i];
    }
}

// level 2: one wave per query cluster whose run holds at most `long_run` records; the longer runs are listed for
// k_match_select_block.  members[b]: b's member count, which a rank's record count must reach
__global__ void __launch_bounds__(256)
k_match_select_wave(const uint32_t *__restrict__ start2, const uint64_t *__restrict__ rec2, uint32_t nb, uint32_t k, uint32_t long_run,
                    const uint32_t *__restrict__ members, const uint32_t *__restrict__ slot_of_rank, uint32_t *__restrict__ long_list,
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
    for (uint32_t c = blockIdx.x * 4 + wv; c < nb; c += gridDim.x * 4) {   // (wave-uniform)
        const uint32_t b = start2[c], len = start2[c + 1] - b;
        if (len > long_run) {
            if (lane == 0) long_list[atomicAdd(long_count, 1u)] = c;
            continue;
        }
        T.run(rec2 + b, len, UniformNeed{members[c]}, slot_of_rank, k, lane, best_cluster + (uint64_t)c * k, best_score + (uint64_t)c * k,
              n_feasible + c);
    }
}

// level 2: one workgroup per listed long run (grid-stride over the list)
__global__ void __launch_bounds__(256)
k_match_select_block(const uint32_t *__restrict__ start2, const uint64_t *__restrict__ rec2, uint32_t k, const uint32_t *__restrict__ members,
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
        const uint32_t c = long_list[i];
        const uint32_t b = start2[c], len = start2[c + 1] - b;
        T.run(rec2 + b, len, UniformNeed{members[c]}, slot_of_rank, k, threadIdx.x, best_cluster + (uint64_t)c * k, best_score + (uint64_t)c * k,
              n_feasible + c);
    }
}

// a wave per item, up to 8 workgroups per CU's worth (256 CUs), the rest grid-stride
uint32_t wave_grid(uint32_t n) {
    return std::max(1u, std::min((n + 3) / 4, 2048u));
}

}  // namespace

hipError_t launch_match(const uint64_t *edges, uint64_t cap_per_shard, const unsigned long long *counts, uint64_t max_count, uint64_t total,
                        uint32_t q0, uint32_t nq, uint32_t r0, uint32_t nm, uint32_t nb, uint32_t k, const uint32_t *member_rank,
                        const uint32_t *members_of_rank, const uint32_t *slot_of_rank, const uint32_t *query_slot, const uint32_t *query_members,
                        uint32_t *scratch, uint32_t *start, uint64_t *scan_scratch, uint64_t *rec, uint64_t *feas, uint64_t rec_capacity,
                        uint32_t *scratch2, uint32_t *start2, uint32_t *best_cluster, int32_t *best_score, uint32_t *n_feasible, hipStream_t s) {
    // at most total / (LONG_RUN + 1) runs of either level can be long (level 2 holds at most `total` records): no workgroups for
    // runs that cannot exist
    const uint64_t max_long = total / (LONG_RUN + 1);
    // level 1
    uint32_t *long_count = scratch + 2 * (size_t)nq, *long_list = long_count + 1;
    hipError_t e = launch_assign_gather(edges, cap_per_shard, counts, max_count, q0, nq, r0, nm, member_rank, scratch, start, scan_scratch, rec,
                                        rec_capacity, s);
    if (e != hipSuccess) return e;
    uint32_t *n_feas = scratch2, *cnt2 = scratch2 + nq, *cursor2 = cnt2 + nb, *long_count2 = cursor2 + nb, *long_list2 = long_count2 + 1;
    e = hipMemsetAsync(cnt2, 0, ((size_t)2 * nb + 1) * sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_match_feasible_wave, dim3(capped_grid("k_match_feasible_wave", wave_grid(nq))), dim3(256), 0, s, start, rec, nq, LONG_RUN,
                       members_of_rank, long_list, long_count, feas, n_feas);
    if (const uint32_t n_block = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(nq, max_long), 1024))
        hipLaunchKernelGGL(k_match_feasible_block, dim3(capped_grid("k_match_feasible_block", n_block)), dim3(256), 0, s,
                           start, rec, members_of_rank, long_list, long_count, feas, n_feas);
    // level 2: the gather into the query clusters' runs (rec is free again: it holds them)
    const uint32_t count_grid = capped_grid("k_match_count", std::max(1u, std::min((nq + 255) / 256, 1024u)));
    hipLaunchKernelGGL(k_match_count, dim3(count_grid), dim3(256), 0, s, n_feas, query_slot, nq, cnt2);
    e = launch_scan_u32(cnt2, start2, nb, scan_scratch, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_match_copy, dim3(capped_grid("k_match_copy", wave_grid(nq))), dim3(256), 0, s, start, feas, n_feas, query_slot, nq, start2, cursor2,
                       rec, rec_capacity);
    hipLaunchKernelGGL(k_match_select_wave, dim3(capped_grid("k_match_select_wave", wave_grid(nb))), dim3(256), 0, s, start2, rec, nb, k, LONG_RUN,
                       query_members, slot_of_rank, long_list2, long_count2, best_cluster, best_score, n_feasible);
    if (const uint32_t n_block = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(nb, max_long), 1024))
        hipLaunchKernelGGL(k_match_select_block, dim3(capped_grid("k_match_select_block", n_block)), dim3(256), 0, s,
                           start2, rec, k, query_members, slot_of_rank, long_list2, long_count2, best_cluster, best_score, n_feasible);
    return hipGetLastError();
}

}  // namespace hmk
