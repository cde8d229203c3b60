// k_search.hip -- the device side of the query-vs-reference searches (hmk_search.cpp): the HMK_EDGE_SHARDS segments of a
// search pass oriented so that m is the query (the scoring kernels emit (min, max) caller indices under a symmetric matrix)
// and packed into one block; the best k references of every query selected on the device (count, scan, scatter, select).
// Every store here is an ordinary vector store; the counters are vector atomics.
#include "hmk_device.h"
#include "hmk_grid.h"

namespace hmk {

namespace {

// the edge with m = the end that lies in the query range [q0, q1) (the other end is a reference: the ranges are disjoint)
__device__ __forceinline__ uint64_t orient_to_query(uint64_t e, uint32_t q0, uint32_t nq) {
    const uint32_t x = (uint32_t)(e >> 40), m = (uint32_t)(e >> 16) & 0xFFFFFFu;
    if (m - q0 < nq) return e;
    return pack_edge(m, x, (int)(uint32_t)e);
}

// selection key of a query's hit: larger = better, i.e. score descending, then reference index ascending.  Scores are >= the
// threshold >= -30000, so a key is never 0 (the "nothing" of the selection below).
__device__ __forceinline__ uint64_t hit_key(uint64_t e) {
    const int score = (int)(int16_t)(e & 0xFFFFu);
    const uint32_t x = (uint32_t)(e >> 40);
    return ((uint64_t)(uint32_t)(score + 32768) << 32) | (uint64_t)(0xFFFFFFFFu - x);
}

// offset of segment `shard` in the packed block, and the segment's own count (clamped to the segment: an overflowed pass is
// scored again by the caller before any of this runs)
__device__ __forceinline__ uint64_t segment_base(const unsigned long long *counts, uint64_t cap_per_shard, uint32_t shard, uint64_t *cnt) {
    uint64_t base = 0;
    for (uint32_t q = 0; q < shard; q++) base += min((uint64_t)counts[q], cap_per_shard);
    *cnt = min((uint64_t)counts[shard], cap_per_shard);
    return base;
}

__global__ void __launch_bounds__(256)
k_search_compact(const uint64_t *__restrict__ edges, uint64_t cap_per_shard, const unsigned long long *__restrict__ counts, uint32_t q0,
                 uint32_t nq, uint64_t *__restrict__ out, uint64_t out_capacity) {
    const uint32_t shard = blockIdx.y;
    uint64_t cnt;
    const uint64_t base = segment_base(counts, cap_per_shard, shard, &cnt);
    const uint64_t *seg = edges + (uint64_t)shard * cap_per_shard;
    for (uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x; k < cnt; k += (uint64_t)gridDim.x * 256)
        if (base + k < out_capacity) out[base + k] = orient_to_query(seg[k], q0, nq);
}

// hits per query (cnt: zeroed uint32[nq])
__global__ void __launch_bounds__(256)
k_search_count(const uint64_t *__restrict__ edges, uint64_t cap_per_shard, const unsigned long long *__restrict__ counts, uint32_t q0,
               uint32_t nq, uint32_t *__restrict__ cnt) {
    const uint32_t shard = blockIdx.y;
    const uint64_t n = min((uint64_t)counts[shard], cap_per_shard);
    const uint64_t *seg = edges + (uint64_t)shard * cap_per_shard;
    for (uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (uint64_t)gridDim.x * 256) {
        const uint64_t e = orient_to_query(seg[k], q0, nq);
        atomicAdd(&cnt[((uint32_t)(e >> 16) & 0xFFFFFFu) - q0], 1u);
    }
}

// every hit's key into its query's run keys[start[q] .. start[q + 1]) (cursor: zeroed uint32[nq]; order inside a run arbitrary)
__global__ void __launch_bounds__(256)
k_search_scatter(const uint64_t *__restrict__ edges, uint64_t cap_per_shard, const unsigned long long *__restrict__ counts, uint32_t q0,
                 uint32_t nq, const uint32_t *__restrict__ start, uint32_t *__restrict__ cursor, uint64_t *__restrict__ keys, uint64_t keys_capacity) {
    const uint32_t shard = blockIdx.y;
    const uint64_t n = min((uint64_t)counts[shard], cap_per_shard);
    const uint64_t *seg = edges + (uint64_t)shard * cap_per_shard;
    for (uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (uint64_t)gridDim.x * 256) {
        const uint64_t e = orient_to_query(seg[k], q0, nq);
        const uint32_t q = ((uint32_t)(e >> 16) & 0xFFFFFFu) - q0;
        const uint64_t pos = (uint64_t)start[q] + atomicAdd(&cursor[q], 1u);
        if (pos < keys_capacity) keys[pos] = hit_key(e);
    }
}

__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const uint64_t w = __shfl_xor(v, o, 64);
        v = w > v ? w : v;
    }
    return v;
}

// the k best keys of one run, one after the other: round t takes the largest key below round t - 1's.  `lanes` threads share the
// run (a wave, or a workgroup that reduces its waves' maxima through `red`).  Lane 0 writes the query's row of the output.
template <int LANES>
__device__ __forceinline__ void select_best(const uint64_t *__restrict__ run, uint32_t len, uint32_t k, uint32_t lane, uint64_t *red,
                                            uint32_t *__restrict__ hit_index, int32_t *__restrict__ hit_score, uint32_t *__restrict__ n_hits) {
    uint64_t prev = ~0ull;
    uint32_t found = 0;
    for (uint32_t t = 0; t < k; t++) {
        uint64_t best = 0;
        for (uint32_t i = lane; i < len; i += LANES) {
            const uint64_t v = run[i];
            if (v < prev && v > best) best = v;
        }
        best = wave_max_u64(best);
        if (LANES > 64) {
            __syncthreads();   // the previous round's reads of red[] are done
            if ((lane & 63u) == 0) red[lane >> 6] = best;
            __syncthreads();
            best = 0;
            for (int w = 0; w < LANES / 64; w++) best = red[w] > best ? red[w] : best;
        }
        if (best == 0) break;   // (uniform over the lanes: every lane reduced the same values)
        if (lane == 0) {
            hit_index[t] = 0xFFFFFFFFu - (uint32_t)best;
            hit_score[t] = (int32_t)(best >> 32) - 32768;
        }
        found++;
        prev = best;
    }
    if (lane == 0) {
        for (uint32_t t = found; t < k; t++) { hit_index[t] = 0xFFFFFFFFu; hit_score[t] = INT32_MIN; }
        *n_hits = found;
    }
}

// one wave per query whose run holds at most `long_run` hits (4 queries per workgroup)
__global__ void __launch_bounds__(256)
k_search_best_wave(const uint32_t *__restrict__ start, const uint64_t *__restrict__ keys, uint32_t nq, uint32_t k, uint32_t long_run,
                   uint32_t *__restrict__ hit_index, int32_t *__restrict__ hit_score, uint32_t *__restrict__ n_hits) {
    const uint32_t q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= nq) return;
    const uint32_t b = start[q], len = start[q + 1] - b;
    if (len > long_run) return;
    select_best<64>(keys + b, len, k, threadIdx.x & 63u, nullptr, hit_index + (uint64_t)q * k, hit_score + (uint64_t)q * k, n_hits + q);
}

// one workgroup per query with a longer run (the others leave at once)
__global__ void __launch_bounds__(256)
k_search_best_block(const uint32_t *__restrict__ start, const uint64_t *__restrict__ keys, uint32_t nq, uint32_t k, uint32_t long_run,
                    uint32_t *__restrict__ hit_index, int32_t *__restrict__ hit_score, uint32_t *__restrict__ n_hits) {
    __shared__ uint64_t red[4];
    const uint32_t q = blockIdx.x;
    const uint32_t b = start[q], len = start[q + 1] - b;
    if (len <= long_run) return;
    select_best<256>(keys + b, len, k, threadIdx.x, red, hit_index + (uint64_t)q * k, hit_score + (uint64_t)q * k, n_hits + q);
}

// workgroups per segment: from the longest segment's count (the host has the counts), ~2,048 edges each
uint32_t seg_grid_x(uint64_t max_count) {
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(128, (max_count + 2047) / 2048));
}

}  // namespace

hipError_t launch_search_compact(const uint64_t *edges, uint64_t cap_per_shard, const unsigned long long *counts, uint64_t max_count,
                                 uint32_t q0, uint32_t nq, uint64_t *out, uint64_t out_capacity, hipStream_t s) {
    const dim3 seg_grid(capped_grid("k_search_compact", seg_grid_x(max_count)), HMK_EDGE_SHARDS);
    hipLaunchKernelGGL(k_search_compact, seg_grid, dim3(256), 0, s, edges, cap_per_shard, counts, q0, nq, out, out_capacity);
    return hipGetLastError();
}

hipError_t launch_search_best(const uint64_t *edges, uint64_t cap_per_shard, const unsigned long long *counts, uint64_t max_count,
                              uint32_t q0, uint32_t nq, uint32_t k, uint32_t *cnt_cursor, uint32_t *start, uint64_t *scan_scratch, uint64_t *keys, uint64_t keys_capacity,
                              uint32_t *hit_index, int32_t *hit_score, uint32_t *n_hits, hipStream_t s) {
    constexpr uint32_t LONG_RUN = 4096;   // longer runs: a workgroup each
    uint32_t *cnt = cnt_cursor, *cursor = cnt_cursor + nq;
    hipError_t e = hipMemsetAsync(cnt_cursor, 0, (size_t)2 * nq * sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    const uint32_t seg_x = seg_grid_x(max_count);
    const dim3 count_grid(capped_grid("k_search_count", seg_x), HMK_EDGE_SHARDS), scatter_grid(capped_grid("k_search_scatter", seg_x), HMK_EDGE_SHARDS);
    hipLaunchKernelGGL(k_search_count, count_grid, dim3(256), 0, s, edges, cap_per_shard, counts, q0, nq, cnt);
    e = launch_scan_u32(cnt, start, nq, scan_scratch, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_search_scatter, scatter_grid, dim3(256), 0, s, edges, cap_per_shard, counts, q0, nq, start, cursor, keys, keys_capacity);
    hipLaunchKernelGGL(k_search_best_wave, dim3((nq + 3) / 4), dim3(256), 0, s, start, keys, nq, k, LONG_RUN, hit_index, hit_score, n_hits);
    hipLaunchKernelGGL(k_search_best_block, dim3(nq), dim3(256), 0, s, start, keys, nq, k, LONG_RUN, hit_index, hit_score, n_hits);
    return hipGetLastError();
}

}  // namespace hmk
