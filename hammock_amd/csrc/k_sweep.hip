// k_sweep.hip -- the packed edges of ONE neighbour pass at `threshold`, dealt into one run per level min(score, threshold_hi) -
// threshold with the runs laid out from the top level down (hmk_greedy_sweep*; hmk_sweep.cpp).  The edges with score >= t are then
// the prefix dealt[0 .. prefix[t - threshold]) of one buffer: the clustering tail takes every threshold's graph as one segment of it,
// and nothing is copied or compacted per level.  The whole 8-byte edge is kept: the tail needs the score.
//   k_sweep_hist   the level of every edge: a histogram per workgroup in LDS, then one 64-bit global add per non-empty level and workgroup
//   k_sweep_scan   the runs (one workgroup): start and cursor of each level, descending, and prefix[l] = the edges of the levels >= l
//   k_sweep_deal   every edge into its level's run: per chunk an LDS rank, one returning global atomic per non-empty level and chunk
//                  for the place, the edges behind it
// An edge is tested (x < n, m < n, x != m) before anything is indexed with it; k_sweep_hist raises the flag, both kernels leave
// such an edge out, and the host does not start a tail on a flagged call.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "hmk_sweep.h"
#include "hmk_grid.h"

namespace hmk {

namespace {

// the run that holds chunk c (workgroup-uniform)
__device__ __forceinline__ uint32_t sweep_run_of(const EdgeRuns &E, uint32_t c) {
    uint32_t lo = 0, hi = E.n_runs;   // chunk_start[lo] <= c < chunk_start[hi]
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (E.chunk_start[mid] <= c) lo = mid;
        else hi = mid;
    }
    return lo;
}

// entry j of the lane in chunk c -> its level, or -1: past the run's end, invalid (then *bad is raised, if given) or below thr.
// w = the edge as stored.
__device__ __forceinline__ int sweep_level(const EdgeRuns &E, uint32_t run, uint32_t c, int j, uint32_t n, int thr, int thr_hi,
                                           unsigned long long *bad, uint64_t &w) {
    const unsigned long long k = (unsigned long long)(c - E.chunk_start[run]) * EDGE_RUN_CHUNK + (unsigned)j * 256u + threadIdx.x;
    w = 0;
    if (k >= E.count[run]) return -1;
    w = E.base[(unsigned long long)run * E.stride + k];
    const uint32_t x = HMK_EDGE_X(w), m = HMK_EDGE_M(w);
    if (x >= n || m >= n || x == m) {
        if (bad) atomicOr(bad, 1ull);
        return -1;
    }
    const int score = HMK_EDGE_SCORE(w);
    return score >= thr ? min(score, thr_hi) - thr : -1;
}

}  // namespace

__global__ void __launch_bounds__(256) k_sweep_hist(const EdgeRuns E, uint32_t n, int thr, int thr_hi, SweepState *__restrict__ st) {
    __shared__ uint32_t cnt[SWEEP_MAX_LEVELS];
    cnt[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t n_chunks = E.chunk_start[E.n_runs];
    uint32_t in_lds = 0;   // chunks counted since the last flush (workgroup-uniform)
    for (uint32_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const uint32_t run = sweep_run_of(E, c);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            uint64_t w;
            const int level = sweep_level(E, run, c, j, n, thr, thr_hi, &st->flag, w);
            if (level >= 0) atomicAdd(&cnt[level], 1u);
        }
        if (++in_lds == SWEEP_FLUSH_CHUNKS) {   // (only a launch capped to very few workgroups over 10^9 edges gets here)
            __syncthreads();
            if (cnt[threadIdx.x]) atomicAdd(&st->hist[threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
            cnt[threadIdx.x] = 0;
            in_lds = 0;
            __syncthreads();
        }
    }
    __syncthreads();
    if (cnt[threadIdx.x]) atomicAdd(&st->hist[threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
}

__global__ void __launch_bounds__(256) k_sweep_scan(uint32_t n_levels, SweepState *__restrict__ st) {
    __shared__ unsigned long long h[SWEEP_MAX_LEVELS];
    const uint32_t l = threadIdx.x;
    h[l] = l < n_levels ? st->hist[l] : 0ull;
    __syncthreads();
    if (l >= n_levels) return;
    unsigned long long above = 0;   // the edges of the levels above l: their runs come first
    for (uint32_t k = l + 1; k < n_levels; k++) above += h[k];
    st->start[l] = st->cursor[l] = above;
    st->prefix[l] = above + h[l];
}

__global__ void __launch_bounds__(256) k_sweep_deal(const EdgeRuns E, uint32_t n, int thr, int thr_hi, SweepState *st,
                                                    uint64_t *__restrict__ dealt) {
    __shared__ uint32_t cnt[SWEEP_MAX_LEVELS];
    __shared__ unsigned long long base[SWEEP_MAX_LEVELS];
    const uint32_t n_chunks = E.chunk_start[E.n_runs];
    for (uint32_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const uint32_t run = sweep_run_of(E, c);
        cnt[threadIdx.x] = 0;
        __syncthreads();
        uint64_t w[4];
        int level[4];
        uint32_t rank[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            level[j] = sweep_level(E, run, c, j, n, thr, thr_hi, nullptr, w[j]);   // (k_sweep_hist has flagged the invalid ones)
            rank[j] = level[j] >= 0 ? atomicAdd(&cnt[level[j]], 1u) : 0u;
        }
        __syncthreads();
        if (cnt[threadIdx.x]) base[threadIdx.x] = atomicAdd(&st->cursor[threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (level[j] < 0) continue;
            const unsigned long long at = base[level[j]] + rank[j];
            if (at < st->prefix[level[j]]) dealt[at] = w[j];   // (the run is exactly as long as k_sweep_hist counted: it ends at prefix[level])
        }
        __syncthreads();
    }
}

// -----------------------------------------------------------------------------
// launchers
// -----------------------------------------------------------------------------
namespace {
uint32_t sweep_grid(const char *kernel, const EdgeRuns &E) { return capped_grid(kernel, std::min<uint32_t>(E.chunk_start[E.n_runs], SWEEP_MAX_GRID)); }
}  // namespace

hipError_t launch_sweep_hist(const EdgeRuns &E, uint32_t n, int thr, int thr_hi, SweepState *st, hipStream_t s) {
    if (E.chunk_start[E.n_runs] == 0) return hipSuccess;
    hipLaunchKernelGGL(k_sweep_hist, dim3(sweep_grid("k_sweep_hist", E)), dim3(256), 0, s, E, n, thr, thr_hi, st);
    return hipGetLastError();
}

hipError_t launch_sweep_scan(uint32_t n_levels, SweepState *st, hipStream_t s) {
    hipLaunchKernelGGL(k_sweep_scan, dim3(1), dim3(SWEEP_MAX_LEVELS), 0, s, n_levels, st);
    return hipGetLastError();
}

hipError_t launch_sweep_deal(const EdgeRuns &E, uint32_t n, int thr, int thr_hi, SweepState *st, uint64_t *dealt, hipStream_t s) {
    if (E.chunk_start[E.n_runs] == 0) return hipSuccess;
    hipLaunchKernelGGL(k_sweep_deal, dim3(sweep_grid("k_sweep_deal", E)), dim3(256), 0, s, E, n, thr, thr_hi, st, dealt);
    return hipGetLastError();
}

}  // namespace hmk
