// k_components.hip -- connected components of the neighbour graph {score >= t}, for t = threshold ... threshold_hi, from the packed
// edges of ONE neighbour pass at `threshold` (hmk_components_shifted, hmk_components_from_edges_dev; hmk_components.cpp).
//   k_cc_init         parent[i] = i, size[i] = 0
//   k_cc_hist         level = min(score, threshold_hi) - threshold of every edge: a histogram per workgroup in LDS, then one global add
//                     per level and workgroup
//   k_cc_scan         the levels' runs (one workgroup): start, cursor, and n_edges(t) = the histogram's suffix sum
//   k_cc_partition    (x, m) of every edge into its level's run: per chunk an LDS count, one returning global atomic per level and
//                     chunk for the place, the edges behind it
//   k_cc_union        one level's run into the union-find; k_cc_union_edges: the same straight from the packed edges (a single level)
//   k_cc_flatten      parent[v] = root(v), size[root] += 1
//   k_cc_sizes        singletons and the largest component from size[], which it clears
// The union-find (cc_find, cc_unite) and the argument for its relaxed agent-scope atomics are in hmk_cc_device.h, shared with
// k_density.hip.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "hmk_cc_device.h"
#include "hmk_components.h"
#include "hmk_grid.h"

namespace hmk {

namespace {

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor(v, o));
    return v;
}

// the run that holds chunk c (workgroup-uniform)
__device__ __forceinline__ uint32_t cc_run_of(const EdgeRuns &E, uint32_t c) {
    uint32_t lo = 0, hi = E.n_runs;   // chunk_start[lo] <= c < chunk_start[hi]
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (E.chunk_start[mid] <= c) lo = mid;
        else hi = mid;
    }
    return lo;
}

struct CcEdge { uint32_t x, m; int level; };   // level < 0: not an edge of this call

// entry j of the lane in chunk c: tested before any array is touched with its indices (bad: where an invalid one is flagged, or null)
__device__ __forceinline__ CcEdge cc_edge(const EdgeRuns &E, uint32_t run, uint32_t c, int j, uint32_t n, int thr, int thr_hi, uint32_t *bad) {
    CcEdge e{0, 0, -1};
    const unsigned long long k = (unsigned long long)(c - E.chunk_start[run]) * EDGE_RUN_CHUNK + (unsigned)j * 256u + threadIdx.x;
    if (k >= E.count[run]) return e;
    const uint64_t w = E.base[(unsigned long long)run * E.stride + k];
    e.x = HMK_EDGE_X(w);
    e.m = HMK_EDGE_M(w);
    if (e.x >= n || e.m >= n || e.x == e.m) {
        if (bad) atomicOr(bad, 1u);
        return e;
    }
    const int score = HMK_EDGE_SCORE(w);
    if (score >= thr) e.level = min(score, thr_hi) - thr;
    return e;
}

}  // namespace

__global__ void __launch_bounds__(256) k_cc_init(uint32_t *__restrict__ parent, uint32_t *__restrict__ size, uint32_t n) {
    for (unsigned long long v = (unsigned long long)blockIdx.x * 256 + threadIdx.x; v < n; v += (unsigned long long)gridDim.x * 256) {
        parent[v] = (uint32_t)v;
        size[v] = 0;
    }
}

__global__ void __launch_bounds__(256) k_cc_hist(const EdgeRuns E, uint32_t n, int thr, int thr_hi, CcState *__restrict__ st) {
    __shared__ uint32_t cnt[CC_MAX_LEVELS];
    cnt[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t n_chunks = E.chunk_start[E.n_runs];
    uint32_t in_lds = 0;   // chunks counted since the last flush (workgroup-uniform): EDGE_RUN_CHUNK each, far from 2^32
    for (uint32_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const uint32_t run = cc_run_of(E, c);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const CcEdge e = cc_edge(E, run, c, j, n, thr, thr_hi, &st->levels[0].reserved);
            if (e.level >= 0) atomicAdd(&cnt[e.level], 1u);
        }
        if (++in_lds == (1u << 20)) {   // (a workgroup that takes 2^20 chunks: one capped to a single workgroup at 10^9 edges)
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

__global__ void __launch_bounds__(256) k_cc_scan(uint32_t n_levels, CcState *__restrict__ st) {
    const uint32_t l = threadIdx.x;
    if (l >= n_levels) return;
    unsigned long long before = 0, total = 0;
    for (uint32_t k = 0; k < n_levels; k++) {
        const unsigned long long h = st->hist[k];
        if (k < l) before += h;
        total += h;
    }
    st->start[l] = st->cursor[l] = before;
    st->levels[l].n_edges = total - before;
    if (l == 0) st->start[n_levels] = total;
}

__global__ void __launch_bounds__(256) k_cc_partition(const EdgeRuns E, uint32_t n, int thr, int thr_hi, CcState *st,
                                                      uint64_t *__restrict__ runs) {
    __shared__ uint32_t cnt[CC_MAX_LEVELS];
    __shared__ unsigned long long base[CC_MAX_LEVELS];
    const uint32_t n_chunks = E.chunk_start[E.n_runs];
    for (uint32_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const uint32_t run = cc_run_of(E, c);
        cnt[threadIdx.x] = 0;
        __syncthreads();
        CcEdge e[4];
        uint32_t rank[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            e[j] = cc_edge(E, run, c, j, n, thr, thr_hi, nullptr);   // (k_cc_hist has flagged the invalid ones)
            rank[j] = e[j].level >= 0 ? atomicAdd(&cnt[e[j].level], 1u) : 0u;
        }
        __syncthreads();
        if (cnt[threadIdx.x]) base[threadIdx.x] = atomicAdd(&st->cursor[threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (e[j].level < 0) continue;
            const unsigned long long at = base[e[j].level] + rank[j];
            if (at < st->start[e[j].level + 1]) runs[at] = (uint64_t)e[j].x << 32 | e[j].m;   // (the run is exactly as long as k_cc_hist counted)
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) k_cc_union(const uint64_t *__restrict__ runs, uint32_t level, uint32_t *parent, CcState *__restrict__ st) {
    const unsigned long long r0 = st->start[level], len = st->start[level + 1] - r0;
    uint32_t hooks = 0;
    for (unsigned long long k = (unsigned long long)blockIdx.x * 256 + threadIdx.x; k < len; k += (unsigned long long)gridDim.x * 256) {
        const uint64_t w = runs[r0 + k];
        hooks += cc_unite(parent, (uint32_t)(w >> 32), (uint32_t)w) ? 1u : 0u;
    }
    hooks = wave_sum(hooks);
    if ((threadIdx.x & 63) == 0 && hooks) atomicAdd(&st->levels[level].n_components, hooks);
}

__global__ void __launch_bounds__(256) k_cc_union_edges(const EdgeRuns E, uint32_t n, int thr, uint32_t *parent, CcState *__restrict__ st) {
    const uint32_t n_chunks = E.chunk_start[E.n_runs];
    uint32_t hooks = 0, edges = 0;
    for (uint32_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const uint32_t run = cc_run_of(E, c);
#pragma unroll 1
        for (int j = 0; j < 4; j++) {
            const CcEdge e = cc_edge(E, run, c, j, n, thr, thr, &st->levels[0].reserved);
            if (e.level < 0) continue;
            edges++;
            hooks += cc_unite(parent, e.x, e.m) ? 1u : 0u;
        }
    }
    hooks = wave_sum(hooks);
    edges = wave_sum(edges);
    if ((threadIdx.x & 63) == 0) {
        if (hooks) atomicAdd(&st->levels[0].n_components, hooks);
        if (edges) atomicAdd((unsigned long long *)&st->levels[0].n_edges, (unsigned long long)edges);
    }
}

// (a launch of its own: nothing hooks while it runs, so a plain load sees a parent or, where another lane has flattened it already,
// the root -- either way an ancestor)
__global__ void __launch_bounds__(256) k_cc_flatten(uint32_t *parent, uint32_t *size, uint32_t n) {
    for (unsigned long long v0 = (unsigned long long)blockIdx.x * 256; v0 < n; v0 += (unsigned long long)gridDim.x * 256) {
        const unsigned long long v = v0 + threadIdx.x;
        if (v >= n) continue;
        uint32_t r = (uint32_t)v, p = parent[r];
        while (p != r) {
            r = p;
            p = parent[r];
        }
        parent[v] = r;
        // one add per distinct root of the wave: in a graph that is one component, one add per wave and not 64 to one word
        for (bool done = false; !done;) {
            const uint32_t lead = __builtin_amdgcn_readfirstlane(r);
            const unsigned long long same = __ballot(r == lead);
            if (r == lead) {
                if ((unsigned)__ffsll((long long)same) - 1u == (threadIdx.x & 63u)) atomicAdd(size + lead, (uint32_t)__popcll(same));
                done = true;
            }
        }
    }
}

__global__ void __launch_bounds__(256) k_cc_sizes(uint32_t *__restrict__ size, uint32_t n, uint32_t level, CcState *__restrict__ st) {
    uint32_t ones = 0, largest = 0;
    for (unsigned long long v = (unsigned long long)blockIdx.x * 256 + threadIdx.x; v < n; v += (unsigned long long)gridDim.x * 256) {
        const uint32_t s = size[v];
        if (s == 0) continue;
        ones += s == 1 ? 1u : 0u;
        largest = max(largest, s);
        size[v] = 0;
    }
    ones = wave_sum(ones);
    largest = wave_max(largest);
    if ((threadIdx.x & 63) == 0) {
        if (ones) atomicAdd(&st->levels[level].n_singletons, ones);
        if (largest) atomicMax(&st->levels[level].largest, largest);
    }
}

// -----------------------------------------------------------------------------
// launchers
// -----------------------------------------------------------------------------
namespace {
uint32_t vertex_grid(const char *kernel, uint32_t n) { return capped_grid(kernel, std::min<uint32_t>((n + 255) / 256, 2048)); }
uint32_t chunk_grid(const char *kernel, const EdgeRuns &E) { return capped_grid(kernel, std::min<uint32_t>(E.chunk_start[E.n_runs], 4096)); }
}  // namespace

hipError_t launch_cc_init(uint32_t *parent, uint32_t *size, uint32_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_cc_init, dim3(vertex_grid("k_cc_init", n)), dim3(256), 0, s, parent, size, n);
    return hipGetLastError();
}

hipError_t launch_cc_hist(const EdgeRuns &E, uint32_t n, int thr, int thr_hi, CcState *st, hipStream_t s) {
    if (E.chunk_start[E.n_runs] == 0) return hipSuccess;
    hipLaunchKernelGGL(k_cc_hist, dim3(chunk_grid("k_cc_hist", E)), dim3(256), 0, s, E, n, thr, thr_hi, st);
    return hipGetLastError();
}

hipError_t launch_cc_scan(uint32_t n_levels, CcState *st, hipStream_t s) {
    hipLaunchKernelGGL(k_cc_scan, dim3(1), dim3(CC_MAX_LEVELS), 0, s, n_levels, st);
    return hipGetLastError();
}

hipError_t launch_cc_partition(const EdgeRuns &E, uint32_t n, int thr, int thr_hi, CcState *st, uint64_t *runs, hipStream_t s) {
    if (E.chunk_start[E.n_runs] == 0) return hipSuccess;
    hipLaunchKernelGGL(k_cc_partition, dim3(chunk_grid("k_cc_partition", E)), dim3(256), 0, s, E, n, thr, thr_hi, st, runs);
    return hipGetLastError();
}

hipError_t launch_cc_union(const uint64_t *runs, unsigned long long total_edges, uint32_t level, uint32_t *parent, CcState *st, hipStream_t s) {
    if (total_edges == 0) return hipSuccess;
    const uint32_t blocks = capped_grid("k_cc_union", (uint32_t)std::min<unsigned long long>((total_edges + 255) / 256, 2048));
    hipLaunchKernelGGL(k_cc_union, dim3(blocks), dim3(256), 0, s, runs, level, parent, st);
    return hipGetLastError();
}

hipError_t launch_cc_union_edges(const EdgeRuns &E, uint32_t n, int thr, uint32_t *parent, CcState *st, hipStream_t s) {
    if (E.chunk_start[E.n_runs] == 0) return hipSuccess;
    hipLaunchKernelGGL(k_cc_union_edges, dim3(chunk_grid("k_cc_union_edges", E)), dim3(256), 0, s, E, n, thr, parent, st);
    return hipGetLastError();
}

hipError_t launch_cc_flatten(uint32_t *parent, uint32_t *size, uint32_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_cc_flatten, dim3(vertex_grid("k_cc_flatten", n)), dim3(256), 0, s, parent, size, n);
    return hipGetLastError();
}

hipError_t launch_cc_sizes(uint32_t *size, uint32_t n, uint32_t level, CcState *st, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_cc_sizes, dim3(vertex_grid("k_cc_sizes", n)), dim3(256), 0, s, size, n, level, st);
    return hipGetLastError();
}

}  // namespace hmk
