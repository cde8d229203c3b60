// k_density.hip -- density clustering (DBSCAN on the similarity graph, made independent of any order) of the neighbour graph
// {score >= t}, for t = threshold_hi down to threshold, from the packed edges of ONE neighbour pass at `threshold`
// (hmk_density_shifted, hmk_density_from_edges_dev; hmk_density.cpp).  As t falls, degrees only grow, so the set of core vertices
// and the set of core-core edges only grow: one union-find, one anchor key and one degree per vertex carry over from level to level.
//   k_den_init      parent[i] = i; key, size, degree, state = 0
//   k_den_degree    the level's own run: +1 to both ends.  The pass writes edges row by row, so lanes of a wave share an end: equal
//                   ends of a wave are combined by ballot before the global add (up to DEN_COMBINE distinct values, then one by one)
//   k_den_core      state: core as of this level -> core; non-core with degree >= min_neighbors -> core as of this level (counted)
//   k_den_link      over the edges >= t.  An edge is looked at iff it lies in the level's own run or one of its ends turned core at
//                   this level: only such an edge can do something it has not done at an earlier level.  Both ends core: cc_unite.
//                   One end core: an atomic maximum of (score + 32768) << 32 | (0xFFFFFFFF - core index) into the other end's key.
//                   If no vertex turned core at this level, only the level's own run can matter, and the workgroups start there.
//   k_den_labels    core: the root, flattened; border: the root of the anchor its key names; noise.  The level's rows, size[label]
//                   += 1 (combined by ballot as the degrees), the three counts
//   k_den_sizes     the core roots (= clusters), the largest cluster from size[], which it clears
// The state bytes do not change while k_den_link runs, and it reads them by plain loads: they were written by the launch before.
// parent[] is only accessed through cc_find / cc_unite there (hmk_cc_device.h: relaxed atomics at agent scope, and why an old
// parent does no harm); the keys only by atomic maximum, so the final key is the maximum over all offers whatever their order.  An
// edge is tested (x < n, m < n, x != m) before anything is indexed with it.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "hmk_cc_device.h"
#include "hmk_density.h"
#include "hmk_grid.h"

namespace hmk {

namespace {

__device__ __forceinline__ uint32_t den_wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ uint32_t den_wave_max(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor(v, o));
    return v;
}

// the run that holds chunk c (workgroup-uniform)
__device__ __forceinline__ uint32_t den_run_of(const EdgeRuns &E, uint32_t c) {
    uint32_t lo = 0, hi = E.n_runs;   // chunk_start[lo] <= c < chunk_start[hi]
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (E.chunk_start[mid] <= c) lo = mid;
        else hi = mid;
    }
    return lo;
}

struct DenEdge {
    uint32_t x, m;
    int score;
    bool ok;    // an edge of this call: inside its run, valid, score >= thr
    bool own;   // it lies in the level's own run
};

// entry j of the lane in chunk c: tested before any array is touched with its indices (bad: where an invalid one is flagged, or null)
__device__ __forceinline__ DenEdge den_edge(const DenEdges &D, uint32_t run, uint32_t c, int j, uint32_t n, int thr, unsigned long long *bad) {
    DenEdge e{0, 0, 0, false, false};
    const unsigned long long k = (unsigned long long)(c - D.E.chunk_start[run]) * DEN_CHUNK + (unsigned)j * 256u + threadIdx.x;
    if (k >= D.E.count[run]) return e;
    const uint64_t w = D.E.base[(unsigned long long)run * D.E.stride + k];
    e.x = HMK_EDGE_X(w);
    e.m = HMK_EDGE_M(w);
    if (e.x >= n || e.m >= n || e.x == e.m) {
        if (bad) atomicOr(bad, 1ull);
        return e;
    }
    e.score = HMK_EDGE_SCORE(w);
    e.ok = e.score >= thr;
    e.own = run > 0 || k >= D.own_start;
    return e;
}

// arr[v] += 1 for every lane with `todo`, the lanes of a wave that name the same v combined into one add: up to DEN_COMBINE
// distinct values by ballot, the lanes left after that one by one.  Every lane of the wave calls it (todo = false: nothing to add).
__device__ __forceinline__ void den_add_combined(uint32_t *arr, uint32_t v, bool todo) {
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll 1
    for (int it = 0; it < DEN_COMBINE; it++) {
        const unsigned long long pend = __ballot(todo);
        if (!pend) return;
        const uint32_t src = (uint32_t)__ffsll((long long)pend) - 1u;
        const uint32_t lead = (uint32_t)__shfl((int)v, (int)src);
        const bool mine = todo && v == lead;
        const unsigned long long same = __ballot(mine);
        if (mine) {
            if (lane == src) atomicAdd(arr + lead, (uint32_t)__popcll(same));
            todo = false;
        }
    }
    if (todo) atomicAdd(arr + v, 1u);
}

// the root of v by plain loads (a launch in which nothing hooks: a word holds a parent or, where a lane has flattened it, the root)
__device__ __forceinline__ uint32_t den_root(const uint32_t *parent, uint32_t v) {
    uint32_t p = parent[v];
    while (p != v) {
        v = p;
        p = parent[v];
    }
    return v;
}

}  // namespace

__global__ void __launch_bounds__(256) k_den_init(const DenVertex V, uint32_t n) {
    for (unsigned long long v = (unsigned long long)blockIdx.x * 256 + threadIdx.x; v < n; v += (unsigned long long)gridDim.x * 256) {
        V.key[v] = 0;
        V.parent[v] = (uint32_t)v;
        V.size[v] = 0;
        V.degree[v] = 0;
        V.state[v] = DEN_NOT_CORE;
    }
}

__global__ void __launch_bounds__(256) k_den_degree(const DenEdges D, uint32_t n, int thr, uint32_t *__restrict__ degree, DenState *__restrict__ st,
                                                    uint32_t level) {
    const uint32_t n_chunks = D.E.chunk_start[D.E.n_runs];
    uint32_t edges = 0;
    for (uint32_t c = (uint32_t)(D.own_start / DEN_CHUNK) + blockIdx.x; c < n_chunks; c += gridDim.x) {
        const uint32_t run = den_run_of(D.E, c);
#pragma unroll 1
        for (int j = 0; j < 4; j++) {
            const DenEdge e = den_edge(D, run, c, j, n, thr, &st->flag);
            const bool mine = e.ok && e.own;
            edges += mine ? 1u : 0u;
            den_add_combined(degree, e.x, mine);
            den_add_combined(degree, e.m, mine);
        }
    }
    edges = den_wave_sum(edges);
    if ((threadIdx.x & 63) == 0 && edges) atomicAdd(&st->level[level].n_edges, (unsigned long long)edges);
}

__global__ void __launch_bounds__(256) k_den_core(uint32_t n, uint32_t min_neighbors, const uint32_t *__restrict__ degree, uint8_t *__restrict__ state,
                                                  DenState *__restrict__ st, uint32_t level) {
    uint32_t fresh = 0;
    for (unsigned long long v = (unsigned long long)blockIdx.x * 256 + threadIdx.x; v < n; v += (unsigned long long)gridDim.x * 256) {
        const uint8_t s = state[v];
        if (s == DEN_CORE_NEW) state[v] = DEN_CORE;
        else if (s == DEN_NOT_CORE && degree[v] >= min_neighbors) {
            state[v] = DEN_CORE_NEW;
            fresh++;
        }
    }
    fresh = den_wave_sum(fresh);
    if ((threadIdx.x & 63) == 0 && fresh) atomicAdd(&st->level[level].new_core, fresh);
}

__global__ void __launch_bounds__(256) k_den_link(const DenEdges D, uint32_t n, int thr, const uint8_t *__restrict__ state, uint32_t *parent,
                                                  unsigned long long *key, DenState *st, uint32_t level) {
    const uint32_t n_chunks = D.E.chunk_start[D.E.n_runs];
    // no vertex turned core at this level: the older edges have done all they can do, the workgroups start at the level's own run
    const uint32_t first = st->level[level].new_core ? 0u : (uint32_t)(D.own_start / DEN_CHUNK);
    uint32_t looked = 0;
    for (uint32_t c = first + blockIdx.x; c < n_chunks; c += gridDim.x) {
        const uint32_t run = den_run_of(D.E, c);
#pragma unroll 1
        for (int j = 0; j < 4; j++) {
            const DenEdge e = den_edge(D, run, c, j, n, thr, nullptr);   // (k_den_degree or the sweep's histogram has flagged the invalid ones)
            if (!e.ok) continue;
            const uint8_t sx = state[e.x], sm = state[e.m];
            if (!(e.own || sx == DEN_CORE_NEW || sm == DEN_CORE_NEW)) continue;
            looked++;
            if (sx != DEN_NOT_CORE && sm != DEN_NOT_CORE) cc_unite(parent, e.x, e.m);
            else if (sx != DEN_NOT_CORE || sm != DEN_NOT_CORE) {
                const uint32_t core = sx != DEN_NOT_CORE ? e.x : e.m, other = sx != DEN_NOT_CORE ? e.m : e.x;
                atomicMax(key + other, (unsigned long long)(uint32_t)(e.score + 32768) << 32 | (0xFFFFFFFFu - core));
            }
        }
    }
    looked = den_wave_sum(looked);
    if ((threadIdx.x & 63) == 0 && looked) atomicAdd(&st->level[level].looked, (unsigned long long)looked);
}

__global__ void __launch_bounds__(256) k_den_labels(uint32_t n, const DenVertex V, uint32_t *__restrict__ cluster_row, uint32_t *__restrict__ anchor_row,
                                                    uint32_t *__restrict__ degree_row, DenState *__restrict__ st, uint32_t level) {
    uint32_t cores = 0, borders = 0, noise = 0;
    for (unsigned long long v0 = (unsigned long long)blockIdx.x * 256; v0 < n; v0 += (unsigned long long)gridDim.x * 256) {
        const unsigned long long v = v0 + threadIdx.x;
        const bool in = v < n;
        uint32_t label = 0xFFFFFFFFu, anchor = 0xFFFFFFFFu;
        if (in) {
            if (V.state[v] != DEN_NOT_CORE) {
                anchor = (uint32_t)v;
                label = den_root(V.parent, anchor);
                V.parent[v] = label;
                cores++;
            } else if (const unsigned long long k = V.key[v]) {
                anchor = 0xFFFFFFFFu - (uint32_t)k;
                label = den_root(V.parent, anchor);
                borders++;
            } else noise++;
            if (cluster_row) cluster_row[v] = label;
            if (anchor_row) anchor_row[v] = anchor;
            if (degree_row) degree_row[v] = V.degree[v];
        }
        den_add_combined(V.size, label, in && label != 0xFFFFFFFFu);
    }
    cores = den_wave_sum(cores);
    borders = den_wave_sum(borders);
    noise = den_wave_sum(noise);
    if ((threadIdx.x & 63) == 0) {
        if (cores) atomicAdd(&st->level[level].n_core, cores);
        if (borders) atomicAdd(&st->level[level].n_border, borders);
        if (noise) atomicAdd(&st->level[level].n_noise, noise);
    }
}

__global__ void __launch_bounds__(256) k_den_sizes(uint32_t n, const DenVertex V, DenState *__restrict__ st, uint32_t level) {
    uint32_t roots = 0, largest = 0;
    for (unsigned long long v = (unsigned long long)blockIdx.x * 256 + threadIdx.x; v < n; v += (unsigned long long)gridDim.x * 256) {
        if (V.state[v] != DEN_NOT_CORE && V.parent[v] == (uint32_t)v) roots++;
        const uint32_t s = V.size[v];
        if (s == 0) continue;
        largest = max(largest, s);
        V.size[v] = 0;
    }
    roots = den_wave_sum(roots);
    largest = den_wave_max(largest);
    if ((threadIdx.x & 63) == 0) {
        if (roots) atomicAdd(&st->level[level].n_clusters, roots);
        if (largest) atomicMax(&st->level[level].largest, largest);
    }
}

// -----------------------------------------------------------------------------
// launchers
// -----------------------------------------------------------------------------
namespace {
uint32_t vertex_grid(const char *kernel, uint32_t n) { return capped_grid(kernel, std::min<uint32_t>((n + 255) / 256, DEN_MAX_GRID)); }
uint32_t chunk_grid(const char *kernel, uint32_t chunks) { return capped_grid(kernel, std::min<uint32_t>(chunks, DEN_MAX_GRID)); }
}  // namespace

hipError_t launch_den_init(const DenVertex &v, uint32_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_den_init, dim3(vertex_grid("k_den_init", n)), dim3(256), 0, s, v, n);
    return hipGetLastError();
}

hipError_t launch_den_degree(const DenEdges &D, uint32_t n, int thr, const DenVertex &v, DenState *st, uint32_t level, hipStream_t s) {
    const uint32_t n_chunks = D.E.chunk_start[D.E.n_runs], first = (uint32_t)(D.own_start / DEN_CHUNK);
    if (n_chunks <= first) return hipSuccess;
    hipLaunchKernelGGL(k_den_degree, dim3(chunk_grid("k_den_degree", n_chunks - first)), dim3(256), 0, s, D, n, thr, v.degree, st, level);
    return hipGetLastError();
}

hipError_t launch_den_core(uint32_t n, uint32_t min_neighbors, const DenVertex &v, DenState *st, uint32_t level, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_den_core, dim3(vertex_grid("k_den_core", n)), dim3(256), 0, s, n, min_neighbors, v.degree, v.state, st, level);
    return hipGetLastError();
}

hipError_t launch_den_link(const DenEdges &D, uint32_t n, int thr, const DenVertex &v, DenState *st, uint32_t level, hipStream_t s) {
    const uint32_t n_chunks = D.E.chunk_start[D.E.n_runs];
    if (n_chunks == 0) return hipSuccess;
    hipLaunchKernelGGL(k_den_link, dim3(chunk_grid("k_den_link", n_chunks)), dim3(256), 0, s, D, n, thr, v.state, v.parent, v.key, st, level);
    return hipGetLastError();
}

hipError_t launch_den_labels(uint32_t n, const DenVertex &v, uint32_t *cluster_row, uint32_t *anchor_row, uint32_t *degree_row, DenState *st,
                             uint32_t level, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_den_labels, dim3(vertex_grid("k_den_labels", n)), dim3(256), 0, s, n, v, cluster_row, anchor_row, degree_row, st, level);
    return hipGetLastError();
}

hipError_t launch_den_sizes(uint32_t n, const DenVertex &v, DenState *st, uint32_t level, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_den_sizes, dim3(vertex_grid("k_den_sizes", n)), dim3(256), 0, s, n, v, st, level);
    return hipGetLastError();
}

}  // namespace hmk
