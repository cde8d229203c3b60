// k_orders.hip -- what hmk_greedy_orders runs behind its ONE neighbour pass (hmk_orders.cpp): the greedy clustering is asked for
// under many orders of the set, the scores do not depend on the order, so the pass's packed edges are renamed per order and the
// clustering tail takes them as they are.
//   k_orders_relabel   per order: every edge (x, m, score) as (min(pos[x], pos[m]), max(...), score), pos = the order's inverse
//                      permutation.  8 bytes in, 8 bytes out, two 4-byte gathers from a table of 4 n bytes (0.4 MB at 10^5, L2-resident;
//                      4 MB at 10^6: it fits one XCD's L2 of 4 MB only just, beside the streams -- the gathers then hit the 256 MB
//                      MALL).  The 16 score bits are copied, not re-derived: a negative score stays what it was.
//   k_orders_support   once, behind the last tail: one pass over the ORIGINAL edges with the valid orders' cluster ids transposed,
//                      ids[n][n_valid] -- an edge costs two contiguous gathers of n_valid ids.  With complete linkage every pair inside
//                      a cluster is an edge, so the support of a pair (the valid orders in which it shares a cluster) lives on the
//                      edge list.  Every output is an integer sum: independent of schedule and grid.
//                        the support edge   wave-aggregated room-taking: one returning atomic per wave and step
//                        per-order sums     counted in LDS per workgroup, then one 64-bit atomic per counter and workgroup
//                        partner counts     fire-and-forget 32-bit adds per row (only edges with support: the pairs inside clusters)
// An edge is tested (x < n, m < n, x != m) before anything is indexed with it.  Plain HIP C++, vector stores only.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "hmk_orders.h"
#include "hmk_grid.h"

namespace hmk {

namespace {

// the run that holds chunk c (workgroup-uniform)
__device__ __forceinline__ uint32_t orders_run_of(const EdgeRuns &E, uint32_t c) {
    uint32_t lo = 0, hi = E.n_runs;   // chunk_start[lo] <= c < chunk_start[hi]
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (E.chunk_start[mid] <= c) lo = mid;
        else hi = mid;
    }
    return lo;
}

// entry j of the lane in chunk c: its place k in the run (false: past the run's end) and the edge as stored
__device__ __forceinline__ bool orders_edge(const EdgeRuns &E, uint32_t run, uint32_t c, int j, unsigned long long &k, uint64_t &w) {
    k = (unsigned long long)(c - E.chunk_start[run]) * EDGE_RUN_CHUNK + (unsigned)j * 256u + threadIdx.x;
    if (k >= E.count[run]) return false;
    w = E.base[(unsigned long long)run * E.stride + k];
    return true;
}

}  // namespace

__global__ void __launch_bounds__(256) k_orders_relabel(const EdgeRuns E, const OrderRuns R, uint32_t n, const uint32_t *__restrict__ pos,
                                                        uint64_t *__restrict__ out, OrdersState *__restrict__ st) {
    const uint32_t n_chunks = E.chunk_start[E.n_runs];
    for (uint32_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const uint32_t run = orders_run_of(E, c);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            unsigned long long k;
            uint64_t w;
            if (!orders_edge(E, run, c, j, k, w)) continue;
            const uint32_t x = HMK_EDGE_X(w), m = HMK_EDGE_M(w);
            if (x >= n || m >= n || x == m) {   // (never from a pass: the place keeps the edge as it is, the host refuses the call)
                atomicOr(&st->flag, 1ull);
                out[R.off[run] + k] = w;
                continue;
            }
            const uint32_t a = pos[x], b = pos[m];
            out[R.off[run] + k] = (uint64_t)min(a, b) << 40 | (uint64_t)max(a, b) << 16 | (w & 0xFFFFull);
        }
    }
}

__global__ void __launch_bounds__(256) k_orders_support(const EdgeRuns E, uint32_t n, const int32_t *__restrict__ ids, uint32_t nv,
                                                        uint64_t *__restrict__ out, unsigned long long cap, uint32_t *__restrict__ ever,
                                                        uint32_t *__restrict__ always, OrdersState *__restrict__ st) {
    __shared__ uint32_t tog[ORDERS_MAX], first[ORDERS_MAX];
    tog[threadIdx.x] = 0;
    first[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t n_chunks = E.chunk_start[E.n_runs];
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t n_always = 0;
    uint32_t in_lds = 0;   // chunks counted since the last flush (workgroup-uniform)
    for (uint32_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const uint32_t run = orders_run_of(E, c);
#pragma unroll 1
        for (int j = 0; j < 4; j++) {
            unsigned long long k;
            uint64_t w = 0;
            uint32_t x = 0, m = 0, sup = 0;
            if (orders_edge(E, run, c, j, k, w)) {
                x = HMK_EDGE_X(w);
                m = HMK_EDGE_M(w);
                if (x >= n || m >= n || x == m) {
                    atomicOr(&st->flag, 1ull);
                } else {
                    const int32_t *rx = ids + (size_t)x * nv, *rm = ids + (size_t)m * nv;
                    const bool eq0 = rx[0] == rm[0];
                    for (uint32_t v = 0; v < nv; v++) {
                        if (rx[v] != rm[v]) continue;
                        sup++;
                        atomicAdd(&tog[v], 1u);
                        if (eq0) atomicAdd(&first[v], 1u);
                    }
                }
            }
            // room for the wave's support edges: one returning atomic by its first lane that has one
            const unsigned long long has = __ballot(sup > 0);
            if (has) {
                const uint32_t lead = (uint32_t)__ffsll((long long)has) - 1u;
                unsigned long long base = 0;
                if (lane == lead) base = atomicAdd(&st->n_support, (unsigned long long)__popcll(has));
                const uint32_t b_lo = __shfl((uint32_t)base, (int)lead), b_hi = __shfl((uint32_t)(base >> 32), (int)lead);
                if (sup > 0) {
                    const unsigned long long at = ((unsigned long long)b_hi << 32 | b_lo) + (unsigned long long)__popcll(has & ((1ull << lane) - 1ull));
                    if (out && at < cap) out[at] = (uint64_t)min(x, m) << 40 | (uint64_t)max(x, m) << 16 | (uint64_t)sup;
                    atomicAdd(ever + x, 1u);
                    atomicAdd(ever + m, 1u);
                    if (sup == nv) {
                        atomicAdd(always + x, 1u);
                        atomicAdd(always + m, 1u);
                        n_always++;
                    }
                }
            }
        }
        if (++in_lds == ORDERS_FLUSH_CHUNKS) {   // (only a launch capped to very few workgroups over 10^9 edges gets here)
            __syncthreads();
            if (tog[threadIdx.x]) atomicAdd(&st->together[threadIdx.x], (unsigned long long)tog[threadIdx.x]);
            if (first[threadIdx.x]) atomicAdd(&st->with_first[threadIdx.x], (unsigned long long)first[threadIdx.x]);
            tog[threadIdx.x] = 0;
            first[threadIdx.x] = 0;
            in_lds = 0;
            __syncthreads();
        }
    }
    __syncthreads();
    if (tog[threadIdx.x]) atomicAdd(&st->together[threadIdx.x], (unsigned long long)tog[threadIdx.x]);
    if (first[threadIdx.x]) atomicAdd(&st->with_first[threadIdx.x], (unsigned long long)first[threadIdx.x]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n_always += __shfl_xor(n_always, o);
    if (lane == 0 && n_always) atomicAdd(&st->n_always, (unsigned long long)n_always);
}

// -----------------------------------------------------------------------------
// launchers
// -----------------------------------------------------------------------------
namespace {
uint32_t orders_grid(const char *kernel, const EdgeRuns &E) { return capped_grid(kernel, std::min<uint32_t>(E.chunk_start[E.n_runs], ORDERS_MAX_GRID)); }
}  // namespace

hipError_t launch_orders_relabel(const EdgeRuns &E, const OrderRuns &R, uint32_t n, const uint32_t *pos, uint64_t *out, OrdersState *st,
                                 hipStream_t s) {
    if (E.chunk_start[E.n_runs] == 0) return hipSuccess;
    hipLaunchKernelGGL(k_orders_relabel, dim3(orders_grid("k_orders_relabel", E)), dim3(256), 0, s, E, R, n, pos, out, st);
    return hipGetLastError();
}

hipError_t launch_orders_support(const EdgeRuns &E, uint32_t n, const int32_t *ids, uint32_t n_valid, uint64_t *out, unsigned long long cap,
                                 uint32_t *ever, uint32_t *always, OrdersState *st, hipStream_t s) {
    if (E.chunk_start[E.n_runs] == 0 || n_valid == 0) return hipSuccess;
    hipLaunchKernelGGL(k_orders_support, dim3(orders_grid("k_orders_support", E)), dim3(256), 0, s, E, n, ids, n_valid, out, cap, ever, always, st);
    return hipGetLastError();
}

}  // namespace hmk
