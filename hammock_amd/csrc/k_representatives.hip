// k_representatives.hip -- the representatives of the neighbour graph {score >= t}: i is one iff no representative r < i is its
// neighbour, i.e. the lexicographically first maximal independent set, decided in synchronous rounds (hmk_representatives_shifted,
// hmk_representatives_from_edges_dev; hmk_representatives.cpp).  Every vertex is UNDECIDED, REP or REDUNDANT; round r = 1, 2, ... is
//   k_rep_mark*     over the live edges {lo < hi}, reading state[] only: lo REP and hi UNDECIDED -> stamp 2r + 1 on hi, edge dropped;
//                   both UNDECIDED -> stamp 2r on hi, edge kept (appended to the other live buffer: a ballot per wave, one returning
//                   atomic per chunk of 1,024 edges); anything else -> edge dropped.  A stamp goes into mark[hi] with lo behind it,
//                   stamp << 32 | (0xFFFFFFFF - lo), by one 64-bit atomicMax: the highest stamp, and under stamp 2r the smallest
//                   undecided smaller neighbour.  Rounds 1 and 2 (k_rep_mark_first) read the level's edges where they lie and test
//                   them -- in round 1 every vertex is undecided, so every edge stays live and nothing is appended, round 2 reads the
//                   same edges again and appends the first live list (round 1 also notes every edge's smaller end in touched[]:
//                   with mark != 0, the larger end of an edge, that is every vertex that has a neighbour); later rounds read the
//                   live buffer, whose length stays on the device
//   k_rep_decide    over the vertices: UNDECIDED with stamp 2r + 1 -> REDUNDANT; with anything below 2r -> REP (all its smaller
//                   neighbours are redundant); with 2r -> REDUNDANT if the neighbour u that mark[] names has a stamp below 2r itself
//                   (u was undecided when the marking kernel ran and becomes REP in this very launch), else it stays.  Counts those
//                   that stay, and the last workgroup stores round << 32 | undecided where the host polls it
// and behind the rounds
//   k_rep_assign    over all edges of the level: for a REP a next to a REDUNDANT b, atomicMin(covered_by[b], a) and a 64-bit
//                   atomicMax(key[b], (score + 32768) << 32 | (0xFFFFFFFF - a)): the largest score, among equals the smaller index
//   k_rep_finish    nearest, nearest_score from the keys, the representatives' own entries, the level's counts.
// A marking kernel decides by state[] alone, written by the decision kernel before it, and writes mark[] and the other live buffer
// (its one look at mark[] only spares atomics that would change nothing: rep_step); a decision kernel reads mark[], which nothing
// in it writes, and each lane writes only its own vertex's state, which no other lane reads.  A decision is made only once it is
// forced, so the state after every round is a function of the graph alone: the same result, and the same number of rounds, on
// every grid and schedule.  The look at u decides more per round than the plain scheme (stamp 2r: stay) and never less, so no
// level takes more rounds than that scheme; an ascending path takes half.
// mark[], covered_by[] and key[] only take agent-scope atomic maxima and minima inside a launch and are read by plain loads in the
// next one.
// An edge is tested (x < n, m < n, x != m) before anything is indexed with it.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "hmk_representatives.h"
#include "hmk_grid.h"

namespace hmk {

namespace {

__device__ __forceinline__ uint32_t rep_wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// a word that atomics of this launch write, as whatever cache holds it has it: a relaxed load at wavefront scope is a plain load
template <class T> __device__ __forceinline__ T rep_look(const T *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }

// the run that holds chunk c (workgroup-uniform)
__device__ __forceinline__ uint32_t rep_run_of(const EdgeRuns &E, uint32_t c) {
    uint32_t lo = 0, hi = E.n_runs;   // chunk_start[lo] <= c < chunk_start[hi]
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (E.chunk_start[mid] <= c) lo = mid;
        else hi = mid;
    }
    return lo;
}

// entry j of the lane in chunk c: true = an edge of this level, x != m both below n, score >= thr.  An invalid one raises *bad, if given.
__device__ __forceinline__ bool rep_edge(const EdgeRuns &E, uint32_t run, uint32_t c, int j, uint32_t n, int thr, uint32_t *bad, uint32_t &x,
                                         uint32_t &m, int &score) {
    const unsigned long long k = (unsigned long long)(c - E.chunk_start[run]) * REP_CHUNK + (unsigned)j * 256u + threadIdx.x;
    if (k >= E.count[run]) return false;
    const uint64_t w = E.base[(unsigned long long)run * E.stride + k];
    x = HMK_EDGE_X(w);
    m = HMK_EDGE_M(w);
    if (x >= n || m >= n || x == m) {
        if (bad) atomicOr(bad, 1u);
        return false;
    }
    score = HMK_EDGE_SCORE(w);
    return score >= thr;
}

// What round `round` does with the edge {lo < hi}; true: it stays live.
__device__ __forceinline__ bool rep_step(const uint8_t *__restrict__ state, unsigned long long *mark, uint32_t round, uint32_t lo, uint32_t hi) {
    if (state[hi] != REP_UNDECIDED) return false;
    const uint8_t sl = state[lo];
    if (sl == REP_REDUNDANT) return false;
    // A plain look before the atomic: mark[hi] only ever rises, so a word seen at or above this edge's value -- however old the copy a
    // cache hands out -- means the atomic would change nothing; a stale smaller word costs an atomic, never the result.  A vertex
    // with d smaller neighbours takes about ln d atomics per round instead of d.
    const unsigned long long mine = (unsigned long long)(2u * round + (sl == REP_REP ? 1u : 0u)) << 32 | (0xFFFFFFFFu - lo);
    if (rep_look(mark + hi) < mine) atomicMax(mark + hi, mine);
    return sl == REP_UNDECIDED;
}

// The chunk's kept edges behind *cursor: the lane's rank by one ballot per entry, the waves' totals in LDS, one returning atomic
// per chunk.  Every lane of the workgroup calls it.
__device__ __forceinline__ void rep_append(const bool keep[4], const uint64_t w[4], unsigned long long *cursor, uint64_t *__restrict__ out,
                                           uint64_t cap, uint32_t *wave_tot, unsigned long long *chunk_base) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t rank[4], tot = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const unsigned long long b = __ballot(keep[j]);
        rank[j] = tot + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
        tot += (uint32_t)__popcll(b);
    }
    if (lane == 0) wave_tot[wave] = tot;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t all = wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
        *chunk_base = all ? atomicAdd(cursor, (unsigned long long)all) : 0ull;
    }
    __syncthreads();
    unsigned long long at = *chunk_base;
    for (uint32_t k = 0; k < wave; k++) at += wave_tot[k];
#pragma unroll
    for (int j = 0; j < 4; j++)
        if (keep[j] && at + rank[j] < cap) out[at + rank[j]] = w[j];   // (never more kept than read: cap is the level's edge count)
    __syncthreads();
}

}  // namespace

__global__ void __launch_bounds__(256) k_rep_init(const RepVertex v, uint32_t n) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256) {
        v.key[i] = 0ull;
        v.mark[i] = 0ull;
        v.covered_by[i] = 0xFFFFFFFFu;
        v.state[i] = REP_UNDECIDED;
        v.touched[i] = 0;
    }
}

__global__ void __launch_bounds__(256) k_rep_mark_first(uint32_t round, const EdgeRuns E, uint32_t n, int thr, const RepVertex v, RepState *st,
                                                        uint64_t *__restrict__ live0, uint64_t cap) {
    __shared__ uint32_t wave_tot[4];
    __shared__ unsigned long long chunk_base;
    const uint32_t n_chunks = E.chunk_start[E.n_runs];
    uint32_t edges = 0;
    for (uint32_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {   // workgroup-uniform
        const uint32_t run = rep_run_of(E, c);
        bool keep[4];
        uint64_t w[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            uint32_t x = 0, m = 0;
            int score = 0;
            keep[j] = false;
            w[j] = 0;
            if (!rep_edge(E, run, c, j, n, thr, round == 1 ? &st->flag : nullptr, x, m, score)) continue;
            edges++;
            const uint32_t lo = min(x, m), hi = max(x, m);
            if (round == 1) {   // every vertex is undecided: no state to look up; the smaller end is noted as having a neighbour
                const unsigned long long mine = 2ull << 32 | (0xFFFFFFFFu - lo);
                if (rep_look(v.mark + hi) < mine) atomicMax(v.mark + hi, mine);
                if (!rep_look(v.touched + lo)) v.touched[lo] = 1;
                continue;
            }
            keep[j] = rep_step(v.state, v.mark, round, lo, hi);
            w[j] = (uint64_t)lo << 32 | hi;
        }
        if (round != 1) rep_append(keep, w, &st->live[0], live0, cap, wave_tot, &chunk_base);   // (round 1 keeps them all, where they are)
    }
    if (round != 1) return;
    edges = rep_wave_sum(edges);
    if ((threadIdx.x & 63) == 0 && edges) atomicAdd(&st->n_edges, (unsigned long long)edges);
}

__global__ void __launch_bounds__(256) k_rep_mark(uint32_t round, const RepVertex v, RepState *st, const uint64_t *__restrict__ live_in,
                                                  uint64_t *__restrict__ live_out, uint64_t cap) {
    __shared__ uint32_t wave_tot[4];
    __shared__ unsigned long long chunk_base;
    const unsigned long long len = min(st->live[(round - 1) & 1], (unsigned long long)cap);   // (nothing in this launch writes it)
    const unsigned long long n_chunks = (len + REP_CHUNK - 1) / REP_CHUNK;
    for (unsigned long long c = blockIdx.x; c < n_chunks; c += gridDim.x) {   // workgroup-uniform
        bool keep[4];
        uint64_t w[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const unsigned long long k = c * REP_CHUNK + (unsigned)j * 256u + threadIdx.x;
            keep[j] = false;
            w[j] = 0;
            if (k >= len) continue;
            w[j] = live_in[k];
            keep[j] = rep_step(v.state, v.mark, round, (uint32_t)(w[j] >> 32), (uint32_t)w[j]);
        }
        rep_append(keep, w, &st->live[round & 1], live_out, cap, wave_tot, &chunk_base);
    }
}

__global__ void __launch_bounds__(256) k_rep_decide(uint32_t round, uint32_t n, const RepVertex v, RepState *st, unsigned long long *host_word) {
    uint32_t left = 0;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256) {
        if (v.state[i] != REP_UNDECIDED) continue;
        const unsigned long long mk = v.mark[i];
        const uint32_t s = (uint32_t)(mk >> 32);
        if (s == 2u * round + 1u) v.state[i] = REP_REDUNDANT;
        else if (s == 2u * round) {
            const uint32_t u = 0xFFFFFFFFu - (uint32_t)mk;   // undecided when this round's marks were made, and below i
            if ((uint32_t)(v.mark[u] >> 32) < 2u * round) v.state[i] = REP_REDUNDANT;   // u becomes REP in this launch
            else left++;
        } else v.state[i] = REP_REP;
    }
    // the waves' counts through LDS, then ONE returning atomic per workgroup on one word that holds both the workgroups that are
    // through (the high half) and their count so far (n <= 2^24): the workgroup that finds all others there has the total, no fence
    __shared__ uint32_t wave_left[4];
    left = rep_wave_sum(left);
    if ((threadIdx.x & 63) == 0) wave_left[threadIdx.x >> 6] = left;
    __syncthreads();
    if (threadIdx.x != 0) return;
    const uint32_t mine = wave_left[0] + wave_left[1] + wave_left[2] + wave_left[3];
    const unsigned long long before = atomicAdd(&st->tally, 1ull << 32 | mine);
    if ((uint32_t)(before >> 32) != gridDim.x - 1) return;
    const uint32_t undecided = (uint32_t)before + mine;
    const unsigned long long live = round == 1 ? st->n_edges : st->live[round & 1];   // (the marking kernel's: a launch ago)
    atomicExch(&st->tally, 0ull);
    atomicExch(&st->live[(round + 1) & 1], 0ull);   // the next round appends there
    if (undecided == 0) atomicCAS(&st->rounds, 0u, round);
    if (round <= REP_TRACE) st->trace[round - 1] = live;
    if (host_word) {
        __hip_atomic_store(host_word + 1, live, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(host_word, ((unsigned long long)round << 32) | undecided, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

__global__ void __launch_bounds__(256) k_rep_assign(const EdgeRuns E, uint32_t n, int thr, const RepVertex v) {
    const uint32_t n_chunks = E.chunk_start[E.n_runs];
    for (uint32_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const uint32_t run = rep_run_of(E, c);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            uint32_t x = 0, m = 0;
            int score = 0;
            if (!rep_edge(E, run, c, j, n, thr, nullptr, x, m, score)) continue;   // (round 1 has flagged the invalid ones)
            const uint8_t sx = v.state[x], sm = v.state[m];
            uint32_t a, b;   // the representative and the redundant end
            if (sx == REP_REP && sm == REP_REDUNDANT) { a = x; b = m; }
            else if (sm == REP_REP && sx == REP_REDUNDANT) { a = m; b = x; }
            else continue;
            // (a plain look first, as in rep_step: the words only fall / only rise)
            const unsigned long long key = (unsigned long long)(uint32_t)(score + 32768) << 32 | (0xFFFFFFFFu - a);
            if (a < rep_look(v.covered_by + b)) atomicMin(v.covered_by + b, a);
            if (key > rep_look(v.key + b)) atomicMax(v.key + b, key);
        }
    }
}

__global__ void __launch_bounds__(256) k_rep_finish(uint32_t n, const RepVertex v, RepState *st) {
    uint32_t reps = 0, isolated = 0;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256) {
        isolated += v.touched[i] || v.mark[i] ? 0u : 1u;   // neither the smaller nor the larger end of any edge
        if (v.state[i] == REP_REDUNDANT) {
            const unsigned long long key = v.key[i];
            v.nearest[i] = 0xFFFFFFFFu - (uint32_t)key;
            v.nearest_score[i] = (int32_t)(uint32_t)(key >> 32) - 32768;
        } else {
            reps++;
            v.covered_by[i] = (uint32_t)i;
            v.nearest[i] = (uint32_t)i;
            v.nearest_score[i] = INT32_MAX;
        }
    }
    reps = rep_wave_sum(reps);
    isolated = rep_wave_sum(isolated);
    if ((threadIdx.x & 63) == 0) {
        if (reps) atomicAdd(&st->n_rep, reps);
        if (isolated) atomicAdd(&st->n_isolated, isolated);
    }
}

// -----------------------------------------------------------------------------
// launchers
// -----------------------------------------------------------------------------
namespace {
uint32_t vertex_grid(const char *kernel, uint32_t n) { return capped_grid(kernel, std::min<uint32_t>((n + 255) / 256, REP_MAX_GRID)); }
uint32_t chunk_grid(const char *kernel, const EdgeRuns &E) { return capped_grid(kernel, std::min<uint32_t>(E.chunk_start[E.n_runs], REP_MAX_GRID)); }
}  // namespace

hipError_t launch_rep_init(const RepVertex &v, uint32_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_rep_init, dim3(vertex_grid("k_rep_init", n)), dim3(256), 0, s, v, n);
    return hipGetLastError();
}

hipError_t launch_rep_mark_first(uint32_t round, const EdgeRuns &E, uint32_t n, int thr, const RepVertex &v, RepState *st, uint64_t *live0,
                                 uint64_t cap, hipStream_t s) {
    if (E.chunk_start[E.n_runs] == 0) return hipSuccess;
    hipLaunchKernelGGL(k_rep_mark_first, dim3(chunk_grid("k_rep_mark_first", E)), dim3(256), 0, s, round, E, n, thr, v, st, live0, cap);
    return hipGetLastError();
}

hipError_t launch_rep_mark(uint32_t round, uint64_t total_edges, const RepVertex &v, RepState *st, uint64_t *live0, uint64_t *live1, uint64_t cap,
                           hipStream_t s) {
    if (total_edges == 0) return hipSuccess;
    const uint32_t blocks = capped_grid("k_rep_mark", (uint32_t)std::min<uint64_t>((total_edges + REP_CHUNK - 1) / REP_CHUNK, REP_MAX_GRID));
    uint64_t *live[2] = {live0, live1};
    hipLaunchKernelGGL(k_rep_mark, dim3(blocks), dim3(256), 0, s, round, v, st, live[(round - 1) & 1], live[round & 1], cap);
    return hipGetLastError();
}

hipError_t launch_rep_decide(uint32_t round, uint32_t n, const RepVertex &v, RepState *st, unsigned long long *host_word, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_rep_decide, dim3(vertex_grid("k_rep_decide", n)), dim3(256), 0, s, round, n, v, st, host_word);
    return hipGetLastError();
}

hipError_t launch_rep_assign(const EdgeRuns &E, uint32_t n, int thr, const RepVertex &v, hipStream_t s) {
    if (E.chunk_start[E.n_runs] == 0) return hipSuccess;
    hipLaunchKernelGGL(k_rep_assign, dim3(chunk_grid("k_rep_assign", E)), dim3(256), 0, s, E, n, thr, v);
    return hipGetLastError();
}

hipError_t launch_rep_finish(uint32_t n, const RepVertex &v, RepState *st, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_rep_finish, dim3(vertex_grid("k_rep_finish", n)), dim3(256), 0, s, n, v, st);
    return hipGetLastError();
}

}  // namespace hmk
