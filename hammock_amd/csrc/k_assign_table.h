// k_assign_table.h -- the LDS aggregation of one run of (cluster rank << 32 | score + 32768) records, shared by the assignment
// (k_assign.hip) and the cluster match (k_match.hip).  Per cluster rank: hits and minimum score in an open-addressing table, a
// rank feasible when its hits equal what `need[rank]` asks (the assignment: the cluster's member count; the match's second
// level: the query cluster's member count, the same for every rank).  Keys: (min score + 32768) << 32 | (0xFFFFFFFF - rank),
// larger = better, never 0.  Every store is an ordinary vector store; the counters are vector atomics.
#ifndef HMK_K_ASSIGN_TABLE_H
#define HMK_K_ASSIGN_TABLE_H
#include "hmk_device.h"

namespace hmk {

// a `need` that is the same for every rank (the match's second level)
struct UniformNeed {
    uint32_t v;
    __device__ __forceinline__ uint32_t operator[](uint32_t) const { return v; }
};

// The per-run work of one run, shared by a wave (LANES = 64) and a workgroup (LANES = 256).
// The table (SLOTS entries: rank, hits, minimum; the occupied slots listed in `used`) is empty on entry and on exit.
// A run whose clusters do not fit the table (more than 3/4 of SLOTS distinct, or probing found no free slot) is walked again
// with its clusters split into `parts` classes, rank mod parts, one table fill per class; parts doubles until every class
// fits (it must once parts * SLOTS * 3/4 exceeds the number of clusters).  The best k of all classes are kept in registers:
// lane t < k holds the t-th best key so far, and every class's selection runs over its feasible keys and those k.
template <int LANES, int SLOTS>
struct RunTable {
    int32_t *keys;
    uint32_t *hits;
    uint32_t *mn;
    uint16_t *used;
    uint32_t *n_used;
    uint64_t *red;   // LANES / 64 words (workgroup only)

    static constexpr int PER = SLOTS / LANES;   // occupied slots a lane harvests
    static constexpr int UNROLL = 4;            // run records in flight per lane
    static constexpr uint32_t HASH_SHIFT = SLOTS == 2048 ? 21 : SLOTS == 1024 ? 22 : SLOTS == 512 ? 23 : 24;
    static_assert(SLOTS == 2048 || SLOTS == 1024 || SLOTS == 512 || SLOTS == 256, "table sizes");
    static_assert(SLOTS % LANES == 0 && LANES >= 32, "a lane per best-k entry (k <= 32)");

    __device__ __forceinline__ void sync() const {
        if (LANES > 64) __syncthreads();
        else __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    }

    __device__ __forceinline__ bool any(bool v) const {
        if (LANES > 64) return __syncthreads_or(v) != 0;
        return __ballot(v) != 0;
    }

    __device__ __forceinline__ uint64_t max_u64(uint64_t v, uint32_t lane) const {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const uint64_t w = __shfl_xor(v, o, 64);
            v = w > v ? w : v;
        }
        if (LANES > 64) {
            __syncthreads();   // the previous reduction's reads of red[] are done
            if ((lane & 63u) == 0) red[lane >> 6] = v;
            __syncthreads();
            v = 0;
#pragma unroll
            for (int w = 0; w < LANES / 64; w++) v = red[w] > v ? red[w] : v;
        }
        return v;
    }

    __device__ __forceinline__ uint32_t sum_u32(uint32_t v, uint32_t lane) const {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
        if (LANES > 64) {
            __syncthreads();
            if ((lane & 63u) == 0) red[lane >> 6] = v;
            __syncthreads();
            v = 0;
#pragma unroll
            for (int w = 0; w < LANES / 64; w++) v += (uint32_t)red[w];
        }
        return v;
    }

    __device__ __forceinline__ void init(uint32_t lane) const {
        for (uint32_t sl = lane; sl < (uint32_t)SLOTS; sl += LANES) { keys[sl] = -1; hits[sl] = 0; mn[sl] = 0xFFFFFFFFu; }
        if (lane == 0) *n_used = 0;
        sync();
    }

    __device__ __forceinline__ void clean(uint32_t lane) const {
        const uint32_t nu = *n_used;
        for (uint32_t i = lane; i < nu; i += LANES) { const uint32_t sl = used[i]; keys[sl] = -1; hits[sl] = 0; mn[sl] = 0xFFFFFFFFu; }
        sync();   // (every lane has read n_used)
        if (lane == 0) *n_used = 0;
        sync();
    }

    // -> false: probing found no free slot
    __device__ __forceinline__ bool insert(int32_t c, uint32_t score) const {
        uint32_t sl = ((uint32_t)c * 2654435761u) >> HASH_SHIFT;
        for (int probes = 0; probes < SLOTS; probes++) {
            const int32_t old = atomicCAS(&keys[sl], -1, c);
            if (old == -1) used[atomicAdd(n_used, 1u)] = (uint16_t)sl;   // (at most SLOTS slots can be taken)
            if (old == -1 || old == c) {
                atomicAdd(&hits[sl], 1u);
                atomicMin(&mn[sl], score);
                return true;
            }
            sl = (sl + 1) & (SLOTS - 1);
        }
        return false;
    }

    // the run's records whose rank falls into class `part` of `parts` into the table; -> it did not fit
    __device__ __forceinline__ bool fill(const uint64_t *__restrict__ run, uint32_t len, uint32_t part, uint32_t parts, uint32_t lane) const {
        bool full = false;
        for (uint32_t i0 = 0; i0 < len; i0 += LANES * UNROLL) {   // uniform
            uint64_t r[UNROLL];
#pragma unroll
            for (int u = 0; u < UNROLL; u++) {
                const uint32_t i = i0 + (uint32_t)u * LANES + lane;
                r[u] = i < len ? run[i] : ~0ull;
            }
#pragma unroll
            for (int u = 0; u < UNROLL; u++) {
                const uint32_t c = (uint32_t)(r[u] >> 32);
                if (r[u] != ~0ull && (c & (parts - 1)) == part && !full) full = !insert((int32_t)c, (uint32_t)r[u]);
            }
        }
        sync();
        return any(full) || *n_used > (uint32_t)SLOTS * 3 / 4;
    }

    // the table's feasible clusters (hits == need[rank]) merged into the best k held by lanes 0..k-1; -> how many were feasible
    template <class Need>
    __device__ __forceinline__ uint32_t harvest(Need members_of_rank, uint32_t k, uint32_t lane, uint64_t &best) const {
        const uint32_t nu = *n_used;
        uint64_t key[PER];
        uint32_t n_ok = 0;
#pragma unroll
        for (int j = 0; j < PER; j++) {
            const uint32_t i = (uint32_t)j * LANES + lane;
            key[j] = 0;
            if (i < nu) {
                const uint32_t sl = used[i];
                const uint32_t c = (uint32_t)keys[sl];
                if (hits[sl] == members_of_rank[c]) {
                    key[j] = ((uint64_t)mn[sl] << 32) | (uint64_t)(0xFFFFFFFFu - c);
                    n_ok++;
                }
            }
        }
        n_ok = sum_u32(n_ok, lane);
        if (n_ok == 0) return 0;   // (uniform)
        // round t takes the largest key below round t - 1's among this class's keys and the best k so far
        const uint64_t held = lane < k ? best : 0;
        uint64_t prev = ~0ull, mine = 0;
        for (uint32_t t = 0; t < k; t++) {
            uint64_t cand = held < prev ? held : 0;
#pragma unroll
            for (int j = 0; j < PER; j++)
                if (key[j] < prev && key[j] > cand) cand = key[j];
            cand = max_u64(cand, lane);
            if (cand == 0) break;   // (uniform)
            if (lane == t) mine = cand;
            prev = cand;
        }
        best = mine;
        return n_ok;
    }

    // the whole run; lanes 0..k-1 write its row of the outputs
    template <class Need>
    __device__ __forceinline__ void run(const uint64_t *__restrict__ rec, uint32_t len, Need members_of_rank,
                                        const uint32_t *__restrict__ slot_of_rank, uint32_t k, uint32_t lane,
                                        uint32_t *__restrict__ best_cluster, int32_t *__restrict__ best_score, uint32_t *__restrict__ n_feasible) const {
        uint64_t best = 0;
        uint32_t feasible = 0;
        for (uint32_t parts = 1; len > 0; parts *= 2) {
            best = 0;
            feasible = 0;
            bool fits = true;
            for (uint32_t part = 0; part < parts && fits; part++) {
                fits = !fill(rec, len, part, parts, lane);
                if (fits) feasible += harvest(members_of_rank, k, lane, best);
                clean(lane);
            }
            if (fits) break;
        }
        if (lane < k) {
            best_cluster[lane] = best ? slot_of_rank[0xFFFFFFFFu - (uint32_t)best] : 0xFFFFFFFFu;
            best_score[lane] = best ? (int32_t)(best >> 32) - 32768 : INT32_MIN;
        }
        if (lane == 0) *n_feasible = feasible;
    }

    // every feasible cluster of the table (hits == need[rank]) appended to out[*n_out ..] as rank << 32 | min score + 32768
    // (n_out: an LDS counter; order arbitrary)
    template <class Need>
    __device__ __forceinline__ void harvest_all(Need need, uint64_t *__restrict__ out, uint32_t *n_out, uint32_t lane) const {
        const uint32_t nu = *n_used;
        for (uint32_t i = lane; i < nu; i += LANES) {
            const uint32_t sl = used[i];
            const uint32_t c = (uint32_t)keys[sl];
            if (hits[sl] == need[c]) out[atomicAdd(n_out, 1u)] = ((uint64_t)c << 32) | mn[sl];
        }
    }

    // the whole run, every feasible cluster written to out[0 ..) (at most len records: a feasible cluster has a hit) and
    // their number to *n_feasible; the class split as run's, a restart overwrites what the classes before it wrote
    template <class Need>
    __device__ __forceinline__ void run_all(const uint64_t *__restrict__ rec, uint32_t len, Need need, uint32_t lane, uint64_t *__restrict__ out,
                                            uint32_t *n_out, uint32_t *__restrict__ n_feasible) const {
        for (uint32_t parts = 1; len > 0; parts *= 2) {
            if (lane == 0) *n_out = 0;
            sync();
            bool fits = true;
            for (uint32_t part = 0; part < parts && fits; part++) {
                fits = !fill(rec, len, part, parts, lane);
                if (fits) harvest_all(need, out, n_out, lane);
                clean(lane);   // (its barriers order the appends before the count is read)
            }
            if (fits) break;
        }
        if (lane == 0) *n_feasible = len ? *n_out : 0;
    }
};

constexpr int WAVE_SLOTS = 512, BLOCK_SLOTS = 2048;   // a wave's table (4 per workgroup), a workgroup's

}  // namespace hmk
#endif
