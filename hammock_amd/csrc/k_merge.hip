// k_merge.hip -- the cluster-level graph of given clusters (hmk_merge.cpp), built from the sequence-level CSR of their members: for
// every cluster A the clusters B != A all of whose members are neighbours of all of A's (hits == |A| * |B|), with the minimum score
// -- ClinkageClusterScorer.clusterScore (ClinkageClusterScorer.java:30-49) for every pair of clusters at once.
// The run of cluster A is the concatenation of its members' CSR rows: its length is known from the row starts (k_merge_len + a scan),
// so nothing is counted or scattered.  One wave per cluster whose rows hold at most LONG_RUN entries, one workgroup per longer one;
// the rows are walked in place, neighbour -> slot through cluster_of[], the own slot skipped, (slot -> hits, minimum) aggregated in the
// LDS table of k_assign_table.h (its insert / clean / overflow classes; the fill here reads CSR entries instead of 64-bit records).
// A's feasible clusters land at A's run offset of a scratch buffer (a feasible cluster has a hit: they fit), their number in cnt[A];
// after a scan k_merge_compact stores the lists into the host's pinned block.
// Every store here is an ordinary vector store; the counters are vector atomics.
#include "hmk_device.h"
#include "k_assign_table.h"
#include "hmk_grid.h"

namespace hmk {

namespace {

constexpr uint32_t LONG_RUN = 4096;   // longer runs: a workgroup each

// row lengths in the order of the slots' member lists
__global__ void __launch_bounds__(256)
k_merge_len(const uint64_t *__restrict__ start, const uint32_t *__restrict__ cl_members, uint32_t nm, uint32_t *__restrict__ mlen) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < nm; i += gridDim.x * 256) {
        const uint32_t r = cl_members[i];
        mlen[i] = (uint32_t)(start[r + 1] - start[r]);
    }
}

struct Clusters {
    const uint64_t *start;        // CSR row starts, indexed by the sequence itself
    const void *adj;              // NbrPacked[] (m << 8 | score - thr) or Nbr[]
    const uint32_t *cl_start;     // [ncl + 1]
    const uint32_t *cl_members;   // [nm] absolute indices, slot by slot
    const uint32_t *cluster_of;   // [nm] slot of member r0 + i
    const uint32_t *mstart;       // [nm + 1] prefix sums of the row lengths in cl_members order
    uint32_t r0, nm;
    int thr;
    uint32_t upper_only;
};

// The run of cluster `own` (members cl_members[m0 .. m1), `len` entries in all) into the table, the neighbours whose slots fall into
// class `part` of `parts`; -> it did not fit.  The run is walked as ONE range of entries, a lane per entry: entry e lies in the row of
// the last member whose prefix sum mstart[] is <= e (a branch-free search of log2(members) steps, the same for every lane), so a
// cluster of many short rows costs what its entries cost, not a round of dependent loads per member; UNROLL entries per lane are in
// flight before the first one goes into the table.
template <bool PACKED, int LANES, int SLOTS>
__device__ __forceinline__ bool fill_rows(const RunTable<LANES, SLOTS> &T, const Clusters &C, uint32_t own, uint32_t m0, uint32_t m1, uint32_t len,
                                          uint32_t part, uint32_t parts, uint32_t lane) {
    constexpr int UNROLL = 4;
    bool full = false;
    const uint32_t base = C.mstart[m0];
    const uint32_t top = m1 - m0 > 1 ? 1u << (31 - __clz((int)(m1 - m0 - 1))) : 0;   // the search's first step: the largest power of two below the member count
    for (uint32_t e0 = 0; e0 < len; e0 += LANES * UNROLL) {   // (uniform)
        uint32_t e[UNROLL], pos[UNROLL], m[UNROLL], v[UNROLL];
        bool ok[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; u++) {
            e[u] = e0 + (uint32_t)u * LANES + lane;
            ok[u] = e[u] < len;
            if (!ok[u]) e[u] = 0;
            pos[u] = m0;
        }
        for (uint32_t step = top; step; step >>= 1) {   // (uniform)
#pragma unroll
            for (int u = 0; u < UNROLL; u++) {
                const uint32_t nx = pos[u] + step;
                if (nx < m1 && C.mstart[nx] - base <= e[u]) pos[u] = nx;
            }
        }
#pragma unroll
        for (int u = 0; u < UNROLL; u++) {
            const uint64_t q = C.start[C.cl_members[pos[u]]] + (e[u] - (C.mstart[pos[u]] - base));
            m[u] = 0xFFFFFFFFu;
            v[u] = 0;
            if (ok[u]) {
                if (PACKED) {
                    const uint32_t w = ((const uint32_t *)C.adj)[q];
                    m[u] = w >> 8;
                    v[u] = w & 0xFFu;
                } else {
                    const Nbr nb = ((const Nbr *)C.adj)[q];
                    m[u] = nb.m;
                    v[u] = (uint32_t)(nb.s - C.thr);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < UNROLL; u++) {
            if (m[u] - C.r0 >= C.nm) continue;   // (past the run's end; never otherwise: the pass is the triangle inside the range)
            const uint32_t c = C.cluster_of[m[u] - C.r0];
            if (c != own && (c & (parts - 1)) == part && !full) full = !T.insert((int32_t)c, v[u]);
        }
    }
    T.sync();
    return T.any(full) || *T.n_used > (uint32_t)SLOTS * 3 / 4;
}

// the whole run of cluster `own`: every feasible cluster to out[0 .. ) as slot << 32 | min (score - thr), their number to *n_feasible
// (room: the run's length); the class split of RunTable::run_all
template <bool PACKED, int LANES, int SLOTS>
__device__ __forceinline__ void run_cluster(const RunTable<LANES, SLOTS> &T, const Clusters &C, uint32_t own, uint32_t len, uint32_t lane,
                                            uint64_t *__restrict__ out, uint32_t *n_out, uint32_t *__restrict__ n_feasible) {
    const uint32_t m0 = C.cl_start[own], m1 = C.cl_start[own + 1];
    const uint64_t na = m1 - m0;
    for (uint32_t parts = 1; len > 0; parts *= 2) {
        if (lane == 0) *n_out = 0;
        T.sync();
        bool fits = true;
        for (uint32_t part = 0; part < parts && fits; part++) {
            fits = !fill_rows<PACKED>(T, C, own, m0, m1, len, part, parts, lane);
            if (fits) {
                const uint32_t nu = *T.n_used;
                for (uint32_t i = lane; i < nu; i += LANES) {
                    const uint32_t sl = T.used[i];
                    const uint32_t c = (uint32_t)T.keys[sl];
                    const uint64_t need = na * (uint64_t)(C.cl_start[c + 1] - C.cl_start[c]);   // (< 2^32: the host refuses larger products)
                    if ((uint64_t)T.hits[sl] == need && (!C.upper_only || c > own)) {
                        const uint32_t at = atomicAdd(n_out, 1u);
                        if (at < len) out[at] = ((uint64_t)c << 32) | T.mn[sl];
                    }
                }
            }
            T.clean(lane);   // (its barriers order the appends before the count is read)
        }
        if (fits) break;
    }
    if (lane == 0) *n_feasible = len ? min(*n_out, len) : 0;
}

// one wave per cluster whose run holds at most `long_run` entries (4 waves per workgroup, grid-stride); the longer runs are listed in
// long_list[0 .. *long_count) for k_merge_block
template <bool PACKED>
__global__ void __launch_bounds__(256)
k_merge_wave(Clusters C, uint32_t ncl, uint32_t long_run, const uint32_t *__restrict__ mstart, uint32_t *__restrict__ long_list,
             uint32_t *__restrict__ long_count, uint64_t *__restrict__ tmp, uint32_t *__restrict__ cnt) {
    __shared__ int32_t keys_all[4 * WAVE_SLOTS];
    __shared__ uint32_t hits_all[4 * WAVE_SLOTS];
    __shared__ uint32_t mn_all[4 * WAVE_SLOTS];
    __shared__ uint16_t used_all[4 * WAVE_SLOTS];
    __shared__ uint32_t n_used_all[4], n_out_all[4];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const RunTable<64, WAVE_SLOTS> T{keys_all + wv * WAVE_SLOTS, hits_all + wv * WAVE_SLOTS, mn_all + wv * WAVE_SLOTS,
                                     used_all + wv * WAVE_SLOTS, n_used_all + wv, nullptr};
    T.init(lane);
    for (uint32_t a = blockIdx.x * 4 + wv; a < ncl; a += gridDim.x * 4) {   // (wave-uniform)
        const uint32_t b = mstart[C.cl_start[a]], len = mstart[C.cl_start[a + 1]] - b;
        if (len > long_run) {
            if (lane == 0) long_list[atomicAdd(long_count, 1u)] = a;
            continue;
        }
        run_cluster<PACKED>(T, C, a, len, lane, tmp + b, n_out_all + wv, cnt + a);
    }
}

// one workgroup per listed long run (grid-stride over the list)
template <bool PACKED>
__global__ void __launch_bounds__(256)
k_merge_block(Clusters C, const uint32_t *__restrict__ mstart, const uint32_t *__restrict__ long_list, const uint32_t *__restrict__ long_count,
              uint64_t *__restrict__ tmp, uint32_t *__restrict__ cnt) {
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
        const uint32_t a = long_list[i];
        const uint32_t b = mstart[C.cl_start[a]], len = mstart[C.cl_start[a + 1]] - b;
        run_cluster<PACKED>(T, C, a, len, threadIdx.x, tmp + b, &n_out, cnt + a);
    }
}

// the lists to the host: a wave per cluster stores its records at ostart[a] of `out` (the host's pinned block by its device address) as
// a << 40 | b << 16 | score (HMK_EDGE_*)
__global__ void __launch_bounds__(256)
k_merge_compact(uint32_t ncl, const uint32_t *__restrict__ cl_start, const uint32_t *__restrict__ mstart, const uint64_t *__restrict__ tmp,
                const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ ostart, int thr, uint64_t *__restrict__ out, uint64_t out_capacity) {
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    for (uint32_t a = blockIdx.x * 4 + wv; a < ncl; a += gridDim.x * 4) {   // (wave-uniform)
        const uint32_t n = cnt[a];
        const uint64_t *src = tmp + mstart[cl_start[a]];
        const uint64_t dst = ostart[a];
        for (uint32_t i = lane; i < n; i += 64) {
            const uint64_t r = src[i];
            const int32_t score = (int32_t)(uint32_t)r + thr;
            if (dst + i < out_capacity)
                out[dst + i] = pack_edge(a, (uint32_t)(r >> 32), score);
        }
    }
}

// a wave per item, up to 8 workgroups per CU's worth (256 CUs), the rest grid-stride
uint32_t wave_grid(uint32_t n) {
    return std::max(1u, std::min((n + 3) / 4, 2048u));
}

}  // namespace

hipError_t launch_merge_graph(bool packed, const uint64_t *start, const void *adj, int thr, uint32_t r0, uint32_t nm, uint32_t ncl,
                              const uint32_t *cl_start, const uint32_t *cl_members, const uint32_t *cluster_of, bool upper_only, uint64_t entries,
                              uint32_t *mlen, uint32_t *mstart, uint64_t *tmp, uint32_t *cnt, uint32_t *ostart, uint32_t *scratch,
                              uint64_t *scan_scratch, hipStream_t s) {
    if (nm == 0 || ncl == 0) return hipSuccess;
    const Clusters C{start, adj, cl_start, cl_members, cluster_of, mstart, r0, nm, thr, upper_only ? 1u : 0u};
    uint32_t *long_count = scratch, *long_list = scratch + 1;
    hipError_t e = hipMemsetAsync(long_count, 0, sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    const uint32_t len_grid = capped_grid("k_merge_len", std::max(1u, std::min((nm + 255) / 256, 1024u)));
    hipLaunchKernelGGL(k_merge_len, dim3(len_grid), dim3(256), 0, s, start, cl_members, nm, mlen);
    e = launch_scan_u32(mlen, mstart, nm, scan_scratch, s);
    if (e != hipSuccess) return e;
    // at most entries / (LONG_RUN + 1) runs can be long: no workgroups for runs that cannot exist
    uint32_t n_block = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(ncl, entries / (LONG_RUN + 1)), 1024);
    const uint32_t n_wave = capped_grid(packed ? "k_merge_wave<true>" : "k_merge_wave<false>", wave_grid(ncl));
    if (n_block) n_block = capped_grid(packed ? "k_merge_block<true>" : "k_merge_block<false>", n_block);
    if (packed) {
        hipLaunchKernelGGL(k_merge_wave<true>, dim3(n_wave), dim3(256), 0, s, C, ncl, LONG_RUN, mstart, long_list, long_count, tmp, cnt);
        if (n_block) hipLaunchKernelGGL(k_merge_block<true>, dim3(n_block), dim3(256), 0, s, C, mstart, long_list, long_count, tmp, cnt);
    } else {
        hipLaunchKernelGGL(k_merge_wave<false>, dim3(n_wave), dim3(256), 0, s, C, ncl, LONG_RUN, mstart, long_list, long_count, tmp, cnt);
        if (n_block) hipLaunchKernelGGL(k_merge_block<false>, dim3(n_block), dim3(256), 0, s, C, mstart, long_list, long_count, tmp, cnt);
    }
    return launch_scan_u32(cnt, ostart, ncl, scan_scratch, s);
}

hipError_t launch_merge_compact(uint32_t ncl, const uint32_t *cl_start, const uint32_t *mstart, const uint64_t *tmp, const uint32_t *cnt,
                                const uint32_t *ostart, int thr, uint64_t *out, uint64_t out_capacity, hipStream_t s) {
    if (ncl == 0) return hipSuccess;
    const uint32_t grid = capped_grid("k_merge_compact", wave_grid(ncl));
    hipLaunchKernelGGL(k_merge_compact, dim3(grid), dim3(256), 0, s, ncl, cl_start, mstart, tmp, cnt, ostart, thr, out, out_capacity);
    return hipGetLastError();
}

}  // namespace hmk
