// k_linkage.hip -- complete-linkage scores INSIDE given clusters (hmk_cluster_linkage_shifted, hmk_linkage.cpp): per slot the
// minimum ShiftedScorer score over the unordered pairs of its members (ClinkageClusterScorer.java:30-49 without the early exit,
// applied inside one cluster), the pair that attains it, the number of pairs below the threshold; per member its own minimum
// and count.  The pair space is block-diagonal, sum of s (s - 1) / 2 over the slots, and nothing proportional to it is stored:
//   k_linkage_flat    slots of up to LINK_FLAT_MAX members: the pairs of all of them enumerated flat, one pair per lane, slot and
//                     pair decoded from the prefix sums of s (s - 1) / 2
//   k_linkage_tiled   larger slots: LINK_TILE x LINK_TILE tiles of the triangle of the slot's member list, on or below the
//                     diagonal only; a tile's rows in LDS, one column per lane
// Both run the literal scorer (shifted_score_literal, hmk_device.h) with seq1 = the pair's larger index, as the edges of
// hmk_neighbors_shifted are oriented.  A slot's minimum and its tie rule (smallest a, then smallest b, a < b) are one 64-bit
// atomicMin of (score + 32768) << 48 | a << 24 | b: reduced in the wave first, one atomic per wave and slot segment.
#include <algorithm>

#include "hmk_link_device.h"
#include "hmk_grid.h"

namespace hmk {

namespace {

__device__ __forceinline__ uint64_t link_key(int score, uint32_t a, uint32_t b) {
    return ((uint64_t)(uint32_t)(score + 32768) << 48) | ((uint64_t)a << 24) | (uint64_t)b;
}

__device__ __forceinline__ uint64_t shfl_up_u64(uint64_t v, int d) {
    const uint32_t lo = __shfl_up((uint32_t)v, d), hi = __shfl_up((uint32_t)(v >> 32), d);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int d) {
    const uint32_t lo = __shfl_xor((uint32_t)v, d), hi = __shfl_xor((uint32_t)(v >> 32), d);
    return ((uint64_t)hi << 32) | lo;
}

}  // namespace

// -----------------------------------------------------------------------------
// accumulators: one launch per call, on the call's stream
// -----------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_linkage_init(uint64_t *__restrict__ key, unsigned long long *__restrict__ below, uint32_t n_clusters, int32_t *__restrict__ member_min,
               uint32_t *__restrict__ member_below, uint32_t nm) {
    const uint32_t n = max(n_clusters, member_min ? nm : 0u);
    for (uint32_t k = blockIdx.x * 256 + threadIdx.x; k < n; k += gridDim.x * 256) {
        if (k < n_clusters) { key[k] = ~0ull; below[k] = 0; }
        if (member_min && k < nm) { member_min[k] = INT32_MAX; member_below[k] = 0; }
    }
}

// -----------------------------------------------------------------------------
// small slots: a lane per pair
// -----------------------------------------------------------------------------
// Flat slot f = slot fslot[f] with the members tab[fmstart[f] .. fmstart[f + 1]) (indices of the uploaded set, ascending) and the
// pairs fpstart[f] .. fpstart[f + 1) of the flat pair space.  A block takes chunks of 256 consecutive pairs: the lanes of a wave
// hold a few consecutive slots, so the slot side is a segmented scan over the wave (one atomic per wave and slot segment); the
// member side goes through LDS counters indexed by the member's place behind the chunk's first slot (a chunk of 256 pairs spans
// at most 2 * 256 + 2 * LINK_FLAT_MAX members: a whole slot of s members has at least s / 2 pairs), one atomic per touched member.
constexpr int LINK_MEMB = 2 * 256 + 2 * LINK_FLAT_MAX;

__global__ void __launch_bounds__(256)
k_linkage_flat(const uint8_t *__restrict__ res32, const uint8_t *__restrict__ len, const int32_t *__restrict__ Mg,
               const uint32_t *__restrict__ tab, const uint32_t *__restrict__ fslot, const uint32_t *__restrict__ fmstart,
               const unsigned long long *__restrict__ fpstart, uint32_t nf, unsigned long long n_pairs, uint32_t r0, int X, int p, int thr,
               uint64_t *__restrict__ key, unsigned long long *__restrict__ below, int32_t *__restrict__ member_min,
               uint32_t *__restrict__ member_below) {
    __shared__ __attribute__((aligned(16))) int M[576];
    __shared__ __attribute__((aligned(16))) uint32_t seqs[256 * 2 * SEQ_STRIDE_DW];
    __shared__ int lmin[LINK_MEMB];
    __shared__ uint32_t lbelow[LINK_MEMB];
    __shared__ uint32_t span[2];   // the chunk's first member place, one past its last
    const int tid = threadIdx.x;
    const uint32_t lane = tid & 63u;
    for (int e = tid; e < 576; e += 256) M[e] = Mg[e];
    uint32_t *s1 = seqs + tid * 2 * SEQ_STRIDE_DW;
    uint32_t *s2 = s1 + SEQ_STRIDE_DW;
    const bool members = member_min != nullptr;   // (uniform)
    const unsigned long long n_chunks = (n_pairs + 255) / 256;
    for (unsigned long long chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        __syncthreads();   // the matrix stands; the last chunk's counters have been flushed
        if (members) for (int e = tid; e < LINK_MEMB; e += 256) { lmin[e] = INT32_MAX; lbelow[e] = 0; }
        const unsigned long long k = chunk * 256 + tid;
        const unsigned long long k_last = min(n_pairs, chunk * 256 + 256) - 1;
        const bool valid = k < n_pairs;
        uint32_t f = 0xFFFFFFFFu, a = 0, b = 0, ia = 0, ib = 0, mbase = 0;
        int score = INT32_MAX;
        if (valid) {
            f = run_of<unsigned long long>(fpstart, nf, k);
            const TriEntry e = tri_entry((uint32_t)(k - fpstart[f]));
            ib = e.row;
            ia = e.col;
            mbase = fmstart[f];
            a = tab[mbase + ia];
            b = tab[mbase + ib];   // a < b: the members of a slot are in index order
            if (members && tid == 0) span[0] = mbase;
            if (members && k == k_last) span[1] = fmstart[f + 1];
            score = link_pair_score(M, s1, s2, res32, len, a, b, X, p);
        }
        const bool low = valid && score < thr;
        // ---- the slot side: segmented scan over the wave's lanes (the slots of consecutive pairs never decrease)
        uint64_t best = valid ? link_key(score, a, b) : ~0ull;
        uint32_t cnt = low ? 1u : 0u;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t of = __shfl_up(f, d), oc = __shfl_up(cnt, d);
            const uint64_t ob = shfl_up_u64(best, d);
            if (lane >= (uint32_t)d && of == f) { best = min(best, ob); cnt += oc; }
        }
        const uint32_t nf_next = __shfl_down(f, 1);
        if (valid && (lane == 63 || nf_next != f)) {   // the segment's last lane holds its minimum and count
            atomicMin((unsigned long long *)&key[fslot[f]], (unsigned long long)best);
            if (cnt) atomicAdd(&below[fslot[f]], (unsigned long long)cnt);
        }
        // ---- the member side
        if (members) {
            __syncthreads();   // counters cleared, span written
            const uint32_t first = span[0];
            if (valid) {
                const uint32_t pa = mbase + ia - first, pb = mbase + ib - first;
                if (pb < (uint32_t)LINK_MEMB) {
                    atomicMin(&lmin[pa], score);
                    atomicMin(&lmin[pb], score);
                    if (low) { atomicAdd(&lbelow[pa], 1u); atomicAdd(&lbelow[pb], 1u); }
                } else {   // (never: see LINK_MEMB; kept so that no index leaves the counters)
                    atomicMin(&member_min[a - r0], score);
                    atomicMin(&member_min[b - r0], score);
                    if (low) { atomicAdd(&member_below[a - r0], 1u); atomicAdd(&member_below[b - r0], 1u); }
                }
            }
            __syncthreads();
            const uint32_t count = min(span[1] - first, (uint32_t)LINK_MEMB);
            for (uint32_t e = tid; e < count; e += 256) {
                const int mn = lmin[e];
                if (mn != INT32_MAX) {
                    const uint32_t m = tab[first + e] - r0;
                    atomicMin(&member_min[m], mn);
                    if (lbelow[e]) atomicAdd(&member_below[m], lbelow[e]);
                }
            }
        }
    }
}

// -----------------------------------------------------------------------------
// large slots: tiles of the triangle of the slot's member list
// -----------------------------------------------------------------------------
// Big slot g = slot bslot[g] with the members tab[bmstart[g] .. bmstart[g + 1]) and the tiles btstart[g] .. btstart[g + 1): tile
// t = i (i + 1) / 2 + j, j <= i, is rows [i T, (i + 1) T) x columns [j T, (j + 1) T) of the member list (T = LINK_TILE = the
// block size), of which the pairs row place > column place count.  The rows' residues lie in LDS and are read by all lanes at
// once; a lane keeps its column in LDS (9-dword stride, as k_pairs) and, over the rows, its column's key, count and minimum;
// a row's minimum is a wave reduction and its count a ballot, both kept by lane (row & 63) until the wave has done its rows.
__global__ void __launch_bounds__(256)
k_linkage_tiled(const uint8_t *__restrict__ res32, const uint8_t *__restrict__ len, const int32_t *__restrict__ Mg,
                const uint32_t *__restrict__ tab, const uint32_t *__restrict__ bslot, const uint32_t *__restrict__ bmstart,
                const uint32_t *__restrict__ btstart, uint32_t nb, uint32_t n_tiles, uint32_t r0, int X, int p, int thr,
                uint64_t *__restrict__ key, unsigned long long *__restrict__ below, int32_t *__restrict__ member_min,
                uint32_t *__restrict__ member_below) {
    constexpr int T = LINK_TILE;
    static_assert(T == 256, "a tile is as wide as the block");
    __shared__ __attribute__((aligned(16))) int M[576];
    __shared__ __attribute__((aligned(16))) uint32_t colseq[T * SEQ_STRIDE_DW];
    __shared__ __attribute__((aligned(16))) uint32_t rowseq[T * 8];
    __shared__ uint32_t rowidx[T];
    __shared__ int rowlen[T];
    __shared__ int rmin[T];
    __shared__ uint32_t rbelow[T];
    const int tid = threadIdx.x;
    const uint32_t lane = tid & 63u, wave = tid >> 6;
    for (int e = tid; e < 576; e += 256) M[e] = Mg[e];
    const bool members = member_min != nullptr;   // (uniform)
    uint32_t *mine = colseq + tid * SEQ_STRIDE_DW;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        uint32_t g, i, j;
        link_tile_decode(btstart, nb, tile, g, i, j);
        const uint32_t mbase = bmstart[g], s = bmstart[g + 1] - mbase;
        const uint32_t row0 = i * T, col0 = j * T;           // places in the member list; row0 < s
        const uint32_t nrows = min((uint32_t)T, s - row0), ncols = min((uint32_t)T, s - col0);
        __syncthreads();   // the matrix stands; the last tile's rows have been flushed
        if ((uint32_t)tid < nrows) {
            const uint32_t idx = tab[mbase + row0 + tid];
            link_stage_row(rowseq, tid, res32, idx);
            rowidx[tid] = idx;
            rowlen[tid] = len[idx];
        }
        rmin[tid] = INT32_MAX;
        rbelow[tid] = 0;
        const bool has_col = (uint32_t)tid < ncols;
        uint32_t cidx = 0;
        int clen = 0;
        if (has_col) {
            cidx = tab[mbase + col0 + tid];
            stage_sequence(mine, res32, cidx);
            clen = len[cidx];
        }
        __syncthreads();
        // the wave's rows: on the diagonal tile a row counts for the wave only beyond the wave's first column
        const uint32_t r_first = (i == j) ? wave * 64 + 1 : 0;
        const bool wave_has_cols = wave * 64 < ncols;
        uint64_t best = ~0ull;
        uint32_t cnt = 0;
        if (wave_has_cols && r_first < nrows) {
#pragma unroll 1
            for (uint32_t q = r_first >> 6; q * 64 < nrows; q++) {
                int acc_min = INT32_MAX;
                uint32_t acc_below = 0;
#pragma unroll 1
                for (uint32_t r = max(q * 64, r_first); r < min(q * 64 + 64, nrows); r++) {
                    const bool active = has_col && col0 + (uint32_t)tid < row0 + r;
                    int score = INT32_MAX;
                    if (active) {
                        score = shifted_score_literal(M, reinterpret_cast<const uint8_t *>(rowseq + r * 8), rowlen[r],
                                                      reinterpret_cast<const uint8_t *>(mine), clen, X, p);
                        const uint64_t kk = link_key(score, cidx, rowidx[r]);   // rows ascend: of equal scores the first row stays
                        if (kk < best) best = kk;
                    }
                    const bool low = active && score < thr;
                    if (low) cnt++;
                    if (members) {
                        int wmin = score;
#pragma unroll
                        for (int d = 32; d >= 1; d >>= 1) wmin = min(wmin, __shfl_xor(wmin, d));
                        const uint32_t nlow = (uint32_t)__popcll(__ballot(low));
                        if (lane == (r & 63u)) { acc_min = wmin; acc_below = nlow; }
                    }
                }
                if (members && acc_min != INT32_MAX) {
                    atomicMin(&rmin[q * 64 + lane], acc_min);
                    if (acc_below) atomicAdd(&rbelow[q * 64 + lane], acc_below);
                }
            }
        }
        // the column side: the lane's own minimum is its key's score
        if (members && best != ~0ull) {
            atomicMin(&member_min[cidx - r0], (int)(uint32_t)(best >> 48) - 32768);
            if (cnt) atomicAdd(&member_below[cidx - r0], cnt);
        }
        // the slot: one atomic per wave
        uint64_t wbest = best;
        uint32_t wcnt = cnt;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            wbest = min(wbest, shfl_xor_u64(wbest, d));
            wcnt += __shfl_xor(wcnt, d);
        }
        if (lane == 0 && wbest != ~0ull) {
            atomicMin((unsigned long long *)&key[bslot[g]], (unsigned long long)wbest);
            if (wcnt) atomicAdd(&below[bslot[g]], (unsigned long long)wcnt);
        }
        if (members) {
            __syncthreads();
            if ((uint32_t)tid < nrows && rmin[tid] != INT32_MAX) {
                atomicMin(&member_min[rowidx[tid] - r0], rmin[tid]);
                if (rbelow[tid]) atomicAdd(&member_below[rowidx[tid] - r0], rbelow[tid]);
            }
        }
    }
}

// -----------------------------------------------------------------------------
// launchers
// -----------------------------------------------------------------------------
hipError_t launch_linkage_init(uint64_t *key, unsigned long long *below, uint32_t n_clusters, int32_t *member_min, uint32_t *member_below,
                               uint32_t nm, hipStream_t s) {
    const uint32_t n = std::max(n_clusters, member_min ? nm : 0u);
    if (n == 0) return hipSuccess;
    const uint32_t blocks = capped_grid("k_linkage_init", std::min<uint32_t>((n + 255) / 256, 4096));
    hipLaunchKernelGGL(k_linkage_init, dim3(blocks), dim3(256), 0, s, key, below, n_clusters, member_min, member_below, nm);
    return hipGetLastError();
}

hipError_t launch_linkage_flat(const uint8_t *res32, const uint8_t *len, const int32_t *d_matrix, const impl::LinkView &V, uint32_t r0, int X, int p,
                               int thr, uint64_t *key, unsigned long long *below, int32_t *member_min, uint32_t *member_below, hipStream_t s) {
    if (V.flat_pairs == 0 || V.nf == 0) return hipSuccess;
    const unsigned long long chunks = (V.flat_pairs + 255) / 256;
    const uint32_t blocks = capped_grid("k_linkage_flat", (uint32_t)std::min<unsigned long long>(chunks, 65536));
    hipLaunchKernelGGL(k_linkage_flat, dim3(blocks), dim3(256), 0, s, res32, len, d_matrix, V.tab, V.fslot, V.fmstart, V.fpstart, V.nf, V.flat_pairs,
                       r0, X, p, thr, key, below, member_min, member_below);
    return hipGetLastError();
}

hipError_t launch_linkage_tiled(const uint8_t *res32, const uint8_t *len, const int32_t *d_matrix, const impl::LinkView &V, uint32_t r0, int X, int p,
                                int thr, uint64_t *key, unsigned long long *below, int32_t *member_min, uint32_t *member_below, hipStream_t s) {
    if (V.n_tiles == 0 || V.nb == 0) return hipSuccess;
    const uint32_t blocks = capped_grid("k_linkage_tiled", std::min<uint32_t>(V.n_tiles, 65536));
    hipLaunchKernelGGL(k_linkage_tiled, dim3(blocks), dim3(256), 0, s, res32, len, d_matrix, V.tab, V.bslot, V.bmstart, V.btstart, V.nb, V.n_tiles,
                       r0, X, p, thr, key, below, member_min, member_below);
    return hipGetLastError();
}

}  // namespace hmk
