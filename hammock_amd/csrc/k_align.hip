// k_align.hip -- centre-star alignment of given clusters around their medoids (hmk_cluster_align_shifted, hmk_align.cpp): per member
// the sum of its ShiftedScorer scores against the other members of its slot, per slot the member with the largest sum (the centre),
// per member scoreWithShift against its slot's centre (ShiftedScorer.java:48-95), per slot the smallest shift and the largest
// shift + length.  The pair space is that of k_linkage.hip -- block-diagonal, sum of s (s - 1) / 2 over the slots, decoded from the
// same host tables (hmk_linkage.h: LinkTables) -- and nothing proportional to it is stored:
//   k_align_init        the accumulators of the call
//   k_align_sums_flat   slots of up to LINK_FLAT_MAX members: a lane per pair, the members' partial sums in LDS
//   k_align_sums_tiled  larger slots: LINK_TILE x LINK_TILE tiles on or below the diagonal, a column per lane, a row per wave reduction
//   k_align_center      a lane per member: the slot's key (largest sum, then smallest index), one atomic per wave and slot segment
//   k_align_shift       a lane per member: the literal scorer against the centre the key names, the slot's extent
// The pair kernels score with seq1 = the pair's larger index, as k_linkage.hip does.  Integer adds, minima and maxima only: no result
// depends on the schedule.
#include <algorithm>

#include "hmk_align.h"
#include "hmk_link_device.h"
#include "hmk_grid.h"

namespace hmk {

namespace {

// 64-bit add of a signed partial sum (two's complement: the unsigned add is the signed one)
__device__ __forceinline__ void add_sum(long long *dst, int v) {
    atomicAdd(reinterpret_cast<unsigned long long *>(dst), (unsigned long long)(long long)v);
}

// The centre's key.  |score| <= 32,767 (check_link_scores proves both ends) and a slot has fewer than 2^24 members (n <= 2^24), so
// |sum| < 2^15 * 2^24 = 2^39: sum + 2^39 lies in [0, 2^40) and leaves the low 24 bits to the index.  A 64-bit maximum keeps the
// largest sum and, among equal sums, the largest 0xFFFFFF - index: the smallest index.
__device__ __forceinline__ uint64_t center_key(long long sum, uint32_t index) {
    return ((uint64_t)(sum + (1ll << 39)) << 24) | (uint64_t)(0xFFFFFFu - index);
}
__device__ __forceinline__ uint32_t key_index(uint64_t key) { return 0xFFFFFFu - ((uint32_t)key & 0xFFFFFFu); }

__device__ __forceinline__ uint64_t shfl_up_u64(uint64_t v, int d) {
    const uint32_t lo = __shfl_up((uint32_t)v, d), hi = __shfl_up((uint32_t)(v >> 32), d);
    return ((uint64_t)hi << 32) | lo;
}

// place t of tab -> its run (flat slots 0 .. nf - 1, then big slots nf ...: never decreasing in t) and the caller's slot
__device__ __forceinline__ void slot_of_place(const AlignSlots &T, uint32_t t, uint32_t &run, uint32_t &slot) {
    if (t < T.fmstart[T.nf]) {
        run = run_of<uint32_t>(T.fmstart, T.nf, t);
        slot = T.fslot[run];
    } else {
        const uint32_t g = run_of<uint32_t>(T.bmstart, T.nb, t);
        run = T.nf + g;
        slot = T.bslot[g];
    }
}

}  // namespace

// -----------------------------------------------------------------------------
// accumulators: cleared by every call, so that no state survives one
// -----------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_align_init(AlignOut out, uint32_t n_clusters, uint32_t nm) {
    const uint32_t n = max(n_clusters, nm);
    for (uint32_t k = blockIdx.x * 256 + threadIdx.x; k < n; k += gridDim.x * 256) {
        if (k < n_clusters) { out.key[k] = 0; out.min_shift[k] = INT32_MAX; out.max_end[k] = INT32_MIN; }
        if (k < nm) { out.sum[k] = 0; out.score[k] = INT32_MAX; out.shift[k] = 0; }
    }
}

// -----------------------------------------------------------------------------
// small slots: a lane per pair
// -----------------------------------------------------------------------------
// The decode is k_linkage_flat's: chunks of 256 consecutive pairs of the flat pair space, the members' partial sums in LDS at the
// member's place behind the chunk's first slot (LINK_MEMB places: see k_linkage.hip).  A chunk holds 256 pairs and a score's
// magnitude is at most 32,767 (check_link_scores), so a member's partial sum of one chunk is at most 256 * 32,767 < 2^23 in
// magnitude: int32 in LDS cannot overflow.  Then one 64-bit global add per touched member and chunk.
constexpr int ALIGN_MEMB = 2 * 256 + 2 * LINK_FLAT_MAX;

__global__ void __launch_bounds__(256)
k_align_sums_flat(const uint8_t *__restrict__ res32, const uint8_t *__restrict__ len, const int32_t *__restrict__ Mg,
                  const uint32_t *__restrict__ tab, const uint32_t *__restrict__ fmstart, const unsigned long long *__restrict__ fpstart,
                  uint32_t nf, unsigned long long n_pairs, uint32_t r0, int X, int p, long long *__restrict__ sum) {
    __shared__ __attribute__((aligned(16))) int M[576];
    __shared__ __attribute__((aligned(16))) uint32_t seqs[256 * 2 * SEQ_STRIDE_DW];
    __shared__ int lsum[ALIGN_MEMB];
    __shared__ uint32_t span[2];   // the chunk's first member place, one past its last
    const int tid = threadIdx.x;
    for (int e = tid; e < 576; e += 256) M[e] = Mg[e];
    uint32_t *s1 = seqs + tid * 2 * SEQ_STRIDE_DW;
    uint32_t *s2 = s1 + SEQ_STRIDE_DW;
    const unsigned long long n_chunks = (n_pairs + 255) / 256;
    for (unsigned long long chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        __syncthreads();   // the matrix stands; the last chunk's sums have been flushed
        for (int e = tid; e < ALIGN_MEMB; e += 256) lsum[e] = 0;
        const unsigned long long k = chunk * 256 + tid;
        const unsigned long long k_last = min(n_pairs, chunk * 256 + 256) - 1;
        const bool valid = k < n_pairs;
        uint32_t a = 0, b = 0, ia = 0, ib = 0, mbase = 0;
        int score = 0;
        if (valid) {
            const uint32_t f = run_of<unsigned long long>(fpstart, nf, k);
            const TriEntry e = tri_entry((uint32_t)(k - fpstart[f]));
            ib = e.row;
            ia = e.col;
            mbase = fmstart[f];
            a = tab[mbase + ia];
            b = tab[mbase + ib];   // a < b: the members of a slot are in index order
            if (tid == 0) span[0] = mbase;
            if (k == k_last) span[1] = fmstart[f + 1];
            score = link_pair_score(M, s1, s2, res32, len, a, b, X, p);
        }
        __syncthreads();   // sums cleared, span written
        const uint32_t first = span[0];
        if (valid) {
            const uint32_t pa = mbase + ia - first, pb = mbase + ib - first;   // pa < pb
            if (pb < (uint32_t)ALIGN_MEMB) {
                atomicAdd(&lsum[pa], score);
                atomicAdd(&lsum[pb], score);
            } else {   // (never: see LINK_MEMB in k_linkage.hip; kept so that no index leaves the sums)
                add_sum(&sum[a - r0], score);
                add_sum(&sum[b - r0], score);
            }
        }
        __syncthreads();
        const uint32_t count = min(span[1] - first, (uint32_t)ALIGN_MEMB);
        for (uint32_t e = tid; e < count; e += 256) {
            const int v = lsum[e];
            if (v) add_sum(&sum[tab[first + e] - r0], v);   // (a partial sum of 0 adds nothing)
        }
    }
}

// -----------------------------------------------------------------------------
// large slots: tiles of the triangle of the slot's member list
// -----------------------------------------------------------------------------
// The tiles, the staging and the wave's rows are k_linkage_tiled's.  Column side: the lane's own int32 sum over the tile's rows (at
// most 256 * 32,767), one global add per lane.  Row side: a row's sum over the wave's 64 columns is a wave reduction, kept by lane
// (row & 63) until the wave has done 64 rows, then one LDS add per row and wave, then one global add per row and tile.
__global__ void __launch_bounds__(256)
k_align_sums_tiled(const uint8_t *__restrict__ res32, const uint8_t *__restrict__ len, const int32_t *__restrict__ Mg,
                   const uint32_t *__restrict__ tab, const uint32_t *__restrict__ bmstart, const uint32_t *__restrict__ btstart, uint32_t nb,
                   uint32_t n_tiles, uint32_t r0, int X, int p, long long *__restrict__ sum) {
    constexpr int T = LINK_TILE;
    static_assert(T == 256, "a tile is as wide as the block");
    __shared__ __attribute__((aligned(16))) int M[576];
    __shared__ __attribute__((aligned(16))) uint32_t colseq[T * SEQ_STRIDE_DW];
    __shared__ __attribute__((aligned(16))) uint32_t rowseq[T * 8];
    __shared__ uint32_t rowidx[T];
    __shared__ int rowlen[T];
    __shared__ int rsum[T];
    const int tid = threadIdx.x;
    const uint32_t lane = tid & 63u, wave = tid >> 6;
    for (int e = tid; e < 576; e += 256) M[e] = Mg[e];
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
        rsum[tid] = 0;
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
        int csum = 0;
        if (wave_has_cols && r_first < nrows) {
#pragma unroll 1
            for (uint32_t q = r_first >> 6; q * 64 < nrows; q++) {
                int acc = 0;
#pragma unroll 1
                for (uint32_t r = max(q * 64, r_first); r < min(q * 64 + 64, nrows); r++) {
                    const bool active = has_col && col0 + (uint32_t)tid < row0 + r;
                    int score = 0;
                    if (active) {
                        score = shifted_score_literal(M, reinterpret_cast<const uint8_t *>(rowseq + r * 8), rowlen[r],
                                                      reinterpret_cast<const uint8_t *>(mine), clen, X, p);
                        csum += score;
                    }
                    int wsum = score;
#pragma unroll
                    for (int d = 32; d >= 1; d >>= 1) wsum += __shfl_xor(wsum, d);
                    if (lane == (r & 63u)) acc = wsum;
                }
                if (acc) atomicAdd(&rsum[q * 64 + lane], acc);
            }
        }
        if (csum) add_sum(&sum[cidx - r0], csum);
        __syncthreads();
        if ((uint32_t)tid < nrows && rsum[tid]) add_sum(&sum[rowidx[tid] - r0], rsum[tid]);
    }
}

// -----------------------------------------------------------------------------
// the centre of every slot
// -----------------------------------------------------------------------------
// Grid-stride over the places of tab, 256 per block and step.  The runs of consecutive places never decrease, so the slot's maximum
// is a segmented scan over the wave and one 64-bit atomicMax per wave and slot segment.
__global__ void __launch_bounds__(256)
k_align_center(AlignSlots T, uint32_t r0, const long long *__restrict__ sum, uint64_t *__restrict__ key) {
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t base = blockIdx.x * 256; base < T.nt; base += gridDim.x * 256) {   // (uniform: every lane takes every step)
        const uint32_t t = base + threadIdx.x;
        const bool valid = t < T.nt;
        uint32_t run = 0xFFFFFFFFu, slot = 0;
        uint64_t best = 0;
        if (valid) {
            slot_of_place(T, t, run, slot);
            const uint32_t m = T.tab[t];
            best = center_key(sum[m - r0], m);
        }
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t orun = __shfl_up(run, d);
            const uint64_t ob = shfl_up_u64(best, d);
            if (lane >= (uint32_t)d && orun == run) best = max(best, ob);
        }
        const uint32_t next = __shfl_down(run, 1);
        if (valid && (lane == 63 || next != run))   // the segment's last lane holds its maximum
            atomicMax((unsigned long long *)&key[slot], (unsigned long long)best);
    }
}

// -----------------------------------------------------------------------------
// every member against its slot's centre
// -----------------------------------------------------------------------------
// A lane per place of tab: the centre is read from the slot's finished key (k_align_center, earlier on the stream), both sequences are
// staged in the lane's LDS and scored by the literal scorer with seq1 = the centre, which tracks the first strict maximum of the
// shift loop (ShiftedScorer.java:86-89) and applies the sign rule (:91-93).  The centre itself keeps the cleared INT32_MAX / 0 and
// enters the slot's extent with shift 0.  The extent is reduced per wave and slot segment as the key is.
__global__ void __launch_bounds__(256)
k_align_shift(const uint8_t *__restrict__ res32, const uint8_t *__restrict__ len, const int32_t *__restrict__ Mg, AlignSlots T, uint32_t r0,
              uint32_t r1, int X, int p, AlignOut out) {
    __shared__ __attribute__((aligned(16))) int M[576];
    __shared__ __attribute__((aligned(16))) uint32_t seqs[256 * 2 * SEQ_STRIDE_DW];
    const int tid = threadIdx.x;
    const uint32_t lane = tid & 63u;
    for (int e = tid; e < 576; e += 256) M[e] = Mg[e];
    __syncthreads();
    uint32_t *s1 = seqs + tid * 2 * SEQ_STRIDE_DW;
    uint32_t *s2 = s1 + SEQ_STRIDE_DW;
    for (uint32_t base = blockIdx.x * 256; base < T.nt; base += gridDim.x * 256) {   // (uniform: every lane takes every step)
        const uint32_t t = base + tid;
        const bool valid = t < T.nt;
        uint32_t run = 0xFFFFFFFFu, slot = 0;
        int lo = INT32_MAX, hi = INT32_MIN;
        bool valid_z = true;
        if (valid) {
            slot_of_place(T, t, run, slot);
            const uint32_t m = T.tab[t], z = key_index(out.key[slot]);
            int shift = 0;
            if (z < r0 || z >= r1) {   // (never: the key holds a member; no index from it is used unchecked, and the host refuses a slot without extent)
                valid_z = false;
            } else if (m != z) {
                stage_sequence(s1, res32, z);
                stage_sequence(s2, res32, m);
                const int score = shifted_score_literal(M, reinterpret_cast<const uint8_t *>(s1), len[z], reinterpret_cast<const uint8_t *>(s2),
                                                        len[m], X, p, &shift);
                out.score[m - r0] = score;
                out.shift[m - r0] = shift;
            }
            if (valid_z) {
                lo = shift;
                hi = shift + (int)len[m];
            }
        }
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t orun = __shfl_up(run, d);
            const int olo = __shfl_up(lo, d), ohi = __shfl_up(hi, d);
            if (lane >= (uint32_t)d && orun == run) { lo = min(lo, olo); hi = max(hi, ohi); }
        }
        const uint32_t next = __shfl_down(run, 1);
        if (valid && (lane == 63 || next != run)) {
            atomicMin(&out.min_shift[slot], lo);
            atomicMax(&out.max_end[slot], hi);
        }
    }
}

// -----------------------------------------------------------------------------
// launchers
// -----------------------------------------------------------------------------
hipError_t launch_align_init(const AlignOut &out, uint32_t n_clusters, uint32_t nm, hipStream_t s) {
    const uint32_t n = std::max(n_clusters, nm);
    if (n == 0) return hipSuccess;
    const uint32_t blocks = capped_grid("k_align_init", std::min<uint32_t>((n + 255) / 256, 4096));
    hipLaunchKernelGGL(k_align_init, dim3(blocks), dim3(256), 0, s, out, n_clusters, nm);
    return hipGetLastError();
}

hipError_t launch_align_sums_flat(const uint8_t *res32, const uint8_t *len, const int32_t *d_matrix, const impl::LinkView &V, uint32_t r0, int X,
                                  int p, long long *sum, hipStream_t s) {
    if (V.flat_pairs == 0 || V.nf == 0) return hipSuccess;
    const unsigned long long chunks = (V.flat_pairs + 255) / 256;
    const uint32_t blocks = capped_grid("k_align_sums_flat", (uint32_t)std::min<unsigned long long>(chunks, 65536));
    hipLaunchKernelGGL(k_align_sums_flat, dim3(blocks), dim3(256), 0, s, res32, len, d_matrix, V.tab, V.fmstart, V.fpstart, V.nf, V.flat_pairs, r0, X,
                       p, sum);
    return hipGetLastError();
}

hipError_t launch_align_sums_tiled(const uint8_t *res32, const uint8_t *len, const int32_t *d_matrix, const impl::LinkView &V, uint32_t r0, int X,
                                   int p, long long *sum, hipStream_t s) {
    if (V.n_tiles == 0 || V.nb == 0) return hipSuccess;
    const uint32_t blocks = capped_grid("k_align_sums_tiled", std::min<uint32_t>(V.n_tiles, 65536));
    hipLaunchKernelGGL(k_align_sums_tiled, dim3(blocks), dim3(256), 0, s, res32, len, d_matrix, V.tab, V.bmstart, V.btstart, V.nb, V.n_tiles, r0, X,
                       p, sum);
    return hipGetLastError();
}

hipError_t launch_align_center(const AlignSlots &T, uint32_t r0, const long long *sum, uint64_t *key, hipStream_t s) {
    if (T.nt == 0) return hipSuccess;
    const uint32_t blocks = capped_grid("k_align_center", std::min<uint32_t>((T.nt + 255) / 256, 65536));
    hipLaunchKernelGGL(k_align_center, dim3(blocks), dim3(256), 0, s, T, r0, sum, key);
    return hipGetLastError();
}

hipError_t launch_align_shift(const uint8_t *res32, const uint8_t *len, const int32_t *d_matrix, const AlignSlots &T, uint32_t r0, uint32_t r1,
                              int X, int p, const AlignOut &out, hipStream_t s) {
    if (T.nt == 0) return hipSuccess;
    const uint32_t blocks = capped_grid("k_align_shift", std::min<uint32_t>((T.nt + 255) / 256, 65536));
    hipLaunchKernelGGL(k_align_shift, dim3(blocks), dim3(256), 0, s, res32, len, d_matrix, T, r0, r1, X, p, out);
    return hipGetLastError();
}

}  // namespace hmk
