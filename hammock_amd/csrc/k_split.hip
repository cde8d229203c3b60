// k_split.hip -- every score INSIDE given clusters (hmk_clinkage_split, hmk_split.cpp): per slot the dense strict lower triangle of
// its member list, int16 per pair, entry q = i (i - 1) / 2 + j (j < i) = score(seq1 = member i, seq2 = member j).  The host's
// nearest-neighbour chain of a slot reads its candidate lists straight off that triangle.  The pair space and its decoding are
// k_linkage.hip's (hmk_link_device.h); where that kernel reduces, these store:
//   k_split_flat    slots of up to LINK_FLAT_MAX members: a lane per pair of the flat pair space, and the flat pair number IS the
//                   output index -- a wave stores 128 contiguous bytes
//   k_split_tiled   larger slots: LINK_TILE x LINK_TILE tiles on or below the diagonal, a workgroup per quarter of a tile's rows; the
//                   rows in LDS, a column per lane; for each row the lanes of a wave store consecutive int16 of one triangle row
// No atomics, no cursor, nothing to overflow: every entry of the array is written exactly once.
#include <algorithm>

#include "hmk_link_device.h"
#include "hmk_grid.h"
#include "hmk_split.h"

namespace hmk {

__global__ void __launch_bounds__(256)
k_split_flat(const uint8_t *__restrict__ res32, const uint8_t *__restrict__ len, const int32_t *__restrict__ Mg,
             const uint32_t *__restrict__ tab, const uint32_t *__restrict__ fmstart, const unsigned long long *__restrict__ fpstart, uint32_t nf,
             unsigned long long n_pairs, int X, int p, int16_t *__restrict__ scores) {
    __shared__ __attribute__((aligned(16))) int M[576];
    __shared__ __attribute__((aligned(16))) uint32_t seqs[256 * 2 * SEQ_STRIDE_DW];
    const int tid = threadIdx.x;
    for (int e = tid; e < 576; e += 256) M[e] = Mg[e];
    __syncthreads();
    uint32_t *s1 = seqs + tid * 2 * SEQ_STRIDE_DW;   // (the lane's own two sequences: no barrier between chunks)
    uint32_t *s2 = s1 + SEQ_STRIDE_DW;
    const unsigned long long n_chunks = (n_pairs + 255) / 256;
    for (unsigned long long chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const unsigned long long k = chunk * 256 + tid;
        if (k >= n_pairs) continue;
        const uint32_t f = run_of<unsigned long long>(fpstart, nf, k);
        const TriEntry e = tri_entry((uint32_t)(k - fpstart[f]));   // the entry of the slot's own triangle that pair k is
        const uint32_t mbase = fmstart[f];
        const uint32_t a = tab[mbase + e.col], b = tab[mbase + e.row];   // a < b: the members of a slot are in index order
        scores[k] = (int16_t)link_pair_score(M, s1, s2, res32, len, a, b, X, p);
    }
}

// A work item is a quarter of a tile, SPLIT_ROWS of its rows x its LINK_TILE columns: the tiles are k_linkage_tiled's, but a lane that
// scores all 256 rows of its column keeps a workgroup busy for so long that the last round of tiles left a fifth of the device idle
// on one slot of 20,000 members (measured on both sides).
constexpr int SPLIT_ROWS = 64;

__global__ void __launch_bounds__(256)
k_split_tiled(const uint8_t *__restrict__ res32, const uint8_t *__restrict__ len, const int32_t *__restrict__ Mg,
              const uint32_t *__restrict__ tab, const uint32_t *__restrict__ bmstart, const uint32_t *__restrict__ btstart,
              const unsigned long long *__restrict__ tbase, uint32_t nb, uint32_t n_tiles, int X, int p, int16_t *__restrict__ scores) {
    constexpr int T = LINK_TILE, R = SPLIT_ROWS, PARTS = T / R;
    static_assert(T == 256 && R == 64, "a tile is as wide as the block, a quarter as high as a wave is wide");
    __shared__ __attribute__((aligned(16))) int M[576];
    __shared__ __attribute__((aligned(16))) uint32_t colseq[T * SEQ_STRIDE_DW];
    __shared__ __attribute__((aligned(16))) uint32_t rowseq[R * 8];
    __shared__ int rowlen[R];
    const int tid = threadIdx.x;
    const uint32_t wave = tid >> 6;
    for (int e = tid; e < 576; e += 256) M[e] = Mg[e];
    uint32_t *mine = colseq + tid * SEQ_STRIDE_DW;
    const unsigned long long n_items = (unsigned long long)n_tiles * PARTS;
    for (unsigned long long item = blockIdx.x; item < n_items; item += gridDim.x) {
        const uint32_t tile = (uint32_t)(item / PARTS), part = (uint32_t)(item % PARTS);
        uint32_t g, i, j;
        link_tile_decode(btstart, nb, tile, g, i, j);
        const uint32_t mbase = bmstart[g], s = bmstart[g + 1] - mbase;
        const uint32_t row0 = i * T + part * R, col0 = j * T;   // places in the member list
        if (row0 >= s) continue;                                 // (the same for the whole workgroup: the slot's last row block is short)
        const uint32_t nrows = min((uint32_t)R, s - row0), ncols = min((uint32_t)T, s - col0);
        __syncthreads();   // the matrix stands; the last item's rows have been read
        if ((uint32_t)tid < nrows) {
            const uint32_t idx = tab[mbase + row0 + tid];
            link_stage_row(rowseq, tid, res32, idx);
            rowlen[tid] = len[idx];
        }
        const bool has_col = (uint32_t)tid < ncols;
        int clen = 0;
        if (has_col) {
            const uint32_t cidx = tab[mbase + col0 + tid];
            stage_sequence(mine, res32, cidx);
            clen = len[cidx];
        }
        __syncthreads();
        // on the diagonal tile a row holds entries for a wave only beyond the wave's first column
        const uint32_t col = col0 + (uint32_t)tid, wave_col0 = col0 + wave * 64;
        int16_t *tri = scores + tbase[g];
        if (wave * 64 < ncols && wave_col0 + 1 < row0 + nrows) {   // (wave-uniform: some row of the item lies beyond the wave's first column)
#pragma unroll 1
            for (uint32_t r = (wave_col0 >= row0 ? wave_col0 - row0 + 1 : 0); r < nrows; r++) {
                const uint32_t row = row0 + r;
                if (has_col && col < row) {   // the entry lies inside the slot's triangle: row < s and col < row
                    const int score = shifted_score_literal(M, reinterpret_cast<const uint8_t *>(rowseq + r * 8), rowlen[r],
                                                            reinterpret_cast<const uint8_t *>(mine), clen, X, p);
                    tri[(unsigned long long)row * (row - 1) / 2 + col] = (int16_t)score;
                }
            }
        }
    }
}

// -----------------------------------------------------------------------------
// launchers
// -----------------------------------------------------------------------------
hipError_t launch_split_flat(const uint8_t *res32, const uint8_t *len, const int32_t *d_matrix, const impl::LinkView &V, int X, int p,
                             int16_t *scores, hipStream_t s) {
    if (V.flat_pairs == 0 || V.nf == 0) return hipSuccess;
    const unsigned long long chunks = (V.flat_pairs + 255) / 256;
    const uint32_t blocks = capped_grid("k_split_flat", (uint32_t)std::min<unsigned long long>(chunks, 65536));
    hipLaunchKernelGGL(k_split_flat, dim3(blocks), dim3(256), 0, s, res32, len, d_matrix, V.tab, V.fmstart, V.fpstart, V.nf, V.flat_pairs, X, p,
                       scores);
    return hipGetLastError();
}

hipError_t launch_split_tiled(const uint8_t *res32, const uint8_t *len, const int32_t *d_matrix, const impl::LinkView &V, int X, int p,
                              int16_t *scores, hipStream_t s) {
    if (V.n_tiles == 0 || V.nb == 0) return hipSuccess;
    const uint32_t blocks =
        capped_grid("k_split_tiled", (uint32_t)std::min<unsigned long long>((unsigned long long)V.n_tiles * (LINK_TILE / SPLIT_ROWS), 65536));
    hipLaunchKernelGGL(k_split_tiled, dim3(blocks), dim3(256), 0, s, res32, len, d_matrix, V.tab, V.bmstart, V.btstart, V.tbase, V.nb, V.n_tiles, X,
                       p, scores);
    return hipGetLastError();
}

}  // namespace hmk
