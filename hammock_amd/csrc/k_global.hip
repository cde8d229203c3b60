// k_global.hip -- GlobalAlignmentScorer (Gotoh's global alignment with affine gaps, hmk_device.h: global_score_literal) on the
// length-bucketed tiles of the LocalAlignmentScorer plans: register-resident striped DP and the literal form, thresholded
// pairs -> edge list.
#include "hmk_device.h"

namespace hmk {

// One strip of KL lines (DP lines line0 + 1 .. line0 + KL of the wave-uniform row sequence, whose query profile stands in LDS at
// strip_addr: four int8 per dword) against this lane's column sequence (boff[j] = residue * 32), column by column.  Per column
// H[j] / F[j] hold H / F of the line above the strip on entry and of the strip's last line on exit; per line hd / ho / e hold
// H[line-1][j], H[line][j] + open, E[line][j] of the column to the left.  `last` leaves as H of the strip's last line in column ncols.
template <int LBMAX, int KL>
__device__ __forceinline__ void global_strip(uint32_t strip_addr, int line0, int ncols, const uint32_t (&boff)[LBMAX], int (&H)[LBMAX],
                                             int (&F)[LBMAX], int gap_open, int gap_extend, int &last) {
    int hd[KL], ho[KL], e[KL];
#pragma unroll
    for (int k = 0; k < KL; k++) {   // column 0: H[i][0] = open + (i - 1) ext, H[0][0] = 0, E[i][0] = -inf
        const int h0 = gap_open + (line0 + k) * gap_extend;
        ho[k] = h0 + gap_open;
        hd[k] = h0 - gap_extend;
        e[k] = GLOBAL_NEG_INF;
    }
    if (line0 == 0) hd[0] = 0;
#pragma unroll
    for (int j = 0; j < LBMAX; j++) {
        if (j < ncols) {   // (wave-uniform)
            const uint32_t q = lds_read<uint32_t>(strip_addr + boff[j]);
            int habove = H[j], fabove = F[j];
            int hoabove = habove + gap_open;
#pragma unroll
            for (int k = 0; k < KL; k++) {   // 8 VALU instructions per cell: H + open is added once for the cell below and the cell to the right
                const int sc = (int)(int8_t)(q >> (8 * k));
                const int ev = max(e[k] + gap_extend, ho[k]);
                const int fv = max(fabove + gap_extend, hoabove);
                const int h = max(hd[k] + sc, max(ev, fv));
                hd[k] = habove;
                habove = h;
                hoabove = h + gap_open;
                ho[k] = hoabove;
                fabove = fv;
                e[k] = ev;
            }
            H[j] = habove;
            F[j] = fabove;
            last = habove;
        }
    }
}

// global(seq1 = the row at row_q_addr, la lines; seq2 = this lane's column sequence, lb columns): the cell (la, lb).  The last
// strip has the la mod 4 lines the row still has, so the columns' H are those of line la when it ends.
template <int LBMAX>
__device__ __forceinline__ int global_row(uint32_t row_q_addr, int la, int lb, const uint32_t (&boff)[LBMAX], int gap_open,
                                          int gap_extend) {
    int H[LBMAX], F[LBMAX];
#pragma unroll
    for (int j = 0; j < LBMAX; j++) { H[j] = gap_open + j * gap_extend; F[j] = GLOBAL_NEG_INF; }   // line 0
    int last = 0;
    const int full = la >> 2, kl = la & 3;   // whole strips, then the 1..3 lines the row still has (none: line la ended the last whole strip)
    for (int st = 0; st < full; st++) global_strip<LBMAX, 4>(row_q_addr + (uint32_t)st * 4u, 4 * st, lb, boff, H, F, gap_open, gap_extend, last);
    const uint32_t addr = row_q_addr + (uint32_t)full * 4u;
    if (kl == 3) global_strip<LBMAX, 3>(addr, 4 * full, lb, boff, H, F, gap_open, gap_extend, last);
    else if (kl == 2) global_strip<LBMAX, 2>(addr, 4 * full, lb, boff, H, F, gap_open, gap_extend, last);
    else if (kl == 1) global_strip<LBMAX, 1>(addr, 4 * full, lb, boff, H, F, gap_open, gap_extend, last);
    return last;
}

// what a tile keeps of (row, column): everything (two sets), column > row (diag == 1: the triangle of one class) or
// column != row (diag == 2: all ordered pairs of one class)
__device__ __forceinline__ bool global_keeps(uint32_t diag, uint32_t row, uint32_t col) {
    return diag == 0 || (diag == 1 ? col > row : col != row);
}

// -----------------------------------------------------------------------------
// k_neighbors_global: thresholded pairs with GlobalAlignmentScorer -> edge list
// -----------------------------------------------------------------------------
// The tiles of a PlanLocal: one (row length la, column length lb) class per tile, so the DP's bounds are wave-uniform.  One
// column sequence (seq2) per lane, its H and F in VGPRs; the 16 rows (seq1) as query profiles in LDS.  The edge of (row, column)
// carries global(seq1 = row, seq2 = column): a symmetric pass (P.symmetric: classes la <= lb, triangle tiles) stores it as
// (min, max), every other pass as m = row (P.row_is_m).  Needs |M| <= 127 (int8 profiles).
template <int LBMAX>
__global__ void __launch_bounds__(256)
k_neighbors_global(const NeighborParams P, const uint32_t tile_base, const int32_t *__restrict__ Mg, int gap_open, int gap_extend,
                   int threshold) {
    constexpr int R = 16;
    constexpr int QROW = 25 * 8 * 4;
    constexpr int STAGE_CAP = 128;
    constexpr int REC_DW = 3;
    __shared__ __attribute__((aligned(16))) uint8_t smem[R * QROW + 576 + R * 32 + 4 * STAGE_CAP * REC_DW * 4];
    int8_t *m8 = reinterpret_cast<int8_t *>(smem + R * QROW);
    uint8_t *rowres = smem + R * QROW + 576;
    uint32_t *stage_all = reinterpret_cast<uint32_t *>(smem + R * QROW + 576 + R * 32);
    const Tile T = P.tiles[tile_base + blockIdx.x];
    const TileClass *Cp = P.classes + T.cls;
    const int la = Cp->la, lb = Cp->lb;   // la: row (seq1) length, lb: column (seq2) length
    const uint32_t shard = tile_shard(tile_base + blockIdx.x);
    const int tid = threadIdx.x;
    HMK_LDS uint32_t *stage = (HMK_LDS uint32_t *)stage_all + (tid >> 6) * (STAGE_CAP * REC_DW);

    for (int e = tid; e < 576; e += 256) m8[e] = (int8_t)Mg[e];
    for (int e = tid; e < R * 32; e += 256) {
        const uint32_t r = (uint32_t)e >> 5, k = e & 31;
        rowres[e] = (r < T.nrows && k < P.lpad) ? P.res_sorted[(size_t)(T.row0 + r) * P.lpad + k] : 0;
    }
    __syncthreads();
    __shared__ int row_len[R];
    if (tid < R) row_len[tid] = (uint32_t)tid < T.nrows ? la : 0;
    __syncthreads();
    build_profiles<R>(reinterpret_cast<uint32_t *>(smem), m8, rowres, row_len, T.nrows, 1, tid);
    __syncthreads();

    const uint32_t q_addr = lds_addr(smem);
    const uint32_t col_end = T.col0 + T.ncols;
    const uint32_t wave_last = (uint32_t)__builtin_amdgcn_readfirstlane(tid) | 63u;   // the wave's last lane
    uint32_t cnt = 0;
    for (uint32_t c0 = T.col0; c0 < col_end; c0 += 256) {
        const uint32_t col = c0 + tid;
        const bool col_ok = col < col_end;
        uint32_t boff[LBMAX];
        {
            uint32_t words[8];
#pragma unroll
            for (int q = 0; q < 8; q++) words[q] = 0;
            if (col_ok) {
                const u32x4 *src = reinterpret_cast<const u32x4 *>(P.res_sorted + (size_t)col * P.lpad);
                const u32x4 v0 = src[0];
                words[0] = v0.x; words[1] = v0.y; words[2] = v0.z; words[3] = v0.w;
                if (LBMAX > 16) {
                    const u32x4 v1 = src[1];
                    words[4] = v1.x; words[5] = v1.y; words[6] = v1.z; words[7] = v1.w;
                }
            }
#pragma unroll
            for (int j = 0; j < LBMAX; j++) {
                const uint32_t c = (col_ok && j < lb) ? ((words[j >> 2] >> ((j & 3) * 8)) & 0xFFu) : 24u;
                boff[j] = c * 32u;
            }
        }
        for (uint32_t r = 0; r < T.nrows; r++) {
            if (T.diag == 1 && c0 + wave_last <= T.row0 + r) continue;   // a triangle tile: none of this wave's columns is beyond the row
            const int score = global_row<LBMAX>(q_addr + r * QROW, la, lb, boff, gap_open, gap_extend);
            const bool keep = col_ok && score >= threshold && global_keeps(T.diag, T.row0 + r, col);
            const uint64_t mask = __ballot(keep);
            if (mask != 0) {
                if (cnt > (uint32_t)(STAGE_CAP - 64)) {
                    flush_stage<0>(stage, cnt, P, T, 0, false, shard);
                    cnt = 0;
                }
                if (keep) {
                    HMK_LDS uint32_t *rec = stage + (cnt + mbcnt64(mask)) * REC_DW;
                    rec[0] = col;
                    rec[1] = r;
                    rec[2] = (uint32_t)score;
                }
                cnt += (uint32_t)__popcll(mask);
            }
        }
    }
    flush_stage<0>(stage, cnt, P, T, 0, false, shard);
}

// -----------------------------------------------------------------------------
// k_neighbors_global_literal: the same pass with global_score_literal
// -----------------------------------------------------------------------------
// For matrices with an entry outside +-127 (no int8 profile).  Same tiles, same edges, one column per lane.
__global__ void __launch_bounds__(256)
k_neighbors_global_literal(const NeighborParams P, const uint32_t tile_base, const int32_t *__restrict__ Mg, int gap_open,
                           int gap_extend, int threshold) {
    constexpr int R = 16, STAGE_CAP = 128, REC_DW = 3;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    int *M = reinterpret_cast<int *>(smem);                                   // 576 dwords
    uint32_t *colseq = reinterpret_cast<uint32_t *>(smem + 2304);             // 256 x 9 dwords
    uint32_t *rowseq = colseq + 256 * SEQ_STRIDE_DW;                          // R x 8 dwords
    uint32_t *dp = rowseq + R * 8;                                            // 33 x 256 dwords: one DP line per lane
    uint32_t *stage_all = dp + 33 * 256;
    const Tile T = P.tiles[tile_base + blockIdx.x];
    const TileClass *Cp = P.classes + T.cls;
    const int la = Cp->la, lb = Cp->lb;
    const uint32_t shard = tile_shard(tile_base + blockIdx.x);
    const int tid = threadIdx.x;
    HMK_LDS uint32_t *stage = (HMK_LDS uint32_t *)stage_all + (tid >> 6) * (STAGE_CAP * REC_DW);
    for (int e = tid; e < 576; e += 256) M[e] = Mg[e];
    for (int e = tid; e < R * 8; e += 256) {
        const int r = e >> 3, q = e & 7;
        uint32_t v = 0;
        if ((uint32_t)r < T.nrows && (uint32_t)(q * 4) < P.lpad)
            v = reinterpret_cast<const uint32_t *>(P.res_sorted + (size_t)(T.row0 + r) * P.lpad)[q];
        rowseq[e] = v;
    }
    __syncthreads();
    uint32_t cnt = 0;
    const uint32_t col_end = T.col0 + T.ncols;
    uint32_t *mine = colseq + tid * SEQ_STRIDE_DW;
    for (uint32_t c0 = T.col0; c0 < col_end; c0 += 256) {
        const uint32_t col = c0 + tid;
        if (col < col_end) {
            const uint32_t *src = reinterpret_cast<const uint32_t *>(P.res_sorted + (size_t)col * P.lpad);
            for (uint32_t q = 0; q < P.lpad / 4; q++) mine[q] = src[q];
        }
        for (uint32_t r = 0; r < T.nrows; r++) {
            if (cnt > (uint32_t)(STAGE_CAP - 64)) {
                flush_stage<0>(stage, cnt, P, T, 0, false, shard);
                cnt = 0;
            }
            bool keep = col < col_end && global_keeps(T.diag, T.row0 + r, col);
            int score = 0;
            if (keep) {
                score = global_score_literal(M, reinterpret_cast<const uint8_t *>(rowseq + r * 8), la,
                                             reinterpret_cast<const uint8_t *>(mine), lb, gap_open, gap_extend, dp + tid, 256);
                keep = score >= threshold;
            }
            const uint64_t mask = __ballot(keep);
            if (mask != 0) {
                if (keep) {
                    HMK_LDS uint32_t *rec = stage + (cnt + mbcnt64(mask)) * REC_DW;
                    rec[0] = col;
                    rec[1] = r;
                    rec[2] = (uint32_t)score;
                }
                cnt += (uint32_t)__popcll(mask);
            }
        }
    }
    flush_stage<0>(stage, cnt, P, T, 0, false, shard);
}

// -----------------------------------------------------------------------------
// launcher
// -----------------------------------------------------------------------------
// literal: the matrix has an entry outside +-127; lbmax: the set's longest sequence
hipError_t launch_neighbors_global(int lbmax, bool literal, const NeighborParams &P, uint32_t tile_base, uint32_t n_tiles,
                                   const int32_t *d_matrix, int gap_open, int gap_extend, int threshold, hipStream_t s) {
    if (n_tiles == 0) return hipSuccess;
    if (literal) {
        const size_t lds = 2304 + 256 * SEQ_STRIDE_DW * 4 + 16 * 8 * 4 + 33 * 256 * 4 + 4 * 128 * 3 * 4;
        hipLaunchKernelGGL(k_neighbors_global_literal, dim3(n_tiles), dim3(256), lds, s, P, tile_base, d_matrix, gap_open, gap_extend,
                           threshold);
    } else if (lbmax <= 16) {
        hipLaunchKernelGGL((k_neighbors_global<16>), dim3(n_tiles), dim3(256), 0, s, P, tile_base, d_matrix, gap_open, gap_extend, threshold);
    } else {
        hipLaunchKernelGGL((k_neighbors_global<32>), dim3(n_tiles), dim3(256), 0, s, P, tile_base, d_matrix, gap_open, gap_extend, threshold);
    }
    return hipGetLastError();
}

}  // namespace hmk
