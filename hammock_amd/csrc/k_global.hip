// k_global.hip -- GlobalAlignmentScorer (Gotoh's global alignment with affine gaps, hmk_device.h: global_score_literal) on the
// length-bucketed tiles of the LocalAlignmentScorer plans: register-resident striped DP and the literal form, thresholded
// pairs -> edge list.
#include "hmk_tile_device.h"

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
    constexpr int R = TILE_ROWS;
    constexpr int QROW = 25 * 8 * 4;
    constexpr int STAGE_CAP = 128;
    __shared__ __attribute__((aligned(16))) uint8_t smem[R * QROW + 576 + R * 32 + HitStage<STAGE_CAP>::BYTES];
    int8_t *m8 = reinterpret_cast<int8_t *>(smem + R * QROW);
    uint8_t *rowres = smem + R * QROW + 576;
    const Tile T = P.tiles[tile_base + blockIdx.x];
    const TileClass *Cp = P.classes + T.cls;
    const int la = Cp->la, lb = Cp->lb;   // la: row (seq1) length, lb: column (seq2) length
    const int tid = threadIdx.x;
    HitStage<STAGE_CAP> hits(reinterpret_cast<uint32_t *>(smem + R * QROW + 576 + R * 32), P, T, tile_shard(tile_base + blockIdx.x));

    load_tile_rows(m8, rowres, Mg, P.res_sorted, P.lpad, T.row0, T.nrows, tid);
    __syncthreads();
    __shared__ int row_len[R];
    if (tid < R) row_len[tid] = (uint32_t)tid < T.nrows ? la : 0;
    __syncthreads();
    build_profiles<R>(reinterpret_cast<uint32_t *>(smem), m8, rowres, row_len, T.nrows, 1, tid);
    __syncthreads();

    const uint32_t q_addr = lds_addr(smem);
    const uint32_t col_end = T.col0 + T.ncols;
    const uint32_t wave_last = (uint32_t)__builtin_amdgcn_readfirstlane(tid) | 63u;   // the wave's last lane
    for (uint32_t c0 = T.col0; c0 < col_end; c0 += 256) {
        const uint32_t col = c0 + tid;
        const bool col_ok = col < col_end;
        uint32_t boff[LBMAX];
        column_offsets<LBMAX, 32>(P.res_sorted, P.lpad, col, col_ok, lb, boff);
        for (uint32_t r = 0; r < T.nrows; r++) {
            if (T.diag == 1 && c0 + wave_last <= T.row0 + r) continue;   // a triangle tile: none of this wave's columns is beyond the row
            const int score = global_row<LBMAX>(q_addr + r * QROW, la, lb, boff, gap_open, gap_extend);
            hits.put(col_ok && score >= threshold && tile_keeps(T.diag, T.row0 + r, col), col, r, score);
        }
    }
    hits.drain();
}

// -----------------------------------------------------------------------------
// k_neighbors_global_literal: the same pass with global_score_literal
// -----------------------------------------------------------------------------
// For matrices with an entry outside +-127 (no int8 profile).  Same tiles, same edges, one column per lane: the literal tile
// kernel of hmk_tile_device.h.
struct GlobalLiteral {
    static constexpr bool DP_LINE = true;
    int gap_open, gap_extend;
    __device__ __forceinline__ int score(const int *M, const uint8_t *row, int la, const uint8_t *col, int lb, uint32_t *dp) const {
        return global_score_literal(M, row, la, col, lb, gap_open, gap_extend, dp, 256);
    }
};

__global__ void __launch_bounds__(256)
k_neighbors_global_literal(const NeighborParams P, const uint32_t tile_base, const int32_t *__restrict__ Mg, int gap_open,
                           int gap_extend, int threshold) {
    literal_tile(P, tile_base + blockIdx.x, Mg, GlobalLiteral{gap_open, gap_extend}, threshold);
}

// -----------------------------------------------------------------------------
// launcher
// -----------------------------------------------------------------------------
// literal: the matrix has an entry outside +-127; lbmax: the set's longest sequence
hipError_t launch_neighbors_global(int lbmax, bool literal, const NeighborParams &P, uint32_t tile_base, uint32_t n_tiles,
                                   const int32_t *d_matrix, int gap_open, int gap_extend, int threshold, hipStream_t s) {
    if (n_tiles == 0) return hipSuccess;
    if (literal) {
        hipLaunchKernelGGL(k_neighbors_global_literal, dim3(n_tiles), dim3(256), LiteralTile<GlobalLiteral::DP_LINE>::BYTES, s, P, tile_base, d_matrix,
                           gap_open, gap_extend, threshold);
    } else if (lbmax <= 16) {
        hipLaunchKernelGGL((k_neighbors_global<16>), dim3(n_tiles), dim3(256), 0, s, P, tile_base, d_matrix, gap_open, gap_extend, threshold);
    } else {
        hipLaunchKernelGGL((k_neighbors_global<32>), dim3(n_tiles), dim3(256), 0, s, P, tile_base, d_matrix, gap_open, gap_extend, threshold);
    }
    return hipGetLastError();
}

}  // namespace hmk
