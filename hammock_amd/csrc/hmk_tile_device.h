// hmk_tile_device.h -- what the tile kernels of k_local.hip, k_global.hip and the literal tier of k_neighbors.hip share: the profile
// tile frame (rows as query profiles in LDS, one column sequence per lane as profile offsets) and the literal tile kernel.
#ifndef HMK_TILE_DEVICE_H
#define HMK_TILE_DEVICE_H

#include "hmk_device.h"

namespace hmk {

// -----------------------------------------------------------------------------
// the profile tile frame
// -----------------------------------------------------------------------------
constexpr int TILE_ROWS = 16;   // rows per tile (PlanLocal) and per workgroup pass of a dense block

// the matrix as int8 and the residues of the rows [row0, row0 + nrows) (32 bytes each, zero beyond lpad and beyond nrows) into LDS
__device__ __forceinline__ void load_tile_rows(int8_t *m8, uint8_t *rowres, const int32_t *Mg, const uint8_t *res, uint32_t lpad,
                                               uint32_t row0, uint32_t nrows, int tid) {
    for (int e = tid; e < 576; e += 256) m8[e] = (int8_t)Mg[e];
    for (int e = tid; e < TILE_ROWS * 32; e += 256) {
        const uint32_t r = (uint32_t)e >> 5, k = e & 31;
        rowres[e] = (r < nrows && k < lpad) ? res[(size_t)(row0 + r) * lpad + k] : 0;
    }
}

// query profiles of R rows into LDS: entry (r, c, iq) = four int8 (score * scale) for lines 4 iq .. 4 iq + 3;
// -128 for the pad residue (c == 24) and for lines beyond the row's length
template <int R>
__device__ __forceinline__ void build_profiles(uint32_t *q, const int8_t *m8, const uint8_t *rowres, const int *row_len,
                                               uint32_t nrows, int scale, int tid) {
    for (int e = tid; e < R * 25 * 8; e += 256) {
        const int r = e / 200, rem = e - r * 200, c = rem >> 3, iq = rem & 7;
        const int l1 = (uint32_t)r < nrows ? row_len[r] : 0;
        uint32_t dw = 0;
        for (int k = 0; k < 4; k++) {
            const int i = iq * 4 + k;
            int v = -128;
            if (i < l1 && c < 24) v = m8[rowres[r * 32 + i] * 24 + c] * scale;
            dw |= ((uint32_t)v & 0xFFu) << (8 * k);
        }
        q[e] = dw;
    }
}

// its int16 twin (the packed DP, sw_row_pk): entry (r, c, strip) = four int16, 4 * score; row_len(r): the length of row r < nrows
template <int R, class RowLen>
__device__ __forceinline__ void build_profiles_i16(u32x2 *q, const int8_t *m8, const uint8_t *rowres, uint32_t nrows, int tid,
                                                   RowLen row_len) {
    for (int e = tid; e < R * 25 * 8; e += 256) {
        const int r = e / 200, rem = e - r * 200, c = rem >> 3, iq = rem & 7;
        const int l1 = (uint32_t)r < nrows ? row_len(r) : 0;
        uint32_t w[2] = {0, 0};
        for (int k = 0; k < 4; k++) {
            const int i = iq * 4 + k;
            int v = -128;
            if (i < l1 && c < 24) v = m8[rowres[r * 32 + i] * 24 + c] * 4;
            w[k >> 1] |= ((uint32_t)v & 0xFFFFu) << (16 * (k & 1));
        }
        q[e] = u32x2{w[0], w[1]};
    }
}

// This lane's column sequence (`col` of `res`, rows of lpad bytes; `ok`: there is one) -> the byte offsets of its residues' profile
// entries, STRIDE bytes per residue (32: int8 profiles, 64: int16); the pad residue 24 at and beyond `len`, and where !ok.
template <int LBMAX, int STRIDE>
__device__ __forceinline__ void column_offsets(const uint8_t *res, uint32_t lpad, uint32_t col, bool ok, int len,
                                               uint32_t (&boff)[LBMAX]) {
    uint32_t words[8];
#pragma unroll
    for (int q = 0; q < 8; q++) words[q] = 0;
    if (ok) {
        const u32x4 *src = reinterpret_cast<const u32x4 *>(res + (size_t)col * lpad);
        const u32x4 v0 = src[0];
        words[0] = v0.x; words[1] = v0.y; words[2] = v0.z; words[3] = v0.w;
        if (LBMAX > 16) {
            const u32x4 v1 = src[1];
            words[4] = v1.x; words[5] = v1.y; words[6] = v1.z; words[7] = v1.w;
        }
    }
#pragma unroll
    for (int j = 0; j < LBMAX; j++) {
        const uint32_t c = (ok && j < len) ? ((words[j >> 2] >> ((j & 3) * 8)) & 0xFFu) : 24u;
        boff[j] = c * (uint32_t)STRIDE;
    }
}

// -----------------------------------------------------------------------------
// the literal tile kernel: one of hmk_device.h's literal scorers on the tiles of a plan, one column per lane
// -----------------------------------------------------------------------------
// Dynamic LDS of the kernel, in bytes from its start.  The kernel and its launcher both take them from here.
template <bool DP_LINE>
struct LiteralTile {
    static constexpr int STAGE_CAP = 128;
    static constexpr int M = 0;                                          // int32[576]
    static constexpr int COLSEQ = M + 576 * 4;                           // 256 lanes x SEQ_STRIDE_DW dwords
    static constexpr int ROWSEQ = COLSEQ + 256 * SEQ_STRIDE_DW * 4;      // TILE_ROWS x 8 dwords
    static constexpr int DP = ROWSEQ + TILE_ROWS * 8 * 4;                // 33 x 256 dwords: one DP line per lane (DP_LINE)
    static constexpr int STAGE = DP + (DP_LINE ? 33 * 256 * 4 : 0);
    static constexpr int BYTES = STAGE + HitStage<STAGE_CAP>::BYTES;
};

// The body of the three literal kernels.  Scorer: DP_LINE, and score(M, row, la, col, lb, dp) -- the score the edge of (row, column)
// carries, i.e. which of the two is seq1 is the scorer's business; dp: this lane's DP line (stride 256 dwords) where DP_LINE.
template <class Scorer>
__device__ __forceinline__ void literal_tile(const NeighborParams &P, uint32_t tile, const int32_t *__restrict__ Mg, const Scorer &scorer,
                                             int threshold) {
    using L = LiteralTile<Scorer::DP_LINE>;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    int *M = reinterpret_cast<int *>(smem + L::M);
    uint32_t *colseq = reinterpret_cast<uint32_t *>(smem + L::COLSEQ);
    uint32_t *rowseq = reinterpret_cast<uint32_t *>(smem + L::ROWSEQ);
    uint32_t *dp = reinterpret_cast<uint32_t *>(smem + L::DP);

    const Tile T = P.tiles[tile];
    const TileClass *Cp = P.classes + T.cls;
    const int la = Cp->la, lb = Cp->lb;
    const int tid = threadIdx.x;
    HitStage<L::STAGE_CAP> hits(reinterpret_cast<uint32_t *>(smem + L::STAGE), P, T, tile_shard(tile));

    for (int e = tid; e < 576; e += 256) M[e] = Mg[e];
    for (int e = tid; e < TILE_ROWS * 8; e += 256) {
        const int r = e >> 3, q = e & 7;
        uint32_t v = 0;
        if ((uint32_t)r < T.nrows && (uint32_t)(q * 4) < P.lpad)
            v = reinterpret_cast<const uint32_t *>(P.res_sorted + (size_t)(T.row0 + r) * P.lpad)[q];
        rowseq[e] = v;
    }
    __syncthreads();

    const uint32_t col_end = T.col0 + T.ncols;
    uint32_t *mine = colseq + tid * SEQ_STRIDE_DW;
    for (uint32_t c0 = T.col0; c0 < col_end; c0 += 256) {
        const uint32_t col = c0 + tid;
        if (col < col_end) {
            const uint32_t *src = reinterpret_cast<const uint32_t *>(P.res_sorted + (size_t)col * P.lpad);
            for (uint32_t q = 0; q < P.lpad / 4; q++) mine[q] = src[q];
        }
        for (uint32_t r = 0; r < T.nrows; r++) {
            bool keep = col < col_end && tile_keeps(T.diag, T.row0 + r, col);
            int score = 0;
            if (keep) {
                score = scorer.score(M, reinterpret_cast<const uint8_t *>(rowseq + r * 8), la, reinterpret_cast<const uint8_t *>(mine), lb,
                                     dp + tid);
                keep = score >= threshold;
            }
            hits.put(keep, col, r, score);
        }
    }
    hits.drain();
}

}  // namespace hmk
#endif
