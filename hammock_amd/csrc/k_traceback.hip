// k_traceback.hip -- the gapped alignments behind GlobalAlignmentScorer's scores (hammock_hip.h: hmk_align_pairs_global).  One pair
// per lane: the recurrence of global_score_literal (hmk_device.h) in int32 with the DP line in registers, four direction bits per
// cell beside it in LDS, then one walk from (n, m) back to (0, 0) that reads one dword per step.
#include "hmk_device.h"
#include "hmk_grid.h"
#include "hmk_traceback.h"

namespace hmk {

// the direction bits of a cell (i, j >= 1; the boundaries need none)
//   bits 1..0  the first rule that holds for H[i][j]: 0 the diagonal, 1 E[i][j], 2 F[i][j]
//   bit  2     E[i][j] == E[i][j-1] + gap_extend   (an extension, preferred over an opening)
//   bit  3     F[i][j] == F[i-1][j] + gap_extend
enum { TB_DIAG = 0, TB_E = 1, TB_F = 2, TB_E_EXT = 4, TB_F_EXT = 8 };

// LMAX: the longest sequence (a multiple of 8), NT: lanes of a workgroup.  LDS: the matrix, seq1 of every lane (k_pairs' staging: the
// line loop reads one byte of it per line) and the bits as [line][dword][lane] -- eight cells of a line per dword, a lane's dwords NT
// apart, so the 64 lanes of a wave touch 64 consecutive dwords whatever cells they stand on.  seq2 and the DP line (H, F of the line
// above) live in registers: the column loop is unrolled, in groups of eight columns up to the longest seq2 of the wave, and columns
// beyond a lane's own seq2 hold values that no cell within it reads (residues beyond a sequence's end are 0 in res32).
// Nothing passes from one pair of a lane to its next: H, F and the bit dwords of every (line <= n, group <= m / 8) the walk can
// reach are written afresh, and the walk reads no other.
template <int LMAX, int NT>
__global__ void __launch_bounds__(NT)
k_traceback_global(const uint8_t *__restrict__ res32, const uint8_t *__restrict__ len, const int32_t *__restrict__ Mg,
                   const uint32_t *__restrict__ pi, const uint32_t *__restrict__ pj, uint64_t n_pairs, int gap_open, int gap_extend,
                   int32_t *__restrict__ score, uint8_t *__restrict__ n_cols, unsigned long long *__restrict__ gap1,
                   unsigned long long *__restrict__ gap2) {
    constexpr int NDW = LMAX / 8;
    __shared__ int M[576];
    __shared__ uint32_t seq1[NT * SEQ_STRIDE_DW];
    __shared__ uint32_t bits[LMAX * NDW * NT];
    const int tid = threadIdx.x;
    for (int e = tid; e < 576; e += NT) M[e] = Mg[e];
    __syncthreads();
    uint32_t *s1 = seq1 + tid * SEQ_STRIDE_DW;
    const uint8_t *s1b = reinterpret_cast<const uint8_t *>(s1);
    uint32_t *mybits = bits + tid;
    for (uint64_t base = (uint64_t)blockIdx.x * NT; base < n_pairs; base += (uint64_t)gridDim.x * NT) {   // (workgroup-uniform)
        const uint64_t k = base + tid;
        const bool ok = k < n_pairs;
        const uint32_t i1 = ok ? pi[k] : 0u, i2 = ok ? pj[k] : 0u;
        stage_sequence(s1, res32, i1);
        uint32_t w2[NDW * 2];   // seq2, four residues per dword
        {
            const u32x4 *src = reinterpret_cast<const u32x4 *>(res32 + (size_t)i2 * 32);
            const u32x4 lo = src[0];
            w2[0] = lo.x; w2[1] = lo.y; w2[2] = lo.z; w2[3] = lo.w;
            if constexpr (LMAX > 16) {
                const u32x4 hi = src[1];
                w2[4] = hi.x; w2[5] = hi.y;
                if constexpr (LMAX > 24) { w2[6] = hi.z; w2[7] = hi.w; }
            }
        }
        const int l1 = ok ? min((int)len[i1], LMAX) : 0, l2 = ok ? min((int)len[i2], LMAX) : 0;
        int wm = l2;   // the wave's longest seq2 (every lane of the wave is here)
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) wm = max(wm, __shfl_xor(wm, o, 64));
        const int ng = __builtin_amdgcn_readfirstlane((wm + 7) >> 3);

        int H[LMAX + 1], F[LMAX + 1];
        H[0] = 0;
#pragma unroll
        for (int col = 1; col <= LMAX; col++) { H[col] = gap_open + (col - 1) * gap_extend; F[col] = GLOBAL_NEG_INF; }   // line 0
        for (int line = 1; line <= l1; line++) {
            const int *Mrow = M + s1b[line - 1] * 24;
            int diag = H[0];                                    // H[line-1][0]
            int left = gap_open + (line - 1) * gap_extend;      // H[line][0]
            int e = GLOBAL_NEG_INF;                             // E[line][0]
            H[0] = left;
#pragma unroll
            for (int g = 0; g < NDW; g++) {
                if (g < ng) {   // (wave-uniform)
                    uint32_t word = 0;
#pragma unroll
                    for (int c = 0; c < 8; c++) {
                        const int col = 8 * g + c + 1;
                        const int r2 = (int)((w2[(col - 1) >> 2] >> (8 * ((col - 1) & 3))) & 0xFFu);
                        const int up_h = H[col], up_f = F[col];
                        const int e_ext = e + gap_extend, f_ext = up_f + gap_extend;
                        e = max(e_ext, left + gap_open);
                        const int f = max(f_ext, up_h + gap_open);
                        const int d = diag + Mrow[r2];
                        const int h = max(d, max(e, f));
                        uint32_t nib = h == d ? TB_DIAG : h == e ? TB_E : TB_F;
                        nib |= e == e_ext ? TB_E_EXT : 0u;
                        nib |= f == f_ext ? TB_F_EXT : 0u;
                        word |= nib << (4 * c);
                        H[col] = h;
                        F[col] = f;
                        diag = up_h;
                        left = h;
                    }
                    mybits[((line - 1) * NDW + g) * NT] = word;
                }
            }
        }
        int sc = H[0];   // H[l1][l2]
#pragma unroll
        for (int col = 1; col <= LMAX; col++) sc = col == l2 ? H[col] : sc;

        // the walk: columns leave right to left, so each one shifts the masks up and the leftmost ends in bit 0
        unsigned long long g1 = 0, g2 = 0;
        int i = l1, j = l2, state = TB_DIAG, nc = 0;   // state: TB_DIAG stands for H
        while (i > 0 || j > 0) {
            uint32_t b1, b2;   // this column's gap in seq1 / in seq2
            if (i == 0) { b1 = 1; b2 = 0; j--; }
            else if (j == 0) { b1 = 0; b2 = 1; i--; }
            else {
                const uint32_t nib = (mybits[((i - 1) * NDW + ((j - 1) >> 3)) * NT] >> (4 * ((j - 1) & 7))) & 15u;
                if (state == TB_DIAG) state = (int)(nib & 3u);
                if (state == TB_DIAG) { b1 = 0; b2 = 0; i--; j--; }
                else if (state == TB_E) { b1 = 1; b2 = 0; j--; state = nib & TB_E_EXT ? TB_E : TB_DIAG; }
                else { b1 = 0; b2 = 1; i--; state = nib & TB_F_EXT ? TB_F : TB_DIAG; }
            }
            g1 = (g1 << 1) | b1;
            g2 = (g2 << 1) | b2;
            nc++;
        }
        if (ok) {
            score[k] = sc;
            n_cols[k] = (uint8_t)nc;
            gap1[k] = g1;
            gap2[k] = g2;
        }
    }
}

// -----------------------------------------------------------------------------
// launcher
// -----------------------------------------------------------------------------
hipError_t launch_traceback_global(int lmax, const uint8_t *res32, const uint8_t *len, const int32_t *d_matrix, const uint32_t *pi,
                                   const uint32_t *pj, uint64_t n_pairs, int gap_open, int gap_extend, int32_t *score, uint8_t *n_cols,
                                   unsigned long long *gap1, unsigned long long *gap2, hipStream_t s) {
    if (n_pairs == 0) return hipSuccess;
    // the bits are LMAX^2 / 2 bytes per lane, and they bound the waves a CU holds: the smallest form that takes the set's longest sequence
    const uint32_t nt = lmax <= 16 ? 256u : 64u;
    uint64_t blocks = (n_pairs + nt - 1) / nt;
    if (blocks > 65536) blocks = 65536;
    blocks = capped_grid(lmax <= 16 ? "k_traceback_global<16>" : lmax <= 24 ? "k_traceback_global<24>" : "k_traceback_global<32>", (uint32_t)blocks);
    if (lmax <= 16)
        hipLaunchKernelGGL((k_traceback_global<16, 256>), dim3((uint32_t)blocks), dim3(256), 0, s, res32, len, d_matrix, pi, pj, n_pairs, gap_open,
                           gap_extend, score, n_cols, gap1, gap2);
    else if (lmax <= 24)
        hipLaunchKernelGGL((k_traceback_global<24, 64>), dim3((uint32_t)blocks), dim3(64), 0, s, res32, len, d_matrix, pi, pj, n_pairs, gap_open,
                           gap_extend, score, n_cols, gap1, gap2);
    else
        hipLaunchKernelGGL((k_traceback_global<32, 64>), dim3((uint32_t)blocks), dim3(64), 0, s, res32, len, d_matrix, pi, pj, n_pairs, gap_open,
                           gap_extend, score, n_cols, gap1, gap2);
    return hipGetLastError();
}

}  // namespace hmk
