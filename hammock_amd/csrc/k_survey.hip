// k_survey.hip -- the score survey of a pair space of the uploaded set (hmk_score_survey_shifted, hmk_survey.cpp): the histogram of the
// ShiftedScorer scores, per row its best partner and the number of its partners at or above a threshold.  Every pair is scored once by
// the literal scorer (shifted_score_literal, hmk_device.h) and reduced on the device; nothing proportional to pairs or tiles is stored:
//   k_survey_init     the accumulators of the call
//   k_survey_tiled    LINK_TILE x LINK_TILE tiles, a tile's rows in LDS, one column per lane (the walk of k_linkage_tiled)
//                       triangle   rows and columns are places of the one range, tiles on or below the diagonal, the pairs row place >
//                                  column place, seq1 = the row (the larger index); both ends of a pair take part in the row outputs
//                       rectangle  rows are references, columns are queries, all tiles, seq1 = the column (the query); only the queries
//                                  have row outputs, so only the lanes' own reductions run
//   k_survey_decode   best_score / best_index from the rows' keys
// Integer adds, minima and maxima only: no result depends on the schedule.
#include <algorithm>

#include "hmk_link_device.h"
#include "hmk_survey.h"
#include "hmk_grid.h"

namespace hmk {

namespace {

// the largest score, then the smallest partner; 0 is below every key (a partner is below 2^24)
__device__ __forceinline__ unsigned long long survey_key(int score, uint32_t partner) {
    return ((unsigned long long)(uint32_t)(score + 32768) << 32) | (unsigned long long)(0xFFFFFFFFu - partner);
}

// tile t = i (i + 1) / 2 + j, j <= i (link_tile_decode's arithmetic for one slot)
__device__ __forceinline__ void tri_tile(uint32_t t, uint32_t &i, uint32_t &j) {
    i = (uint32_t)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while (i > 0 && (uint64_t)i * (i + 1) / 2 > t) i--;
    while ((uint64_t)(i + 1) * (i + 2) / 2 <= t) i++;
    j = t - (uint32_t)((uint64_t)i * (i + 1) / 2);
}

}  // namespace

// The workgroup's histogram.  Scores concentrate (a seventh of a wave-instruction's lanes on one bin for random peptides, all 64 for
// copies of one string), so a bin is kept SURVEY_COPIES times, lane l adding to copy l % SURVEY_COPIES; the copies of a bin lie in
// neighbouring banks.  HIST_WAVE instead adds once per distinct bin of a wave-instruction (wave_groups), into one copy.
constexpr int SURVEY_COPIES = 4;
enum { HIST_NONE = 0, HIST_COPIES = 1, HIST_WAVE = 2 };

// -----------------------------------------------------------------------------
// accumulators: cleared by every call, so that no state survives one
// -----------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_survey_init(SurveyAcc acc, uint32_t n_bins, uint32_t nq) {
    const uint32_t n = max(max(n_bins, acc.rowkey ? nq : 0u), (uint32_t)SURVEY_COUNTS);
    for (uint32_t k = blockIdx.x * 256 + threadIdx.x; k < n; k += gridDim.x * 256) {
        if (k < n_bins) acc.hist[k] = 0;
        if (k < (uint32_t)SURVEY_COUNTS) acc.counts[k] = 0;
        if (k < 2) acc.range[k] = k ? INT32_MIN : INT32_MAX;
        if (acc.rowkey && k < nq) { acc.rowkey[k] = 0; acc.degree[k] = 0; }
    }
}

// -----------------------------------------------------------------------------
// the pairs
// -----------------------------------------------------------------------------
// Column side (both pair spaces): the lane keeps its column's key and count over the tile's rows -- the rows ascend, so of equal scores
// the first row, the smallest partner, stays -- and sends one global atomic each per tile.  Row side (triangle): a row's largest score
// over the wave's 64 columns is a wave reduction, its first lane at that score the smallest partner (the columns ascend with the lanes),
// its count a ballot; lane (row & 63) keeps them until the wave has done 64 rows, then one LDS atomic per row and wave, then one global
// atomic per row and tile (k_align_sums_tiled's scheme).
// Histogram: 32-bit counters in LDS, cleared at the head of every tile and flushed at its end with one 64-bit global add per non-zero
// bin.  A tile holds at most LINK_TILE^2 = 65,536 pairs, so no counter -- bin copy, below or above -- can pass 65,536 between two flushes.
// The counters are the kernel's dynamic LDS, n_bins x copies of them (4 KB at 256 bins): sized by the limit of 1,024 bins, 16 KB, they took
// the kernel from 6 to 4 workgroups per CU, and that, not the atomics, was what the histogram cost.
template <bool TRI, int HFORM, bool ROWS>
__global__ void __launch_bounds__(256)
k_survey_tiled(const uint8_t *__restrict__ res32, const uint8_t *__restrict__ len, const int32_t *__restrict__ Mg, uint32_t q0, uint32_t nq,
               uint32_t r0, uint32_t nr, uint32_t n_tiles, uint32_t tiles_across, int X, int p, int thr, int lo, uint32_t n_bins,
               SurveyAcc acc) {
    constexpr int T = LINK_TILE;
    static_assert(T == 256, "a tile is as wide as the block");
    constexpr bool HIST = HFORM != HIST_NONE;
    constexpr int COPIES = HFORM == HIST_COPIES ? SURVEY_COPIES : 1;
    constexpr bool ROW_SIDE = TRI && ROWS;
    __shared__ __attribute__((aligned(16))) int M[576];
    __shared__ __attribute__((aligned(16))) uint32_t colseq[T * SEQ_STRIDE_DW];
    __shared__ __attribute__((aligned(16))) uint32_t rowseq[T * 8];
    __shared__ uint8_t rowlen[T];
    __shared__ unsigned long long rkey[ROW_SIDE ? T : 1];
    __shared__ uint32_t rdeg[ROW_SIDE ? T : 1];
    extern __shared__ uint32_t lhist[];   // n_bins * COPIES counters (launch_form sizes it)
    __shared__ uint32_t ltail[2];   // pairs below / above the window
    const int tid = threadIdx.x;
    const uint32_t lane = tid & 63u, wave = tid >> 6;
    for (int e = tid; e < 576; e += 256) M[e] = Mg[e];
    uint32_t *mine = colseq + tid * SEQ_STRIDE_DW;
    const uint32_t rbase = TRI ? q0 : r0, n_rows_all = TRI ? nq : nr;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        uint32_t i, j;
        if (TRI) tri_tile(tile, i, j);
        else { i = tile / tiles_across; j = tile - i * tiles_across; }
        const uint32_t row0 = i * T, col0 = j * T;           // places in the ranges; row0 < n_rows_all, col0 < nq
        const uint32_t nrows = min((uint32_t)T, n_rows_all - row0), ncols = min((uint32_t)T, nq - col0);
        __syncthreads();   // the matrix stands; the last tile's rows and bins have been flushed
        if ((uint32_t)tid < nrows) {
            const uint32_t idx = rbase + row0 + tid;
            link_stage_row(rowseq, tid, res32, idx);
            rowlen[tid] = len[idx];
        }
        if (ROW_SIDE) { rkey[tid] = 0; rdeg[tid] = 0; }
        if (HIST) {
            for (uint32_t e = tid; e < n_bins * COPIES; e += 256) lhist[e] = 0;
            if (tid < 2) ltail[tid] = 0;
        }
        const bool has_col = (uint32_t)tid < ncols;
        const uint32_t cidx = q0 + col0 + tid;
        int clen = 0;
        if (has_col) {
            stage_sequence(mine, res32, cidx);
            clen = len[cidx];
        }
        __syncthreads();
        // the wave's rows: on the triangle's diagonal tile a row counts for the wave only beyond the wave's first column
        const uint32_t r_first = (TRI && i == j) ? wave * 64 + 1 : 0;
        const bool wave_has_cols = wave * 64 < ncols;
        unsigned long long ckey = 0;
        uint32_t cnt = 0, below = 0, above = 0;
        int smin = INT32_MAX, smax = INT32_MIN;
        if (wave_has_cols && r_first < nrows) {
#pragma unroll 1
            for (uint32_t q = r_first >> 6; q * 64 < nrows; q++) {
                unsigned long long acc_key = 0;
                uint32_t acc_deg = 0;
#pragma unroll 1
                for (uint32_t r = max(q * 64, r_first); r < min(q * 64 + 64, nrows); r++) {
                    const bool active = has_col && (!TRI || col0 + (uint32_t)tid < row0 + r);
                    int score = INT32_MIN;
                    bool hit = false;
                    uint32_t bin = 0xFFFFFFFFu;
                    if (active) {
                        const uint8_t *rs = reinterpret_cast<const uint8_t *>(rowseq + r * 8), *cs = reinterpret_cast<const uint8_t *>(mine);
                        score = TRI ? shifted_score_literal(M, rs, rowlen[r], cs, clen, X, p)
                                    : shifted_score_literal(M, cs, clen, rs, rowlen[r], X, p);
                        hit = score >= thr;
                        if (hit) cnt++;
                        smin = min(smin, score);
                        smax = max(smax, score);
                        if (ROWS) {
                            const unsigned long long kk = survey_key(score, rbase + row0 + r);
                            if (kk > ckey) ckey = kk;
                        }
                        if (HIST) {
                            const int d = score - lo;   // (|score| <= 32,768 and |lo| <= 100,000)
                            if (d < 0) below++;
                            else if (d >= (int)n_bins) above++;
                            else bin = (uint32_t)d;
                        }
                    }
                    if (HFORM == HIST_COPIES) {
                        if (bin != 0xFFFFFFFFu) atomicAdd(&lhist[bin * COPIES + (lane & (COPIES - 1))], 1u);
                    } else if (HFORM == HIST_WAVE) {
                        const WaveGroup g = wave_groups(bin, bin != 0xFFFFFFFFu);
                        if (bin != 0xFFFFFFFFu && g.rank == 0) atomicAdd(&lhist[bin], g.size);
                    }
                    if (ROW_SIDE) {
                        int wmax = score;
#pragma unroll
                        for (int d = 32; d >= 1; d >>= 1) wmax = max(wmax, __shfl_xor(wmax, d));
                        const unsigned long long at_max = __ballot(active && score == wmax);
                        const uint32_t nhit = (uint32_t)__popcll(__ballot(hit));
                        if (lane == (r & 63u)) {
                            acc_deg = nhit;
                            acc_key = at_max ? survey_key(wmax, q0 + col0 + wave * 64 + (uint32_t)(__ffsll((long long)at_max) - 1)) : 0;
                        }
                    }
                }
                if (ROW_SIDE && acc_key) {
                    atomicMax(&rkey[q * 64 + lane], acc_key);
                    if (acc_deg) atomicAdd(&rdeg[q * 64 + lane], acc_deg);
                }
            }
        }
        // the column side
        if (ROWS && ckey) {
            atomicMax(&acc.rowkey[cidx - q0], ckey);
            if (cnt) atomicAdd(&acc.degree[cidx - q0], cnt);
        }
        if (HIST) {
            if (below) atomicAdd(&ltail[0], below);
            if (above) atomicAdd(&ltail[1], above);
        }
        // the call's totals: one atomic per wave
        uint32_t wcnt = cnt;
        int wmin = smin, wmaxs = smax;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            wcnt += __shfl_xor(wcnt, d);
            wmin = min(wmin, __shfl_xor(wmin, d));
            wmaxs = max(wmaxs, __shfl_xor(wmaxs, d));
        }
        if (lane == 0 && wmin != INT32_MAX) {
            atomicMin(&acc.range[0], wmin);
            atomicMax(&acc.range[1], wmaxs);
            if (wcnt) atomicAdd(&acc.counts[SURVEY_AT_OR_ABOVE], (unsigned long long)wcnt);
        }
        if (ROW_SIDE || HIST) __syncthreads();
        if (ROW_SIDE) {
            if ((uint32_t)tid < nrows && rkey[tid]) {
                atomicMax(&acc.rowkey[row0 + tid], rkey[tid]);
                if (rdeg[tid]) atomicAdd(&acc.degree[row0 + tid], rdeg[tid]);
            }
        }
        if (HIST) {
            for (uint32_t b = tid; b < n_bins; b += 256) {
                uint32_t v = 0;
#pragma unroll
                for (int c = 0; c < COPIES; c++) v += lhist[b * COPIES + c];
                if (v) atomicAdd(&acc.hist[b], (unsigned long long)v);
            }
            if (tid < 2 && ltail[tid]) atomicAdd(&acc.counts[tid], (unsigned long long)ltail[tid]);
        }
    }
}

// -----------------------------------------------------------------------------
// the rows' keys -> best_score, best_index
// -----------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_survey_decode(SurveyAcc acc, uint32_t nq) {
    for (uint32_t k = blockIdx.x * 256 + threadIdx.x; k < nq; k += gridDim.x * 256) {
        const unsigned long long key = acc.rowkey[k];
        acc.best_score[k] = key ? (int)(uint32_t)(key >> 32) - 32768 : INT32_MIN;
        acc.best_index[k] = key ? 0xFFFFFFFFu - (uint32_t)key : 0xFFFFFFFFu;
    }
}

// -----------------------------------------------------------------------------
// launchers
// -----------------------------------------------------------------------------
uint32_t survey_tiles(bool triangle, uint32_t nq, uint32_t nr) {   // (n <= 2^24: at most 2^31 + 2^15 tiles)
    const uint64_t tq = ((uint64_t)nq + LINK_TILE - 1) / LINK_TILE, tr = ((uint64_t)nr + LINK_TILE - 1) / LINK_TILE;
    return (uint32_t)(triangle ? tq * (tq + 1) / 2 : tq * tr);
}

hipError_t launch_survey_init(const SurveyAcc &acc, uint32_t n_bins, uint32_t nq, hipStream_t s) {
    const uint32_t n = std::max(std::max(n_bins, acc.rowkey ? nq : 0u), (uint32_t)SURVEY_COUNTS);
    const uint32_t blocks = capped_grid("k_survey_init", std::min<uint32_t>((n + 255) / 256, 4096));
    hipLaunchKernelGGL(k_survey_init, dim3(blocks), dim3(256), 0, s, acc, n_bins, nq);
    return hipGetLastError();
}

namespace {

template <bool TRI, int HFORM, bool ROWS>
void launch_form(uint32_t blocks, hipStream_t s, const uint8_t *res32, const uint8_t *len, const int32_t *d_matrix, uint32_t q0, uint32_t nq,
                 uint32_t r0, uint32_t nr, uint32_t n_tiles, uint32_t across, int X, int p, int thr, int lo, uint32_t n_bins,
                 const SurveyAcc &acc) {
    hipLaunchKernelGGL((k_survey_tiled<TRI, HFORM, ROWS>), dim3(blocks), dim3(256), (size_t)n_bins * (HFORM == HIST_COPIES ? SURVEY_COPIES : 1) * 4, s, res32, len, d_matrix, q0, nq, r0, nr, n_tiles, across, X,
                       p, thr, lo, n_bins, acc);
}

template <bool TRI, typename... A>
void launch_side(int hform, bool rows, A... a) {
    if (hform == HIST_NONE) launch_form<TRI, HIST_NONE, true>(a...);
    else if (hform == HIST_COPIES) { if (rows) launch_form<TRI, HIST_COPIES, true>(a...); else launch_form<TRI, HIST_COPIES, false>(a...); }
    else { if (rows) launch_form<TRI, HIST_WAVE, true>(a...); else launch_form<TRI, HIST_WAVE, false>(a...); }
}

}  // namespace

hipError_t launch_survey_tiled(const uint8_t *res32, const uint8_t *len, const int32_t *d_matrix, bool triangle, uint32_t q0, uint32_t nq,
                               uint32_t r0, uint32_t nr, int X, int p, int thr, int score_lo, uint32_t n_bins, int hist_form,
                               const SurveyAcc &acc, hipStream_t s) {
    const uint32_t n_tiles = survey_tiles(triangle, nq, nr);
    const bool rows = acc.rowkey != nullptr;
    if (n_tiles == 0) return hipSuccess;
    if ((n_bins == 0 && !rows) || n_bins > HMK_SURVEY_MAX_BINS) return hipErrorInvalidValue;   // (the bins size the dynamic LDS)
    const int hform = n_bins == 0 ? HIST_NONE : hist_form == SURVEY_HIST_WAVE ? HIST_WAVE : HIST_COPIES;
    const uint32_t across = (nq + LINK_TILE - 1) / LINK_TILE;
    const uint32_t blocks = capped_grid("k_survey_tiled", std::min<uint32_t>(n_tiles, 65536));
    if (triangle) launch_side<true>(hform, rows, blocks, s, res32, len, d_matrix, q0, nq, r0, nr, n_tiles, across, X, p, thr, score_lo, n_bins, acc);
    else launch_side<false>(hform, rows, blocks, s, res32, len, d_matrix, q0, nq, r0, nr, n_tiles, across, X, p, thr, score_lo, n_bins, acc);
    return hipGetLastError();
}

hipError_t launch_survey_decode(const SurveyAcc &acc, uint32_t nq, hipStream_t s) {
    if (nq == 0 || !acc.rowkey) return hipSuccess;
    const uint32_t blocks = capped_grid("k_survey_decode", std::min<uint32_t>((nq + 255) / 256, 4096));
    hipLaunchKernelGGL(k_survey_decode, dim3(blocks), dim3(256), 0, s, acc, nq);
    return hipGetLastError();
}

}  // namespace hmk
