// hmk_traceback.h -- the launcher of k_traceback.hip (the gapped alignments behind GlobalAlignmentScorer's scores: direction bits beside
// the DP, then one walk back per pair) and the host call on top of it (hmk_traceback.cpp).
#ifndef HMK_TRACEBACK_H
#define HMK_TRACEBACK_H

#include <hip/hip_runtime_api.h>
#include <stdint.h>

struct hmk_ctx;

namespace hmk {

// One pair per lane: score[k] = global(seq1 = pi[k], seq2 = pj[k]); n_cols[k], gap1[k], gap2[k] = the alignment the walk of
// hammock_hip.h (hmk_align_pairs_global) finds.  lmax: the set's longest sequence (<= 16, <= 24 and <= 32 have an instantiation each).
hipError_t launch_traceback_global(int lmax, const uint8_t *res32, const uint8_t *len, const int32_t *d_matrix, const uint32_t *pi,
                                   const uint32_t *pj, uint64_t n_pairs, int gap_open, int gap_extend, int32_t *score, uint8_t *n_cols,
                                   unsigned long long *gap1, unsigned long long *gap2, hipStream_t s);

namespace impl {
// hmk_align_pairs_global behind its null-context check
int align_pairs_global(hmk_ctx *ctx, const uint32_t *i, const uint32_t *j, uint64_t n_pairs, int gap_open, int gap_extend, int32_t *score,
                       uint8_t *n_cols, uint64_t *gap1, uint64_t *gap2);
}

}  // namespace hmk
#endif
