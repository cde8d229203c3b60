// hmk_survey.h -- launchers of k_survey.hip (the score survey of a triangle or a rectangle of the uploaded set: histogram, best partner and
// degree per row), used by hmk_survey.cpp.
#ifndef HMK_SURVEY_H
#define HMK_SURVEY_H

#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace hmk {

// The accumulators of one call.  hist[n_bins] counts the pairs scoring score_lo + k; counts = {pairs below the window, pairs above it, pairs
// at or above the threshold}; range = {smallest score, largest score}.  Per row [q - q0]: rowkey takes (score + 32768) << 32 |
// (0xFFFFFFFF - partner) under a 64-bit maximum (the largest score, then the smallest partner index; 0: no partner), degree the partners at
// or above the threshold; best_score / best_index are the decoded key (k_survey_decode).  rowkey == null: no row outputs.
struct SurveyAcc {
    unsigned long long *hist;
    unsigned long long *counts;
    int32_t *range;
    unsigned long long *rowkey;
    uint32_t *degree;
    int32_t *best_score;
    uint32_t *best_index;
};
enum { SURVEY_BELOW = 0, SURVEY_ABOVE = 1, SURVEY_AT_OR_ABOVE = 2, SURVEY_COUNTS = 3 };

// the tiles of a call: LINK_TILE x LINK_TILE pairs each; the triangle's on or below the diagonal of its one range, the rectangle's all
uint32_t survey_tiles(bool triangle, uint32_t nq, uint32_t nr);

// hist = 0, counts = 0, range = {INT32_MAX, INT32_MIN}; rowkey = 0, degree = 0
hipError_t launch_survey_init(const SurveyAcc &acc, uint32_t n_bins, uint32_t nq, hipStream_t s);
// Every pair of the triangle inside [q0, q0 + nq) (seq1 = the larger index) or of the rectangle [q0, q0 + nq) x [r0, r0 + nr) (seq1 = the
// query) scored once by the literal scorer and reduced into acc.  n_bins == 0: the form without the histogram; acc.rowkey == null: the
// form without the row reductions (one of the two is wanted).  threshold and score_lo within +-100,000 (the caller clamps them: no score
// leaves int16).  hist_form: how a workgroup's LDS histogram takes a wave-instruction's scores (DESIGN.md 5.18 has both measured).
enum { SURVEY_HIST_COPIES = 0,   // one add per lane, each bin kept four times, lane l adding to copy l % 4 (what every call runs)
       SURVEY_HIST_WAVE = 1 };   // one add per distinct bin of the wave-instruction (wave_groups), one copy
hipError_t launch_survey_tiled(const uint8_t *res32, const uint8_t *len, const int32_t *d_matrix, bool triangle, uint32_t q0, uint32_t nq,
                               uint32_t r0, uint32_t nr, int X, int p, int thr, int score_lo, uint32_t n_bins, int hist_form,
                               const SurveyAcc &acc, hipStream_t s);
// best_score / best_index from rowkey (INT32_MIN / UINT32_MAX for a row without a partner)
hipError_t launch_survey_decode(const SurveyAcc &acc, uint32_t nq, hipStream_t s);

}  // namespace hmk
#endif
