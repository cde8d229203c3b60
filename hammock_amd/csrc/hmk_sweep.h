// hmk_sweep.h -- launchers of k_sweep.hip (the packed edges of one neighbour pass dealt into one run per threshold level, whole
// edges, the top level first), used by hmk_sweep.cpp (hmk_greedy_sweep*).
#ifndef HMK_SWEEP_H
#define HMK_SWEEP_H

#include <hip/hip_runtime_api.h>

#include "hmk_internal.h"

namespace hmk {

constexpr uint32_t SWEEP_MAX_LEVELS = 256;     // threshold_hi - threshold <= 255
constexpr uint32_t SWEEP_MAX_GRID = 2048;      // workgroups of k_sweep_hist / k_sweep_deal (8 per compute unit of 256)
constexpr uint32_t SWEEP_FLUSH_CHUNKS = 1u << 21;   // k_sweep_hist adds its LDS counters to the global ones after that many chunks:
                                                    // 2^31 edges at most in one 32-bit counter

// The per-call device block (SB_SWEEP_STATE), zeroed at the start of a call.  Level l = min(score, threshold_hi) - threshold.
//   hist     edges per level
//   start    where level l's run begins in the dealt buffer: the runs lie from the top level down, start[l] = the edges of the levels
//            above l; cursor: where the next chunk's edges of level l go
//   prefix   prefix[l] = start[l] + hist[l] = the edges with score >= threshold + l: they are dealt[0 .. prefix[l])
//   flag     non-zero once an edge named an index >= n or a self pair
// prefix and flag lie together: the host reads them in one copy.
struct SweepState {
    unsigned long long hist[SWEEP_MAX_LEVELS];
    unsigned long long start[SWEEP_MAX_LEVELS];
    unsigned long long cursor[SWEEP_MAX_LEVELS];
    unsigned long long prefix[SWEEP_MAX_LEVELS];
    unsigned long long flag;
};

// level of an edge = min(score, thr_hi) - thr into st->hist; edges below thr are left out, invalid ones (index >= n, self pair)
// flagged and left out
hipError_t launch_sweep_hist(const EdgeRuns &E, uint32_t n, int thr, int thr_hi, SweepState *st, hipStream_t s);
// start, cursor and prefix from hist (one workgroup)
hipError_t launch_sweep_scan(uint32_t n_levels, SweepState *st, hipStream_t s);
// every counted edge, all 8 bytes of it, into its level's run of `dealt`
hipError_t launch_sweep_deal(const EdgeRuns &E, uint32_t n, int thr, int thr_hi, SweepState *st, uint64_t *dealt, hipStream_t s);

}  // namespace hmk
#endif
