// hmk_sizing.h -- the sizing rules every clustering call depends on, each written once as a pure function of plain numbers: the band
// request, the adjacency entry format, the edge buffer's first capacity and its capacity after an overflow.  No HIP header and no
// context: the host compiler alone builds it (tests/tools/sizing_probe.cpp does).
#ifndef HMK_SIZING_H
#define HMK_SIZING_H
#include <stdint.h>

#include <algorithm>

#include "../../include/hammock_hip.h"

namespace hmk { namespace sizing {

// Band: phase 1 of the merge (LimitedGreedySequenceClusterer.java:77-120) reads the adjacency rows in order and stops once
// maxClusters clusters exist, normally a little after row maxClusters.  -> the rows whose tiles a pass launches first (0: no
// band -- a small input, no cluster limit, or a band that would be most of the pass).
inline int64_t band_request(uint32_t n, int64_t max_clusters) {
    if (max_clusters <= 0 || n < 16384) return 0;
    const int64_t band = std::min<int64_t>(n, 2 * max_clusters + 1024);
    return band * 2 > (int64_t)n ? 0 : band;
}

// Adjacency entries are 4 bytes (m << 8 | score - threshold) when no score can exceed threshold + 255.
inline bool adjacency_packed(int max_len, int min_len, int max_m, int shift_penalty, int max_shift, int threshold, bool force_8byte) {
    const long long top = (long long)max_len * std::max(0, max_m) +
                          (long long)std::max(0, shift_penalty) * ((max_len - min_len) + 2LL * max_shift);
    return top - threshold <= 255 && !force_8byte;
}

// First capacity of a device's edge buffer: 0.3 % of the pair space (uniform random 12-mers at the default threshold give 0.26 %),
// twice that for an asymmetric matrix; one of several devices scores 1 / devices of it, + a quarter for uneven shards.  Never below
// what the buffer has (`have`) or 2^20, the guess never above 2^31; a multiple of HMK_EDGE_SHARDS.  A segment that overflows makes the
// call size the buffer to the counts and score again.  forced_guess != 0 replaces the guess (HMK_EDGE_GUESS: the retry path's tests).
inline uint64_t edge_capacity_guess(bool symmetric, uint32_t n, uint32_t devices, uint64_t forced_guess, uint64_t have) {
    double edges = (double)n * (n - 1) / 2 * (symmetric ? 0.003 : 0.006);
    if (devices > 1) edges = edges / devices * 1.25;
    const uint64_t guess = forced_guess ? forced_guess : (uint64_t)edges + (1u << 20);
    const uint64_t cap = std::max<uint64_t>({std::min<uint64_t>(guess, 1ull << 31), (uint64_t)1 << 20, have});
    return (cap + HMK_EDGE_SHARDS - 1) / HMK_EDGE_SHARDS * HMK_EDGE_SHARDS;
}

// A segment held max_segment_count entries too many for its capacity: what the buffer grows to before the pass is scored again.
inline uint64_t edge_capacity_after_overflow(uint64_t max_segment_count) {
    const uint64_t mx = max_segment_count;
    return (uint64_t)HMK_EDGE_SHARDS * (mx + mx / 8 + 1024);
}

// The separation call (hmk_separation.cpp) cuts its cluster-sorted partner order of nm places into segments; a work item is one block
// of 256 members against one segment.  One segment would give ceil(nm / 256) items -- 391 at 10^5 members on 256 CUs, 14 at 3,383 --
// so: enough segments for SEPARATION_ITEMS items (sixteen for each of a gfx950's 256 CUs: with four, all of one size and resident at
// once, the CUs that took a fifth set the time), at most SEPARATION_MAX_SEGMENTS
// (the scratch is members x segments records), no segment shorter than 256 places (a staged chunk), all segments but the last of one
// length.  forced_len != 0 replaces the length (HMK_TEST_SEPARATION_SEGMENT: any length >= 1, any number of segments).
constexpr uint32_t SEPARATION_ITEMS = 4096, SEPARATION_MAX_SEGMENTS = 64, SEPARATION_MIN_SEGMENT = 256;
struct SeparationSegments { uint32_t length, count; };
inline SeparationSegments separation_segments(uint32_t nm, uint32_t forced_len) {
    if (nm == 0) return {0, 0};
    uint32_t len = forced_len;
    if (len == 0) {
        const uint32_t blocks = (nm + 255) / 256;
        uint32_t want = std::min((SEPARATION_ITEMS + blocks - 1) / blocks, SEPARATION_MAX_SEGMENTS);
        want = std::max(1u, std::min(want, nm / SEPARATION_MIN_SEGMENT));
        len = (nm + want - 1) / want;
    }
    len = std::min(len, nm);
    return {len, (nm + len - 1) / len};
}

// The density call (hmk_density.cpp) keeps the requested rows (n_arrays of cluster, anchor, degree; 4 bytes per vertex and level) of
// several levels on the device and brings them back with one copy per array, so that no level waits for the host: as many levels as
// fit DENSITY_ROWS_BUDGET bytes, at least one, at most the call's n_levels.  21 levels of 10^6 vertices, all three arrays, are one
// batch (252 MB); 256 levels of them are 22 batches.
constexpr uint64_t DENSITY_ROWS_BUDGET = 256ull << 20;
inline uint32_t density_rows_per_batch(uint32_t n, uint32_t n_arrays, uint32_t n_levels) {
    const uint64_t level_bytes = (uint64_t)n * 4 * n_arrays;
    if (level_bytes == 0) return std::max(n_levels, 1u);
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(n_levels, DENSITY_ROWS_BUDGET / level_bytes));
}
inline uint64_t density_rows_bytes(uint32_t n, uint32_t n_arrays, uint32_t per_batch) {
    return std::max<uint64_t>((uint64_t)n * 4 * n_arrays * per_batch, 64);
}

} }  // namespace hmk::sizing
#endif
