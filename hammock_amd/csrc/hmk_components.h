// hmk_components.h -- launchers of k_components.hip (connected components of the thresholded neighbour graph, at one threshold or
// a range of them), used by hmk_components.cpp.
#ifndef HMK_COMPONENTS_H
#define HMK_COMPONENTS_H

#include <hip/hip_runtime_api.h>

#include "hmk_internal.h"

namespace hmk {

constexpr uint32_t CC_MAX_LEVELS = 256;   // threshold_hi - threshold <= 255

// The per-call device block behind the levels' results (SB_CC_STATE): zeroed at the start of a call.
//   levels   as the ABI's, except n_components = the hooks of that level's launch (the host turns them into counts) and
//            levels[0].reserved = non-zero once an edge named an index >= n or a self pair
//   hist     edges per level; start: the levels' runs in the partitioned buffer (ascending level), cursor: where the next chunk of a
//            level goes
struct CcState {
    hmk_component_level levels[CC_MAX_LEVELS];
    unsigned long long hist[CC_MAX_LEVELS];
    unsigned long long start[CC_MAX_LEVELS + 1];
    unsigned long long cursor[CC_MAX_LEVELS];
};

// parent[i] = i, size[i] = 0
hipError_t launch_cc_init(uint32_t *parent, uint32_t *size, uint32_t n, hipStream_t s);
// level of an edge = min(score, thr_hi) - thr; edges below thr are left out, invalid ones (index >= n, self pair) flagged and left out
hipError_t launch_cc_hist(const EdgeRuns &E, uint32_t n, int thr, int thr_hi, CcState *st, hipStream_t s);
// start / cursor from hist, levels[l].n_edges = edges of the levels >= l (one workgroup)
hipError_t launch_cc_scan(uint32_t n_levels, CcState *st, hipStream_t s);
// every counted edge's (x, m), as x << 32 | m, into its level's run of `runs`
hipError_t launch_cc_partition(const EdgeRuns &E, uint32_t n, int thr, int thr_hi, CcState *st, uint64_t *runs, hipStream_t s);
// the union of one level's run (total_edges: the edges of all levels, which sizes the grid -- the level's own count stays on the device)
hipError_t launch_cc_union(const uint64_t *runs, unsigned long long total_edges, uint32_t level, uint32_t *parent, CcState *st, hipStream_t s);
// the union straight from the edge runs (a single level): counts the edges >= thr into levels[0].n_edges
hipError_t launch_cc_union_edges(const EdgeRuns &E, uint32_t n, int thr, uint32_t *parent, CcState *st, hipStream_t s);
// parent[v] = v's root, size[root] += 1
hipError_t launch_cc_flatten(uint32_t *parent, uint32_t *size, uint32_t n, hipStream_t s);
// levels[level].n_singletons / largest from size[], which is cleared
hipError_t launch_cc_sizes(uint32_t *size, uint32_t n, uint32_t level, CcState *st, hipStream_t s);

}  // namespace hmk
#endif
