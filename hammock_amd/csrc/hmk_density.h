// hmk_density.h -- launchers of k_density.hip (density clustering of the thresholded neighbour graph: degrees, core vertices, a
// union-find over the core-core edges and an anchor key per vertex, all carried from the top level down), used by hmk_density.cpp.
#ifndef HMK_DENSITY_H
#define HMK_DENSITY_H

#include <hip/hip_runtime_api.h>

#include "hmk_sweep.h"

namespace hmk {

constexpr uint32_t DEN_CHUNK = EDGE_RUN_CHUNK;   // edges a workgroup takes at a time (4 per lane): the chunks of an EdgeRuns
constexpr uint32_t DEN_MAX_GRID = 2048;       // workgroups of a launch over edges or vertices (8 per compute unit of 256)
constexpr int DEN_COMBINE = 4;                // distinct values a wave combines by ballot before its lanes add one by one

enum : uint8_t { DEN_NOT_CORE = 0, DEN_CORE = 1, DEN_CORE_NEW = 2 };   // core since an earlier level; core as of this level

// The per-call device block (SB_DEN_STATE), zeroed at the start of a call: one record per level, so that no level waits for the
// host to read the one before.
//   n_edges   the valid edges >= threshold k_den_degree counted (a single level; a range has the sweep's prefixes)
//   looked    the edges k_den_link looked at: the level's own and the older ones with an end that turned core at this level
//   new_core  the vertices that turned core at this level (k_den_core); k_den_link reads it
//   n_core, n_border, n_noise   k_den_labels' counts;  n_clusters, largest   k_den_sizes'
//   flag      non-zero once an edge named an index >= n or a self pair
struct DenLevel {
    unsigned long long n_edges, looked;
    uint32_t new_core, n_core, n_border, n_noise, n_clusters, largest;
};
struct DenState {
    unsigned long long flag;
    DenLevel level[SWEEP_MAX_LEVELS];
};

// The per-vertex arrays of a call (SB_DEN_VERT), n entries each; all but size[] carry over from level to level.
struct DenVertex {
    unsigned long long *key;   // the best core neighbour so far: (score + 32768) << 32 | (0xFFFFFFFF - index), by atomic maximum; 0: none
                               // (the format of RepVertex::key)
    uint32_t *parent;          // the union-find over the core vertices (a non-core vertex is its own root and never touched)
    uint32_t *size;            // members per label of the level at hand: k_den_labels adds, k_den_sizes clears
    uint32_t *degree;          // edges >= t that touch the vertex
    uint8_t *state;            // DEN_*
};
inline size_t den_vertex_bytes(uint32_t n) { return (size_t)n * (8 + 3 * 4 + 1) + 64; }
inline DenVertex den_vertex_arrays(void *block, uint32_t n) {
    DenVertex v;
    v.key = (unsigned long long *)block;
    v.parent = (uint32_t *)(v.key + n);
    v.size = v.parent + n;
    v.degree = v.size + n;
    v.state = (uint8_t *)(v.degree + n);
    return v;
}

// The edges of one level: E names the edges >= t (a range: the prefix of the dealt buffer, one run; a single level: the call's
// edges where they lie, those below thr and the invalid ones left out by every kernel); the level's own run, the edges that are not
// edges of the level above, begins at entry own_start of run 0 (0: every edge is the level's own).
struct DenEdges {
    EdgeRuns E;
    unsigned long long own_start;
};

// parent[i] = i, key, size, degree, state = 0
hipError_t launch_den_init(const DenVertex &v, uint32_t n, hipStream_t s);
// the level's own run: +1 to both ends' degrees, equal ends of a wave combined first; counts the edges into lv->n_edges and flags
// the invalid ones
hipError_t launch_den_degree(const DenEdges &D, uint32_t n, int thr, const DenVertex &v, DenState *st, uint32_t level, hipStream_t s);
// DEN_CORE_NEW -> DEN_CORE; a non-core vertex with degree >= min_neighbors -> DEN_CORE_NEW, counted into new_core
hipError_t launch_den_core(uint32_t n, uint32_t min_neighbors, const DenVertex &v, DenState *st, uint32_t level, hipStream_t s);
// over the edges >= t: an edge is looked at iff it lies in the level's own run or one of its ends is DEN_CORE_NEW
hipError_t launch_den_link(const DenEdges &D, uint32_t n, int thr, const DenVertex &v, DenState *st, uint32_t level, hipStream_t s);
// cluster, anchor and degree of every vertex into the rows given (device memory, each may be null), size[label] += 1, the three counts
hipError_t launch_den_labels(uint32_t n, const DenVertex &v, uint32_t *cluster_row, uint32_t *anchor_row, uint32_t *degree_row, DenState *st,
                             uint32_t level, hipStream_t s);
// n_clusters = the core roots, largest from size[], which it clears
hipError_t launch_den_sizes(uint32_t n, const DenVertex &v, DenState *st, uint32_t level, hipStream_t s);

}  // namespace hmk
#endif
