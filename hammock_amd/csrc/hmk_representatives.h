// hmk_representatives.h -- launchers of k_representatives.hip (the lexicographically first maximal independent set of the
// thresholded neighbour graph by synchronous rounds, and every other vertex's representatives), used by hmk_representatives.cpp.
#ifndef HMK_REPRESENTATIVES_H
#define HMK_REPRESENTATIVES_H

#include <hip/hip_runtime_api.h>

#include "hmk_sweep.h"

namespace hmk {

constexpr uint32_t REP_CHUNK = EDGE_RUN_CHUNK;   // edges a workgroup takes at a time (4 per lane): the chunks of an EdgeRuns
constexpr uint32_t REP_MAX_GRID = 2048;       // workgroups of a launch over edges or vertices (8 per compute unit of 256)

enum : uint8_t { REP_UNDECIDED = 0, REP_REP = 1, REP_REDUNDANT = 2 };

// The per-level device block (SB_REP_STATE), zeroed before every level.
//   live      live[b] = the undecided-undecided edges in live buffer b: round r appends to buffer r & 1 and reads buffer (r - 1) & 1;
//             the decision kernel of round r clears live[(r + 1) & 1] for the round behind it
//   tally     the decision kernel's workgroups that are through << 32 | the vertices they leave undecided: 0 again when the kernel ends
//   rounds    the first round that left no vertex undecided (0: none yet)
//   n_edges   the edges >= thr a round-1 launch over an EdgeRuns counted
//   n_rep, n_isolated   the finish kernel's counts
//   flag      non-zero once an edge named an index >= n or a self pair
//   trace     the live edges behind each of the first REP_TRACE rounds (HMK_GREEDY_TIMING prints them)
constexpr uint32_t REP_TRACE = 32;
struct RepState {
    unsigned long long live[2];
    unsigned long long n_edges;
    unsigned long long tally;
    uint32_t rounds, n_rep, n_isolated, flag;
    unsigned long long trace[REP_TRACE];
};

// The per-vertex arrays of one level (SB_REP_VERT), n entries each.
struct RepVertex {
    unsigned long long *key;   // the best representative neighbour so far: (score + 32768) << 32 | (0xFFFFFFFF - index); 0: none
    unsigned long long *mark;  // stamp << 32 | (0xFFFFFFFF - lo), by atomic maximum.  Stamp 2r: an undecided smaller neighbour in round r,
                               // lo = the smallest of them; stamp 2r + 1: a representative smaller neighbour
    uint32_t *covered_by, *nearest;
    int32_t *nearest_score;
    uint8_t *state;            // REP_*
    uint8_t *touched;          // 1: the vertex is the smaller end of an edge of this level (the larger end of one has mark != 0)
};
inline size_t rep_vertex_bytes(uint32_t n) { return (size_t)n * (2 * 8 + 3 * 4 + 2) + 64; }
inline RepVertex rep_vertex_arrays(void *block, uint32_t n) {
    RepVertex v;
    v.key = (unsigned long long *)block;
    v.mark = v.key + n;
    v.covered_by = (uint32_t *)(v.mark + n);
    v.nearest = v.covered_by + n;
    v.nearest_score = (int32_t *)(v.nearest + n);
    v.state = (uint8_t *)(v.nearest_score + n);
    v.touched = v.state + n;
    return v;
}

// every vertex undecided, mark 0, covered_by 0xFFFFFFFF, key 0, untouched
hipError_t launch_rep_init(const RepVertex &v, uint32_t n, hipStream_t s);
// Rounds 1 and 2 over the level's edges E where they lie (those with score >= thr; invalid ones flagged and left out).  Round 1
// counts them into st->n_edges and appends nothing: every vertex is undecided, every edge stays live.  Round 2 reads them again and
// appends the undecided-undecided ones as lo << 32 | hi to live0 (room for `cap` entries).
hipError_t launch_rep_mark_first(uint32_t round, const EdgeRuns &E, uint32_t n, int thr, const RepVertex &v, RepState *st, uint64_t *live0,
                                 uint64_t cap, hipStream_t s);
// Round r >= 3 over the live buffer the round before wrote (its length is st->live[(r - 1) & 1]; total_edges, the level's, sizes the
// grid) into the other one
hipError_t launch_rep_mark(uint32_t round, uint64_t total_edges, const RepVertex &v, RepState *st, uint64_t *live0, uint64_t *live1, uint64_t cap,
                           hipStream_t s);
// The decisions of round r; the last workgroup stores round << 32 | undecided into host_word[0] and the live count into host_word[1]
hipError_t launch_rep_decide(uint32_t round, uint32_t n, const RepVertex &v, RepState *st, unsigned long long *host_word, hipStream_t s);
// covered_by (minimum) and key (maximum) from every edge of the level
hipError_t launch_rep_assign(const EdgeRuns &E, uint32_t n, int thr, const RepVertex &v, hipStream_t s);
// nearest, nearest_score from the keys, the representatives' own entries, st->n_rep and st->n_isolated
hipError_t launch_rep_finish(uint32_t n, const RepVertex &v, RepState *st, hipStream_t s);

}  // namespace hmk
#endif
