// hmk_orders.h -- launchers of k_orders.hip (the packed edges of one neighbour pass renamed into another order of the set; the
// co-clustering support of every edge over the orders' clusterings), used by hmk_orders.cpp (hmk_greedy_orders*).  The edges are
// named by an EdgeRuns (hmk_internal.h).
#ifndef HMK_ORDERS_H
#define HMK_ORDERS_H

#include <hip/hip_runtime_api.h>

#include "hmk_internal.h"
#include "hmk_sweep.h"

namespace hmk {

constexpr uint32_t ORDERS_MAX = 256;             // orders per call: a support fits the edge's score field with room to spare
constexpr uint32_t ORDERS_MAX_GRID = 2048;       // workgroups of the two kernels (8 per compute unit of 256)
constexpr uint32_t ORDERS_FLUSH_CHUNKS = 1u << 21;   // k_orders_support adds its LDS counters to the global ones after that many chunks:
                                                     // 2^31 edges at most in one 32-bit counter

// where run s of the edges begins in the renamed buffer: the runs back to back (passed by value beside EdgeRuns)
struct OrderRuns {
    unsigned long long off[HMK_EDGE_SHARDS];
};

// The per-call device block (SB_ORD_STATE), zeroed at the start of a call.
//   together    per valid order v: the edges whose ends share a cluster in v; with_first: ... and in valid order 0 as well
//   n_support   edges with support >= 1 (the next place in the support buffer); n_always: support == n_valid
//   total       the number of renamed edges: the count word of the tail's one segment (set once, behind the zeroing)
//   flag        non-zero once an edge named an index >= n or a self pair
// n_support ... flag lie together: the host reads them in one copy.
struct OrdersState {
    unsigned long long together[ORDERS_MAX];
    unsigned long long with_first[ORDERS_MAX];
    unsigned long long n_support, n_always, total, flag;
};

// every edge (x, m, score) as (min(pos[x], pos[m]), max(...), score) at the same place of the runs laid back to back; the 16 score
// bits are copied.  pos[n]: the order's inverse permutation.
hipError_t launch_orders_relabel(const EdgeRuns &E, const OrderRuns &R, uint32_t n, const uint32_t *pos, uint64_t *out, OrdersState *st,
                                 hipStream_t s);
// support of every edge = the valid orders v with ids[x][v] == ids[m][v] (ids: [n][n_valid], the transposed cluster ids).  An edge
// with support >= 1 goes to out[] (x < m, support in the score field) while there is room (cap entries; out may be null), counts
// towards ever[x], ever[m] and, at support == n_valid, always[x], always[m]; the per-order sums go to st.
hipError_t launch_orders_support(const EdgeRuns &E, uint32_t n, const int32_t *ids, uint32_t n_valid, uint64_t *out, unsigned long long cap,
                                 uint32_t *ever, uint32_t *always, OrdersState *st, hipStream_t s);

}  // namespace hmk
#endif
