// hmk_separation.h -- launchers of k_separation.hip (the separation of given clusters: per member the sum of its scores against its own
// slot and against the nearest other slot), used by hmk_separation.cpp.
#ifndef HMK_SEPARATION_H
#define HMK_SEPARATION_H

#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace hmk {

// The host's tables of one call, O(members + clusters).  A place is a position of the cluster-sorted partner order.
//   ord[nm]       the members (indices of the uploaded set) sorted by slot, in index order inside a slot
//   pslot[nm]     the slot of the member at a place
//   mslot[nm]     the slot of member r0 + k (the caller's member_cluster)
//   cstart[ncl+1] the slots' first places; slot c holds the places [cstart[c], cstart[c + 1])
struct SepTables {
    const uint32_t *ord, *pslot, *mslot, *cstart;
    uint32_t nm, n_clusters;
    uint32_t seg_len, n_segments;   // segment s = the places [s seg_len, min(nm, (s + 1) seg_len))
};

// What a walk leaves per (segment, member), at [segment * nm + member - r0]; sums of the member's scores against the partners of the
// segment that are not the member itself:
//   own    the partners of the member's own slot
//   head   the partners of the slot that was open at the segment's first place, when the segment does not start on a slot boundary and
//          that slot is not the member's own.  A segment that lies wholly inside one slot and touches neither of its ends has this
//          piece only.
//   tail   the partners of the slot still open after the segment's last place, when that is not the slot of `head` continued and not
//          the member's own
//   best   of the other slots that lie wholly inside the segment the one with the largest mean, the smallest slot among equal means:
//          its sum, size and number (size 0: none)
struct SepRecords {
    long long *own, *head, *tail, *best_sum;
    uint32_t *best_size, *best_slot;
};
constexpr size_t SEP_RECORD_BYTES = 40;

// the four outputs per member
struct SepOut {
    long long *own_sum, *near_sum;
    uint32_t *near_cluster;
    uint8_t *misplaced;
};

// work items of the walk: blocks of LINK_TILE members x segments
uint32_t separation_items(uint32_t nm, uint32_t n_segments);

// Every ordered pair (member, partner != member) of [r0, r0 + nm) scored once by the literal scorer (symmetric matrices: the score of a
// pair does not depend on the orientation) and reduced into rec.
hipError_t launch_separation_walk(const uint8_t *res32, const uint8_t *len, const int32_t *d_matrix, const SepTables &T, uint32_t r0, int X, int p,
                                  const SepRecords &rec, hipStream_t s);
// The members' records joined in segment order -> out.
hipError_t launch_separation_merge(const SepTables &T, const SepRecords &rec, const SepOut &out, hipStream_t s);

}  // namespace hmk
#endif
