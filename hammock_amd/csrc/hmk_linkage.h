// hmk_linkage.h -- launchers of k_linkage.hip (complete-linkage scores inside given clusters), used by hmk_linkage.cpp, and the two
// sizes the host tables of the pairs inside given clusters are built around (hmk_slots.h: LinkTables, LinkView).
#ifndef HMK_LINKAGE_H
#define HMK_LINKAGE_H

#include "hmk_slots.h"

namespace hmk {

// Slots of up to LINK_FLAT_MAX members have their pairs enumerated flat, a lane per pair; larger ones are tiled, LINK_TILE rows x
// LINK_TILE columns of the slot's member list per block (where the boundary sits and why).
constexpr int LINK_FLAT_MAX = 256;
constexpr int LINK_TILE = 256;

// key[n_clusters] = all ones, below[n_clusters] = 0; with member_min != null, member_min[nm] = INT32_MAX, member_below[nm] = 0
hipError_t launch_linkage_init(uint64_t *key, unsigned long long *below, uint32_t n_clusters, int32_t *member_min, uint32_t *member_below,
                               uint32_t nm, hipStream_t s);
// The accumulators of both kernels: key[slot] takes (score + 32768) << 48 | a << 24 | b (a < b, indices of the uploaded set) under a
// 64-bit minimum, below[slot] the pairs scoring below thr; member_min / member_below[member - r0] the same per member (both null:
// not wanted).  V: the uploaded tables.
//   flat    the flat slots' pairs (V.fslot, V.fmstart, V.fpstart)
hipError_t launch_linkage_flat(const uint8_t *res32, const uint8_t *len, const int32_t *d_matrix, const impl::LinkView &V, uint32_t r0, int X, int p,
                               int thr, uint64_t *key, unsigned long long *below, int32_t *member_min, uint32_t *member_below, hipStream_t s);
//   tiled   the big slots' tiles (V.bslot, V.bmstart, V.btstart)
hipError_t launch_linkage_tiled(const uint8_t *res32, const uint8_t *len, const int32_t *d_matrix, const impl::LinkView &V, uint32_t r0, int X, int p,
                                int thr, uint64_t *key, unsigned long long *below, int32_t *member_min, uint32_t *member_below, hipStream_t s);

}  // namespace hmk
#endif
