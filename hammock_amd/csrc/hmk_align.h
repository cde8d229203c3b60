// hmk_align.h -- launchers of k_align.hip (centre-star alignment of given clusters around their medoids), used by hmk_align.cpp.
// The work is decoded from the host tables of the pairs inside given clusters (hmk_slots.h: LinkTables, LinkView).
#ifndef HMK_ALIGN_H
#define HMK_ALIGN_H

#include "hmk_slots.h"

namespace hmk {

// The accumulators of one call.  Per slot: key[n_clusters] takes (member_sum + 2^39) << 24 | (0xFFFFFF - member) under a 64-bit
// maximum (the largest sum, then the smallest index), min_shift / max_end the smallest shift and the largest shift + length of the
// slot's members.  Per member [member - r0]: sum = its score against the other members of its slot, score / shift = scoreWithShift
// (seq1 = the slot's centre, seq2 = the member).
struct AlignOut {
    uint64_t *key;
    int32_t *min_shift, *max_end;
    long long *sum;
    int32_t *score, *shift;
};

// key = 0, min_shift = INT32_MAX, max_end = INT32_MIN; sum = 0, score = INT32_MAX, shift = 0 (what a centre and a slot of one keep)
hipError_t launch_align_init(const AlignOut &out, uint32_t n_clusters, uint32_t nm, hipStream_t s);
// the sums of the flat slots' members (V: the uploaded tables, as launch_linkage_flat takes them)
hipError_t launch_align_sums_flat(const uint8_t *res32, const uint8_t *len, const int32_t *d_matrix, const impl::LinkView &V, uint32_t r0, int X,
                                  int p, long long *sum, hipStream_t s);
// the sums of the big slots' members (as launch_linkage_tiled takes them)
hipError_t launch_align_sums_tiled(const uint8_t *res32, const uint8_t *len, const int32_t *d_matrix, const impl::LinkView &V, uint32_t r0, int X,
                                   int p, long long *sum, hipStream_t s);
// The tables' slots as both member kernels walk them: place t of tab (nt places: the flat slots' members, then the big slots') lies in
// flat slot run_of(fmstart, t) or big slot run_of(bmstart, t).
struct AlignSlots {
    const uint32_t *tab, *fslot, *fmstart, *bslot, *bmstart;
    uint32_t nf, nb, nt;
};
// key[slot] from the finished sums
hipError_t launch_align_center(const AlignSlots &T, uint32_t r0, const long long *sum, uint64_t *key, hipStream_t s);
// score / shift of every member against its slot's centre (read from key), min_shift / max_end per slot
hipError_t launch_align_shift(const uint8_t *res32, const uint8_t *len, const int32_t *d_matrix, const AlignSlots &T, uint32_t r0, uint32_t r1,
                              int X, int p, const AlignOut &out, hipStream_t s);

}  // namespace hmk
#endif
