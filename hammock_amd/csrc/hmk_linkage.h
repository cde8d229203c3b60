// hmk_linkage.h -- launchers of k_linkage.hip (complete-linkage scores inside given clusters), used by hmk_linkage.cpp, and the host
// tables of the pairs inside given clusters, which hmk_split.cpp (k_split.hip) decodes its work from too.
#ifndef HMK_LINKAGE_H
#define HMK_LINKAGE_H

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include <vector>

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
// not wanted).  tab: the members by slot, each slot's in index order, the flat slots' first.
//   flat    fslot[nf]: the caller's slot; fmstart[nf + 1]: its members' places in tab; fpstart[nf + 1]: prefix sums of s (s - 1) / 2,
//           n_pairs = fpstart[nf]
hipError_t launch_linkage_flat(const uint8_t *res32, const uint8_t *len, const int32_t *d_matrix, const uint32_t *tab, const uint32_t *fslot,
                               const uint32_t *fmstart, const unsigned long long *fpstart, uint32_t nf, unsigned long long n_pairs, uint32_t r0,
                               int X, int p, int thr, uint64_t *key, unsigned long long *below, int32_t *member_min, uint32_t *member_below,
                               hipStream_t s);
//   tiled   bslot[nb], bmstart[nb + 1] likewise; btstart[nb + 1]: prefix sums of t (t + 1) / 2 with t = ceil(s / LINK_TILE),
//           n_tiles = btstart[nb]
hipError_t launch_linkage_tiled(const uint8_t *res32, const uint8_t *len, const int32_t *d_matrix, const uint32_t *tab, const uint32_t *bslot,
                                const uint32_t *bmstart, const uint32_t *btstart, uint32_t nb, uint32_t n_tiles, uint32_t r0, int X, int p,
                                int thr, uint64_t *key, unsigned long long *below, int32_t *member_min, uint32_t *member_below, hipStream_t s);

// The host tables both calls upload, O(members + clusters): the members of the slots of two or more by slot, each slot's in index
// order, the flat slots' first; per flat / big slot the caller's slot and its members' places in tab; the prefix sums the kernels
// decode their work from.  One block of 32-bit words h (offsets o_*, in words), the 64-bit tables 8-byte aligned behind the others:
//   tab | fslot[nf] | fmstart[nf + 1] | bslot[nb] | bmstart[nb + 1] | btstart[nb + 1] | fpstart[nf + 1] (u64) | tbase[nb + 1] (u64)
// tbase[g]: where big slot g's dense triangle of s (s - 1) / 2 entries begins in an array that holds the flat pair space first
// (k_split.hip); tbase[nb] = total_pairs.
struct LinkTables {
    std::vector<uint32_t> h;
    uint32_t nf = 0, nb = 0, n_tiles = 0;
    size_t o_tab = 0, o_fslot = 0, o_fmstart = 0, o_bslot = 0, o_bmstart = 0, o_btstart = 0, o_fpstart = 0, o_tbase = 0;
    unsigned long long flat_pairs = 0, total_pairs = 0;
    const unsigned long long *fpstart() const { return reinterpret_cast<const unsigned long long *>(h.data() + o_fpstart); }
    const unsigned long long *tbase() const { return reinterpret_cast<const unsigned long long *>(h.data() + o_tbase); }
};
// members[c]: slot c's member count (check_clusters); member_cluster[nm]: the slot of member r0 + i (hmk_linkage.cpp)
void build_link_tables(uint32_t r0, uint32_t nm, const uint32_t *member_cluster, uint32_t n_clusters, const std::vector<uint32_t> &members,
                       LinkTables &T);

}  // namespace hmk
#endif
