// hmk_slots.h -- what the calls over given clusters ("the members [r0, r1) with a slot per member": hmk_linkage.cpp, hmk_split.cpp,
// hmk_separation.cpp, hmk_align.cpp, hmk_profile.cpp) share on the host: the slots' check, their members and counts, the host tables
// of the pairs inside them and the device's view of those tables, which the launchers of k_linkage.hip, k_split.hip, k_align.hip and
// k_profile.hip take.  Plain functions: each entry point still lists its own steps.  Not part of the public ABI.
#ifndef HMK_SLOTS_H
#define HMK_SLOTS_H

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include <vector>

struct hmk_ctx;

namespace hmk { namespace impl {

// The range and slot checks of a call without cluster ids (check_clusters with the ids 1 ... n_clusters and no query range; `what`
// names the call in the range message) -> members[c] = slot c's member count.
int check_slots(hmk_ctx *ctx, const char *what, uint32_t r0, uint32_t r1, const uint32_t *member_cluster, uint32_t n_clusters,
                std::vector<uint32_t> &members);
// the parameter checks of a call that scores the pairs inside slots of the members [r0, r1): check_shifted over the range, and the
// lowest possible score fits int16, the indices 24 bits
int check_link_scores(hmk_ctx *ctx, int X, int p, int thr, uint32_t r0, uint32_t r1);

// The slots' members: slot c = list[start[c] .. start[c + 1]), places in [0, nm), ascending.
struct SlotMembers {
    std::vector<uint32_t> start, list;
    SlotMembers(uint32_t nm, const uint32_t *member_cluster, uint32_t n_clusters, const std::vector<uint32_t> &members);
};

// the slots of two or more members, and the pairs inside them: the sum of s (s - 1) / 2
struct SlotCounts {
    uint32_t n_multi;
    uint64_t pairs;
};
SlotCounts count_slots(const std::vector<uint32_t> &members);

// The host tables of the pairs inside given clusters, O(members + clusters): the members of the slots of two or more by slot, each
// slot's in index order, the flat slots' (up to LINK_FLAT_MAX members, hmk_linkage.h) first; per flat / big slot the caller's slot
// and its members' places in tab; the prefix sums the kernels decode their work from.  One block of 32-bit words h (offsets o_*, in
// words), the 64-bit tables 8-byte aligned behind the others:
//   tab | fslot[nf] | fmstart[nf + 1] | bslot[nb] | bmstart[nb + 1] | btstart[nb + 1] | fpstart[nf + 1] (u64) | tbase[nb + 1] (u64)
// fpstart: prefix sums of s (s - 1) / 2 over the flat slots, flat_pairs = fpstart[nf]; btstart: prefix sums of t (t + 1) / 2 with
// t = ceil(s / LINK_TILE) over the big ones, n_tiles = btstart[nb].  tbase[g]: where big slot g's dense triangle of s (s - 1) / 2
// entries begins in an array that holds the flat pair space first (k_split.hip); tbase[nb] = total_pairs.
struct LinkTables {
    std::vector<uint32_t> h;
    uint32_t nf = 0, nb = 0, n_tiles = 0;
    size_t o_tab = 0, o_fslot = 0, o_fmstart = 0, o_bslot = 0, o_bmstart = 0, o_btstart = 0, o_fpstart = 0, o_tbase = 0;
    unsigned long long flat_pairs = 0, total_pairs = 0;
    const unsigned long long *fpstart() const { return reinterpret_cast<const unsigned long long *>(h.data() + o_fpstart); }
    const unsigned long long *tbase() const { return reinterpret_cast<const unsigned long long *>(h.data() + o_tbase); }
};
// members[c]: slot c's member count (check_slots); member_cluster[nm]: the slot of member r0 + i
void build_link_tables(uint32_t r0, uint32_t nm, const uint32_t *member_cluster, uint32_t n_clusters, const std::vector<uint32_t> &members,
                       LinkTables &T);

// The uploaded tables as the launchers take them: LinkTables' arrays in device memory and its counts; nt = the places of tab.
struct LinkView {
    const uint32_t *tab, *fslot, *fmstart, *bslot, *bmstart, *btstart;
    const unsigned long long *fpstart, *tbase;
    uint32_t nf, nb, n_tiles, nt;
    unsigned long long flat_pairs;
};
// room for T in SB_LINK_TAB -> *V = its view there (the error goes to ctx)
int reserve_link_tables(hmk_ctx *ctx, const LinkTables &T, LinkView *V);
// T into SB_LINK_TAB, enqueued on Q
hipError_t upload_link_tables(hmk_ctx *ctx, const LinkTables &T, hipStream_t Q);

} }  // namespace hmk::impl
#endif
