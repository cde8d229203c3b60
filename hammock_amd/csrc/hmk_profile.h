// hmk_profile.h -- launchers of k_profile.hip (column counts, information content, match states and leave-one-out KLD of given
// clusters under a given placement), used by hmk_profile.cpp.  The multi-member slots are walked through the host tables of the
// pairs inside given clusters (hmk_slots.h: LinkTables, LinkView); what the profile adds to them is ProfileIn.
#ifndef HMK_PROFILE_H
#define HMK_PROFILE_H

#include "hmk_slots.h"

namespace hmk {

constexpr int PROFILE_SYMBOLS = 21, PROFILE_RESIDUES = 20, PROFILE_MAX_WIDTH = 96;   // (HMK_PROFILE_SYMBOLS, HMK_PROFILE_MAX_WIDTH)
// A slot of PROFILE_LARGE_MIN members or more is counted in LDS, PROFILE_CHUNK members per workgroup step; a smaller one by a lane
// per member straight into the global words.  Measured (tools/bench_profile.py): on 65,536 12-mers in equal slots the
// lane-per-member form is the faster one at slots of 2 and 4 members, the LDS form from 8 members on.
constexpr uint32_t PROFILE_LARGE_MIN = 8;
constexpr uint32_t PROFILE_CHUNK = 1024;

// The call's inputs on the device.  Per member [m - r0]: its slot and its column; per slot: its member count and where its columns
// begin (cstart[n_clusters] = n_cols; n_cols <= 96 * 2^24 < 2^32).  chunk[3 * k ..]: first place in tab, places, slot of chunk k of
// the large slots.
struct ProfileIn {
    const uint32_t *mslot, *column, *size, *cstart, *chunk;
    uint32_t nm, n_clusters, n_cols, n_chunks, large_min;
};

// The call's results on the device.  Per column: counts[col * 21 + sym], ic, flags (bit 0 conserved, bit 1 match state); per slot:
// the conserved columns, the first and the last of them (slot-relative; UINT32_MAX / 0 where none is); per member [m - r0] the KLDs.
struct ProfileOut {
    uint32_t *counts;
    double *ic;
    uint8_t *flags;
    uint32_t *n_conserved, *first, *last;
    double *kld_match, *kld_all;
};

// what the kernels read of hmk_profile_params (the frequency table and the background are staged in LDS by k_profile_kld)
struct ProfileParams {
    double min_ic, max_gap_proportion, beta, sigma, scale;
    int allow_inner_gaps;
    const double *freq_bg;   // device: frequency[400] | background[20]
};

// counts = 0; n_conserved = 0, first = UINT32_MAX, last = 0; both KLDs = 0.0 (what the member of a slot of one keeps)
hipError_t launch_profile_init(const ProfileIn &in, const ProfileOut &out, hipStream_t s);
// the residues of the members of slots below large_min: a lane per member of the range
hipError_t launch_profile_counts_small(const uint8_t *res32, const uint8_t *len, uint32_t r0, const ProfileIn &in, uint32_t *counts,
                                       hipStream_t s);
// the residues of the larger slots: a chunk of a slot's places in tab per workgroup step, counted in LDS, non-zero words flushed
hipError_t launch_profile_counts_large(const uint8_t *res32, const uint8_t *len, const impl::LinkView &V, uint32_t r0, const ProfileIn &in,
                                       uint32_t *counts, hipStream_t s);
// a lane per column: the gap count, ic, the conserved bit; per slot the conserved columns' number, first and last
hipError_t launch_profile_columns(const ProfileIn &in, const ProfileParams &P, const ProfileOut &out, hipStream_t s);
// a lane per column: the match-state bit from the slot's finished first / last
hipError_t launch_profile_match(const ProfileIn &in, const ProfileParams &P, const ProfileOut &out, hipStream_t s);
// a lane per place of V.tab (V.nt places, the multi-member slots' members by slot): both KLDs of the member
hipError_t launch_profile_kld(const uint8_t *res32, const uint8_t *len, const impl::LinkView &V, uint32_t r0, const ProfileIn &in,
                              const ProfileParams &P, const ProfileOut &out, hipStream_t s);

}  // namespace hmk
#endif
