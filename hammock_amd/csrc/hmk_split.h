// hmk_split.h -- launchers of k_split.hip (every score inside given clusters, as dense triangles), used by hmk_split.cpp.
#ifndef HMK_SPLIT_H
#define HMK_SPLIT_H

#include "hmk_linkage.h"

namespace hmk {

// scores: int16[total_pairs] (LinkTables).  A slot's entry q = i (i - 1) / 2 + j, j < i (places in the slot's member list, which is in
// index order), holds score(seq1 = member i, seq2 = member j): the orientation of the edges of hmk_neighbors_shifted.
//   flat    the triangles of the flat slots back to back: entry k of the flat pair space is scores[k].  tab, fmstart, fpstart, nf,
//           n_pairs as launch_linkage_flat's
hipError_t launch_split_flat(const uint8_t *res32, const uint8_t *len, const int32_t *d_matrix, const uint32_t *tab, const uint32_t *fmstart,
                             const unsigned long long *fpstart, uint32_t nf, unsigned long long n_pairs, int X, int p, int16_t *scores,
                             hipStream_t s);
//   tiled   big slot g's triangle at scores + tbase[g] (tbase[nb + 1]: 64-bit prefix sums of s (s - 1) / 2 behind the flat pair space);
//           bmstart, btstart, nb, n_tiles as launch_linkage_tiled's
hipError_t launch_split_tiled(const uint8_t *res32, const uint8_t *len, const int32_t *d_matrix, const uint32_t *tab, const uint32_t *bmstart,
                              const uint32_t *btstart, const unsigned long long *tbase, uint32_t nb, uint32_t n_tiles, int X, int p,
                              int16_t *scores, hipStream_t s);

}  // namespace hmk
#endif
