// hmk_split.h -- launchers of k_split.hip (every score inside given clusters, as dense triangles), used by hmk_split.cpp.
#ifndef HMK_SPLIT_H
#define HMK_SPLIT_H

#include "hmk_linkage.h"

namespace hmk {

// scores: int16[total_pairs] (LinkTables).  A slot's entry q = i (i - 1) / 2 + j, j < i (places in the slot's member list, which is in
// index order), holds score(seq1 = member i, seq2 = member j): the orientation of the edges of hmk_neighbors_shifted.  V: the
// uploaded tables.
//   flat    the triangles of the flat slots back to back: entry k of the flat pair space is scores[k]
hipError_t launch_split_flat(const uint8_t *res32, const uint8_t *len, const int32_t *d_matrix, const impl::LinkView &V, int X, int p,
                             int16_t *scores, hipStream_t s);
//   tiled   big slot g's triangle at scores + V.tbase[g]
hipError_t launch_split_tiled(const uint8_t *res32, const uint8_t *len, const int32_t *d_matrix, const impl::LinkView &V, int X, int p,
                              int16_t *scores, hipStream_t s);

}  // namespace hmk
#endif
