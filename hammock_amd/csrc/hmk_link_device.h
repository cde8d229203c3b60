// hmk_link_device.h -- device code shared by the kernels that walk the pairs INSIDE given clusters: k_linkage.hip (minimum and counts
// per slot and member) and k_split.hip (every score, as dense triangles).  Both decode the same host tables (hmk_slots.h:
// LinkTables) and score a pair the same way: the literal scorer with seq1 = the pair's larger index.
#ifndef HMK_LINK_DEVICE_H
#define HMK_LINK_DEVICE_H

#include "hmk_device.h"
#include "hmk_linkage.h"

namespace hmk {

namespace {

// largest k in [0, n) with start[k] <= x (start[0] = 0 <= x < start[n])
template <typename T>
__device__ __forceinline__ uint32_t run_of(const T *__restrict__ start, uint32_t n, T x) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (start[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

// q = i (i - 1) / 2 + j with j < i: the row of the strict lower triangle that holds entry q
__device__ __forceinline__ uint32_t tri_row(uint32_t q) {
    uint32_t i = (uint32_t)((1.0f + sqrtf(1.0f + 8.0f * (float)q)) * 0.5f);
    while (i > 1 && (uint64_t)i * (i - 1) / 2 > q) i--;
    while ((uint64_t)(i + 1) * i / 2 <= q) i++;
    return i;
}

// entry q of a strict lower triangle: its row and its column, col < row
struct TriEntry { uint32_t row, col; };
__device__ __forceinline__ TriEntry tri_entry(uint32_t q) {
    TriEntry e;
    e.row = tri_row(q);
    e.col = q - e.row * (e.row - 1) / 2;
    return e;
}

// the pair's score, a < b indices of the uploaded set: both staged in the lane's LDS (s1, s2), seq1 = b
__device__ __forceinline__ int link_pair_score(const int *M, uint32_t *s1, uint32_t *s2, const uint8_t *__restrict__ res32,
                                               const uint8_t *__restrict__ len, uint32_t a, uint32_t b, int X, int p) {
    stage_sequence(s1, res32, b);
    stage_sequence(s2, res32, a);
    return shifted_score_literal(M, reinterpret_cast<const uint8_t *>(s1), len[b], reinterpret_cast<const uint8_t *>(s2), len[a], X, p);
}

// tile number -> big slot g and the tile's block row i >= block column j (tile t of a slot = i (i + 1) / 2 + j)
__device__ __forceinline__ void link_tile_decode(const uint32_t *__restrict__ btstart, uint32_t nb, uint32_t tile, uint32_t &g, uint32_t &i,
                                                 uint32_t &j) {
    g = run_of<uint32_t>(btstart, nb, tile);
    const uint32_t t = tile - btstart[g];
    i = (uint32_t)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while (i > 0 && (uint64_t)i * (i + 1) / 2 > t) i--;
    while ((uint64_t)(i + 1) * (i + 2) / 2 <= t) i++;
    j = t - (uint32_t)((uint64_t)i * (i + 1) / 2);
}

// row `row` of a tile: the 32 residue bytes of sequence idx into rowseq (8 dwords per row, read by all lanes at once)
__device__ __forceinline__ void link_stage_row(uint32_t *rowseq, uint32_t row, const uint8_t *__restrict__ res32, uint32_t idx) {
    const u32x4 *src = reinterpret_cast<const u32x4 *>(res32 + (size_t)idx * 32);
    reinterpret_cast<u32x4 *>(rowseq)[row * 2] = src[0];
    reinterpret_cast<u32x4 *>(rowseq)[row * 2 + 1] = src[1];
}

}  // namespace

}  // namespace hmk
#endif
