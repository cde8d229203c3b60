// k_separation.hip -- the separation of given clusters (hmk_cluster_separation_shifted, hmk_separation.cpp): per member the sum of its
// ShiftedScorer scores against the other members of its own slot, and of all other slots the one with the largest mean score, with its
// sum.  The sums per (member, slot) are never stored: the partners are walked in cluster-sorted order (SepTables::ord), a lane carries
// one running sum and closes it where the order leaves a slot -- the same place for every lane, so the close is a uniform branch.
//   k_separation_walk    work item = LINK_TILE members, one per lane, x one segment of the partner order; the partners staged LINK_TILE
//                        at a time and read by all lanes at once (the rectangle form of k_survey_tiled); a record per (segment, member)
//   k_separation_merge   one lane per member: its records joined in segment order, the four member outputs
// Every pair is scored by the literal scorer (shifted_score_literal, hmk_device.h) with the lane's member as seq1, as k_survey_tiled's
// rectangle scores its queries (the other way round the walk measured a third slower): under the symmetric matrix the call insists on,
// the score does not depend on the orientation.  Integer adds and comparisons only, no atomics:
// no result depends on the grid, the segment length or the schedule.
#include <algorithm>

#include "hmk_link_device.h"
#include "hmk_separation.h"
#include "hmk_grid.h"

namespace hmk {

namespace {

// The best slot so far: replaced only by a strictly larger mean.  The slots arrive in ascending order, so the smallest slot of equal
// means stays.  sum / size > best_sum / best_size by cross-multiplication: |sum| <= 2^15 size, the two slots are disjoint parts of at
// most 2^24 members, so a product stays below 2^15 * 2^23 * 2^23.
struct SepBest {
    long long sum;
    uint32_t size, slot;
};
__device__ __forceinline__ void sep_consider(SepBest &b, long long sum, uint32_t size, uint32_t slot) {
    if (b.size == 0 || sum * (long long)b.size > b.sum * (long long)size) {
        b.sum = sum;
        b.size = size;
        b.slot = slot;
    }
}

}  // namespace

// -----------------------------------------------------------------------------
// the pairs
// -----------------------------------------------------------------------------
// Beside a staged partner go its index (the lane's own member adds nothing), its slot, and the slot's size if the partner holds the
// slot's last place (0: the slot goes on).  A lane adds a chunk's scores in 32 bits (LINK_TILE scores of at most 2^15) and folds them
// into the slot's 64-bit sum at the chunk's end and at a close.
__global__ void __launch_bounds__(256)
k_separation_walk(const uint8_t *__restrict__ res32, const uint8_t *__restrict__ len, const int32_t *__restrict__ Mg, SepTables T, uint32_t r0,
                  uint32_t n_items, int X, int p, SepRecords rec) {
    constexpr int TL = LINK_TILE;
    static_assert(TL == 256, "a member block and a staged chunk are as wide as the workgroup");
    __shared__ __attribute__((aligned(16))) int M[576];
    __shared__ __attribute__((aligned(16))) uint32_t colseq[TL * SEQ_STRIDE_DW];
    __shared__ __attribute__((aligned(16))) uint32_t rowseq[TL * 8];
    __shared__ uint8_t rowlen[TL];
    __shared__ uint32_t ridx[TL], rslot[TL], rsize[TL];
    const int tid = threadIdx.x;
    const uint32_t wave = tid >> 6;
    for (int e = tid; e < 576; e += 256) M[e] = Mg[e];
    uint32_t *mine = colseq + tid * SEQ_STRIDE_DW;
    for (uint32_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        const uint32_t block = item / T.n_segments, seg = item - block * T.n_segments;
        const uint32_t m0 = block * TL, nmem = min((uint32_t)TL, T.nm - m0);          // m0 < nm
        const uint32_t p0 = seg * T.seg_len, p1 = min(T.nm, p0 + T.seg_len);          // p0 < p1 <= nm
        const bool has_me = (uint32_t)tid < nmem;
        const uint32_t me = r0 + m0 + tid;
        int mylen = 0;
        uint32_t myslot = 0xFFFFFFFFu;
        if (has_me) {
            stage_sequence(mine, res32, me);
            mylen = len[me];
            myslot = T.mslot[m0 + tid];
        }
        // the segment's ends (the same for every lane): does it start inside a slot, does it end inside one
        const uint32_t hs = T.pslot[p0], ts = T.pslot[p1 - 1];
        bool head_open = p0 > T.cstart[hs];
        const bool has_tail = p1 < T.cstart[ts + 1];
        const bool wave_has_members = wave * 64 < nmem;
        long long run = 0, own = 0, head = 0, tail = 0;
        SepBest best{0, 0, 0xFFFFFFFFu};
        for (uint32_t c0 = p0; c0 < p1; c0 += TL) {
            const uint32_t cn = min((uint32_t)TL, p1 - c0);
            __syncthreads();   // the matrix stands; the last chunk has been read
            if ((uint32_t)tid < cn) {
                const uint32_t place = c0 + tid, idx = T.ord[place], sl = T.pslot[place], end = T.cstart[sl + 1];
                link_stage_row(rowseq, tid, res32, idx);
                rowlen[tid] = len[idx];
                ridx[tid] = idx;
                rslot[tid] = sl;
                rsize[tid] = place + 1 == end ? end - T.cstart[sl] : 0;
            }
            __syncthreads();
            if (!wave_has_members) continue;
            int run32 = 0;
#pragma unroll 1
            for (uint32_t k = 0; k < cn; k++) {
                if (has_me && ridx[k] != me) {
                    const uint8_t *rs = reinterpret_cast<const uint8_t *>(rowseq + k * 8), *cs = reinterpret_cast<const uint8_t *>(mine);
                    run32 += shifted_score_literal(M, cs, mylen, rs, rowlen[k], X, p);
                }
                const uint32_t closing = (uint32_t)__builtin_amdgcn_readfirstlane((int)rsize[k]);
                if (closing) {   // the same for every lane
                    const uint32_t slot = (uint32_t)__builtin_amdgcn_readfirstlane((int)rslot[k]);
                    const long long sum = run + run32;
                    run = 0;
                    run32 = 0;
                    if (slot == myslot) own += sum;
                    else if (head_open) head = sum;
                    else sep_consider(best, sum, closing, slot);
                    head_open = false;
                }
            }
            run += run32;
        }
        if (has_tail) {   // a slot is still open: never closed here at all (one piece, kept as the head) or opened here
            if (ts == myslot) own += run;
            else if (head_open) head = run;
            else tail = run;
        }
        if (has_me) {
            const size_t r = (size_t)seg * T.nm + m0 + tid;
            rec.own[r] = own;
            rec.head[r] = head;
            rec.tail[r] = tail;
            rec.best_sum[r] = best.sum;
            rec.best_size[r] = best.size;
            rec.best_slot[r] = best.slot;
        }
    }
}

// -----------------------------------------------------------------------------
// a member's records in segment order -> its outputs
// -----------------------------------------------------------------------------
// The open pieces of one slot are joined across the segments it spans and closed where it ends; the candidates -- a closed join, a
// segment's best -- arrive in ascending slot order, under the walk's comparison.
__global__ void __launch_bounds__(256)
k_separation_merge(SepTables T, SepRecords rec, SepOut out) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < T.nm; i += gridDim.x * 256) {
        const uint32_t myslot = T.mslot[i];
        long long own = 0, open = 0;
        SepBest best{0, 0, 0xFFFFFFFFu};
        for (uint32_t seg = 0; seg < T.n_segments; seg++) {
            const uint32_t p0 = seg * T.seg_len, p1 = min(T.nm, p0 + T.seg_len);
            const uint32_t hs = T.pslot[p0], ts = T.pslot[p1 - 1];
            const bool has_head = p0 > T.cstart[hs], has_tail = p1 < T.cstart[ts + 1];
            const size_t r = (size_t)seg * T.nm + i;
            own += rec.own[r];
            if (has_head) open += rec.head[r];
            if (has_head && has_tail && hs == ts) continue;   // wholly inside one slot: the slot stays open
            if (has_head) {
                if (hs != myslot) sep_consider(best, open, T.cstart[hs + 1] - T.cstart[hs], hs);
                open = 0;
            }
            const uint32_t bsize = rec.best_size[r];
            if (bsize) sep_consider(best, rec.best_sum[r], bsize, rec.best_slot[r]);
            if (has_tail) open = rec.tail[r];
        }
        const uint32_t mine = T.cstart[myslot + 1] - T.cstart[myslot];
        out.own_sum[i] = own;
        out.near_sum[i] = best.size ? best.sum : 0;
        out.near_cluster[i] = best.slot;
        // own / (mine - 1) < near / size, strictly
        out.misplaced[i] = best.size && mine >= 2 && own * (long long)best.size < best.sum * (long long)(mine - 1);
    }
}

// -----------------------------------------------------------------------------
// launchers
// -----------------------------------------------------------------------------
uint32_t separation_items(uint32_t nm, uint32_t n_segments) {
    const uint64_t items = (((uint64_t)nm + LINK_TILE - 1) / LINK_TILE) * n_segments;
    return items > 0x7FFFFFFFull ? 0xFFFFFFFFu : (uint32_t)items;
}

hipError_t launch_separation_walk(const uint8_t *res32, const uint8_t *len, const int32_t *d_matrix, const SepTables &T, uint32_t r0, int X, int p,
                                  const SepRecords &rec, hipStream_t s) {
    const uint32_t n_items = separation_items(T.nm, T.n_segments);
    if (n_items == 0) return hipSuccess;
    if (n_items == 0xFFFFFFFFu || T.seg_len == 0) return hipErrorInvalidValue;
    const uint32_t blocks = capped_grid("k_separation_walk", std::min<uint32_t>(n_items, 65536));
    hipLaunchKernelGGL(k_separation_walk, dim3(blocks), dim3(256), 0, s, res32, len, d_matrix, T, r0, n_items, X, p, rec);
    return hipGetLastError();
}

hipError_t launch_separation_merge(const SepTables &T, const SepRecords &rec, const SepOut &out, hipStream_t s) {
    if (T.nm == 0) return hipSuccess;
    const uint32_t blocks = capped_grid("k_separation_merge", std::min<uint32_t>((T.nm + 255) / 256, 4096));
    hipLaunchKernelGGL(k_separation_merge, dim3(blocks), dim3(256), 0, s, T, rec, out);
    return hipGetLastError();
}

}  // namespace hmk
