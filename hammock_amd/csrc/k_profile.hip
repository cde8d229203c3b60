// k_profile.hip -- the profile of given clusters under a given placement (hmk_cluster_profile, hmk_profile.cpp): per column the
// letter counts (FileIOManager.getPositionLetterCounts, FileIOManager.java:1221-1247), the information content
// (getInformationContents / getInformationContent, :1195-1211, :1421-1439) and the match states (defineMatchStates, :1265-1300);
// per member the leave-one-out KLD against its own slot (Statistics.getPeptideKld / getCorrectedFrequencies,
// Statistics.java:238-300).  A member's row is never built: it is `column` gaps, the peptide, gaps up to the slot's width.
//   k_profile_init          the accumulators of the call
//   k_profile_counts_small  slots below large_min members: a lane per member, its residues straight into the slot's global words
//   k_profile_counts_large  larger slots: PROFILE_CHUNK members per workgroup step counted in LDS, the non-zero words flushed
//   k_profile_columns       a lane per column: gaps, ic, the conserved bit; per slot the conserved columns' number, first and last
//   k_profile_match         a lane per column: the match-state bit
//   k_profile_kld           a lane per member in table order: both KLDs, the frequency table and the background in LDS
// Counts are integer sums, a column's ic is one lane's, a member's KLDs are one lane's in column order: no result depends on the
// grid or the schedule.  The floating-point code is compiled without contraction, so that the operations are the ones written.
#include <algorithm>

#include "hmk_profile.h"
#include "hmk_link_device.h"
#include "hmk_grid.h"

#pragma clang fp contract(off)

namespace hmk {

namespace {

constexpr int R = PROFILE_RESIDUES, S = PROFILE_SYMBOLS, W = PROFILE_MAX_WIDTH;

// getInformationContent (FileIOManager.java:1421-1439) over the 20 residue counts of one column, in symbol order; nongap = their sum
__device__ __forceinline__ double information_content(const uint32_t *__restrict__ cnt, uint32_t nongap) {
    double enthropy = 0.0;
    for (int s = 0; s < R; s++) {
        const uint32_t c = cnt[s];
        if (c == 0) continue;   // (the map holds the letters that occur)
        const double probab = ((double)c + 0.0) / (double)nongap;                      // :1431
        enthropy += probab * (log(probab) / log(2.0));                                 // :1436
    }
    return -(log(0.05) / log(2.0)) + enthropy;                                         // :1438
}

// One column's term of getPeptideKld (Statistics.java:253-269) for a member with letter a in it: cnt = the column's 21 counts with
// the member inside, members = the slot's member count (>= 2).  false: only gaps remain without the member (:262-265).
__device__ __forceinline__ bool kld_term(const uint32_t *__restrict__ cnt, uint32_t members, uint32_t a, const double *freq, const double *bg,
                                         double beta, double sigma, double scale, double &term) {
    const double sum = (double)(members - 1);                                          // :258-261, :277-280
    if (cnt[R] == members - 1) return false;                                           // :262
    double gi = 0.0;
    for (uint32_t j = 0; j < (uint32_t)R; j++) {                                       // :283-289 (a count of 0 adds 0.0)
        const uint32_t c = cnt[j] - (j == a ? 1u : 0u);                                // :254
        const double fj = ((double)c + 0.0) / sum;                                     // :285
        gi += fj * freq[j * R + a];                                                    // :286-287
    }
    const double fi = ((double)(cnt[a] - 1u) + 0.0) / sum;                             // :292
    const double Qi = (((sum - 1) * fi) + (beta * gi)) / ((sum - 1) + beta);           // :296
    double positionKld = log(Qi / bg[a]) * (sum / (sum + sigma));                      // :267
    positionKld = positionKld * scale;                                                 // :268
    term = positionKld;
    return true;
}

}  // namespace

// -----------------------------------------------------------------------------
// accumulators: cleared by every call, so that no state survives one
// -----------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_profile_init(ProfileIn in, ProfileOut out) {
    const uint64_t words = (uint64_t)in.n_cols * S;
    const uint64_t n = max(words, (uint64_t)max(in.nm, in.n_clusters));
    for (uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (uint64_t)gridDim.x * 256) {
        if (k < words) out.counts[k] = 0;
        if (k < in.n_clusters) { out.n_conserved[k] = 0; out.first[k] = 0xFFFFFFFFu; out.last[k] = 0; }
        if (k < in.nm) { out.kld_match[k] = 0.0; out.kld_all[k] = 0.0; }
    }
}

// -----------------------------------------------------------------------------
// counts, small slots: a lane per member of the range
// -----------------------------------------------------------------------------
// A slot below large_min members puts at most large_min - 1 adds on a word, and the slots' words lie apart: the adds go to global
// memory as they are.  Members of larger slots are skipped (k_profile_counts_large counts them).  The gap count is not summed: it
// is the member count less the residues (k_profile_columns).
__global__ void __launch_bounds__(256)
k_profile_counts_small(const uint8_t *__restrict__ res32, const uint8_t *__restrict__ len, uint32_t r0, ProfileIn in,
                       uint32_t *__restrict__ counts) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < in.nm; i += gridDim.x * 256) {
        const uint32_t slot = in.mslot[i];
        if (in.size[slot] >= in.large_min) continue;
        const uint32_t c0 = in.cstart[slot], width = in.cstart[slot + 1] - c0, col = in.column[i], L = len[r0 + i];
        const uint8_t *seq = res32 + (size_t)(r0 + i) * 32;
#pragma unroll 1
        for (uint32_t k = 0; k < L; k++) {
            const uint32_t a = seq[k];
            if (col + k < width && a < (uint32_t)R)   // (always: the host has checked both; no index leaves the slot's words)
                atomicAdd(&counts[(uint64_t)(c0 + col + k) * S + a], 1u);
        }
    }
}

// -----------------------------------------------------------------------------
// counts, large slots: chunks of a slot's members in LDS
// -----------------------------------------------------------------------------
// chunk k = PROFILE_CHUNK consecutive places of tab inside one slot (the last chunk of a slot: what is left).  96 x 20 words of
// LDS; a word takes at most PROFILE_CHUNK adds.  Only the non-zero words go to global memory: one add per word, chunk and slot
// instead of one per residue.
__global__ void __launch_bounds__(256)
k_profile_counts_large(const uint8_t *__restrict__ res32, const uint8_t *__restrict__ len, const uint32_t *__restrict__ tab, uint32_t r0,
                       ProfileIn in, uint32_t *__restrict__ counts) {
    __shared__ uint32_t lcnt[W * R];
    const uint32_t tid = threadIdx.x;
    for (uint32_t chunk = blockIdx.x; chunk < in.n_chunks; chunk += gridDim.x) {
        const uint32_t begin = in.chunk[3 * chunk], places = in.chunk[3 * chunk + 1], slot = in.chunk[3 * chunk + 2];
        const uint32_t c0 = in.cstart[slot], width = min(in.cstart[slot + 1] - c0, (uint32_t)W);
        __syncthreads();   // the last chunk's words have been flushed
        for (uint32_t e = tid; e < (uint32_t)(W * R); e += 256) lcnt[e] = 0;
        __syncthreads();
        for (uint32_t e = tid; e < places; e += 256) {
            const uint32_t m = tab[begin + e], col = in.column[m - r0], L = len[m];
            const uint8_t *seq = res32 + (size_t)m * 32;
#pragma unroll 1
            for (uint32_t k = 0; k < L; k++) {
                const uint32_t a = seq[k];
                if (col + k < width && a < (uint32_t)R) atomicAdd(&lcnt[(col + k) * R + a], 1u);   // (always: as above)
            }
        }
        __syncthreads();
        for (uint32_t e = tid; e < width * R; e += 256) {
            const uint32_t v = lcnt[e];
            if (v) atomicAdd(&counts[(uint64_t)(c0 + e / R) * S + e % R], v);
        }
    }
}

// -----------------------------------------------------------------------------
// columns: gaps, information content, the conserved bit; per slot the conserved columns
// -----------------------------------------------------------------------------
// Grid-stride over the columns of all slots, 256 per block and step.  The slots of consecutive columns never decrease, so the
// slot's number of conserved columns, the first and the last are a segmented scan over the wave and one atomic each per wave and
// slot segment, as k_align_center's key is.  The decision ic >= min_ic is made here and nowhere else.
__global__ void __launch_bounds__(256)
k_profile_columns(ProfileIn in, ProfileParams P, ProfileOut out) {
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t base = blockIdx.x * 256; base < in.n_cols; base += gridDim.x * 256) {   // (uniform: every lane takes every step)
        const uint32_t g = base + threadIdx.x;
        const bool valid = g < in.n_cols;
        uint32_t slot = 0xFFFFFFFFu, n = 0, lo = 0xFFFFFFFFu, hi = 0;
        if (valid) {
            slot = run_of<uint32_t>(in.cstart, in.n_clusters, g);
            const uint32_t members = in.size[slot];
            uint32_t *cnt = out.counts + (uint64_t)g * S;
            uint32_t nongap = 0;
            for (int s = 0; s < R; s++) nongap += cnt[s];
            const uint32_t gaps = members - min(nongap, members);
            cnt[R] = gaps;
            double ic = -1.0;                                                          // FileIOManager.java:1207
            if (((double)gaps + 0.0) / (double)members <= P.max_gap_proportion)        // :1204
                ic = information_content(cnt, nongap);
            out.ic[g] = ic;
            const bool conserved = ic >= P.min_ic;                                     // :1271, :1281
            out.flags[g] = conserved ? 1 : 0;
            if (conserved) { n = 1; lo = hi = g - in.cstart[slot]; }
        }
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t oslot = __shfl_up(slot, d), on = __shfl_up(n, d), olo = __shfl_up(lo, d), ohi = __shfl_up(hi, d);
            if (lane >= (uint32_t)d && oslot == slot) { n += on; lo = min(lo, olo); hi = max(hi, ohi); }
        }
        const uint32_t next = __shfl_down(slot, 1);
        if (valid && n && (lane == 63 || next != slot)) {   // the segment's last lane holds its totals
            atomicAdd(&out.n_conserved[slot], n);
            atomicMin(&out.first[slot], lo);
            atomicMax(&out.last[slot], hi);
        }
    }
}

// -----------------------------------------------------------------------------
// the match states (defineMatchStates, FileIOManager.java:1265-1300)
// -----------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_profile_match(ProfileIn in, ProfileParams P, ProfileOut out) {
    for (uint32_t g = blockIdx.x * 256 + threadIdx.x; g < in.n_cols; g += gridDim.x * 256) {
        const uint32_t slot = run_of<uint32_t>(in.cstart, in.n_clusters, g), rel = g - in.cstart[slot];
        const uint8_t f = out.flags[g] & 1;
        const bool match = P.allow_inner_gaps ? f != 0                                              // :1269-1276
                                              : (out.first[slot] <= rel && rel <= out.last[slot]);   // :1277-1297 (first = all ones: none)
        out.flags[g] = f | (match ? 2 : 0);
    }
}

// -----------------------------------------------------------------------------
// the members' KLDs (Statistics.getPeptideKld, Statistics.java:238-273)
// -----------------------------------------------------------------------------
// A lane per place of tab: the members of a slot are consecutive places, so a wave's lanes read the same slot's counts.  The
// columns of the member's residues left to right; where the member has a gap nothing is added (:249-252).
__global__ void __launch_bounds__(256)
k_profile_kld(const uint8_t *__restrict__ res32, const uint8_t *__restrict__ len, const uint32_t *__restrict__ tab, uint32_t nt, uint32_t r0,
              ProfileIn in, ProfileParams P, ProfileOut out) {
    __shared__ double freq[R * R];
    __shared__ double bg[R];
    for (int e = threadIdx.x; e < R * R + R; e += 256) {
        if (e < R * R) freq[e] = P.freq_bg[e]; else bg[e - R * R] = P.freq_bg[e];
    }
    __syncthreads();
    for (uint32_t t = blockIdx.x * 256 + threadIdx.x; t < nt; t += gridDim.x * 256) {
        const uint32_t m = tab[t], i = m - r0, slot = in.mslot[i], members = in.size[slot];
        const uint32_t c0 = in.cstart[slot], width = in.cstart[slot + 1] - c0, col = in.column[i], L = len[m];
        const uint8_t *seq = res32 + (size_t)m * 32;
        double all = 0.0, match = 0.0;
#pragma unroll 1
        for (uint32_t k = 0; k < L; k++) {
            const uint32_t a = seq[k];
            if (col + k >= width || a >= (uint32_t)R || members < 2) continue;   // (never: the host has checked them)
            const uint64_t g = (uint64_t)c0 + col + k;
            double term;
            if (!kld_term(out.counts + g * S, members, a, freq, bg, P.beta, P.sigma, P.scale, term)) continue;
            all += term;                                                               // :269
            if (out.flags[g] & 2) match += term;                                       // :246
        }
        out.kld_all[i] = all;
        out.kld_match[i] = match;
    }
}

// -----------------------------------------------------------------------------
// launchers
// -----------------------------------------------------------------------------
hipError_t launch_profile_init(const ProfileIn &in, const ProfileOut &out, hipStream_t s) {
    const uint64_t n = std::max<uint64_t>((uint64_t)in.n_cols * S, std::max(in.nm, in.n_clusters));
    if (n == 0) return hipSuccess;
    const uint32_t blocks = capped_grid("k_profile_init", (uint32_t)std::min<uint64_t>((n + 255) / 256, 4096));
    hipLaunchKernelGGL(k_profile_init, dim3(blocks), dim3(256), 0, s, in, out);
    return hipGetLastError();
}

hipError_t launch_profile_counts_small(const uint8_t *res32, const uint8_t *len, uint32_t r0, const ProfileIn &in, uint32_t *counts,
                                       hipStream_t s) {
    if (in.nm == 0) return hipSuccess;
    const uint32_t blocks = capped_grid("k_profile_counts_small", std::min<uint32_t>((in.nm + 255) / 256, 65536));
    hipLaunchKernelGGL(k_profile_counts_small, dim3(blocks), dim3(256), 0, s, res32, len, r0, in, counts);
    return hipGetLastError();
}

hipError_t launch_profile_counts_large(const uint8_t *res32, const uint8_t *len, const impl::LinkView &V, uint32_t r0, const ProfileIn &in,
                                       uint32_t *counts, hipStream_t s) {
    if (in.n_chunks == 0) return hipSuccess;
    const uint32_t blocks = capped_grid("k_profile_counts_large", std::min<uint32_t>(in.n_chunks, 65536));
    hipLaunchKernelGGL(k_profile_counts_large, dim3(blocks), dim3(256), 0, s, res32, len, V.tab, r0, in, counts);
    return hipGetLastError();
}

hipError_t launch_profile_columns(const ProfileIn &in, const ProfileParams &P, const ProfileOut &out, hipStream_t s) {
    if (in.n_cols == 0) return hipSuccess;
    const uint32_t blocks = capped_grid("k_profile_columns", std::min<uint32_t>((in.n_cols + 255) / 256, 65536));
    hipLaunchKernelGGL(k_profile_columns, dim3(blocks), dim3(256), 0, s, in, P, out);
    return hipGetLastError();
}

hipError_t launch_profile_match(const ProfileIn &in, const ProfileParams &P, const ProfileOut &out, hipStream_t s) {
    if (in.n_cols == 0) return hipSuccess;
    const uint32_t blocks = capped_grid("k_profile_match", std::min<uint32_t>((in.n_cols + 255) / 256, 65536));
    hipLaunchKernelGGL(k_profile_match, dim3(blocks), dim3(256), 0, s, in, P, out);
    return hipGetLastError();
}

hipError_t launch_profile_kld(const uint8_t *res32, const uint8_t *len, const impl::LinkView &V, uint32_t r0, const ProfileIn &in,
                              const ProfileParams &P, const ProfileOut &out, hipStream_t s) {
    if (V.nt == 0) return hipSuccess;
    const uint32_t blocks = capped_grid("k_profile_kld", std::min<uint32_t>((V.nt + 255) / 256, 65536));
    hipLaunchKernelGGL(k_profile_kld, dim3(blocks), dim3(256), 0, s, res32, len, V.tab, V.nt, r0, in, P, out);
    return hipGetLastError();
}

}  // namespace hmk
