// k_scan.hip -- the device side of the scan of peptides along long targets (hmk_scan.cpp): window scores
// w(q, t, s) of ShiftedScorer.scoreWithShift(seq1 = peptide, seq2 = target) (ShiftedScorer.java:67-85) for every offset s, in two
// bit-exact forms -- byte lanes over the 8-peptides-per-entry table E[i][c] of DESIGN.md 5.1 with a lane's "column" the window that
// starts at its target position, and plain int32 sums -- the reduction of the window hits per (peptide, target), and the coverage
// of the targets' residues by the returned records.
// Every store here is an ordinary vector store; the counters are vector atomics.
#include "hmk_device.h"
#include "hmk_grid.h"
#include "hmk_scan.h"

namespace hmk {

namespace {

constexpr uint32_t SCAN_STAGE = 128;                  // records a wave stages in LDS before it takes room in the hit buffer
constexpr uint32_t SCAN_EXT = SCAN_CHUNK + HMK_MAX_LEN;   // staged target residues of a chunk: its windows' first residues + m - 1 more
constexpr uint32_t SCAN_SUBS = SCAN_CHUNK / 256;      // windows per lane and chunk

__device__ __forceinline__ unsigned long long wave_bcast_u64(unsigned long long v) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return ((unsigned long long)hi << 32) | lo;
}

__device__ __forceinline__ void store_hit(hmk_scan_hit *dst, const u32x4 &r) { *reinterpret_cast<u32x4 *>(dst) = r; }

// a wave's staged records to the hit buffer: one returning atomic per flush.  The count runs on beyond the capacity (the host
// grows the buffer to it and scores again); only records inside it are stored.
__device__ __forceinline__ void scan_flush(const u32x4 *stage, uint32_t cnt, const ScanParams &P) {
    if (cnt == 0) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");   // staged ds_writes land before the reads below
    const uint32_t lane = threadIdx.x & 63u;
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(P.count, (unsigned long long)cnt);
    base = wave_bcast_u64(base);
    for (uint32_t k = lane; k < cnt; k += 64)
        if (base + k < P.cap) store_hit(P.hits + base + k, stage[k]);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");   // reads done before the stage is reused
}

// Appends every lane's `c` records (next() yields them one after the other) to the wave's stage; called by all 64 lanes.  A step
// with more hits than the stage holds (every lane, several peptides each) stores them directly.
template <class Next>
__device__ __forceinline__ void scan_emit(u32x4 *stage, uint32_t &cnt, const ScanParams &P, uint32_t c, Next next) {
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t incl = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t v = __shfl_up(incl, o, 64);
        if (lane >= (uint32_t)o) incl += v;
    }
    const uint32_t total = __builtin_amdgcn_readfirstlane(__shfl(incl, 63, 64));
    const uint32_t excl = incl - c;
    if (cnt + total > SCAN_STAGE) {
        scan_flush(stage, cnt, P);
        cnt = 0;
    }
    if (total > SCAN_STAGE) {
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(P.count, (unsigned long long)total);
        base = wave_bcast_u64(base);
        for (uint32_t j = 0; j < c; j++) {
            const u32x4 r = next();
            if (base + excl + j < P.cap) store_hit(P.hits + base + excl + j, r);
        }
    } else {
        for (uint32_t j = 0; j < c; j++) stage[cnt + excl + j] = next();
        cnt += total;
    }
}

// the chunk's target residues with max_shift sentinels beyond the target's ends: ext[k] = residue at position w0 + k - X
__device__ __forceinline__ void stage_target(uint8_t *ext, const ScanParams &P, uint64_t tbase, uint32_t n, uint32_t w0, uint32_t m) {
    for (uint32_t k = threadIdx.x; k < SCAN_CHUNK + m - 1; k += 256) {
        const long long pos = (long long)w0 + k - P.X;
        ext[k] = (pos >= 0 && pos < (long long)n) ? P.tres[tbase + (uint64_t)pos] : (uint8_t)SCAN_SENTINEL;
    }
}

// which groups of the run the byte lanes take against a target with d = n - m (bit k: group k); the literal form takes the others
__device__ __forceinline__ uint32_t scan_packed_groups(const ScanParams &P, const ScanRun &R, long long d) {
    if (P.no_packed) return 0;
    const long long limit = scan_bound_limit((int)R.m, P.X, P.p, P.thr, d, P.bias, P.max_m);
    uint32_t mask = 0;
    for (uint32_t k = 0; k < SCAN_RUN_GROUPS; k++)
        if (k * SCAN_GROUP < R.count && (long long)R.bound[k] <= limit) mask |= 1u << k;
    return mask;
}

// E[group][position][column]: byte r = M[peptide r's residue at the position][column] + bias, the sentinel column the bias alone,
// the bytes of a group's missing peptides 0.  One workgroup per run at a time.
__global__ void __launch_bounds__(256) k_scan_tables(ScanParams P, uint64_t *__restrict__ tables) {
    for (uint32_t r = blockIdx.x; r < P.n_runs; r += gridDim.x) {
        const ScanRun R = P.runs[r];
        const uint32_t per_group = R.m * SCAN_COLUMNS, groups = (R.count + SCAN_GROUP - 1) / SCAN_GROUP;
        for (uint32_t e = threadIdx.x; e < groups * per_group; e += 256) {
            const uint32_t gi = e / per_group, i = (e % per_group) / SCAN_COLUMNS, c = e % SCAN_COLUMNS;
            uint64_t v = 0;
            for (uint32_t b = 0; b < SCAN_GROUP; b++) {
                const uint32_t idx = gi * SCAN_GROUP + b;
                if (idx >= R.count) break;
                const uint32_t a = P.res32[(size_t)P.qlist[R.first + idx] * 32 + i];
                const int cell = (c < SCAN_SENTINEL ? P.M[a * HMK_ALPHABET + c] : 0) + P.bias;
                v |= (uint64_t)(uint32_t)cell << (8 * b);
            }
            tables[(size_t)R.table + e] = v;
        }
    }
}

// The byte-lane form for peptides of length M.  A tile is (chunk of a target, run of up to 8 groups); the workgroup stages the
// chunk's residues and the groups' tables, a lane fetches the M residues of its window once and walks the groups: one 8-byte
// table read per position and group, the adds in SWAR, "w >= threshold" the lane's top bit, the hits' scores cut out of the
// accumulators where they are.
template <int M>
__global__ void __launch_bounds__(256) k_scan_packed(ScanParams P, uint32_t run0, uint32_t n_runs_m) {
    constexpr uint32_t PER_GROUP = M * SCAN_COLUMNS;   // entries
    __shared__ uint64_t tab[SCAN_RUN_GROUPS * PER_GROUP];
    __shared__ uint8_t ext[SCAN_EXT];
    __shared__ u32x4 stage_all[4][SCAN_STAGE];
    u32x4 *stage = stage_all[threadIdx.x >> 6];
    uint32_t cnt = 0;
    const uint32_t tab_addr = lds_addr(tab);
    // run-major tiles, a contiguous span per workgroup: the tables of a run are loaded once for all the chunks the span holds of it
    const uint64_t n_tiles = (uint64_t)P.n_chunks * n_runs_m, span = (n_tiles + gridDim.x - 1) / gridDim.x;
    const uint64_t tile_end = min(n_tiles, (blockIdx.x + 1) * span);
    uint32_t loaded = 0xFFFFFFFFu;
    for (uint64_t tile = blockIdx.x * span; tile < tile_end; tile++) {
        const uint32_t run = run0 + (uint32_t)(tile / P.n_chunks);
        const ScanChunk Ck = P.chunks[tile % P.n_chunks];
        const ScanRun R = P.runs[run];
        const uint64_t tbase = P.toff[Ck.t];
        const uint32_t n = (uint32_t)(P.toff[Ck.t + 1] - tbase);
        const int d = (int)n - M;
        const uint32_t nwin = (uint32_t)(d + 2 * P.X + 1);
        if (Ck.w0 >= nwin) continue;                      // (uniform over the workgroup, as everything up to the lane's window)
        const uint32_t groups = scan_packed_groups(P, R, d);
        if (groups == 0) continue;
        __syncthreads();                                  // the previous tile's reads of ext and tab are done
        stage_target(ext, P, tbase, n, Ck.w0, M);
        if (run != loaded) {
            const uint32_t entries = (R.count + SCAN_GROUP - 1) / SCAN_GROUP * PER_GROUP;   // every group of the run, whatever this target takes
            for (uint32_t e = threadIdx.x; e < entries; e += 256) tab[e] = P.tables[(size_t)R.table + e];
            loaded = run;
        }
        __syncthreads();
        const int g = 128 - P.thr + d * P.p;
#pragma unroll 1
        for (uint32_t sub = 0; sub < SCAN_SUBS; sub++) {
            const uint32_t wl = sub * 256 + threadIdx.x, w = Ck.w0 + wl;
            if (Ck.w0 + sub * 256 + (threadIdx.x & ~63u) >= nwin) continue;   // the whole wave is beyond the last window
            const bool active = w < nwin;
            const int s = (int)w - P.X;
            const int over = s < 0 ? -s : (s > d ? s - d : 0);
            const uint32_t start = (uint32_t)((g + 2 * P.p * over - P.bias * M) & 0xFF) * 0x01010101u;
            uint32_t roff[M];
#pragma unroll
            for (int i = 0; i < M; i++) roff[i] = tab_addr + (uint32_t)ext[wl + i] * 8u;
#pragma unroll
            for (uint32_t gi = 0; gi < SCAN_RUN_GROUPS; gi++) {
                if (!((groups >> gi) & 1u)) continue;
                uint32_t a0 = start, a1 = start;
#pragma unroll
                for (int i = 0; i < M; i++) {
                    const u32x2 e = *reinterpret_cast<const volatile HMK_LDS u32x2 *>((uintptr_t)(roff[i] + (gi * PER_GROUP + i * SCAN_COLUMNS) * 8u));
                    a0 += e.x;
                    a1 += e.y;
                }
                const uint32_t left = R.count - gi * SCAN_GROUP;      // the group's peptides (8, or fewer in a length's last group)
                const uint64_t valid = left >= SCAN_GROUP ? ~0ull : ((1ull << (8 * left)) - 1ull);
                uint64_t hm = active ? (((uint64_t)a1 << 32 | a0) & 0x8080808080808080ull & valid) : 0ull;
                if (__ballot(hm != 0) == 0) continue;
                const uint64_t acc = (uint64_t)a1 << 32 | a0;
                scan_emit(stage, cnt, P, (uint32_t)__popcll(hm), [&]() {
                    const uint32_t b = (uint32_t)(__ffsll((long long)hm) - 1) >> 3;
                    hm &= hm - 1;
                    const int score = (int)((acc >> (8 * b)) & 0xFFu) - 128 + P.thr;
                    u32x4 r;
                    r.x = P.qlist[R.first + gi * SCAN_GROUP + b];
                    r.y = Ck.t;
                    r.z = (uint32_t)score;
                    r.w = (uint32_t)s;
                    return r;
                });
            }
        }
    }
    scan_flush(stage, cnt, P);
}

// The literal form: a lane is one (peptide, window), int32 sums, the matrix and the staged chunk in LDS.  It scores every group
// the byte lanes do not take (other lengths, other parameters, classes that leave the byte range, HMK_NO_SCAN_PACKED).
__global__ void __launch_bounds__(256) k_scan_literal(ScanParams P) {
    __shared__ int Ml[HMK_ALPHABET * HMK_ALPHABET];
    __shared__ uint8_t ext[SCAN_EXT];
    __shared__ uint32_t pep[SCAN_RUN_GROUPS * SCAN_GROUP * 8];   // the run's peptides, 32 bytes each
    __shared__ u32x4 stage_all[4][SCAN_STAGE];
    u32x4 *stage = stage_all[threadIdx.x >> 6];
    uint32_t cnt = 0;
    for (uint32_t k = threadIdx.x; k < HMK_ALPHABET * HMK_ALPHABET; k += 256) Ml[k] = P.M[k];
    const uint64_t n_tiles = (uint64_t)P.n_chunks * P.n_runs;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const ScanChunk Ck = P.chunks[tile / P.n_runs];
        const ScanRun R = P.runs[(uint32_t)(tile % P.n_runs)];
        const uint64_t tbase = P.toff[Ck.t];
        const uint32_t n = (uint32_t)(P.toff[Ck.t + 1] - tbase);
        const int m = (int)R.m, d = (int)n - m;
        const uint32_t nwin = (uint32_t)(d + 2 * P.X + 1);
        if (Ck.w0 >= nwin) continue;
        const uint32_t n_groups = (R.count + SCAN_GROUP - 1) / SCAN_GROUP;
        const uint32_t groups = ((1u << n_groups) - 1u) & ~scan_packed_groups(P, R, d);
        if (groups == 0) continue;
        __syncthreads();                                  // the previous tile's reads are done (and Ml stands)
        stage_target(ext, P, tbase, n, Ck.w0, (uint32_t)m);
        for (uint32_t k = threadIdx.x; k < R.count * 8; k += 256)
            pep[k] = reinterpret_cast<const uint32_t *>(P.res32 + (size_t)P.qlist[R.first + k / 8] * 32)[k % 8];
        __syncthreads();
        const uint8_t *pepb = reinterpret_cast<const uint8_t *>(pep);
        for (uint32_t idx = 0; idx < R.count; idx++) {
            if (!((groups >> (idx / SCAN_GROUP)) & 1u)) continue;
            for (uint32_t sub = 0; sub < SCAN_SUBS; sub++) {
                const uint32_t wl = sub * 256 + threadIdx.x, w = Ck.w0 + wl;
                if (Ck.w0 + sub * 256 + (threadIdx.x & ~63u) >= nwin) continue;
                const int s = (int)w - P.X;
                int sum = d * P.p;                                          // ShiftedScorer.java:79
                if (s < 0) sum += -s * 2 * P.p;                             // :80-82
                if (s > d) sum += (s - d) * 2 * P.p;                        // :83-85
                for (int i = 0; i < m; i++) {                               // :69-77: the cells of the overlap
                    const uint32_t c = ext[wl + i];
                    if (c < SCAN_SENTINEL) sum += Ml[pepb[idx * 32 + i] * HMK_ALPHABET + c];
                }
                const bool hit = w < nwin && sum >= P.thr;
                if (__ballot(hit) == 0) continue;
                scan_emit(stage, cnt, P, hit ? 1u : 0u, [&]() {
                    u32x4 r;
                    r.x = P.qlist[R.first + idx];
                    r.y = Ck.t;
                    r.z = (uint32_t)sum;
                    r.w = (uint32_t)s;
                    return r;
                });
            }
        }
    }
    scan_flush(stage, cnt, P);
}

// ---- pair mode: the best window of every (query, target) ------------------------------------------------------------------
// An open-addressing table of (pair + 1, value); value = (score + 2^30) << 32 | ~(offset + X): the larger value is the higher
// score, then the smaller offset -- the first strict maximum of the loop at ShiftedScorer.java:86-89.  Maxima of integers: the
// table's CONTENT as a set does not depend on the schedule or the grid (only where a pair's slot lies does).

__device__ __forceinline__ uint64_t scan_mix(uint64_t k) {
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
    return k;
}

__global__ void __launch_bounds__(256)
k_scan_pair_insert(const hmk_scan_hit *__restrict__ hits, uint64_t n, uint32_t q0, uint32_t t0, uint32_t nt, int X,
                   unsigned long long *__restrict__ keys, unsigned long long *__restrict__ vals, uint64_t slots) {
    for (uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (uint64_t)gridDim.x * 256) {
        const hmk_scan_hit h = hits[k];
        const unsigned long long key = (unsigned long long)(h.query - q0) * nt + (h.target - t0) + 1ull;
        const unsigned long long val = ((unsigned long long)(uint32_t)(h.score + (1 << 30)) << 32) | (0xFFFFFFFFu - (uint32_t)(h.offset + X));
        uint64_t slot = scan_mix(key) & (slots - 1);
        for (uint64_t probe = 0; probe < slots; probe++) {   // (the table is at most half full: the walk ends long before)
            const unsigned long long old = atomicCAS(&keys[slot], 0ull, key);
            if (old == 0ull || old == key) {
                atomicMax(&vals[slot], val);
                break;
            }
            slot = (slot + 1) & (slots - 1);
        }
    }
}

// the table's entries as records.  A workgroup stages what it finds in LDS and takes room in the output once per PAIR_STAGE - 256
// records or more: one returning atomic per flush, not per wave (3 x 10^7 pairs: 25 ms -> the time of reading the table).
constexpr uint32_t PAIR_STAGE = 2048;
__global__ void __launch_bounds__(256)
k_scan_pair_compact(const unsigned long long *__restrict__ keys, const unsigned long long *__restrict__ vals, uint64_t slots, uint32_t q0,
                    uint32_t t0, uint32_t nt, int X, hmk_scan_hit *__restrict__ out, uint64_t out_cap, unsigned long long *__restrict__ count) {
    __shared__ u32x4 stage[PAIR_STAGE];
    __shared__ uint32_t staged;
    __shared__ unsigned long long out_base;
    if (threadIdx.x == 0) staged = 0;
    const uint64_t rounds = (slots + (uint64_t)gridDim.x * 256 - 1) / ((uint64_t)gridDim.x * 256);
    for (uint64_t it = 0; it <= rounds; it++) {            // (every thread takes every round: the barriers are workgroup-wide)
        __syncthreads();                                   // the round before has staged its records
        const uint32_t have = staged;
        __syncthreads();                                   // every thread has read the count before any thread adds to it below:
                                                           // the flush decision is the same in all four waves by construction
        if (have + 256 > PAIR_STAGE || (it == rounds && have)) {
            if (threadIdx.x == 0) out_base = atomicAdd(count, (unsigned long long)have);
            __syncthreads();
            for (uint32_t k = threadIdx.x; k < have; k += 256)
                if (out_base + k < out_cap) store_hit(out + out_base + k, stage[k]);
            __syncthreads();                               // the stage is read before it is filled again
            if (threadIdx.x == 0) staged = 0;
            __syncthreads();
        }
        if (it == rounds) break;
        const uint64_t k = (it * gridDim.x + blockIdx.x) * 256 + threadIdx.x;
        const unsigned long long key = k < slots ? keys[k] : 0ull;
        if (key == 0ull) continue;
        const unsigned long long v = vals[k];
        u32x4 r;
        r.x = q0 + (uint32_t)((key - 1) / nt);
        r.y = t0 + (uint32_t)((key - 1) % nt);
        r.z = (uint32_t)((int)(uint32_t)(v >> 32) - (1 << 30));
        r.w = (uint32_t)((int)(0xFFFFFFFFu - (uint32_t)v) - X);
        stage[atomicAdd(&staged, 1u)] = r;                 // (an LDS atomic; at most 256 per round, and a round starts with room for them)
    }
}

// ---- coverage ---------------------------------------------------------------------------------------------------------------
// two adds per record and array into a difference array (+ at the window's first covered position, - behind its last unless
// that is the target's end), then an inclusive scan per target.  Integer sums: independent of any order.
__global__ void __launch_bounds__(256)
k_scan_cover_add(const hmk_scan_hit *__restrict__ recs, uint64_t n, const uint8_t *__restrict__ len, const int32_t *__restrict__ sizes,
                 const uint64_t *__restrict__ toff, uint32_t t0, uint32_t *__restrict__ cc, unsigned long long *__restrict__ cs) {
    const uint64_t origin = toff[t0];
    for (uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (uint64_t)gridDim.x * 256) {
        const hmk_scan_hit h = recs[k];
        const uint64_t base = toff[h.target] - origin;
        const long long tn = (long long)(toff[h.target + 1] - toff[h.target]);
        const long long a = h.offset > 0 ? h.offset : 0;
        const long long b = (long long)h.offset + len[h.query] < tn ? (long long)h.offset + len[h.query] : tn;
        const unsigned long long size = sizes ? (unsigned long long)sizes[h.query] : 1ull;
        if (a >= tn || b <= a) continue;   // (cannot happen: max_shift < m keeps a residue of every window on the target)
        atomicAdd(&cc[base + a], 1u);
        atomicAdd(&cs[base + a], size);
        if (b < tn) {
            atomicAdd(&cc[base + b], 0xFFFFFFFFu);
            atomicAdd(&cs[base + b], 0ull - size);
        }
    }
}

// one workgroup per target at a time: 2,048 positions per step (8 per thread), the carry in registers
__global__ void __launch_bounds__(256)
k_scan_cover_scan(const uint64_t *__restrict__ toff, uint32_t t0, uint32_t nt, uint32_t *__restrict__ cc, unsigned long long *__restrict__ cs) {
    __shared__ uint32_t s32[256];
    __shared__ unsigned long long s64[256];
    const uint64_t origin = toff[t0];
    for (uint32_t t = blockIdx.x; t < nt; t += gridDim.x) {
        const uint64_t base = toff[t0 + t] - origin, tn = toff[t0 + t + 1] - toff[t0 + t];
        uint32_t carry32 = 0;
        unsigned long long carry64 = 0;
        for (uint64_t blk = 0; blk < tn; blk += 2048) {
            const uint64_t i0 = blk + (uint64_t)threadIdx.x * 8;
            uint32_t v32[8];
            unsigned long long v64[8];
            uint32_t t32 = 0;
            unsigned long long t64 = 0;
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const bool in = i0 + j < tn;
                t32 += in ? cc[base + i0 + j] : 0u;
                t64 += in ? cs[base + i0 + j] : 0ull;
                v32[j] = t32;
                v64[j] = t64;
            }
            __syncthreads();                               // the previous step's reads of s32 / s64 are done
            s32[threadIdx.x] = t32;
            s64[threadIdx.x] = t64;
            __syncthreads();
            for (uint32_t o = 1; o < 256; o <<= 1) {       // inclusive scan of the threads' sums
                const uint32_t a32 = threadIdx.x >= o ? s32[threadIdx.x - o] : 0u;
                const unsigned long long a64 = threadIdx.x >= o ? s64[threadIdx.x - o] : 0ull;
                __syncthreads();
                s32[threadIdx.x] += a32;
                s64[threadIdx.x] += a64;
                __syncthreads();
            }
            const uint32_t before32 = carry32 + s32[threadIdx.x] - t32;
            const unsigned long long before64 = carry64 + s64[threadIdx.x] - t64;
#pragma unroll
            for (int j = 0; j < 8; j++)
                if (i0 + j < tn) {
                    cc[base + i0 + j] = before32 + v32[j];
                    cs[base + i0 + j] = before64 + v64[j];
                }
            carry32 += s32[255];
            carry64 += s64[255];
        }
    }
}

uint32_t stride_grid(uint64_t n) { return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(4096, (n + 255) / 256)); }

template <int M>
void launch_packed_m(const ScanParams &P, uint32_t run0, uint32_t n_runs_m, hipStream_t s) {
    const uint64_t tiles = (uint64_t)P.n_chunks * n_runs_m;
    const uint32_t grid = capped_grid("k_scan_packed", (uint32_t)std::min<uint64_t>(tiles, 3072));
    hipLaunchKernelGGL((k_scan_packed<M>), dim3(grid), dim3(256), 0, s, P, run0, n_runs_m);
}

}  // namespace

hipError_t launch_scan_tables(const ScanParams &P, uint64_t *tables, hipStream_t s) {
    if (P.n_runs == 0) return hipSuccess;
    hipLaunchKernelGGL(k_scan_tables, dim3(capped_grid("k_scan_tables", std::min<uint32_t>(P.n_runs, 65536))), dim3(256), 0, s, P, tables);
    return hipGetLastError();
}

hipError_t launch_scan_packed(int m, const ScanParams &P, uint32_t run0, uint32_t n_runs_m, hipStream_t s) {
    if (n_runs_m == 0 || P.n_chunks == 0) return hipSuccess;
    switch (m) {
#define HMK_SCAN_M(L) case L: launch_packed_m<L>(P, run0, n_runs_m, s); break;
        HMK_SCAN_M(6) HMK_SCAN_M(7) HMK_SCAN_M(8) HMK_SCAN_M(9) HMK_SCAN_M(10) HMK_SCAN_M(11) HMK_SCAN_M(12) HMK_SCAN_M(13)
        HMK_SCAN_M(14) HMK_SCAN_M(15) HMK_SCAN_M(16) HMK_SCAN_M(17) HMK_SCAN_M(18) HMK_SCAN_M(19) HMK_SCAN_M(20)
#undef HMK_SCAN_M
        default: return hipErrorInvalidValue;   // no byte-lane kernel of that length: a missing kernel is an error
    }
    return hipGetLastError();
}

hipError_t launch_scan_literal(const ScanParams &P, hipStream_t s) {
    const uint64_t tiles = (uint64_t)P.n_chunks * P.n_runs;
    if (tiles == 0) return hipSuccess;
    hipLaunchKernelGGL(k_scan_literal, dim3(capped_grid("k_scan_literal", (uint32_t)std::min<uint64_t>(tiles, 3072))), dim3(256), 0, s, P);
    return hipGetLastError();
}

hipError_t launch_scan_pairs(const hmk_scan_hit *hits, uint64_t n, uint32_t q0, uint32_t t0, uint32_t nt, int X, unsigned long long *keys,
                             unsigned long long *vals, uint64_t slots, hmk_scan_hit *out, uint64_t out_cap, unsigned long long *count,
                             hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_scan_pair_insert, dim3(capped_grid("k_scan_pair_insert", stride_grid(n))), dim3(256), 0, s, hits, n, q0, t0, nt, X,
                       keys, vals, slots);
    hipLaunchKernelGGL(k_scan_pair_compact, dim3(capped_grid("k_scan_pair_compact", stride_grid(slots))), dim3(256), 0, s, keys, vals, slots,
                       q0, t0, nt, X, out, out_cap, count);
    return hipGetLastError();
}

hipError_t launch_scan_coverage(const hmk_scan_hit *recs, uint64_t n, const uint8_t *len, const int32_t *sizes, const uint64_t *toff,
                                uint32_t t0, uint32_t nt, uint32_t *cov_count, unsigned long long *cov_size, hipStream_t s) {
    if (nt == 0) return hipSuccess;
    if (n)
        hipLaunchKernelGGL(k_scan_cover_add, dim3(capped_grid("k_scan_cover_add", stride_grid(n))), dim3(256), 0, s, recs, n, len, sizes, toff,
                           t0, cov_count, cov_size);
    hipLaunchKernelGGL(k_scan_cover_scan, dim3(capped_grid("k_scan_cover_scan", std::min<uint32_t>(nt, 65536))), dim3(256), 0, s, toff, t0, nt,
                       cov_count, cov_size);
    return hipGetLastError();
}

}  // namespace hmk
