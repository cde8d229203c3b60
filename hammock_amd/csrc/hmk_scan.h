// hmk_scan.h -- what the scan of peptides along long targets (hmk_scan.cpp, k_scan.hip) shares between host and
// device: the work lists, the kernels' parameter block, and the rule that says which (peptide group, target) classes the byte-lane
// form may score (the launchers of k_scan.hip are declared in hmk_kernels.h).  The rule is plain C++ with no HIP in it:
// tests/tools/scan_host_check.cpp compiles it for the CPU.
#ifndef HMK_SCAN_H
#define HMK_SCAN_H

#include <stdint.h>

#include "../../include/hammock_hip.h"

#if defined(__HIP__) || defined(__HIPCC__)
#define HMK_SCAN_HD __host__ __device__
#else
#define HMK_SCAN_HD
#endif

namespace hmk {

constexpr uint32_t SCAN_CHUNK = 1024;        // windows of one target a workgroup stages at a time (tests/test_scan.py mirrors it)
constexpr uint32_t SCAN_GROUP = 8;           // peptides per table entry (E[i][c], 8 biased bytes)
constexpr uint32_t SCAN_RUN_GROUPS = 8;      // groups of one length a workgroup keeps tables of: a run is up to 64 peptides
constexpr uint32_t SCAN_COLUMNS = 25;        // the 24 residues and the sentinel beyond a target's ends (its cells hold the bias only)
constexpr uint32_t SCAN_SENTINEL = 24;
constexpr int SCAN_PACKED_MIN_LEN = 6, SCAN_PACKED_MAX_LEN = 20, SCAN_PACKED_MAX_SHIFT = 5;   // Hammock's domain: the byte-lane form's shapes
constexpr uint64_t SCAN_FIRST_HITS = 1u << 16;   // records the window-hit scratch holds at first (it grows to what a pass needed)

// up to SCAN_RUN_GROUPS groups of peptides of ONE length m: positions [first, first + count) of the call's length-sorted query list
struct ScanRun {
    uint32_t first, count, m;
    uint32_t table;      // where the run's tables start in ScanParams::tables (8-byte entries): [group][position][column]
    int32_t bound[SCAN_RUN_GROUPS];   // per group: no window of any of its peptides sums to more than this (scan_row_bound)
};
struct ScanChunk { uint32_t t, w0; };   // target, first window (offset + max_shift) of the chunk

struct ScanParams {
    const uint8_t *res32;        // the sequences' residues, 32 bytes each (ensure_res32)
    const uint32_t *qlist;       // the queries of the call sorted by (length, index)
    const ScanRun *runs;
    const ScanChunk *chunks;
    const uint8_t *tres;         // every target's residues
    const uint64_t *toff;        // ... and their offsets [n_targets + 1]
    const int32_t *M;            // the matrix, int32[576]
    const uint64_t *tables;      // k_scan_tables' output
    hmk_scan_hit *hits;          // window hits: `cap` records, *count = how many the pass found (stored: the first `cap`)
    unsigned long long *count;
    uint64_t cap;
    uint32_t n_runs, n_chunks;
    int X, p, thr, bias, max_m;
    uint32_t no_packed;          // HMK_NO_SCAN_PACKED: the literal form scores every class
};

// Sum over a peptide's residues of the best non-negative cell of the residue's matrix row: no window of the peptide, whatever
// its overlap with the target, sums to more (the rule of hmk_plan.cpp's row bounds; the peptide is seq1, so rows only).
inline long long scan_row_bound(const int32_t *M, const uint8_t *res, int m) {
    long long b = 0;
    for (int i = 0; i < m; i++) {
        long long best = 0;
        for (int c = 0; c < HMK_ALPHABET; c++) best = M[res[i] * HMK_ALPHABET + c] > best ? M[res[i] * HMK_ALPHABET + c] : best;
        b += best;
    }
    return b;
}

// The lane-range proof of the byte-lane form for peptides of length m against a target with d = n - m (classify()'s rule,
// hmk_plan.cpp, with d * p folded into the threshold).  A lane starts at g + penalty(s) - bias * m with g = 128 - (threshold - d p),
// adds m biased cells (>= 0 each, the sentinel's hold the bias alone) and ends at 128 + w - threshold; windows that hang over by
// k = 0 .. X residues pay 2 p k (ShiftedScorer.java:80-85).  Returns the largest row bound for which every lane of every window
// stays in [0, 255], or -1 when none does: a group of peptides takes the byte lanes iff its bound is <= this.
HMK_SCAN_HD inline long long scan_bound_limit(int m, int X, int p, int thr, long long d, int bias, int max_m) {
    if (m < SCAN_PACKED_MIN_LEN || m > SCAN_PACKED_MAX_LEN || X > SCAN_PACKED_MAX_SHIFT) return -1;
    if ((long long)max_m + bias > 255) return -1;
    const long long g = 128 - (long long)thr + d * p;
    long long limit = 1LL << 40;
    for (int k = 0; k <= X; k++) {
        const long long pen = 2LL * p * k;
        if (g + pen - (long long)bias * m < 0) return -1;
        const long long room = 255 - g - pen;
        limit = room < limit ? room : limit;
    }
    return limit < 0 ? -1 : limit;
}

}  // namespace hmk
#endif
