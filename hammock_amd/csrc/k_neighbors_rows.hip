// k_neighbors_rows.hip -- which row-packed instantiation (k_neighbors_rows.h) a (max shift, lengths) class runs, and the
// dispatch to the part (k_rows_part.hip) that holds it; the key entries and tile tables of a key-sorted plan.
#include "k_rows_shapes.h"

namespace hmk {

// column-length capacities of the capacity form
int rows_cap_for(int lb) { return lb <= 12 ? 12 : lb <= 16 ? 16 : lb <= 20 ? 20 : 0; }

namespace {
// part that holds the shape, or -1
int rows_part_of(int X, int d, int cap, bool exact) {
    if (exact) {
#define HMK_F(PV, XV, L) if (X == XV && d == 0 && cap == L) return PV;
        HMK_ROWS_EXACT_LIST(HMK_F)
#undef HMK_F
        return -1;
    }
#define HMK_C(PV, XV, DV, CAPV) if (X == XV && d == DV && cap == CAPV) return PV;
    HMK_ROWS_CAP_LIST(HMK_C)
#undef HMK_C
    return -1;
}
}  // namespace

int rows_per_tile_rows(int X, int d, int cap, bool exact, bool key_pairs) {
    if (rows_part_of(X, d, cap, exact) < 0) return 0;
    if (key_pairs) return rows_keyed(X, d, cap, exact, ROWS_KEY_PAIR_GROUPS) ? 8 * ROWS_KEY_PAIR_GROUPS : 0;
    return 8 * rows_groups(X, d, cap, exact);
}

// is there a row-packed instantiation for this class?  exact: every sequence of the set has length lb
bool rows_kernel_available(int X, int la, int lb, bool exact) {
    if (la < lb || lb < 2 * X || X < 1) return false;
    return rows_part_of(X, la - lb, exact ? lb : rows_cap_for(lb), exact) >= 0;
}

hipError_t launch_neighbors_rows(int X, int d, int cap, bool exact, const NeighborParams &P, uint32_t tile_base,
                                 uint32_t n_tiles, bool key_pairs, hipStream_t s) {
    if (n_tiles == 0) return hipSuccess;
    switch (rows_part_of(X, d, cap, exact)) {
#define HMK_P(p) case p: return launch_rows_part_##p(X, d, cap, exact, P, tile_base, n_tiles, key_pairs, s);
        HMK_P(0) HMK_P(1) HMK_P(2) HMK_P(3) HMK_P(4) HMK_P(5) HMK_P(6) HMK_P(7) HMK_P(8) HMK_P(9) HMK_P(10) HMK_P(11) HMK_P(12)
#undef HMK_P
    }
    return hipErrorInvalidValue;
}

hipError_t warm_neighbors_rows_module() { return warm_rows_part_0(); }

// One thread per keytab dword: entry (row group g, key q, residue c), dword 2u + h = byte t: cell(row 8g + 4h + t, key position + u - X, c)
// + bias, as the tile's table build (rows_tile) writes it -- zero for a row at or past n; dwords past the 2X + 1 planes zero.
// Key 0's entries hold the planes' START values as well: byte u of cinit (TileClass::cinit of the plan's one class) is added to
// every byte of dwords 2u, 2u + 1, so a row at or past n holds the initial lane alone -- what the kernel starts such a row at
// anyway.  No byte carries: initial lane + one cell is a partial sum of a lane classify() proved to end <= 255.
struct KeytabInit { uint32_t w[8]; };
__global__ void __launch_bounds__(256) k_rows_keytab(const uint8_t *__restrict__ res_sorted, uint32_t lpad, uint32_t n,
                                                     const uint8_t *__restrict__ mb, int case_b, int X, int L, const KeytabInit cinit,
                                                     uint32_t *__restrict__ keytab, uint32_t n_groups) {
    const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (uint64_t)n_groups * 2 * HMK_ALPHABET * KEYTAB_DWORDS) return;
    const int d = (int)(e % KEYTAB_DWORDS), c = (int)(e / KEYTAB_DWORDS % HMK_ALPHABET), q = (int)(e / (KEYTAB_DWORDS * HMK_ALPHABET) % 2);
    const uint32_t g = (uint32_t)(e / (2 * HMK_ALPHABET * KEYTAB_DWORDS));
    const int u = d >> 1, h = d & 1, i = rows_key_pos(X, L, q) + u - X;
    uint32_t v = 0;
    if (u <= 2 * X && i >= 0 && i < L) {
        for (int t = 0; t < 4; t++) {
            const uint32_t r = 8 * g + 4 * h + t;
            if (r < n) {
                const int a = res_sorted[(size_t)r * lpad + i];
                v |= (uint32_t)(case_b ? mb[c * HMK_ALPHABET + a] : mb[a * HMK_ALPHABET + c]) << (8 * t);
            }
        }
    }
    if (q == 0 && u <= 2 * X) v += ((cinit.w[u >> 2] >> ((u & 3) * 8)) & 0xFFu) * 0x01010101u;
    keytab[(size_t)g * KEYGROUP_DWORDS + e % KEYGROUP_KEY_DWORDS] = v;   // (the group's record: key entries, then its tile table)
}

// One thread per tile-table dword (hmk_internal.h, ROWS_TILE_TABLE): group g, row position k, residue c, half h = byte t: cell(row 8g + 4h
// + t, k, c) + bias, zero for a row at or past n -- the dword rows_tile's build writes at pos_addr(g, k) + 8c + 4h.  A row-shared group,
// by the planner's own rule (row_shared set: 8 live rows, equal at both key positions), holds its merged entries: at key position 0 the
// high dword is key position 1's.
__global__ void __launch_bounds__(256) k_rows_rowtab(const uint8_t *__restrict__ res_sorted, uint32_t lpad, uint32_t n,
                                                     const uint8_t *__restrict__ mb, int case_b, int X, int L, int row_shared,
                                                     uint32_t *__restrict__ keytab, uint32_t n_groups) {
    const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (uint64_t)n_groups * ROWTAB_DWORDS) return;
    const uint32_t g = (uint32_t)(e / ROWTAB_DWORDS);
    const int d = (int)(e % ROWTAB_DWORDS), h = d & 1, c = (d >> 1) % HMK_ALPHABET, k = d / (2 * HMK_ALPHABET);
    const int k0 = rows_key_pos(X, L, 0), k1 = rows_key_pos(X, L, 1);
    int i = k;
    if (row_shared && k == k0 && h == 1 && 8 * g + 8 <= n) {
        const uint8_t *first = res_sorted + (size_t)(8 * g) * lpad;
        bool same = true;
        for (int r = 1; r < 8; r++) same = same && first[(size_t)r * lpad + k0] == first[k0] && first[(size_t)r * lpad + k1] == first[k1];
        if (same) i = k1;
    }
    uint32_t v = 0;
    if (i < L) {
        for (int t = 0; t < 4; t++) {
            const uint32_t r = 8 * g + 4 * h + t;
            if (r < n) {
                const int a = res_sorted[(size_t)r * lpad + i];
                v |= (uint32_t)(case_b ? mb[c * HMK_ALPHABET + a] : mb[a * HMK_ALPHABET + c]) << (8 * t);
            }
        }
    }
    keytab[(size_t)g * KEYGROUP_DWORDS + KEYGROUP_KEY_DWORDS + d] = v;
}

hipError_t launch_rows_keytab(const uint8_t *res_sorted, uint32_t lpad, uint32_t n, const uint8_t *mb, int case_b, int X, int L,
                              const uint32_t (&cinit)[8], uint32_t *keytab, uint32_t n_groups) {
    const uint64_t total = (uint64_t)n_groups * 2 * HMK_ALPHABET * KEYTAB_DWORDS;
    if (total == 0) return hipSuccess;
    KeytabInit ci;
    for (int k = 0; k < 8; k++) ci.w[k] = cinit[k];
    hipLaunchKernelGGL(k_rows_keytab, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, nullptr, res_sorted, lpad, n, mb, case_b, X, L, ci,
                       keytab, n_groups);
    return hipGetLastError();
}

hipError_t launch_rows_rowtab(const uint8_t *res_sorted, uint32_t lpad, uint32_t n, const uint8_t *mb, int case_b, int X, int L,
                              bool row_shared, uint32_t *keytab, uint32_t n_groups) {
    const uint64_t total = (uint64_t)n_groups * ROWTAB_DWORDS;
    if (total == 0) return hipSuccess;
    if (L != ROWTAB_POSITIONS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_rows_rowtab, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, nullptr, res_sorted, lpad, n, mb, case_b, X, L,
                       row_shared ? 1 : 0, keytab, n_groups);
    return hipGetLastError();
}

}  // namespace hmk
