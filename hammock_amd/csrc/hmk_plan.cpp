// hmk_plan.cpp -- the planner of every neighbour pass.  The steps all plans share (length sort, kernel choice per class, the tiles
// of a row chunk, launch-group order, device copies, parameter checks); score bounds and lane classes (classify); the builders:
// build_plan (all-vs-all: triangle or full square), build_plan_search / build_plan_triangle (the rectangle of two ranges, the
// triangle of one), build_plan_local and build_plan_local_search (the LocalAlignmentScorer and GlobalAlignmentScorer passes).
#include "hmk_ctx.h"

namespace hmk { namespace impl {

// std::stable_sort's result on several threads: contiguous runs sorted on their own, then merged pairwise (std::merge takes
// from the left run on ties)
template <class T, class Cmp>
void parallel_stable_sort(std::vector<T> &v, Cmp before) {
    const size_t n = v.size();
    const unsigned hw = usable_cpus();
    size_t runs = 1;
    while (runs < 8 && runs < (hw ? hw : 1u) && n / (2 * runs) >= 32768) runs *= 2;
    if (runs == 1) { std::stable_sort(v.begin(), v.end(), before); return; }
    std::vector<size_t> cut(runs + 1);
    for (size_t r = 0; r <= runs; r++) cut[r] = n * r / runs;
    {
        std::vector<std::thread> pool;
        for (size_t r = 1; r < runs; r++) pool.emplace_back([&, r] { std::stable_sort(v.begin() + (long)cut[r], v.begin() + (long)cut[r + 1], before); });
        std::stable_sort(v.begin(), v.begin() + (long)cut[1], before);
        for (std::thread &th : pool) th.join();
    }
    std::vector<T> other(n);
    std::vector<T> *from = &v, *to = &other;
    for (size_t width = 1; width < runs; width *= 2) {
        std::vector<std::thread> pool;
        for (size_t r = 0; r < runs; r += 2 * width) {
            auto job = [&, r] {
                std::merge(from->begin() + (long)cut[r], from->begin() + (long)cut[r + width], from->begin() + (long)cut[r + width],
                           from->begin() + (long)cut[r + 2 * width], to->begin() + (long)cut[r], before);
            };
            if (r + 2 * width < runs) pool.emplace_back(job); else job();
        }
        for (std::thread &th : pool) th.join();
        std::swap(from, to);
    }
    if (from != &v) v.swap(other);
}

namespace {

// ---- the steps every builder shares ------------------------------------------------------------------------------------------
// bucket starts by length: the sequences of length l are the sorted positions [l] .. [l + 1]
using Buckets = uint32_t[HMK_MAX_LEN + 2];

// "sorted order": the caller ranges [a0, a1) and then [b0, b1) (empty: one range), each counting-sorted by length (stable: a
// bucket keeps the caller's order)
void sort_by_length(const hmk_ctx *ctx, uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1, Buckets &ba, Buckets &bb,
                    std::vector<uint32_t> &perm) {
    const uint32_t lo[2] = {a0, b0}, hi[2] = {a1, b1};
    uint32_t *const bucket[2] = {ba, bb};
    perm.resize((size_t)(a1 - a0) + (b1 - b0));
    for (int side = 0; side < 2; side++) {
        uint32_t *b = bucket[side];
        std::fill(b, b + HMK_MAX_LEN + 2, 0u);
        for (uint32_t k = lo[side]; k < hi[side]; k++) b[ctx->len[k] + 1]++;
        b[0] = side ? a1 - a0 : 0u;
        for (int l = 0; l <= HMK_MAX_LEN; l++) b[l + 1] += b[l];
        Buckets fill;
        std::memcpy(fill, b, sizeof(fill));
        for (uint32_t k = lo[side]; k < hi[side]; k++) perm[fill[ctx->len[k]]++] = k;
    }
}

// The kernel of a class: row-packed kernels (k_neighbors_rows.hip) take every 8-bit-lane class they have an instantiation for,
// the shift-packed or direct tiers the rest.  key = the launch group: (kernel family, entry dwords | length difference, column capacity)
using GroupKey = std::tuple<int, int, int>;
struct KernelChoice { bool rows; int lbk; uint32_t R; GroupKey key; };   // lbk: column capacity; R: rows per tile

KernelChoice choose_kernel(const TileClass &tc, int X, bool use_rows, bool rows_exact, bool exact, bool key_pairs = false) {
    const int la = tc.la, lb = tc.lb;
    KernelChoice k;
    k.rows = use_rows && tc.path == PATH_U8 && la >= lb && (rows_exact || rows_kernel_available(X, la, lb, false));
    k.lbk = k.rows ? (rows_exact ? lb : rows_cap_for(lb)) : exact ? 12 : swar_lbmax_for(lb);
    k.R = k.rows ? (uint32_t)rows_per_tile_rows(X, la - lb, k.lbk, rows_exact, key_pairs)
                 : tc.path == PATH_DIRECT ? 16u : (uint32_t)swar_rows_per_tile(k.lbk, tc.nw, exact);
    k.key = k.rows ? GroupKey((int)PATH_ROWS, la - lb, k.lbk)
                   : GroupKey((int)tc.path, tc.path == PATH_DIRECT ? 0 : (int)tc.nw, tc.path == PATH_DIRECT ? 0 : k.lbk);
    return k;
}

uint32_t add_class(std::vector<TileClass> &classes, hmk_neighbor_stats &S, const TileClass &tc, bool rows) {
    classes.push_back(tc);
    if (tc.path == PATH_U8) S.classes_u8++;
    else if (tc.path == PATH_U16) S.classes_u16++;
    else S.classes_direct++;
    if (rows) S.classes_rows++;
    return (uint32_t)classes.size() - 1;
}

// a band (build_plan): the tiles of a chunk whose rows are in it, or whose first column is below col_end, are flagged (Tile::pad0,
// host side only) and their pairs counted
struct Band { bool rows; uint32_t col_end; uint64_t pairs; };

// The tiles of the row chunk [r0, r0 + nr) against the columns [c_lo, c_hi), appended to dst; -> the pairs they hold.
// equal_runs: equal column runs of whole 256-column batches instead of full runs of `cols` + one short rest -- no tiny tiles whose
// table build is not amortised, and an even tail (the local plans take full runs).
// diag: rows and columns index the same sorted positions, and a tile that reaches the diagonal keeps only column > row (1) or
// drops the diagonal (2); 0: two different sets.  Tiles left without a pair are not emitted.
uint64_t emit_tiles(std::vector<Tile> &dst, uint32_t cls, uint32_t r0, uint32_t nr, uint32_t c_lo, uint32_t c_hi, uint32_t cols,
                    bool equal_runs, uint32_t diag, Band *band = nullptr) {
    if (c_lo >= c_hi) return 0;
    uint32_t run = cols;
    if (equal_runs) {
        const uint32_t k_runs = (c_hi - c_lo + cols - 1) / cols;
        run = std::min(cols, ((c_hi - c_lo + k_runs - 1) / k_runs + 255u) & ~255u);
    }
    uint64_t total = 0;
    for (uint32_t c0 = c_lo; c0 < c_hi; c0 += run) {
        Tile t{};
        t.row0 = r0; t.nrows = nr;
        t.col0 = c0; t.ncols = std::min(run, c_hi - c0);
        t.cls = cls;
        t.diag = (c0 < r0 + nr && c0 + t.ncols > r0) ? diag : 0u;
        uint64_t pairs = (uint64_t)nr * t.ncols;
        if (t.diag == 1) {
            pairs = 0;
            for (uint32_t r = r0; r < r0 + nr; r++) {
                const uint32_t lo = std::max(c0, r + 1), hi = c0 + t.ncols;
                if (hi > lo) pairs += hi - lo;
            }
        } else if (t.diag == 2) {
            for (uint32_t r = r0; r < r0 + nr; r++)
                if (r >= c0 && r < c0 + t.ncols) pairs--;
        }
        if (pairs == 0) continue;
        total += pairs;
        if (band && (band->rows || c0 < band->col_end)) {
            t.pad0 = 1u;
            band->pairs += pairs;
        }
        dst.push_back(t);
    }
    return total;
}

// The launch groups and the flat tile array they index.  Workgroups are dispatched in tile order: biggest tiles first keeps the
// tail of a launch short; band tiles before all others (they are launched on their own by hmk_greedy_cluster).
// (10^6 sequences: a million tiles; the stable sort of them was 30 of the plan's 55 ms on one thread)
std::vector<Tile> order_groups(std::map<GroupKey, std::vector<Tile>> &grouped, const std::vector<TileClass> &classes, int X,
                               std::vector<Group> &groups) {
    std::vector<Tile> tiles;
    for (auto &kv : grouped) {
        if (kv.second.empty()) continue;
        parallel_stable_sort(kv.second, [](const Tile &a, const Tile &b) {
            if (a.pad0 != b.pad0) return a.pad0 > b.pad0;
            return (uint64_t)a.nrows * a.ncols > (uint64_t)b.nrows * b.ncols;
        });
        uint32_t n_band = 0;
        uint64_t work = 0;
        for (const Tile &t : kv.second) {
            n_band += t.pad0;
            const TileClass &tc = classes[t.cls];
            const int lb = std::min((int)tc.la, (int)tc.lb), d = std::abs((int)tc.la - (int)tc.lb);
            work += (uint64_t)t.nrows * t.ncols * (uint64_t)std::max(1, lb * (2 * X + d + 1) - X * (X + 1));
        }
        groups.push_back(Group{std::get<0>(kv.first), std::get<1>(kv.first), std::get<2>(kv.first), (uint32_t)tiles.size(),
                               (uint32_t)kv.second.size(), n_band, work});
        tiles.insert(tiles.end(), kv.second.begin(), kv.second.end());
    }
    return tiles;
}

// The device copies every plan has.  Residues in sorted order: `stride` bytes per sequence (zero-padded) and `tail` bytes after
// the last, each residue times `mul` (the exact kernel reads them pre-multiplied by its entry size).
int upload_plan(hmk_ctx *ctx, PlanArrays &pl, const std::vector<uint32_t> &perm, size_t stride, size_t tail, int mul,
                const std::vector<TileClass> &classes, const std::vector<Tile> &tiles) {
    const uint32_t n = (uint32_t)perm.size();
    std::vector<uint8_t> res_sorted((size_t)n * stride + tail, 0);
    {   // (rows are independent: several threads for large sets -- 10 ms on one at 10^6)
        const unsigned hw = usable_cpus();
        const unsigned T = n >= (1u << 18) ? std::max(1u, std::min(8u, hw ? hw : 1u)) : 1u;
        auto fill = [&](uint32_t lo, uint32_t hi) {
            for (uint32_t s = lo; s < hi; s++) {
                const uint32_t k = perm[s];
                uint8_t *row = &res_sorted[(size_t)s * stride];
                if (mul == 1) std::memcpy(row, &ctx->res[ctx->off[k]], ctx->len[k]);
                else for (uint32_t q = 0; q < ctx->len[k]; q++) row[q] = (uint8_t)(ctx->res[ctx->off[k] + q] * mul);
            }
        };
        std::vector<std::thread> pool;
        for (unsigned t = 1; t < T; t++) pool.emplace_back(fill, (uint32_t)((uint64_t)n * t / T), (uint32_t)((uint64_t)n * (t + 1) / T));
        fill(0, (uint32_t)((uint64_t)n / T));
        for (std::thread &th : pool) th.join();
    }
    HIPCHK(ctx, hipMalloc((void **)&pl.d_res_sorted, res_sorted.size()));
    HIPCHK(ctx, hipMemcpy(pl.d_res_sorted, res_sorted.data(), res_sorted.size(), hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMalloc((void **)&pl.d_perm, (size_t)n * 4));
    HIPCHK(ctx, hipMemcpy(pl.d_perm, perm.data(), (size_t)n * 4, hipMemcpyHostToDevice));
    // (identity: the sorted positions ARE the caller indices -- one length; a rectangle's references right behind queries from 0)
    pl.perm_identity = true;
    for (uint32_t q = 0; q < n && pl.perm_identity; q++) pl.perm_identity = perm[q] == q;
    HIPCHK(ctx, hipMalloc((void **)&pl.d_classes, std::max<size_t>(1, classes.size()) * sizeof(TileClass)));
    if (!classes.empty())
        HIPCHK(ctx, hipMemcpy(pl.d_classes, classes.data(), classes.size() * sizeof(TileClass), hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMalloc((void **)&pl.d_tiles, std::max<size_t>(1, tiles.size()) * sizeof(Tile)));
    if (!tiles.empty())
        HIPCHK(ctx, hipMemcpy(pl.d_tiles, tiles.data(), tiles.size() * sizeof(Tile), hipMemcpyHostToDevice));
    return HMK_OK;
}

void free_arrays(PlanArrays &pl) {
    if (pl.d_res_sorted) (void)hipFree(pl.d_res_sorted);
    if (pl.d_perm) (void)hipFree(pl.d_perm);
    if (pl.d_classes) (void)hipFree(pl.d_classes);
    if (pl.d_tiles) (void)hipFree(pl.d_tiles);
}

// the matrix as biased bytes (what the shifted tiers' tables are built from)
int upload_biased_matrix(hmk_ctx *ctx, Plan &pl) {
    const int bias = ctx->min_m < 0 ? -ctx->min_m : 0;
    uint8_t mb[576];
    for (int e = 0; e < 576; e++) {
        const long long v = (long long)ctx->M[e] + bias;
        mb[e] = (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);  // only read by classes that passed the range check
    }
    HIPCHK(ctx, hipMalloc((void **)&pl.d_mb, 576));
    HIPCHK(ctx, hipMemcpy(pl.d_mb, mb, 576, hipMemcpyHostToDevice));
    return HMK_OK;
}

// what every shifted pass checks on its parameters after max_shift >= 0; `shortest`: the shortest sequence the pass scores
int check_shift_threshold_scores(hmk_ctx *ctx, int X, int p, int thr, int shortest) {
    if (X >= shortest)
        return fail(ctx, HMK_ERR_SHIFT_TOO_BIG, "Shift too big: " + std::to_string(shortest - 1) + " is maximum, but " + std::to_string(X) +
                                                    " found");  // ShiftedScorer.java:59-62
    if (thr < -30000 || thr > 30000) return fail(ctx, HMK_ERR_BAD_ARG, "threshold outside [-30000, 30000]");
    // edge scores travel as int16: the largest score any pair (of the whole set) can reach must fit
    const long long top = (long long)ctx->max_len * std::max(0, ctx->max_m) +
                          (long long)std::max(0, p) * ((ctx->max_len - ctx->min_len) + 2LL * X);
    if (top > 32767)
        return fail(ctx, HMK_ERR_BAD_ARG, "scores up to " + std::to_string(top) + " are possible with this matrix / shift penalty: "
                                           "they do not fit the int16 score of a packed edge");
    return HMK_OK;
}

}  // namespace

void free_plan(Plan &pl) {
    free_arrays(pl);
    if (pl.d_mb) (void)hipFree(pl.d_mb);
    if (pl.d_keyrun) (void)hipFree(pl.d_keyrun);
    if (pl.d_keytab) (void)hipFree(pl.d_keytab);
    pl = Plan();
}

void free_plan_local(PlanLocal &pl) {
    free_arrays(pl);
    pl = PlanLocal();
}

void free_plans(hmk_ctx *ctx) {
    for (Plan *pl : {&ctx->plan, &ctx->plan_search, &ctx->plan_assign, &ctx->plan_match, &ctx->plan_continue, &ctx->plan_continue_tri,
                     &ctx->plan_merge})
        free_plan(*pl);
    for (PlanLocal *pl : {&ctx->plan_local, &ctx->plan_global, &ctx->plan_local_search, &ctx->plan_local_assign, &ctx->plan_local_match}) free_plan_local(*pl);
}

// Lane layout of one (row length, column length) class; see DESIGN.md "SWAR tables".
// row_bound < 0: lanes are proven to fit for ANY pair of the class (every cell at the matrix maximum).
// row_bound >= 0: the caller guarantees score(row, anything) <= row_bound for the rows it will put into
// this class (sum of the row residues' best cells), which lets long peptides keep 8-bit lanes.
// *u8_row_limit receives the largest row_bound for which 8-bit lanes fit (or -1 if they never do).
void classify(const hmk_ctx *ctx, int la, int lb, int X, int p, int thr, TileClass *out, long long row_bound,
              long long *u8_row_limit) {
    TileClass c{};
    const int m = std::min(la, lb), nl = std::max(la, lb);
    const int d = nl - m;
    const int nd = 2 * X + d + 1;
    c.la = (uint8_t)la;
    c.lb = (uint8_t)lb;
    c.nd = (uint8_t)std::min(nd, 255);
    c.case_b = lb < la;
    c.x = (uint8_t)X;
    c.d = d;
    const int bias = ctx->min_m < 0 ? -ctx->min_m : 0;
    const long long cell_max = (long long)ctx->max_m + bias;
    c.path = PATH_DIRECT;
    for (int attempt = 0; attempt < 2 && c.path == PATH_DIRECT; attempt++) {
        const bool u16 = attempt == 1;
        const long long lane_max = u16 ? 65535 : 255;
        const long long g = (u16 ? 32768LL : 128LL) - thr;
        const int max_nd = u16 ? 16 : 32;
        if (nd > max_nd || cell_max > 255) continue;
        bool ok = true, lower_ok = true;
        long long ci[32], limit = 1LL << 40;
        for (int t = 0; t < nd; t++) {
            const int s = t - X;
            const long long ncell = s <= 0 ? m + s : std::min(m, nl - s);
            long long pen = (long long)d * p;                       // ShiftedScorer.java:79
            if (s < 0) pen += (long long)(-s) * 2 * p;              // :80-82
            if (s > d) pen += (long long)(s - d) * 2 * p;           // :83-85
            const long long c0 = g + pen - bias * ncell;            // lane value = g + pen + sum of the cells
            if (c0 < 0) lower_ok = false;
            const long long top = row_bound >= 0 ? g + pen + row_bound : c0 + ncell * cell_max;
            if (top > lane_max) ok = false;
            limit = std::min(limit, lane_max - g - pen);
            ci[t] = c0;
        }
        if (!u16 && u8_row_limit) *u8_row_limit = lower_ok ? limit : -1;
        if (!ok || !lower_ok) continue;
        c.path = u16 ? PATH_U16 : PATH_U8;
        c.g = (int32_t)g;
        const int lpd = u16 ? 2 : 4, bits = u16 ? 16 : 8;
        const int ndw = (nd + lpd - 1) / lpd;
        c.nw = (uint8_t)ndw;  // 1..8 dwords per table entry, each count has its own kernel
        for (int t = 0; t < nd; t++) c.cinit[t / lpd] |= (uint32_t)ci[t] << ((t % lpd) * bits);
    }
    *out = c;
}

// band_rows: tiles that touch a sequence with caller index < band_rows are put first in every launch group, so that a
// first launch of only those tiles completes the adjacency rows phase 1 of the greedy merge reads first
// (hmk_greedy_cluster); -1 = the caller does not care (any cached plan with the other parameters will do).
int build_plan(hmk_ctx *ctx, int X, int p, int thr, uint32_t part, uint32_t n_parts, int64_t band_rows, bool key_sort_ok) {
    Plan &pl = ctx->plan;
    const int want_keys = key_sort_ok ? ctx->sw.key_sort : 0;
    if (pl.valid && pl.X == X && pl.p == p && pl.thr == thr && pl.part == part && pl.n_parts == n_parts &&
        (band_rows < 0 || pl.band_req == band_rows) && pl.no_rows_kernel == ctx->sw.no_rows_kernel && pl.key_sort == want_keys &&
        pl.row_shared == !ctx->sw.no_row_shared && pl.key_row_pairs == ctx->sw.key_row_pairs && pl.row_run_share == !ctx->sw.no_row_run_share &&
        pl.tile_tables == !ctx->sw.no_tile_tables)
        return HMK_OK;
    free_plan(pl);
    if (band_rows < 0) band_rows = 0;
    const int64_t band_req = band_rows;
    const bool plan_timing = ctx->sw.greedy_timing;
    const auto plan_t0 = std::chrono::steady_clock::now();
    auto plan_lap = [&](const char *what) {
        if (plan_timing)
            fprintf(stderr, "[hmk plan] %s at %.2f ms\n", what,
                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - plan_t0).count());
    };
    const uint32_t n = ctx->n;
    if (n == 0) return fail(ctx, HMK_ERR_NO_SEQUENCES, "no sequences set (hmk_set_sequences)");
    if (X < 0) return fail(ctx, HMK_ERR_BAD_ARG, "max_shift must be >= 0");
    if (n_parts == 0 || part >= n_parts) return fail(ctx, HMK_ERR_BAD_ARG, "part must be < n_parts");
    int st = check_shift_threshold_scores(ctx, X, p, thr, ctx->min_len);
    if (st) return st;

    Buckets bucket, none;
    std::vector<uint32_t> perm;
    sort_by_length(ctx, 0, n, 0, 0, bucket, none, perm);
    // Per-sequence score bound: no pair involving sequence k scores above bound[k] = sum over its residues
    // of the best (non-negative) cell of that residue's matrix row/column.  If some class does not fit
    // 8-bit lanes for arbitrary pairs, its bucket is ordered by this bound and the rows below the class's
    // limit still run on 8-bit lanes (for BLOSUM62 a 20-mer's bound is its self-score, ~112 +- 8, against
    // a limit of 127 + threshold).
    bool refine = false;
    for (int la = 1; la <= HMK_MAX_LEN && !refine; la++)
        for (int lb = 1; lb <= HMK_MAX_LEN && !refine; lb++) {
            if (bucket[la] == bucket[la + 1] || bucket[lb] == bucket[lb + 1]) continue;
            if (ctx->symmetric && lb > la) continue;
            TileClass tc;
            long long limit = -1;
            classify(ctx, la, lb, X, p, thr, &tc, -1, &limit);
            if (tc.path != PATH_U8 && limit >= 0) refine = true;
        }
    std::vector<uint32_t> bound_sorted;  // bound of the sequence at each sorted position (refine only)
    constexpr uint32_t BCAP = 4095;      // bounds are only compared with limits < 65536; clamped for the counting sort
    // refine, but EVERY row of every class that needs its bound has one within the class's limit (uniform 15- or 20-mers at the
    // reference's default threshold: a 20-mer's bound is ~112 +- 8 against a limit of 161): the buckets keep the caller's order
    // -- no reordering, so the band of a clustering call survives and a one-length set keeps its compile-time-length kernel
    bool all_rows_fit = false;
    if (refine) {
        long long best[HMK_ALPHABET];
        for (int a = 0; a < HMK_ALPHABET; a++) {
            long long b = 0;
            for (int y = 0; y < HMK_ALPHABET; y++)
                b = std::max<long long>(b, std::max(ctx->M[a * HMK_ALPHABET + y], ctx->M[y * HMK_ALPHABET + a]));
            best[a] = b;
        }
        std::vector<uint32_t> bound(n);
        for (uint32_t k = 0; k < n; k++) {
            long long b = 0;
            for (uint32_t q = ctx->off[k]; q < ctx->off[k + 1]; q++) b += best[ctx->res[q]];
            bound[k] = (uint32_t)std::min<long long>(b, BCAP);
        }
        {
            uint32_t bucket_max[HMK_MAX_LEN + 2] = {0};
            for (uint32_t k = 0; k < n; k++) bucket_max[ctx->len[k]] = std::max(bucket_max[ctx->len[k]], bound[k]);
            all_rows_fit = true;
            for (int la = 1; la <= HMK_MAX_LEN && all_rows_fit; la++)
                for (int lb = 1; lb <= HMK_MAX_LEN && all_rows_fit; lb++) {
                    if (bucket[la] == bucket[la + 1] || bucket[lb] == bucket[lb + 1]) continue;
                    if (ctx->symmetric && lb > la) continue;
                    TileClass tc;
                    long long limit = -1;
                    classify(ctx, la, lb, X, p, thr, &tc, -1, &limit);
                    if (tc.path == PATH_U8) continue;
                    if (limit < 0 || (long long)bucket_max[la] > std::min<long long>(limit, BCAP - 1)) all_rows_fit = false;
                }
        }
        // stable counting sort of every length bucket by bound
        std::vector<uint32_t> sorted(n), cnt(BCAP + 2);
        for (int l = 1; l <= HMK_MAX_LEN && !all_rows_fit; l++) {
            const uint32_t b0 = bucket[l], b1 = bucket[l + 1];
            if (b0 == b1) continue;
            std::fill(cnt.begin(), cnt.end(), 0u);
            for (uint32_t q = b0; q < b1; q++) cnt[bound[perm[q]] + 1]++;
            for (uint32_t v = 0; v <= BCAP; v++) cnt[v + 1] += cnt[v];
            for (uint32_t q = b0; q < b1; q++) sorted[b0 + cnt[bound[perm[q]]]++] = perm[q];
        }
        if (!all_rows_fit) perm.swap(sorted);
        bound_sorted.resize(n);
        for (uint32_t q = 0; q < n; q++) bound_sorted[q] = bound[perm[q]];
    }
    // band members of a length bucket are its leading sorted positions (the counting sort keeps caller order); a
    // bucket reordered by score bound has no such prefix, so the band is dropped there (phase 1 then waits for the pass)
    uint32_t band_end[HMK_MAX_LEN + 2];
    if (refine && !all_rows_fit) band_rows = 0;
    for (int l = 0; l <= HMK_MAX_LEN; l++) {
        band_end[l] = bucket[l];
        if (band_rows > 0)
            while (band_end[l] < bucket[l + 1] && perm[band_end[l]] < (uint64_t)band_rows) band_end[l]++;
    }
    pl.band_rows = (uint32_t)band_rows;
    pl.band_req = band_req;
    plan_lap("buckets and score bounds");
    pl.lbmax = swar_lbmax_for(ctx->max_len);
    pl.lpad = ctx->max_len <= 16 ? 16 : 32;
    // The exact hot kernel: every sequence has length 12, max shift 3, and the (12, 12) class fits 8-bit
    // lanes in 8-byte entries.  It reads residues pre-multiplied by the entry size (upload_plan's mul).
    // A set of one length may have a row-packed kernel with the length at compile time.  HMK_NO_ROWS_KERNEL=1: the shift-packed
    // kernels of round 1-2.
    const bool use_rows = !ctx->sw.no_rows_kernel;
    pl.no_rows_kernel = ctx->sw.no_rows_kernel;
    pl.exact = false;
    pl.rows_exact = false;
    if (use_rows && ctx->min_len == ctx->max_len) {
        TileClass t1;
        classify(ctx, ctx->min_len, ctx->min_len, X, p, thr, &t1);
        // (8-bit lanes for any pair of the class, or -- by their score bounds -- for every row the set has)
        pl.rows_exact = (t1.path == PATH_U8 || (refine && all_rows_fit)) && rows_kernel_available(X, ctx->min_len, ctx->min_len, true);
    }
    if (!use_rows && ctx->min_len == 12 && ctx->max_len == 12 && X == 3) {
        TileClass t12;
        classify(ctx, 12, 12, X, p, thr, &t12);
        pl.exact = t12.path == PATH_U8 && t12.nw == 2;
    }
    // Key sort: a one-length set whose bucket keeps the caller's order and runs a rows_keyed shape is ordered by the
    // residues at the two key positions -- all but a band prefix, which keeps the caller's order (band_end stays what it is) -- with
    // a stable counting sort.  Run ids over the whole order: equal at a window's two ends <=> the window shares the key.  Plain
    // single-part passes only (key_sort_ok): a clustering call's scoring counts degrees per row group and its CSR build reads the
    // edges in row order (both slower on the sorted order: 10^5 call 4.04 -> 4.44 ms), and shards keep their caller-order rows.
    pl.key_sort = want_keys;
    pl.row_shared = !ctx->sw.no_row_shared;
    pl.key_row_pairs = ctx->sw.key_row_pairs;
    pl.row_run_share = !ctx->sw.no_row_run_share;
    pl.tile_tables = !ctx->sw.no_tile_tables;
    std::vector<uint32_t> keyrun;
    const int L1 = ctx->min_len;
    const bool key_sorted = pl.key_sort > 0 && pl.rows_exact && !(refine && !all_rows_fit) &&
                            rows_keyed(X, 0, L1, true, rows_per_tile_rows(X, 0, L1, true) / 8) && n >= 2;
    if (key_sorted) {
        const int k0 = rows_key_pos(X, L1, 0), k1 = rows_key_pos(X, L1, 1);
        auto key_of = [&](uint32_t k) { return (uint32_t)ctx->res[ctx->off[k] + k0] * HMK_ALPHABET + ctx->res[ctx->off[k] + k1]; };
        const uint32_t b0 = band_end[L1], b1 = bucket[L1 + 1];
        std::vector<uint32_t> cnt(HMK_ALPHABET * HMK_ALPHABET + 1, 0u), sorted(perm.begin() + b0, perm.begin() + b1);
        for (uint32_t q = b0; q < b1; q++) cnt[key_of(perm[q]) + 1]++;
        for (int v = 0; v < HMK_ALPHABET * HMK_ALPHABET; v++) cnt[v + 1] += cnt[v];
        for (uint32_t q = b0; q < b1; q++) sorted[cnt[key_of(perm[q])]++] = perm[q];
        std::copy(sorted.begin(), sorted.end(), perm.begin() + b0);
        keyrun.resize(2 * (size_t)n);
        uint32_t r0 = 0, r01 = 0;
        for (uint32_t q = 0; q < n; q++) {
            const uint32_t k = perm[q], c0 = ctx->res[ctx->off[k] + k0], c1 = ctx->res[ctx->off[k] + k1];
            if (q > 0) {
                const uint32_t kp = perm[q - 1];
                const bool same0 = ctx->res[ctx->off[kp] + k0] == c0;
                r0 += same0 ? 0u : 1u;
                r01 += (pl.key_sort == 2 && same0 && ctx->res[ctx->off[kp] + k1] == c1) ? 0u : 1u;   // (one key: no window shares both)
            }
            keyrun[2 * (size_t)q] = r0 << 5 | c0;
            keyrun[2 * (size_t)q + 1] = r01 << 5 | c1;
        }
    }
    // Column runs: long runs amortise the table build (65,536 columns: 3.55 ms for the whole 10^5 pass against
    // 3.60 ms with 16,384), short ones keep the tail of a small launch short (a 1/8 shard: 0.478 ms with 16,384,
    // 0.532 ms with 65,536).  Take the longest run that still leaves ~8 rounds of workgroups (256 CUs x 7).
    auto tiles_about = [&](uint64_t tile_rows, uint32_t cols) { return ((uint64_t)n / tile_rows / n_parts + 1) * ((uint64_t)n / (2 * cols) + 1); };
    auto cols_for = [&](uint64_t tile_rows) {
        uint32_t cols = 65536;
        while (cols > 16384 && tiles_about(tile_rows, cols) < 8 * 1792) cols /= 2;
        return cols;
    };
    // Paired tiles (k_neighbors_rows.h): a key-sorted plan takes 16-row tiles -- two row groups behind one column
    // set-up -- when the 16-row plan still has KEY_PAIR_MIN_TILES tiles, six rounds of the 2,048 workgroup slots (256 CUs x 8).  The
    // constant lies just below the smallest plan pairing was measured on (74,041 12-mers, about 13,900 tiles, -1.2 % and
    // -2.2 % in two sessions; 10^5, about 25,000, -2.3 %); small sets, which do not fill the slots even with 8-row tiles, keep those.  HMK_KEY_ROW_PAIRS=0|1
    // overrides the rule.
    constexpr uint64_t KEY_PAIR_MIN_TILES = 6 * 2048;
    const uint64_t paired_rows = key_sorted ? (uint64_t)rows_per_tile_rows(X, 0, L1, true, true) : 0;
    pl.key_pairs = paired_rows != 0 && (ctx->sw.key_row_pairs >= 0 ? ctx->sw.key_row_pairs == 1
                                                                   : tiles_about(paired_rows, cols_for(paired_rows)) >= KEY_PAIR_MIN_TILES);
    const uint64_t tile_rows = pl.key_pairs ? paired_rows : pl.rows_exact ? (uint64_t)rows_per_tile_rows(X, 0, ctx->min_len, true) : use_rows ? 16 : 6;
    pl.cols_per_tile = cols_for(tile_rows);
    // (not below 4,096 columns: a tile's dead time -- its chain of dependent loads before the first table read, the flush after
    // the last -- is about four 256-column batches long, and short tiles pay it several times over on every workgroup slot.
    // 10^4 12-mers: 1,024 / 2,048 / 4,096 / 16,384 columns per tile 0.090 / 0.061 / 0.053 / 0.051 ms, although the last leaves
    // a third of the slots empty; 3 x 10^4: 2,048 / 4,096 / 8,192 0.354 / 0.301 / 0.294 ms.)
    while (pl.cols_per_tile > 4096 && ((uint64_t)n / tile_rows + 1) * ((uint64_t)n / (2 * pl.cols_per_tile) + 1) < 4096)
        pl.cols_per_tile /= 2;

    // ---- classes and tiles --------------------------------------------------------
    std::vector<TileClass> classes;
    std::map<GroupKey, std::vector<Tile>> grouped;
    hmk_neighbor_stats &S = pl.stats;
    S = hmk_neighbor_stats{};
    S.symmetric = ctx->symmetric;
    uint64_t row_chunk_counter = 0;   // over every chunk of every class, in class order: chunk c belongs to part c % n_parts
    for (int la = 1; la <= HMK_MAX_LEN; la++) {
        const uint32_t rb = bucket[la], re = bucket[la + 1];
        if (rb == re) continue;
        for (int lb = 1; lb <= HMK_MAX_LEN; lb++) {
            const uint32_t cb = bucket[lb], ce = bucket[lb + 1];
            if (cb == ce) continue;
            // unordered pairs: the LONGER bucket supplies the rows, so a pair costs one table lookup per
            // residue of its SHORTER sequence (the column), ShiftedScorer.java:51-57 decides S/L by length anyway
            if (ctx->symmetric && lb > la) continue;
            const bool same = la == lb;
            if (same && re - rb < 2) continue;
            // row ranges of this (la, lb) pair: all rows in one class, or -- when 8-bit lanes do not fit every
            // conceivable pair -- the rows whose score bound fits (8-bit lanes) and the rest (16-bit / literal)
            struct Range { uint32_t lo, hi; TileClass tc; };
            std::vector<Range> ranges;
            {
                TileClass tc0;
                long long limit = -1;
                classify(ctx, la, lb, X, p, thr, &tc0, -1, &limit);
                uint32_t split = rb;  // rows [rb, split) fit 8-bit lanes by their bound
                if (refine && tc0.path != PATH_U8 && limit >= 0) {
                    const uint32_t lim = (uint32_t)std::min<long long>(limit, BCAP - 1);  // a clamped bound never passes
                    split = all_rows_fit ? re   // (caller order kept: every row of the bucket is within the limit)
                                         : (uint32_t)(std::upper_bound(bound_sorted.begin() + rb, bound_sorted.begin() + re, lim) -
                                                      bound_sorted.begin());
                    if (split > rb) {
                        TileClass t8;
                        classify(ctx, la, lb, X, p, thr, &t8, lim);
                        if (t8.path == PATH_U8) ranges.push_back(Range{rb, split, t8});
                        else split = rb;
                    }
                }
                if (split < re) ranges.push_back(Range{split, re, tc0});
            }
            for (const Range &rg : ranges) {
                const KernelChoice k = choose_kernel(rg.tc, X, use_rows, pl.rows_exact, pl.exact, pl.key_pairs);
                const uint32_t cls = add_class(classes, S, rg.tc, k.rows);
                std::vector<Tile> &dst = grouped[k.key];
                const bool tri = same && ctx->symmetric;   // triangle: the columns after the first row of a chunk, column > row
                for (uint32_t r0 = rg.lo; r0 < rg.hi; r0 += k.R) {
                    if ((row_chunk_counter++ % n_parts) != part) continue;
                    Band band{r0 < band_end[la], band_end[lb], 0};
                    S.pairs_scored += emit_tiles(dst, cls, r0, std::min(k.R, rg.hi - r0), tri ? r0 + 1 : cb, ce, pl.cols_per_tile, true,
                                                 tri ? 1u : same ? 2u : 0u, &band);
                    pl.band_pairs += band.pairs;
                }
            }
        }
    }
    plan_lap("classes and tiles");
    std::vector<Tile> tiles = order_groups(grouped, classes, X, pl.groups);
    S.n_tiles = (uint32_t)tiles.size();
    plan_lap("tile order");
    // Row-shared groups of a key-sorted plan (k_neighbors_rows.h, RowsShape::rs_row): 8 live rows with the same residue at key
    // position 0 and the same at key position 1.  A group with a row past the end never is: the merged entries would add cells to
    // the dead rows' lanes that their zero entries do not.
    if (key_sorted && pl.row_shared) {
        const int k0 = rows_key_pos(X, L1, 0), k1 = rows_key_pos(X, L1, 1);
        auto keys_at = [&](uint32_t q) { const uint32_t k = perm[q]; return (uint32_t)ctx->res[ctx->off[k] + k0] << 8 | ctx->res[ctx->off[k] + k1]; };
        for (Tile &t : tiles) {
            for (uint32_t g = 0; 8 * g + 8 <= t.nrows; g++) {
                bool same = true;
                for (uint32_t r = 1; r < 8 && same; r++) same = keys_at(t.row0 + 8 * g + r) == keys_at(t.row0 + 8 * g);
                if (same) t.row_shared |= 1u << g;
            }
            // Run-shared tiles of a paired plan (k_neighbors_rows.h, accumulate_run): 16 live rows, both groups row-shared with the
            // SAME two key residues -- the second group's merged cells are the first group's, which hands them over in registers.
            if (pl.key_pairs && pl.row_run_share && t.nrows == 8u * ROWS_KEY_PAIR_GROUPS && (t.row_shared & 3u) == 3u &&
                keys_at(t.row0 + 8) == keys_at(t.row0))
                t.row_shared |= ROWS_RUN_SHARED;
        }
        plan_lap("row-shared groups");
    }
    // Tile tables (hmk_internal.h, ROWS_TILE_TABLE): what a tile's table build writes depends on the sorted residues, the matrix and the
    // group's row-shared flag only -- the same in every pass on this plan, and about eleven tiles per row group build it again in each.  The
    // plan builds the tables once, below, and every tile copies its groups'.  (One class, chunks from position 0 in steps of 8 or 16 rows:
    // group g of a tile is row group (row0 >> 3) + g.)
    const bool tile_tables = key_sorted && pl.tile_tables && L1 == ROWTAB_POSITIONS;
    if (tile_tables)
        for (Tile &t : tiles) t.row_shared |= ROWS_TILE_TABLE;
    pl.table_tiles = tile_tables ? (uint32_t)tiles.size() : 0u;
    pl.table_bytes = tile_tables ? (uint64_t)((n + 7) / 8) * ROWTAB_DWORDS * 4 : 0u;
    pl.paired_tiles = pl.key_pairs ? (uint32_t)tiles.size() : 0u;
    pl.run_shared_tiles = 0;
    for (const Tile &t : tiles) pl.run_shared_tiles += (t.row_shared & ROWS_RUN_SHARED) ? 1u : 0u;

    // ---- device copies ------------------------------------------------------------
    // (+ 16: the row-packed kernel's unaligned tail loads may touch the bytes after the last row)
    st = upload_plan(ctx, pl, perm, (size_t)pl.lpad, 16, pl.exact ? 8 : 1, classes, tiles);
    if (!st) st = upload_biased_matrix(ctx, pl);
    if (st) return st;
    if (key_sorted) {   // run ids, and the key table built on the device from the sorted residues (hipMemcpy above: they are there)
        // (the table holds the class's initial lanes, which depend on (X, p, thr): it lives and dies with this plan, whose cache
        // key those are; a key-sorted plan has the one class of its one length)
        if (classes.size() != 1) return fail(ctx, HMK_ERR_DEVICE, "key-sorted plan with more than one class");
        const uint32_t n_groups = (n + 7) / 8;
        const size_t tab_dwords = (size_t)n_groups * KEYGROUP_DWORDS;
        HIPCHK(ctx, hipMalloc((void **)&pl.d_keyrun, keyrun.size() * 4));
        HIPCHK(ctx, hipMemcpy(pl.d_keyrun, keyrun.data(), keyrun.size() * 4, hipMemcpyHostToDevice));
        HIPCHK(ctx, hipMalloc((void **)&pl.d_keytab, tab_dwords * 4));
        HIPCHK(ctx, launch_rows_keytab(pl.d_res_sorted, (uint32_t)pl.lpad, n, pl.d_mb, classes.at(0).case_b, X, L1, classes.at(0).cinit, pl.d_keytab,
                                       n_groups));
        if (tile_tables)
            HIPCHK(ctx, launch_rows_rowtab(pl.d_res_sorted, (uint32_t)pl.lpad, n, pl.d_mb, classes.at(0).case_b, X, L1, pl.row_shared, pl.d_keytab,
                                           n_groups));
        HIPCHK(ctx, hipStreamSynchronize(nullptr));
    }
    pl.X = X; pl.p = p; pl.thr = thr; pl.part = part; pl.n_parts = n_parts;
    pl.valid = true;
    plan_lap("device copies");
    return HMK_OK;
}

// The rectangle of a shifted search.  One class per (query length, reference length); every tile holds rows of one side and a
// column run of the other (no triangle: Tile::diag = 0, no pair inside one side).  Which side supplies the rows:
//   symmetric matrix  the side with the LONGER sequences (the row-packed kernels need row length >= column length), at equal lengths
//                     the side with MORE sequences (rows are the parallel dimension: 10^2 queries x 10^5 references are 6,250
//                     row groups of references, not 13 of queries).  The kernels emit (min, max) caller indices; the search turns
//                     every edge to m = query afterwards (k_search.hip).
//   asymmetric        the references: every shifted tier scores sequenceScore(seq1 = column, seq2 = row) and emits (x = row,
//                     m = column) (k_neighbors.hip, the all-vs-all asymmetric pass), so with the queries as columns the edges
//                     come out m = query = seq1 as they are.  Classes the row-packed kernels cannot take (row length < column
//                     length) run on the shift-packed or direct tiers, as in the all-vs-all asymmetric pass.
// No score-bound refinement (build_plan's `refine`): a class whose 8-bit lanes do not fit every pair runs on 16-bit lanes.
// No key sort, no band, no parts.
// tri (build_plan_triangle): the TRIANGLE of the pairs inside the one range [q0, q1) = [r0, r1) -- hmk_greedy_continue's new x new --
// under a symmetric matrix: the range is sorted once, the longer bucket supplies the rows, and a class of one length keeps the
// columns after each row (Tile::diag = 1, as build_plan's triangle); edges (min, max) as above.
static int build_plan_rect(hmk_ctx *ctx, Plan &pl, int X, int p, int thr, uint32_t q0, uint32_t q1, uint32_t r0, uint32_t r1, bool tri) {
    if (pl.valid && pl.X == X && pl.p == p && pl.thr == thr && pl.q0 == q0 && pl.q1 == q1 && pl.r0 == r0 && pl.r1 == r1 &&
        pl.no_rows_kernel == ctx->sw.no_rows_kernel)
        return HMK_OK;
    free_plan(pl);
    if (tri && !ctx->symmetric) return fail(ctx, HMK_ERR_BAD_ARG, "a triangle plan needs a symmetric matrix");
    Buckets bq, br;
    std::vector<uint32_t> perm;
    sort_by_length(ctx, q0, q1, r0, tri ? r0 : r1, bq, br, perm);
    if (tri) std::memcpy(br, bq, sizeof(br));   // (one range: rows and columns index the same sorted positions)
    int mn = HMK_MAX_LEN, mx = 1;
    for (int l = 1; l <= HMK_MAX_LEN; l++)
        if (bq[l] != bq[l + 1] || br[l] != br[l + 1]) { mn = std::min(mn, l); mx = std::max(mx, l); }
    pl.lpad = mx <= 16 ? 16 : 32;
    pl.lbmax = swar_lbmax_for(mx);
    const bool use_rows = !ctx->sw.no_rows_kernel;
    pl.no_rows_kernel = ctx->sw.no_rows_kernel;
    pl.exact = false;
    pl.rows_exact = false;
    if (use_rows && mn == mx) {
        TileClass t1;
        classify(ctx, mn, mn, X, p, thr, &t1);
        pl.rows_exact = t1.path == PATH_U8 && rows_kernel_available(X, mn, mn, true);
    }

    struct Cls { TileClass tc; KernelChoice k; bool tri; uint32_t rb, re, cb, ce; };
    std::vector<Cls> cl;
    for (int lq = 1; lq <= HMK_MAX_LEN; lq++) {
        const uint32_t nql = bq[lq + 1] - bq[lq];
        if (!nql) continue;
        for (int lr = 1; lr <= HMK_MAX_LEN; lr++) {
            const uint32_t nrl = br[lr + 1] - br[lr];
            if (!nrl) continue;
            if (tri && (lr > lq || (lq == lr && nql < 2))) continue;   // (unordered pairs: the longer bucket supplies the rows)
            const bool rows_q = tri || (ctx->symmetric && (lq > lr || (lq == lr && nql >= nrl)));
            Cls c{};
            c.tri = tri && lq == lr;
            c.rb = rows_q ? bq[lq] : br[lr]; c.re = rows_q ? bq[lq + 1] : br[lr + 1];
            c.cb = rows_q ? br[lr] : bq[lq]; c.ce = rows_q ? br[lr + 1] : bq[lq + 1];
            classify(ctx, rows_q ? lq : lr, rows_q ? lr : lq, X, p, thr, &c.tc);
            c.k = choose_kernel(c.tc, X, use_rows, pl.rows_exact, false);
            cl.push_back(c);
        }
    }
    // Column runs from the rectangle (not from n): the longest run that still leaves ~8 rounds of workgroups (256 CUs x 7), not
    // below 4,096 columns (a tile's dead time, build_plan) -- unless the rows alone make less than one round (a handful of rows
    // against many columns: 5 references x 5 x 10^4 queries under an asymmetric matrix), where shorter runs are the only parallelism.
    uint64_t row_groups = 0;
    for (const Cls &c : cl) row_groups += (c.re - c.rb + c.k.R - 1) / c.k.R;
    auto tiles_at = [&](uint32_t cols) {
        uint64_t t = 0;
        for (const Cls &c : cl) t += (uint64_t)((c.re - c.rb + c.k.R - 1) / c.k.R) * ((c.ce - c.cb + cols - 1) / cols);
        return t;
    };
    const uint32_t floor_cols = row_groups >= 1792 ? 4096 : 1024;
    pl.cols_per_tile = 65536;
    while (pl.cols_per_tile > floor_cols && tiles_at(pl.cols_per_tile) < 8 * 1792) pl.cols_per_tile /= 2;

    std::vector<TileClass> classes;
    std::map<GroupKey, std::vector<Tile>> grouped;
    hmk_neighbor_stats &S = pl.stats;
    S = hmk_neighbor_stats{};
    S.symmetric = ctx->symmetric;
    for (const Cls &c : cl) {
        const uint32_t cls = add_class(classes, S, c.tc, c.k.rows);
        std::vector<Tile> &dst = grouped[c.k.key];
        for (uint32_t y0 = c.rb; y0 < c.re; y0 += c.k.R)   // (triangle: the columns after the chunk's first row)
            S.pairs_scored += emit_tiles(dst, cls, y0, std::min(c.k.R, c.re - y0), c.tri ? y0 + 1 : c.cb, c.ce, pl.cols_per_tile, true,
                                         c.tri ? 1u : 0u);
    }
    const std::vector<Tile> tiles = order_groups(grouped, classes, X, pl.groups);
    S.n_tiles = (uint32_t)tiles.size();

    int st = upload_plan(ctx, pl, perm, (size_t)pl.lpad, 16, 1, classes, tiles);   // (+ 16: as build_plan)
    if (!st) st = upload_biased_matrix(ctx, pl);
    if (st) return st;
    pl.X = X; pl.p = p; pl.thr = thr;
    pl.q0 = q0; pl.q1 = q1; pl.r0 = r0; pl.r1 = r1;
    pl.valid = true;
    return HMK_OK;
}

int build_plan_search(hmk_ctx *ctx, Plan &pl, int X, int p, int thr, uint32_t q0, uint32_t q1, uint32_t r0, uint32_t r1) {
    return build_plan_rect(ctx, pl, X, p, thr, q0, q1, r0, r1, false);
}

int build_plan_triangle(hmk_ctx *ctx, Plan &pl, int X, int p, int thr, uint32_t q0, uint32_t q1) {
    return build_plan_rect(ctx, pl, X, p, thr, q0, q1, q0, q1, true);
}

// ---- LocalAlignmentScorer passes: tiles of ordered (row length, column length) classes, 16 rows (the local kernels' rows per
// tile) against full column runs; sequences in 32-byte rows ------------------------------------------------------------------
// rows = the buckets bq, columns = br of the sorted order `perm`; `self`: both are the same set, no sequence is paired with itself
// (2: all ordered pairs; 1: every unordered pair once -- the classes la <= lb, column > row where la == lb)
static int finish_plan_local(hmk_ctx *ctx, PlanLocal &pl, const Buckets &bq, const Buckets &br, const std::vector<uint32_t> &perm,
                             uint32_t cols, uint32_t part, uint32_t n_parts, uint32_t self) {
    std::vector<TileClass> classes;
    std::vector<Tile> tiles;
    constexpr uint32_t R = 16;
    uint64_t row_chunk_counter = 0;
    pl.pairs = 0;
    for (int la = 1; la <= HMK_MAX_LEN; la++) {          // rows = seq1 (lines)
        const uint32_t rb = bq[la], re = bq[la + 1];
        if (rb == re) continue;
        for (int lb = self == 1 ? la : 1; lb <= HMK_MAX_LEN; lb++) {      // columns = seq2
            const uint32_t cb = br[lb], ce = br[lb + 1];
            if (cb == ce) continue;
            TileClass tc{};
            tc.la = (uint8_t)la;
            tc.lb = (uint8_t)lb;
            const uint32_t cls = (uint32_t)classes.size();
            classes.push_back(tc);
            for (uint32_t r0 = rb; r0 < re; r0 += R) {
                if ((row_chunk_counter++ % n_parts) != part) continue;
                // (triangle: the columns after the chunk's first row)
                pl.pairs += emit_tiles(tiles, cls, r0, std::min(R, re - r0), self == 1 && la == lb ? r0 + 1 : cb, ce, cols, false, la == lb ? self : 0u);
            }
        }
    }
    pl.n_tiles = (uint32_t)tiles.size();
    pl.part = part; pl.n_parts = n_parts;
    return upload_plan(ctx, pl, perm, 32, 0, 1, classes, tiles);
}

int build_plan_local(hmk_ctx *ctx, PlanLocal &pl, uint32_t part, uint32_t n_parts, bool triangle) {
    if (pl.valid && pl.part == part && pl.n_parts == n_parts && pl.triangle == triangle) return HMK_OK;
    free_plan_local(pl);
    const uint32_t n = ctx->n;
    if (n == 0) return fail(ctx, HMK_ERR_NO_SEQUENCES, "no sequences set (hmk_set_sequences)");
    if (n_parts == 0 || part >= n_parts) return fail(ctx, HMK_ERR_BAD_ARG, "part must be < n_parts");
    Buckets bucket, none;
    std::vector<uint32_t> perm;
    sort_by_length(ctx, 0, n, 0, 0, bucket, none, perm);
    const int st = finish_plan_local(ctx, pl, bucket, bucket, perm, 16384, part, n_parts, triangle ? 1u : 2u);
    if (st) return st;
    pl.triangle = triangle;
    pl.valid = true;
    return HMK_OK;
}

// The rectangle of a LocalAlignmentScorer search: rows = queries (seq1, lines), columns = references (seq2), one class per
// (query length, reference length); the tiles' edges come out m = row = query (row_is_m, k_local.hip).
int build_plan_local_search(hmk_ctx *ctx, PlanLocal &pl, uint32_t q0, uint32_t q1, uint32_t r0, uint32_t r1) {
    if (pl.valid && pl.q0 == q0 && pl.q1 == q1 && pl.r0 == r0 && pl.r1 == r1) return HMK_OK;
    free_plan_local(pl);
    Buckets bq, br;
    std::vector<uint32_t> perm;
    sort_by_length(ctx, q0, q1, r0, r1, bq, br, perm);
    uint64_t row_chunks = 0;
    for (int l = 1; l <= HMK_MAX_LEN; l++) row_chunks += (bq[l + 1] - bq[l] + 15) / 16;
    // column runs of up to 16,384 (build_plan_local), shorter while the rectangle would not fill the GPU once (few queries)
    uint32_t cols = 16384;
    while (cols > 1024 && row_chunks * (((uint64_t)(r1 - r0) + cols - 1) / cols) < 4 * 1792) cols /= 2;
    const int st = finish_plan_local(ctx, pl, bq, br, perm, cols, 0, 1, 0u);
    if (st) return st;
    pl.q0 = q0; pl.q1 = q1; pl.r0 = r0; pl.r1 = r1;
    pl.valid = true;
    return HMK_OK;
}

// what a shifted pass over the ranges [q0, q1) and [r0, r1) checks on its parameters: the all-vs-all pass's checks (build_plan),
// the shift against the two ranges' shortest sequence, as hmk_score_block_shifted does
int check_shifted(hmk_ctx *ctx, int X, int p, int thr, uint32_t q0, uint32_t q1, uint32_t r0, uint32_t r1) {
    if (X < 0) return fail(ctx, HMK_ERR_BAD_ARG, "max_shift must be >= 0");
    int mn = 255;
    for (uint32_t k = q0; k < q1; k++) mn = std::min<int>(mn, ctx->len[k]);
    for (uint32_t k = r0; k < r1; k++) mn = std::min<int>(mn, ctx->len[k]);
    return check_shift_threshold_scores(ctx, X, p, thr, mn);
}

} }  // namespace hmk::impl
