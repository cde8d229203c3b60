// hmk_search.cpp -- query-vs-reference search: queries [q0, q1) against references [r0, r1) of the hmk_set_sequences set, two
// disjoint ranges.  The rectangle's plans (build_plan_search: the shifted tiers; build_plan_local_search: the LocalAlignmentScorer
// tiles), the passes, the query-side orientation and best-k selection on the device (k_search.hip), the extern "C" entry points.
#include "hmk_ctx.h"

namespace hmk { namespace impl {

namespace {

// the caller order of the two ranges, each counting-sorted by length: queries first, then references.  bq / br: bucket starts
// (sorted positions) of each length, [l] .. [l + 1]
void sort_rectangle(const hmk_ctx *ctx, uint32_t q0, uint32_t q1, uint32_t r0, uint32_t r1, uint32_t (&bq)[HMK_MAX_LEN + 2],
                    uint32_t (&br)[HMK_MAX_LEN + 2], std::vector<uint32_t> &perm) {
    const uint32_t nq = q1 - q0;
    std::fill(bq, bq + HMK_MAX_LEN + 2, 0u);
    std::fill(br, br + HMK_MAX_LEN + 2, 0u);
    for (uint32_t k = q0; k < q1; k++) bq[ctx->len[k] + 1]++;
    for (uint32_t k = r0; k < r1; k++) br[ctx->len[k] + 1]++;
    br[0] = nq;
    for (int l = 0; l <= HMK_MAX_LEN; l++) { bq[l + 1] += bq[l]; br[l + 1] += br[l]; }
    perm.resize((size_t)nq + (r1 - r0));
    uint32_t fq[HMK_MAX_LEN + 2], fr[HMK_MAX_LEN + 2];
    std::memcpy(fq, bq, sizeof(fq));
    std::memcpy(fr, br, sizeof(fr));
    for (uint32_t k = q0; k < q1; k++) perm[fq[ctx->len[k]]++] = k;
    for (uint32_t k = r0; k < r1; k++) perm[fr[ctx->len[k]]++] = k;
}

bool is_identity_from(const std::vector<uint32_t> &perm) {
    for (size_t s = 0; s < perm.size(); s++) if (perm[s] != perm[0] + s) return false;
    return true;
}

}  // namespace

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
// No score-bound refinement (hmk_plan.cpp's `refine`): a class whose 8-bit lanes do not fit every pair runs on 16-bit lanes.
// No key sort.
// tri (build_plan_triangle): the TRIANGLE of the pairs inside the one range [q0, q1) = [r0, r1) -- hmk_greedy_continue's new x new --
// under a symmetric matrix: the range is sorted once, the longer bucket supplies the rows, and a class of one length keeps the
// columns after each row (Tile::diag = 1, as build_plan's triangle); edges (min, max) as above.
namespace {
int build_plan_rect(hmk_ctx *ctx, Plan &pl, int X, int p, int thr, uint32_t q0, uint32_t q1, uint32_t r0, uint32_t r1, bool tri);
}  // namespace

int build_plan_search(hmk_ctx *ctx, int X, int p, int thr, uint32_t q0, uint32_t q1, uint32_t r0, uint32_t r1) {
    return build_plan_rect(ctx, ctx->plan_search, X, p, thr, q0, q1, r0, r1, false);
}

int build_plan_search(hmk_ctx *ctx, Plan &pl, int X, int p, int thr, uint32_t q0, uint32_t q1, uint32_t r0, uint32_t r1) {
    return build_plan_rect(ctx, pl, X, p, thr, q0, q1, r0, r1, false);
}

int build_plan_triangle(hmk_ctx *ctx, Plan &pl, int X, int p, int thr, uint32_t q0, uint32_t q1) {
    return build_plan_rect(ctx, pl, X, p, thr, q0, q1, q0, q1, true);
}

namespace {
int build_plan_rect(hmk_ctx *ctx, Plan &pl, int X, int p, int thr, uint32_t q0, uint32_t q1, uint32_t r0, uint32_t r1, bool tri) {
    if (pl.valid && pl.X == X && pl.p == p && pl.thr == thr && pl.q0 == q0 && pl.q1 == q1 && pl.r0 == r0 && pl.r1 == r1 &&
        pl.no_rows_kernel == ctx->sw.no_rows_kernel)
        return HMK_OK;
    free_plan(pl);
    if (tri && !ctx->symmetric) return fail(ctx, HMK_ERR_BAD_ARG, "a triangle plan needs a symmetric matrix");
    const uint32_t nq = q1 - q0, nr = tri ? 0 : r1 - r0, N = nq + nr;
    uint32_t bq[HMK_MAX_LEN + 2], br[HMK_MAX_LEN + 2];
    std::vector<uint32_t> perm;
    sort_rectangle(ctx, q0, q1, r0, tri ? r0 : r1, bq, br, perm);
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

    struct Cls { TileClass tc; bool rows, tri; int lbk; uint32_t R, rb, re, cb, ce; };
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
            const int la = rows_q ? lq : lr, lb = rows_q ? lr : lq;
            c.rb = rows_q ? bq[lq] : br[lr]; c.re = rows_q ? bq[lq + 1] : br[lr + 1];
            c.cb = rows_q ? br[lr] : bq[lq]; c.ce = rows_q ? br[lr + 1] : bq[lq + 1];
            classify(ctx, la, lb, X, p, thr, &c.tc);
            c.rows = use_rows && c.tc.path == PATH_U8 && la >= lb && (pl.rows_exact || rows_kernel_available(X, la, lb, false));
            c.lbk = c.rows ? (pl.rows_exact ? lb : rows_cap_for(lb)) : swar_lbmax_for(lb);
            c.R = c.rows ? (uint32_t)rows_per_tile_rows(X, la - lb, c.lbk, pl.rows_exact)
                         : c.tc.path == PATH_DIRECT ? 16u : (uint32_t)swar_rows_per_tile(c.lbk, c.tc.nw, false);
            cl.push_back(c);
        }
    }
    // Column runs from the rectangle (not from n): the longest run that still leaves ~8 rounds of workgroups (256 CUs x 7), not
    // below 4,096 columns (a tile's dead time, hmk_plan.cpp) -- unless the rows alone make less than one round (a handful of rows
    // against many columns: 5 references x 5 x 10^4 queries under an asymmetric matrix), where shorter runs are the only parallelism.
    uint64_t row_groups = 0;
    for (const Cls &c : cl) row_groups += (c.re - c.rb + c.R - 1) / c.R;
    auto tiles_at = [&](uint32_t cols) {
        uint64_t t = 0;
        for (const Cls &c : cl) t += (uint64_t)((c.re - c.rb + c.R - 1) / c.R) * ((c.ce - c.cb + cols - 1) / cols);
        return t;
    };
    const uint32_t floor_cols = row_groups >= 1792 ? 4096 : 1024;
    pl.cols_per_tile = 65536;
    while (pl.cols_per_tile > floor_cols && tiles_at(pl.cols_per_tile) < 8 * 1792) pl.cols_per_tile /= 2;
    const uint32_t COLS = pl.cols_per_tile;

    std::vector<TileClass> classes;
    std::map<std::tuple<int, int, int>, std::vector<Tile>> grouped;  // (path, nw | length difference, column capacity)
    hmk_neighbor_stats &S = pl.stats;
    S = hmk_neighbor_stats{};
    S.symmetric = ctx->symmetric;
    for (const Cls &c : cl) {
        const TileClass &tc = c.tc;
        const uint32_t cls = (uint32_t)classes.size();
        classes.push_back(tc);
        if (tc.path == PATH_U8) S.classes_u8++;
        else if (tc.path == PATH_U16) S.classes_u16++;
        else S.classes_direct++;
        if (c.rows) S.classes_rows++;
        std::vector<Tile> &dst = grouped[c.rows ? std::make_tuple((int)PATH_ROWS, (int)tc.la - (int)tc.lb, c.lbk)
                                                : std::make_tuple((int)tc.path, tc.path == PATH_DIRECT ? 0 : (int)tc.nw,
                                                                  tc.path == PATH_DIRECT ? 0 : c.lbk)];
        for (uint32_t y0 = c.rb; y0 < c.re; y0 += c.R) {
            const uint32_t c_lo = c.tri ? y0 + 1 : c.cb;   // triangle: the columns after the chunk's first row
            if (c_lo >= c.ce) continue;
            // equal column runs (whole 256-column batches), as in build_plan
            const uint32_t k_runs = (c.ce - c_lo + COLS - 1) / COLS;
            const uint32_t run = std::min(COLS, ((c.ce - c_lo + k_runs - 1) / k_runs + 255u) & ~255u);
            for (uint32_t x0 = c_lo; x0 < c.ce; x0 += run) {
                Tile t{};
                t.row0 = y0; t.nrows = std::min(c.R, c.re - y0);
                t.col0 = x0; t.ncols = std::min(run, c.ce - x0);
                t.cls = cls;
                uint64_t pairs = (uint64_t)t.nrows * t.ncols;
                if (c.tri && x0 < y0 + t.nrows) {   // the tile reaches the diagonal: keep column > row
                    t.diag = 1;
                    pairs = 0;
                    for (uint32_t r = y0; r < y0 + t.nrows; r++) {
                        const uint32_t lo = std::max(x0, r + 1), hi = x0 + t.ncols;
                        if (hi > lo) pairs += hi - lo;
                    }
                    if (pairs == 0) continue;
                }
                S.pairs_scored += pairs;
                dst.push_back(t);
            }
        }
    }
    std::vector<Tile> tiles;
    for (auto &kv : grouped) {
        if (kv.second.empty()) continue;
        std::stable_sort(kv.second.begin(), kv.second.end(), [](const Tile &a, const Tile &b) {   // biggest tiles first
            return (uint64_t)a.nrows * a.ncols > (uint64_t)b.nrows * b.ncols;
        });
        uint64_t work = 0;
        for (const Tile &t : kv.second) {
            const TileClass &tc = classes[t.cls];
            const int lb = std::min((int)tc.la, (int)tc.lb), d = std::abs((int)tc.la - (int)tc.lb);
            work += (uint64_t)t.nrows * t.ncols * (uint64_t)std::max(1, lb * (2 * X + d + 1) - X * (X + 1));
        }
        pl.groups.push_back(Group{std::get<0>(kv.first), std::get<1>(kv.first), std::get<2>(kv.first), (uint32_t)tiles.size(),
                                  (uint32_t)kv.second.size(), 0u, work});
        tiles.insert(tiles.end(), kv.second.begin(), kv.second.end());
    }
    S.n_tiles = (uint32_t)tiles.size();

    std::vector<uint8_t> res_sorted((size_t)N * pl.lpad + 16, 0);   // + 16: the row-packed kernel's tail loads (build_plan)
    for (uint32_t s = 0; s < N; s++)
        std::memcpy(&res_sorted[(size_t)s * pl.lpad], &ctx->res[ctx->off[perm[s]]], ctx->len[perm[s]]);
    const int bias = ctx->min_m < 0 ? -ctx->min_m : 0;
    uint8_t mb[576];
    for (int e = 0; e < 576; e++) {
        const long long v = (long long)ctx->M[e] + bias;
        mb[e] = (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
    }
    HIPCHK(ctx, hipMalloc((void **)&pl.d_res_sorted, res_sorted.size()));
    HIPCHK(ctx, hipMemcpy(pl.d_res_sorted, res_sorted.data(), res_sorted.size(), hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMalloc((void **)&pl.d_perm, (size_t)N * 4));
    HIPCHK(ctx, hipMemcpy(pl.d_perm, perm.data(), (size_t)N * 4, hipMemcpyHostToDevice));
    // (identity: the sorted positions ARE the caller indices -- references right behind the queries, one length)
    pl.perm_identity = perm[0] == 0 && is_identity_from(perm);
    HIPCHK(ctx, hipMalloc((void **)&pl.d_mb, 576));
    HIPCHK(ctx, hipMemcpy(pl.d_mb, mb, 576, hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMalloc((void **)&pl.d_classes, std::max<size_t>(1, classes.size()) * sizeof(TileClass)));
    if (!classes.empty())
        HIPCHK(ctx, hipMemcpy(pl.d_classes, classes.data(), classes.size() * sizeof(TileClass), hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMalloc((void **)&pl.d_tiles, std::max<size_t>(1, tiles.size()) * sizeof(Tile)));
    if (!tiles.empty())
        HIPCHK(ctx, hipMemcpy(pl.d_tiles, tiles.data(), tiles.size() * sizeof(Tile), hipMemcpyHostToDevice));
    pl.X = X; pl.p = p; pl.thr = thr;
    pl.q0 = q0; pl.q1 = q1; pl.r0 = r0; pl.r1 = r1;
    pl.valid = true;
    return HMK_OK;
}
}  // namespace

// The rectangle of a LocalAlignmentScorer search: rows = queries (seq1, lines), columns = references (seq2), one class per
// (query length, reference length); the tiles' edges come out m = row = query (row_is_m, k_local.hip).
int build_plan_local_search(hmk_ctx *ctx, uint32_t q0, uint32_t q1, uint32_t r0, uint32_t r1) {
    return build_plan_local_search(ctx, ctx->plan_local_search, q0, q1, r0, r1);
}

int build_plan_local_search(hmk_ctx *ctx, PlanLocal &pl, uint32_t q0, uint32_t q1, uint32_t r0, uint32_t r1) {
    if (pl.valid && pl.q0 == q0 && pl.q1 == q1 && pl.r0 == r0 && pl.r1 == r1) return HMK_OK;
    free_plan_local(pl);
    const uint32_t N = (q1 - q0) + (r1 - r0);
    uint32_t bq[HMK_MAX_LEN + 2], br[HMK_MAX_LEN + 2];
    std::vector<uint32_t> perm;
    sort_rectangle(ctx, q0, q1, r0, r1, bq, br, perm);
    constexpr uint32_t R = 16;   // rows per tile of the local kernels (build_plan_local)
    uint64_t row_chunks = 0, col_total = 0;
    for (int l = 1; l <= HMK_MAX_LEN; l++) row_chunks += (bq[l + 1] - bq[l] + R - 1) / R;
    col_total = r1 - r0;
    // column runs of up to 16,384 (build_plan_local), shorter while the rectangle would not fill the GPU once (few queries)
    uint32_t COLS = 16384;
    while (COLS > 1024 && row_chunks * ((col_total + COLS - 1) / COLS) < 4 * 1792) COLS /= 2;
    std::vector<TileClass> classes;
    std::vector<Tile> tiles;
    pl.pairs = 0;
    for (int la = 1; la <= HMK_MAX_LEN; la++) {
        const uint32_t rb = bq[la], re = bq[la + 1];
        if (rb == re) continue;
        for (int lb = 1; lb <= HMK_MAX_LEN; lb++) {
            const uint32_t cb = br[lb], ce = br[lb + 1];
            if (cb == ce) continue;
            TileClass tc{};
            tc.la = (uint8_t)la;
            tc.lb = (uint8_t)lb;
            const uint32_t cls = (uint32_t)classes.size();
            classes.push_back(tc);
            for (uint32_t y0 = rb; y0 < re; y0 += R)
                for (uint32_t x0 = cb; x0 < ce; x0 += COLS) {
                    Tile t{};
                    t.row0 = y0; t.nrows = std::min(R, re - y0); t.col0 = x0; t.ncols = std::min(COLS, ce - x0); t.cls = cls;
                    pl.pairs += (uint64_t)t.nrows * t.ncols;
                    tiles.push_back(t);
                }
        }
    }
    pl.n_tiles = (uint32_t)tiles.size();
    std::vector<uint8_t> res_sorted((size_t)N * 32, 0);
    for (uint32_t s = 0; s < N; s++) std::memcpy(&res_sorted[(size_t)s * 32], &ctx->res[ctx->off[perm[s]]], ctx->len[perm[s]]);
    HIPCHK(ctx, hipMalloc((void **)&pl.d_res_sorted, res_sorted.size()));
    HIPCHK(ctx, hipMemcpy(pl.d_res_sorted, res_sorted.data(), res_sorted.size(), hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMalloc((void **)&pl.d_perm, (size_t)N * 4));
    HIPCHK(ctx, hipMemcpy(pl.d_perm, perm.data(), (size_t)N * 4, hipMemcpyHostToDevice));
    pl.perm_identity = perm[0] == 0 && is_identity_from(perm);
    HIPCHK(ctx, hipMalloc((void **)&pl.d_classes, std::max<size_t>(1, classes.size()) * sizeof(TileClass)));
    if (!classes.empty())
        HIPCHK(ctx, hipMemcpy(pl.d_classes, classes.data(), classes.size() * sizeof(TileClass), hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMalloc((void **)&pl.d_tiles, std::max<size_t>(1, tiles.size()) * sizeof(Tile)));
    if (!tiles.empty())
        HIPCHK(ctx, hipMemcpy(pl.d_tiles, tiles.data(), tiles.size() * sizeof(Tile), hipMemcpyHostToDevice));
    pl.part = 0; pl.n_parts = 1;
    pl.q0 = q0; pl.q1 = q1; pl.r0 = r0; pl.r1 = r1;
    pl.valid = true;
    return HMK_OK;
}

// what the shifted search checks on its parameters (the all-vs-all pass's checks, build_plan; the shift against the two ranges'
// shortest sequence, as hmk_score_block_shifted does)
int check_shifted(hmk_ctx *ctx, int X, int p, int thr, uint32_t q0, uint32_t q1, uint32_t r0, uint32_t r1) {
    if (X < 0) return fail(ctx, HMK_ERR_BAD_ARG, "max_shift must be >= 0");
    int mn = 255;
    for (uint32_t k = q0; k < q1; k++) mn = std::min<int>(mn, ctx->len[k]);
    for (uint32_t k = r0; k < r1; k++) mn = std::min<int>(mn, ctx->len[k]);
    if (X >= mn)
        return fail(ctx, HMK_ERR_SHIFT_TOO_BIG, "Shift too big: " + std::to_string(mn - 1) + " is maximum, but " + std::to_string(X) +
                                                    " found");  // ShiftedScorer.java:59-62
    if (thr < -30000 || thr > 30000) return fail(ctx, HMK_ERR_BAD_ARG, "threshold outside [-30000, 30000]");
    const long long top = (long long)ctx->max_len * std::max(0, ctx->max_m) +
                          (long long)std::max(0, p) * ((ctx->max_len - ctx->min_len) + 2LL * X);
    if (top > 32767)
        return fail(ctx, HMK_ERR_BAD_ARG, "scores up to " + std::to_string(top) + " are possible with this matrix / shift penalty: "
                                           "they do not fit the int16 score of a packed edge");
    return HMK_OK;
}

namespace {

enum { SEARCH_SHIFTED = 0, SEARCH_LOCAL = 1 };

// the argument checks every search makes before it looks at the device (a host-only context answers them too)
int check_ranges(hmk_ctx *ctx, uint32_t q0, uint32_t q1, uint32_t r0, uint32_t r1) {
    if (q0 > q1 || r0 > r1 || q1 > ctx->n || r1 > ctx->n)
        return fail(ctx, HMK_ERR_BAD_ARG, "search ranges must lie within [0, n) with q0 <= q1 and r0 <= r1 (n = " + std::to_string(ctx->n) + ")");
    if (q0 < q1 && r0 < r1 && q0 < r1 && r0 < q1) return fail(ctx, HMK_ERR_BAD_ARG, "the query and reference ranges overlap");
    return HMK_OK;
}

// the search pass into the context's edge buffer (grown until every segment fits); counts and the kernels' device time
int search_pass(hmk_ctx *ctx, int scorer, int a, int b, int thr, uint32_t q0, uint32_t q1, uint32_t r0, uint32_t r1, uint64_t want_cap,
                unsigned long long counts[HMK_EDGE_SHARDS], double *ms, hmk_neighbor_stats *stats) {
    int st = scorer == SEARCH_SHIFTED ? build_plan_search(ctx, a, b, thr, q0, q1, r0, r1) : build_plan_local_search(ctx, q0, q1, r0, r1);
    if (st) return st;
    st = neighbors_grow(ctx, want_cap, counts, ms, [&](uint64_t *d_edges, uint64_t cap, unsigned long long *d_counts) {
        return scorer == SEARCH_SHIFTED ? launch_plan(ctx, ctx->plan_search, a, b, thr, d_edges, cap, d_counts, nullptr)
                                        : launch_plan_local(ctx, ctx->plan_local_search, a, b, thr, d_edges, cap, d_counts, nullptr);
    });
    if (st) return st;
    uint64_t total = 0;
    for (int s = 0; s < HMK_EDGE_SHARDS; s++) total += counts[s];
    if (scorer == SEARCH_SHIFTED) {
        *stats = ctx->plan_search.stats;
    } else {
        *stats = hmk_neighbor_stats{};
        stats->pairs_scored = ctx->plan_local_search.pairs;
        stats->n_tiles = ctx->plan_local_search.n_tiles;
    }
    stats->n_edges = total;
    stats->kernel_ms = *ms;
    return HMK_OK;
}

uint64_t max_count(const unsigned long long counts[HMK_EDGE_SHARDS]) {
    return *std::max_element(counts, counts + HMK_EDGE_SHARDS);
}

int search_edges(hmk_ctx *ctx, int scorer, uint32_t q0, uint32_t q1, uint32_t r0, uint32_t r1, int a, int b, int thr, uint64_t *edges,
                 uint64_t capacity, uint64_t *n_edges, hmk_neighbor_stats *stats) {
    if (!ctx) return fail(nullptr, HMK_ERR_BAD_ARG, "null context");
    std::lock_guard<std::mutex> lock(ctx->mu);
    refresh_switches(ctx);
    if (!n_edges) return fail(ctx, HMK_ERR_BAD_ARG, "n_edges must not be null");
    if (capacity && !edges) return fail(ctx, HMK_ERR_BAD_ARG, "null edge buffer");
    int st = check_ranges(ctx, q0, q1, r0, r1);
    if (st) return st;
    *n_edges = 0;
    st = need_device(ctx);
    if (st) return st;
    hmk_neighbor_stats S{};
    S.symmetric = scorer == SEARCH_SHIFTED && ctx->symmetric;
    if (q0 == q1 || r0 == r1) {
        if (stats) *stats = S;
        return HMK_OK;
    }
    st = scorer == SEARCH_SHIFTED ? check_shifted(ctx, a, b, thr, q0, q1, r0, r1) : check_local_fits(ctx, a, b, thr);
    if (st) return st;
    unsigned long long counts[HMK_EDGE_SHARDS];
    double ms = 0;
    st = search_pass(ctx, scorer, a, b, thr, q0, q1, r0, r1, capacity, counts, &ms, &S);
    if (st) return st;
    const uint64_t total = S.n_edges;
    *n_edges = total;
    if (stats) *stats = S;
    if (total > capacity) return fail(ctx, HMK_ERR_CAPACITY, "edge buffer too small: " + std::to_string(total) + " needed");
    if (total == 0) return HMK_OK;
    HIPCHK(ctx, ensure_buf(ctx, SB_SEARCH_OUT, total * sizeof(uint64_t)));
    uint64_t *d_out = buf<uint64_t>(ctx, SB_SEARCH_OUT);
    HIPCHK(ctx, launch_search_compact(ctx->d_edges, ctx->d_edges_cap / HMK_EDGE_SHARDS, ctx->d_counts, max_count(counts), q0, q1 - q0, d_out, total, nullptr));
    HIPCHK(ctx, hipMemcpy(edges, d_out, total * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return HMK_OK;
}

}  // namespace

} }  // namespace hmk::impl

extern "C" {

int hmk_search_shifted(hmk_ctx *ctx, uint32_t q0, uint32_t q1, uint32_t r0, uint32_t r1, int max_shift, int shift_penalty, int threshold,
                       uint64_t *edges, uint64_t capacity, uint64_t *n_edges, hmk_neighbor_stats *stats) {
    return search_edges(ctx, SEARCH_SHIFTED, q0, q1, r0, r1, max_shift, shift_penalty, threshold, edges, capacity, n_edges, stats);
}

int hmk_search_local(hmk_ctx *ctx, uint32_t q0, uint32_t q1, uint32_t r0, uint32_t r1, int gap_open, int gap_extend, int threshold,
                     uint64_t *edges, uint64_t capacity, uint64_t *n_edges, hmk_neighbor_stats *stats) {
    return search_edges(ctx, SEARCH_LOCAL, q0, q1, r0, r1, gap_open, gap_extend, threshold, edges, capacity, n_edges, stats);
}

int hmk_search_best_shifted(hmk_ctx *ctx, uint32_t q0, uint32_t q1, uint32_t r0, uint32_t r1, int max_shift, int shift_penalty,
                            int threshold, uint32_t k, uint32_t *hit_index, int32_t *hit_score, uint32_t *n_hits,
                            hmk_neighbor_stats *stats) {
    if (!ctx) return fail(nullptr, HMK_ERR_BAD_ARG, "null context");
    std::lock_guard<std::mutex> lock(ctx->mu);
    refresh_switches(ctx);
    if (k < 1 || k > 32) return fail(ctx, HMK_ERR_BAD_ARG, "k must be 1..32");
    int st = check_ranges(ctx, q0, q1, r0, r1);
    if (st) return st;
    const uint32_t nq = q1 - q0;
    if (nq && (!hit_index || !hit_score || !n_hits)) return fail(ctx, HMK_ERR_BAD_ARG, "null output buffer");
    st = need_device(ctx);
    if (st) return st;
    hmk_neighbor_stats S{};
    S.symmetric = ctx->symmetric;
    if (nq == 0 || r0 == r1) {
        for (uint64_t t = 0; t < (uint64_t)nq * k; t++) { hit_index[t] = 0xFFFFFFFFu; hit_score[t] = INT32_MIN; }
        for (uint32_t q = 0; q < nq; q++) n_hits[q] = 0;
        if (stats) *stats = S;
        return HMK_OK;
    }
    st = check_shifted(ctx, max_shift, shift_penalty, threshold, q0, q1, r0, r1);
    if (st) return st;
    unsigned long long counts[HMK_EDGE_SHARDS];
    double ms = 0;
    st = search_pass(ctx, SEARCH_SHIFTED, max_shift, shift_penalty, threshold, q0, q1, r0, r1, 0, counts, &ms, &S);
    if (st) return st;
    const uint64_t total = S.n_edges;
    if (total > 0xFFFFFFFFull) return fail(ctx, HMK_ERR_OOM, "more than 2^32 - 1 hits above the threshold: raise the threshold");
    const uint64_t nk = (uint64_t)nq * k;
    HIPCHK(ctx, ensure_buf(ctx, SB_SEARCH_CNT, (size_t)2 * nq * 4));
    HIPCHK(ctx, ensure_buf(ctx, SB_SEARCH_START, ((size_t)nq + 1) * 4));
    HIPCHK(ctx, ensure_buf(ctx, SB_SEARCH_SCAN, scan_scratch_bytes(nq)));
    HIPCHK(ctx, ensure_buf(ctx, SB_SEARCH_OUT, std::max<uint64_t>(total, 1) * sizeof(uint64_t)));
    HIPCHK(ctx, ensure_buf(ctx, SB_SEARCH_HITS, nk * 8 + (size_t)nq * 4));
    uint32_t *d_index = buf<uint32_t>(ctx, SB_SEARCH_HITS);
    int32_t *d_score = (int32_t *)(d_index + nk);
    uint32_t *d_nhits = d_index + 2 * nk;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    HIPCHK(ctx, hipEventCreate(&e0));
    hipError_t e = hipEventCreate(&e1);
    if (e == hipSuccess) e = hipEventRecord(e0, nullptr);
    if (e == hipSuccess)
        e = launch_search_best(ctx->d_edges, ctx->d_edges_cap / HMK_EDGE_SHARDS, ctx->d_counts, max_count(counts), q0, nq, k, buf<uint32_t>(ctx, SB_SEARCH_CNT),
                               buf<uint32_t>(ctx, SB_SEARCH_START), buf<uint64_t>(ctx, SB_SEARCH_SCAN), buf<uint64_t>(ctx, SB_SEARCH_OUT),
                               std::max<uint64_t>(total, 1), d_index, d_score, d_nhits, nullptr);
    if (e == hipSuccess) e = hipEventRecord(e1, nullptr);
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    float sel_ms = 0;
    if (e == hipSuccess) e = hipEventElapsedTime(&sel_ms, e0, e1);
    (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (e != hipSuccess) return fail(ctx, e == hipErrorOutOfMemory ? HMK_ERR_OOM : HMK_ERR_DEVICE, std::string("best-k selection: ") + hipGetErrorString(e));
    HIPCHK(ctx, hipMemcpy(hit_index, d_index, nk * 4, hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(hit_score, d_score, nk * 4, hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(n_hits, d_nhits, (size_t)nq * 4, hipMemcpyDeviceToHost));
    S.kernel_ms = ms + sel_ms;
    if (stats) *stats = S;
    return HMK_OK;
}

}  // extern "C"
