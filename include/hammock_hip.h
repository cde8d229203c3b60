/*
 * hammock_hip.h -- C ABI of libhammock_hip.so, the MI355X (gfx950) drop-in for
 * the greedy initial-clustering hot path of krejciadam/hammock v1.2.0.
 *
 * The reference has no FFI seam of its own; its seams are the Java interfaces
 * below (paths relative to src/cz/krejciadam/hammock/).  Each entry point names
 * the reference interface it replaces.  A JNI / cgo / ctypes binding binds
 * exactly these symbols (INTEGRATION.md shows the Java side).
 *
 * Conventions
 *   - plain C types only; every output buffer is caller-allocated
 *   - residues are indices 0..23 over "ARNDCQEGHILKMFPSTWYVBZX*"
 *     (UniqueSequence.java:23-26); the scoring matrix is int[24][24] row-major
 *     exactly as FileIOManager.loadScoringMatrix returns it (FileIOManager.java:46-81)
 *   - score(i, j) always means SequenceScorer.sequenceScore(seq1 = sequence i,
 *     seq2 = sequence j) (SequenceScorer.java:14)
 *   - every function returns an hmk_status; hmk_last_error() gives the text
 *   - there is no CPU fallback: a scoring call on a context without a usable
 *     GPU returns HMK_ERR_DEVICE
 */
#ifndef HAMMOCK_HIP_H
#define HAMMOCK_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HMK_ABI_VERSION 4
#define HMK_ALPHABET 24
#define HMK_MAX_LEN 32          /* longest sequence the GPU kernels accept */
#define HMK_MAX_SEQUENCES (1u << 24)
#define HMK_EDGE_SHARDS 64      /* output segments of the neighbour kernel (ABI 3: 64, was 16 -- a segment's cursor is ONE address, and a
                                 * pass whose waves drain 4 x 10^5 stages serialises on 16 of them) */

typedef enum {
    HMK_OK = 0,
    HMK_ERR_BAD_ARG = 1,
    HMK_ERR_SHIFT_TOO_BIG = 2,          /* DataException, ShiftedScorer.java:59-62 */
    HMK_ERR_DEVICE = 3,                 /* HIP error / no usable gfx950 device */
    HMK_ERR_OOM = 4,
    HMK_ERR_REFERENCE_WOULD_CRASH = 5,  /* NullPointerException in
                                           LimitedGreedySequenceClusterer.java:97/104/108
                                           (surfaces at Hammock.java:153-157) */
    HMK_ERR_CAPACITY = 6,               /* caller's edge buffer too small; *n_edges = needed */
    HMK_ERR_NO_SEQUENCES = 7
} hmk_status;

typedef struct hmk_ctx hmk_ctx;

/* Edge of the thresholded neighbour graph, packed in one uint64:
 *   bits 63..40  x      (sequence index, 24 bit)
 *   bits 39..16  m      (sequence index, 24 bit)
 *   bits 15..0   score  (int16, two's complement)
 * meaning  sequenceScore(seq1 = m, seq2 = x) = score >= threshold.
 * With a symmetric matrix each unordered pair appears once with x < m. */
#define HMK_EDGE_X(e) ((uint32_t)((e) >> 40))
#define HMK_EDGE_M(e) ((uint32_t)(((e) >> 16) & 0xFFFFFFu))
#define HMK_EDGE_SCORE(e) ((int32_t)(int16_t)((e) & 0xFFFFu))

/* ---- context ---------------------------------------------------------- */

/* Replaces `new ShiftedScorer(scoringMatrix, ..)` / `new LocalAlignmentScorer`
 * construction state (ShiftedScorer.java:28-32, LocalAlignmentScorer.java:20-24):
 * holds the matrix (Hammock.scoringMatrix, Hammock.java:46,1264) on `device`.
 * device >= 0: HIP device ordinal.  device == -1: host-only context (only the
 * host-side calls hmk_greedy_from_edges / hmk_set_sequences work).
 * The context comes warm: its streams, events, pinned blocks, the DMA paths of
 * both directions and the kernels' code objects are set up here (25-35 ms after
 * HIP itself has started), not inside the first clustering call -- the reference
 * constructs its scorer before it starts the clock of "Clustering time"
 * (Hammock.java:402-406), and a host may create the context on another thread
 * while it reads its input (hammock_cli.cpp does).  HMK_LAZY_CONTEXT=1 defers. */
int hmk_create(const int32_t matrix[HMK_ALPHABET * HMK_ALPHABET], int device, hmk_ctx **ctx);
/* The same on several GPUs of one node (BASELINE config 5: "pair-space sharded 8 x MI355X over xGMI"): devices[0] is the
 * root.  hmk_set_sequences uploads to every device; hmk_greedy_cluster scores shard d of n_devices on device d (row
 * blocks dealt cyclically, no collective inside the scoring), gathers the peers' edge segments to the root with direct
 * xGMI peer copies (every peer over its own link; a gather to the one device whose host runs the merge moves 1/n of an
 * all-gather's bytes) and runs the merge tail there.  The result is identical to the single-device call.  Every other
 * entry point works on the root device.  n_devices = 1 is hmk_create.  (One PROCESS per GPU with an RCCL all-gather
 * -- hammock_amd/dist.py -- is the other multi-GPU form; both end in hmk_greedy_from_edges_dev on rank/device 0.) */
int hmk_create_multi(const int32_t matrix[HMK_ALPHABET * HMK_ALPHABET], const int *devices, int n_devices, hmk_ctx **ctx);
int hmk_device_count(const hmk_ctx *ctx); /* devices behind this context (0 for a host-only context) */
void hmk_destroy(hmk_ctx *ctx);
const char *hmk_last_error(const hmk_ctx *ctx); /* ctx may be NULL */
int hmk_abi_version(void);
/* Device time (HIP events, milliseconds) of the scoring kernel(s) the last hmk_score_pairs_* /
 * hmk_score_block_* / hmk_score_with_shift call launched; excludes the host<->device copies. */
double hmk_last_kernel_ms(const hmk_ctx *ctx);

/* The List<UniqueSequence> handed to SequenceClusterer.cluster
 * (SequenceClusterer.java:24), flattened in the caller's (greedy) order:
 * residues concatenated, offsets[n+1], sizes[n] = UniqueSequence.size()
 * (UniqueSequence.java:82-88; NULL = all 1).  Copies everything. */
int hmk_set_sequences(hmk_ctx *ctx, const uint8_t *residues, const uint32_t *offsets,
                      const int32_t *sizes, uint32_t n);

/* ---- pairwise scorers (parity probes of SequenceScorer.sequenceScore) ---- */

/* out[k] = ShiftedScorer(matrix, shift_penalty, max_shift).sequenceScore(i[k], j[k])
 * (ShiftedScorer.java:48-100).  HMK_ERR_SHIFT_TOO_BIG if max_shift >= the
 * shorter length of any pair. */
int hmk_score_pairs_shifted(hmk_ctx *ctx, const uint32_t *i, const uint32_t *j, uint64_t n_pairs,
                            int max_shift, int shift_penalty, int32_t *out);
/* AligningSequenceScorer.scoreWithShift (AligningSequenceScorer.java:11, ShiftedScorer.java:48-95):
 * score[k] and shift[k] = AligningScorerResult.getScore() / getShift() for the pair (i[k], j[k]);
 * the first strict maximum wins (:86-89), the sign follows :91-93. */
int hmk_score_with_shift(hmk_ctx *ctx, const uint32_t *i, const uint32_t *j, uint64_t n_pairs,
                         int max_shift, int shift_penalty, int32_t *score, int32_t *shift);
/* out[k] = LocalAlignmentScorer(matrix, gap_open, gap_extend).sequenceScore(i[k], j[k])
 * (LocalAlignmentScorer.java:27-86); i = seq1 = lines, j = seq2 = columns. */
int hmk_score_pairs_local(hmk_ctx *ctx, const uint32_t *i, const uint32_t *j, uint64_t n_pairs,
                          int gap_open, int gap_extend, int32_t *out);
/* GlobalAlignmentScorer: the optimal score of a global alignment of two whole sequences under the matrix with an affine gap
 * (Gotoh); the reference has no counterpart.  With n = |seq1|, m = |seq2|:
 *     H[0][0] = 0
 *     H[0][j] = E[0][j] = gap_open + (j - 1) gap_extend      H[i][0] = F[i][0] = gap_open + (i - 1) gap_extend
 *     E[i][0] = F[0][j] = -infinity
 *     E[i][j] = max(E[i][j-1] + gap_extend, H[i][j-1] + gap_open)
 *     F[i][j] = max(F[i-1][j] + gap_extend, H[i-1][j] + gap_open)
 *     H[i][j] = max(H[i-1][j-1] + M[seq1[i-1]][seq2[j-1]], E[i][j], F[i][j])          score = H[n][m]
 * Penalties are ADDED (LocalAlignmentScorer's convention): a gap of length k costs gap_open + (k - 1) gap_extend, end gaps
 * like inner ones.  Arguments: -127 <= gap_open <= gap_extend <= 0 (under it the recurrence is the maximum over all
 * alignments; gap_open > gap_extend is not defined) and 32 * max(0, largest matrix entry) <= 32767, else HMK_ERR_BAD_ARG --
 * answered before the device is looked at (a host-only context answers them too), as are the thresholds' [-30000, 30000]
 * in the two edge calls below.  The lowest score, the all-gap alignment, is >= -8,128.  A symmetric matrix gives a symmetric
 * score; a 0 / -1 matrix with penalties -1 / -1 gives minus the Levenshtein distance.
 * Out of scope: assign, match and best-k forms with this scorer; multi-device sharding beyond part / n_parts.
 * out[k] = global(seq1 = i[k], seq2 = j[k]). */
int hmk_score_pairs_global(hmk_ctx *ctx, const uint32_t *i, const uint32_t *j, uint64_t n_pairs,
                           int gap_open, int gap_extend, int32_t *out);
/* The alignment behind that score (traceback): H, E, F are exactly the tables above, seq1 = i[k] (n residues), seq2 = j[k] (m).
 * ONE deterministic walk from (n, m) in state H to (0, 0) emits the alignment's columns right to left:
 *     i = 0            every remaining residue of seq2 is a column with a gap in seq1
 *     j = 0            every remaining residue of seq1 is a column with a gap in seq2
 *     H at (i, j)      the first that holds:  H[i][j] == H[i-1][j-1] + M[seq1[i-1]][seq2[j-1]] -> a pair column, H at (i-1, j-1);
 *                      H[i][j] == E[i][j] -> state E at (i, j);  otherwise state F at (i, j)
 *     E at (i, j)      a column seq2[j-1] against a gap in seq1; E at (i, j-1) if E[i][j] == E[i][j-1] + gap_extend (an optimal
 *                      extension is preferred over an opening), otherwise H at (i, j-1)
 *     F at (i, j)      the mirror: seq1[i-1] against a gap in seq2; F at (i-1, j) if F[i][j] == F[i-1][j] + gap_extend, else H at (i-1, j)
 * The emitted alignment, rescored column by column, scores H[n][m].  Per pair:
 *     score[k]  = H[n][m] (= hmk_score_pairs_global)         n_cols[k] = the alignment's width, max(n, m) <= n_cols <= n + m <= 64
 *     gap1[k]   bit c set: column c has a gap in seq1        gap2[k]   bit c set: column c has a gap in seq2
 * with column 0 the LEFTMOST: gap1 & gap2 == 0, popcount(gap1) = n_cols - n, popcount(gap2) = n_cols - m, bits at and above n_cols
 * are zero.  Arguments, checks and their order as hmk_score_pairs_global (i[k] == j[k] is allowed; n_pairs = 0 writes nothing);
 * hmk_last_kernel_ms covers the kernel.  One kernel for every matrix a context admits (int32 throughout). */
int hmk_align_pairs_global(hmk_ctx *ctx, const uint32_t *i, const uint32_t *j, uint64_t n_pairs,
                           int gap_open, int gap_extend, int32_t *score, uint8_t *n_cols, uint64_t *gap1, uint64_t *gap2);
/* Dense block: out[(r - r0) * (c1 - c0) + (c - c0)] = score(r, c), r0<=r<r1, c0<=c<c1. */
int hmk_score_block_shifted(hmk_ctx *ctx, uint32_t r0, uint32_t r1, uint32_t c0, uint32_t c1,
                            int max_shift, int shift_penalty, int32_t *out);
int hmk_score_block_local(hmk_ctx *ctx, uint32_t r0, uint32_t r1, uint32_t c0, uint32_t c1,
                          int gap_open, int gap_extend, int32_t *out);
/* ... = global(seq1 = r, seq2 = c) (hmk_score_pairs_global) */
int hmk_score_block_global(hmk_ctx *ctx, uint32_t r0, uint32_t r1, uint32_t c0, uint32_t c1,
                           int gap_open, int gap_extend, int32_t *out);

/* ---- all-vs-all thresholded neighbour graph (the hot kernel) ------------ */

typedef struct {
    uint64_t n_edges;        /* edges produced by this call */
    uint64_t pairs_scored;   /* pairs the kernels evaluated (unordered unless asymmetric) */
    uint32_t n_tiles;        /* workgroups launched */
    uint32_t symmetric;      /* 1: matrix symmetric, triangle only */
    uint32_t classes_u8;     /* (row length, column length) classes on the 8-bit lane path */
    uint32_t classes_u16;    /* ... on the 16-bit lane path */
    uint32_t classes_direct; /* ... on the generic one-cell-at-a-time path */
    uint32_t classes_rows;   /* of the 8-bit lane classes: how many run the row-packed kernels (8 rows per table entry) */
    double kernel_ms;        /* device time of the scoring kernels (HIP events) */
} hmk_neighbor_stats;

/* Scores every pair with ShiftedScorer semantics and returns the pairs with
 * score >= threshold as packed edges (see HMK_EDGE_*).  This is the batch
 * form of what ClinkageClusterScorer.clusterScore's early exit
 * (ClinkageClusterScorer.java:36-48) asks of the scorer pair by pair.
 * The pair space is split row-block-wise into n_parts shards; this call
 * computes shard `part` (single GPU: part = 0, n_parts = 1).
 * edges: host buffer of `capacity` entries; *n_edges receives the count
 * (HMK_ERR_CAPACITY and the needed count if it does not fit). */
int hmk_neighbors_shifted(hmk_ctx *ctx, int max_shift, int shift_penalty, int threshold,
                          uint32_t part, uint32_t n_parts, uint64_t *edges, uint64_t capacity,
                          uint64_t *n_edges, hmk_neighbor_stats *stats);

/* The same for LocalAlignmentScorer(matrix, gap_open, gap_extend) (LocalAlignmentScorer.java:27-86): ALL
 * ORDERED pairs (the scorer depends on the argument order) with sequenceScore(seq1 = m, seq2 = x) >= threshold,
 * as edges (x, m, score).  This is the batch form of the stage-2 pre-filter `sequenceScore(first, i) >= 12`
 * (ClustalRunner.java:81-96, Hammock.java:118-121,645-649).  Gap penalties <= 0 and |matrix| <= 127 run the striped
 * register kernels; anything else (the reference restricts neither) runs the literal DP on the same tiles. */
int hmk_neighbors_local(hmk_ctx *ctx, int gap_open, int gap_extend, int threshold, uint32_t part,
                        uint32_t n_parts, uint64_t *edges, uint64_t capacity, uint64_t *n_edges,
                        hmk_neighbor_stats *stats);

/* The same for GlobalAlignmentScorer (hmk_score_pairs_global), edges with the contract of hmk_neighbors_shifted: under a
 * symmetric matrix each unordered pair with global >= threshold once, x < m, and only those pairs are scored
 * (stats->pairs_scored = n (n - 1) / 2 over all parts, stats->symmetric = 1); otherwise ALL ORDERED pairs, score =
 * global(seq1 = m, seq2 = x).  Register-resident DP for matrices within +-127, the literal DP on the same tiles otherwise.
 * Parts are dealt by row chunk as in hmk_neighbors_local.  stats: n_edges, pairs_scored, n_tiles, symmetric, kernel_ms. */
int hmk_neighbors_global(hmk_ctx *ctx, int gap_open, int gap_extend, int threshold, uint32_t part,
                         uint32_t n_parts, uint64_t *edges, uint64_t capacity, uint64_t *n_edges,
                         hmk_neighbor_stats *stats);

/* Device-resident form: asynchronous on `stream` (a hipStream_t, may be NULL),
 * no host synchronisation.  d_edges: device buffer of `capacity` uint64,
 * logically HMK_EDGE_SHARDS segments of capacity / HMK_EDGE_SHARDS entries;
 * d_counts: device uint64[HMK_EDGE_SHARDS], zeroed by the call, receives the
 * number of edges each segment WANTED to hold (may exceed the segment size:
 * overflow, entries beyond the segment are dropped). */
int hmk_neighbors_shifted_dev(hmk_ctx *ctx, int max_shift, int shift_penalty, int threshold,
                              uint32_t part, uint32_t n_parts, void *d_edges, uint64_t capacity,
                              void *d_counts, void *stream);
/* Device to device, asynchronous on `stream`: packs the HMK_EDGE_SHARDS segments of a
 * hmk_neighbors_shifted_dev result into one contiguous block d_out[0 .. *d_total) (at most
 * out_capacity entries are written) -- the block a fixed-size all-gather ships to the other ranks. */
int hmk_compact_edges_dev(hmk_ctx *ctx, const void *d_edges, uint64_t capacity, const void *d_counts,
                          void *d_out, uint64_t out_capacity, void *d_total, void *stream);
/* "Row blocks": the 4-byte-per-edge form of a rank's edges that the multi-GPU exchange ships (half the
 * xGMI bytes of the packed edges).  Device to device, asynchronous on `stream`; calls on one context must be
 * stream-ordered (they share context-owned scratch).  Regroups the HMK_EDGE_SHARDS segments by x:
 *   d_row_start  uint32[n + 2]: entries of row x are d_adj[d_row_start[x] .. d_row_start[x + 1]);
 *                [n] = number of edges, [n + 1] = edges whose score - threshold did not fit 0..255
 *                (must be 0 for the block to be usable; fall back to hmk_compact_edges_dev otherwise)
 *   d_adj        uint32[adj_capacity]: m << 8 | (score - threshold); order inside a row is arbitrary.
 * n = the sequences of hmk_set_sequences.  Part of the replacement for the per-candidate
 * scoring loop's hand-over (NearestCluster results, LimitedGreedySequenceClusterer.java:118-180). */
int hmk_pack_rows_dev(hmk_ctx *ctx, const void *d_edges, uint64_t capacity, const void *d_counts, int threshold,
                      void *d_row_start, void *d_adj, uint64_t adj_capacity, void *stream);
/* Inverse: writes the row block's edges as packed 8-byte edges to d_edges_out[0 .. d_row_start[n]). */
int hmk_unpack_rows_dev(hmk_ctx *ctx, const void *d_row_start, const void *d_adj, int threshold, void *d_edges_out,
                        uint64_t out_capacity, void *stream);
/* pairs / tiles of the plan the last hmk_neighbors_shifted[_dev] call used */
int hmk_neighbors_last_plan(hmk_ctx *ctx, hmk_neighbor_stats *stats);
/* ... of that plan: its 16-row tiles (0: the plan is not paired) and those of them whose second row group takes the merged cells of
 * the two key positions from the first (both groups row-shared with the same two key residues; HMK_NO_ROW_RUN_SHARE=1: none) */
int hmk_neighbors_last_plan_shared(hmk_ctx *ctx, uint32_t *paired_tiles, uint32_t *run_shared_tiles);
/* ... of that plan: the tiles that copy their row groups' tables from the plan instead of building them (a key-sorted plan: all of
 * its tiles; any other plan, or HMK_NO_TILE_TABLES=1: 0) and the bytes of device memory those tables take (0 with no such tile) */
int hmk_neighbors_last_plan_tables(hmk_ctx *ctx, uint32_t *table_tiles, uint64_t *table_bytes);

/* ---- query-vs-reference search ---------------------------------------------- */

/* Queries [q0, q1) against references [r0, r1) of the hmk_set_sequences set: the pairs (q, r) with
 * score(q, r) >= threshold, where score(q, r) = ShiftedScorer(matrix, shift_penalty, max_shift).sequenceScore(seq1 = q,
 * seq2 = r) (ShiftedScorer.java:48-100) -- the argument order ClinkageClusterScorer.clusterScore uses when a new sequence's
 * cluster is scored against an existing one (ClinkageClusterScorer.java:36-38).  Upload queries and references together
 * once (hmk_set_sequences), then search the two ranges; only the Q x R pairs are scored.
 *   ranges     disjoint, within [0, n); HMK_ERR_BAD_ARG otherwise (checked before the device is: a host-only context
 *              answers it).  An empty range: HMK_OK, 0 edges.
 *   edges      packed as HMK_EDGE_*, ALWAYS m = query and x = reference, whatever the matrix's symmetry (unlike the
 *              (min, max) edges of hmk_neighbors_shifted); order unspecified.  HMK_ERR_CAPACITY and *n_edges = the
 *              number needed if `capacity` is too small.
 *   checks     HMK_ERR_SHIFT_TOO_BIG when max_shift >= the shortest length within the two ranges (the check of
 *              hmk_score_block_shifted; ShiftedScorer.java:59-62); the int16 score fit and threshold limits of
 *              hmk_neighbors_shifted.
 *   stats      pairs_scored = (q1 - q0)(r1 - r0), the class counters, n_tiles, kernel_ms.
 * On a hmk_create_multi context the search runs on the root device. */
int hmk_search_shifted(hmk_ctx *ctx, uint32_t q0, uint32_t q1, uint32_t r0, uint32_t r1,
                       int max_shift, int shift_penalty, int threshold,
                       uint64_t *edges, uint64_t capacity, uint64_t *n_edges, hmk_neighbor_stats *stats);
/* The same for LocalAlignmentScorer(matrix, gap_open, gap_extend).sequenceScore(seq1 = q = lines, seq2 = r = columns)
 * (LocalAlignmentScorer.java:27-86): the striped kernels under hmk_neighbors_local's preconditions, the literal DP
 * otherwise.  stats: n_edges, pairs_scored, n_tiles, kernel_ms. */
int hmk_search_local(hmk_ctx *ctx, uint32_t q0, uint32_t q1, uint32_t r0, uint32_t r1,
                     int gap_open, int gap_extend, int threshold,
                     uint64_t *edges, uint64_t capacity, uint64_t *n_edges, hmk_neighbor_stats *stats);
/* The same for global(seq1 = q, seq2 = r) (hmk_score_pairs_global): ranges and checks as hmk_search_local, the argument
 * checks of hmk_neighbors_global; ALWAYS m = query and x = reference. */
int hmk_search_global(hmk_ctx *ctx, uint32_t q0, uint32_t q1, uint32_t r0, uint32_t r1,
                      int gap_open, int gap_extend, int threshold,
                      uint64_t *edges, uint64_t capacity, uint64_t *n_edges, hmk_neighbor_stats *stats);
/* The best k (1 <= k <= 32) references of every query among those with score(q, r) >= threshold (scores as in
 * hmk_search_shifted), by score descending, then reference index ascending, selected on the device (the edge list never
 * travels to the host): hit_index[(q - q0) * k + t], hit_score[(q - q0) * k + t], n_hits[q - q0] = how many are valid;
 * unused slots hold UINT32_MAX / INT32_MIN.  Never HMK_ERR_CAPACITY (the call grows its own scratch).  stats->kernel_ms
 * includes the selection; stats->n_edges = all hits above the threshold. */
int hmk_search_best_shifted(hmk_ctx *ctx, uint32_t q0, uint32_t q1, uint32_t r0, uint32_t r1,
                            int max_shift, int shift_penalty, int threshold, uint32_t k,
                            uint32_t *hit_index, int32_t *hit_score, uint32_t *n_hits,
                            hmk_neighbor_stats *stats);

/* ---- assignment of new sequences to existing clusters ----------------------------- */

/* Which existing cluster does each new sequence join?  The decision of NearestClusterRunner /
 * findNearestClusterParallel (ClinkageSequenceClusterer.java:137-177, 243-294) with ClinkageClusterScorer
 * (ClinkageClusterScorer.java:30-49), accepted when getScore() >= threshold (LimitedGreedySequenceClusterer.java:59-66),
 * for every new sequence at once.  One uploaded set (hmk_set_sequences) holds both sides:
 *   members    [r0, r1): member r belongs to cluster slot member_cluster[r - r0] in [0, n_clusters); slot c carries the
 *              Java id cluster_id[c] (distinct).  Cluster.size() of slot c is the sum of its members' `sizes` as
 *              uploaded (Cluster.java:156-158; 1 each when sizes was NULL) -- the library sums them.
 *   new        [q0, q1), disjoint from the members.
 * score(m, x) = ShiftedScorer(matrix, shift_penalty, max_shift).sequenceScore(seq1 = member m, seq2 = new x): the call
 * ClinkageSequenceClusterer.java:263 makes (scorer.clusterScore(existing cluster, new sequence's cluster)) -- the
 * OPPOSITE orientation of hmk_search_* (seq1 = query).  Cluster c is feasible for x iff every member m of c has
 * score(m, x) >= threshold; its complete-linkage score is then min over m of score(m, x) (ClinkageClusterScorer's value;
 * its early exit only matters for infeasible clusters).  Feasible clusters rank by score descending, then size()
 * descending, then cluster_id ascending; rank 1 is the cluster findNearestClusterParallel returns.
 * The clusters are frozen: every new sequence is classified on its own, a new sequence never sees another new one, and
 * two new sequences given the same cluster are not checked against each other (classification, not clustering).
 *   outputs    best_cluster[(x - q0) * k + t] = the slot of rank t + 1, best_score[...] its complete-linkage score;
 *              unused slots UINT32_MAX / INT32_MIN.  n_feasible[x - q0] = ALL feasible clusters (not capped at k); 0 =
 *              unassigned.  Selected on the device (the edge list never travels to the host).
 *   checks     HMK_ERR_BAD_ARG (before the device is looked at: a host-only context answers them): ranges overlapping or
 *              outside [0, n); k outside 1..32; a member_cluster value >= n_clusters; a slot without a member; two equal
 *              cluster_ids.  Then the checks of hmk_search_shifted (the shift against both ranges, the threshold and
 *              int16 limits).  Never HMK_ERR_CAPACITY (the call grows its own scratch).
 *   stats      as hmk_search_shifted's; kernel_ms includes the aggregation and selection.
 * On a hmk_create_multi context the assignment runs on the root device. */
int hmk_assign_shifted(hmk_ctx *ctx, uint32_t q0, uint32_t q1, uint32_t r0, uint32_t r1,
                       const uint32_t *member_cluster, const int32_t *cluster_id, uint32_t n_clusters,
                       int max_shift, int shift_penalty, int threshold, uint32_t k,
                       uint32_t *best_cluster, int32_t *best_score, uint32_t *n_feasible,
                       hmk_neighbor_stats *stats);
/* The same with LocalAlignmentScorer(matrix, gap_open, gap_extend).sequenceScore(seq1 = member = lines, seq2 = new =
 * columns) (LocalAlignmentScorer.java:27-86), under the preconditions of hmk_search_local. */
int hmk_assign_local(hmk_ctx *ctx, uint32_t q0, uint32_t q1, uint32_t r0, uint32_t r1,
                     const uint32_t *member_cluster, const int32_t *cluster_id, uint32_t n_clusters,
                     int gap_open, int gap_extend, int threshold, uint32_t k,
                     uint32_t *best_cluster, int32_t *best_score, uint32_t *n_feasible,
                     hmk_neighbor_stats *stats);

/* ---- match of query clusters to existing clusters -------------------------------- */

/* Which existing cluster does each query cluster match?  ClinkageClusterScorer.clusterScore(existing cluster, query cluster)
 * (ClinkageClusterScorer.java:30-49) ranked as findNearestClusterParallel ranks it (ClinkageSequenceClusterer.java:137-177,
 * 258-293), for every query cluster at once -- hmk_assign_shifted is the case of one member per query cluster.  One uploaded
 * set (hmk_set_sequences) holds both sides:
 *   queries    [q0, q1): sequence x belongs to query slot query_cluster[x - q0] in [0, n_query_clusters); every slot has a
 *              member.
 *   members    [r0, r1), disjoint from the queries, with member_cluster, cluster_id and n_clusters as hmk_assign_shifted's
 *              (Cluster.size() = the sum of the members' uploaded sizes).
 * score(m, x) = sequenceScore(seq1 = member m, seq2 = query x), the orientation of ClinkageSequenceClusterer.java:263.
 * Existing cluster a is feasible for query cluster b iff every pair (m in a, x in b) has score(m, x) >= threshold; its
 * complete-linkage score is then the minimum over those pairs.  Feasible clusters rank by score descending, then size()
 * descending, then cluster_id ascending; rank 1 is the cluster findNearestClusterParallel(existing clusters, b) returns.
 * A match means the union of the two clusters is still a complete-linkage cluster.  Classification, not merging: two query
 * clusters matched to the same existing cluster are not checked against each other.
 *   outputs    best_cluster[b * k + t] = the slot of rank t + 1, best_score[b * k + t] its score; unused entries
 *              UINT32_MAX / INT32_MIN.  n_feasible[b] = ALL feasible clusters (not capped at k); 0 = no match.  With one
 *              member per query slot all three equal hmk_assign_shifted's on the same arguments.
 *   checks     HMK_ERR_BAD_ARG (before the device is looked at: a host-only context answers them): those of
 *              hmk_assign_shifted; a null query_cluster with a non-empty query range; a query_cluster value >= n_query_clusters;
 *              a query slot without a member.  Then the checks of hmk_search_shifted.  Never HMK_ERR_CAPACITY (the call grows
 *              its own scratch); more than 2^32 - 1 hits: HMK_ERR_OOM.
 *   stats      as hmk_assign_shifted's; kernel_ms includes the pass, both aggregation levels and the selection.
 * On a hmk_create_multi context the match runs on the root device. */
int hmk_match_clusters_shifted(hmk_ctx *ctx, uint32_t q0, uint32_t q1, const uint32_t *query_cluster, uint32_t n_query_clusters,
                               uint32_t r0, uint32_t r1, const uint32_t *member_cluster, const int32_t *cluster_id, uint32_t n_clusters,
                               int max_shift, int shift_penalty, int threshold, uint32_t k,
                               uint32_t *best_cluster, int32_t *best_score, uint32_t *n_feasible, hmk_neighbor_stats *stats);
/* The same with LocalAlignmentScorer(matrix, gap_open, gap_extend).sequenceScore(seq1 = member, seq2 = query), under the
 * preconditions of hmk_search_local. */
int hmk_match_clusters_local(hmk_ctx *ctx, uint32_t q0, uint32_t q1, const uint32_t *query_cluster, uint32_t n_query_clusters,
                             uint32_t r0, uint32_t r1, const uint32_t *member_cluster, const int32_t *cluster_id, uint32_t n_clusters,
                             int gap_open, int gap_extend, int threshold, uint32_t k,
                             uint32_t *best_cluster, int32_t *best_score, uint32_t *n_feasible, hmk_neighbor_stats *stats);

/* ---- continuing a greedy clustering with new sequences ---------------------------- */

typedef struct {
    uint64_t n_edges;            /* edges at or above the threshold: new x members plus new x new */
    uint64_t pairs_scored;       /* pairs the two passes scored (members x members is never scored) */
    uint32_t n_joined;           /* new sequences that joined a cluster */
    uint32_t loop_rounds;        /* rounds of the device-side loop */
    uint32_t host_precheck;      /* 1: the device pre-check could not hold the lists (a row overflowed its tables, or a region of
                                    its buffer overran twice): the host built them */
    uint32_t reserved;
    double kernel_ms;            /* the two passes (device time) */
    double loop_ms;              /* CSR, pre-check and loop (wall) */
} hmk_continue_stats;

/* Continues a greedy clustering: the second loop of LimitedGreedySequenceClusterer.cluster
 * (LimitedGreedySequenceClusterer.java:59-67) with actualClusters = the given clusters (members in the given order) and
 * actualSequences = the new sequences in index order, scorer ShiftedScorer(matrix, shift_penalty, max_shift), cluster
 * scorer ClinkageClusterScorer(threshold).  One uploaded set (hmk_set_sequences) holds both sides:
 *   members    [r0, r1): member r is in slot member_cluster[r - r0] of [0, n_clusters); slot c has the Java id
 *              cluster_id[c] (distinct).  Cluster.size() starts as the sum of the members' uploaded sizes.
 *   new        [q0, q1), disjoint from the members, taken in the order q0, q0 + 1, ... (either side may come first).
 * New sequence x joins the cluster findNearestClusterParallel returns (ClinkageSequenceClusterer.java:243-294) if its
 * complete-linkage score is >= threshold: cluster c is feasible iff every member m of c -- the new sequences that joined
 * c before x included -- has score(m, x) >= threshold; feasible clusters rank by score, then size() descending, then id
 * ascending.  A joiner adds its uploaded size to size() (Cluster.java:70-74).  A new sequence that joins nothing stays a
 * singleton and is never a candidate for a later one (remainingSequences, :63-65): new sequences never seed clusters
 * (phase 1, :77-120, does not run).  So continuing is NOT greedy on the old sequences followed by the new ones: there,
 * phase 1 could have absorbed a new sequence into a fresh cluster.
 * Only new x members and new x new are scored, on the GPU; the pre-check and the loop run on the device
 * (hmk_greedy_cluster's k_greedy_precheck and k_loop_* rounds).
 *   joined[x - q0]       the slot x joined, or -1
 *   member_rank[x - q0]  x's position in Cluster.getSequences() after the call (the slot's member count plus the earlier
 *                        new sequences that joined it), or -1
 *   checks     HMK_ERR_BAD_ARG before the device is looked at (a host-only context answers them): the checks of
 *              hmk_assign_shifted, and an asymmetric matrix -- the device loop needs score(a, b) = score(b, a), and all
 *              17 matrices the reference ships are symmetric.  Then the checks of hmk_search_shifted.  Never
 *              HMK_ERR_CAPACITY (the call grows its own scratch).  Zero slots: every new sequence stays alone.
 * On a hmk_create_multi context the call runs on the root device. */
int hmk_greedy_continue(hmk_ctx *ctx, uint32_t q0, uint32_t q1, uint32_t r0, uint32_t r1,
                        const uint32_t *member_cluster, const int32_t *cluster_id, uint32_t n_clusters,
                        int max_shift, int shift_penalty, int threshold, int32_t *joined, int32_t *member_rank,
                        hmk_continue_stats *stats);

/* ---- greedy clustering -------------------------------------------------- */

typedef struct {
    uint64_t n_edges;            /* neighbour edges consumed */
    int32_t phase1_stop_index;   /* `index` when firstPhase ends (LimitedGreedy..java:90) */
    int32_t phase1_clusters;
    int32_t phase1_orphans;
    int32_t crash_case;          /* 0; or 1,2,3 = which NPE the reference would throw */
    int32_t crash_index;
    int32_t n_result_clusters;   /* size of the returned List<Cluster> */
    int32_t n_multi;             /* clusters with more than one member */
    int32_t reserved;
    double neighbors_ms;         /* GPU scoring (hmk_greedy_cluster only) */
    double greedy_ms;            /* host greedy merge */
} hmk_greedy_stats;

/* Replaces LimitedGreedySequenceClusterer(scorer, threshold, maxClusters).cluster(sequences)
 * (LimitedGreedySequenceClusterer.java:22,39-69) with scorer =
 * ShiftedScorer(matrix, shift_penalty, max_shift), on the sequences of
 * hmk_set_sequences (already in greedy order, UniqueSequence.sortSequences).
 *   cluster_id[n]   : id of the cluster holding sequence k (= index of its seed,
 *                     LimitedGreedySequenceClusterer.java:82)
 *   result_order[n] : ids of the returned clusters in list order (clusters first,
 *                     then singletons); first n_result_clusters entries valid; may be NULL
 *   member_rank[n]  : position of sequence k inside Cluster.getSequences() of its
 *                     cluster (insertion order, seed = 0); may be NULL
 * Returns HMK_ERR_REFERENCE_WOULD_CRASH where the reference throws
 * NullPointerException (stats->crash_case says which). */
int hmk_greedy_cluster(hmk_ctx *ctx, int max_shift, int shift_penalty, int threshold,
                       int max_clusters, int32_t *cluster_id, int32_t *result_order,
                       int32_t *member_rank, hmk_greedy_stats *stats);

/* The host-side greedy merge alone, on an edge list produced by
 * hmk_neighbors_shifted (all shards concatenated, any order).
 * symmetric != 0: each edge stands for both directions. */
int hmk_greedy_from_edges(hmk_ctx *ctx, const uint64_t *edges, uint64_t n_edges, int symmetric,
                          int threshold, int max_clusters, int32_t *cluster_id,
                          int32_t *result_order, int32_t *member_rank, hmk_greedy_stats *stats);

/* The same with the edges in device memory (one contiguous block of packed edges, e.g. what the ranks'
 * all-gather left on every GPU): adjacency built on the device, one pinned copy to the host, host merge --
 * the tail of hmk_greedy_cluster without the scoring (LimitedGreedySequenceClusterer.java:39-120 on a
 * precomputed neighbour graph).  Invalid edges (index >= n, self pairs) give HMK_ERR_BAD_ARG. */
int hmk_greedy_from_edges_dev(hmk_ctx *ctx, const void *d_edges, uint64_t n_edges, int symmetric,
                              int max_clusters, int32_t *cluster_id, int32_t *result_order,
                              int32_t *member_rank, hmk_greedy_stats *stats);

/* ---- greedy clusterings at a range of thresholds --------------------------------------- */

typedef struct {
    uint64_t n_edges;            /* pairs with score >= t */
    int32_t  status;             /* HMK_OK or HMK_ERR_REFERENCE_WOULD_CRASH at this t */
    int32_t  crash_case, crash_index;
    int32_t  phase1_stop_index, phase1_clusters, phase1_orphans;
    int32_t  n_result_clusters, n_multi;     /* as hmk_greedy_stats at this t */
    uint32_t n_singletons;       /* result clusters of one sequence */
    uint32_t largest;            /* sequences (not Cluster.size()) in the largest cluster */
    double   tail_ms;            /* wall time of this level's tail */
} hmk_greedy_level;

typedef struct {
    uint64_t n_edges, pairs_scored;   /* edges >= threshold; 0 pairs for the _from_edges forms: nothing is scored */
    uint32_t n_levels, reserved;      /* threshold_hi - threshold + 1 */
    double kernel_ms;            /* the scoring pass, HIP events */
    double deal_ms;              /* the three k_sweep kernels, HIP events (0 for hmk_greedy_sweep_from_edges) */
} hmk_greedy_sweep_stats;

/* Replaces one LimitedGreedySequenceClusterer(scorer, t, maxClusters).cluster(sequences)
 * (LimitedGreedySequenceClusterer.java:22,39-69) per threshold t = threshold ... threshold_hi, scorer =
 * ShiftedScorer(matrix, shift_penalty, max_shift), with ONE scoring pass at `threshold`: the neighbour graph at the lowest threshold
 * holds every higher threshold's graph, each edge carries its score.
 *   cluster_id, result_order, member_rank   each [n_levels][n] or NULL; row t - threshold is exactly what
 *                           hmk_greedy_cluster(..., t, max_clusters, ...) writes (entries of result_order behind the level's
 *                           n_result_clusters are -1)
 *   levels[t - threshold]   may be NULL; the fields it shares with hmk_greedy_stats are that call's stats
 *   a level where the reference would throw: the failure is recorded in that level (status, crash_case, crash_index), its rows
 *                           are filled with -1, the sweep goes on and returns HMK_OK.  Any other error ends the call.
 *   checks                  HMK_ERR_BAD_ARG before the device is looked at (a host-only context answers them): threshold_hi <
 *                           threshold, threshold_hi - threshold > 255, threshold_hi > 32767, levels and all three arrays NULL
 *                           with n > 0.  Then the checks of hmk_greedy_cluster at `threshold`.  Never HMK_ERR_CAPACITY (the call
 *                           grows its own scratch).  No sequences: HMK_OK, zeroed levels.
 * The pass is hmk_neighbors_shifted's (same plan slot, same kernels) into the context's edge buffer; behind it k_sweep.hip: a
 * histogram of the edges' levels min(score, threshold_hi) - threshold, the whole edges dealt into one run per level with the top
 * level first, so that the edges with score >= t are a prefix of one buffer; then per level the tail of hmk_greedy_cluster on that
 * prefix.  On a hmk_create_multi context the call runs on the root device. */
int hmk_greedy_sweep(hmk_ctx *ctx, int max_shift, int shift_penalty, int threshold, int threshold_hi, int max_clusters,
                     int32_t *cluster_id, int32_t *result_order, int32_t *member_rank, hmk_greedy_level *levels,
                     hmk_greedy_sweep_stats *stats);

/* The same (LimitedGreedySequenceClusterer.java:22,39-69, once per threshold) from packed HMK_EDGE_* edges as
 * hmk_greedy_from_edges takes them, any order; the scores are read from the edges, an edge with a score below `threshold` is
 * ignored, one above threshold_hi counts at every level and keeps its score; an index >= n or a self pair is HMK_ERR_BAD_ARG.
 * On the host: the edges sorted by level by counting, hmk_greedy_from_edges's merge per prefix.  Works on a host-only context, and
 * is the second implementation the device path is tested against. */
int hmk_greedy_sweep_from_edges(hmk_ctx *ctx, const uint64_t *edges, uint64_t n_edges, int symmetric, int threshold, int threshold_hi,
                                int max_clusters, int32_t *cluster_id, int32_t *result_order, int32_t *member_rank,
                                hmk_greedy_level *levels, hmk_greedy_sweep_stats *stats);

/* The same (LimitedGreedySequenceClusterer.java:22,39-69, once per threshold) with the edges in device memory (the context's
 * device), through the kernels and tails of hmk_greedy_sweep.  An index >= n or a self pair is found on the device, before any
 * array is indexed with it: HMK_ERR_BAD_ARG. */
int hmk_greedy_sweep_from_edges_dev(hmk_ctx *ctx, const void *d_edges, uint64_t n_edges, int symmetric, int threshold, int threshold_hi,
                                    int max_clusters, int32_t *cluster_id, int32_t *result_order, int32_t *member_rank,
                                    hmk_greedy_level *levels, hmk_greedy_sweep_stats *stats);

/* ---- greedy clusterings under many orders of the set: order stability -------------------- */

typedef struct {
    int32_t  status;             /* HMK_OK or HMK_ERR_REFERENCE_WOULD_CRASH in this order */
    int32_t  crash_case, crash_index;        /* as hmk_greedy_stats; crash_index is a position of THIS order */
    int32_t  phase1_stop_index, phase1_clusters, phase1_orphans;
    int32_t  n_result_clusters, n_multi;     /* as hmk_greedy_stats in this order */
    uint32_t n_singletons;       /* result clusters of one sequence */
    uint32_t largest;            /* sequences (not Cluster.size()) in the largest cluster */
    uint64_t pairs_together;     /* unordered pairs inside one cluster in this order = the sum of C(members, 2) over its clusters */
    uint64_t pairs_with_first;   /* of those, also together in the first valid order */
    double   tail_ms;            /* wall time of this order's relabel and tail */
} hmk_greedy_order;

typedef struct {
    uint64_t n_edges, pairs_scored;   /* edges >= threshold; 0 pairs for the _from_edges form: nothing is scored */
    uint32_t n_orders, n_valid;       /* valid = orders in which the reference does not throw */
    uint64_t pairs_ever, pairs_always;   /* pairs with support >= 1 / == n_valid */
    uint32_t n_consensus, n_consensus_singletons, consensus_largest, reserved;
    double kernel_ms;            /* the scoring pass, HIP events */
    double relabel_ms;           /* all k_orders_relabel launches, HIP events */
    double support_ms;           /* k_orders_support and the consensus kernels, HIP events (the three: 0 for the _from_edges form) */
} hmk_greedy_orders_stats;

/* Replaces one LimitedGreedySequenceClusterer(scorer, threshold, maxClusters).cluster(list k)
 * (LimitedGreedySequenceClusterer.java:22,39-69) per order k, scorer = ShiftedScorer(matrix, shift_penalty, max_shift), with ONE
 * scoring pass: list k = the uploaded set in order k with its sizes, i.e. what UniqueSequence.sortSequences would hand over under
 * another -R.  The greedy clustering depends on the order by construction (:39-120); the scores do not.
 *   orders[k][pos]         uploaded index of the sequence standing at position pos of order k; every row a permutation of [0, n);
 *                          1 <= n_orders <= 256
 *   cluster_id, result_order, member_rank   each [n_orders][n] or NULL, indexed by UPLOADED index, clusters named by the uploaded
 *                          index of their seed: cluster_id[k][i] = seed of i's cluster, result_order[k][j] = seed of the j-th returned
 *                          cluster (-1 behind n_result_clusters), member_rank[k][i] as in hmk_greedy_cluster.  The reference's id of
 *                          a cluster is its seed's position in order k: with pos_k = the inverse of orders[k], pos_k[cluster_id[k][i]].
 *                          For the identity order the rows and the shared stats fields are exactly hmk_greedy_cluster's; for any
 *                          order they are that call's result on the permuted upload, mapped back.
 *   per_order[k]           may be NULL.  An order where the reference would throw is recorded there (status, crash_case,
 *                          crash_index), its rows are -1, it takes no part in anything below; the call goes on and returns HMK_OK.
 *   support                support(i, j) = the valid orders in which i and j share a cluster.  With complete linkage every pair
 *                          inside a cluster is an edge of the neighbour graph at `threshold`, so the support lives on the edge list.
 *   support_edges          every pair with support >= 1 once, as HMK_EDGE_*: x < m (uploaded indices), the support (<= 256) in the
 *                          score field, order unspecified -- a valid input of hmk_components_from_edges with a support level as its
 *                          threshold.  NULL: none returned, no error.  HMK_ERR_CAPACITY when `capacity` is too small (every other
 *                          output is written); *n_support_edges (may be NULL) = the number needed, in either case.
 *   partners_ever[i], partners_always[i]   the j with support(i, j) >= 1 / == n_valid
 *   consensus[i]           smallest uploaded index in i's component of the graph of the pairs with support >= min_support;
 *                          min_support 0 means n_valid.  At n_valid the components are exactly the meet of the valid partitions
 *                          ("together in every order" is an equivalence relation); below that the consensus is SINGLE linkage over
 *                          the support: two sequences may share a consensus cluster without ever having shared a cluster.  A level
 *                          above n_valid is reached by no pair.  Without a valid order every sequence is alone, the partner counts 0.
 *   checks                 HMK_ERR_BAD_ARG before the device is looked at (a host-only context answers them): n_orders outside
 *                          1 .. 256, NULL orders or stats, a row that is no permutation, min_support > n_orders, NULL support_edges
 *                          with capacity > 0, every output NULL with n > 0, an asymmetric matrix (the orientation of an equal-length
 *                          pair's score depends on who comes first, ShiftedScorer.java:51-57, and the pass scores one).  Then the
 *                          checks of hmk_greedy_cluster at `threshold`.  No sequences: HMK_OK, zeroed outputs.
 * The pass is hmk_neighbors_shifted's (same plan slot, same kernels) into the context's edge buffer; behind it k_orders.hip: per order
 * the edges renamed to the order's positions and the tail of hmk_greedy_cluster on them (Cluster.size() through a permuted view: the
 * sequences are not uploaded again, the context's sizes are not touched), once the supports over the original edges with the cluster
 * ids transposed, then k_components.hip's union-find over the support edges.  On a hmk_create_multi context the call runs on the
 * root device. */
int hmk_greedy_orders(hmk_ctx *ctx, int max_shift, int shift_penalty, int threshold, int max_clusters,
                      const uint32_t *orders, uint32_t n_orders, uint32_t min_support,
                      int32_t *cluster_id, int32_t *result_order, int32_t *member_rank, hmk_greedy_order *per_order,
                      uint32_t *partners_always, uint32_t *partners_ever, uint32_t *consensus,
                      uint64_t *support_edges, uint64_t capacity, uint64_t *n_support_edges, hmk_greedy_orders_stats *stats);

/* The same from packed HMK_EDGE_* edges: each unordered pair once, either orientation, any order; the scores are read from the
 * edges, an edge below `threshold` is ignored, an index >= n or a self pair is HMK_ERR_BAD_ARG.  Plain host code: relabel,
 * hmk_greedy_from_edges's merge per order, supports by a loop, a sequential union-find.  Works on a host-only context, and is the
 * second implementation the device path is tested against. */
int hmk_greedy_orders_from_edges(hmk_ctx *ctx, const uint64_t *edges, uint64_t n_edges, int threshold, int max_clusters,
                                 const uint32_t *orders, uint32_t n_orders, uint32_t min_support,
                                 int32_t *cluster_id, int32_t *result_order, int32_t *member_rank, hmk_greedy_order *per_order,
                                 uint32_t *partners_always, uint32_t *partners_ever, uint32_t *consensus,
                                 uint64_t *support_edges, uint64_t capacity, uint64_t *n_support_edges, hmk_greedy_orders_stats *stats);

/* ---- clinkage mode ------------------------------------------------------- */

typedef struct {
    uint64_t n_edges;            /* neighbour edges consumed */
    int32_t merges;              /* clusters joined (ClinkageSequenceClusterer.java:96-111) */
    int32_t searches;            /* nearest-neighbour searches (:77) */
    int32_t n_result_clusters;   /* size of the returned List<Cluster> */
    int32_t reserved;
    double neighbors_ms;         /* GPU scoring */
    double chain_ms;             /* host nearest-neighbour chain */
} hmk_clinkage_stats;

/* Replaces ClinkageSequenceClusterer(ShiftedScorer(matrix, shift_penalty, max_shift), threshold).cluster(sequences)
 * (ClinkageSequenceClusterer.java:29-33,43-124; driver Hammock.java:449-462; the reference's default initial clustering
 * for up to 10,000 unique sequences, Hammock.java:371-377) on the sequences of hmk_set_sequences, which are in LOAD
 * order -- clinkage mode does not sort.  The whole pair space is scored on the GPU; the nearest-neighbour chain runs
 * on the host over the thresholded graph.
 *   cluster_id[n]   : id of the returned cluster holding sequence k: k + 1 for a sequence left alone, n + 2, n + 3, ...
 *                     for merged clusters in merge order (:49-55,97)
 *   result_order[n] : ids of the returned clusters in list order = iteration order of the java.util.HashSet
 *                     readyClusters (:121-123; Java 8 and later); first n_result_clusters entries valid; may be NULL
 *   member_rank[n]  : position of sequence k inside Cluster.getSequences() (:105-106); may be NULL
 * The cacheSizeLimit of -L/--cache_size_limit never reaches the clusterer in the reference (Hammock.java:459 uses the
 * two-argument constructor), so there is no such parameter.  Needs a symmetric matrix (HMK_ERR_BAD_ARG otherwise: the
 * reference's score cache is keyed by the unordered pair, so with score(a,b) != score(b,a) its result depends on which
 * direction happened to be asked first).  An empty input is HMK_ERR_REFERENCE_WOULD_CRASH (NoSuchElementException, :118).
 * So is an input on which the reference's chain returns to a cluster that is still on its stack (a tie of score, size
 * and id order, :96-113 pushes it again): the reference then works with a stale Cluster object and throws
 * NoSuchElementException or returns a list in which a sequence belongs to two clusters -- there is no cluster_id[] for
 * that (hmk_last_error names the cluster; four 6-mers suffice, tests/test_oracle.py). */
int hmk_clinkage_cluster(hmk_ctx *ctx, int max_shift, int shift_penalty, int threshold, int32_t *cluster_id,
                         int32_t *result_order, int32_t *member_rank, hmk_clinkage_stats *stats);

/* Optional.  Sizes the context's grow-only device and pinned buffers for a first hmk_greedy_cluster / hmk_clinkage_cluster
 * call on n_sequences sequences (edge buffer at the first guess of 0.3 % of the pair space, adjacency, CSR and second-loop
 * scratch: 36 GB at 10^6), so that a host which knows the sequence count early -- hammock-hip after it has read its input --
 * can have the allocations done on another thread while it is still sorting and packing the sequences.  Calls on a context
 * are serialised; a later call that needs more grows the buffers as usual.  HMK_OK on a host-only context (nothing to do).
 * The two buffers a call needs LAST (the adjacency and the CSR's bucket records, 2 x 11 GB at 10^6) are obtained on a thread
 * of the library's own after this function has returned -- on some hosts fresh device memory of that size takes 0.3-1.5 s to
 * get --; a clustering call that starts in the meantime scores, hands the band over and runs phase 1 first and enqueues its
 * CSR step when they are there (hmk_destroy joins the thread). */
int hmk_reserve(hmk_ctx *ctx, uint32_t n_sequences);

/* Which java.util.HashSet iteration order hmk_clinkage_cluster / hmk_clinkage_from_edges emulate for
 * `activeClusters.iterator().next()` (ClinkageSequenceClusterer.java:70, the arbitrary start of every chain) and for the
 * returned list (:118-123).  version 8 (default): Java 8 and later; 7: JDK 7u6 ... 7u80 (the reference is a Java 1.7
 * project, nbproject/project.properties:45-46); 6: JDK 6 and JDK 7 before 7u6.  The orders differ in hash spreading, in
 * where a new entry joins its bucket's chain and in what a resize does to a chain; cluster MEMBERSHIP differs only where a
 * tie of score, size and id order lets the chain start decide.  HMK_ERR_BAD_ARG for any other version. */
int hmk_set_java_hashset(hmk_ctx *ctx, int version);


/* The host-side nearest-neighbour chain alone, on the edge list of a symmetric matrix as hmk_neighbors_shifted produces it
 * (each unordered pair once, any order; all shards concatenated).  Works on a host-only context (device = -1). */
int hmk_clinkage_from_edges(hmk_ctx *ctx, const uint64_t *edges, uint64_t n_edges, int32_t *cluster_id,
                            int32_t *result_order, int32_t *member_rank, hmk_clinkage_stats *stats);

/* ---- merging given clusters by complete linkage ----------------------------------- */

typedef struct {
    uint64_t n_edges;          /* sequence-level edges at or above the threshold */
    uint64_t pairs_scored;
    uint64_t cluster_pairs;    /* unordered pairs of given clusters that are feasible for each other */
    int32_t  merges, searches, n_result_clusters, reserved;
    double   kernel_ms;        /* the scoring pass (device) */
    double   graph_ms;         /* CSR + cluster graph (device) */
    double   chain_ms;         /* host nearest-neighbour chain */
} hmk_merge_stats;

/* The cluster-level graph of given clusters.  Members [r0, r1) of the hmk_set_sequences set with member_cluster and n_clusters
 * as hmk_assign_shifted takes them.  Clusters a and b are feasible for each other iff every pair (member of a, member of b)
 * scores >= threshold with ShiftedScorer(matrix, shift_penalty, max_shift); their complete-linkage score is then the minimum
 * over those pairs (ClinkageClusterScorer.java:30-49).  Scores inside a cluster are never looked at.
 *   pairs      every unordered pair {a, b} of slots, a != b, feasible for each other, once, packed as HMK_EDGE_* with x = the
 *              smaller slot, m = the larger slot, score = the complete-linkage score; order unspecified.  HMK_ERR_CAPACITY and
 *              *n_pairs = the number needed if `capacity` is too small.
 *   checks     HMK_ERR_BAD_ARG before the device is looked at (a host-only context answers them): the range and slot checks of
 *              hmk_assign_shifted (without ids), an asymmetric matrix, two clusters whose member counts multiply to 2^32 or
 *              more.  Then the checks of hmk_search_shifted.
 * Only the triangle inside [r0, r1) is scored; the sequence-level edges and their CSR stay on the device, the cluster graph is
 * built there (k_merge.hip) and only the cluster pairs cross to the host.  On a hmk_create_multi context the call runs on the
 * root device. */
int hmk_cluster_pairs_shifted(hmk_ctx *ctx, uint32_t r0, uint32_t r1, const uint32_t *member_cluster, uint32_t n_clusters,
                              int max_shift, int shift_penalty, int threshold, uint64_t *pairs, uint64_t capacity,
                              uint64_t *n_pairs, hmk_merge_stats *stats);

/* Merges given clusters: ClinkageSequenceClusterer(ShiftedScorer(matrix, shift_penalty, max_shift), threshold).cluster
 * (ClinkageSequenceClusterer.java:43-124) with its seeding (:50-55, one cluster per sequence) replaced by "activeClusters =
 * the given clusters, added in slot order 0, 1, ..."; every other line is the reference's.
 *   slot c     a Cluster with Java id cluster_id[c] (distinct, within [1, 2^30]) and the members of the slot in index order
 *              (Cluster.getSequences()); size() = the sum of the members' uploaded sizes, getUniqueSize() = the member count.
 *   ids        currentId after the seeding is max(cluster_id) + 1, so merged clusters get max + 2, max + 3, ... in merge
 *              order (:97); with the slots being the singletons 1 ... n this is hmk_clinkage_cluster.
 *   ranking    cluster score = ClinkageClusterScorer.clusterScore; nearest cluster by score, then size() descending, then
 *              smaller id (:137-177, :258-293); chain starts and the returned list's order are HashSet<Cluster> iteration
 *              orders (:70, :118-123) of the Java version hmk_set_java_hashset selects.
 *   inside     scores inside a given cluster are never looked at: it need not be a complete-linkage cluster itself.
 *   merged_id[n_clusters]     id of the returned cluster that holds slot c (its own id if it merged with nothing)
 *   result_order[n_clusters]  ids of the returned clusters in list order, first n_result_clusters valid; may be NULL
 *   member_rank[r1 - r0]      position in the returned Cluster.getSequences() (:105-106); may be NULL
 * Zero clusters: HMK_ERR_REFERENCE_WOULD_CRASH (NoSuchElementException, :118); so is a chain that returns to a cluster still
 * on its stack (see hmk_clinkage_cluster).  One cluster: returned as it is.  A HashSet bucket that Java 8+ would turn into a
 * tree bin is not modelled: HMK_ERR_BAD_ARG.  With the consecutive ids of hmk_clinkage_cluster that cannot happen; with
 * caller-chosen ids it can (eight ids in one bucket of a table of 64 or more), so choose consecutive ids where possible.
 * Checks as hmk_cluster_pairs_shifted's, plus duplicate ids and an id outside [1, 2^30]; never HMK_ERR_CAPACITY. */
int hmk_clinkage_merge(hmk_ctx *ctx, uint32_t r0, uint32_t r1, const uint32_t *member_cluster, const int32_t *cluster_id,
                       uint32_t n_clusters, int max_shift, int shift_penalty, int threshold, int32_t *merged_id,
                       int32_t *result_order, int32_t *member_rank, hmk_merge_stats *stats);

/* The same from a sequence-level edge list as hmk_neighbors_shifted produces it (indices of the uploaded set, each unordered
 * pair once, any order; edges with an end outside [r0, r1) or with both ends in one slot are ignored).  Works on a host-only
 * context (device = -1): the cluster graph is built on the host. */
int hmk_clinkage_merge_from_edges(hmk_ctx *ctx, const uint64_t *edges, uint64_t n_edges, uint32_t r0, uint32_t r1,
                                  const uint32_t *member_cluster, const int32_t *cluster_id, uint32_t n_clusters,
                                  int32_t *merged_id, int32_t *result_order, int32_t *member_rank, hmk_merge_stats *stats);

/* ---- complete-linkage scores inside given clusters -------------------------------- */

typedef struct {
    uint64_t pairs_scored;     /* sum over slots of s(s-1)/2 */
    uint32_t n_multi;          /* slots with two or more members */
    uint32_t n_violating;      /* slots with a pair below the threshold */
    uint32_t launches, reserved;
    double   kernel_ms;        /* device time, HIP events */
} hmk_linkage_stats;

/* Is a given clustering a set of complete-linkage clusters at these parameters, and which clusters and members break it?  The
 * half hmk_cluster_pairs_shifted leaves open: that call covers the pairs between clusters, this one the pairs inside a cluster.
 * Members [r0, r1) of the hmk_set_sequences set with member_cluster and n_clusters as hmk_cluster_pairs_shifted takes them.
 *   score      score(a, b) = ShiftedScorer(matrix, shift_penalty, max_shift).sequenceScore(seq1 = the larger index, seq2 = the
 *              smaller) (ShiftedScorer.java:48-100), the orientation of the edges of hmk_neighbors_shifted.
 *   per slot c, over the unordered pairs {a, b} of distinct members of c:
 *     min_score[c]         the minimum score: what ClinkageClusterScorer.clusterScore computes without its early exit
 *                          (ClinkageClusterScorer.java:30-49), applied inside a single cluster
 *     min_a[c] < min_b[c]  the pair that attains it (indices of the uploaded set); among tied pairs the smallest min_a, then the
 *                          smallest min_b
 *     n_below[c]           the number of pairs with score < threshold (a pair scoring exactly the threshold is not below): slot c
 *                          is a complete-linkage cluster at these parameters iff n_below[c] == 0
 *     a slot of one member gets INT32_MAX, UINT32_MAX, UINT32_MAX, 0
 *   per member m (both arrays may be NULL, together): member_min[m - r0] = the minimum score of m against the other members of
 *     its slot (INT32_MAX in a slot of one member), member_below[m - r0] = how many of those scores are below the threshold: the
 *     members to evict.
 *   checks     HMK_ERR_BAD_ARG before the device is looked at (a host-only context answers them): the range and slot checks of
 *              hmk_cluster_pairs_shifted, a null member_cluster with a non-empty range, a null required output, an asymmetric
 *              matrix.  Then the checks of hmk_search_shifted over the range (the shift against the shortest length, threshold
 *              and int16 limits; here the lowest possible score must fit int16 as well).  Never HMK_ERR_CAPACITY.
 * Every pair inside a slot is scored, sum of s(s-1)/2, and nothing else: no pass over [r0, r1), no edge list.  Slots of few
 * members have their pairs enumerated flat over all such slots, large ones are tiled (k_linkage.hip); the scratch is
 * O(members + clusters).  On a hmk_create_multi context the call runs on the root device. */
int hmk_cluster_linkage_shifted(hmk_ctx *ctx, uint32_t r0, uint32_t r1, const uint32_t *member_cluster, uint32_t n_clusters,
                                int max_shift, int shift_penalty, int threshold, int32_t *min_score, uint32_t *min_a,
                                uint32_t *min_b, uint64_t *n_below, int32_t *member_min, uint32_t *member_below,
                                hmk_linkage_stats *stats);

/* ---- splitting given clusters by complete linkage ------------------------------------ */

typedef struct {
    uint64_t pairs_scored;       /* sum over slots of s(s-1)/2 (0 for hmk_clinkage_split_from_edges: nothing is scored) */
    uint64_t n_edges;            /* pairs inside a slot scoring >= threshold (_from_edges: the edges it kept) */
    uint32_t n_multi;            /* slots with two or more members */
    uint32_t n_split;            /* slots returned in more than one part */
    uint32_t n_result_clusters;  /* parts of all slots: the n_clusters that goes with split_cluster */
    uint32_t merges;             /* clusters joined, all chains (ClinkageSequenceClusterer.java:96-111) */
    int32_t  crash_slot;         /* the slot HMK_ERR_REFERENCE_WOULD_CRASH names, -1 otherwise */
    int32_t  reserved;
    double   kernel_ms;          /* device time of the scoring, HIP events */
    double   chain_ms;           /* host wall time of all chains, their seeding included */
    double   copy_ms;            /* device time of the triangles' copy to the host, HIP events */
} hmk_split_stats;

/* Splits given clusters: the reverse of hmk_clinkage_merge.  That call runs the reference's complete-linkage chain between given
 * clusters and never looks inside one; this one runs it inside each given cluster and never looks between two.  It is what acts
 * on hmk_cluster_linkage_shifted's answer: a cluster file that fails that check -- a looser threshold, another matrix, another
 * tool, an edit by hand -- comes back as complete-linkage clusters at these parameters without being clustered from nothing.
 * Members [r0, r1) of the hmk_set_sequences set with member_cluster and n_clusters as hmk_cluster_linkage_shifted takes them.
 *   per slot c with the members m_0 < m_1 < ... < m_(s-1): what hmk_clinkage_cluster returns for a set that holds exactly those s
 *     sequences in that order (ClinkageSequenceClusterer.java:43-124 on the slot alone): the uploaded sizes (Cluster.size(), the
 *     tie-break), the HashSet order hmk_set_java_hashset selects.
 *   n_parts[c]             the number of returned clusters of slot c; 1 for a slot of one member
 *   part_id[m - r0]        the Java id inside the slot's own run: k + 1 for the member at place k left alone, s + 2, s + 3, ...
 *                          for merged clusters in merge order; may be NULL
 *   member_rank[m - r0]    the position in the returned Cluster.getSequences(); may be NULL
 *   part_order[part_start[c] .. part_start[c] + n_parts[c])   the slot's returned ids in list order; part_start[c] = the number of
 *                          members in slots below c, part_start has n_clusters + 1 entries and part_order r1 - r0; NULL together
 *                          or not at all
 *   split_cluster[m - r0]  required: all parts numbered densely, slots in slot order and inside a slot its parts in list order.
 *                          split_cluster with stats.n_result_clusters is the member_cluster / n_clusters of the new clustering
 *                          for every other call here: hmk_cluster_linkage_shifted finds no pair below the threshold in it.
 *   crash parity           a slot whose chain returns to a cluster still on its stack (see hmk_clinkage_cluster) makes the call
 *                          return HMK_ERR_REFERENCE_WOULD_CRASH; hmk_last_error and stats.crash_slot name the lowest such slot,
 *                          whatever the number of host threads; the outputs are then unspecified.  An empty range is HMK_OK with
 *                          nothing written.  The tree-bin case of hmk_clinkage_merge cannot arise: a slot's ids are consecutive.
 *   checks                 HMK_ERR_BAD_ARG before the device is looked at (a host-only context answers them): every check of
 *                          hmk_cluster_linkage_shifted (so a slot without members is refused, the matrix must be symmetric, and
 *                          the scores must fit int16 at both ends: they travel as int16); a null split_cluster or n_parts with a
 *                          non-empty range; part_order without part_start or the reverse; more than 2^30 pairs inside the slots of
 *                          one call, sum of s(s-1)/2 -- pass fewer slots per call then, slots are independent.  The bound keeps
 *                          the score buffer at 2 GiB and the candidate lists at what hmk_clinkage_cluster takes on a dense graph
 *                          of that many pairs.  Never HMK_ERR_CAPACITY.
 * Every pair inside a slot is scored and stored, a dense strict lower triangle of int16 per slot (k_split.hip; flat for slots of
 * few members, tiled for large ones, as the linkage call's kernels); the triangles cross to the host in one piece and the chains
 * run there, one per slot, on up to 8 threads; the result does not depend on their number.  On a hmk_create_multi context the call
 * runs on the root device. */
int hmk_clinkage_split(hmk_ctx *ctx, uint32_t r0, uint32_t r1, const uint32_t *member_cluster, uint32_t n_clusters,
                       int max_shift, int shift_penalty, int threshold, uint32_t *split_cluster, uint32_t *n_parts,
                       int32_t *part_id, int32_t *member_rank, int32_t *part_order, uint32_t *part_start,
                       hmk_split_stats *stats);

/* The same from a sequence-level edge list as hmk_neighbors_shifted packs it (indices of the uploaded set, each unordered pair
 * once, any order; edges with an end outside [r0, r1) or with ends in two slots are ignored).  Works on a host-only context
 * (device = -1).  Checks as hmk_clinkage_split's without those of the scoring parameters. */
int hmk_clinkage_split_from_edges(hmk_ctx *ctx, const uint64_t *edges, uint64_t n_edges, uint32_t r0, uint32_t r1,
                                  const uint32_t *member_cluster, uint32_t n_clusters, uint32_t *split_cluster,
                                  uint32_t *n_parts, int32_t *part_id, int32_t *member_rank, int32_t *part_order,
                                  uint32_t *part_start, hmk_split_stats *stats);

/* ---- connected components of the neighbour graph -------------------------------------- */

typedef struct {
    uint64_t n_edges;        /* pairs with score >= t */
    uint32_t n_components;   /* components of the graph {score >= t} */
    uint32_t n_singletons;   /* components of one member */
    uint32_t largest;        /* members of the largest component */
    uint32_t reserved;
} hmk_component_level;

typedef struct {
    uint64_t n_edges;        /* edges >= threshold */
    uint64_t pairs_scored;   /* 0 for the _from_edges forms: nothing is scored */
    uint32_t n_levels;       /* threshold_hi - threshold + 1 */
    uint32_t n_components, n_singletons, largest;   /* at `threshold` */
    double   kernel_ms;      /* the scoring pass, HIP events */
    double   components_ms;  /* the kernels behind the pass on the device, HIP events (0 for hmk_components_from_edges) */
} hmk_components_stats;

/* The connected components of the neighbour graph of the whole hmk_set_sequences set, a ~ b iff
 * ShiftedScorer(matrix, shift_penalty, max_shift).sequenceScore >= t, for every t = threshold ... threshold_hi from ONE scoring
 * pass at `threshold`.  What a component means to the other calls: ClinkageClusterScorer.clusterScore returns MIN_VALUE + 1 as
 * soon as one pair of two clusters is below the threshold (ClinkageClusterScorer.java:36-48), so no cluster that the greedy or the
 * complete-linkage calls here (cluster, assign, continue, match, merge, split) can form at t crosses a component at t, and a
 * component of one member is a singleton in all of them.  Components are independent inputs for hmk_clinkage_split / _merge.
 *   component[i]            the smallest index of the uploaded set in i's component at the level `threshold`; may be NULL.  It
 *                           does not depend on the order of the edges, on the plan's order or on the pass's segments.
 *   levels[t - threshold]   for t = threshold ... threshold_hi; may be NULL.  threshold_hi == threshold is the single-level call.
 *   checks                  HMK_ERR_BAD_ARG before the device is looked at (a host-only context answers them): threshold_hi <
 *                           threshold, threshold_hi - threshold > 255, component and levels both NULL with n > 0, an asymmetric
 *                           matrix (as hmk_clinkage_cluster).  Then the checks of hmk_neighbors_shifted at `threshold`.  Never
 *                           HMK_ERR_CAPACITY (the call grows its own scratch).  No sequences: HMK_OK, zeroed levels.
 * The pass is hmk_neighbors_shifted's (same plan slot, same kernels) into the context's edge buffer; behind it k_components.hip: a
 * histogram of the edges' levels min(score, threshold_hi) - threshold, the edges dealt into one run per level, and per level from
 * threshold_hi down one lock-free union-find launch (the larger root is hooked under the smaller), one that flattens the trees and
 * counts the members per root, one that reads singletons and the largest component off those counts.  A single-level call without
 * `levels` unites straight from the pass's segments.  Only the levels and one label array cross to the host.  On a
 * hmk_create_multi context the call runs on the root device. */
int hmk_components_shifted(hmk_ctx *ctx, int max_shift, int shift_penalty, int threshold, int threshold_hi,
                           uint32_t *component, hmk_component_level *levels, hmk_components_stats *stats);

/* The same from packed HMK_EDGE_* edges: each unordered pair once, either orientation, any order; the scores are read from the
 * edges, an edge with a score below `threshold` is ignored; an index >= n or a self pair is HMK_ERR_BAD_ARG.  A plain sequential
 * union-find on the host (edges sorted by score, descending, by counting): works on a host-only context, and is the second
 * implementation the device path is tested against.  No symmetry check: nothing is scored. */
int hmk_components_from_edges(hmk_ctx *ctx, const uint64_t *edges, uint64_t n_edges, int threshold, int threshold_hi,
                              uint32_t *component, hmk_component_level *levels, hmk_components_stats *stats);

/* The same with the edges in device memory (the context's device), through the kernels of hmk_components_shifted.  An index >= n
 * or a self pair is found on the device, before any array is touched with it: HMK_ERR_BAD_ARG. */
int hmk_components_from_edges_dev(hmk_ctx *ctx, const void *d_edges, uint64_t n_edges, int threshold, int threshold_hi,
                                  uint32_t *component, hmk_component_level *levels, hmk_components_stats *stats);

/* ---- representatives: a non-redundant subset of the set --------------------------------- */

typedef struct {
    uint64_t n_edges;             /* edges given with score >= t (as the other calls count them: every entry of the list) */
    uint32_t n_representatives;
    uint32_t n_isolated;          /* sequences without any neighbour at t (each one is a representative) */
    uint32_t largest;             /* members of the largest group by `nearest`, its representative included */
    uint32_t n_rounds;            /* rounds the device needed at this level; 0 for hmk_representatives_from_edges */
    uint32_t reserved[2];
} hmk_representative_level;

typedef struct {
    uint64_t n_edges;             /* edges >= threshold */
    uint64_t pairs_scored;        /* 0 for the _from_edges forms: nothing is scored */
    uint32_t n_levels;            /* threshold_hi - threshold + 1 */
    uint32_t n_representatives, n_isolated, largest;   /* at `threshold` */
    uint32_t rounds_total;        /* the sum of the levels' n_rounds */
    uint32_t reserved;
    double   kernel_ms;           /* the scoring pass, HIP events */
    double   select_ms;           /* everything behind the pass on the device, the levels' copies included, HIP events (0 for
                                     hmk_representatives_from_edges) */
} hmk_representatives_stats;

/* The representatives of the hmk_set_sequences set at every t = threshold ... threshold_hi, from ONE scoring pass at `threshold`:
 * the greedy incremental selection of CD-HIT and UCLUST on the neighbour graph a ~ b iff ShiftedScorer(matrix, shift_penalty,
 * max_shift).sequenceScore >= t.  Walk the sequences in caller order; a sequence becomes a representative unless an earlier
 * representative is its neighbour.  On the graph that is the lexicographically first maximal independent set.  The set is not
 * monotone in t: every level is decided on its own.
 *   representative          i is one iff no representative r < i is a neighbour of i, decided for i = 0, 1, 2, ... in order
 *   covered_by[l][i]        i itself for a representative, else the smallest-index representative among i's neighbours (it is < i)
 *   nearest[l][i], nearest_score[l][i]   i and INT32_MAX for a representative, else the representative neighbour with the largest
 *                           score (it may have a larger index than i), among equal scores the smaller index, and that score
 *   levels[l]               l = t - threshold; the arrays are [n_levels][n], each may be NULL, levels may be NULL
 *   checks                  HMK_ERR_BAD_ARG before the device is looked at (a host-only context answers them): threshold_hi <
 *                           threshold, threshold_hi - threshold > 255, threshold_hi > 32767, all four outputs NULL with n > 0, an
 *                           asymmetric matrix (as hmk_components_shifted).  Then the checks of hmk_neighbors_shifted at `threshold`.
 *                           Never HMK_ERR_CAPACITY (the call grows its own scratch).  No sequences: HMK_OK, zeroed levels.
 * The pass is hmk_neighbors_shifted's (same plan slot, same kernels) into the context's edge buffer.  A range is dealt by the
 * kernels of hmk_greedy_sweep into one run per level with the top level first, so that the edges >= t are a prefix; a single level
 * reads the pass's segments where they lie.  Per level k_representatives.hip runs synchronous rounds: a marking kernel over the
 * live edges that only reads the vertices' states, a decision kernel over the vertices; a vertex is decided only once its decision
 * is forced, so the result and n_rounds do not depend on the grid or the schedule.  The host polls a progress word and keeps one
 * round in the queue beside the running one.  Two more kernels assign covered_by and nearest.  Only the result arrays cross to the
 * host.  On a hmk_create_multi context the call runs on the root device. */
int hmk_representatives_shifted(hmk_ctx *ctx, int max_shift, int shift_penalty, int threshold, int threshold_hi,
                                uint32_t *covered_by, uint32_t *nearest, int32_t *nearest_score,
                                hmk_representative_level *levels, hmk_representatives_stats *stats);

/* The same from packed HMK_EDGE_* edges read as an undirected graph: a pair is adjacent if it appears in either orientation, any
 * number of times, and its score is the largest it appears with; edges below `threshold` are ignored, one above threshold_hi counts
 * at every level and keeps its score; an index >= n or a self pair is HMK_ERR_BAD_ARG.  This is the definition written plainly on
 * the host (lower adjacency by counting, one walk in index order per level, one pass over the edges for covered_by and nearest):
 * it works on a host-only context, and is the second implementation the device path is tested against.  No symmetry check:
 * nothing is scored. */
int hmk_representatives_from_edges(hmk_ctx *ctx, const uint64_t *edges, uint64_t n_edges, int threshold, int threshold_hi,
                                   uint32_t *covered_by, uint32_t *nearest, int32_t *nearest_score,
                                   hmk_representative_level *levels, hmk_representatives_stats *stats);

/* The same with the edges in device memory (the context's device), through the kernels of hmk_representatives_shifted.  An index
 * >= n or a self pair is found on the device, before any array is indexed with it: HMK_ERR_BAD_ARG. */
int hmk_representatives_from_edges_dev(hmk_ctx *ctx, const void *d_edges, uint64_t n_edges, int threshold, int threshold_hi,
                                       uint32_t *covered_by, uint32_t *nearest, int32_t *nearest_score,
                                       hmk_representative_level *levels, hmk_representatives_stats *stats);

/* ---- density clustering: core, border and noise sequences ------------------------------- */

#define HMK_DENSITY_NOISE 0xFFFFFFFFu   /* cluster[i] and anchor[i] of a noise sequence */

typedef struct {
    uint64_t n_edges;             /* edges given with score >= t (every entry of the list) */
    uint32_t n_core;              /* sequences with at least min_neighbors neighbours at t */
    uint32_t n_border;            /* not core, next to a core sequence */
    uint32_t n_noise;             /* the rest: n_core + n_border + n_noise = n */
    uint32_t n_clusters;          /* connected components of the core sequences under core-core edges */
    uint32_t largest;             /* members of the largest cluster, core and border */
    uint32_t reserved;
} hmk_density_level;

typedef struct {
    uint64_t n_edges;             /* edges >= threshold */
    uint64_t pairs_scored;        /* 0 for the _from_edges forms: nothing is scored */
    uint32_t n_levels;            /* threshold_hi - threshold + 1 */
    uint32_t min_neighbors;
    uint32_t n_core, n_border, n_noise, n_clusters, largest;   /* at `threshold` */
    uint32_t reserved;
    double   kernel_ms;           /* the scoring pass, HIP events */
    double   density_ms;          /* everything behind the pass on the device, the copies included, HIP events (0 for
                                     hmk_density_from_edges) */
} hmk_density_stats;

/* Density clustering (DBSCAN on the similarity graph) of the hmk_set_sequences set at every t = threshold ... threshold_hi, from
 * ONE scoring pass at `threshold`.  The graph at t is a ~ b iff ShiftedScorer(matrix, shift_penalty, max_shift).sequenceScore >= t,
 * the graph of hmk_components_shifted.  Unlike DBSCAN proper the result does not depend on any order:
 *   degree[l][i]            the edges >= t that touch i (i itself is not counted: min_neighbors = DBSCAN's minPts - 1)
 *   core                    degree >= min_neighbors
 *   cluster[l][i]           core: the smallest core index of i's connected component in the subgraph of the core sequences
 *                           (core-core edges only); border: the cluster of its anchor; noise: HMK_DENSITY_NOISE
 *   anchor[l][i]            core: i.  Border (not core, at least one core neighbour): the core neighbour with the largest score,
 *                           among equal scores the smallest index.  Noise (everything else): HMK_DENSITY_NOISE
 *   levels[l]               l = t - threshold; the arrays are [n_levels][n], each may be NULL, levels may be NULL
 *   min_neighbors = 0       every sequence is core: cluster is `component` of hmk_components_shifted, n_clusters = n_components
 *   checks                  HMK_ERR_BAD_ARG before the device is looked at (a host-only context answers them): min_neighbors < 0,
 *                           threshold_hi < threshold, threshold_hi - threshold > 255, threshold_hi > 32767, all four outputs NULL
 *                           with n > 0, an asymmetric matrix (as hmk_components_shifted).  Then the checks of
 *                           hmk_neighbors_shifted at `threshold`.  Never HMK_ERR_CAPACITY (the call grows its own scratch).  No
 *                           sequences: HMK_OK, zeroed levels.
 * The pass is hmk_neighbors_shifted's (same plan slot, same kernels) into the context's edge buffer.  A range is dealt by the
 * kernels of hmk_greedy_sweep into one run per level with the top level first, so that the edges >= t are a prefix; a single level
 * reads the pass's segments where they lie.  As t falls, degrees, the core set and the set of core-core edges only grow: one
 * union-find and one anchor key per sequence carry over from the top level down (k_density.hip).  Per level: the level's own edges
 * add to the degrees; the sequences that turn core are marked; the link kernel reads the level's own edges and every older edge
 * with an end that turned core at this level (both ends core: union; one: an atomic maximum into the other end's anchor key);
 * labels and sizes follow.  No host synchronisation between levels; only the levels' block and the requested rows cross to the
 * host.  On a hmk_create_multi context the call runs on the root device. */
int hmk_density_shifted(hmk_ctx *ctx, int max_shift, int shift_penalty, int threshold, int threshold_hi, int min_neighbors,
                        uint32_t *cluster, uint32_t *anchor, uint32_t *degree, hmk_density_level *levels, hmk_density_stats *stats);

/* The same from packed HMK_EDGE_* edges, by hmk_components_from_edges' contract: each unordered pair once, in either orientation
 * and any order; edges below `threshold` are ignored, one above threshold_hi counts at every level (and keeps its score where
 * anchors are compared); an index >= n or a self pair is HMK_ERR_BAD_ARG.  A pair given k times counts k times towards both ends'
 * degrees (the host and the device form agree on it); for clusters and anchors repetition changes nothing else.  This is the
 * definition written plainly on the host (degrees per level by counting, a sequential union-find over the core-core edges, one pass
 * for the anchors): it works on a host-only context, and is the second implementation the device path is tested against.  No
 * symmetry check: nothing is scored. */
int hmk_density_from_edges(hmk_ctx *ctx, const uint64_t *edges, uint64_t n_edges, int threshold, int threshold_hi, int min_neighbors,
                           uint32_t *cluster, uint32_t *anchor, uint32_t *degree, hmk_density_level *levels, hmk_density_stats *stats);

/* The same with the edges in device memory (the context's device), through the kernels of hmk_density_shifted.  An index >= n or a
 * self pair is found on the device, before any array is indexed with it: HMK_ERR_BAD_ARG. */
int hmk_density_from_edges_dev(hmk_ctx *ctx, const void *d_edges, uint64_t n_edges, int threshold, int threshold_hi, int min_neighbors,
                               uint32_t *cluster, uint32_t *anchor, uint32_t *degree, hmk_density_level *levels, hmk_density_stats *stats);

/* ---- aligning given clusters around their medoids --------------------------------------- */

typedef struct {
    uint64_t pairs_scored;   /* sum over slots of s(s-1)/2, plus one pair per non-centre member of a multi-member slot */
    uint32_t n_multi;        /* slots with two or more members */
    uint32_t max_width;      /* the widest alignment of the call */
    uint32_t launches, reserved;
    double   kernel_ms;      /* device time, HIP events */
} hmk_align_stats;

/* A centre-star alignment of every given cluster in the model of the scorer that formed it: ShiftedScorer.scoreWithShift
 * (ShiftedScorer.java:48-95) is an ungapped alignment of two peptides and its result carries the shift
 * (AligningScorerResult.getShift()).  The alignment is gap-free inside a peptide and deterministic.  It is NOT the Clustal Omega
 * alignment the reference builds per cluster (ClustalRunner.java:34-66) and agrees with it only by accident.
 * Members [r0, r1) of the hmk_set_sequences set with member_cluster and n_clusters as hmk_cluster_linkage_shifted takes them.  There
 * is no threshold: nothing is thresholded.
 *   score(a, b)            ShiftedScorer(matrix, shift_penalty, max_shift).sequenceScore(seq1 = the larger index, seq2 = the smaller)
 *                          (ShiftedScorer.java:48-100): the orientation of hmk_cluster_linkage_shifted
 *   member_sum[m - r0]     the sum of score(m, b) over the other members b of m's slot; 0 in a slot of one member; may be NULL
 *   center[c]              the member of slot c with the largest member_sum (the medoid), among ties the smallest index; a slot of one
 *                          member is its own centre.  center_sum[c] is that member's sum.
 *   center_score, shift    [m - r0], for a member m other than its slot's centre z: scoreWithShift(seq1 = z, seq2 = m), getScore() /
 *                          getShift() -- exactly what hmk_score_with_shift returns for i = z, j = m: the first strict maximum in the
 *                          loop's order (:86-89) and the sign rule of :91-93.  Read through :69-77 and :91-93, residue k of m then
 *                          stands under residue k + shift of z.  For m = z: shift = 0 and center_score = INT32_MAX (no comparison is
 *                          made; the convention hmk_cluster_linkage_shifted has for a slot of one member).
 *   column[m - r0]         shift[m] - (the smallest shift in m's slot, the centre's 0 included)
 *   width[c]               the maximum over the slot's members of column + length
 *   the aligned row of m   column times '-', then the peptide, then '-' up to width.  The call builds no strings.
 *   checks                 HMK_ERR_BAD_ARG before the device is looked at (a host-only context answers them): the range and slot
 *                          checks of hmk_cluster_linkage_shifted (a slot without members is refused), a null member_cluster with a
 *                          non-empty range, a null required output, an asymmetric matrix.  Then the checks of hmk_search_shifted over
 *                          the range that do not concern a threshold: HMK_ERR_SHIFT_TOO_BIG against the shortest length, and scores
 *                          that fit int16 at both ends as hmk_cluster_linkage_shifted proves them -- which is what bounds the sums:
 *                          |member_sum| < 2^15 * 2^24 -- and n <= 2^24.  An empty range is HMK_OK with nothing written.  Never
 *                          HMK_ERR_CAPACITY.  Without a device HMK_ERR_DEVICE: there is no CPU fallback.
 * Every pair inside a slot is scored once for the sums and every non-centre member once more against its centre, and nothing else
 * (k_align.hip); the scratch is O(members + clusters), and the centres never leave the device between the kernels.  Only integer
 * adds, minima and maxima: the result does not depend on the schedule.  On a hmk_create_multi context the call runs on the root
 * device. */
int hmk_cluster_align_shifted(hmk_ctx *ctx, uint32_t r0, uint32_t r1, const uint32_t *member_cluster, uint32_t n_clusters,
                              int max_shift, int shift_penalty,
                              uint32_t *center, int64_t *center_sum, uint32_t *width,               /* n_clusters each, required */
                              int64_t *member_sum,                                                   /* r1 - r0, may be NULL */
                              int32_t *center_score, int32_t *shift, uint32_t *column,               /* r1 - r0 each, required */
                              hmk_align_stats *stats);

/* ---- the score survey of a pair space -------------------------------------------------- */

#define HMK_SURVEY_MAX_BINS 1024
typedef struct {
    uint64_t pairs_scored;    /* triangle: s(s-1)/2 for s = q1 - q0; rectangle: (q1 - q0)(r1 - r0) */
    uint64_t n_below;         /* pairs with score <  score_lo          (not in hist) */
    uint64_t n_above;         /* pairs with score >= score_lo + n_bins (not in hist) */
    uint64_t n_at_or_above;   /* pairs with score >= threshold */
    int32_t  score_min, score_max;   /* over the scored pairs; INT32_MAX / INT32_MIN when there are none */
    uint32_t launches, reserved;
    double   kernel_ms;       /* HIP events */
} hmk_survey_stats;

/* What the pair scores of a set look like, before a threshold is chosen for any other call: the histogram of the scores, every
 * sequence's best partner, every sequence's number of partners at a threshold.  The output is O(n_bins + rows) whatever the density;
 * every pair is scored once and reduced on the device (k_survey.hip), nothing proportional to the pairs is stored or copied.
 * The ranges are index ranges of the hmk_set_sequences set.
 *   triangle  [q0, q1) == [r0, r1): every unordered pair of distinct members, score = ShiftedScorer(matrix, shift_penalty,
 *             max_shift).sequenceScore(seq1 = the larger index, seq2 = the smaller) -- the orientation of hmk_cluster_linkage_shifted
 *             and of the neighbour edges.  An asymmetric matrix is HMK_ERR_BAD_ARG, as in that call.
 *   rectangle disjoint ranges: every (q, r), score = sequenceScore(seq1 = q, seq2 = r) as in hmk_search_shifted; any matrix.
 *   hist[k]              the pairs with score == score_lo + k, k < n_bins; sum(hist) + n_below + n_above == pairs_scored
 *   best_score[q - q0]   the maximum over the row's partners: in the triangle all other members (on both sides of the row), in the
 *                        rectangle the references
 *   best_index[q - q0]   the smallest partner index attaining it (an index of the uploaded set)
 *   degree[q - q0]       the partners with score >= threshold (a pair scoring exactly the threshold counts); the triangle has
 *                        sum(degree) == 2 n_at_or_above, the rectangle sum(degree) == n_at_or_above
 *                        A row without partners gets INT32_MIN, UINT32_MAX, 0.
 *   checks               HMK_ERR_BAD_ARG before the device is looked at (a host-only context answers them): ranges outside [0, n) or
 *                        overlapping in part, n_bins > HMK_SURVEY_MAX_BINS, hist == NULL with n_bins != 0 or the reverse, some but
 *                        not all of the three row pointers, hist and the row outputs all absent on a non-empty pair space,
 *                        stats == NULL, an asymmetric matrix with a triangle.  Then the checks of hmk_cluster_align_shifted over the
 *                        two ranges (none concerns the threshold, which may be any int): HMK_ERR_SHIFT_TOO_BIG against the shortest
 *                        length, scores that fit int16 at both ends, n <= 2^24.  An empty pair space (one range empty, a triangle of
 *                        one member) is HMK_OK: hist zeroed, the rows' no-partner values.  Never HMK_ERR_CAPACITY.  Without a
 *                        device HMK_ERR_DEVICE: there is no CPU fallback.
 * Only integer adds, minima and maxima: the result does not depend on the schedule, and every call clears its accumulators first.  On
 * a hmk_create_multi context the call runs on the root device. */
int hmk_score_survey_shifted(hmk_ctx *ctx, uint32_t q0, uint32_t q1, uint32_t r0, uint32_t r1,
                             int max_shift, int shift_penalty, int threshold,
                             int score_lo, uint32_t n_bins, uint64_t *hist,             /* n_bins; NULL iff n_bins == 0 */
                             int32_t *best_score, uint32_t *best_index, uint32_t *degree, /* q1 - q0 each; NULL together */
                             hmk_survey_stats *stats);

/* ---- the separation of given clusters: own cluster against the nearest other one ------------ */

typedef struct {
    uint64_t pairs_scored;   /* nm (nm - 1) for nm = r1 - r0: the ordered pairs reduced */
    uint32_t n_misplaced;    /* members with misplaced == 1 (counted whether or not misplaced is given) */
    uint32_t n_multi;        /* slots with two or more members */
    uint32_t n_segments;     /* pieces the cluster-sorted partner order was cut into (1: every walk sees whole slots only) */
    uint32_t launches, reserved;
    double   kernel_ms;      /* device time, HIP events */
} hmk_separation_stats;

/* How well separated given clusters are, and which members sit closer to another cluster than to their own: the average-linkage
 * statistic behind a silhouette.  Members [r0, r1) of the hmk_set_sequences set with member_cluster and n_clusters as
 * hmk_cluster_linkage_shifted takes them.  There is no threshold: nothing is thresholded.  Members count one each: the uploaded sizes
 * are not used.  Below, |A| is the number of members of slot A in the range.
 *   score(a, b)            ShiftedScorer(matrix, shift_penalty, max_shift).sequenceScore(seq1 = the larger index, seq2 = the smaller)
 *                          (ShiftedScorer.java:48-100): the orientation of hmk_cluster_linkage_shifted, hmk_cluster_align_shifted and
 *                          the triangle of hmk_score_survey_shifted
 *   own_sum[m - r0]        for m in slot A: the sum of score(m, b) over the other members b of A; 0 when |A| = 1.  Equal to
 *                          hmk_cluster_align_shifted's member_sum.
 *   near_cluster[m - r0]   the nearest other slot: with sum_C = the sum of score(m, b) over b in C for every slot C other than A, the
 *                          slot with the largest mean sum_C / |C|, among equal means the smallest slot index.  Means are compared
 *                          exactly, by 64-bit cross-multiplication: |sum_C| <= 2^15 |C|, two slots are disjoint and n <= 2^24, so
 *                          every product stays below 2^61.  UINT32_MAX with n_clusters == 1.
 *   near_sum[m - r0]       that slot's sum_C; 0 with n_clusters == 1
 *   misplaced[m - r0]      1 iff |A| >= 2, another slot exists and own_sum / (|A| - 1) < near_sum / |C| strictly, C the nearest
 *                          slot, decided by cross-multiplication again; else 0.  A member of a slot of one is never misplaced.  May
 *                          be NULL.
 *   cluster_misplaced[c]   the misplaced members of slot c; may be NULL
 *   cluster_own_sum[c]     the sum of own_sum over the members of slot c; may be NULL
 *   checks                 HMK_ERR_BAD_ARG before the device is looked at (a host-only context answers them): the range and slot
 *                          checks of hmk_cluster_linkage_shifted (a slot without members is refused), a null member_cluster with a
 *                          non-empty range, a null required output, stats == NULL, an asymmetric matrix.  Then the checks of
 *                          hmk_cluster_align_shifted over the range: HMK_ERR_SHIFT_TOO_BIG against the shortest length, scores that
 *                          fit int16 at both ends, n <= 2^24.  An empty range is HMK_OK with nothing written.  Never
 *                          HMK_ERR_CAPACITY.  Without a device HMK_ERR_DEVICE: there is no CPU fallback.
 * Every ordered pair of distinct members is scored once and added to a running sum per (member, slot) that is closed where the
 * cluster-sorted partner order leaves the slot (k_separation.hip); no sum per (member, slot) is ever stored: the scratch is
 * O(members x n_segments + clusters) with n_segments <= 64.  Only integer adds and comparisons, no atomics: the result does not depend
 * on the grid, the segment length or the schedule.  On a hmk_create_multi context the call runs on the root device. */
int hmk_cluster_separation_shifted(hmk_ctx *ctx, uint32_t r0, uint32_t r1, const uint32_t *member_cluster, uint32_t n_clusters,
                                   int max_shift, int shift_penalty,
                                   int64_t *own_sum, int64_t *near_sum, uint32_t *near_cluster,       /* r1 - r0 each, required */
                                   uint8_t *misplaced,                                                 /* r1 - r0, may be NULL */
                                   uint32_t *cluster_misplaced, int64_t *cluster_own_sum,              /* n_clusters each, may be NULL */
                                   hmk_separation_stats *stats);

/* ---- the profile of given clusters: column counts, information content, match states, KLD ---- */

#define HMK_PROFILE_SYMBOLS 21     /* the 20 residues in the alphabet's order, then the gap */
#define HMK_PROFILE_MAX_WIDTH 96
typedef struct {
    double  min_ic, max_gap_proportion;        /* Hammock.minIc 1.2, maxGapProportion 0.2 */
    int32_t min_conserved_positions, allow_inner_gaps;
    double  beta, sigma, scale;                /* Statistics.java:21-23: 200, 10, 2.88539 */
    double  frequency[20 * 20];                /* [observed j][scored i], as loadFrequencyMatrix (FileIOManager.java:90-118) reads a
                                                * row-normalised q_ij file: row j of the file, column i */
    double  background[20];                    /* the divisor of Statistics.java:267, per scored letter */
} hmk_profile_params;

typedef struct {
    uint64_t columns;            /* the sum of width[] over all slots: what col_capacity must hold (set with HMK_ERR_CAPACITY too) */
    uint32_t n_multi;            /* slots with two or more members */
    uint32_t omitted;            /* slots of one member, left out of the system means (Hammock.java:684-692) */
    uint32_t small_members;      /* members counted by the form for small slots (a lane per member) */
    uint32_t large_chunks;       /* chunks of the form for large slots (one workgroup step each) */
    uint32_t launches, reserved;
    double   system_kld_match;   /* Statistics.getMeanSystemKld(paths, false), Hammock.java:694; NaN (0.0 / 0) without a multi-member slot */
    double   system_kld_all;     /* ... (paths, true), :695 */
    double   kernel_ms;          /* device time, HIP events */
} hmk_profile_stats;

/* What the reference reads from a cluster's alignment, for every given cluster at once.  Members [r0, r1) of the hmk_set_sequences
 * set with member_cluster and n_clusters as hmk_cluster_linkage_shifted takes them.  The call takes a placement, not a scorer:
 * column[m - r0] is where member m's first residue stands in its slot's alignment -- what hmk_cluster_align_shifted returns, or any
 * ungapped placement of the caller's.  Below, slot c has s members.
 *   rows                   the aligned row of m is column gaps, then the peptide, then gaps up to width[c]
 *   width[c]               the maximum over the slot's members of column + length
 *   col_start[c]           where slot c's columns begin in the per-column arrays; col_start[n_clusters] = stats->columns
 *   counts[col][sym]       the rows of the slot with symbol sym in that column (FileIOManager.getPositionLetterCounts, :1221-1247);
 *                          HMK_PROFILE_SYMBOLS words per column, the gap is symbol 20.  May be NULL.
 *   ic[col]                FileIOManager.getInformationContents (:1195-1211): -1.0 unless (gaps + 0.0) / s <= max_gap_proportion
 *                          (:1204), else getInformationContent (:1421-1439): -(log(0.05) / log(2)) + the sum over the non-gap symbols
 *                          present of p * (log(p) / log(2)), p = count / (s - gaps), the sum in symbol order.  May be NULL.
 *   col_flags[col]         bit 0, conserved: ic >= min_ic (:1271, :1281).  Bit 1, match state (defineMatchStates, :1265-1300): bit 0
 *                          if allow_inner_gaps, else every column from the slot's first to its last conserved one (:1277-1297).  May
 *                          be NULL.
 *   n_conserved, n_match   [c] the columns of the slot with bit 0 / with bit 1
 *   passes[c]              n_conserved >= min_conserved_positions (checkConservedStates, :1172-1181, which always counts with inner
 *                          gaps allowed; used at Hammock.java:1683)
 *   kld_all, kld_match     [m - r0] Statistics.getPeptideKld (:238-273) of m's row against its own slot's counts, over all columns
 *                          and over the match-state columns only.  Per column, left to right: skipped where m has a gap (:249-252);
 *                          m's own letter is taken out of the counts (:253-254); sum = s - 1 (:258-261); skipped if what remains is
 *                          only gaps (:262-265); else with a = m's letter, fj = count_j / sum over the 20 residues (the gaps stay
 *                          inside sum, :277-280, :285), g = the sum in symbol order of fj * frequency[j][a] (:283-289),
 *                          fi = count_a / sum (0 where m was the only one: the letter lives on the pseudocount alone),
 *                          Q = ((sum - 1) * fi + beta * g) / ((sum - 1) + beta) (:296), and the column adds
 *                          log(Q / background[a]) * (sum / (sum + sigma)) * scale (:267-269).  0.0 for the member of a slot of one.
 *   kld_match_mean[c], kld_all_mean[c]
 *                          the slot's sum in member index order / s (getMeanClusterKld, :194-197); 0.0 for a slot of one
 *   stats->system_kld_*    the sum over the members of multi-member slots, in member index order, / their number
 *                          (getMeanSystemKld, :178-184, over the paths of Hammock.java:684-692); stats->omitted counts the slots of
 *                          one member left out
 *   summation order        symbols in symbol order, columns left to right, members in index order.  This is not the iteration order
 *                          of the JVM's HashMap and no bit parity with the Java's doubles is claimed.  The device functions are
 *                          compiled without contraction: the operations are the ones written above.
 *   the decision           ic >= min_ic is made once, on the device; col_flags, n_conserved, n_match, passes and kld_match all
 *                          follow that one decision.  It can be a tie in exact arithmetic: ten members, one letter twice and eight
 *                          letters once, have log2 20 - 0.2 log2 5 - 0.8 log2 10 = 1.2 exactly, the reference's default minIc; which
 *                          side the doubles fall on is rounding (and, in the Java, map order).
 *   determinism            counts are integer sums; ic is computed by one lane per column, a member's KLDs by one lane in column
 *                          order: every output is bit-identical between calls and between grids.
 *   checks                 HMK_ERR_BAD_ARG before the device is looked at (a host-only context answers them): the range and slot
 *                          checks of hmk_cluster_linkage_shifted (a slot without members is refused), a null member_cluster or column
 *                          with a non-empty range, a null required output, params or stats, column + length > HMK_PROFILE_MAX_WIDTH,
 *                          a non-finite min_ic, max_gap_proportion outside [0, 1], negative min_conserved_positions, and beta, sigma,
 *                          scale, any frequency or background entry that is not finite and > 0.  Then
 *                          HMK_ERR_REFERENCE_WOULD_CRASH for a residue code >= 20 (B, Z, X, *) in the range: frequencyMatrix.get()
 *                          is null for it at Statistics.java:286.  Then HMK_ERR_CAPACITY with stats->columns set when col_capacity
 *                          < the sum of the widths.  An empty range is HMK_OK: col_start[0] = 0, nothing else written.  Without a
 *                          device HMK_ERR_DEVICE: there is no CPU fallback.
 * hmk_cluster_align_shifted cannot produce a width above HMK_PROFILE_MAX_WIDTH: the shift loop of scoreWithShift runs over
 * [-max_shift, max_shift + diff] with max_shift < the shorter length, so a shift lies in [-31, 31], column <= 62 and width <= 94.
 * Scratch is O(members + columns); the masks never leave the device between the kernels (k_profile.hip).  On a hmk_create_multi
 * context the call runs on the root device. */
int hmk_cluster_profile(hmk_ctx *ctx, uint32_t r0, uint32_t r1, const uint32_t *member_cluster, uint32_t n_clusters,
                        const uint32_t *column,                                                         /* r1 - r0 */
                        const hmk_profile_params *params,
                        uint32_t *width, uint32_t *n_conserved, uint32_t *n_match, uint8_t *passes,     /* n_clusters each, required */
                        double *kld_match_mean, double *kld_all_mean,                                   /* n_clusters each, required */
                        uint64_t *col_start,                                                            /* n_clusters + 1, required */
                        uint64_t col_capacity,                                                          /* columns the next three hold */
                        uint32_t *counts,                                                               /* x HMK_PROFILE_SYMBOLS, may be NULL */
                        double *ic, uint8_t *col_flags,                                                 /* may be NULL */
                        double *kld_match, double *kld_all,                                             /* r1 - r0 each, required */
                        hmk_profile_stats *stats);

/* ---- scanning peptides along long targets ----------------------------------------- */

/* A second resident set: the TARGETS, sequences longer than any peptide the library takes (an antigen, a proteome), which the
 * sequences of hmk_set_sequences are scanned along (hmk_scan_shifted).  Residues concatenated in the alphabet's codes 0..23,
 * offsets[n_targets + 1]; everything is copied.  Targets and sequences are independent: either call may come first, neither
 * disturbs the other; the next call replaces the targets, n_targets = 0 clears them.  A host-only context stores them and
 * answers the checks.  HMK_ERR_BAD_ARG for: a target length outside [HMK_MAX_LEN + 1, HMK_TARGET_MAX_LEN] (a target is by
 * definition the longer sequence, so seq1 = peptide is always the shorter one and the equal-length role swap of
 * ShiftedScorer.java:51-57 cannot occur; shorter "targets" are sequences, hmk_search_shifted serves them), a residue code
 * >= 24, offsets that do not start at 0 or do not ascend, more than 2^31 - 1 residues in all, a null pointer with
 * n_targets > 0.  On a hmk_create_multi context the targets live on the root device. */
#define HMK_TARGET_MAX_LEN (1u << 20)
int hmk_set_targets(hmk_ctx *ctx, const uint8_t *residues, const uint64_t *offsets, uint32_t n_targets);

typedef struct { uint32_t query, target; int32_t score, offset; } hmk_scan_hit;   /* 16 bytes */
typedef struct {
    uint64_t n_hits;            /* records returned (or needed, with HMK_ERR_CAPACITY) */
    uint64_t windows_scored;    /* sum over (q, t) of d + 2X + 1 */
    uint64_t window_hits;       /* windows at or above the threshold, before any reduction per pair */
    uint64_t windows_packed;    /* of windows_scored: scored by the byte-lane form */
    uint64_t windows_literal;   /* ... by the plain int32 form */
    uint32_t n_tiles, launches;
    double   kernel_ms;         /* HIP events, scoring (a pass repeated into a larger scratch included) + reduction + coverage */
} hmk_scan_stats;

#define HMK_SCAN_ALL_WINDOWS 1u
/* Where do the peptides sit on the targets?  Queries [q0, q1) of the hmk_set_sequences set slide along targets [t0, t1) of the
 * hmk_set_targets set as ShiftedScorer(matrix, shift_penalty, max_shift).scoreWithShift(seq1 = query, seq2 = target) slides
 * them (ShiftedScorer.java:48-95).  With m, n the two lengths, d = n - m, X = max_shift, p = shift_penalty, the WINDOW SCORE
 * w(q, t, s) of every offset s in [-X, d + X] (:67) is the sum of the cells M[q[i]][t[i + s]] over the overlap (:69-77; the
 * matrix index is [peptide residue][target residue]) + d p (:79) + 2 p (-s) for s < 0 (:80-82) or 2 p (s - d) for s > d
 * (:83-85).  `offset` = s is where the peptide's residue 0 stands on the target (negative: it hangs over the start);
 * AligningScorerResult.getShift() is -offset (:91-93).
 *   flags = 0              pair mode, the reference's sequenceScore: one record per pair (q, t) whose best window reaches the
 *                          threshold, with that maximum and the SMALLEST s attaining it (the first strict maximum, :86-89).
 *                          The window hits never reach the host.
 *   HMK_SCAN_ALL_WINDOWS   window mode: one record per (q, t, s) with w >= threshold; repeats on a target show as several.
 *   hits, capacity         record order unspecified.  HMK_ERR_CAPACITY with stats->n_hits = the number needed when `capacity`
 *                          is too small; the call grows its own device scratch.
 *   coverage_count, coverage_size   may be NULL; per residue position of the targets [t0, t1), indexed offsets[t] - offsets[t0]
 *                          + position: the number of returned records (of the call's mode) whose window covers the position
 *                          (positions max(s, 0) .. min(s + m, n) - 1), and the sum of those records' peptides' sizes as
 *                          uploaded (UniqueSequence.size(); 1 each without sizes), in 64 bits.  Summed on the device.
 *   checks                 answered before the device is looked at (a host-only context answers them): HMK_ERR_BAD_ARG for a
 *                          null stats, null hits with capacity > 0, unknown flag bits, max_shift < 0, a threshold outside
 *                          [-30000, 30000], |p| (HMK_TARGET_MAX_LEN + 2X) + 32 max|M| not below 2^30; HMK_ERR_NO_SEQUENCES
 *                          without a sequence set, or without targets when t1 > t0; HMK_ERR_BAD_ARG for ranges outside the two
 *                          sets; HMK_ERR_SHIFT_TOO_BIG when max_shift >= the shortest length in [q0, q1) (:59-62).  An empty
 *                          range on either side: HMK_OK, 0 records, zeroed coverage.  Then, without a device, HMK_ERR_DEVICE.
 *   stats                  the counters above; windows_packed + windows_literal = windows_scored.  Two bit-exact kernels score:
 *                          byte lanes (peptide lengths 6..20, max_shift <= 5, where the lane-range proof holds for the group
 *                          of peptides and the target's length) and plain int32 sums (everything else).
 * On a hmk_create_multi context the scan runs on the root device. */
int hmk_scan_shifted(hmk_ctx *ctx, uint32_t q0, uint32_t q1, uint32_t t0, uint32_t t1,
                     int max_shift, int shift_penalty, int threshold, uint32_t flags,
                     hmk_scan_hit *hits, uint64_t capacity,
                     uint32_t *coverage_count, uint64_t *coverage_size,   /* per residue of targets [t0, t1), may be NULL */
                     hmk_scan_stats *stats);

/* Where the time of the last hmk_greedy_cluster / hmk_greedy_from_edges_dev call of this context went
 * (milliseconds; the span of Hammock.java:406-411 minus the sort).  score_ms and csr_ms are device times (HIP events on
 * the call's stream), the others host wall time.  The parts overlap (phase 1 runs while the rest of the pair space is
 * being scored), so they do not add up to total_ms. */
typedef struct {
    double plan_ms;          /* tiling plan (cached between calls with the same parameters) */
    double score_ms;         /* neighbour kernels, first launch to last edge */
    double csr_ms;           /* edge segments -> CSR adjacency on the device */
    double wait_rows_ms;     /* host waiting for adjacency rows (band hand-over, later fetches) */
    double phase1_ms;        /* firstPhase, LimitedGreedySequenceClusterer.java:77-120 (includes wait_rows_ms) */
    double precheck_ms;      /* device pre-check of the second loop (:59-66) incl. copies */
    double exchange_ms;      /* multi-device calls: routing the edges to the devices that own their rows, until the last block has landed */
    double device_loop_ms;   /* the second loop on the device in optimistic rounds (large inputs), incl. copies */
    double host_precheck_ms; /* host wall time between the end of phase 1 and the sequential part: the wait for the full CSR, the
                              * pre-check and the device-side loop (includes precheck_ms and device_loop_ms) */
    double sequential_ms;    /* the order-dependent loop :59-66 itself */
    double total_ms;
    uint64_t cand_entries;   /* (leftover, feasible cluster) pairs after phase 1 */
    uint64_t band_bytes;     /* bytes of the band, as prepared for phase 1, that crossed PCIe (0: the band went as whole rows, or not at all) */
    uint64_t loop_rounds;    /* rounds of the device-side second loop, 0 if the loop ran on the host */
} hmk_greedy_phases;
int hmk_greedy_last_phases(const hmk_ctx *ctx, hmk_greedy_phases *out);

#ifdef __cplusplus
}
#endif
#endif /* HAMMOCK_HIP_H */
