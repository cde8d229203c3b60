"""The rectangle and triangle plans (build_plan_rect, hmk_plan.cpp: build_plan_search / build_plan_triangle, and build_plan_local_search)
tested as hard as the all-vs-all planner is in test_gpu_parity.py.  Everything is integer and bit-exact: every comparison is
np.array_equal on sorted packed edges or on (index, score) tables against oracle.c_oracle.

Two observation points return the COMPLETE edge set of a plan:
  rectangle  Context.search_shifted / search_local: rows = queries, columns = references of the oracle block, every edge m = query;
  triangle   Context.cluster_pairs_shifted(r0, r1, member_cluster = arange(nm), n_clusters = nm): with one member per slot the
             complete-linkage score of a slot pair is the pair's score, so the result is {(a, b, score(a, b)): a < b, score >= thr}
             in slot numbers; last_merge_stats.pairs_scored / n_edges come straight from the plan and the pass.

A rectangle plan has no row-bound refinement, so which lane tier a (row length, column length) class runs follows from classify's
closed rule alone; lane_path() restates it and the tests assert the tier that ran (NeighborStats.classes_*).  MergeStats carries
no class counts: a triangle is checked by its edge set and its three counts.

The CPU tests (the tier coverage of the sweep's seed, the hit-count facts of the best-k recipe, the predicate's table) run
anywhere; the GPU tests need an MI355X (-m gpu).  tests/tools/fuzz_rect.py runs the sweep for as many trials as asked."""
import numpy as np
import pytest

from conftest import random_peptides
from lane_model import java_round, lane_path

import hammock_amd
from hammock_amd.synth import synth_peptides
import test_assign
import test_continue
import test_match
from test_search import asymmetric, numpy_best

LONG_RUN = 4096          # k_search.hip: longer runs of one query's hits take the workgroup-per-query selection
FIRST_EDGE_BUFFER = 1 << 20   # neighbors_grow's first edge buffer (entries)


@pytest.fixture(scope="module")
def gpu():
    """skips the GPU tests where no HIP device is visible"""
    try:
        import torch
        ok = torch.cuda.is_available()
    except Exception:
        ok = False
    if not ok:
        pytest.skip("needs an MI355X (no HIP device visible)")
    return 0


# ---- matrices, sequences, the predicate ------------------------------------------------------------------------------------------

def matrix_named(matrices, name):
    """blosum62 | clip14 = np.clip(blosum62, -1, 4) (symmetric; 8-bit lanes fit every length 6..20 at the reference's defaults);
    either with the suffix _asym: the +-2 perturbation of test_search.py::asymmetric"""
    base, _, asym = name.partition("_")
    M = np.asarray(matrices["blosum62"], dtype=np.int32)
    if base == "clip14":
        M = np.clip(M, -1, 4).astype(np.int32)
    else:
        assert base == "blosum62"
    return asymmetric(M) if asym else M.copy()


def predicted_tiers(M, lens_q, lens_r, X, p, thr):
    """the classes of a rectangle -- one per (query length, reference length) present -- by the tier the predicate gives them"""
    out = {"u8": 0, "u16": 0, "direct": 0}
    for lq in np.unique(lens_q):
        for lr in np.unique(lens_r):
            out[lane_path(M, int(lq), int(lr), X, p, thr)] += 1
    return out


def predicted_u8_rows_first(M, lens_q, lens_r, X, p, thr):
    """the 8-bit classes whose reference is at least as long as the query: under an asymmetric matrix the rows are the references,
    and only these may run a row-packed kernel"""
    return sum(lane_path(M, int(lq), int(lr), X, p, thr) == "u8" for lq in np.unique(lens_q) for lr in np.unique(lens_r) if lr >= lq)


def peptides(rng, n, lo, hi, related=0.25):
    """n DISTINCT peptides of lengths lo..hi in random order.  A share of them are 1-2-substitution mutants of the others, some a
    residue shorter or longer: hits exist at every threshold, under every matrix and across length classes"""
    base = random_peptides(rng, n - int(n * related), lo, hi)
    seen = {q.tobytes() for q in base}
    out = list(base)
    while len(out) < n:
        q = base[int(rng.integers(len(base)))].copy()
        k = min(int(rng.integers(1, 3)), len(q))
        q[rng.choice(len(q), k, replace=False)] = rng.integers(0, 20, k)
        r = rng.random()
        if r < 0.25 and len(q) > lo:
            q = q[1:] if rng.random() < 0.5 else q[:-1]
        elif r < 0.5 and len(q) < hi:
            q = np.append(q, rng.integers(0, 20)).astype(np.uint8)
        if q.tobytes() in seen:
            continue
        seen.add(q.tobytes())
        out.append(q)
    return [out[k] for k in rng.permutation(n)]


def ctx_with(M, seqs, sizes=None):
    ctx = hammock_amd.Context(M, device=0)
    res, off = hammock_amd.pack_sequences(seqs)
    ctx.set_sequences(residues=res, offsets=off, sizes=sizes)
    return ctx, res, off


def lengths(off, rng_):
    return np.diff(np.asarray(off, dtype=np.int64))[rng_[0]:rng_[1]]


# ---- expectations ---------------------------------------------------------------------------------------------------------------

def block_of(coracle, M, res, off, q, r, scorer, a, b):
    """[nq, nr] of score(seq1 = query, seq2 = reference), as test_search.py::oracle_hits builds it"""
    st, blk = coracle.score_block(M, res, off, np.arange(*q), np.arange(*r), scorer, a, b)
    assert st == 0
    return blk


def rect_hits(blk, q, r, thr):
    """the sorted packed edges of the block: m = query, x = reference"""
    qi, ri = np.nonzero(blk >= thr)
    return np.sort(hammock_amd.pack_edges(r[0] + ri, q[0] + qi, blk[qi, ri]))


def triangle_hits(blk, thr):
    """{(a, b, score): a < b, score >= thr} of a square block, in slot numbers"""
    a, b = np.nonzero(np.triu(blk >= thr, 1))
    return np.sort(hammock_amd.pack_edges(a, b, blk[a, b]))


def check_search(ctx, blk, q, r, X, p, thr, what):
    edges, st = ctx.search_shifted(*q, *r, X, p, thr)
    want = rect_hits(blk, q, r, thr)
    assert st.pairs_scored == (q[1] - q[0]) * (r[1] - r[0]), what
    assert st.n_edges == len(want), (what, st.n_edges, len(want))
    assert np.array_equal(np.sort(edges), want), (what, len(edges), len(want), st.classes_u8, st.classes_u16, st.classes_direct,
                                                  st.classes_rows)
    return st, want


def check_best(ctx, blk, q, r, X, p, thr, k, what):
    idx, sc = ctx.search_best_shifted(*q, *r, X, p, thr, k)
    widx, wsc = numpy_best(blk, np.arange(*r), thr, k)
    assert np.array_equal(idx, widx) and np.array_equal(sc, wsc), what
    return widx


def check_triangle(ctx, blk, r0, r1, X, p, thr, what):
    """blk: the square oracle block of [r0, r1) under a symmetric matrix"""
    nm = r1 - r0
    want = triangle_hits(blk, thr)
    got = ctx.cluster_pairs_shifted(r0, r1, np.arange(nm), nm, X, p, thr)
    ms = ctx.last_merge_stats
    assert ms.pairs_scored == nm * (nm - 1) // 2, what
    assert ms.n_edges == len(want), (what, ms.n_edges, len(want))
    assert ms.cluster_pairs == len(want), (what, ms.cluster_pairs, len(want))
    assert np.array_equal(np.sort(got), want), (what, len(got), len(want))
    return want


def assert_tier(st, M, la, lb, X, p, thr, what):
    """a one-class rectangle: the tier the predicate gives it is the one that ran"""
    if lane_path(M, la, lb, X, p, thr) == "u8":
        assert st.classes_rows == 1 and st.classes_u8 == 1, (what, st.classes_rows, st.classes_u8, st.classes_u16, st.classes_direct)
    else:
        assert st.classes_rows == 0 and st.classes_u16 + st.classes_direct == 1 and st.classes_u8 == 0, (
            what, st.classes_rows, st.classes_u8, st.classes_u16, st.classes_direct)


# ---- (a) uniform lengths 6..20 at the reference's defaults ---------------------------------------------------------------------------

# Primes: no multiple of any rows-per-tile, nor of 256 columns.  At one length the side with more sequences supplies the rows, so
# the SMALLER side is the columns: above 1,024 (where cols_per_tile bottoms out for plans this small) a class has two column runs.
UNIFORM_A, UNIFORM_B = 3001, 1237
UNIFORM_TRI = (211, 211 + 1511)   # the triangle's sub-range: r0 > 0, 1,511 members (two column runs for the first chunks)


def uniform_defaults(L):
    return min(java_round(L / 4), L - 1), java_round(1.7 * L), java_round(0.4 * L)


def test_lane_predicate_at_the_reference_defaults(matrices):
    """What case (a) relies on: without a row bound BLOSUM62 keeps 8-bit lanes up to L = 13 at round(1.7 L) and up to L = 12 at
    round(0.4 L) -- no rectangle under BLOSUM62 at the defaults reaches the X = 4 and X = 5 exact shapes -- and
    np.clip(blosum62, -1, 4) keeps them for every L in 6..20 at both thresholds: all 15 exact shapes."""
    b62, c14 = matrix_named(matrices, "blosum62"), matrix_named(matrices, "clip14")
    assert (c14 == c14.T).all()
    for L in range(6, 21):
        X, hi, lo = uniform_defaults(L)
        assert (lane_path(b62, L, L, X, 0, hi) == "u8") == (L <= 13), L
        assert (lane_path(b62, L, L, X, 0, lo) == "u8") == (L <= 12), L
        assert lane_path(b62, L, L, X, 0, hi) in ("u8", "u16") and lane_path(b62, L, L, X, 0, lo) in ("u8", "u16")
        assert lane_path(c14, L, L, X, 0, hi) == "u8" and lane_path(c14, L, L, X, 0, lo) == "u8", L
    assert sorted({uniform_defaults(L)[0] for L in range(6, 21)}) == [2, 3, 4, 5]


@pytest.mark.gpu
@pytest.mark.parametrize("mat", ["blosum62", "clip14"])
@pytest.mark.parametrize("L", list(range(6, 21)))
def test_rect_uniform_lengths_at_the_reference_defaults(gpu, matrices, coracle, L, mat):
    """Every uniform length 6..20 at X = round(L / 4) and thresholds round(1.7 L) / round(0.4 L), as a rectangle in two layouts
    (more queries than references and in front of them: the queries are the rows; fewer and behind them: the references are)
    and as a triangle over a sub-range: the tier the predicate names ran, and the edge sets equal the oracle's."""
    M = matrix_named(matrices, mat)
    X, thr_hi, thr_lo = uniform_defaults(L)
    rng = np.random.default_rng(1000 + L)
    seqs = peptides(rng, UNIFORM_A + UNIFORM_B, L, L)
    ctx, res, off = ctx_with(M, seqs)
    A, B = (0, UNIFORM_A), (UNIFORM_A, UNIFORM_A + UNIFORM_B)
    for q, r in ((A, B), (B, A)):
        blk = block_of(coracle, M, res, off, q, r, 0, X, 0)
        for thr in (thr_hi, thr_lo):
            what = (L, mat, q, r, X, thr)
            st, want = check_search(ctx, blk, q, r, X, 0, thr, what)
            assert_tier(st, M, L, L, X, 0, thr, what)
            assert len(want) > 0, what
        if mat == "blosum62":
            assert len(want) > 0.05 * UNIFORM_A * UNIFORM_B     # the low threshold really is dense
    t0, t1 = UNIFORM_TRI
    blk = block_of(coracle, M, res, off, (t0, t1), (t0, t1), 0, X, 0)
    for thr in (thr_hi, thr_lo):
        assert len(check_triangle(ctx, blk, t0, t1, X, 0, thr, (L, mat, "triangle", X, thr))) > 0


# ---- (b) mixed lengths at every max shift 1..5 -----------------------------------------------------------------------------------------

# (len lo, len hi, X, p, thr): the rows of test_gpu_parity.py::test_neighbors_mixed_lengths_other_shifts and an X = 3 row over 7..20
MIXED = [(6, 12, 2, -1, 14), (10, 20, 4, -1, 25), (13, 20, 5, 0, 30), (4, 9, 1, 0, 10), (7, 20, 3, -1, 23)]
MIXED_IDS = [f"len{lo}-{hi}_X{X}_p{p}_thr{thr}" for lo, hi, X, p, thr in MIXED]
MIXED_A, MIXED_B = 2203, 1409
MIXED_TRI = (307, 307 + 1201)
# Coverage guard, not a measurement: classes_rows of a first run on the final build, the same in both orientations (the
# all-vs-all test's floors do not carry over: that planner refines with row bounds, this one does not).  (matrix, X) -> floor.
MIXED_ROWS_FLOOR = {("blosum62", 1): 34, ("blosum62", 2): 49, ("blosum62", 3): 153, ("blosum62", 4): 76, ("blosum62", 5): 18,
                    ("clip14", 1): 34, ("clip14", 2): 49, ("clip14", 3): 196, ("clip14", 4): 115, ("clip14", 5): 52}


@pytest.mark.gpu
@pytest.mark.parametrize("mat", ["blosum62", "clip14"])
@pytest.mark.parametrize("case", MIXED, ids=MIXED_IDS)
def test_rect_mixed_lengths_every_shift(gpu, matrices, coracle, case, mat):
    """Mixed lengths at max shifts 1..5: the rectangle in both orientations and the triangle.  The row-packed classes are at
    least the recorded floor (under the clipped matrix at least one at every max shift) and at most the classes the predicate
    calls 8-bit."""
    lo, hi, X, p, thr = case
    M = matrix_named(matrices, mat)
    rng = np.random.default_rng(2000 + 10 * X + lo)
    seqs = peptides(rng, MIXED_A + MIXED_B, lo, hi)
    ctx, res, off = ctx_with(M, seqs)
    A, B = (0, MIXED_A), (MIXED_A, MIXED_A + MIXED_B)
    floor = MIXED_ROWS_FLOOR[(mat, X)]
    if mat == "clip14":
        assert floor >= 1
    for q, r in ((A, B), (B, A)):
        blk = block_of(coracle, M, res, off, q, r, 0, X, p)
        st, want = check_search(ctx, blk, q, r, X, p, thr, (case, mat, q, r))
        assert len(want) > 0
        tiers = predicted_tiers(M, lengths(off, q), lengths(off, r), X, p, thr)
        print(f"rect-mixed {mat} {case} q={q}: classes_rows={st.classes_rows} u8={st.classes_u8} u16={st.classes_u16} "
              f"direct={st.classes_direct} predicted={tiers}")
        assert (st.classes_u8, st.classes_u16, st.classes_direct) == (tiers["u8"], tiers["u16"], tiers["direct"]), (case, mat, q)
        assert floor <= st.classes_rows <= tiers["u8"], (case, mat, q, st.classes_rows, floor, tiers)
    t0, t1 = MIXED_TRI
    blk = block_of(coracle, M, res, off, (t0, t1), (t0, t1), 0, X, p)
    assert len(check_triangle(ctx, blk, t0, t1, X, p, thr, (case, mat, "triangle"))) > 0


# ---- (c) the same under an asymmetric matrix ---------------------------------------------------------------------------------------------

# as MIXED_ROWS_FLOOR: classes_rows of a first run on the final build, the same in both range orders
MIXED_ROWS_FLOOR_ASYM = {("blosum62_asym", 1): 20, ("blosum62_asym", 2): 28, ("blosum62_asym", 3): 80, ("blosum62_asym", 4): 40,
                         ("blosum62_asym", 5): 10, ("clip14_asym", 1): 20, ("clip14_asym", 2): 28, ("clip14_asym", 3): 105,
                         ("clip14_asym", 4): 63, ("clip14_asym", 5): 30}


@pytest.mark.gpu
@pytest.mark.parametrize("mat", ["blosum62_asym", "clip14_asym"])
@pytest.mark.parametrize("case", MIXED, ids=MIXED_IDS)
def test_rect_mixed_lengths_asymmetric(gpu, matrices, coracle, case, mat):
    """Rows are always the references; classes with row length < column length run the shift-packed or literal tier, so the
    row-packed classes are at most the 8-bit classes with reference length >= query length, and at least the recorded floor.
    Both range orders; the triangle refuses the matrix."""
    lo, hi, X, p, thr = case
    M = matrix_named(matrices, mat)
    assert not (M == M.T).all()
    rng = np.random.default_rng(3000 + 10 * X + lo)
    seqs = peptides(rng, MIXED_A + MIXED_B, lo, hi)
    ctx, res, off = ctx_with(M, seqs)
    A, B = (0, MIXED_A), (MIXED_A, MIXED_A + MIXED_B)
    floor = MIXED_ROWS_FLOOR_ASYM[(mat, X)]
    assert floor >= 1      # no silent fall-back of a whole asymmetric rectangle to the shift-packed tier
    for q, r in ((A, B), (B, A)):
        lq, lr = lengths(off, q), lengths(off, r)
        assert lr.max() >= lq.min() and lr.min() < lq.max()   # classes with row (reference) length >= column length, and with less
        blk = block_of(coracle, M, res, off, q, r, 0, X, p)
        st, want = check_search(ctx, blk, q, r, X, p, thr, (case, mat, q, r))
        assert st.symmetric == 0 and len(want) > 0
        swapped = block_of(coracle, M, res, off, r, q, 0, X, p).T
        assert not np.array_equal(rect_hits(swapped, q, r, thr), want)   # the orientation matters for this input
        tiers = predicted_tiers(M, lq, lr, X, p, thr)
        assert (st.classes_u8, st.classes_u16, st.classes_direct) == (tiers["u8"], tiers["u16"], tiers["direct"]), (case, mat, q)
        cap = predicted_u8_rows_first(M, lq, lr, X, p, thr)
        print(f"rect-asym {mat} {case} q={q}: classes_rows={st.classes_rows} u8 with lr >= lq={cap}")
        assert floor <= st.classes_rows <= cap, (case, mat, q, st.classes_rows, floor, cap)
    with pytest.raises(ValueError, match="symmetric"):
        ctx.cluster_pairs_shifted(MIXED_TRI[0], MIXED_TRI[1], np.arange(MIXED_TRI[1] - MIXED_TRI[0]), MIXED_TRI[1] - MIXED_TRI[0], X, p, thr)


@pytest.mark.gpu
@pytest.mark.parametrize("new_first", [True, False])
def test_rect_assign_asymmetric_mixed_lengths(gpu, matrices, coracle, new_first):
    """assign_shifted builds its plan with the two ranges swapped: the opposite orientation of the search's, on the X = 3 row"""
    lo, hi, X, p, thr = MIXED[4]
    M = matrix_named(matrices, "blosum62_asym")
    rng = np.random.default_rng(3100)
    members, mc, new = test_assign.families(rng, 1409, 1103, lo + 1, hi, trim=True)   # (trim: down to lo)
    mc = test_assign.relabel(mc)
    ctx, res, off, qr, rr, ids, msz = test_assign.setup(M, new, members, mc, rng, new_first)
    lq, lr = lengths(off, qr), lengths(off, rr)
    assert lr.max() >= lq.min() and lr.min() < lq.max() and min(lq.min(), lr.min()) > X
    blk = test_assign.block(coracle, M, res, off, qr, rr, 0, X, p)
    want = test_assign.expected(blk, mc, ids, msz, thr, 4)
    assert (want[2] > 0).any() and (want[2] == 0).any()
    test_assign.check(ctx.assign_shifted(*qr, *rr, mc, ids, X, p, thr, 4), want)
    st = ctx.last_assign_stats
    assert st.symmetric == 0 and st.pairs_scored == len(new) * len(members) and st.n_edges == int((blk >= thr).sum())


def test_triangle_refuses_an_asymmetric_matrix_before_the_device(matrices):
    ctx = hammock_amd.Context(matrix_named(matrices, "blosum62_asym"), device=-1)
    ctx.set_sequences(["ACDEFGHIK", "ACDEFGHIKL", "MNPQRSTVW", "WYVACDEFG"])
    with pytest.raises(ValueError, match="symmetric"):
        ctx.cluster_pairs_shifted(1, 4, np.arange(3), 3, 2, 0, 10)


# ---- (d) HMK_NO_ROWS_KERNEL -------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("mat,lo,hi", [("blosum62", 7, 7), ("blosum62", 12, 12), ("clip14", 20, 20), ("blosum62", 7, 20)],
                         ids=["blosum62_L7", "blosum62_L12", "clip14_L20", "blosum62_mixed7-20"])
def test_rect_no_rows_kernel_switch_rebuilds_the_plan(gpu, matrices, coracle, monkeypatch, mat, lo, hi):
    """HMK_NO_ROWS_KERNEL=1: no class runs a row-packed kernel and the edges are the oracle's; cleared on the same context, the
    plan (whose cache key carries the switch) is rebuilt with the row-packed classes back, and the edges are equal again."""
    M = matrix_named(matrices, mat)
    if lo == hi:
        X, thr, _ = uniform_defaults(lo)
        p = 0
    else:
        _, _, X, p, thr = MIXED[4]
    rng = np.random.default_rng(4000 + lo + hi)
    nA, nB = 1409, 1103
    seqs = peptides(rng, nA + nB, lo, hi)
    ctx, res, off = ctx_with(M, seqs)
    layouts = [((0, nA), (nA, nA + nB)), ((nA, nA + nB), (0, nA))]
    blks = [block_of(coracle, M, res, off, q, r, 0, X, p) for q, r in layouts]
    tri = (101, 101 + 907)
    tblk = block_of(coracle, M, res, off, tri, tri, 0, X, p)
    for (q, r), blk in zip(layouts, blks):
        monkeypatch.setenv("HMK_NO_ROWS_KERNEL", "1")
        st, want = check_search(ctx, blk, q, r, X, p, thr, (mat, lo, hi, q, "no rows kernel"))
        assert st.classes_rows == 0 and st.classes_u8 >= 1 and len(want) > 0
        check_triangle(ctx, tblk, *tri, X, p, thr, (mat, lo, hi, "triangle, no rows kernel"))
        monkeypatch.delenv("HMK_NO_ROWS_KERNEL")
        st, _ = check_search(ctx, blk, q, r, X, p, thr, (mat, lo, hi, q, "rows kernel back"))
        assert st.classes_rows >= 1
        check_triangle(ctx, tblk, *tri, X, p, thr, (mat, lo, hi, "triangle, rows kernel back"))


# ---- (e) randomised sweep ------------------------------------------------------------------------------------------------------------------

SWEEP_SEED, SWEEP_TRIALS = 2025, 48


def sweep_trial(rng, trial, matrices, coracle):
    """One trial's parameters: the generator of test_gpu_parity.py::test_neighbors_fuzz_lane_classification (matrix kinds shipped /
    random symmetric / asymmetric / extreme +-120; lengths lo in 1..13, hi <= 32; X below the shortest length and <= 8; p in -6..2;
    the threshold at a random quantile of 4,000 oracle-scored pairs) plus a split of the set into queries and references at a
    random point in a random range order -- every third trial two ranges that do not touch and do not start at 0 --, k of the
    best-k selection by trial and the gap penalties of the every-fourth-trial search_local (as test_local_fuzz draws them: 0..-40,
    and 3 / -1, the literal kernel, for every eighth of them).  Which trial of a block of four runs search_local moves with the
    block, and k moves with the block of three, so neither is tied to the matrix kind (trial % 4) or to the range layout
    (trial % 3).  Every draw is made for every trial, so trial t of a seed is the same whatever ran before it."""
    names = sorted(matrices)
    kind = trial % 4
    if kind == 0:
        M = np.asarray(matrices[names[int(rng.integers(len(names)))]], dtype=np.int32).copy()
    elif kind == 1:
        A = rng.integers(-8, 16, size=(24, 24)).astype(np.int32)
        M = np.minimum(A, A.T)
    elif kind == 2:
        M = np.asarray(matrices["blosum62"], dtype=np.int32).copy()
        M += rng.integers(-2, 3, size=(24, 24)).astype(np.int32)
    else:
        M = rng.integers(-120, 121, size=(24, 24)).astype(np.int32)
        M = np.minimum(M, M.T) if trial % 8 == 3 else M
    lo = int(rng.integers(1, 14))
    hi = int(min(32, lo + rng.integers(0, 20)))
    n = int(rng.integers(150, 420))
    if hi <= 8:   # no more than half the distinct peptides that exist (length-1 sets: 20)
        n = min(n, sum(20 ** L for L in range(lo, hi + 1)) // 2)
    res, off = synth_peptides(int(rng.integers(1, 10 ** 6)), n, lo, hi)
    lens = np.diff(off.astype(np.int64))
    X = int(rng.integers(0, min(int(lens.min()), 9)))
    p = int(rng.integers(-6, 3))
    i = rng.integers(0, n, 4000).astype(np.uint32)
    j = rng.integers(0, n, 4000).astype(np.uint32)
    quantile = float(rng.choice([0.0, 0.5, 0.9, 0.99, 0.999]))
    # the two ranges, at least 2 sequences each (the triangle runs over the query range)
    if trial % 3 == 2:
        while True:
            a0, a1, a2, a3 = (int(c) for c in np.sort(rng.choice(np.arange(1, n + 1), 4, replace=False)))
            if a1 - a0 >= 2 and a3 - a2 >= 2:
                break
        A, B = (a0, a1), (a2, a3)
    else:
        cut = int(rng.integers(2, n - 1))
        A, B = (0, cut), (cut, n)
    q, r = (B, A) if int(rng.integers(2)) else (A, B)
    go, ge = -int(rng.integers(0, 41)), -int(rng.integers(0, 41))
    local = trial % 4 == (trial // 4) % 4
    if local and (trial // 4) % 8 == 7:
        go, ge = 3, -1   # a positive penalty: the literal kernel
    st, sc = coracle.score_pairs(M, res, off, i, j, 0, X, p)
    assert st == 0
    thr = int(np.quantile(sc, quantile))
    return {"trial": trial, "kind": kind, "M": M, "symmetric": bool((M == M.T).all()), "lo": lo, "hi": hi, "n": n, "res": res, "off": off,
            "X": X, "p": p, "thr": thr, "q": q, "r": r, "k": (1, 5, 32)[(trial // 3) % 3], "local": local, "go": go, "ge": ge}


def sweep_describe(t):
    return {k: (list(v) if isinstance(v, tuple) else v) for k, v in t.items() if k not in ("M", "res", "off")} | {
        "Mmin": int(t["M"].min()), "Mmax": int(t["M"].max())}


def sweep_local_kernel(t):
    """which LocalAlignmentScorer kernel a trial's search_local runs (hmk_pass.cpp: local_literal, local_enc): the literal DP for
    a positive penalty or entries beyond int8, the tagged-max (packed) forms for entries and penalties within -31..31, else the
    plain striped kernel"""
    M, go, ge = t["M"], t["go"], t["ge"]
    if go > 0 or ge > 0 or M.min() < -127 or M.max() > 127:
        return "literal"
    if M.min() >= -31 and M.max() <= 31 and go >= -31 and ge >= -31:
        return "tagged"
    return "plain"


def sweep_predicted(t):
    return predicted_tiers(t["M"], lengths(t["off"], t["q"]), lengths(t["off"], t["r"]), t["X"], t["p"], t["thr"])


def sweep_run(t, coracle):
    """the checks of one trial on a fresh context -> the rectangle plan's NeighborStats"""
    M, res, off, q, r, X, p, thr = (t[k] for k in ("M", "res", "off", "q", "r", "X", "p", "thr"))
    what = sweep_describe(t)
    ctx = hammock_amd.Context(M, device=0)
    ctx.set_sequences(residues=res, offsets=off)
    blk = block_of(coracle, M, res, off, q, r, 0, X, p)
    st, _ = check_search(ctx, blk, q, r, X, p, thr, what)
    tiers = sweep_predicted(t)
    assert (st.classes_u8, st.classes_u16, st.classes_direct) == (tiers["u8"], tiers["u16"], tiers["direct"]), (what, tiers)
    check_best(ctx, blk, q, r, X, p, thr, t["k"], what)
    if t["symmetric"]:
        check_triangle(ctx, block_of(coracle, M, res, off, q, q, 0, X, p), *q, X, p, thr, what)
    if t["local"]:
        lblk = block_of(coracle, M, res, off, q, r, 1, t["go"], t["ge"])
        lthr = int(np.quantile(lblk, 0.9))
        edges, lst = ctx.search_local(*q, *r, t["go"], t["ge"], lthr)
        assert lst.pairs_scored == blk.size, what
        assert np.array_equal(np.sort(edges), rect_hits(lblk, q, r, lthr)), (what, "search_local", lthr)
    ctx.close()
    return st


def test_sweep_seed_reaches_every_tier(matrices, coracle):
    """The sweep's seed, on the CPU: by the predicate its 48 rectangles hold 8-bit, 16-bit and literal classes, symmetric
    matrices (triangles), both range orders, and ranges that leave sequences outside; its 12 search_local trials run under
    every matrix kind and launch the tagged-max, the plain striped and the literal kernels."""
    rng = np.random.default_rng(SWEEP_SEED)
    total = {"u8": 0, "u16": 0, "direct": 0}
    triangles = behind = outside = 0
    local_kernels, local_kinds, k_by_layout = {"literal": 0, "tagged": 0, "plain": 0}, set(), set()
    for trial in range(SWEEP_TRIALS):
        t = sweep_trial(rng, trial, matrices, coracle)
        if t["local"]:
            local_kernels[sweep_local_kernel(t)] += 1
            local_kinds.add(t["kind"])
        k_by_layout.add((trial % 3 == 2, t["k"]))
        for key, v in sweep_predicted(t).items():
            total[key] += v
        (q0, q1), (r0, r1) = t["q"], t["r"]
        assert q1 - q0 >= 2 and r1 - r0 >= 2 and (q1 <= r0 or r1 <= q0) and t["X"] < lengths(t["off"], (0, t["n"])).min()
        triangles += t["symmetric"]
        behind += q0 > r0
        outside += (q1 - q0) + (r1 - r0) < t["n"]
    assert total["u8"] and total["u16"] and total["direct"], total
    assert triangles >= 12 and behind >= 8 and outside == SWEEP_TRIALS // 3
    # search_local meets every matrix kind and all three of its kernels; touching and separated ranges meet every k
    assert sum(local_kernels.values()) == SWEEP_TRIALS // 4 and all(local_kernels.values()), local_kernels
    assert local_kinds == {0, 1, 2, 3}
    assert k_by_layout == {(sep, k) for sep in (False, True) for k in (1, 5, 32)}


@pytest.mark.gpu
def test_rect_fuzz_lane_classification(gpu, matrices, coracle):
    """48 trials: search_shifted, search_best_shifted, the triangle (symmetric matrices) and every fourth trial search_local
    against the oracle; no trial is skipped or expects an error, and all three lane tiers ran."""
    rng = np.random.default_rng(SWEEP_SEED)
    used = {"u8": 0, "u16": 0, "direct": 0, "rows": 0}
    for trial in range(SWEEP_TRIALS):
        st = sweep_run(sweep_trial(rng, trial, matrices, coracle), coracle)
        used["u8"] += st.classes_u8
        used["u16"] += st.classes_u16
        used["direct"] += st.classes_direct
        used["rows"] += st.classes_rows
    assert used["u8"] and used["u16"] and used["direct"], used   # (the row-packed coverage is cases (a) and (b)'s)


@pytest.mark.gpu
def test_rect_and_triangle_refuse_scores_beyond_int16(gpu, matrices):
    """an argument error before any launch, for both plans"""
    M = matrix_named(matrices, "blosum62")
    res, off = synth_peptides(2, 300, 8, 20)
    ctx = hammock_amd.Context(M, device=0)
    ctx.set_sequences(residues=res, offsets=off)
    with pytest.raises(ValueError, match="int16"):
        ctx.search_shifted(0, 100, 100, 300, 3, 2000, 20)
    with pytest.raises(ValueError, match="int16"):
        ctx.search_best_shifted(0, 100, 100, 300, 3, 2000, 20, 4)
    with pytest.raises(ValueError, match="int16"):
        ctx.cluster_pairs_shifted(50, 250, np.arange(200), 200, 3, 2000, 20)
    edges, _ = ctx.search_shifted(0, 100, 100, 300, 3, 2, 20)      # a small positive penalty is fine
    assert len(edges) > 0
    assert len(ctx.cluster_pairs_shifted(50, 250, np.arange(200), 200, 3, 2, 20)) > 0


# ---- (f) dense results that outgrow the first edge buffer -------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["search_shifted", "search_local", "search_best_shifted", "cluster_pairs_shifted"])
def test_rect_dense_results_outgrow_the_first_edge_buffer(gpu, matrices, coracle, entry):
    """Every pair is a hit (threshold -30000), more than 2^20 of them, on a FRESH context: the pass's grow-and-rescore path;
    then the same call again on the grown context."""
    M = matrix_named(matrices, "blosum62")
    rng = np.random.default_rng(6000)
    nq, nr, X, p, thr = 1499, 1511, 3, -1, -30000
    seqs = peptides(rng, nq + nr, 8, 14)
    ctx, res, off = ctx_with(M, seqs)
    q, r = (nr, nr + nq), (0, nr)
    if entry == "cluster_pairs_shifted":
        t = (503, 503 + 1709)
        assert (t[1] - t[0]) * (t[1] - t[0] - 1) // 2 > FIRST_EDGE_BUFFER
        blk = block_of(coracle, M, res, off, t, t, 0, X, p)
        for _ in range(2):
            assert len(check_triangle(ctx, blk, *t, X, p, thr, entry)) == blk.shape[0] * (blk.shape[0] - 1) // 2
        return
    assert nq * nr > FIRST_EDGE_BUFFER
    if entry == "search_local":
        blk = block_of(coracle, M, res, off, q, r, 1, -5, -1)
        want = rect_hits(blk, q, r, thr)
        assert len(want) == nq * nr
        for _ in range(2):
            edges, st = ctx.search_local(*q, *r, -5, -1, thr)
            assert st.pairs_scored == nq * nr and np.array_equal(np.sort(edges), want)
        return
    blk = block_of(coracle, M, res, off, q, r, 0, X, p)
    for _ in range(2):
        if entry == "search_shifted":
            _, want = check_search(ctx, blk, q, r, X, p, thr, entry)
            assert len(want) == nq * nr
        else:
            check_best(ctx, blk, q, r, X, p, thr, 32, entry)
            assert ctx.last_search_stats.n_edges == nq * nr


# ---- (g) best-k selection shapes -----------------------------------------------------------------------------------------------------------------

BESTK = {"X": 3, "p": 0, "thr": 24, "nq": 40 + 40 + 2201, "f1_refs": 4097, "f2_refs": 4000, "rnd_refs": 1500}


_bestk_cache = []


def bestk_recipe(matrices, co):
    """Two families of 1-2-substitution mutants of WCHYPWCHYPWC and MFIKDMFIKDMF (4,097 and 4,000 references of each) plus 1,500
    random 12-mer references; the queries are 40 mutants of each family and 2,201 random 12-mers, in that order, all in front of
    the references -> (blosum62, res, off, nq, the oracle block [nq, nr] at X = 3, p = 0)"""
    if _bestk_cache:       # (the CPU guard and the GPU test share one oracle block)
        return _bestk_cache[0]
    M = matrix_named(matrices, "blosum62")
    rng = np.random.default_rng(7)
    seen = set()

    def family(centre, n):
        out = []
        while len(out) < n:
            s = centre.copy()
            k = int(rng.integers(1, 3))
            s[rng.choice(12, k, replace=False)] = rng.integers(0, 20, k)
            if s.tobytes() in seen:
                continue
            seen.add(s.tobytes())
            out.append(s)
        return out

    f1 = family(hammock_amd.encode("WCHYPWCHYPWC"), BESTK["f1_refs"] + 40)
    f2 = family(hammock_amd.encode("MFIKDMFIKDMF"), BESTK["f2_refs"] + 40)
    sres, soff = co.synth(73, 3800, 12)
    rnd = [s for s in (sres[soff[k]:soff[k + 1]].copy() for k in range(3800)) if s.tobytes() not in seen]
    n_rq = BESTK["nq"] - 80
    queries = f1[:40] + f2[:40] + rnd[:n_rq]
    refs = f1[40:] + f2[40:] + rnd[n_rq:n_rq + BESTK["rnd_refs"]]
    res, off = hammock_amd.pack_sequences(queries + refs)
    nq = len(queries)
    st, blk = co.score_block(M, res, off, np.arange(nq), np.arange(nq, nq + len(refs)), 0, BESTK["X"], BESTK["p"])
    assert st == 0
    _bestk_cache.append((M, res, off, nq, blk))
    return _bestk_cache[0]


def bestk_facts(matrices, coracle, k=32):
    """the five facts of the recipe, from the oracle block alone: queries with 0 hits, with 1..k-1, with k..4,096 and with more
    than 4,096 in ONE call of more than 2,048 queries (the scan leaves one 2,048-entry tile) whose count is no multiple of 4"""
    _, _, _, nq, blk = bestk_recipe(matrices, coracle)
    cnt = (blk >= BESTK["thr"]).sum(axis=1)
    groups = {"0": int((cnt == 0).sum()), "1..k-1": int(((cnt >= 1) & (cnt < k)).sum()),
              "k..4096": int(((cnt >= k) & (cnt <= LONG_RUN)).sum()), ">4096": int((cnt > LONG_RUN).sum())}
    assert all(groups.values()), groups
    assert sum(groups.values()) == nq and nq > 2048 and nq % 4 != 0
    assert (cnt[:40] > LONG_RUN).all() and not (cnt[80:] > LONG_RUN).any()   # the first family's queries are the long runs
    return groups


def test_bestk_recipe_holds_every_run_shape(matrices, coracle):
    groups = bestk_facts(matrices, coracle, 32)
    assert groups[">4096"] >= 40 and groups["0"] > 100 and groups["1..k-1"] > 100 and groups["k..4096"] > 40, groups


@pytest.mark.gpu
def test_rect_best_k_run_shapes_in_one_call(gpu, matrices, coracle):
    """One search_best_shifted call over more than 2,048 queries whose runs are empty, shorter than k, up to 4,096 and longer;
    then every run exactly 4,096 and exactly 4,097 hits long (the boundary between the wave and the workgroup selection)."""
    bestk_facts(matrices, coracle, 32)          # asserted from the oracle block before the GPU answers
    M, res, off, nq, blk = bestk_recipe(matrices, coracle)
    n = len(off) - 1
    X, p, thr = BESTK["X"], BESTK["p"], BESTK["thr"]
    ctx = hammock_amd.Context(M, device=0)
    ctx.set_sequences(residues=res, offsets=off)
    for k in (1, 32):
        check_best(ctx, blk, (0, nq), (nq, n), X, p, thr, k, ("recipe", k))
        assert ctx.last_search_stats.n_edges == int((blk >= thr).sum())
    nq_b = 601
    for n_refs in (LONG_RUN, LONG_RUN + 1):
        sub = blk[:nq_b, :n_refs]
        assert ((sub >= -30000).sum(axis=1) == n_refs).all()
        check_best(ctx, sub, (0, nq_b), (nq, nq + n_refs), X, p, -30000, 32, ("boundary", n_refs))
        assert ctx.last_search_stats.n_edges == nq_b * n_refs


# ---- (h) one long-lived context ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_rect_plans_do_not_survive_an_upload(gpu, matrices, coracle):
    """Three uploads with different length profiles into ONE context, and after each the same calls with identical ranges and
    parameters: every plan's cache key matches the previous upload's, so only set_sequences' invalidation of the plan slots keeps
    a stale plan from answering."""
    M = matrix_named(matrices, "blosum62")
    rng = np.random.default_rng(8000)
    nq, nm, X, p, thr, k = 701, 1201, 3, -1, 22, 3
    q, r = (0, nq), (nq, nq + nm)
    ctx = hammock_amd.Context(M, device=0)
    previous = None
    for lo, hi in ((8, 12), (12, 12), (14, 20)):
        members, mc, queries, qc = test_match.two_sides(rng, nm, nq, lo, hi)
        mc = test_assign.relabel(mc)
        msz = rng.integers(1, 6, size=nm).astype(np.int32)
        nsz = np.ones(nq, np.int32)
        ids = rng.permutation(np.arange(int(mc.max()) + 1) * 7 + 100).astype(np.int32)
        res, off = hammock_amd.pack_sequences(queries + members)
        ctx.set_sequences(residues=res, offsets=off, sizes=np.concatenate([nsz, msz]))
        what = ("upload", lo, hi)
        blk = block_of(coracle, M, res, off, q, r, 0, X, p)
        _, want = check_search(ctx, blk, q, r, X, p, thr, what)
        assert len(want) > 0 and (previous is None or not np.array_equal(want, previous))
        previous = want
        check_best(ctx, blk, q, r, X, p, thr, 5, what)
        mblk = test_assign.block(coracle, M, res, off, q, r, 0, X, p)         # [member, new]
        test_assign.check(ctx.assign_shifted(*q, *r, mc, ids, X, p, thr, k), test_assign.expected(mblk, mc, ids, msz, thr, k))
        mn, nn = test_continue.blocks(coracle, M, res, off, q, r, X, p)
        wj, wr = test_continue.restate(mn, nn, mc, ids, msz, nsz, thr)
        gj, gr = ctx.greedy_continue(*q, *r, mc, ids, X, p, thr)
        assert np.array_equal(gj, wj) and np.array_equal(gr, wr), what
        assert (wj >= 0).any()
        test_match.check(ctx.match_clusters_shifted(*q, qc, *r, mc, ids, X, p, thr, k),
                         test_match.expected(mblk, mc, ids, msz, qc, thr, k))
        check_triangle(ctx, block_of(coracle, M, res, off, r, r, 0, X, p), *r, X, p, thr, what)
