"""Every narrowing of a score at the exact edge of its field.  The shifted-scorer path is exact because classify() (hmk_plan.cpp)
proves that a shift plane's lane starts at g + penalty - bias * cells >= 0 and ends at g + penalty + score <= 255 (65535); after the
pass a score is narrowed again into the hit record's 8-bit score - threshold, the int16 of a packed edge, the 4-byte adjacency entry,
the band's candidate key and the 4-byte row blocks of the exchange.  A one-unit slip in any of them shows only for a pair whose lane
lands on 0, 255 or 65535 or whose score - threshold is 0, 255 or 256 -- which random peptides never produce.  tests/lane_model.py
builds such pairs (synonym residues: two DISTINCT peptides that score what a peptide scores against itself).

The CPU tests (unmarked) prove with the oracle that every input does what its GPU case claims: at thr_lo a scored pair's winning
plane ends at exactly lane_max, at thr_hi a plane starts at exactly 0 and a pair keeps it there, one threshold further the class
leaves the tier, bound-exact rows have the bounds they claim, the adjacency cases hold score - threshold = 0, 255 and 256.  The GPU
tests (-m gpu, an MI355X) take their inputs from the same cached builders and compare edges and clusterings with the oracle for
exact equality; each asserts the tier that ran against the predicate."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

import hammock_amd
from hammock_amd.synth import synth_peptides
import lane_model as lm
from oracle import c_oracle

THR_LIMIT = 30000          # check_shift_threshold_scores: thresholds outside [-30000, 30000] are refused
SWITCHES = ("HMK_NO_KEY_SORT", "HMK_KEY_SORT_KEYS", "HMK_NO_ROW_SHARED", "HMK_NO_ROWS_KERNEL", "HMK_ADJ_8BYTE", "HMK_NO_BAND")
N_ORDINARY = 300
N_TOP = 17                 # more than two row groups' worth: the key-sorted order holds a full row group of top words


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need an MI355X; no HIP device is visible")
    return 0


# ---- matrices ---------------------------------------------------------------------------------------------------------------------------

_matrices = {}


def matrix(name):
    """b62s: BLOSUM62 with B, Z, X exact copies of W, K, I;  c14s: the same of np.clip(blosum62, -1, 4);  b62s_x3: b62s * 3 (top of a
    12-mer pair 396);  top16: (b62s + 4) * 16, non-negative with maximum 240 (a 12-mer pair's top is 2,880: 16-bit lanes end at 65535
    at threshold -29,887);  bot16: (b62s - 10) * 17, minimum -238 (bias * 12 = 2,856: 16-bit lanes start at 0 at threshold 29,912);
    both16: np.clip(b62s, -4, 4) * 30, maximum = bias = 120 (24-mers: 24 * 120 = 2,880 serves both 16-bit edges);
    i16: b62s with W against W at 1,000, the largest entry a context accepts"""
    if not _matrices:
        with open(os.path.join(GOLDEN, "matrices.json")) as fh:
            b62 = np.asarray(json.load(fh)["matrices"]["blosum62"], dtype=np.int32)
        s = lm.with_synonyms(b62)
        _matrices.update({"b62": b62, "b62s": s, "c14s": lm.with_synonyms(lm.clip14(b62)), "b62s_x3": s * 3, "top16": (s + 4) * 16,
                          "bot16": (s - 10) * 17, "both16": np.clip(s, -4, 4) * 30})
        w = b62.copy()
        w[lm.code("W"), lm.code("W")] = 1000
        _matrices["i16"] = lm.with_synonyms(w)
    return _matrices[name]


def test_synonym_matrices_keep_range_and_symmetry():
    b62 = matrix("b62")
    for base, syn in ((b62, matrix("b62s")), (lm.clip14(b62), matrix("c14s"))):
        assert (syn == syn.T).all() and syn.min() == base.min() and syn.max() == base.max()
        assert (syn[:20, :20] == base[:20, :20]).all()
        for o, c in lm.SYNONYMS:
            o, c = lm.code(o), lm.code(c)
            assert (syn[c] == syn[o]).all() and (syn[:, c] == syn[:, o]).all() and syn[c, c] == syn[o, o] == syn[o, c]
    assert matrix("top16").min() == 0 and matrix("top16").max() == 240
    assert matrix("bot16").min() == -238 and matrix("bot16").max() + 238 == 255
    assert matrix("i16").max() == 1000


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------

class Input:
    """one planted set: the words, where its families are, and the oracle's all-pairs block per (max shift, penalty), computed once"""

    def __init__(self, M, seqs, marks):
        self.M, self.seqs = M, seqs
        self.res, self.off = hammock_amd.pack_sequences(seqs)
        self.n = len(seqs)
        where = {w.tobytes(): k for k, w in enumerate(seqs)}
        assert len(where) == self.n        # distinct
        self.idx = {name: np.array([where[w.tobytes()] for w in words], dtype=np.uint32) for name, words in marks.items()}
        self._blocks = {}

    def block(self, X, p):
        """[n, n] of score(seq1 = i, seq2 = j) by the C oracle"""
        if (X, p) not in self._blocks:
            st, blk = c_oracle.score_block(self.M, self.res, self.off, np.arange(self.n), np.arange(self.n), 0, X, p)
            assert st == 0
            blk.setflags(write=False)
            self._blocks[(X, p)] = blk
        return self._blocks[(X, p)]

    def edges(self, X, p, thr):
        """the all-vs-all pass's sorted packed edges under a symmetric matrix: x < m"""
        blk = self.block(X, p)
        m, x = np.nonzero(np.tril(blk >= thr, -1))
        return np.sort(hammock_amd.pack_edges(x, m, blk[m, x]))

    def pairs(self, a, b, X, p):
        """oracle scores of every pair (i in family a, j in family b), i != j -> (i, j, score)"""
        i, j = np.meshgrid(self.idx[a], self.idx[b], indexing="ij")
        keep = i != j
        return i[keep], j[keep], self.block(X, p)[i[keep], j[keep]]


_inputs = {}


def planted(mat, la, lb, extra=None):
    """The families of a (la, lb) class, la >= lb, plus about 300 ordinary peptides of those lengths, in one random order; n is no
    multiple of 8 and the first and the last sequence are top words.  top_long / top_short: N_TOP words each over the synonym pair
    at the matrix maximum (at length 12 with the original at both key positions, 5 and 6); bot_row / bot_col: a word of length la and words of length lb whose every cell is the
    matrix minimum (for la > lb also the pair of one length each, so every class of the set has one).  extra: (name, words) lists"""
    key = (mat, la, lb, extra)
    if key in _inputs:
        return _inputs[key]
    M = matrix(mat)
    rng = np.random.default_rng(100 * la + lb)
    fixed = lambda L: (5, 6) if L == 12 else ()
    marks = {"top_long": lm.top_words(M, la, N_TOP, rng, fixed(la))}
    marks["top_short"] = marks["top_long"] if la == lb else lm.top_words(M, lb, N_TOP, rng, fixed(lb))
    marks["bot_row"], marks["bot_col"] = lm.bottom_words(M, la, lb, 5, rng)
    groups = [marks["top_long"], marks["bot_row"], marks["bot_col"]]
    if la != lb:
        groups.append(marks["top_short"])
    for name, words in (EXTRA[extra](M) if extra else ()):
        marks[name] = words
        groups.append(words)
    planted_words = [w for g in groups for w in g]
    n_ord = N_ORDINARY
    while (len(planted_words) + n_ord) % 8 == 0:
        n_ord += 1
    seqs = lm.shuffled(rng, planted_words, lm.ordinary(rng, n_ord, [la, lb], avoid=planted_words))
    # a top word first and one last: the reference's greedy clusterer fails on a first sequence without a neighbour and on a last
    # one without a cluster to join (its searches of an empty list return a dummy), and top words have neighbours at every
    # threshold their score reaches
    for spot, w in ((0, marks["top_long"][0]), (len(seqs) - 1, marks["top_long"][1])):
        k = next(k for k, v in enumerate(seqs) if v is w)
        seqs[spot], seqs[k] = seqs[k], seqs[spot]
    _inputs[key] = Input(M, seqs, marks)
    assert _inputs[key].n % 8 != 0 and _inputs[key].n <= 600
    return _inputs[key]


def thresholds(win):
    lo, hi = win
    return [t for t in dict.fromkeys((lo - 1, lo, hi, hi + 1)) if -THR_LIMIT <= t <= THR_LIMIT]


# ---- the claims, proven on the CPU -----------------------------------------------------------------------------------------------------

def prove_edges(inp, la, lb, X, p, kind, top=True, bottom=True):
    """what a GPU case relies on, by the oracle and the predicate alone -> (thr_lo, thr_hi)"""
    M = inp.M
    lane_max, half, _ = lm.LANES[kind]
    win = lm.lane_window(M, la, lb, X, p, kind)
    assert win is not None, (la, lb, X, p, kind)
    lo, hi = win
    assert lm.lane_path(M, la, lb, X, p, lo) == kind and lm.lane_path(M, la, lb, X, p, hi) == kind
    assert lm.lane_path(M, la, lb, X, p, lo - 1) != kind and lm.lane_path(M, la, lb, X, p, hi + 1) != kind
    bias = lm.bias_of(M)
    if top:
        assert -THR_LIMIT <= lo - 1
        # the winning plane's lane ends at g + score (its penalty is part of the score)
        i, j, sc = inp.pairs("top_long", "top_short", X, p)
        at_max = half - lo + sc == lane_max
        assert at_max.any() and not (half - lo + sc > lane_max).any()
        k = int(np.flatnonzero(at_max)[0])
        assert lm.shifted_score(M, inp.seqs[i[k]], inp.seqs[j[k]], X, p) == sc[k]      # (the model agrees with the oracle)
        assert half - lo + inp.block(X, p).max() <= lane_max or la != lb      # nothing of a one-length set goes beyond
    if bottom:
        assert hi + 1 <= THR_LIMIT
        at_zero = [t for t, (_, ncell, pen) in enumerate(lm.planes(la, lb, X, p)) if half - hi + pen - bias * ncell == 0]
        assert at_zero
        row, col = inp.seqs[inp.idx["bot_row"][0]], inp.seqs[inp.idx["bot_col"][0]]
        assert len(row) == la and len(col) == lb
        sums = lm.plane_sums(M, row, col, X, p)
        for t in at_zero:                       # lane = start + sum of (cell + bias): every cell at the minimum keeps it at 0
            s, cells, pen = sums[t]
            assert cells + bias * lm.planes(la, lb, X, p)[t][1] == 0
        assert max(c + pen for _, c, pen in sums) == inp.block(X, p)[inp.idx["bot_row"][0], inp.idx["bot_col"][0]]
    return lo, hi


# ---- (a) one-length row-packed forms ----------------------------------------------------------------------------------------------------

def one_length_cases():
    """(matrix, L, X, p): L = 6 .. 17 under synonym-BLOSUM62 (18 .. 20 have no 8-bit window) and L = 6 .. 20 under synonym-clip14 at
    the reference's max shift and p = 0 -- all 15 exact shapes; L = 12 also at p = -2 and +2 (under clip14 at p = -2 the lower edge
    binds on a shifted plane)"""
    out = [("b62s", L, lm.uniform_defaults(L)[0], 0) for L in range(6, 18)]
    out += [("c14s", L, lm.uniform_defaults(L)[0], 0) for L in range(6, 21)]
    out += [("b62s", 12, 3, -2), ("b62s", 12, 3, 2), ("c14s", 12, 3, -2)]
    return out


ONE_LENGTH = one_length_cases()
ONE_LENGTH_IDS = [f"{mat}_L{L}_X{X}_p{p}" for mat, L, X, p in ONE_LENGTH]


def test_one_length_windows_are_the_ones_the_planner_documents():
    """the windows come from the predicate; a few of them, as DESIGN.md and the planner's comments state them"""
    b, c = matrix("b62s"), matrix("c14s")
    assert lm.lane_window(b, 12, 12, 3, 0, "u8") == (5, 80) and lm.lane_window(b, 17, 17, 4, 0, "u8") == (60, 60)
    assert all(lm.lane_window(b, L, L, lm.uniform_defaults(L)[0], 0, "u8") is None for L in (18, 19, 20))
    assert lm.lane_window(c, 12, 12, 3, 0, "u8") == (-79, 116) and lm.lane_window(c, 12, 12, 3, -2, "u8") == (-79, 107)
    assert lm.lane_window(b, 14, 12, 3, -1, "u8") == (3, 78) and lm.lane_window(b, 20, 18, 5, -3, "u8") is None
    assert sorted({X for _, _, X, _ in ONE_LENGTH}) == [2, 3, 4, 5]


@pytest.mark.parametrize("case", ONE_LENGTH, ids=ONE_LENGTH_IDS)
def test_one_length_inputs_reach_both_edges(case):
    mat, L, X, p = case
    inp = planted(mat, L, L)
    lo, hi = prove_edges(inp, L, L, X, p, "u8")
    if (mat, p) == ("c14s", -2):     # the plane that starts at 0 is a shifted one
        assert all(lm.planes(L, L, X, p)[t][0] != 0 for t, (_, n, pen) in enumerate(lm.planes(L, L, X, p))
                   if 128 - hi + pen - lm.bias_of(inp.M) * n == 0)
    for thr in (lo, hi):
        assert lm.allpairs_tiers(inp.M, inp.seqs, X, p, thr) == {"u8": 1, "u16": 0, "direct": 0}
    # one below the window the rows whose bound still fits keep 8-bit lanes and the top words leave (under clip14 every residue's
    # best cell is the maximum: no row fits); one above nothing fits
    assert lm.allpairs_tiers(inp.M, inp.seqs, X, p, lo - 1) == {"u8": 1 if mat == "b62s" else 0, "u16": 1, "direct": 0}
    assert lm.allpairs_tiers(inp.M, inp.seqs, X, p, hi + 1) == {"u8": 0, "u16": 1, "direct": 0}
    assert (len(inp.edges(X, p, hi)) > 0) == (L * inp.M.max() >= hi)       # (short words cannot reach the upper thresholds at all)


def saved_env(env):
    """the switches are read by the library at every call: set them for one block, then put back what was there"""
    class _Env:
        def __enter__(self):
            self.keep = {k: os.environ.get(k) for k in SWITCHES}
            for k in self.keep:
                os.environ.pop(k, None)
            os.environ.update(env)

        def __exit__(self, *a):
            for k, v in self.keep.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
    return _Env()


def context(inp):
    ctx = hammock_amd.Context(inp.M, device=0)
    ctx.set_sequences(residues=inp.res, offsets=inp.off)
    return ctx


def check_allpairs(ctx, inp, X, p, thr, what, rows="all"):
    """one all-vs-all pass: the classes ran on the tiers the predicate gives them, the edges are the oracle's -> stats"""
    edges, st = ctx.neighbors_shifted(X, p, thr)
    tiers = lm.allpairs_tiers(inp.M, inp.seqs, X, p, thr)
    ran = (st.classes_u8, st.classes_u16, st.classes_direct, st.classes_rows)
    want = inp.edges(X, p, thr)
    got = np.sort(edges)
    assert st.n_edges == len(want), (what, thr, st.n_edges, len(want), ran, tiers)
    assert np.array_equal(got, want), (what, thr, len(got), len(want), ran, tiers)
    assert ran[:3] == (tiers["u8"], tiers["u16"], tiers["direct"]), (what, thr, ran, tiers)
    if rows == "all":
        assert st.classes_rows == st.classes_u8, (what, thr, ran)
    elif rows == "none":
        assert st.classes_rows == 0, (what, thr, ran)
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("case", ONE_LENGTH, ids=ONE_LENGTH_IDS)
def test_one_length_rows_kernels_at_the_lane_edges(gpu, case):
    """the compile-time-length forms (6-9-mers: the rescoring flush; longer: in-loop extraction) at thr_lo - 1, thr_lo, thr_hi and
    thr_hi + 1; the last row group has dead rows"""
    mat, L, X, p = case
    inp = planted(mat, L, L)
    ctx = context(inp)
    for thr in thresholds(lm.lane_window(inp.M, L, L, X, p, "u8")):
        check_allpairs(ctx, inp, X, p, thr, case)
    ctx.close()


# ---- (b) key-sorted and row-shared 12-mers ---------------------------------------------------------------------------------------------------

def test_key_sorted_input_has_a_row_shared_group_of_top_words():
    """in the key-sorted order (stable, by the residues at positions 5 and 6) some full row group is row-shared -- one key, the top
    words' -- and most of its rows are top words (an ordinary peptide with the same key residues may sit among them)"""
    inp = planted("b62s", 12, 12)
    keys = np.array([int(w[5]) * 24 + int(w[6]) for w in inp.seqs])
    order = np.argsort(keys, kind="stable")
    top = set(inp.idx["top_long"].tolist())
    groups = [order[g:g + 8] for g in range(0, inp.n - 7, 8)]
    assert any(len(set(keys[g])) == 1 and sum(int(k) in top for k in g) >= 4 for g in groups)
    assert any(len(set(keys[g])) == 1 for g in groups) and any(len(set(keys[g])) > 1 for g in groups)


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{}, {"HMK_NO_ROW_SHARED": "1"}, {"HMK_NO_KEY_SORT": "1"}], ids=["default", "no_row_shared", "no_key_sort"])
def test_key_sorted_and_row_shared_bodies_at_the_lane_edges(gpu, env):
    """the 12-mer input, whose top words share both key residues (merged entries hold the largest bytes there are, and the key
    table's start values the smallest and the largest), under the default switches, without the row-shared bodies and in the
    caller's order"""
    inp = planted("b62s", 12, 12)
    with saved_env(env):
        ctx = context(inp)
        for thr in thresholds(lm.lane_window(inp.M, 12, 12, 3, 0, "u8")):
            check_allpairs(ctx, inp, 3, 0, thr, env)
        ctx.close()


# ---- (c) capacity and per-length forms ------------------------------------------------------------------------------------------------------

# (lb, D, X, p): a two-length set (lb, lb + D); one class for every (max shift, column capacity) of HMK_ROWS_CAP_LIST -- capacity 12
# at every max shift 1 .. 5, 16 at 2 .. 5, 20 at 3 .. 5 -- with D > 0 and p < 0; max shifts 2 and 3 run k_neighbors_rows_lens
MIXED = [(8, 2, 1, -1), (10, 3, 2, -1), (14, 2, 2, -2), (12, 2, 3, -1), (12, 8, 3, -1), (13, 3, 3, -2), (18, 2, 3, -1),
         (10, 4, 4, -1), (13, 3, 4, -2), (17, 2, 4, -1), (11, 2, 5, -1), (14, 3, 5, -2), (18, 2, 5, -3)]
MIXED_IDS = [f"{lb + D}-{lb}_X{X}_p{p}" for lb, D, X, p in MIXED]


def mixed_matrix(lb, D, X, p):
    """synonym-BLOSUM62 where the class has an 8-bit window, else synonym-clip14"""
    return "b62s" if lm.lane_window(matrix("b62s"), lb + D, lb, X, p, "u8") else "c14s"


def test_mixed_cases_cover_every_shift_and_capacity():
    cap = lambda lb: 12 if lb <= 12 else 16 if lb <= 16 else 20
    assert {(X, cap(lb)) for lb, D, X, p in MIXED} == {(1, 12), (2, 12), (2, 16), (3, 12), (3, 16), (3, 20), (4, 12), (4, 16), (4, 20),
                                                      (5, 12), (5, 16), (5, 20)}
    assert all(D > 0 and p < 0 and lb >= 2 * X for lb, D, X, p in MIXED)
    assert {mixed_matrix(*c) for c in MIXED} == {"b62s", "c14s"}


@pytest.mark.parametrize("case", MIXED, ids=MIXED_IDS)
def test_mixed_inputs_reach_both_edges(case):
    """top: a long and a short word whose whole overlap is synonyms; bottom: a long and a short word whose every cell is the minimum"""
    lb, D, X, p = case
    inp = planted(mixed_matrix(*case), lb + D, lb)
    lo, hi = prove_edges(inp, lb + D, lb, X, p, "u8")
    assert lm.lane_path(inp.M, lb + D, lb, X, p, lo - 1) == "u16" and lm.lane_path(inp.M, lb + D, lb, X, p, hi + 1) == "u16"


@pytest.mark.gpu
@pytest.mark.parametrize("case", MIXED, ids=MIXED_IDS)
def test_mixed_length_rows_kernels_at_the_lane_edges(gpu, case):
    lb, D, X, p = case
    inp = planted(mixed_matrix(*case), lb + D, lb)
    ctx = context(inp)
    for thr in thresholds(lm.lane_window(inp.M, lb + D, lb, X, p, "u8")):
        st = check_allpairs(ctx, inp, X, p, thr, case, rows="any")
        if lm.lane_path(inp.M, lb + D, lb, X, p, thr) == "u8":
            # the (X, D, capacity) form and its D = 0 companions all exist (HMK_ROWS_CAP_LIST): every 8-bit class is row-packed,
            # the D > 0 class the case is named for among them
            assert st.classes_rows == st.classes_u8 >= 1, (case, thr, st.classes_rows, st.classes_u8)
    ctx.close()


# ---- (d) shift-packed tier --------------------------------------------------------------------------------------------------------------------

SHIFT_PACKED_U8 = [("b62s", 12, 12, 3, 0), ("b62s", 7, 7, 2, 0), ("c14s", 20, 20, 5, 0), ("b62s", 14, 12, 3, -1), ("b62s", 16, 13, 4, -2)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", SHIFT_PACKED_U8, ids=[f"{m}_{la}-{lb}_X{X}_p{p}" for m, la, lb, X, p in SHIFT_PACKED_U8])
def test_shift_packed_u8_lanes_at_the_lane_edges(gpu, case):
    """HMK_NO_ROWS_KERNEL=1: the same inputs and thresholds on the shift-packed kernels' 8-bit lanes (the CPU proofs are cases (a)
    and (c)'s: every (la, lb, X, p) here is one of theirs)"""
    mat, la, lb, X, p = case
    assert (mat, la, X, p) in ONE_LENGTH if la == lb else (lb, la - lb, X, p) in MIXED and mixed_matrix(lb, la - lb, X, p) == mat
    inp = planted(mat, la, lb)
    with saved_env({"HMK_NO_ROWS_KERNEL": "1"}):
        ctx = context(inp)
        for thr in thresholds(lm.lane_window(inp.M, la, lb, X, p, "u8")):
            check_allpairs(ctx, inp, X, p, thr, case, rows="none")
        ctx.close()


def test_u16_inputs_reach_the_edge_each_can():
    top, bot = planted("top16", 12, 12), planted("bot16", 12, 12)
    lo, hi = prove_edges(top, 12, 12, 3, 0, "u16", bottom=False)
    assert (lo, hi > THR_LIMIT) == (-29887, True)       # a non-negative matrix has no bias: its lanes start at 32768 - thr
    lo, hi = prove_edges(bot, 12, 12, 3, 0, "u16", top=False)
    assert (lo < -THR_LIMIT, hi) == (True, 29912)       # 12 * 17 - 32767 is far below the lowest threshold
    assert lm.lane_path(top.M, 12, 12, 3, 0, -29888) == "direct" and lm.lane_path(bot.M, 12, 12, 3, 0, 29913) == "direct"
    # from 22 cells on one matrix serves both edges: maximum = bias = 120 at length 24
    both = planted("both16", 24, 24)
    assert prove_edges(both, 24, 24, 3, 0, "u16") == (-29887, 29888)
    assert lm.lane_path(both.M, 24, 24, 3, 0, -29888) == "direct" and lm.lane_path(both.M, 24, 24, 3, 0, 29889) == "direct"


@pytest.mark.gpu
def test_shift_packed_u16_lanes_at_the_lane_edges(gpu):
    """16-bit lanes of the 12-mer class.  With 12 cells no matrix reaches both edges inside the threshold limits [-30000, 30000]: the
    top needs cells * max - 32767 >= -30000 and the bottom bias * cells >= 2768, and max + bias <= 255 (from 22 cells on one matrix
    can: test_shift_packed_u16_lanes_both_edges_in_one_class).  So two matrices, one edge each:
    top16 (maximum 240, no bias) at thresholds -29,888 (literal tier) and -29,887 (a pair of top words ends at 65535) -- its
    bottom edge, threshold 32,768, is NOT reached; bot16 (minimum -238) at 29,912 (the all-minimum pair stays at 0) and 29,913
    (literal tier) -- its top edge, threshold -32,563, is NOT reached.  At bot16's thresholds no pair is a hit: a lane that
    started below 0 would wrap to the top of its field and become one."""
    for mat, thrs in (("top16", (-29888, -29887, 0)), ("bot16", (29912, 29913, 100))):
        inp = planted(mat, 12, 12)
        ctx = context(inp)
        for thr in thrs:
            st = check_allpairs(ctx, inp, 3, 0, thr, mat, rows="none")
            assert st.classes_u8 == 0
        assert len(inp.edges(3, 0, thrs[2])) > 0
        ctx.close()


@pytest.mark.gpu
def test_shift_packed_u16_lanes_both_edges_in_one_class(gpu):
    """24-mers under a matrix with maximum = bias = 120: one class whose 16-bit lanes end at 65535 at threshold -29,887 (a pair of top
    words) and start at 0 at 29,888 (the all-minimum pair stays there); one threshold further either way is the literal tier"""
    inp = planted("both16", 24, 24)
    ctx = context(inp)
    for thr in thresholds(lm.lane_window(inp.M, 24, 24, 3, 0, "u16")):
        st = check_allpairs(ctx, inp, 3, 0, thr, "both16", rows="none")
        assert st.classes_u8 == 0
    ctx.close()


# ---- (e) row-bound split ------------------------------------------------------------------------------------------------------------------------

def bound_case(L):
    X, thr, _ = lm.uniform_defaults(L)
    return X, 0, thr


def bound_extra(L):
    def build(M):
        X, p, thr = bound_case(L)
        limit = lm.u8_row_limit(M, L, L, X, p, thr)
        at, at_partner = lm.bound_exact_pair(M, L, limit)
        over, over_partner = lm.bound_exact_pair(M, L, limit + 1)
        return [("at_limit", [at]), ("at_limit_partner", [at_partner]), ("over_limit", [over]), ("over_limit_partner", [over_partner])]
    return build


EXTRA = {"bound15": bound_extra(15), "bound20": bound_extra(20)}


@pytest.mark.parametrize("L", [15, 20])
def test_bound_exact_rows_sit_on_the_row_limit(L):
    inp = planted("b62s", L, L, f"bound{L}")
    X, p, thr = bound_case(L)
    M = inp.M
    assert lm.lane_path(M, L, L, X, p, thr) == "u16"
    limit = lm.u8_row_limit(M, L, L, X, p, thr)
    assert limit == 127 + thr and 128 - thr + limit == 255
    for name, bound in (("at_limit", limit), ("over_limit", limit + 1)):
        row, partner = int(inp.idx[name][0]), int(inp.idx[name + "_partner"][0])
        assert lm.row_bound(M, inp.seqs[row]) == bound == lm.row_bound(M, inp.seqs[partner])
        assert inp.block(X, p)[row, partner] == bound == inp.block(X, p)[partner, row]       # the partner reaches the bound
    bounds = np.array([lm.row_bound(M, s) for s in inp.seqs])
    assert (bounds < limit).sum() >= N_ORDINARY and (bounds > limit + 1).sum() >= N_TOP
    assert lm.allpairs_tiers(M, inp.seqs, X, p, thr) == {"u8": 1, "u16": 1, "direct": 0}


@pytest.mark.gpu
@pytest.mark.parametrize("L", [15, 20])
def test_row_bound_split_at_the_row_limit(gpu, L):
    """build_plan's refine at the reference's defaults: the row whose bound IS the limit runs on 8-bit lanes and its partner takes
    its lane to 255; the row one past the limit runs on 16-bit lanes"""
    inp = planted("b62s", L, L, f"bound{L}")
    X, p, thr = bound_case(L)
    ctx = context(inp)
    st = check_allpairs(ctx, inp, X, p, thr, ("bound", L))
    assert st.classes_u8 > 0 and st.classes_u16 > 0
    ctx.close()


# ---- (f) rectangle and triangle plans ----------------------------------------------------------------------------------------------------------

RECT = [("b62s", 12, 12, 3, 0), ("b62s", 7, 7, 2, 0), ("b62s", 14, 12, 3, -1)]
RECT_IDS = [f"{la}-{lb}" for _, la, lb, _, _ in RECT]


def rect_split(inp):
    """queries = the first 2/5 of the set, references = the rest"""
    cut = inp.n * 2 // 5
    return (0, cut), (cut, inp.n)


def rect_tiers(inp, q, r, X, p, thr):
    lens = np.array([len(s) for s in inp.seqs])
    out = {"u8": 0, "u16": 0, "direct": 0}
    for lq in np.unique(lens[q[0]:q[1]]):
        for lr in np.unique(lens[r[0]:r[1]]):
            out[lm.lane_path(inp.M, int(lq), int(lr), X, p, thr)] += 1
    return out


@pytest.mark.parametrize("case", RECT, ids=RECT_IDS)
def test_rect_split_keeps_an_edge_pair_on_either_side(case):
    """a pair at the top of its lane and a pair at the bottom with one word among the queries and one among the references"""
    mat, la, lb, X, p = case
    inp = planted(mat, la, lb)
    (q0, q1), (r0, r1) = rect_split(inp)
    lo, hi = lm.lane_window(inp.M, la, lb, X, p, "u8")
    i, j, sc = inp.pairs("top_long", "top_short", X, p)
    across = ((i < q1) & (j >= r0)) | ((j < q1) & (i >= r0))
    assert (128 - lo + sc[across] == 255).any()
    bi, bj = int(inp.idx["bot_row"][0]), inp.idx["bot_col"]
    assert ((bi < q1) != (bj < q1)).any()


@pytest.mark.gpu
@pytest.mark.parametrize("case", RECT, ids=RECT_IDS)
def test_rect_and_triangle_plans_at_the_lane_edges(gpu, case):
    """no row-bound refinement: a class past its window goes to 16-bit lanes whole"""
    mat, la, lb, X, p = case
    inp = planted(mat, la, lb)
    q, r = rect_split(inp)
    blk = inp.block(X, p)
    ctx = context(inp)
    for thr in thresholds(lm.lane_window(inp.M, la, lb, X, p, "u8")):
        for a, b in ((q, r), (r, q)):
            edges, st = ctx.search_shifted(*a, *b, X, p, thr)
            sub = blk[a[0]:a[1], b[0]:b[1]]
            qi, ri = np.nonzero(sub >= thr)
            want = np.sort(hammock_amd.pack_edges(b[0] + ri, a[0] + qi, sub[qi, ri]))
            tiers = rect_tiers(inp, a, b, X, p, thr)
            assert np.array_equal(np.sort(edges), want), (case, thr, a, len(edges), len(want))
            assert (st.classes_u8, st.classes_u16, st.classes_direct) == (tiers["u8"], tiers["u16"], tiers["direct"]), (case, thr, a)
            if la == lb:
                assert st.classes_rows == st.classes_u8
        i, j = np.nonzero(np.triu(blk >= thr, 1))
        want = np.sort(hammock_amd.pack_edges(i, j, blk[i, j]))
        got = ctx.cluster_pairs_shifted(0, inp.n, np.arange(inp.n), inp.n, X, p, thr)
        assert ctx.last_merge_stats.n_edges == len(want), (case, thr)
        assert np.array_equal(np.sort(got), want), (case, thr, len(got), len(want))
    ctx.close()


# ---- (g) counting instantiations -----------------------------------------------------------------------------------------------------------------

GREEDY_MAX_CLUSTERS = 40


def oracle_greedy(inp, X, p, thr, maxc):
    """-> (cluster ids, result order, member ranks), or (crash case, crash index) where the reference itself would fail"""
    st, cid, order, stats = c_oracle.greedy_cluster(inp.M, inp.res, inp.off, None, 0, X, p, thr, maxc, 8)
    if st == c_oracle.HMO_ERR_REFERENCE_WOULD_CRASH:
        return stats.crash_case, stats.crash_index
    assert st == 0, (st, thr)
    return cid, order, stats.member_rank


def check_greedy(ctx, inp, X, p, thr, maxc, what):
    want = oracle_greedy(inp, X, p, thr, maxc)
    if len(want) == 2:       # the reference's failure is part of the contract: the same case at the same sequence
        with pytest.raises(hammock_amd.ReferenceWouldCrash) as e:
            ctx.greedy_cluster(X, p, thr, maxc)
        assert (e.value.case, e.value.index) == want, (what, thr)
        return
    ocid, oorder, orank = want
    cid, order, _ = ctx.greedy_cluster(X, p, thr, maxc)
    assert np.array_equal(cid, ocid) and np.array_equal(order, oorder), (what, thr)
    assert np.array_equal(ctx.member_rank[:inp.n], orank), (what, thr)


@pytest.mark.parametrize("L", [12, 7])
def test_greedy_inputs_cluster_at_both_edges(L):
    """the oracle clusters the planted inputs at thr_lo and thr_hi, the top words inside clusters; the one exception is stated: at
    the 7-mers' thr_hi, 100, no pair is a hit (the top is 77) and the reference fails at the first sequence -- the GPU call must
    fail the same way"""
    inp = planted("b62s", L, L)
    X = lm.uniform_defaults(L)[0]
    for thr in lm.lane_window(inp.M, L, L, X, 0, "u8"):
        got = oracle_greedy(inp, X, 0, thr, GREEDY_MAX_CLUSTERS)
        if L * inp.M.max() < thr:
            assert got == (1, 0)
            continue
        cid, order, _ = got
        assert len(order) > 0 and (cid[inp.idx["top_long"]] >= 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("L", [12, 7])
def test_greedy_counting_kernels_at_the_lane_edges(gpu, L):
    """a clustering call's pass runs the degree-counting instantiations (EDGES_COUNT): ids, order and member rank are the oracle's"""
    inp = planted("b62s", L, L)
    X = lm.uniform_defaults(L)[0]
    ctx = context(inp)
    for thr in lm.lane_window(inp.M, L, L, X, 0, "u8"):
        check_greedy(ctx, inp, X, 0, thr, GREEDY_MAX_CLUSTERS, ("greedy", L))
    ctx.close()


# ---- (h) fields after the pass ----------------------------------------------------------------------------------------------------------------------

X3_TOP = 396                      # a pair of 12-mer top words under b62s_x3
ADJ_THR = X3_TOP - 255            # 141: the top pairs' adjacency entries hold 255; one less and entries are 8 bytes


def competitors(M, L=12):
    """two words that score against a top word above the threshold but below the top: the all-original top word with its last 3 and
    its last 6 residues replaced by F (under b62s_x3 against a 12-mer top word: 306 and 216, score - ADJ_THR = 165 and 75 -- one
    with the byte's top bit set, one without)"""
    o, _ = lm.top_residues(M)
    hi, lo = np.full(L, o, dtype=np.uint8), np.full(L, o, dtype=np.uint8)
    hi[L - 3:] = lo[L - 6:] = lm.code("F")
    return hi, lo


def adjacency_extra(M):
    a, b = lm.score_exact_pair(M, 12, ADJ_THR, 3, 0)
    hi, lo = competitors(M)
    return [("rel0_a", [a]), ("rel0_b", [b]), ("rival_hi", [hi]), ("rival_lo", [lo])]


def reference_choice(rel_by_id, byte=lambda r: r):
    """the first sequence's partner by the reference's order over singletons of one size: the best score, then the smaller id;
    byte: how a (mis)reading turns score - threshold into the value compared"""
    return max(rel_by_id, key=lambda k: (byte(rel_by_id[k]), -k))


def as_signed_byte(r):
    return r - 256 if r >= 128 else r


EXTRA["adjacency"] = adjacency_extra


def test_adjacency_input_holds_rel_0_255_and_256():
    inp = planted("b62s_x3", 12, 12, "adjacency")
    blk = inp.block(3, 0)
    assert blk.max() == X3_TOP == 12 * inp.M.max()
    a, b = int(inp.idx["rel0_a"][0]), int(inp.idx["rel0_b"][0])
    assert blk[a, b] == ADJ_THR == blk[b, a]
    rel = blk[np.tril_indices(inp.n, -1)].astype(np.int64)
    assert (rel - ADJ_THR == 0).any() and (rel - ADJ_THR == 255).any() and not (rel - ADJ_THR > 255).any()
    assert (rel - (ADJ_THR - 1) == 256).any()
    assert lm.adjacency_packed(12, 12, int(inp.M.max()), 0, 3, ADJ_THR) and not lm.adjacency_packed(12, 12, int(inp.M.max()), 0, 3, ADJ_THR - 1)
    # the first sequence, a top word, chooses among top words at 255 and two rivals at 165 and 75: a byte read as signed, or the
    # smaller id alone, would choose a rival
    nbr = {int(k): int(blk[0, k]) - ADJ_THR for k in np.flatnonzero(blk[0] >= ADJ_THR) if k != 0}
    hi, lo = int(inp.idx["rival_hi"][0]), int(inp.idx["rival_lo"][0])
    tops = [k for k in nbr if nbr[k] == 255]
    assert 0 in inp.idx["top_long"] and 128 <= nbr[hi] < 255 and 0 < nbr[lo] < 128
    chosen = reference_choice(nbr)
    assert chosen == min(tops) and reference_choice(nbr, as_signed_byte) == lo and min(nbr) in (hi, lo)
    for thr in (ADJ_THR, ADJ_THR - 1):
        cid, order, rank = oracle_greedy(inp, 3, 0, thr, 10)
        assert len(order) > 0 and (cid[inp.idx["top_long"]] >= 0).all()      # a clustering, not a reference failure
        assert cid[0] == cid[chosen] and (rank[0], rank[chosen]) == (0, 1)    # the oracle's first cluster is {0, chosen}


@pytest.mark.gpu
def test_adjacency_entries_at_rel_0_255_and_256(gpu):
    """threshold top - 255: 4-byte entries m << 8 | score - threshold with a pair at 255 and a pair at 0; top - 256: the call must
    switch to 8-byte entries.  Both clusterings are the oracle's, and so are the edges.  The first sequence's choice of partner depends
    on the byte's value: rivals at 165 and 75 with smaller ids stand against the top words at 255."""
    inp = planted("b62s_x3", 12, 12, "adjacency")
    with saved_env({}):      # (an inherited HMK_ADJ_8BYTE would turn both thresholds into the 8-byte path)
        ctx = context(inp)
        for thr in (ADJ_THR, ADJ_THR - 1):
            check_greedy(ctx, inp, 3, 0, thr, 10, "adjacency")
            check_allpairs(ctx, inp, 3, 0, thr, "adjacency", rows="none")
        ctx.close()


BAND_N, BAND_MAX_CLUSTERS = 16384, 3
BAND_ROWS = 2 * BAND_MAX_CLUSTERS + 1024
# Band row 0 is a top word whose ONLY neighbour at 255 is the other top word, far beyond the band at the set's last index; two rivals
# (competitors()) with smaller ids, also beyond the band, are its neighbours at 165 and 75.  Row 0 has no neighbour inside the band,
# so its partner is the first of its far candidates in key order (k_edges.hip, band_far_key: score - threshold in the top byte, then
# size, then the smaller id): the last sequence -- a key whose top byte were read as signed, or cut, or left out would name a rival.
# Two more families over one synonym pair each (any two of a family score 180 and 144 under b62s_x3) form clusters at rows 10 and 20,
# so phase 1 stops at max_clusters inside the band.
BAND_TOP, BAND_FAR_TOP, BAND_RIVAL_HI, BAND_RIVAL_LO = 0, BAND_N - 1, 2000, 3000
BAND_FAMILIES = {("K", "Z"): [10, 900, 2500, 12000], ("I", "X"): [20, 1000, 5000, 15000]}

_band = []


def band_input():
    """16,384 12-mers (the smallest set that gets a band): synthetic ones with the words above planted -> (matrix, residues, offsets)"""
    if not _band:
        M = matrix("b62s_x3")
        res, off = synth_peptides(77, BAND_N, 12)
        rows = res.reshape(BAND_N, 12).copy()
        rows[BAND_TOP], rows[BAND_FAR_TOP] = lm.top_words(M, 12, 2, np.random.default_rng(3), (5, 6))
        rows[BAND_RIVAL_HI], rows[BAND_RIVAL_LO] = competitors(M)
        for pair, spots in BAND_FAMILIES.items():
            for k, w in zip(spots, lm.top_words(M, 12, len(spots), np.random.default_rng(3), (5, 6), pair)):
                rows[k] = w
        assert len(np.unique(rows.view(np.dtype((np.void, 12))))) == BAND_N
        _band.append((M, np.ascontiguousarray(rows.reshape(-1)), off))
    return _band[0]


def band_oracle():
    M, res, off = band_input()
    if len(_band) == 1:
        st, cid, order, stats = c_oracle.greedy_cluster(M, res, off, None, 0, 3, 0, ADJ_THR, BAND_MAX_CLUSTERS, 16)
        assert st == 0
        _band.append((cid, order, stats.member_rank))
    return _band[1]


def test_band_row_chooses_the_far_candidate_at_255():
    """by the oracle: row 0's neighbours are the two rivals and the last sequence, all beyond the band; the reference pairs it with
    the last sequence, and would not under a key that misread the byte or ordered by id alone"""
    M, res, off = band_input()
    assert BAND_ROWS * 2 <= BAND_N and BAND_N >= 16384 and BAND_MAX_CLUSTERS > 0        # band_request gives a band of BAND_ROWS rows
    others = np.arange(1, BAND_N, dtype=np.uint32)
    st, sc = c_oracle.score_pairs(M, res, off, np.zeros(len(others), np.uint32), others, 0, 3, 0)
    assert st == 0
    nbr = {int(k): int(s) - ADJ_THR for k, s in zip(others, sc) if s >= ADJ_THR}
    # (a few synthetic peptides rich in W are neighbours too, at small values; none inside the band, none at 255)
    assert {BAND_RIVAL_HI, BAND_RIVAL_LO, BAND_FAR_TOP} <= set(nbr) and min(nbr) >= BAND_ROWS
    assert [k for k in nbr if nbr[k] == 255] == [BAND_FAR_TOP] and max(nbr) == BAND_FAR_TOP
    assert 128 <= nbr[BAND_RIVAL_HI] < 255 and 0 < nbr[BAND_RIVAL_LO] < 128
    assert reference_choice(nbr) == BAND_FAR_TOP
    assert reference_choice(nbr, as_signed_byte) != BAND_FAR_TOP and reference_choice(nbr, lambda r: 0) == BAND_RIVAL_HI
    assert lm.adjacency_packed(12, 12, int(M.max()), 0, 3, ADJ_THR)
    cid, order, rank = band_oracle()
    assert cid[BAND_TOP] == cid[BAND_FAR_TOP] >= 0 and (rank[BAND_TOP], rank[BAND_FAR_TOP]) == (0, 1)     # the cluster {0, last}
    assert rank[BAND_RIVAL_HI] != 1 or cid[BAND_RIVAL_HI] != cid[BAND_TOP]
    families = [set(cid[np.array(v)].tolist()) for v in BAND_FAMILIES.values()]
    assert all(len(f) == 1 for f in families) and len(set.union(*families) | {int(cid[BAND_TOP])}) == BAND_MAX_CLUSTERS


@pytest.mark.gpu
def test_band_candidate_keys_carry_255(gpu):
    """a clustering call with a band (asserted: band bytes were shipped): rows below 2 * max_clusters + 1,024 are launched first, and
    the candidates beyond them are keyed by entry & 0xFF in the top byte.  Row 0's partner is its far candidate at 255, the set's
    last sequence, against rivals at 165 and 75 with smaller ids."""
    M, res, off = band_input()
    ocid, oorder, orank = band_oracle()
    with saved_env({}):      # (no inherited HMK_NO_BAND)
        ctx = hammock_amd.Context(M, device=0)
        ctx.set_sequences(residues=res, offsets=off)
        cid, order, _ = ctx.greedy_cluster(3, 0, ADJ_THR, BAND_MAX_CLUSTERS)
        assert ctx.greedy_phases()["band_bytes"] > 0
        assert np.array_equal(cid, ocid) and np.array_equal(order, oorder)
        assert np.array_equal(ctx.member_rank[:BAND_N], orank)
        assert cid[BAND_TOP] == cid[BAND_FAR_TOP] and (ctx.member_rank[BAND_TOP], ctx.member_rank[BAND_FAR_TOP]) == (0, 1)
        ctx.close()


@pytest.mark.gpu
def test_row_blocks_at_rel_255_and_256(gpu):
    """hmk_pack_rows_dev / hmk_unpack_rows_dev: with the largest score - threshold at 255 no entry is a misfit and the round trip is
    exact; at 256 the misfits are counted, exactly the top pairs"""
    import torch
    from hammock_amd import _native as N
    inp = planted("b62s_x3", 12, 12, "adjacency")
    ctx = context(inp)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    for thr in (ADJ_THR, ADJ_THR - 1):
        want = inp.edges(3, 0, thr)
        rel = hammock_amd.edge_fields(want)[2].astype(np.int64) - thr
        cap = (len(want) * 2 // N.HMK_EDGE_SHARDS + 4096) * N.HMK_EDGE_SHARDS
        d_edges = torch.empty(cap, dtype=torch.int64, device=dev)
        d_counts = torch.zeros(N.HMK_EDGE_SHARDS, dtype=torch.int64, device=dev)
        ctx.neighbors_shifted_dev(3, 0, thr, 0, 1, d_edges.data_ptr(), cap, d_counts.data_ptr(), stream.cuda_stream)
        head = torch.zeros(inp.n + 2, dtype=torch.int32, device=dev)
        adj = torch.zeros(len(want) + 8, dtype=torch.int32, device=dev)
        ctx.pack_rows_dev(d_edges.data_ptr(), cap, d_counts.data_ptr(), thr, head.data_ptr(), adj.data_ptr(), adj.numel(), stream.cuda_stream)
        h = head.cpu().numpy()
        assert h[inp.n] == len(want)
        if thr == ADJ_THR:
            assert rel.max() == 255 and rel.min() == 0 and h[inp.n + 1] == 0
            out = torch.zeros(len(want), dtype=torch.int64, device=dev)
            ctx.unpack_rows_dev(head.data_ptr(), adj.data_ptr(), thr, out.data_ptr(), out.numel(), stream.cuda_stream)
            assert np.array_equal(np.sort(out.cpu().numpy().view(np.uint64)), want)
        else:
            assert rel.max() == 256 and h[inp.n + 1] == int((rel > 255).sum()) > 0
    ctx.close()


# ---- (i) the int16 of a packed edge -----------------------------------------------------------------------------------------------------------------

# A pass is refused when max_len * max + max(0, p) * (max_len - min_len + 2 X) exceeds 32767.  A score of exactly 32767 cannot be
# produced through the API: it would need max_len * max == 32767 on an unshifted plane (a positive penalty is only paid on planes
# with fewer cells), and with lengths up to 32 that is 31 * 1,057 alone -- a context refuses matrix entries beyond +-1,000.  So:
# the largest score there is, 32 * 1,000 = 32,000, in the edges; a set whose bound is exactly 32,767 (lengths 32 and 25, X = 3,
# p = 59: 32,000 + 59 * 13) accepted and exact; a set whose bound is 32,768 (lengths 32 and 26, p = 64: 32,000 + 64 * 12) refused.
I16_LENS, I16_X, I16_P = (32, 25), 3, 59
I16_OVER_LENS, I16_OVER_P = (32, 26), 64


def int16_bound(M, lens, X, p):
    """check_shift_threshold_scores (hmk_plan.cpp)"""
    return max(lens) * max(0, int(M.max())) + max(0, p) * ((max(lens) - min(lens)) + 2 * X)


def test_int16_inputs_sit_on_the_bound():
    M = matrix("i16")
    assert all(32767 % L or 32767 // L > 1000 for L in range(1, 33))      # no length * entry a context accepts is 32767
    assert int16_bound(M, I16_LENS, I16_X, I16_P) == 32767 and int16_bound(M, I16_OVER_LENS, I16_X, I16_OVER_P) == 32768
    inp = planted("i16", *I16_LENS)
    for p in (0, I16_P):
        blk = inp.block(I16_X, p)
        i, j, sc = inp.pairs("top_long", "top_long", I16_X, p)
        assert blk.max() == 32000 and (sc == 32000).all()
        assert lm.allpairs_tiers(M, inp.seqs, I16_X, p, 30000) == {"u8": 0, "u16": 0, "direct": 3}


@pytest.mark.gpu
def test_int16_edge_scores_up_to_the_bound(gpu):
    """the largest score the API can produce, 32,000, is carried by the edges of the top words' pairs, at p = 0 and in a set whose
    bound is exactly 32,767; a bound of 32,768 is refused by every shifted pass"""
    inp = planted("i16", *I16_LENS)
    ctx = context(inp)
    for p in (0, I16_P):
        for thr in (30000, 40):
            st = check_allpairs(ctx, inp, I16_X, p, thr, ("int16", p), rows="none")
            assert st.classes_direct == 3
        edges, _ = ctx.neighbors_shifted(I16_X, p, 30000)
        assert (hammock_amd.edge_fields(edges)[2] == 32000).sum() == N_TOP * (N_TOP - 1) // 2
    q, r = rect_split(inp)
    edges, _ = ctx.search_shifted(*q, *r, I16_X, I16_P, 30000)
    blk = inp.block(I16_X, I16_P)[q[0]:q[1], r[0]:r[1]]
    qi, ri = np.nonzero(blk >= 30000)
    assert len(qi) > 0 and np.array_equal(np.sort(edges), np.sort(hammock_amd.pack_edges(r[0] + ri, q[0] + qi, blk[qi, ri])))
    ctx.close()
    rng = np.random.default_rng(1)
    over = hammock_amd.Context(inp.M, device=0)
    over.set_sequences(lm.top_words(inp.M, I16_OVER_LENS[0], 3, rng) + lm.top_words(inp.M, I16_OVER_LENS[1], 3, rng))
    with pytest.raises(ValueError, match="int16"):
        over.neighbors_shifted(I16_X, I16_OVER_P, 30000)
    with pytest.raises(ValueError, match="int16"):
        over.search_shifted(0, 3, 3, 6, I16_X, I16_OVER_P, 30000)
    edges, _ = over.neighbors_shifted(I16_X, I16_OVER_P - 1, 30000)       # (32,000 + 63 * 12 = 32,756: fine)
    assert len(edges) > 0
    over.close()
