"""The cluster-level calls at both ends of their int16 score fields.

tests/test_score_field_edges.py takes every narrowing of the neighbour pass to the edge of its field.  The calls built on that pass
narrow a score again -- the 16-bit field of a slot's key (k_linkage.hip), the int16 of the dense triangles (k_split.hip), the int16 read
back out of a packed edge (k_assign.hip, k_search.hip), the 32-bit field of the table and selection keys (k_assign_table.h, k_search.hip,
k_survey.hip), the int32 LDS partial sums and the 64-bit two's-complement adds of k_align.hip, the bins of k_survey.hip -- and every other
file scores with BLOSUM62: +-150 at the most.  A signedness or one-unit slip in any of them shows only where the biased field has its
top bit set (score >= 0) AND where the score is far below zero.  Here the matrix is synonym-BLOSUM62 with the W/B block at 1,000 and C
against D, E, N, Q at -1,000 (the largest entries a context accepts), so that two distinct top words of length L score L x 1,000 and
C^L against a word over {D, E, N, Q} scores -L x 1,000: 32,000 and -32,000 at L = 32, and at L = 30 exactly the thresholds' limits.

Best-k runs at k = 1, 3 and 32: 32 is the largest k hmk_search_best_shifted takes (a larger one is refused, which is asserted too).

The CPU tests (unmarked) prove with the C oracle that the inputs hold what the GPU cases claim.  The GPU tests (-m gpu, an MI355X) take
their inputs from the same cached builders and compare bit for bit with the expectations the owning files compute from the oracle.
"""
import functools
import json
import os
import time

import numpy as np
import pytest

from conftest import GOLDEN
from test_assign import gpu   # noqa: F401  (the fixture that skips where no HIP device is visible)
from test_host_greedy import oracle_edges
from test_split import oracle_split, same
from test_work_loops import capped, cut, link_grids
import test_align as AL
import test_assign as A
import test_linkage as LK
import test_match as MA
import test_merge as ME
import test_search as S
import test_survey as SV

import hammock_amd
from hammock_amd import _native as N
import lane_model as lm
from oracle import c_oracle

INT32_MAX = 2 ** 31 - 1
THR_LIMIT = 30000                      # check_shift_threshold_scores: thresholds outside [-30000, 30000] are refused
PARAMS = [(0, 0), (3, -1)]             # (max shift, shift penalty)
PARAM_IDS = ["X0_p0", "X3_p-1"]
LENGTHS = [32, 30]
LINK_FLAT_MAX = 256
SLOTS = ("top256", "neg256", "top300", "neg300", "plain", "pair_top", "pair_neg")     # slot numbers: the flat pair space runs in this order
SLOT_SIZES = (256, 256, 300, 300, 60, 2, 2)
BEST_K_MAX = 32                        # hmk_search_best_shifted takes k = 1 .. 32


# ---- the matrix ---------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def ends_matrix():
    """ends16: synonym-BLOSUM62 with the W/B block at 1,000 and C against D, E, N, Q at -1,000, both ways"""
    with open(os.path.join(GOLDEN, "matrices.json")) as fh:
        M = lm.with_synonyms(np.asarray(json.load(fh)["matrices"]["blosum62"], dtype=np.int32))
    top = [lm.code("W"), lm.code("B")]
    M[np.ix_(top, top)] = 1000
    for y in "DENQ":
        M[lm.code("C"), lm.code(y)] = M[lm.code(y), lm.code("C")] = -1000
    M.setflags(write=False)
    return M


def int16_top(lens, X, p):
    """check_shift_threshold_scores (hmk_plan.cpp): the largest score the set can reach"""
    return max(lens) * max(0, int(ends_matrix().max())) + max(0, p) * ((max(lens) - min(lens)) + 2 * X)


def int16_bottom(lens, X, p):
    """check_link_scores (hmk_linkage.cpp): the smallest"""
    return max(lens) * min(0, int(ends_matrix().min())) + min(0, p) * ((max(lens) - min(lens)) + 2 * X)


# ---- inputs -------------------------------------------------------------------------------------------------------------------------

class Planted:
    def __init__(self, seqs, **kw):
        self.M, self.seqs, self.n = ends_matrix(), seqs, len(seqs)
        self.res, self.off = hammock_amd.pack_sequences(seqs)
        self.__dict__.update(kw)
        for v in self.__dict__.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)


@functools.lru_cache(maxsize=None)
def ends_set(L):
    """1,176 words of length L in one shuffled order, in the seven slots of SLOTS: top* hold distinct top words (any two score
    L x 1,000), neg* distinct words over {D, E, N, Q} and one C^L, plain ordinary peptides, the pairs two top words and a bottom word
    with C^L.  C^L is a string of its own: it is there three times (the copies precedent of test_align), everything else is distinct.
    In neg256 C^L is the slot's largest index -- the last row of the slot's triangle, 255 consecutive pairs of the flat pair space, which
    top256's 32,640 pairs ahead of it put into ONE chunk of 256; in neg300 it sits at a middle place."""
    M = ends_matrix()
    rng = np.random.default_rng(16_000 + L)
    tops = lm.top_words(M, L, 256 + 300 + 2, rng)
    (c_word,), cols = lm.bottom_words(M, L, L, 255 + 299 + 1, rng)
    assert c_word.tolist() == [lm.code("C")] * L and len(cols) == 555
    plain = lm.ordinary(rng, 60, [L], avoid=tops + cols + [c_word])
    groups = [tops[:256], cols[:255] + [c_word.copy()], tops[256:556], cols[255:554] + [c_word.copy()], plain, tops[556:],
              [cols[554], c_word.copy()]]
    words = [w for g in groups for w in g]
    slot = np.repeat(np.arange(len(groups)), [len(g) for g in groups])
    perm = rng.permutation(len(words))
    words, mc = [words[k] for k in perm], slot[perm].astype(np.uint32)
    is_c = np.array([np.array_equal(w, c_word) for w in words])
    c_at = {}
    for name, place in (("neg256", -1), ("neg300", 150), ("pair_neg", None)):
        m = np.flatnonzero(mc == SLOTS.index(name))
        src = int(m[is_c[m]][0])
        dst = src if place is None else int(m[place])
        words[src], words[dst] = words[dst], words[src]
        is_c[src], is_c[dst] = is_c[dst], is_c[src]
        c_at[name] = dst
    return Planted(words, L=L, mc=mc, ncl=len(SLOTS), c_at=c_at, is_c=is_c)


def slot(name):
    return SLOTS.index(name)


@functools.lru_cache(maxsize=None)
def triangle(L, X, p):
    """int64 [n, n] of ends_set(L): entry (a, b) and (b, a), a > b, = the oracle's score(seq1 = a, seq2 = b)"""
    e = ends_set(L)
    hi, lo = np.tril_indices(e.n, -1)
    st, sc = c_oracle.score_pairs(e.M, e.res, e.off, hi, lo, 0, X, p)
    assert st == 0
    T = np.zeros((e.n, e.n), dtype=np.int64)
    T[hi, lo] = sc
    T[lo, hi] = sc
    T.setflags(write=False)
    return T


@functools.lru_cache(maxsize=None)
def inside(L, X, p):
    """(a, b, slot, score) of the pairs inside the slots, a < b, seq1 = b: test_linkage.score_inside's, read out of triangle()"""
    a, b, sl = LK.inside_pairs(ends_set(L).mc)
    out = (a, b, sl, triangle(L, X, p)[b, a])
    for arr in out:
        arr.setflags(write=False)
    return out


def flat_chunks(mc):
    """the flat pair space as k_linkage_flat / k_align_sums_flat walk it (build_link_tables, tri_entry): the slots of 2 .. 256 members
    in slot order, a slot's pairs by row (the larger place) then column -> (a, b, chunk of 256 consecutive pairs)"""
    aa, bb = [], []
    for c in range(int(mc.max()) + 1):
        m = np.flatnonzero(mc == c)
        if 2 <= m.size <= LINK_FLAT_MAX:
            row, col = np.tril_indices(m.size, -1)
            aa.append(m[col])
            bb.append(m[row])
    a, b = np.concatenate(aa), np.concatenate(bb)
    return a, b, np.arange(a.size) // 256


def swapped_slots(mc):
    """the slot numbers of top256 and neg256 exchanged: neg256's pairs start the flat pair space, and top256's last row is one chunk's"""
    return np.array([1, 0, 2, 3, 4, 5, 6], dtype=np.uint32)[mc]


@functools.lru_cache(maxsize=None)
def mixed_set():
    """the L = 32 and L = 30 families together, for the rectangle calls.  Queries (the new sequences) first: two top 32-mers, C^30, an
    ordinary 32-mer and 30-mer, C^32, a top 30-mer.  Then the clusters, each contiguous, its members shuffled: A 40 top 32-mers, B 40
    top 30-mers, D 40 words over {D, E, N, Q} of length 30, O 20 ordinary peptides.  All strings distinct."""
    M = ends_matrix()
    rng = np.random.default_rng(16_100)
    t32, t30 = lm.top_words(M, 32, 42, rng), lm.top_words(M, 30, 41, rng)
    (c30,), d30 = lm.bottom_words(M, 30, 30, 40, rng)
    (c32,), _ = lm.bottom_words(M, 32, 30, 1, rng)
    plain = lm.ordinary(rng, 22, [30, 32], avoid=t32 + t30 + d30 + [c30, c32])
    o32 = next(w for w in plain if len(w) == 32)
    o30 = next(w for w in plain if len(w) == 30)
    rest = [w for w in plain if w is not o32 and w is not o30]
    queries = [t32[40], t32[41], c30, o32, o30, c32, t30[40]]
    clusters = [t32[:40], t30[:40], d30, rest]
    members = [g[k] for g in clusters for k in rng.permutation(len(g))]
    mc = np.repeat(np.arange(4), [len(g) for g in clusters]).astype(np.uint32)
    seqs = queries + members
    assert len({w.tobytes() for w in seqs}) == len(seqs)
    nq = len(queries)
    start = nq + np.concatenate([[0], np.cumsum([len(g) for g in clusters])])
    return Planted(seqs, nq=nq, mc=mc, ids=np.array([40, 10, 30, 20], dtype=np.int32), sizes=np.ones(len(members), dtype=np.int32),
                   q={"top32": 0, "top32_b": 1, "c30": 2, "plain32": 3, "plain30": 4, "c32": 5, "top30": 6},
                   qc=np.array([0, 0, 1, 2, 3, 4, 5], dtype=np.uint32), start=start)


@functools.lru_cache(maxsize=None)
def mixed_block(X, p):
    """[members, queries] of score(seq1 = member, seq2 = query): the orientation of assign and match"""
    m = mixed_set()
    blk = A.block(c_oracle, m.M, m.res, m.off, (0, m.nq), (m.nq, m.n), 0, X, p)
    blk.setflags(write=False)
    return blk


@functools.lru_cache(maxsize=None)
def neg_rect_set():
    """three copies of C^32, then ends_set(32)'s 299 bottom words of neg300: every pair of the rectangle scores -32,000 at X = 0"""
    e = ends_set(32)
    m = np.flatnonzero((e.mc == slot("neg300")) & ~e.is_c)
    c = e.seqs[e.c_at["neg300"]]
    return Planted([c.copy(), c.copy(), c.copy()] + [e.seqs[k] for k in m], nq=3)


@functools.lru_cache(maxsize=None)
def small_set():
    """32-mers for the accepted / refused penalties: 12 top words, 11 bottom words with C^32, 9 ordinary peptides, in three slots"""
    M = ends_matrix()
    rng = np.random.default_rng(16_200)
    tops = lm.top_words(M, 32, 12, rng)
    (c_word,), cols = lm.bottom_words(M, 32, 32, 11, rng)
    plain = lm.ordinary(rng, 9, [32], avoid=tops + cols + [c_word])
    words = tops + cols + [c_word] + plain
    perm = rng.permutation(len(words))
    mc = np.repeat([0, 1, 2], [12, 12, 9])[perm].astype(np.uint32)
    return Planted([words[k] for k in perm], mc=mc, ncl=3)


# ---- the premises, proven on the CPU ------------------------------------------------------------------------------------------------

def test_the_matrix_is_symmetric_and_a_context_accepts_it():
    M = ends_matrix()
    assert (M == M.T).all() and M.min() == -1000 and M.max() == 1000
    assert lm.top_residues(M) == (lm.code("W"), lm.code("B"))
    ctx = hammock_amd.Context(M, device=-1)
    ctx.set_sequences(residues=small_set().res, offsets=small_set().off)
    ctx.close()


@pytest.mark.parametrize("L", LENGTHS)
def test_ends_sets_hold_both_ends(L):
    e = ends_set(L)
    top, bot = L * 1000, -L * 1000
    assert np.bincount(e.mc).tolist() == list(SLOT_SIZES) and e.n == 1176
    strings = [w.tobytes() for w in e.seqs]
    assert len(set(strings)) == e.n - 2 and e.is_c.sum() == 3 and all(len(w) == L for w in e.seqs)
    n256, n300 = np.flatnonzero(e.mc == slot("neg256")), np.flatnonzero(e.mc == slot("neg300"))
    assert e.c_at["neg256"] == n256.max() and n300[100] < e.c_at["neg300"] < n300[200]
    for X, p in PARAMS:
        a, b, sl, sc = inside(L, X, p)
        assert sc.size == 2 * (256 * 255 // 2 + 300 * 299 // 2) + 60 * 59 // 2 + 2 == 156_752
        (min_score, _, _, _, member_min, _), _ = LK.reduce_scores(a, b, sl, sc, e.n, e.ncl, 0)
        shifted_bottom = -(L - 3) * 1000 - 6     # C^L against a bottom word at (3, -1): 3 cells fewer, 2 x 3 penalties
        for name in ("top256", "top300", "pair_top"):
            assert (sc[sl == slot(name)] == top).all() and min_score[slot(name)] == top
        for name in ("neg256", "neg300", "pair_neg"):
            c = e.c_at[name]
            with_c = (sl == slot(name)) & ((a == c) | (b == c))
            assert with_c.sum() == SLOT_SIZES[slot(name)] - 1
            assert (sc[with_c] == (bot if X == 0 else shifted_bottom)).all()
            assert min_score[slot(name)] == (bot if X == 0 else shifted_bottom) == member_min[c]
            assert sc[(sl == slot(name)) & ~with_c].min(initial=0) > -300      # the bottom words among themselves: about +60
        assert np.abs(sc[sl == slot("plain")]).max() < 20000 and sc[sl == slot("plain")].min() < 0
        # every member sum of neg256 is negative, C^L's the most
        sums = np.zeros(e.n, dtype=np.int64)
        np.add.at(sums, a, sc)
        np.add.at(sums, b, sc)
        assert (sums[n256] < 0).all() and sums[e.c_at["neg256"]] == 255 * (bot if X == 0 else shifted_bottom) == sums[n256].min()
        assert (sums[e.mc == slot("top300")] == 299 * top).all() and sums[e.mc == slot("top300")].max() < 2 ** 31
    # the flat pair space: top256's 32,640 pairs come first, so neg256's last row -- C^L's 255 pairs -- is places 1 .. 255 of one chunk
    fa, fb, chunk = flat_chunks(e.mc)
    T0 = triangle(L, 0, 0)
    assert fa.size == 2 * 32640 + 1770 + 2 and -(-fa.size // 256) == link_grids(e.mc)[0] == 262
    c = e.c_at["neg256"]
    of_c = np.flatnonzero((fa == c) | (fb == c))
    assert of_c.size == 255 and (fb[of_c] == c).all() and np.array_equal(of_c, np.arange(of_c[0], of_c[0] + 255))
    assert len(set(chunk[of_c].tolist())) == 1 and of_c[0] % 256 == 1
    assert T0[fb[of_c], fa[of_c]].sum() == 255 * bot and abs(255 * bot) < 2 ** 23
    # top256's last member has 255 pairs too; they lie in two chunks, 127 + 128 (the slot starts the pair space)
    last = int(np.flatnonzero(e.mc == slot("top256")).max())
    of_t = np.flatnonzero(fb == last)
    assert of_t.size == 255 and not (fa == last).any() and (T0[fb[of_t], fa[of_t]] == top).all()
    assert np.bincount(chunk[of_t] - chunk[of_t][0]).tolist() == [127, 128]
    # ... and in one chunk once the two slots exchange their numbers: a member's 255 pairs at L x 1,000 each in one chunk's int32 sum
    fa, fb, chunk = flat_chunks(swapped_slots(e.mc))
    of_t = np.flatnonzero(fb == last)
    assert of_t.size == 255 and len(set(chunk[of_t].tolist())) == 1 and T0[fb[of_t], fa[of_t]].sum() == 255 * top < 2 ** 23
    if L == 30:
        assert (T0[e.c_at["neg256"], n256[:-1]] == -THR_LIMIT).all() and top == THR_LIMIT


def test_mixed_set_holds_what_the_rectangle_cases_claim():
    m = mixed_set()
    blk = mixed_block(0, 0).astype(np.int64)
    cl = lambda c: blk[m.mc == c]     # noqa: E731
    q = m.q
    assert np.bincount(m.mc).tolist() == [40, 40, 40, 20] and m.start.tolist() == [7, 47, 87, 127, 147]
    assert (cl(0)[:, [q["top32"], q["top32_b"]]] == 32000).all() and (cl(1)[:, [q["top32"], q["top32_b"]]] == 30000).all()
    assert (cl(0)[:, q["top30"]] == 30000).all() and (cl(1)[:, q["top30"]] == 30000).all()
    assert (cl(2)[:, q["c30"]] == -30000).all() and (cl(2)[:, q["c32"]] == -30000).all()
    assert blk.max() == 32000 and blk.min() == -30000
    # assign, by the oracle's block alone: the top 32-mer's clusters at 30,000 are A then B; C^30's at -30,000 are A, B (about -60) and D
    # at exactly -30,000 -- O holds a member with D, E, N or Q, and that member alone would not decide: the block does
    best, score, nf = A.expected(blk, m.mc, m.ids, m.sizes, 30000, 2)
    assert best[q["top32"]].tolist() == [0, 1] and score[q["top32"]].tolist() == [32000, 30000] and nf[q["top32"]] == 2
    assert best[q["top30"]].tolist()[:1] == [1] and score[q["top30"]].tolist() == [30000, 30000] and nf[q["c30"]] == 0
    best, score, nf = A.expected(blk, m.mc, m.ids, m.sizes, -30000, 4)
    feasible = [c for c in range(4) if cl(c)[:, q["c30"]].min() >= -30000]
    assert 2 in feasible and nf[q["c30"]] == len(feasible) and cl(3)[:, q["c30"]].min() < 0
    assert best[q["c30"]][len(feasible) - 1] == 2 and score[q["c30"]][len(feasible) - 1] == -30000
    best, score, nf = A.expected(blk, m.mc, m.ids, m.sizes, -29999, 4)
    assert 2 not in best[q["c30"]].tolist() and nf[q["c30"]] == len(feasible) - 1 and -30000 not in score[q["c30"]].tolist()
    # the cluster graph: at 30,000 A and B alone are feasible for each other, their minimum exactly 30,000
    pairs, _, _ = ME.expected_pairs(c_oracle, m.M, m.res, m.off, m.nq, m.n, m.mc, 0, 0, 30000)
    assert [tuple(int(v) for v in f) for f in zip(*hammock_amd.edge_fields(pairs))] == [(0, 1, 30000)]
    n = neg_rect_set()
    st, blk = c_oracle.score_block(n.M, n.res, n.off, np.arange(3), np.arange(3, n.n), 0, 0, 0)
    assert st == 0 and (blk == -32000).all() and n.n == 302


def test_the_range_checks_accept_every_parameter_set_the_gpu_cases_use():
    for lens in ((32, 32), (30, 30), (32, 30)):
        for X, p in PARAMS + [(3, -96)]:
            assert int16_top(lens, X, p) <= 32767 and int16_bottom(lens, X, p) >= -32768, (lens, X, p)
    # the refusal pairs sit one unit apart at both ends
    assert int16_bottom((32, 32), 3, -128) == -32768 and int16_bottom((32, 32), 3, -129) == -32774 < -32768
    assert int16_top((32, 32), 3, 127) == 32762 <= 32767 and int16_top((32, 32), 3, 128) == 32768
    assert all(-THR_LIMIT <= t <= THR_LIMIT for t in (30000, -30000, 0, -29999))


def test_split_refuses_the_far_side_of_each_bound_on_a_host_only_context():
    """hmk_clinkage_split makes its score checks before it asks for the device; linkage, align and survey ask for the device first"""
    s = small_set()
    ctx = hammock_amd.Context(s.M, device=-1)
    ctx.set_sequences(residues=s.res, offsets=s.off)
    for p in (128, -129):
        with pytest.raises(ValueError, match="int16"):
            ctx.clinkage_split(0, s.n, s.mc, s.ncl, 3, p, 0)
    for thr in (30001, -30001):
        with pytest.raises(ValueError, match="threshold"):
            ctx.clinkage_split(0, s.n, s.mc, s.ncl, 3, 0, thr)
    for p, thr in ((127, 30000), (-128, -30000)):
        with pytest.raises(hammock_amd.DeviceError):
            ctx.clinkage_split(0, s.n, s.mc, s.ncl, 3, p, thr)


# ---- GPU: 1. linkage ----------------------------------------------------------------------------------------------------------------

def link_thresholds(min_score):
    """30,000, -30,000 and one above every slot's lowest score where that is a threshold the call takes"""
    above = sorted({int(v) + 1 for v in min_score if v != INT32_MAX and -THR_LIMIT <= int(v) + 1 <= THR_LIMIT})
    return [THR_LIMIT, -THR_LIMIT] + above


def assert_link_ends(got, e, X):
    top, bot = e.L * 1000, -e.L * 1000
    assert got[0][slot("top256")] == got[0][slot("top300")] == got[0][slot("pair_top")] == top
    if X == 0:
        assert got[0][slot("neg256")] == got[0][slot("neg300")] == got[0][slot("pair_neg")] == bot
        for name in ("neg256", "neg300", "pair_neg"):
            assert e.c_at[name] in (got[1][slot(name)], got[2][slot(name)])
            if got[4] is not None:
                assert got[4][e.c_at[name]] == bot
    if got[4] is not None:
        assert (got[4][e.mc == slot("top300")] == top).all() and (got[4][e.mc == slot("top256")] == top).all()


@pytest.mark.gpu
@pytest.mark.parametrize("X,p", PARAMS, ids=PARAM_IDS)
@pytest.mark.parametrize("L", LENGTHS)
def test_linkage_keys_at_both_ends(gpu, L, X, p):
    """the slot key's 16-bit field at 64,768 / 62,768 (top bit set) and at 768 / 2,768, the argmin pair among 32,640 tied pairs,
    member_min decoded from the key, n_below at both threshold limits and one above each slot's lowest score"""
    e = ends_set(L)
    assert np.bincount(e.mc).tolist() == list(SLOT_SIZES) and link_grids(e.mc)[:2] == (262, 6)
    a, b, sl, sc = inside(L, X, p)
    ctx = LK.device_ctx(e.M, e.res, e.off)
    lowest = LK.reduce_scores(a, b, sl, sc, e.n, e.ncl, 0)[0][0]
    thrs = link_thresholds(lowest)
    assert len(thrs) >= 3 and len(thrs) == len(set(thrs))
    for thr in thrs:
        want, stats = LK.reduce_scores(a, b, sl, sc, e.n, e.ncl, thr)
        for members in (True, False):
            got = ctx.cluster_linkage_shifted(0, e.n, e.mc, e.ncl, X, p, thr, members=members)
            LK.check(got, want, ctx, stats)
            assert (got[4] is None) == (not members)
            assert_link_ends(got, e, X)
        if thr == THR_LIMIT:       # a pair ON the threshold is not below it: at L = 30 every top pair is
            assert got[3][slot("top256")] == 0 and got[3][slot("top300")] == 0 and got[3][slot("plain")] == 60 * 59 // 2
        if thr == -THR_LIMIT:
            assert got[3][slot("neg256")] == (255 if (L, X) == (32, 0) else 0) and got[3][slot("plain")] == 0
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("members", [True, False], ids=["members", "slots_only"])
@pytest.mark.parametrize("L", LENGTHS)
def test_linkage_keys_at_both_ends_on_three_workgroups(gpu, monkeypatch, capfd, L, members):
    e = ends_set(L)
    a, b, sl, sc = inside(L, 0, 0)
    ctx = LK.device_ctx(e.M, e.res, e.off)
    for thr in (THR_LIMIT, -THR_LIMIT):
        want, stats = LK.reduce_scores(a, b, sl, sc, e.n, e.ncl, thr)
        got, lines = capped(monkeypatch, capfd, 3, lambda: ctx.cluster_linkage_shifted(0, e.n, e.mc, e.ncl, 0, 0, thr, members=members))
        LK.check(got, want, ctx, stats)
        assert_link_ends(got, e, 0)
        cut(lines, 3, "k_linkage_flat", 262)
        cut(lines, 3, "k_linkage_tiled", 6)
        assert lines.get("k_linkage_init") == ([(5, 3)] if members else None)     # 1,176 members: 5 workgroups; 7 slots: one
    ctx.close()


# ---- GPU: 2. split ------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def split_expect(L, X, p, thr):
    e = ends_set(L)
    return oracle_split(e.M, e.res, e.off, e.mc, e.ncl, X, p, thr)


def split_matches(ctx, s, X, p, thr, want):
    """the call against oracle_split's answer -> its result, or None where the reference's chain returns to a stacked cluster: then the
    call must say so, for that slot"""
    if isinstance(want[0], str):
        with pytest.raises(hammock_amd.ReferenceWouldCrash) as info:
            ctx.clinkage_split(0, s.n, s.mc, s.ncl, X, p, thr)
        assert info.value.index == want[1]
        return None
    got = ctx.clinkage_split(0, s.n, s.mc, s.ncl, X, p, thr)
    same(got, want, f"thr {thr} ")
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("X,p", PARAMS, ids=PARAM_IDS)
@pytest.mark.parametrize("L", LENGTHS)
def test_split_triangles_at_both_ends(gpu, L, X, p):
    """(int16_t)score into the dense triangles at +-32,000 / +-30,000, and the complete-linkage cut with pairs exactly on the
    thresholds' limits"""
    e = ends_set(L)
    assert np.bincount(e.mc).tolist() == list(SLOT_SIZES)
    ctx = LK.device_ctx(e.M, e.res, e.off)
    for thr in (THR_LIMIT, -THR_LIMIT, 0):
        got = split_matches(ctx, e, X, p, thr, split_expect(L, X, p, thr))
        if got is None:
            continue
        a, b, sl, sc = inside(L, X, p)
        s = ctx.last_split_stats
        assert (s.pairs_scored, s.n_edges) == (sc.size, int((sc >= thr).sum()))
        if thr == THR_LIMIT:       # at L = 30 every top pair sits exactly on the threshold
            assert got[1][slot("top256")] == got[1][slot("top300")] == got[1][slot("pair_top")] == 1
            assert got[1][slot("neg256")] == 256 and got[1][slot("plain")] == 60
        if thr == -THR_LIMIT:
            loses_c = (L, X) == (32, 0)     # -32,000 is below the lowest threshold there is; -30,000 and -29,006 are not
            assert got[1][slot("neg256")] == got[1][slot("neg300")] == got[1][slot("pair_neg")] == (2 if loses_c else 1)
            assert got[1][slot("plain")] == 1
    ctx.close()


# ---- GPU: 3. align ------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def align_expect(L, X, p):
    e = ends_set(L)
    want, stats, _ = AL.expectation(c_oracle, e.M, e.res, e.off, e.mc, e.ncl, X, p)
    for arr in want:
        arr.setflags(write=False)
    return want, stats


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [0, 1, 3])
@pytest.mark.parametrize("X,p", PARAMS, ids=PARAM_IDS)
@pytest.mark.parametrize("L", LENGTHS)
def test_align_sums_at_both_ends(gpu, monkeypatch, capfd, L, X, p, cap):
    """a member's 255 pairs of one flat chunk at -32,000 each in the int32 LDS sums, add_sum of negative partial sums, a slot whose every
    sum is negative (centre_key's bias), sums of 299 x 32,000; under HMK_TEST_GRID_CAP every work loop beyond its first iteration"""
    e = ends_set(L)
    assert np.bincount(e.mc).tolist() == list(SLOT_SIZES)
    want, stats = align_expect(L, X, p)
    ctx = LK.device_ctx(e.M, e.res, e.off)
    if cap:
        monkeypatch.setenv("HMK_TEST_GRID_CAP", str(cap))
    capfd.readouterr()
    got = ctx.cluster_align_shifted(0, e.n, e.mc, e.ncl, X, p)
    AL.check(got, want, ctx, stats)
    bare = ctx.cluster_align_shifted(0, e.n, e.mc, e.ncl, X, p, sums=False)
    assert bare[3] is None
    AL.check(bare, want, ctx, stats)
    grids = AL.wanted_grids(e.mc, e.ncl)
    assert grids == {"k_align_init": 5, "k_align_center": 5, "k_align_shift": 5, "k_align_sums_flat": 262, "k_align_sums_tiled": 6}
    lines = {}
    for kernel, wanted, launched in AL.GRID_LINE.findall(capfd.readouterr().err):
        lines.setdefault(kernel, set()).add((int(wanted), int(launched)))
    assert {k: v for k, v in lines.items() if k.startswith("k_align_")} == {k: {(w, cap)} for k, w in grids.items() if cap and w > cap}
    center, center_sum, _, member_sum, center_score, shift, _ = got
    top = L * 1000
    assert center_sum[slot("top300")] == 299 * top and center_sum[slot("top256")] == 255 * top
    assert (member_sum[e.mc == slot("neg256")] < 0).all() and center_sum[slot("neg256")] < 0 and center_sum[slot("neg300")] < 0
    assert center[slot("neg256")] != e.c_at["neg256"] and member_sum[e.c_at["neg256"]] == 255 * (-top if X == 0 else -(L - 3) * 1000 - 6)
    if X == 0:
        assert all(center_score[e.c_at[name]] == -top for name in ("neg256", "neg300"))
        assert not shift.any()
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [0, 1])
@pytest.mark.parametrize("L", LENGTHS)
def test_align_sums_with_a_chunk_of_255_top_pairs(gpu, monkeypatch, capfd, L, cap):
    """the same input with the slot numbers of top256 and neg256 exchanged: top256's last member now has its 255 pairs in ONE chunk of
    the flat pair space, 255 x 32,000 = 8,160,000 in one int32 LDS sum (the bound the kernel states is 2^23 = 8,388,608)"""
    e = ends_set(L)
    mc = swapped_slots(e.mc)
    want, stats, _ = AL.expectation(c_oracle, e.M, e.res, e.off, mc, e.ncl, 0, 0)
    ctx = LK.device_ctx(e.M, e.res, e.off)
    if cap:
        monkeypatch.setenv("HMK_TEST_GRID_CAP", str(cap))
    capfd.readouterr()
    got = ctx.cluster_align_shifted(0, e.n, mc, e.ncl, 0, 0)
    AL.check(got, want, ctx, stats)
    assert (got[3][e.mc == slot("top256")] == 255 * L * 1000).all() and got[1][0] < 0 and got[1][1] == 255 * L * 1000
    lines = {k: (int(w), int(n)) for k, w, n in AL.GRID_LINE.findall(capfd.readouterr().err)}
    assert lines.get("k_align_sums_flat") == ((262, 1) if cap else None)
    ctx.close()


# ---- GPU: 4. survey -----------------------------------------------------------------------------------------------------------------

SURVEY_WINDOWS = [(32000 - 5, 10), (-32000 - 5, 10), (-32000, 1), (32000, 1), (0, 0)]     # (score_lo, n_bins)
SURVEY_THRESHOLDS = [THR_LIMIT, -THR_LIMIT, 0]


def expect_triangle(L, X, p, thr, lo, bins, rows=True):
    T = triangle(L, X, p)
    n = T.shape[0]
    return SV.reduce_scores(T, ~np.eye(n, dtype=bool), 0, T[np.tril_indices(n, -1)], thr, lo, bins, rows)


def expect_rectangle(blk, r0, thr, lo, bins, rows=True):
    blk = np.asarray(blk, dtype=np.int64)
    return SV.reduce_scores(blk, np.ones(blk.shape, dtype=bool), r0, blk.ravel(), thr, lo, bins, rows)


def survey_triangles(ctx, capfd, cap, L, X, p):
    e = ends_set(L)
    for lo, bins in SURVEY_WINDOWS:
        for thr in SURVEY_THRESHOLDS:
            got, launches = SV.survey(ctx, capfd, cap, True, 0, e.n, 0, e.n, X, p, thr, lo, bins)
            want = expect_triangle(L, X, p, thr, lo, bins)
            SV.check(got, want, launches)
            hist, (best, index, degree), stats = got
            assert stats.score_max == L * 1000 and stats.score_min == (-L * 1000 if X == 0 else -(L - 3) * 1000 - 6)
            if L == 32 and X == 0:
                assert (best[e.mc == slot("top300")] == 32000).all() and stats.n_at_or_above == want[2]["n_at_or_above"]
                if (lo, bins) == (32000, 1):
                    assert hist[0] == 558 * 557 // 2       # any two of the 558 top words, whatever their slots
                if (lo, bins) == (-32000, 1):
                    assert hist[0] == 3 * 555       # three copies of C^32 against 555 bottom words
                    assert stats.n_below == 0 and stats.n_above == stats.pairs_scored - 3 * 555


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [0, 3])
@pytest.mark.parametrize("X,p", PARAMS, ids=PARAM_IDS)
@pytest.mark.parametrize("L", LENGTHS)
def test_survey_triangles_at_both_ends(gpu, monkeypatch, capfd, L, X, p, cap):
    """survey_key and d = score - lo at +-32,000, windows that start at either end, score_min / score_max, thresholds at both limits"""
    e = ends_set(L)
    ctx = LK.device_ctx(e.M, e.res, e.off)
    if cap:
        monkeypatch.setenv("HMK_TEST_GRID_CAP", str(cap))
    survey_triangles(ctx, capfd, cap, L, X, p)
    ctx.close()


def survey_rectangles(ctx_of, capfd, cap):
    """the C^32 copies against bottom words (every best score -32,000, the smallest index among the ties) and the other way round; the
    queries of mixed_set against its clusters and the other way round"""
    n = neg_rect_set()
    ctx = ctx_of(n)
    st, blk = c_oracle.score_block(n.M, n.res, n.off, np.arange(3), np.arange(3, n.n), 0, 0, 0)
    assert st == 0
    for lo, bins in SURVEY_WINDOWS:
        for thr in SURVEY_THRESHOLDS:
            got, launches = SV.survey(ctx, capfd, cap, False, 0, 3, 3, n.n, 0, 0, thr, lo, bins)
            SV.check(got, expect_rectangle(blk, 3, thr, lo, bins), launches)
            _, (best, index, degree), stats = got
            assert best.tolist() == [-32000] * 3 and index.tolist() == [3] * 3 and stats.score_min == stats.score_max == -32000
            assert degree.tolist() == [0] * 3
            got, launches = SV.survey(ctx, capfd, cap, False, 3, n.n, 0, 3, 0, 0, thr, lo, bins)
            SV.check(got, expect_rectangle(blk.T, 0, thr, lo, bins), launches)
            assert (got[1][0] == -32000).all() and not got[1][1].any()
    ctx.close()
    m = mixed_set()
    ctx = ctx_of(m)
    for X, p in PARAMS:
        st, fwd = c_oracle.score_block(m.M, m.res, m.off, np.arange(m.nq), np.arange(m.nq, m.n), 0, X, p)
        st2, back = c_oracle.score_block(m.M, m.res, m.off, np.arange(m.nq, m.n), np.arange(m.nq), 0, X, p)
        assert st == 0 and st2 == 0
        for lo, bins in SURVEY_WINDOWS:
            for thr in SURVEY_THRESHOLDS:
                got, launches = SV.survey(ctx, capfd, cap, False, 0, m.nq, m.nq, m.n, X, p, thr, lo, bins)
                SV.check(got, expect_rectangle(fwd, m.nq, thr, lo, bins), launches)
                assert got[2].score_max == 32000 and got[1][0][m.q["top32"]] == 32000
                if X == 0:
                    assert got[2].score_min == -30000 and got[1][0][m.q["c30"]] < 0
                got, launches = SV.survey(ctx, capfd, cap, False, m.nq, m.n, 0, m.nq, X, p, thr, lo, bins)
                SV.check(got, expect_rectangle(back, 0, thr, lo, bins), launches)
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [0, 3])
def test_survey_rectangles_at_both_ends(gpu, monkeypatch, capfd, cap):
    if cap:
        monkeypatch.setenv("HMK_TEST_GRID_CAP", str(cap))
    survey_rectangles(lambda s: LK.device_ctx(s.M, s.res, s.off), capfd, cap)


@pytest.mark.gpu
def test_survey_other_histogram_form_at_both_ends(gpu, capfd):
    """the wave-aggregated LDS histogram, switched as test_survey.test_the_other_histogram_form_agrees switches it"""
    form = N.lib.hmk_survey_hist_form_for_measurement
    assert form(1) == 0
    try:
        e = ends_set(32)
        ctx = LK.device_ctx(e.M, e.res, e.off)
        survey_triangles(ctx, capfd, 0, 32, 0, 0)
        ctx.close()
        survey_rectangles(lambda s: LK.device_ctx(s.M, s.res, s.off), capfd, 0)
    finally:
        assert form(0) == 1


# ---- GPU: 5. search -----------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_search_hits_and_best_k_at_both_ends(gpu):
    """the int16 of a packed edge read back signed at -30,000 (the floor of the thresholds) and at 32,000; best-k's (score + 32768) << 32
    ordering with 32,000 ahead of 30,000 ahead of negative scores, and 40 hits tied at -30,000 in ascending index"""
    m = mixed_set()
    ctx = LK.device_ctx(m.M, m.res, m.off)
    q_idx, r_idx = np.arange(m.nq), np.arange(m.nq, m.n)
    blk, want = S.oracle_hits(c_oracle, m.M, m.res, m.off, q_idx, r_idx, 0, 0, 0, -THR_LIMIT)
    assert len(want) == m.nq * (m.n - m.nq)      # nothing is below the floor
    edges, st = ctx.search_shifted(0, m.nq, m.nq, m.n, 0, 0, -THR_LIMIT)
    assert np.array_equal(np.sort(edges), want) and st.classes_direct >= 1
    x, mm, score = hammock_amd.edge_fields(edges)
    assert score.min() == -30000 and score.max() == 32000 and (score == -30000).sum() == 2 * 40
    assert set(x[(mm == m.q["c30"]) & (score == -30000)].tolist()) == set(range(int(m.start[2]), int(m.start[3])))
    for thr in (-THR_LIMIT, THR_LIMIT):
        for k in (1, 3, BEST_K_MAX):
            idx, sc = ctx.search_best_shifted(0, m.nq, m.nq, m.n, 0, 0, thr, k)
            widx, wsc = S.numpy_best(blk, r_idx, thr, k)
            assert np.array_equal(idx, widx) and np.array_equal(sc, wsc), (thr, k)
    idx, sc = ctx.search_best_shifted(0, m.nq, m.nq, m.n, 0, 0, -THR_LIMIT, BEST_K_MAX)
    assert sc[m.q["top32"]].tolist() == [32000] * BEST_K_MAX and sc[m.q["top30"]].tolist() == [30000] * BEST_K_MAX
    assert idx[m.q["top32"]].tolist() == list(range(int(m.start[0]), int(m.start[0]) + BEST_K_MAX))
    idx, sc = ctx.search_best_shifted(0, m.nq, m.nq, m.n, 0, 0, THR_LIMIT, BEST_K_MAX)
    assert (idx[m.q["c30"]] == -1).all() and (idx[m.q["plain32"]] == -1).all() and sc[m.q["top32"]].tolist() == [32000] * BEST_K_MAX
    # the top 32-mer against the last 20 members of A and all of B: 20 hits at 32,000, then B's at 30,000, each in ascending index
    a0, b1 = int(m.start[1]) - 20, int(m.start[2])
    t = m.q["top32"]
    idx, sc = ctx.search_best_shifted(t, t + 1, a0, b1, 0, 0, THR_LIMIT, BEST_K_MAX)
    widx, wsc = S.numpy_best(blk[t:t + 1, a0 - m.nq:b1 - m.nq], np.arange(a0, b1), THR_LIMIT, BEST_K_MAX)
    assert np.array_equal(idx, widx) and np.array_equal(sc, wsc)
    assert sc[0].tolist() == [32000] * 20 + [30000] * 12 and idx[0].tolist() == list(range(a0, a0 + BEST_K_MAX))
    # C^30 against cluster D alone: every hit is -30,000, and the ties come in ascending index
    d0, d1 = int(m.start[2]), int(m.start[3])
    c = m.q["c30"]
    dblk = blk[c:c + 1, d0 - m.nq:d1 - m.nq]
    assert (dblk == -30000).all()
    for k in (1, 3, BEST_K_MAX):
        idx, sc = ctx.search_best_shifted(c, c + 1, d0, d1, 0, 0, -THR_LIMIT, k)
        widx, wsc = S.numpy_best(dblk, np.arange(d0, d1), -THR_LIMIT, k)
        assert np.array_equal(idx, widx) and np.array_equal(sc, wsc)
        assert idx[0].tolist() == list(range(d0, d0 + k)) and sc[0].tolist() == [-30000] * k
    idx, _ = ctx.search_best_shifted(c, c + 1, d0, d1, 0, 0, -THR_LIMIT + 1, 3)
    assert (idx == -1).all()
    with pytest.raises(ValueError):       # 32 is the largest k the call takes
        ctx.search_best_shifted(0, m.nq, m.nq, m.n, 0, 0, -THR_LIMIT, 70)
    ctx.close()


# ---- GPU: 6. assign, match, merge ---------------------------------------------------------------------------------------------------

def mixed_ctx():
    m = mixed_set()
    ctx = hammock_amd.Context(m.M, device=0)
    ctx.set_sequences(residues=m.res, offsets=m.off, sizes=np.concatenate([np.ones(m.nq, np.int32), m.sizes]))
    return m, ctx


@pytest.mark.gpu
def test_assign_table_keys_at_both_ends(gpu):
    """(min score + 32768) << 32 with the minimum at 32,000, at 30,000 = the threshold, at exactly -30,000 = the threshold, and one
    threshold above it; two feasible clusters ranked by 32,000 against 30,000"""
    m, ctx = mixed_ctx()
    blk = mixed_block(0, 0)
    q = m.q
    for thr, k in ((THR_LIMIT, 2), (THR_LIMIT, 1), (-THR_LIMIT, 4), (-THR_LIMIT + 1, 4), (0, 4)):
        want = A.expected(blk, m.mc, m.ids, m.sizes, thr, k)
        got = ctx.assign_shifted(0, m.nq, m.nq, m.n, m.mc, m.ids, 0, 0, thr, k)
        A.check(got, want)
        A.cross_check(blk, m.mc, m.ids, m.sizes, thr, want[0], want[1])
        best, score, nf = got
        if (thr, k) == (THR_LIMIT, 2):
            assert best[q["top32"]].tolist() == [0, 1] and score[q["top32"]].tolist() == [32000, 30000]
            assert nf[q["c30"]] == 0 and best[q["c30"]].tolist() == [A.NONE] * 2
        if thr == -THR_LIMIT:
            assert 2 in best[q["c30"]].tolist() and score[q["c30"]][best[q["c30"]].tolist().index(2)] == -30000
        if thr == -THR_LIMIT + 1:
            assert 2 not in best[q["c30"]].tolist() and 2 not in best[q["c32"]].tolist()
    ctx.close()


@pytest.mark.gpu
def test_match_table_keys_at_both_ends(gpu):
    """query clusters: the two new top 32-mers together; C^30 alone (no second word has -1,000 in every cell against D's members);
    the rest alone"""
    m, ctx = mixed_ctx()
    blk = mixed_block(0, 0)
    for thr, k in ((THR_LIMIT, 2), (-THR_LIMIT, 4), (-THR_LIMIT + 1, 4), (0, 1)):
        want = MA.expected(blk, m.mc, m.ids, m.sizes, m.qc, thr, k)
        got = ctx.match_clusters_shifted(0, m.nq, m.qc, m.nq, m.n, m.mc, m.ids, 0, 0, thr, k)
        MA.check(got, want)
        best, score, nf = got
        if thr == THR_LIMIT:
            assert best[0].tolist() == [0, 1] and score[0].tolist() == [32000, 30000] and nf[1] == 0
        if thr == -THR_LIMIT:
            assert 2 in best[1].tolist() and score[1][best[1].tolist().index(2)] == -30000
        if thr == -THR_LIMIT + 1:
            assert 2 not in best[1].tolist()
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("eight", [False, True], ids=["default", "HMK_ADJ_8BYTE"])
def test_merge_cluster_graph_at_both_ends(gpu, monkeypatch, eight):
    """the cluster graph's minimum at exactly 30,000 = the threshold (A with B, nothing else), and at -30,000 with cross minima down to
    the threshold; the merge on the device graph against the merge from the oracle's edges"""
    if eight:
        monkeypatch.setenv("HMK_ADJ_8BYTE", "1")
    m, ctx = mixed_ctx()
    r0, r1 = m.nq, m.n
    all_edges = {thr: oracle_edges(c_oracle, m.M, m.res, m.off, 0, 0, thr, True) for thr in (THR_LIMIT, -THR_LIMIT)}
    for thr in (THR_LIMIT, -THR_LIMIT):
        want, _, _ = ME.expected_pairs(c_oracle, m.M, m.res, m.off, r0, r1, m.mc, 0, 0, thr)
        got = ctx.cluster_pairs_shifted(r0, r1, m.mc, 4, 0, 0, thr)
        assert np.array_equal(np.sort(got), want)
        fields = [tuple(int(v) for v in f) for f in zip(*hammock_amd.edge_fields(np.sort(got)))]
        if thr == THR_LIMIT:
            assert fields == [(0, 1, 30000)]
        else:
            assert (0, 1, 30000) in fields and min(f[2] for f in fields) < 0 and len(fields) >= 2
        try:
            ref = ctx.clinkage_merge_from_edges(all_edges[thr], r0, r1, m.mc, m.ids)
        except hammock_amd.ReferenceWouldCrash:       # the chain returns to a stacked cluster: the device graph must lead there too
            with pytest.raises(hammock_amd.ReferenceWouldCrash):
                ctx.clinkage_merge(r0, r1, m.mc, m.ids, 0, 0, thr)
            assert thr != THR_LIMIT
            continue
        ref_rank, ref_stats = ctx.member_rank.copy(), ctx.last_merge_stats
        merged, order = ctx.clinkage_merge(r0, r1, m.mc, m.ids, 0, 0, thr)
        assert np.array_equal(merged, ref[0]) and np.array_equal(order, ref[1]) and np.array_equal(ctx.member_rank, ref_rank)
        assert ctx.last_merge_stats.merges == ref_stats.merges and ctx.last_merge_stats.cluster_pairs == len(want)
        if thr == THR_LIMIT:
            assert ref_stats.merges == 1 and merged[0] == merged[1] and len({int(v) for v in merged}) == 3
    ctx.close()


# ---- GPU: 7. refusals on a device context -------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_penalties_one_unit_either_side_of_the_int16_bounds(gpu):
    """32-mers at X = 3: p = -128 puts the bottom at exactly -32,768 and p = +127 the top at 32,762 -- accepted, and exact against the
    oracle; p = -129 and p = +128 are refused with "int16" by linkage, align, survey and split"""
    s = small_set()
    ctx = LK.device_ctx(s.M, s.res, s.off)
    hi, lo = np.tril_indices(s.n, -1)
    for p in (-128, 127):
        a, b, sl, sc = LK.score_inside(c_oracle, s.M, s.res, s.off, s.mc, 3, p)
        want, stats = LK.reduce_scores(a, b, sl, sc, s.n, s.ncl, 0)
        LK.check(ctx.cluster_linkage_shifted(0, s.n, s.mc, s.ncl, 3, p, 0), want, ctx, stats)
        assert want[0][0] == 32000 and want[0][1] == max(-(32 - t) * 1000 + 2 * p * t for t in range(4))     # -29,768 and -28,238
        want, stats, _ = AL.expectation(c_oracle, s.M, s.res, s.off, s.mc, s.ncl, 3, p)
        AL.check(ctx.cluster_align_shifted(0, s.n, s.mc, s.ncl, 3, p), want, ctx, stats)
        st, tri = c_oracle.score_pairs(s.M, s.res, s.off, hi, lo, 0, 3, p)
        assert st == 0
        T = np.zeros((s.n, s.n), dtype=np.int64)
        T[hi, lo] = tri
        T[lo, hi] = tri
        got = ctx.score_survey_shifted(0, s.n, 0, s.n, 3, p, 0, score_lo=-32768, n_bins=1024)
        SV.check(got, SV.reduce_scores(T, ~np.eye(s.n, dtype=bool), 0, tri, 0, -32768, 1024), 3)
        split_matches(ctx, s, 3, p, 0, oracle_split(s.M, s.res, s.off, s.mc, s.ncl, 3, p, 0))
    for p in (-129, 128):
        for call in (lambda: ctx.cluster_linkage_shifted(0, s.n, s.mc, s.ncl, 3, p, 0),
                     lambda: ctx.cluster_align_shifted(0, s.n, s.mc, s.ncl, 3, p),
                     lambda: ctx.score_survey_shifted(0, s.n, 0, s.n, 3, p, 0, n_bins=8),
                     lambda: ctx.clinkage_split(0, s.n, s.mc, s.ncl, 3, p, 0)):
            with pytest.raises(ValueError, match="int16"):
                call()
    ctx.close()


# ---- GPU: 8. beyond 32 bits ---------------------------------------------------------------------------------------------------------

BIG_ALIGN_N = 67_200       # 67,199 x 32,000 = 2,150,368,000 > 2^31
BIG_SURVEY_N = 92_700      # 92,700 x 92,699 / 2 = 4,296,598,650 > 2^32


def sample_scores(M, res, off, n, X, p, count=100_000):
    rng = np.random.default_rng(16_300)
    i, j = rng.integers(0, n, count), rng.integers(0, n, count)
    keep = i != j
    st, sc = c_oracle.score_pairs(M, res, off, i[keep], j[keep], 0, X, p)
    assert st == 0
    return sc


@pytest.mark.gpu
def test_align_member_sums_beyond_int32(gpu):
    """one slot of 67,200 distinct top 32-mers at X = 0: every member sum is 2,150,368,000.  The expectation is analytic; its premise --
    any two of the words score 32,000 -- is checked by the oracle on 10^5 random pairs and by lane_model.shifted_score"""
    M = ends_matrix()
    words = lm.top_words(M, 32, BIG_ALIGN_N, np.random.default_rng(16_400))
    res, off = hammock_amd.pack_sequences(words)
    assert (sample_scores(M, res, off, BIG_ALIGN_N, 0, 0) == 32000).all() and lm.shifted_score(M, words[0], words[-1], 0, 0) == 32000
    total = (BIG_ALIGN_N - 1) * 32000
    assert total == 2_150_368_000 > 2 ** 31
    ctx = LK.device_ctx(M, res, off)
    mc = np.zeros(BIG_ALIGN_N, dtype=np.uint32)
    t0 = time.perf_counter()
    center, center_sum, width, member_sum, center_score, shift, column = ctx.cluster_align_shifted(0, BIG_ALIGN_N, mc, 1, 0, 0)
    print(f"align of one slot of {BIG_ALIGN_N}: {time.perf_counter() - t0:.2f} s, kernels {ctx.last_align_stats.kernel_ms:.0f} ms")
    assert member_sum.dtype == np.int64 and (member_sum == total).all()
    assert center.tolist() == [0] and center_sum.tolist() == [total] and width.tolist() == [32]
    assert center_score[0] == INT32_MAX and (center_score[1:] == 32000).all() and not shift.any() and not column.any()
    s = ctx.last_align_stats
    assert (s.pairs_scored, s.n_multi, s.max_width) == (BIG_ALIGN_N * (BIG_ALIGN_N - 1) // 2 + BIG_ALIGN_N - 1, 1, 32)
    ctx.close()


@pytest.mark.gpu
def test_survey_bin_beyond_uint32(gpu):
    """the triangle of 92,700 copies of one 12-mer at X = 0, three bins around the self-pair score: the middle bin, flushed from 32-bit LDS
    counters tile by tile, is 4,296,598,650"""
    M = ends_matrix()
    one = np.random.default_rng(16_500).integers(0, 20, size=12).astype(np.uint8)
    res, off = hammock_amd.pack_sequences([one] * BIG_SURVEY_N)
    s0 = lm.shifted_score(M, one, one, 0, 0)
    assert (sample_scores(M, res, off, BIG_SURVEY_N, 0, 0) == s0).all() and s0 == int(M[one, one].sum())
    pairs = BIG_SURVEY_N * (BIG_SURVEY_N - 1) // 2
    assert pairs == 4_296_598_650 > 2 ** 32
    ctx = LK.device_ctx(M, res, off)
    t0 = time.perf_counter()
    hist, (best, index, degree), stats = ctx.score_survey_shifted(0, BIG_SURVEY_N, 0, BIG_SURVEY_N, 0, 0, s0, score_lo=s0 - 1, n_bins=3)
    print(f"survey of {BIG_SURVEY_N} copies: {time.perf_counter() - t0:.2f} s, kernels {stats.kernel_ms:.0f} ms")
    assert hist.dtype == np.uint64 and hist.tolist() == [0, pairs, 0]
    assert (stats.pairs_scored, stats.n_at_or_above, stats.n_below, stats.n_above) == (pairs, pairs, 0, 0)
    assert stats.score_min == stats.score_max == s0
    assert (degree == BIG_SURVEY_N - 1).all() and (best == s0).all() and index[0] == 1 and not index[1:].any()
    ctx.close()
