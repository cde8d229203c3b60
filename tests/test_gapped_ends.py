"""The gapped scorers at the ends of their score fields, of their tiers and of their strips.

LocalAlignmentScorer (k_local.hip) and GlobalAlignmentScorer (k_global.hip) narrow a score more often than any other path: int8
query profiles read back with a sign extension, 4 * value + tag in int8 table bytes, packed int16 halves with unsigned saturation,
an H | F pair in the int16 halves of one LDS dword with -inf stored as -32768, the int16 score of a packed edge.  The other suites
run them on BLOSUM62-sized numbers and random peptides; a one-unit or signedness slip in any of these shows only at the inputs
below (tests/gapped_ends.py builds them).  Everything is integer and every comparison is exact; expectations come from
tests/global_ref.py (global) and the C oracle's scorer 1 (local), never from another GPU result.

Which kernel a case reaches follows from the host dispatch (hmk_pass.cpp: launch_plan_local, local_enc, local_literal, score_block;
k_global.hip / k_local.hip: the launchers), restated here as global_tier / local_tier / local_form / bucket and asserted per case by
test_every_case_reaches_the_tier_it_is_meant_for:

  k_neighbors_global<16>       test_global_16_against_32 (short16), strips <16, 4> and <16, 1 | 2 | 3> (every la = 1..16), lb = 1..16
  k_neighbors_global<32>       the same test on short17; test_global_register_ends (long32: la, lb up to 32, la & 3 = 0..3)
  k_neighbors_global_literal   test_global_tier_boundary (128 / -128), test_global_literal_ends (+-1,000: 32,000 and -8,128)
  k_pairs<2>                   test_global_block_and_pairs (score_block_global, score_pairs_global)
  k_neighbors_local_pk<12 | 20 | 32, true>    test_local_ends, tagged cases with gap_open <= -1 (last strip of 1..3 lines: la & 3)
  k_neighbors_local_pk<12 | 20 | 32, false>   tagged cases with gap_open = 0; every enc31 case under HMK_LOCAL_SIGNED
  k_neighbors_local<12 | 20 | 32, true>       every enc31 case under HMK_LOCAL_NO_PK
  k_neighbors_local<12 | 20 | 32, false>      the plain cases (entry 32 / -32, penalty -32, reg127)
  k_neighbors_local_literal    lit128, litm128, lit1000 and the positive penalty
  k_local_block_pk<12 | 20 | 32, true | false>, k_local_block<20 | 32, true | false>, k_pairs<1>
                               score_block_local of the same cases, in the same order
The five sets of local_lens have their longest sequence at 12, 13, 20, 21 and 32: both sides of either bucket boundary.

The CPU tests run anywhere and prove that the inputs hold what the GPU cases claim; the GPU tests need an MI355X (-m gpu)."""
import functools
import re
import types

import numpy as np
import pytest

from test_assign import gpu   # noqa: F401  (the fixture that skips where no HIP device is visible)
from test_global import ctx_with, oracle_greedy, ordered_edges, rand_seq, triangle_edges

import gapped_ends as E
import global_ref as G
import hammock_amd

KEEP_ALL = -30000
GLOBAL_PENALTIES = ((-5, -1), (-127, -127), (-127, 0), (0, 0), (-63, -63))
SETS = {"short16": E.short16, "short17": E.short17, "long32": E.long32}
W, B, C_, D = E.W, E.B, E.C_, E.LOW[0]


# ---- the dispatch, restated -------------------------------------------------------------------------------------------------------

def global_tier(M, longest):
    """launch_plan_local / launch_neighbors_global: register <=> -127 <= min M and max M <= 127; <16> <=> the longest sequence <= 16"""
    if M.min() < -127 or M.max() > 127:
        return "literal"
    return "<16>" if longest <= 16 else "<32>"


def local_tier(M, go, ge):
    """local_literal, then local_enc (hmk_pass.cpp)"""
    if go > 0 or ge > 0 or M.min() < -127 or M.max() > 127:
        return "literal"
    if M.min() >= -31 and M.max() <= 31 and -31 <= go <= 0 and -31 <= ge <= 0:
        return "tagged"
    return "plain"


def local_form(tier, go, switch=None):
    """launch_neighbors_local / launch_local_block: the form of the tagged tier"""
    if tier != "tagged":
        return tier
    if switch == "HMK_LOCAL_NO_PK":
        return "unpacked-tagged"
    return "packed-signed" if go == 0 or switch == "HMK_LOCAL_SIGNED" else "packed-saturating"


def bucket(longest):
    return 12 if longest <= 12 else 20 if longest <= 20 else 32


# (test, set, matrix, penalties, tier)
GLOBAL_CASES = (
    [("16 against 32", s, m, p, t) for s, t in (("short16", "<16>"), ("short17", "<32>")) for m in ("blosum62", "reg127", "reg127a")
     for p in GLOBAL_PENALTIES]
    + [("register ends", "long32", m, p, "<32>") for m in ("reg127", "reg127a") for p in GLOBAL_PENALTIES]
    + [("tier boundary", "long32", m, p, "literal") for m in ("lit128", "litm128") for p in ((-127, -127), (-5, -1))]
    + [("literal ends", "long32", m, p, "literal") for m in ("lit1000", "lit1000a") for p in ((-127, -127), (-5, -1))])

ENC31_PENALTIES = ((-31, -31), (-31, 0), (0, -31), (0, 0), (-1, -31))
# (matrix, gap_open, gap_extend, tier)
LOCAL_CASES = (
    [("enc31", go, ge, "tagged") for go, ge in ENC31_PENALTIES]
    + [("enc32", -31, -31, "plain"), ("encm32", -31, -31, "plain"), ("enc31", -32, -1, "plain"), ("enc31", -1, -32, "plain"),
       ("reg127", -127, -127, "plain"), ("reg127", -5, -1, "plain"),
       ("lit128", -40, -9, "literal"), ("litm128", -40, -9, "literal"), ("lit1000", -40, -9, "literal"), ("enc31", 1, -2, "literal")])


# ---- references, computed once ----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def global_table(set_name, matrix_name, go, ge):
    """T[i, j] = global(seq1 = i, seq2 = j) of tests/global_ref.py; short16 is the leading block of short17 (the same sequences)"""
    if set_name == "short16":
        n = len(E.short16())
        T = global_table("short17", matrix_name, go, ge)[:n, :n].copy()
    else:
        T = G.global_table(list(SETS[set_name]()), E.matrix(matrix_name), go, ge)
    T.setflags(write=False)
    return T


@functools.lru_cache(maxsize=None)
def local_table(longest, matrix_name, go, ge):
    """T[i, j] = local(seq1 = i, seq2 = j) of the C oracle on local_lens(longest)"""
    from oracle import c_oracle
    words = E.local_lens(longest)
    res, off = hammock_amd.pack_sequences(list(words))
    idx = np.arange(len(words), dtype=np.uint32)
    st, T = c_oracle.score_block(E.matrix(matrix_name), res, off, idx, idx, 1, go, ge)
    assert st == 0
    T = np.asarray(T, dtype=np.int64)
    T.setflags(write=False)
    return T


def off_diagonal(T):
    return T[~np.eye(T.shape[0], dtype=bool)]


def edges_of(T, thr, sym):
    return triangle_edges(T, thr) if sym else ordered_edges(T, thr)


# ---- CPU: the reference at extreme parameters -------------------------------------------------------------------------------------

def test_reference_equals_the_brute_force_at_extreme_parameters():
    """the existing pin of global_ref uses BLOSUM62 and penalties >= -15; here entries of +-127 and +-1,000 and the ends of the penalty
    range, on words that hold the planted residues"""
    rng = np.random.default_rng(11)
    letters = np.array([W, B, C_, *E.LOW, 0, 9, 17, 4], dtype=np.uint8)
    for name in ("reg127", "reg127a", "lit1000"):
        M = E.matrix(name)
        for k in range(60):
            a = letters[rng.integers(0, len(letters), rng.integers(1, 7))]
            b = letters[rng.integers(0, len(letters), rng.integers(1, 7))]
            go, ge = GLOBAL_PENALTIES[k % len(GLOBAL_PENALTIES)] if k % 6 else (-1, -1)
            want = G.brute_force(a, b, M, go, ge)
            assert G.global_score(a, b, M, go, ge) == want, (name, a, b, go, ge)
            assert int(G.global_class([a], [b], M, go, ge)[0, 0]) == want


# ---- CPU: the values the inputs reach ----------------------------------------------------------------------------------------------

def run(r, L):
    return E.run(r, L)


REACHED = (("lit1000", (-127, -127), run(W, 32), run(W, 32), 32000),
           ("lit1000", (-127, -127), run(C_, 32), run(D, 32), -8128),
           ("lit1000", (-5, -1), run(W, 30), run(W, 30), 30000),
           ("lit1000", (-5, -1), run(W, 30), E.w_run_b(30), 29999),
           ("lit1000a", (-5, -1), run(W, 30), E.w_run_b(30), 29999),
           ("reg127", (-127, -127), run(C_, 32), run(D, 32), -4064),
           ("reg127", (-63, -63), run(C_, 32), run(D, 32), -4032),   # the all-gap alignment wins
           ("reg127", (-63, -63), run(C_, 32), run(D, 1), -2079),
           ("reg127", (-127, 0), run(C_, 32), run(D, 32), -254),
           ("reg127", (0, 0), run(C_, 32), run(D, 32), 0))


def test_values_the_inputs_reach(coracle):
    """W / B is one below W / W, so the only pair of two sequences that scores what W^L scores against itself is W^L and its twin:
    the sets hold W^30, W^32 (long32) and each local set's longest W-word twice"""
    words = E.long32()
    for name, (go, ge), a, b, want in REACHED:
        assert G.global_score(a, b, E.matrix(name), go, ge) == want, (name, go, ge, want)
        for w in (a, b):
            E.indices_of(words, w, 2 if len(w) >= 30 and w[0] == W and w[-1] == W else 1)
    for go, ge in GLOBAL_PENALTIES:
        assert G.global_score(run(W, 32), run(W, 32), E.matrix("reg127"), go, ge) == 4064
        assert G.global_score(run(W, 32), E.w_run_b(32), E.matrix("reg127a"), go, ge) == 4064     # W / B = 127 ...
        assert G.global_score(E.w_run_b(32), run(W, 32), E.matrix("reg127a"), go, ge) <= 4064 - 127   # ... B / W = -127 (or two free gaps)
    T = global_table("long32", "lit1000", -127, -127)
    assert off_diagonal(T).max() == 32000 and off_diagonal(T).min() == -8128
    T = global_table("long32", "reg127", -127, -127)
    assert off_diagonal(T).max() == 4064 and off_diagonal(T).min() == -4064
    # local: the top 32-mer and its twin; two distinct top words are one below
    assert coracle.local_score(E.matrix("enc31"), run(W, 32), run(W, 32), -31, -31) == 992 == 4 * 8 * 31
    assert coracle.local_score(E.matrix("enc31"), run(W, 32), E.w_run_b(32), -31, -31) == 991
    assert coracle.local_score(E.matrix("lit1000"), run(W, 32), run(W, 32), -40, -9) == 32000
    E.indices_of(E.local_lens(32), run(W, 32), 2)
    assert off_diagonal(local_table(32, "enc31", -31, -31)).max() == 992
    assert off_diagonal(local_table(32, "lit1000", -40, -9)).max() == 32000
    for longest in E.LOCAL_MAX:   # every bucket's set reaches its own top
        assert off_diagonal(local_table(longest, "enc31", -31, -31)).max() == 31 * longest


# ---- CPU: witnesses ----------------------------------------------------------------------------------------------------------------
# A deliberately wrong variant of the recurrence per slip; each must give another answer than the reference for a pair of the set the
# matching GPU case runs, or that case could not fail for the slip it is there for.

def slug(*parts):
    return re.sub(r"[^A-Za-z0-9-]+", "_", "_".join(str(p) for p in parts)).strip("_")


def wrap(v, bits):
    half = 1 << (bits - 1)
    return ((v + half) & ((1 << bits) - 1)) - half


def global_model(s1, s2, M, go, ge, sub=None, pad_lines=False, h0j=0, hi0=0, f16=False, mask15=False, h_u16=False, swap=False):
    """the recurrence the way the kernels walk it (line by line, H and F of the line above kept per column), with one slip switched on:
    sub        what the DP reads for a matrix entry (a profile byte read unsigned, clamped, wrapped)
    pad_lines  the last strip run with 4 lines, the missing ones scored -128; the result read after the strip's last line
    h0j, hi0   H[0][j] / H[i][0] off by that many gap_extend
    f16        F kept in 16 bits: -inf = -32768 wraps after one more penalty
    mask15     the final score masked to 15 bits
    h_u16      H of the stored cell read back as uint16
    swap       seq1 and seq2 swapped"""
    if swap:
        s1, s2 = s2, s1
    sub = sub or (lambda v: v)
    lines = [[sub(int(M[a][b])) for b in s2] for a in s1]
    m = len(s2)
    if pad_lines:
        lines += [[-128] * m for _ in range(-len(lines) % 4)]
    back = (lambda h: h & 0xFFFF) if h_u16 else (lambda h: h)
    H = [0] + [go + (j - 1 + h0j) * ge for j in range(1, m + 1)]
    F = [-32768 if f16 else G.NEG] * (m + 1)
    for i in range(1, len(lines) + 1):
        left = go + (i - 1 + hi0) * ge
        Hn, Fn, e = [left], [left], G.NEG
        for j in range(1, m + 1):
            e = max(e + ge, Hn[j - 1] + go)
            f = max(wrap(F[j] + ge, 16) if f16 else F[j] + ge, back(H[j]) + go)
            Hn.append(max(back(H[j - 1]) + lines[i - 1][j - 1], e, f))
            Fn.append(f)
        H, F = Hn, Fn
    return H[m] & 0x7FFF if mask15 else H[m]


def local_tagged_model(s1, s2, M, go, ge):
    """the tagged-max form (k_local.hip: sw_row, ENC): every candidate is 4 * value + tag, the next cell's penalty a byte looked up
    by tag and the profile a byte of 4 * score, both read back as int8"""
    def b(v):
        return wrap(v, 8)
    PU = (b(4 * go + 2), b(4 * go + 1), b(4 * ge), b(4 * go - 1))
    PL = (b(4 * go + 1), b(4 * ge), b(4 * go - 1), b(4 * go - 2))
    m = len(s2)
    H, U = [3] * (m + 1), [4 * go + 2] * (m + 1)
    gm = 0
    for a in s1:
        hd, lc = 3, 4 * go + 1
        for j in range(1, m + 1):
            he = max(hd + b(4 * int(M[a][s2[j - 1]])), U[j], lc, 0)
            gm = max(gm, he)
            hd, H[j] = H[j], he | 3
            U[j], lc = he + PU[he & 3], he + PL[he & 3]
    return gm >> 2


def probe_pairs(words):
    """index pairs of a set, the words over {W, B} and over {C, D, E, N, Q} first and the longest first among them"""
    ends = [k for k, w in enumerate(words) if set(w.tolist()) <= {W, B} or set(w.tolist()) <= {C_, *E.LOW}]
    ends.sort(key=lambda k: -len(words[k]))
    idx = ends[:10] + ends[-4:] + list(range(0, len(words), max(1, len(words) // 10)))
    return [(i, j) for i in idx for j in idx if i != j]


def differs(words, M, penalties, **slip):
    """the first pair of the set (and penalties) at which the slipped model and the reference part, or None"""
    for i, j in probe_pairs(words):
        for go, ge in penalties:
            want = G.global_score(words[i], words[j], M, go, ge)
            if global_model(words[i], words[j], M, go, ge, **slip) != want:
                return i, j, go, ge
    return None


GLOBAL_WITNESSES = (
    # slip, the set and matrix of the GPU case that is there for it, the slip
    ("a profile byte read unsigned", "short16", "reg127", dict(sub=lambda v: v & 0xFF)),
    ("a profile byte read unsigned", "long32", "reg127", dict(sub=lambda v: v & 0xFF)),
    ("a profile byte clamped to +-126", "short16", "reg127", dict(sub=lambda v: max(-126, min(126, v)))),
    ("a profile byte clamped to +-126", "long32", "reg127a", dict(sub=lambda v: max(-126, min(126, v)))),
    ("an entry of 128 wrapped to int8", "long32", "lit128", dict(sub=lambda v: wrap(v, 8))),
    ("an entry of -128 clamped to -127", "long32", "litm128", dict(sub=lambda v: max(-127, v))),
    ("the last strip run with 4 lines", "short16", "reg127", dict(pad_lines=True)),
    ("the last strip run with 4 lines", "long32", "reg127", dict(pad_lines=True)),
    ("H[0][j] off by one gap_extend", "short16", "reg127", dict(h0j=1)),
    ("H[i][0] off by one gap_extend", "short16", "reg127", dict(hi0=1)),
    ("H[0][j] off by one gap_extend", "long32", "reg127", dict(h0j=-1)),
    ("H[i][0] off by one gap_extend", "long32", "reg127", dict(hi0=-1)),
    ("F's -inf wrapped in 16 bits", "long32", "lit1000", dict(f16=True)),
    ("F's -inf wrapped in 16 bits", "short16", "reg127", dict(f16=True)),
    ("the final score masked to 15 bits", "long32", "lit1000", dict(mask15=True)),
    ("H of the literal cell read as uint16", "long32", "lit1000", dict(h_u16=True)),
    ("H of the literal cell read as uint16", "long32", "lit128", dict(h_u16=True)),
    ("seq1 and seq2 swapped", "short16", "reg127a", dict(swap=True)),
    ("seq1 and seq2 swapped", "long32", "reg127a", dict(swap=True)),
    ("seq1 and seq2 swapped", "long32", "lit1000a", dict(swap=True)),
)


def test_the_model_without_a_slip_is_the_reference():
    for set_name, name in (("short16", "reg127a"), ("long32", "lit1000a")):
        words = SETS[set_name]()
        assert differs(words, E.matrix(name), ((-5, -1), (-127, -127)), ) is None


@pytest.mark.parametrize("what,set_name,matrix_name,slip", GLOBAL_WITNESSES, ids=[slug(*w[:3]) for w in GLOBAL_WITNESSES])
def test_global_witnesses_differ_on_the_set_of_their_case(what, set_name, matrix_name, slip):
    penalties = [p for t, s, m, p, _ in GLOBAL_CASES if (s, m) == (set_name, matrix_name)]
    assert penalties, "no GPU case runs this set under this matrix"
    found = differs(SETS[set_name](), E.matrix(matrix_name), penalties, **slip)
    assert found is not None, what
    # (-128 IS an int8, so wrapping it changes nothing and no set could show it; what an off-by-one at that end of the predicate would
    # do is meet the profile's pad value -128 or a clamp to the register tier's range: the witness for litm128 is the clamp)
    assert wrap(-128, 8) == -128 and wrap(128, 8) == -128


def test_local_witnesses_differ_on_the_set_of_their_case(coracle):
    """inside the tagged tier the model is the oracle; one step outside, with the byte wrapped, it is not: (-32, -1) makes the table
    byte 4 * gap_open - 2 = -130, entry 32 the profile byte 128"""
    def first_difference(longest, name, go, ge):
        words, M, T = E.local_lens(longest), E.matrix(name), local_table(longest, name, go, ge)
        for i, j in probe_pairs(words):
            if local_tagged_model(words[i], words[j], M, go, ge) != T[i, j]:
                return i, j
        return None
    for longest in E.LOCAL_MAX:
        for go, ge in ENC31_PENALTIES:
            assert first_difference(longest, "enc31", go, ge) is None, (longest, go, ge)
        assert wrap(4 * -32 - 2, 8) == 126 and wrap(4 * -31 - 2, 8) == -126 and wrap(4 * 32, 8) == -128 and wrap(4 * 31, 8) == 124
        assert first_difference(longest, "enc31", -32, -1) is not None, longest
        assert first_difference(longest, "enc32", -31, -31) is not None, longest
    assert 4 * 32 * 31 + 3 < 1 << 15   # the largest tagged value, reached by the top 32-mer and its twin, fits an int16 half


# ---- CPU: tiers ---------------------------------------------------------------------------------------------------------------------

def test_every_case_reaches_the_tier_it_is_meant_for():
    reached = set()
    for _, set_name, name, (go, ge), tier in GLOBAL_CASES:
        M = E.matrix(name)
        assert -127 <= go <= ge <= 0
        assert global_tier(M, max(len(w) for w in SETS[set_name]())) == tier, (set_name, name)
        reached.add((tier, int(M.min()) if M.min() <= -127 else None, int(M.max()) if M.max() >= 127 else None))
    assert {t for t, _, _ in reached} == {"<16>", "<32>", "literal"}
    for tier, lo, hi in (("<16>", -127, 127), ("<32>", -127, 127), ("literal", -127, 128), ("literal", -128, 127), ("literal", -1000, 1000)):
        assert (tier, lo, hi) in reached   # either side of 127 | 128 and of -127 | -128
    forms = set()
    sides = set()
    for name, go, ge, tier in LOCAL_CASES:
        M = E.matrix(name)
        assert local_tier(M, go, ge) == tier, (name, go, ge)
        for switch in (None, "HMK_LOCAL_SIGNED", "HMK_LOCAL_NO_PK") if name == "enc31" and tier == "tagged" else (None,):
            forms.add(local_form(tier, go, switch))
        sides.add((tier, int(M.min()), int(M.max()), min(go, ge), max(go, ge)))
    assert forms == {"packed-saturating", "packed-signed", "unpacked-tagged", "plain", "literal"}
    for side in (("tagged", -31, 31, -31, -31), ("plain", -31, 32, -31, -31), ("plain", -32, 31, -31, -31),   # entry 31 | 32, -31 | -32
                 ("plain", -31, 31, -32, -1),                                                                  # penalty -31 | -32
                 ("tagged", -31, 31, 0, 0), ("literal", -31, 31, -2, 1),                                       # penalty 0 | positive
                 ("plain", -127, 127, -127, -127), ("literal", -127, 128, -40, -9), ("literal", -128, 127, -40, -9),   # 127 | 128, -127 | -128
                 ("literal", -1000, 1000, -40, -9)):
        assert side in sides, side
    assert [bucket(k) for k in E.LOCAL_MAX] == [12, 20, 20, 32, 32]
    # the context's own bound on the edge score: 32 * 1,000 fits, and with it the threshold range
    assert 32 * 1000 <= 32767 and 30000 < 32 * 1000


# ---- CPU: two restatements of LocalAlignmentScorer ------------------------------------------------------------------------------------

def test_local_oracles_agree_on_the_ends_pairs(coracle):
    from oracle import hammock_oracle as ho
    for longest, cases in ((12, LOCAL_CASES), (32, LOCAL_CASES[::3]), (21, LOCAL_CASES[1::4])):
        words = E.local_lens(longest)
        pairs = probe_pairs(words)[::3]
        for name, go, ge, _ in cases:
            T = local_table(longest, name, go, ge)
            scorer = ho.LocalAlignmentScorer(E.matrix(name).tolist(), go, ge)
            for i, j in pairs:
                got = scorer.sequence_score(types.SimpleNamespace(sequence=words[i].tolist()), types.SimpleNamespace(sequence=words[j].tolist()))
                assert got == T[i, j], (longest, name, go, ge, i, j)


# ---- GPU: global --------------------------------------------------------------------------------------------------------------------

def neighbours_match(ctx, T, go, ge, thr, sym, **parts):
    """neighbors_global at thr: the sorted edges are the reference's; -> the sorted edges"""
    n = T.shape[0]
    edges, st = ctx.neighbors_global(go, ge, thr, **parts)
    edges = np.sort(edges)
    if not parts:
        assert st.pairs_scored == (n * (n - 1) // 2 if sym else n * (n - 1)) and st.symmetric == int(sym)
        want = edges_of(T, thr, sym)
        assert len(edges) == len(want), (thr, len(edges), len(want))
        assert np.array_equal(edges, want), thr
    return edges, st


def quantile(T, q):
    """a selective threshold: the value below which the share q of the pairs lies"""
    v = np.sort(off_diagonal(T))
    return int(v[int(q * (len(v) - 1))])


@pytest.mark.gpu
@pytest.mark.parametrize("go,ge", GLOBAL_PENALTIES)
@pytest.mark.parametrize("matrix_name", ["blosum62", "reg127", "reg127a"])
def test_global_16_against_32(gpu, matrix_name, go, ge):
    """the same pairs on k_neighbors_global<16> (short16: every strip form, 17 row chunks of the 13-mers, the last of 4 rows) and, behind
    one 17-mer, on <32>: every pair at -30000, both against the reference and against each other"""
    M, sym = E.matrix(matrix_name), E.symmetric(matrix_name)
    n16 = len(E.short16())
    per_set = {}
    for set_name in ("short16", "short17"):
        T = global_table(set_name, matrix_name, go, ge)
        ctx = ctx_with(M, list(SETS[set_name]()))
        per_set[set_name], _ = neighbours_match(ctx, T, go, ge, KEEP_ALL, sym)
        assert len(per_set[set_name]) == T.shape[0] * (T.shape[0] - 1) // (2 if sym else 1)
    x, m, _ = hammock_amd.edge_fields(per_set["short17"])
    assert np.array_equal(per_set["short17"][(x < n16) & (m < n16)], per_set["short16"])


@pytest.mark.gpu
@pytest.mark.parametrize("matrix_name,go,ge", [("reg127", -63, -63), ("reg127a", -127, 0)])
def test_global_16_parts_and_a_selective_threshold(gpu, matrix_name, go, ge):
    M, sym = E.matrix(matrix_name), E.symmetric(matrix_name)
    T = global_table("short16", matrix_name, go, ge)
    n = T.shape[0]
    ctx = ctx_with(M, list(E.short16()))
    thr = quantile(T, 0.97)
    assert T.min() < thr < T.max()
    want = edges_of(T, thr, sym)
    assert 0.01 * len(off_diagonal(T)) <= len(want) * (2 if sym else 1) <= 0.1 * len(off_diagonal(T))
    neighbours_match(ctx, T, go, ge, thr, sym)
    for thr_p in (thr, KEEP_ALL):
        parts, pairs = [], 0
        for part in range(3):
            e, st = neighbours_match(ctx, T, go, ge, thr_p, sym, part=part, n_parts=3)
            parts.append(e)
            pairs += st.pairs_scored
        assert pairs == (n * (n - 1) // 2 if sym else n * (n - 1))
        assert all(len(e) for e in parts)
        assert np.array_equal(np.sort(np.concatenate(parts)), edges_of(T, thr_p, sym))


def search_matches(ctx, T, go, ge, thr, q, r):
    """search_global(queries q, references r) at thr against the block T[q, r]"""
    edges, st = ctx.search_global(q[0], q[-1] + 1, r[0], r[-1] + 1, go, ge, thr)
    assert st.pairs_scored == len(q) * len(r)
    want = ordered_edges(T[np.ix_(q, r)], thr, q, r)
    assert len(edges) == len(want), (thr, len(edges), len(want))
    assert np.array_equal(np.sort(edges), want), thr
    return len(edges)


def neighbours_and_search(matrix_name, go, ge, thresholds=None):
    """long32 through neighbors_global and search_global (the first 40 sequences against the rest, then the rest against them) at
    -30000, at the lowest score and one above it: the pair at the minimum is kept, kept, dropped"""
    M, sym = E.matrix(matrix_name), E.symmetric(matrix_name)
    T = global_table("long32", matrix_name, go, ge)
    n = T.shape[0]
    ctx = ctx_with(M, list(E.long32()))
    head, tail = np.arange(40), np.arange(40, n)
    blocks = [(None, None, np.triu(T, 1)[np.triu_indices(n, 1)] if sym else off_diagonal(T)), (head, tail, T[:40, 40:]), (tail, head, T[40:, :40])]
    for q, r, values in blocks:
        lo = int(values.min())
        at_lo = int(np.count_nonzero(values == lo))
        counts = []
        for thr in (KEEP_ALL, lo, lo + 1) + tuple(thresholds or ()):
            if q is None:
                counts.append(len(neighbours_match(ctx, T, go, ge, thr, sym)[0]))
            else:
                counts.append(search_matches(ctx, T, go, ge, thr, q, r))
        assert counts[0] == counts[1] == values.size and counts[2] == values.size - at_lo and at_lo >= 1
    return ctx, T


@pytest.mark.gpu
@pytest.mark.parametrize("go,ge", GLOBAL_PENALTIES)
@pytest.mark.parametrize("matrix_name", ["reg127", "reg127a"])
def test_global_register_ends(gpu, matrix_name, go, ge):
    """entries of +-127 (the last value the int8 profile holds) at the ends of the penalty range, lengths up to 32 with every la & 3"""
    neighbours_and_search(matrix_name, go, ge)


@pytest.mark.gpu
@pytest.mark.parametrize("go,ge", [(-127, -127), (-5, -1)])
@pytest.mark.parametrize("matrix_name", ["lit128", "litm128"])
def test_global_tier_boundary(gpu, matrix_name, go, ge):
    """one entry one step beyond int8: the literal kernel, or 128 would read back as -128"""
    neighbours_and_search(matrix_name, go, ge)


@pytest.mark.gpu
@pytest.mark.parametrize("matrix_name", ["lit1000", "lit1000a"])
def test_global_literal_ends(gpu, matrix_name):
    """entries of +-1,000, the largest a context takes: H = 32,000 and H, F down to -8,128 - 254 in the int16 halves of the literal
    DP's cell, edge scores of 32,000 and -8,128, and the thresholds +-30,000 with a pair exactly there"""
    sym = E.symmetric(matrix_name)
    ctx, T = neighbours_and_search(matrix_name, -127, -127)
    everything, _ = neighbours_match(ctx, T, -127, -127, KEEP_ALL, sym)
    _, _, s = hammock_amd.edge_fields(everything)
    assert s.max() == 32000 and s.min() == -8128
    ctx, T = neighbours_and_search(matrix_name, -5, -1, thresholds=(30000, 29999))
    words = E.long32()
    (a, a2), (b,) = E.indices_of(words, E.run(W, 30), 2), E.indices_of(words, E.w_run_b(30))
    assert T[a, a2] == T[a2, a] == 30000 and T[a, b] == 29999   # seq1 = W^30, seq2 = W^29 B
    at = {thr: neighbours_match(ctx, T, -5, -1, thr, sym)[0] for thr in (30000, 29999)}
    # a symmetric pass stores (min, max); every other pass m = seq1, x = seq2
    top = hammock_amd.pack_edges([min(a, a2)], [max(a, a2)], [30000]) if sym else hammock_amd.pack_edges([a2], [a], [30000])
    below = hammock_amd.pack_edges([min(a, b)], [max(a, b)], [29999]) if sym else hammock_amd.pack_edges([b], [a], [29999])
    assert np.isin(top, at[30000]).all() and np.isin(top, at[29999]).all()
    assert not np.isin(below, at[30000]).any() and np.isin(below, at[29999]).all()
    for thr in (30001, -30001):
        with pytest.raises(ValueError):
            ctx.neighbors_global(-5, -1, thr)
        with pytest.raises(ValueError):
            ctx.search_global(0, 40, 40, len(words), -5, -1, thr)


@pytest.mark.gpu
@pytest.mark.parametrize("matrix_name,penalties", [("lit1000", ((-127, -127), (-5, -1))), ("lit1000a", ((-127, -127), (-5, -1))),
                                                   ("reg127", GLOBAL_PENALTIES)])
def test_global_block_and_pairs(gpu, matrix_name, penalties):
    """k_pairs<2>, the literal DP one pair per lane: the whole set as a block (self pairs too: 32,000) and as pairs in both orders"""
    words = E.long32()
    n = len(words)
    ctx = ctx_with(E.matrix(matrix_name), list(words))
    i, j = np.divmod(np.arange(n * n), n)
    for go, ge in penalties:
        T = global_table("long32", matrix_name, go, ge)
        assert np.array_equal(ctx.score_block_global(0, n, 0, n, go, ge), T)
        assert np.array_equal(ctx.score_pairs_global(i, j, go, ge), T[i, j])
        assert np.array_equal(ctx.score_pairs_global(j, i, go, ge), T[j, i])


# ---- GPU: local ---------------------------------------------------------------------------------------------------------------------

def local_case(longest, name, go, ge):
    """score_block_local of the whole set and neighbors_local at 0 (every ordered pair) and at a selective threshold"""
    words = E.local_lens(longest)
    n = len(words)
    T = local_table(longest, name, go, ge)
    ctx = ctx_with(E.matrix(name), list(words))
    assert np.array_equal(ctx.score_block_local(0, n, 0, n, go, ge), T), (longest, name, go, ge)
    thr = max(quantile(T, 0.9), 1)
    for t in (0, thr):
        edges, st = ctx.neighbors_local(go, ge, t)
        want = ordered_edges(T, t)
        assert st.pairs_scored == n * (n - 1)
        assert len(edges) == len(want), (longest, name, go, ge, t)
        assert np.array_equal(np.sort(edges), want), (longest, name, go, ge, t)
    assert len(want) < len(edges_all(T)) // 4
    return np.sort(edges)


def edges_all(T):
    return ordered_edges(T, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name,go,ge,tier", LOCAL_CASES, ids=[slug(*c) for c in LOCAL_CASES])
@pytest.mark.parametrize("longest", E.LOCAL_MAX)
def test_local_ends(gpu, longest, name, go, ge, tier):
    local_case(longest, name, go, ge)


@pytest.mark.gpu
@pytest.mark.parametrize("go,ge", ENC31_PENALTIES)
@pytest.mark.parametrize("switch", ["HMK_LOCAL_SIGNED", "HMK_LOCAL_NO_PK"])
@pytest.mark.parametrize("longest", E.LOCAL_MAX)
def test_local_ends_in_the_other_tagged_forms(gpu, monkeypatch, longest, switch, go, ge):
    """the enc31 cases on the signed packed form and on the one-column-per-lane tagged form: the same edges (the oracle's)"""
    monkeypatch.setenv(switch, "1")
    local_case(longest, "enc31", go, ge)


# ---- GPU: edit distance at a negative threshold ------------------------------------------------------------------------------------------

def edit_family_set():
    """300 distinct sequences of lengths 11..13 in families: a seed, then variants one and two edits away (substitution, insertion,
    deletion), so indels cross the length classes"""
    rng = np.random.default_rng(12)
    seqs, seen = [], set()

    def edit(s):
        kind = rng.integers(0, 3)
        if kind == 1 and len(s) < 13:
            return np.insert(s, rng.integers(0, len(s) + 1), rng.integers(0, 20)).astype(np.uint8)
        if kind == 2 and len(s) > 11:
            return np.delete(s, rng.integers(0, len(s)))
        s = s.copy()
        s[rng.integers(0, len(s))] = rng.integers(0, 20)
        return s

    while len(seqs) < 300:
        seed = rand_seq(rng, rng.integers(11, 14))
        one = edit(seed)
        for s in (seed, one, edit(seed), edit(one), rand_seq(rng, rng.integers(11, 14))):
            if s.tobytes() not in seen:
                seen.add(s.tobytes())
                seqs.append(s)
    seqs = seqs[:300]
    return [seqs[k] for k in rng.permutation(300)]


def test_edit_family_set_crosses_length_classes():
    seqs = edit_family_set()
    assert {len(s) for s in seqs} == {11, 12, 13}
    T = G.global_table(seqs, G.edit_matrix(), -1, -1)
    i, j = np.nonzero(np.triu(T >= -2, 1))
    assert len(i) >= 150
    assert sum(1 for a, b in zip(i, j) if len(seqs[a]) != len(seqs[b])) >= 40
    for a, b in list(zip(i, j))[:60]:
        assert T[a, b] == -G.levenshtein(seqs[a], seqs[b])


@pytest.mark.gpu
def test_edit_distance_two_composes_with_greedy_and_components(gpu):
    """the scorer's documented use -- the 0 / -1 matrix at -1 / -1, threshold -2 -- fed into the clustering calls: negative scores in
    greedy_from_edges and components_from_edges"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    seqs, thr, maxc = edit_family_set(), -2, 40
    n = len(seqs)
    T = G.global_table(seqs, G.edit_matrix(), -1, -1)
    ctx = ctx_with(G.edit_matrix(), seqs)
    edges, st = ctx.neighbors_global(-1, -1, thr)
    assert st.symmetric == 1
    assert np.array_equal(np.sort(edges), triangle_edges(T, thr))
    cid, order, _ = ctx.greedy_from_edges(edges, True, thr, maxc)
    ocid, oorder, orank = oracle_greedy(seqs, T, thr, maxc)
    assert len(set(ocid.tolist())) < n - 20   # real clusters
    assert cid.tolist() == ocid.tolist()
    assert order.tolist() == oorder
    assert ctx.member_rank[:n].tolist() == orank.tolist()
    comp, _ = ctx.components_from_edges(edges, thr)
    i, j = np.nonzero(np.triu(T >= thr, 1))
    _, label = connected_components(coo_matrix((np.ones(len(i)), (i, j)), shape=(n, n)), directed=False)
    smallest = np.full(label.max() + 1, n)
    np.minimum.at(smallest, label, np.arange(n))
    assert np.asarray(comp).tolist() == smallest[label].tolist()
