"""The tile kernels' hit stage at its edge: thresholds that keep EVERY pair, so all 64 lanes of a wave hit on consecutive rows
and a wave's record count lands exactly on capacity - 64 and then on capacity (the parity tests keep 2-3 % of the pairs and
never get there).  Every staging tile kernel outside the row-packed pass: the local DP in its four forms, the global DP, the
three literal kernels, k_neighbors_planes' packed records and (on a set built for it) k_neighbors_swar's compact ones.  Bit-exact against the oracle; first the oracle's
own edge count is checked to be all n (n - 1) pairs (n (n - 1) / 2 for a symmetric pass), so no case passes while sparse."""
import numpy as np
import pytest

import global_ref as G
import hammock_amd
from hammock_amd.synth import synth_peptides

pytestmark = pytest.mark.gpu

# two lengths each, 200 + 140 sequences: per class column runs of full waves and a partial one, and 9 to 13 rows tiles of 16
SETS = {"short": (9, 12), "long": (14, 25)}
KEEP_ALL_GLOBAL = -30000


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need an MI355X; no HIP device is visible")
    return 0


def make_set(name):
    la, lb = SETS[name]
    seqs = []
    for seed, n, L in ((21, 200, la), (22, 140, lb)):
        res, off = synth_peptides(seed, n, L)
        seqs += [res[off[k]:off[k + 1]] for k in range(n)]
    return seqs


@pytest.fixture(scope="module")
def wide_matrix():
    """symmetric, entries in +-300: beyond int8 profiles and 16-bit shift lanes -- the literal kernels"""
    A = np.random.default_rng(31).integers(-300, 301, size=(24, 24)).astype(np.int32)
    return np.minimum(A, A.T)


class Ref:
    """a set and its oracle tables, each computed once and shared by the cases that need it"""

    def __init__(self, name, coracle):
        self.seqs = make_set(name)
        self.n = len(self.seqs)
        self.res, self.off = hammock_amd.pack_sequences(self.seqs)
        self.coracle = coracle
        self.tables = {}

    def table(self, M, scorer, a, b, idx=None):
        """T[i, j] = score(seq1 = i, seq2 = j); scorer 0 shifted, 1 local (the C oracle), 2 global (global_ref)"""
        key = (M.tobytes(), scorer, a, b, None if idx is None else idx.tobytes())
        if key not in self.tables:
            idx_ = np.arange(self.n, dtype=np.uint32) if idx is None else idx
            if scorer == 2:
                T = G.global_table([self.seqs[k] for k in idx_], M, a, b)
            else:
                st, T = self.coracle.score_block(M, self.res, self.off, idx_, idx_, scorer, a, b)
                assert st == 0
            T = np.asarray(T)
            T.setflags(write=False)
            self.tables[key] = T
        return self.tables[key]

    def ctx(self, M, idx=None):
        ctx = hammock_amd.Context(M, device=0)
        res, off = (self.res, self.off) if idx is None else hammock_amd.pack_sequences([self.seqs[k] for k in idx])
        ctx.set_sequences(residues=res, offsets=off)
        return ctx


@pytest.fixture(scope="module", params=sorted(SETS))
def ref(request, coracle):
    return Ref(request.param, coracle)


def ordered_edges(T, thr):
    """every ordered pair m != x with T[m, x] >= thr as the edge (x, m)"""
    m, x = np.nonzero(T >= thr)
    keep = m != x
    return np.sort(hammock_amd.pack_edges(x[keep], m[keep], T[m[keep], x[keep]]))


def triangle_edges(T, thr):
    """every unordered pair once, x < m, with T[m, x] >= thr (T symmetric)"""
    x, m = np.nonzero(np.triu(T >= thr, 1))
    return np.sort(hammock_amd.pack_edges(x, m, T[m, x]))


def check(edges, want, n_pairs, what):
    assert len(want) == n_pairs, (what, len(want), n_pairs)   # the oracle alone: every pair is kept
    assert np.array_equal(np.sort(edges), want), (what, len(edges), len(want))


@pytest.mark.parametrize("switch", [None, "HMK_LOCAL_SIGNED", "HMK_LOCAL_NO_PK", "HMK_LOCAL_LITERAL"])
def test_local_every_pair(gpu, ref, blosum62, monkeypatch, switch):
    """-5 / -1: the packed saturating DP (k_neighbors_local_pk, stage of 192), its signed form, the one-column-per-lane tagged DP
    and the literal kernel; threshold 0 keeps everything (a local score is never negative)"""
    want = ordered_edges(ref.table(blosum62, 1, -5, -1), 0)
    if switch:
        monkeypatch.setenv(switch, "1")
    edges, st = ref.ctx(blosum62).neighbors_local(-5, -1, 0)
    assert st.pairs_scored == ref.n * (ref.n - 1)
    check(edges, want, ref.n * (ref.n - 1), switch)


def test_local_plain_form_every_pair(gpu, ref, blosum62):
    """-40 / -9 is outside the tagged range: k_neighbors_local<., false>"""
    want = ordered_edges(ref.table(blosum62, 1, -40, -9), 0)
    edges, _ = ref.ctx(blosum62).neighbors_local(-40, -9, 0)
    check(edges, want, ref.n * (ref.n - 1), "plain")


def test_global_every_pair(gpu, ref, blosum62):
    want = triangle_edges(ref.table(blosum62, 2, -5, -1), KEEP_ALL_GLOBAL)
    edges, st = ref.ctx(blosum62).neighbors_global(-5, -1, KEEP_ALL_GLOBAL)
    assert st.symmetric == 1
    check(edges, want, ref.n * (ref.n - 1) // 2, "global")


def test_global_literal_every_pair(gpu, ref, wide_matrix):
    want = triangle_edges(ref.table(wide_matrix, 2, -40, -9), KEEP_ALL_GLOBAL)
    edges, st = ref.ctx(wide_matrix).neighbors_global(-40, -9, KEEP_ALL_GLOBAL)
    assert st.symmetric == 1
    check(edges, want, ref.n * (ref.n - 1) // 2, "global literal")


def test_shifted_direct_every_pair(gpu, ref, wide_matrix):
    T = ref.table(wide_matrix, 0, 3, -1)
    thr = int(T.min())
    edges, st = ref.ctx(wide_matrix).neighbors_shifted(3, -1, thr)
    print(f"direct: threshold {thr}, u8 {st.classes_u8} u16 {st.classes_u16} direct {st.classes_direct} rows {st.classes_rows}")
    assert st.classes_direct > 0 and st.symmetric == 1
    check(edges, triangle_edges(T, thr), ref.n * (ref.n - 1) // 2, "direct")


@pytest.mark.parametrize("subset", ["one length", "mixed"])
def test_shift_packed_every_pair(gpu, ref, blosum62, monkeypatch, subset):
    """HMK_NO_ROWS_KERNEL=1 on blosum62: k_neighbors_planes' packed records, one dword with 8-bit lanes and two with 16-bit lanes, on
    the set and on its longer length alone.  (A threshold below 5 leaves no (12, 12) class that fits 8-bit lanes for ANY pair, so not
    even the 12-mers alone run k_neighbors_swar here: test_swar_every_pair.)  The planner decides the lane width from score BOUNDS:
    - the (9, 9) class fits 8-bit lanes outright while 128 - thr + 9 * 11 <= 255, i.e. thr >= -28, so the short set runs 8-bit
      classes -- its threshold is asserted to be there;
    - a 25-mer's bound (the sum of its residues' best cells, >= 25 * 4 under blosum62) is beyond 127 + thr for every thr < -27, and
      every 25-mer then sits in a 16-bit class: the long set runs 16-bit classes."""
    monkeypatch.setenv("HMK_NO_ROWS_KERNEL", "1")
    lengths = np.asarray([len(s) for s in ref.seqs])
    idx = None if subset == "mixed" else np.nonzero(lengths == lengths.max())[0].astype(np.uint32)
    n = ref.n if idx is None else len(idx)
    T = ref.table(blosum62, 0, 3, -1, idx)
    thr = int(T.min())
    edges, st = ref.ctx(blosum62, idx).neighbors_shifted(3, -1, thr)
    print(f"shift-packed {subset} {sorted(set(lengths))}: threshold {thr}, u8 {st.classes_u8} u16 {st.classes_u16} direct {st.classes_direct}")
    assert st.classes_rows == 0 and st.classes_u8 + st.classes_u16 > 0   # (the (25, 14) class has 18 shift lanes, beyond a 16-bit entry: literal tier)
    if lengths.min() == 9 and subset == "mixed":
        assert thr >= -28 and st.classes_u8 > 0
    if lengths.max() == 25:
        assert thr < -27 and st.classes_u16 > 0
    check(edges, triangle_edges(T, thr), n * (n - 1) // 2, subset)


def test_swar_every_pair(gpu, blosum62, coracle, monkeypatch):
    """k_neighbors_swar's compact records at a full stage.  The kernel runs only on the exact path: every sequence a 12-mer, max
    shift 3, and a (12, 12) class whose 8-bit lanes fit ANY pair with no row bounds (hmk_plan.cpp: classify, pl.exact).  Under
    blosum62 (cells -4 .. 11) the lane of shift 0 tops at 128 - thr + 12 * 11 = 260 - thr and starts at 128 - thr - 48, so that
    needs 5 <= thr <= 80 -- no threshold that keeps every pair of random 12-mers.  Hence 340 variants of one tryptophan-rich core
    with one to three substitutions: their lowest pair score is the threshold, and it is asserted to lie in that range.  One length,
    one class, 8-bit lanes, nothing on 16-bit lanes or the literal tier: the exact path."""
    assert (blosum62.min(), blosum62.max()) == (-4, 11)
    core = hammock_amd.encode("WCHWYWCWWHCW")
    rng = np.random.default_rng(41)
    seen, seqs = set(), []
    while len(seqs) < 340:
        s = core.copy()
        for pos in rng.choice(12, size=int(rng.integers(1, 4)), replace=False):
            s[pos] = rng.integers(0, 20)
        if s.tobytes() not in seen:
            seen.add(s.tobytes())
            seqs.append(s)
    n = len(seqs)
    res, off = hammock_amd.pack_sequences(seqs)
    idx = np.arange(n, dtype=np.uint32)
    rc, T = coracle.score_block(blosum62, res, off, idx, idx, 0, 3, -1)
    assert rc == 0
    thr = int(T.min())
    assert 5 <= thr <= 80, thr
    monkeypatch.setenv("HMK_NO_ROWS_KERNEL", "1")
    ctx = hammock_amd.Context(blosum62, device=0)
    ctx.set_sequences(residues=res, offsets=off)
    edges, st = ctx.neighbors_shifted(3, -1, thr)
    print(f"swar: threshold {thr}, u8 {st.classes_u8} u16 {st.classes_u16} direct {st.classes_direct} rows {st.classes_rows}")
    assert (st.classes_u8, st.classes_u16, st.classes_direct, st.classes_rows) == (1, 0, 0, 0) and st.symmetric == 1
    check(edges, triangle_edges(T, thr), n * (n - 1) // 2, "swar")
