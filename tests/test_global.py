"""GlobalAlignmentScorer (hmk_score_pairs_global / hmk_score_block_global / hmk_neighbors_global / hmk_search_global,
Context.*_global, the CLI's --scorer global): Gotoh's global alignment score with an affine gap, end gaps charged.  The reference
has no counterpart, so the expectation is tests/global_ref.py: the recurrence in plain loops, a brute force over all alignments
and a numpy form per (la, lb) class, pinned against each other and against the known answers of the header's definition.  All
scores are integers and every comparison is exact.  The CPU tests run anywhere; the GPU tests need an MI355X (-m gpu)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import global_ref as G
import hammock_amd
from hammock_amd import _native as N

CLI = os.path.join(ROOT, "hammock_amd", "bin", "hammock-hip")
NEW_SYMBOLS = ("hmk_score_pairs_global", "hmk_score_block_global", "hmk_neighbors_global", "hmk_search_global")
PENALTIES = ((-5, -1), (-11, -1), (-1, -1), (0, 0))
# seq1, seq2, global under BLOSUM62 for each of PENALTIES
KNOWN = (("WVTAPRSLPVLP", "RSPIVRQLPSLP", (20, 16, 28, 35)),
         ("ACDEFGHIKL", "ACDFGHIKL", (47, 41, 51, 52)),
         ("ACDEFGHIKL", "ACDEFGHWWIKL", (51, 45, 55, 57)),
         ("A", "W", (-3, -3, -2, 0)),
         ("AAAAAAA", "W" * 20, (-35, -44, -27, 0)),
         ("HEAGAWGHEE", "PAWHEAE", (14, 2, 27, 33)))


def _blosum62():
    with open(os.path.join(GOLDEN, "matrices.json")) as fh:
        return np.asarray(json.load(fh)["matrices"]["blosum62"], dtype=np.int32)


def asymmetric(M):
    rng = np.random.default_rng(5)
    M = M.copy()
    M[np.triu_indices(24, 1)] += rng.integers(-2, 3, size=276).astype(np.int32)
    return M


def rand_seq(rng, L):
    return rng.integers(0, 20, size=L, dtype=np.uint8)


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


def mixed_set(seed, n12, per_len, lengths=(1, 2, 7, 16, 17, 20, 31, 32)):
    """n12 12-mers in families of five (a seed and variants with up to three substitutions), then per_len random sequences of
    every length of `lengths`, shuffled: the caller's order is not the length-sorted one"""
    rng = np.random.default_rng(seed)
    seqs = []
    while len(seqs) < n12:
        seed12 = rand_seq(rng, 12)
        for v in range(5):
            s = seed12.copy()
            for pos in rng.choice(12, size=min(v, 3), replace=False):
                s[pos] = rng.integers(0, 20)
            seqs.append(s)
    seqs = seqs[:n12]
    for L in lengths:
        seqs += [rand_seq(rng, L) for _ in range(per_len)]
    return [seqs[k] for k in rng.permutation(len(seqs))]


NEIGHBOUR_THRESHOLD = 8   # BLOSUM62, -5 / -1 on big_set: 3.1 % of the unordered pairs (test_threshold_share_of_the_neighbour_set)


@pytest.fixture(scope="module")
def big_set():
    """300 12-mers (a class that crosses a 256-column batch, 19 row chunks with a partial last one, triangle tiles on the
    diagonal) + 40 each of the lengths 1, 2, 7, 16, 17, 20, 31, 32; its reference table under BLOSUM62, -5 / -1"""
    seqs = mixed_set(1, 300, 40)
    return seqs, G.global_table(seqs, _blosum62(), -5, -1)


@pytest.fixture(scope="module")
def small_set():
    """200 sequences of the same make (all ordered pairs, literal tiles)"""
    return mixed_set(2, 80, 15)


def triangle_edges(T, thr):
    """the expected sorted edges of a symmetric pass: each unordered pair once, x < m"""
    i, j = np.nonzero(np.triu(T >= thr, 1))
    return np.sort(hammock_amd.pack_edges(i, j, T[i, j]))


def ordered_edges(T, thr, rows=None, cols=None):
    """... of all ordered pairs: T[r, c] = global(seq1 = rows[r], seq2 = cols[c]) -> edge (x = column, m = row), never r == c"""
    rows = np.arange(T.shape[0]) if rows is None else np.asarray(rows)
    cols = np.arange(T.shape[1]) if cols is None else np.asarray(cols)
    r, c = np.nonzero(T >= thr)
    keep = rows[r] != cols[c]
    r, c = r[keep], c[keep]
    return np.sort(hammock_amd.pack_edges(cols[c], rows[r], T[r, c]))


def ctx_with(M, seqs, device=0):
    ctx = hammock_amd.Context(M, device=device)
    res, off = hammock_amd.pack_sequences(seqs)
    ctx.set_sequences(residues=res, offsets=off)
    return ctx


# ---- CPU ----------------------------------------------------------------------------------------------------------------

def test_global_symbols_in_header_symbols_and_library():
    with open(os.path.join(ROOT, "include", "hammock_hip.h")) as fh:
        header = fh.read()
    for name in NEW_SYMBOLS:
        assert f"int {name}(" in header
        assert name in N.SYMBOLS
        assert hasattr(N.lib, name)
    assert N.lib.hmk_abi_version() == 4
    assert "#define HMK_ABI_VERSION 4" in header


def test_reference_layers_agree_and_give_the_known_answers():
    M = _blosum62()
    for s1, s2, want in KNOWN:
        a, b = hammock_amd.encode(s1), hammock_amd.encode(s2)
        for (go, ge), w in zip(PENALTIES, want):
            assert G.global_score(a, b, M, go, ge) == w, (s1, s2, go, ge)
            assert int(G.global_class([a], [b], M, go, ge)[0, 0]) == w
    rng = np.random.default_rng(3)
    for k in range(400):   # the recurrence is the maximum over all alignments (gap_open <= gap_extend <= 0)
        a, b = rand_seq(rng, rng.integers(1, 7)), rand_seq(rng, rng.integers(1, 7))
        ge = -int(rng.integers(0, 5))
        go = ge - int(rng.integers(0, 12))
        assert G.global_score(a, b, M, go, ge) == G.brute_force(a, b, M, go, ge), (a, b, go, ge)
    for la, lb, go, ge in ((1, 1, -5, -1), (3, 32, -11, -1), (12, 12, -5, -1), (17, 5, 0, 0), (32, 31, -127, -127)):
        A = np.array([rand_seq(rng, la) for _ in range(4)])
        B = np.array([rand_seq(rng, lb) for _ in range(5)])
        T = G.global_class(A, B, M, go, ge)
        for r in range(4):
            for c in range(5):
                assert T[r, c] == G.global_score(A[r], B[c], M, go, ge)
    seqs = [rand_seq(rng, L) for L in (1, 4, 4, 9, 1, 32, 9)]
    T = G.global_table(seqs, M, -5, -1, rows=[6, 0, 2], cols=[1, 5, 3, 4])
    for r, i in enumerate((6, 0, 2)):
        for c, j in enumerate((1, 5, 3, 4)):
            assert T[r, c] == G.global_score(seqs[i], seqs[j], M, -5, -1)


def test_edit_matrix_gives_minus_the_levenshtein_distance():
    rng = np.random.default_rng(4)
    E = G.edit_matrix()
    for k in range(300):
        a, b = rand_seq(rng, rng.integers(1, 13)), rand_seq(rng, rng.integers(1, 13))
        if k % 3 == 0:   # near pairs too: a copy with an edit or two
            b = np.delete(a, rng.integers(0, len(a))) if len(a) > 1 else a
            b = np.insert(b, rng.integers(0, len(b) + 1), rng.integers(0, 20))
        assert G.global_score(a, b, E, -1, -1) == -G.levenshtein(a, b)
    assert G.levenshtein(hammock_amd.encode("ACDEFGHIKL"), hammock_amd.encode("ACDFGHIKL")) == 1


def test_symmetric_under_a_symmetric_matrix_only():
    M = _blosum62()
    A = asymmetric(M)
    rng = np.random.default_rng(6)
    seqs = [rand_seq(rng, L) for L in rng.integers(1, 21, size=40)]
    T = G.global_table(seqs, M, -5, -1)
    assert np.array_equal(T, T.T)
    TA = G.global_table(seqs, A, -5, -1)
    assert not np.array_equal(TA, TA.T)


def test_threshold_share_of_the_neighbour_set(big_set):
    seqs, T = big_set
    n = len(seqs)
    assert n == 620
    hits = int(np.count_nonzero(np.triu(T >= NEIGHBOUR_THRESHOLD, 1)))
    assert 0.005 <= hits / (n * (n - 1) // 2) <= 0.05


def test_global_argument_errors_on_a_host_only_context():
    ctx = hammock_amd.Context(_blosum62(), device=-1)
    ctx.set_sequences(["ACDEFGHIK", "ACDEFGHIKL", "MNPQRSTVW", "WYVACDEFG"])
    i, j = np.array([0, 1], dtype=np.uint32), np.array([2, 3], dtype=np.uint32)
    out = np.zeros(4, dtype=np.int32)
    n_edges = C.c_uint64(0)
    # open > extend; a positive penalty; a penalty below -127
    for go, ge in ((-1, -5), (0, -1), (1, 1), (-5, 1), (3, 0), (-128, -1), (-128, -128), (-200, -1)):
        with pytest.raises(ValueError):
            ctx.score_pairs_global(i, j, go, ge)
        with pytest.raises(ValueError):
            ctx.score_block_global(0, 2, 2, 4, go, ge)
        with pytest.raises(ValueError):
            ctx.neighbors_global(go, ge, 10)
        with pytest.raises(ValueError):
            ctx.search_global(0, 2, 2, 4, go, ge, 10)
        assert N.lib.hmk_score_pairs_global(ctx._h, i.ctypes.data_as(C.POINTER(C.c_uint32)), j.ctypes.data_as(C.POINTER(C.c_uint32)),
                                            2, go, ge, out.ctypes.data_as(C.POINTER(C.c_int32))) == N.HMK_ERR_BAD_ARG
        assert N.lib.hmk_neighbors_global(ctx._h, go, ge, 10, 0, 1, None, 0, C.byref(n_edges), None) == N.HMK_ERR_BAD_ARG
    for thr in (-30001, 30001):
        with pytest.raises(ValueError):
            ctx.neighbors_global(-5, -1, thr)
        with pytest.raises(ValueError):
            ctx.search_global(0, 2, 2, 4, -5, -1, thr)
        assert N.lib.hmk_search_global(ctx._h, 0, 2, 2, 4, -5, -1, thr, None, 0, C.byref(n_edges), None) == N.HMK_ERR_BAD_ARG
    for q0, q1, r0, r1 in ((0, 2, 1, 3), (1, 3, 0, 2), (0, 4, 2, 3), (0, 2, 2, 5), (3, 2, 0, 1)):
        with pytest.raises(ValueError):
            ctx.search_global(q0, q1, r0, r1, -5, -1, 10)


def test_global_valid_arguments_reach_the_device_check():
    ctx = hammock_amd.Context(_blosum62(), device=-1)
    ctx.set_sequences(["ACDEFGHIK", "ACDEFGHIKL", "MNPQRSTVW", "WYVACDEFG"])
    for go, ge in ((-5, -1), (0, 0), (-127, -127), (-127, 0)):
        with pytest.raises(hammock_amd.DeviceError):
            ctx.score_pairs_global([0, 1], [2, 3], go, ge)
        with pytest.raises(hammock_amd.DeviceError):
            ctx.score_block_global(0, 2, 2, 4, go, ge)
        with pytest.raises(hammock_amd.DeviceError):
            ctx.neighbors_global(go, ge, -30000)
        with pytest.raises(hammock_amd.DeviceError):
            ctx.search_global(0, 2, 2, 4, go, ge, 30000)


# ---- GPU ----------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_pairs_known_answers(gpu):
    seqs = [s for s1, s2, _ in KNOWN for s in (s1, s2)]
    ctx = hammock_amd.Context(_blosum62(), device=0)
    ctx.set_sequences(seqs)
    i, j = np.arange(0, len(seqs), 2), np.arange(1, len(seqs), 2)
    for p, (go, ge) in enumerate(PENALTIES):
        want = [w[p] for _, _, w in KNOWN]
        assert ctx.score_pairs_global(i, j, go, ge).tolist() == want
        assert ctx.score_pairs_global(j, i, go, ge).tolist() == want   # BLOSUM62 is symmetric


@pytest.mark.gpu
def test_pairs_and_block_match_the_reference_in_both_orders(gpu):
    rng = np.random.default_rng(7)
    lengths = (1, 2, 3, 5, 7, 12, 16, 17, 20, 31, 32)
    seqs = [rand_seq(rng, lengths[k % len(lengths)]) for k in range(140)]
    M = asymmetric(_blosum62())
    ctx = ctx_with(M, seqs)
    for go, ge in ((-5, -1), (-127, -3)):
        T = G.global_table(seqs, M, go, ge)
        assert np.array_equal(ctx.score_block_global(0, 70, 70, 140, go, ge), T[:70, 70:])
        assert np.array_equal(ctx.score_block_global(70, 140, 0, 70, go, ge), T[70:, :70])
        i, j = rng.integers(0, 140, size=500), rng.integers(0, 140, size=500)
        assert np.array_equal(ctx.score_pairs_global(i, j, go, ge), T[i, j])
        assert np.array_equal(ctx.score_pairs_global(j, i, go, ge), T[j, i])


@pytest.mark.gpu
def test_neighbors_symmetric_edges_parts_and_all_pairs(gpu, big_set):
    seqs, T = big_set
    n = len(seqs)
    ctx = ctx_with(_blosum62(), seqs)
    want = triangle_edges(T, NEIGHBOUR_THRESHOLD)
    edges, st = ctx.neighbors_global(-5, -1, NEIGHBOUR_THRESHOLD)
    x, m, s = hammock_amd.edge_fields(edges)
    assert np.all(x < m)
    assert st.pairs_scored == n * (n - 1) // 2 and st.symmetric == 1
    assert np.array_equal(np.sort(edges), want)
    # parts 0, 1, 2 of 3: disjoint, their union the whole
    parts, pairs = [], 0
    for part in range(3):
        e, pst = ctx.neighbors_global(-5, -1, NEIGHBOUR_THRESHOLD, part=part, n_parts=3)
        parts.append(e)
        pairs += pst.pairs_scored
    assert pairs == n * (n - 1) // 2
    assert sum(len(e) for e in parts) == len(want) and all(len(e) for e in parts)
    assert np.array_equal(np.sort(np.concatenate(parts)), want)
    # every pair a hit: mid-tile stage flushes; a caller's buffer of 1024 is reported too small with the needed count
    buf = np.empty(1024, dtype=np.uint64)
    n_edges = C.c_uint64(0)
    rc = N.lib.hmk_neighbors_global(ctx._h, -5, -1, -30000, 0, 1, buf.ctypes.data_as(C.POINTER(C.c_uint64)), 1024, C.byref(n_edges), None)
    assert rc == N.HMK_ERR_CAPACITY and n_edges.value == n * (n - 1) // 2
    with pytest.raises(BufferError):
        ctx.neighbors_global(-5, -1, -30000, capacity=1024)
    everything, _ = ctx.neighbors_global(-5, -1, -30000, capacity=int(n_edges.value))
    assert len(everything) == n * (n - 1) // 2
    assert np.array_equal(np.sort(everything), triangle_edges(T, -30000))


@pytest.mark.gpu
def test_neighbors_asymmetric_all_ordered_pairs(gpu, small_set):
    seqs = small_set
    n = len(seqs)
    M = asymmetric(_blosum62())
    T = G.global_table(seqs, M, -5, -1)
    assert not np.array_equal(T, T.T)
    ctx = ctx_with(M, seqs)
    for thr in (-12, -30000):
        edges, st = ctx.neighbors_global(-5, -1, thr)
        assert st.pairs_scored == n * (n - 1) and st.symmetric == 0
        assert np.array_equal(np.sort(edges), ordered_edges(T, thr))   # score = global(seq1 = m, seq2 = x)
    assert len(edges) == n * (n - 1)


@pytest.mark.gpu
def test_neighbors_literal_tiles(gpu, small_set):
    seqs = small_set
    M = _blosum62()
    M40 = M * 40
    assert M40.max() == 440
    T = G.global_table(seqs, M40, -120, -40)
    thr = int(np.sort(T[np.triu_indices(len(seqs), 1)])[-600])
    ctx = ctx_with(M40, seqs)
    edges, st = ctx.neighbors_global(-120, -40, thr)
    assert np.array_equal(np.sort(edges), triangle_edges(T, thr))
    everything, _ = ctx.neighbors_global(-120, -40, -30000)
    reg, _ = ctx_with(M, seqs).neighbors_global(-3, -1, -30000)   # the register kernel at 1 / 40 of every figure
    x, m, s = hammock_amd.edge_fields(np.sort(reg))
    assert np.array_equal(np.sort(everything), hammock_amd.pack_edges(x, m, 40 * s))
    # the asymmetric plan and the search on literal tiles too
    A40 = asymmetric(M) * 40
    TA = G.global_table(seqs, A40, -120, -40)
    actx = ctx_with(A40, seqs)
    edges, _ = actx.neighbors_global(-120, -40, thr)
    assert np.array_equal(np.sort(edges), ordered_edges(TA, thr))
    edges, _ = actx.search_global(0, 30, 30, 200, -120, -40, thr)
    assert np.array_equal(np.sort(edges), ordered_edges(TA[:30, 30:], thr, np.arange(30), np.arange(30, 200)))


@pytest.mark.gpu
def test_neighbors_edit_distance_two(gpu):
    rng = np.random.default_rng(8)
    seqs = []
    while len(seqs) < 300:   # families: a seed, variants one and two edits away (substitution, or a deletion and an insertion)
        seed = rand_seq(rng, 12)
        seqs.append(seed)
        one = seed.copy()
        one[rng.integers(0, 12)] = rng.integers(0, 20)
        seqs.append(one)
        two = np.insert(np.delete(seed, rng.integers(0, 12)), rng.integers(0, 12), rng.integers(0, 20))
        seqs.append(two)
        seqs.append(rand_seq(rng, 12))
    seqs = seqs[:300]
    n = len(seqs)
    want = [(i, j, G.levenshtein(seqs[i], seqs[j])) for i in range(n) for j in range(i + 1, n)]
    want = [(i, j, -d) for i, j, d in want if d <= 2]
    assert len(want) >= 150
    ctx = ctx_with(G.edit_matrix(), seqs)
    edges, st = ctx.neighbors_global(-1, -1, -2)
    x, m, s = hammock_amd.edge_fields(np.sort(edges))
    assert list(zip(x.tolist(), m.tolist(), s.tolist())) == sorted(want)


@pytest.mark.gpu
def test_search_global(gpu):
    seqs = mixed_set(9, 100, 30)[:340]
    Q = 40
    for M in (_blosum62(), asymmetric(_blosum62())):
        T = G.global_table(seqs, M, -5, -1, rows=np.arange(Q), cols=np.arange(Q, 340))
        ctx = ctx_with(M, seqs)
        for thr in (-8, -30000):
            edges, st = ctx.search_global(0, Q, Q, 340, -5, -1, thr)
            x, m, s = hammock_amd.edge_fields(edges)
            assert np.all(m < Q) and np.all(x >= Q)   # m = query on every edge
            assert st.pairs_scored == Q * 300
            assert np.array_equal(np.sort(edges), ordered_edges(T, thr, np.arange(Q), np.arange(Q, 340)))
        assert len(edges) == Q * 300
        # references before queries; an empty range
        T2 = G.global_table(seqs, M, -5, -1, rows=np.arange(300, 340), cols=np.arange(0, 300))
        edges, _ = ctx.search_global(300, 340, 0, 300, -5, -1, -8)
        assert np.array_equal(np.sort(edges), ordered_edges(T2, -8, np.arange(300, 340), np.arange(0, 300)))
        edges, st = ctx.search_global(5, 5, Q, 340, -5, -1, -8)
        assert len(edges) == 0 and st.n_edges == 0


class TableScorer:
    """the scorer object the oracle's clusterers are driven by: global(seq1, seq2) of tests/global_ref.py, looked up in the
    table global_table made for these sequences"""
    def __init__(self, useqs, T):
        self.index = {id(u): k for k, u in enumerate(useqs)}
        self.T = T
        self.calls = 0

    def sequence_score(self, seq1, seq2):
        self.calls += 1
        return int(self.T[self.index[id(seq1)], self.index[id(seq2)]])


def composition_case():
    """300 distinct mixed-length sequences with families; threshold and cluster limit of the composition tests"""
    rng = np.random.default_rng(10)
    seqs, seen = [], set()
    while len(seqs) < 300:
        seed = rand_seq(rng, rng.integers(7, 21))
        for v in range(4):
            s = seed.copy()
            if v:
                s[rng.integers(0, len(s))] = rng.integers(0, 20)
            if v == 3 and len(s) > 7:
                s = np.delete(s, rng.integers(0, len(s)))
            if s.tobytes() not in seen:
                seen.add(s.tobytes())
                seqs.append(s)
    seqs = seqs[:300]
    return [seqs[k] for k in rng.permutation(300)], 18, 40


def oracle_greedy(seqs, T, thr, maxc):
    """(cluster id per sequence, result order, member rank) of the oracle's LimitedGreedySequenceClusterer under the table"""
    from oracle import hammock_oracle as ho
    alphabet = "ARNDCQEGHILKMFPSTWYVBZX*"
    useqs = [ho.UniqueSequence("".join(alphabet[c] for c in s)) for s in seqs]
    clusters = ho.LimitedGreedySequenceClusterer(TableScorer(useqs, T), thr, maxc, 1).cluster(useqs)
    index = {id(u): k for k, u in enumerate(useqs)}
    cid = np.full(len(seqs), -1, dtype=np.int64)
    rank = np.full(len(seqs), -1, dtype=np.int64)
    for c in clusters:
        for pos, u in enumerate(c.sequences):
            cid[index[id(u)]] = c.id
            rank[index[id(u)]] = pos
    return cid, [c.id for c in clusters], rank


@pytest.mark.gpu
def test_neighbors_global_composes_with_greedy_and_components(gpu):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    seqs, thr, maxc = composition_case()
    n = len(seqs)
    M = _blosum62()
    T = G.global_table(seqs, M, -5, -1)
    ctx = ctx_with(M, seqs)
    edges, _ = ctx.neighbors_global(-5, -1, thr)
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


# ---- CLI ----------------------------------------------------------------------------------------------------------------

def test_cli_scorer_argument_errors_need_no_device(tmp_path):
    fa = os.path.join(GOLDEN, "musi.fa")
    for mode in (["greedy"], ["search", "--database", fa]):
        for extra, word in ((["--scorer", "bogus"], "--scorer"), (["--scorer", "global", "-x", "3"], "-x"),
                            (["--scorer", "global", "-p", "0"], "-p"),
                            (["--scorer", "global", "--gap_open", "-1", "--gap_extend", "-5"], "--gap_open")):
            out = tmp_path / "out"
            r = subprocess.run([CLI] + mode + ["-i", fa, "-d", str(out)] + extra, capture_output=True, text=True)
            assert r.returncode == 2, (mode, extra, r.stderr)
            assert word in r.stderr
            assert not out.exists()
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert "--scorer" in r.stderr and "--gap_open" in r.stderr and "--gap_extend" in r.stderr


def musi_records(lo, hi):
    with open(os.path.join(GOLDEN, "musi.fa")) as fh:
        lines = fh.read().splitlines()
    return "\n".join(lines[2 * lo:2 * hi]) + "\n"


@pytest.mark.gpu
def test_cli_search_with_the_global_scorer(gpu, tmp_path):
    from oracle import hammock_oracle as ho
    qfa, rfa = tmp_path / "queries.fa", tmp_path / "references.fa"
    qfa.write_text(musi_records(0, 60))
    rfa.write_text(musi_records(60, 400))
    queries = ho.load_unique_sequences_from_fasta(str(qfa))
    refs = ho.load_unique_sequences_from_fasta(str(rfa))
    seqs = [u.sequence for u in queries + refs]
    nq = len(queries)
    T = G.global_table(seqs, _blosum62(), -4, -2, rows=np.arange(nq), cols=np.arange(nq, len(seqs)))
    thr = 12
    rows_all, rows_best = ["query\ttarget\tscore"], ["query\ttarget\tscore"]
    for q in range(nq):
        ok = np.nonzero(T[q] >= thr)[0]
        order = ok[np.lexsort((ok, -T[q, ok]))]   # score descending, then the reference's load order
        for t, r in enumerate(order):
            line = f"{queries[q].get_sequence_string()}\t{refs[r].get_sequence_string()}\t{T[q, r]}"
            rows_all.append(line)
            if t < 2:
                rows_best.append(line)
    assert len(rows_all) > len(rows_best) > 1 + nq // 4
    for extra, want, name in (([], rows_all, "all"), (["--best", "2"], rows_best, "best")):
        out = tmp_path / name
        r = subprocess.run([CLI, "search", "-i", str(qfa), "--database", str(rfa), "-d", str(out), "--scorer", "global", "--gap_open", "-4",
                            "--gap_extend", "-2", "-g", str(thr)] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert "Scorer: global" in r.stderr and "Max shift" not in r.stderr
        assert (out / "search_hits.tsv").read_text().splitlines() == want


@pytest.mark.gpu
def test_cli_greedy_with_the_global_scorer_writes_the_oracles_files(gpu, tmp_path):
    """the first 600 records of tests/golden/musi.fa (the reference table of all 2,457 is minutes of numpy): the three stage-1
    files equal the oracle's writers over the oracle's LimitedGreedySequenceClusterer driven by the Python reference, at the
    defaults of greedy mode (size order, threshold round(1.7 x mean length), limit round(0.025 n)) and -5 / -1"""
    from oracle import hammock_oracle as ho
    fa = tmp_path / "subset.fa"
    fa.write_text(musi_records(0, 600))
    loaded = ho.load_unique_sequences_from_fasta(str(fa))
    labels = ho.get_sorted_labels(loaded)
    seqs = list(loaded)
    sorted_seqs = ho.sort_sequences(seqs, "size", seed=42, labels=labels)
    seqs = seqs if sorted_seqs is None else sorted_seqs
    thr, _, maxc = ho.greedy_defaults(seqs)
    T = G.global_table([u.sequence for u in seqs], _blosum62(), -5, -1)
    clusters = ho.LimitedGreedySequenceClusterer(TableScorer(seqs, T), thr, maxc, 1).cluster(seqs)
    assert sum(1 for c in clusters if len(c.sequences) > 1) >= 5
    exp = tmp_path / "expected"
    exp.mkdir()
    ho.save_cluster_sequences_csv(clusters, str(exp / "initial_clusters_sequences.tsv"), labels)
    ho.write_cluster_sequences_csv(list(loaded), clusters, str(exp / "initial_clusters_sequences_original_order.tsv"), labels)
    ho.save_clusters_csv(clusters, str(exp / "initial_clusters.tsv"), labels)
    out = tmp_path / "out"
    r = subprocess.run([CLI, "greedy", "-i", str(fa), "-d", str(out), "--scorer", "global"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "Scorer: global (global alignment, affine gap). Gap open penalty: -5, gap extend penalty: -1" in r.stderr
    assert f"Setting automatically to: {thr}" in r.stderr and f"Setting automatically to: {maxc}" in r.stderr
    assert "\n--scorer global\n--gap_open -5\n--gap_extend -1\n" in (out / "run.log").read_text()   # the parameter block names them
    for name in ("initial_clusters_sequences.tsv", "initial_clusters_sequences_original_order.tsv", "initial_clusters.tsv"):
        assert (out / name).read_bytes() == (exp / name).read_bytes(), name
    # without the flag the log names no scorer
    plain = tmp_path / "plain"
    r = subprocess.run([CLI, "greedy", "-i", str(fa), "-d", str(plain)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "Scorer" not in r.stderr and "Scorer" not in (plain / "run.log").read_text()
