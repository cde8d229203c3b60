"""Query-vs-reference search (hmk_search_shifted / hmk_search_local / hmk_search_best_shifted, Context.search_*, the CLI's
`search` mode): queries [q0, q1) against references [r0, r1) of one uploaded set, score(q, r) = sequenceScore(seq1 = query,
seq2 = reference), every edge m = query.  Expectations come from oracle.c_oracle.score_block (rows = queries, columns =
references) and oracle/hammock_oracle.py.  The CPU tests run anywhere; the GPU tests need an MI355X (-m gpu)."""
import ctypes as C
import json
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import hammock_amd
from hammock_amd import _native as N
from hammock_amd.synth import synth_peptides

CLI = os.path.join(ROOT, "hammock_amd", "bin", "hammock-hip")
NEW_SYMBOLS = ("hmk_search_shifted", "hmk_search_local", "hmk_search_best_shifted")
ALPHABET = "ARNDCQEGHILKMFPSTWYVBZX*"


def _blosum62():
    with open(os.path.join(GOLDEN, "matrices.json")) as fh:
        return np.asarray(json.load(fh)["matrices"]["blosum62"], dtype=np.int32)


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


def split_seqs(res, off):
    return [np.asarray(res[off[k]:off[k + 1]], dtype=np.uint8) for k in range(len(off) - 1)]


def oracle_hits(coracle, M, res, off, q_idx, r_idx, scorer, a, b, thr):
    """(block [len(q_idx), len(r_idx)] of score(seq1 = q, seq2 = r), the expected sorted packed edges m = q, x = r)"""
    st, blk = coracle.score_block(M, res, off, q_idx, r_idx, scorer, a, b)
    assert st == 0
    qi, ri = np.nonzero(blk >= thr)
    want = hammock_amd.pack_edges(np.asarray(r_idx)[ri], np.asarray(q_idx)[qi], blk[qi, ri])
    return blk, np.sort(want)


def asymmetric(M):
    rng = np.random.default_rng(5)     # the matrix of test_gpu_parity.py::test_neighbors_asymmetric_matrix
    M = M.copy()
    M[np.triu_indices(24, 1)] += rng.integers(-2, 3, size=276).astype(np.int32)
    return M


# ---- CPU ----------------------------------------------------------------------------------------------------------------

def test_search_symbols_in_header_symbols_and_library():
    with open(os.path.join(ROOT, "include", "hammock_hip.h")) as fh:
        header = fh.read()
    for name in NEW_SYMBOLS:
        assert f"int {name}(" in header
        assert name in N.SYMBOLS
        assert hasattr(N.lib, name)
    assert N.lib.hmk_abi_version() == 4


def test_search_argument_errors_on_a_host_only_context():
    ctx = hammock_amd.Context(_blosum62(), device=-1)
    ctx.set_sequences(["ACDEFGHIK", "ACDEFGHIKL", "MNPQRSTVW", "WYVACDEFG"])
    for q0, q1, r0, r1 in ((0, 2, 1, 3), (1, 3, 0, 2), (0, 4, 2, 3), (0, 2, 2, 5), (3, 2, 0, 1), (0, 1, 4, 3)):
        with pytest.raises(ValueError):
            ctx.search_shifted(q0, q1, r0, r1, 2, 0, 10)
        with pytest.raises(ValueError):
            ctx.search_local(q0, q1, r0, r1, -5, -1, 10)
        with pytest.raises(ValueError):
            ctx.search_best_shifted(q0, q1, r0, r1, 2, 0, 10, 3)
    for k in (0, 33):
        with pytest.raises(ValueError):
            ctx.search_best_shifted(0, 2, 2, 4, 2, 0, 10, k)
    # the raw status of a bad range is HMK_ERR_BAD_ARG
    n_edges = C.c_uint64(0)
    st = N.lib.hmk_search_shifted(ctx._h, 0, 3, 2, 4, 2, 0, 10, None, 0, C.byref(n_edges), None)
    assert st == N.HMK_ERR_BAD_ARG
    # valid arguments reach the device check: no CPU fallback
    with pytest.raises(hammock_amd.DeviceError):
        ctx.search_shifted(0, 2, 2, 4, 2, 0, 10)
    with pytest.raises(hammock_amd.DeviceError):
        ctx.search_local(2, 4, 0, 2, -5, -1, 10)
    with pytest.raises(hammock_amd.DeviceError):
        ctx.search_best_shifted(0, 2, 2, 4, 2, 0, 10, 32)


def test_cli_search_needs_database(tmp_path):
    r = subprocess.run([CLI, "search", "-i", os.path.join(GOLDEN, "musi.fa"), "-d", str(tmp_path / "out")],
                       capture_output=True, text=True)
    assert r.returncode == 2
    assert "--database" in r.stderr
    assert not (tmp_path / "out").exists()


def test_cli_search_rejects_devices(tmp_path):
    fa = os.path.join(GOLDEN, "musi.fa")
    r = subprocess.run([CLI, "search", "-i", fa, "--database", fa, "-d", str(tmp_path / "out"), "--devices", "0,1"],
                       capture_output=True, text=True)
    assert r.returncode == 2


def test_cli_help_names_search():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    assert "search" in r.stderr and "--database" in r.stderr and "--best" in r.stderr


# ---- GPU ----------------------------------------------------------------------------------------------------------------

def ctx_with(M, seqs):
    ctx = hammock_amd.Context(M, device=0)
    res, off = hammock_amd.pack_sequences(seqs)
    ctx.set_sequences(residues=res, offsets=off)
    return ctx, res, off


@pytest.mark.gpu
def test_search_uniform_12mers_both_orders(gpu, coracle):
    M = _blosum62()
    Q, R, X, P, THR = 2000, 20000, 3, 0, 20
    res, off = synth_peptides(11, Q + R, 12)
    seqs = split_seqs(res, off)
    ctx, res, off = ctx_with(M, seqs)
    blk, want = oracle_hits(coracle, M, res, off, np.arange(Q), np.arange(Q, Q + R), 0, X, P, THR)
    edges, st = ctx.search_shifted(0, Q, Q, Q + R, X, P, THR)
    x, m, s = hammock_amd.edge_fields(edges)
    assert np.all(m < Q) and np.all(x >= Q)
    assert st.pairs_scored == Q * R
    assert st.classes_rows >= 1
    assert np.array_equal(np.sort(edges), want)
    # the references first: queries are [R, R + Q)
    ctx2, res2, off2 = ctx_with(M, seqs[Q:] + seqs[:Q])
    edges2, st2 = ctx2.search_shifted(R, R + Q, 0, R, X, P, THR)
    qi, ri = np.nonzero(blk >= THR)
    want2 = np.sort(hammock_amd.pack_edges(ri, R + qi, blk[qi, ri]))
    assert st2.pairs_scored == Q * R and st2.classes_rows >= 1
    assert np.array_equal(np.sort(edges2), want2)


@pytest.mark.gpu
@pytest.mark.parametrize("X", [2, 3])
def test_search_mixed_lengths(gpu, coracle, X):
    M = _blosum62()
    rng = np.random.default_rng(40 + X)
    from conftest import random_peptides
    seqs = random_peptides(rng, 3600, 7, 20)
    Q = 600
    lq = np.array([len(s) for s in seqs[:Q]])
    lr = np.array([len(s) for s in seqs[Q:]])
    assert lq.max() > lr.min() and lq.min() < lr.max()   # classes with the queries longer and with them shorter
    ctx, res, off = ctx_with(M, seqs)
    _, want = oracle_hits(coracle, M, res, off, np.arange(Q), np.arange(Q, len(seqs)), 0, X, -1, 14)
    edges, st = ctx.search_shifted(0, Q, Q, len(seqs), X, -1, 14)
    assert st.pairs_scored == Q * (len(seqs) - Q)
    assert np.array_equal(np.sort(edges), want)
    # queries behind the references
    edges, st = ctx.search_shifted(Q, len(seqs), 0, Q, X, -1, 14)
    _, want = oracle_hits(coracle, M, res, off, np.arange(Q, len(seqs)), np.arange(Q), 0, X, -1, 14)
    assert np.array_equal(np.sort(edges), want)


@pytest.mark.gpu
def test_search_asymmetric_matrix(gpu, coracle):
    M = asymmetric(_blosum62())
    res, off = synth_peptides(3, 2000, 10, 13)
    seqs = split_seqs(res, off)
    ctx, res, off = ctx_with(M, seqs)
    for (q0, q1, r0, r1) in ((0, 500, 500, 2000), (1500, 2000, 0, 1500), (0, 1500, 1500, 2000)):
        edges, st = ctx.search_shifted(q0, q1, r0, r1, 3, -1, 18)
        assert st.symmetric == 0
        _, want = oracle_hits(coracle, M, res, off, np.arange(q0, q1), np.arange(r0, r1), 0, 3, -1, 18)
        assert np.array_equal(np.sort(edges), want)


@pytest.mark.gpu
@pytest.mark.parametrize("Q,R", [(5, 50000), (50000, 5)])
def test_search_skewed_shapes(gpu, coracle, Q, R):
    M = _blosum62()
    res, off = synth_peptides(21, Q + R, 12)
    ctx = hammock_amd.Context(M, device=0)
    ctx.set_sequences(residues=res, offsets=off)
    _, want = oracle_hits(coracle, M, res, off, np.arange(Q), np.arange(Q, Q + R), 0, 3, 0, 20)
    edges, st = ctx.search_shifted(0, Q, Q, Q + R, 3, 0, 20)
    assert st.pairs_scored == Q * R
    assert np.array_equal(np.sort(edges), want)


@pytest.mark.gpu
def test_search_threshold_and_capacity_edges(gpu, coracle):
    M = _blosum62()
    res, off = synth_peptides(8, 500, 8, 16)
    ctx = hammock_amd.Context(M, device=0)
    ctx.set_sequences(residues=res, offsets=off)
    Q, R = 200, 300
    edges, st = ctx.search_shifted(0, Q, Q, Q + R, 3, -1, -30000)
    assert len(edges) == Q * R
    _, want = oracle_hits(coracle, M, res, off, np.arange(Q), np.arange(Q, Q + R), 0, 3, -1, -30000)
    assert np.array_equal(np.sort(edges), want)
    edges, _ = ctx.search_shifted(0, Q, Q, Q + R, 3, -1, 30000)
    assert len(edges) == 0
    _, want = oracle_hits(coracle, M, res, off, np.arange(Q), np.arange(Q, Q + R), 0, 3, -1, 15)
    need = len(want)
    assert need > 10
    buf = np.empty(need, dtype=np.uint64)
    n_edges = C.c_uint64(0)
    stats = N.NeighborStats()
    st = N.lib.hmk_search_shifted(ctx._h, 0, Q, Q, Q + R, 3, -1, 15, buf.ctypes.data_as(C.POINTER(C.c_uint64)), need - 1,
                                  C.byref(n_edges), C.byref(stats))
    assert st == N.HMK_ERR_CAPACITY and n_edges.value == need
    with pytest.raises(BufferError):
        ctx.search_shifted(0, Q, Q, Q + R, 3, -1, 15, capacity=need - 1)
    st = N.lib.hmk_search_shifted(ctx._h, 0, Q, Q, Q + R, 3, -1, 15, buf.ctypes.data_as(C.POINTER(C.c_uint64)), need,
                                  C.byref(n_edges), C.byref(stats))
    assert st == 0 and n_edges.value == need
    assert np.array_equal(np.sort(buf), want)
    # an empty range: no edges
    edges, st = ctx.search_shifted(0, 0, Q, Q + R, 3, -1, 15)
    assert len(edges) == 0 and st.pairs_scored == 0


@pytest.mark.gpu
def test_search_shift_check_is_over_the_two_ranges(gpu):
    M = _blosum62()
    res, off = synth_peptides(9, 300, 10, 14)
    seqs = split_seqs(res, off)
    seqs[250] = np.array([1, 2, 3], dtype=np.uint8)   # a 3-mer: max shift 3 is too big for it
    ctx, res, off = ctx_with(M, seqs)
    with pytest.raises(hammock_amd.DataException):
        ctx.search_shifted(200, 300, 0, 100, 3, 0, 20)      # in the query range
    with pytest.raises(hammock_amd.DataException):
        ctx.search_shifted(0, 100, 200, 300, 3, 0, 20)      # in the reference range
    with pytest.raises(hammock_amd.DataException):
        ctx.search_best_shifted(0, 100, 200, 300, 3, 0, 20, 4)
    edges, st = ctx.search_shifted(0, 100, 100, 200, 3, 0, 20)   # elsewhere in the set: fine
    assert st.pairs_scored == 100 * 100


@pytest.mark.gpu
@pytest.mark.parametrize("gaps,thr", [((-5, -1), 15), ((1, 1), 30)], ids=["striped", "literal"])
def test_search_local(gpu, coracle, gaps, thr):
    M = _blosum62()
    rng = np.random.default_rng(77)
    from conftest import random_peptides
    seqs = random_peptides(rng, 1100, 7, 20)
    ctx, res, off = ctx_with(M, seqs)
    Q = 300
    for (q0, q1, r0, r1) in ((0, Q, Q, 1100), (Q, 1100, 0, Q)):
        edges, st = ctx.search_local(q0, q1, r0, r1, gaps[0], gaps[1], thr)
        assert st.pairs_scored == (q1 - q0) * (r1 - r0)
        _, want = oracle_hits(coracle, M, res, off, np.arange(q0, q1), np.arange(r0, r1), 1, gaps[0], gaps[1], thr)
        assert len(want) > 0
        assert np.array_equal(np.sort(edges), want)


def numpy_best(blk, r_idx, thr, k):
    """per query: the k best (score desc, reference index asc) among score >= thr, padded with -1 / INT32_MIN"""
    nq = blk.shape[0]
    idx = np.full((nq, k), -1, dtype=np.int64)
    sc = np.full((nq, k), np.iinfo(np.int32).min, dtype=np.int32)
    r_idx = np.asarray(r_idx, dtype=np.int64)
    for q in range(nq):
        ok = np.nonzero(blk[q] >= thr)[0]
        order = np.lexsort((r_idx[ok], -blk[q, ok].astype(np.int64)))[:k]
        idx[q, :len(order)] = r_idx[ok][order]
        sc[q, :len(order)] = blk[q, ok][order]
    return idx, sc


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 5, 32])
def test_search_best_k(gpu, coracle, k):
    M = _blosum62()
    res, off = synth_peptides(31, 2300, 12)
    seqs = split_seqs(res, off)
    seqs = seqs + seqs[300:500]          # duplicate references: tied scores, the lower index first
    ctx, res, off = ctx_with(M, seqs)
    Q, n = 300, len(seqs)
    blk, _ = oracle_hits(coracle, M, res, off, np.arange(Q), np.arange(Q, n), 0, 3, 0, 20)
    idx, sc = ctx.search_best_shifted(0, Q, Q, n, 3, 0, 20, k)
    widx, wsc = numpy_best(blk, np.arange(Q, n), 20, k)
    assert np.array_equal(idx, widx) and np.array_equal(sc, wsc)
    assert (widx[:, -1] == -1).any()       # some queries have fewer than k hits
    # queries behind the references
    idx, sc = ctx.search_best_shifted(n - Q, n, 0, n - Q, 3, 0, 20, k)
    blk, _ = oracle_hits(coracle, M, res, off, np.arange(n - Q, n), np.arange(0, n - Q), 0, 3, 0, 20)
    widx, wsc = numpy_best(blk, np.arange(0, n - Q), 20, k)
    assert np.array_equal(idx, widx) and np.array_equal(sc, wsc)


@pytest.mark.gpu
def test_search_best_k_long_runs(gpu, coracle):
    """every query has more than 4,096 hits: the workgroup-per-query selection"""
    M = _blosum62()
    res, off = synth_peptides(32, 6050, 12)
    ctx = hammock_amd.Context(M, device=0)
    ctx.set_sequences(residues=res, offsets=off)
    Q, n = 50, 6050
    blk, _ = oracle_hits(coracle, M, res, off, np.arange(Q), np.arange(Q, n), 0, 3, 0, -1000)
    for k in (1, 32):
        idx, sc = ctx.search_best_shifted(0, Q, Q, n, 3, 0, -1000, k)
        widx, wsc = numpy_best(blk, np.arange(Q, n), -1000, k)
        assert np.array_equal(idx, widx) and np.array_equal(sc, wsc)
    assert ctx.last_search_stats.n_edges == Q * (n - Q)


@pytest.mark.gpu
def test_search_equals_the_cross_part_of_all_vs_all(gpu):
    M = _blosum62()
    n, Q = 100000, 10000
    res, off = synth_peptides(1, n, 12)
    ctx = hammock_amd.Context(M, device=0)
    ctx.set_sequences(residues=res, offsets=off)
    whole, _ = ctx.neighbors_shifted(3, 0, 20)
    x, m, s = hammock_amd.edge_fields(whole)    # x < m
    cross = (x < Q) & (m >= Q)
    want = np.sort(hammock_amd.pack_edges(m[cross], x[cross], s[cross]))
    first, st = ctx.search_shifted(0, Q, Q, n, 3, 0, 20)
    assert st.pairs_scored == Q * (n - Q)
    second, _ = ctx.search_shifted(0, Q, Q, n, 3, 0, 20)
    assert np.array_equal(np.sort(first), want)
    assert np.array_equal(np.sort(second), want)


@pytest.mark.gpu
def test_search_interleaved_with_clustering(gpu):
    M = _blosum62()
    res, off = synth_peptides(5, 20000, 12)
    ctx = hammock_amd.Context(M, device=0)
    ctx.set_sequences(residues=res, offsets=off)
    a = ctx.greedy_cluster(3, 0, 20, 500)
    s1, _ = ctx.search_shifted(0, 2000, 2000, 20000, 3, 0, 20)
    b = ctx.greedy_cluster(3, 0, 20, 500)
    s2, _ = ctx.search_shifted(0, 2000, 2000, 20000, 3, 0, 20)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(np.sort(s1), np.sort(s2))


def _java_round(v):
    return int(math.floor(v + 0.5))


@pytest.mark.gpu
def test_cli_search_matches_the_oracle(gpu, coracle, tmp_path):
    from oracle import hammock_oracle as ho
    with open(os.path.join(GOLDEN, "musi.fa")) as fh:
        lines = fh.read().splitlines()
    records = [lines[k:k + 2] for k in range(0, len(lines), 2)]
    half = len(records) // 2
    qfa, rfa = tmp_path / "queries.fa", tmp_path / "references.fa"
    qfa.write_text("\n".join(l for r in records[:half] for l in r) + "\n")
    rfa.write_text("\n".join(l for r in records[half:] for l in r) + "\n")
    queries = ho.load_unique_sequences_from_fasta(str(qfa))
    refs = ho.load_unique_sequences_from_fasta(str(rfa))
    union = queries + refs
    lens = [len(u.sequence) for u in union]
    X = min(_java_round(sum(lens) / len(lens) / 4), min(lens) - 1)
    thr = _java_round(sum(len(u.sequence) for u in queries) / len(queries) * 1.7)
    M = _blosum62()
    res, off = hammock_amd.pack_sequences([np.asarray(u.sequence, dtype=np.uint8) for u in union])
    nq = len(queries)
    st, blk = coracle.score_block(M, res, off, np.arange(nq), np.arange(nq, len(union)), 0, X, 0)
    assert st == 0
    scorer = ho.ShiftedScorer(M.tolist(), 0, X)
    text = lambda u: "".join(ALPHABET[c] for c in u.sequence)  # noqa: E731
    rows_all, rows_best = ["query\ttarget\tscore\tshift"], ["query\ttarget\tscore\tshift"]
    for q in range(nq):
        ok = np.nonzero(blk[q] >= thr)[0]
        order = ok[np.lexsort((ok, -blk[q, ok].astype(np.int64)))]
        for t, r in enumerate(order):
            score, shift = scorer.score_with_shift(queries[q], refs[r])
            assert score == blk[q, r]
            line = f"{text(queries[q])}\t{text(refs[r])}\t{score}\t{shift}"
            rows_all.append(line)
            if t < 3:
                rows_best.append(line)
    assert len(rows_all) > 1 + nq // 20
    for extra, want, name in (([], rows_all, "all"), (["--best", "3"], rows_best, "best")):
        out = tmp_path / name
        r = subprocess.run([CLI, "search", "-i", str(qfa), "--database", str(rfa), "-d", str(out)] + extra,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert "Max shift not set. Setting automatically to: " + str(X) in r.stderr
        assert "not set. Setting automatically to: " + str(thr) in r.stderr
        assert (out / "search_hits.tsv").read_text().splitlines() == want
