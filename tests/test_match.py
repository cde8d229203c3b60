"""Match of query clusters to existing clusters (hmk_match_clusters_shifted / hmk_match_clusters_local, Context.match_clusters_*,
the CLI's `match` mode): query sequences [q0, q1) in query slots against the frozen clusters of the members [r0, r1) of one uploaded
set.  Existing cluster a is feasible for query cluster b iff every pair (m in a, x in b) has score(seq1 = m, seq2 = x) >= threshold
(ClinkageClusterScorer.clusterScore(a, b), the orientation of ClinkageSequenceClusterer.java:263); its score is the minimum over
those pairs.  Expectations come from oracle.c_oracle.score_block and numpy -- test_assign.py's expectation with the minimum taken
over both sides' members -- cross-checked on small cases against the Python oracle's ClinkageClusterScorer.cluster_score +
find_nearest_cluster_parallel.  The CPU tests run anywhere; the GPU tests need an MI355X (-m gpu)."""
import ctypes as C
import gzip
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import hammock_amd
from hammock_amd import _native as N
from hammock_amd.synth import synth_peptides
from test_assign import INT_MIN, NONE, _blosum62, _cluster_file_expectation, asymmetric, gpu, mutate, relabel  # noqa: F401

CLI = os.path.join(ROOT, "hammock_amd", "bin", "hammock-hip")
NEW_SYMBOLS = ("hmk_match_clusters_shifted", "hmk_match_clusters_local")
ALPHABET = "ARNDCQEGHILKMFPSTWYVBZX*"


# ---- the expectation -----------------------------------------------------------------------------------------------------

def expected(blk, member_cluster, cluster_id, member_sizes, query_cluster, thr, k):
    """blk[m, x] = score(seq1 = member m, seq2 = query x) -> (best_cluster uint32[nb, k], best_score int32[nb, k], n_feasible[nb]):
    cluster a feasible for query cluster b iff every (m in a, x in b) scores >= thr, its score the minimum; ranked by score desc,
    size desc, id asc"""
    blk = np.asarray(blk, dtype=np.int64)
    nm, nq = blk.shape
    nc = len(cluster_id)
    qc = np.asarray(query_cluster, dtype=np.int64)
    nb = int(qc.max()) + 1 if nq else 0
    mc = np.asarray(member_cluster, dtype=np.int64)
    ids = np.asarray(cluster_id, dtype=np.int64)
    size = np.bincount(mc, weights=np.asarray(member_sizes, dtype=np.float64), minlength=nc).astype(np.int64)
    best = np.full((nb, k), NONE, dtype=np.uint32)
    score = np.full((nb, k), INT_MIN, dtype=np.int32)
    if nc == 0 or nb == 0:
        return best, score, np.zeros(nb, dtype=np.uint32)
    order = np.argsort(mc, kind="stable")
    mn = np.minimum.reduceat(blk[order], np.searchsorted(mc[order], np.arange(nc)), axis=0)        # [nc, nq]
    qorder = np.argsort(qc, kind="stable")
    mn = np.minimum.reduceat(mn[:, qorder], np.searchsorted(qc[qorder], np.arange(nb)), axis=1)    # [nc, nb]
    feas = mn >= thr
    rank = np.empty(nc, dtype=np.int64)
    rank[np.lexsort((ids, -size))] = np.arange(nc)                   # size desc, id asc
    key = np.where(feas, mn * (nc + 1) + (nc - rank)[:, None], -2 ** 62)   # larger = better
    top = np.argsort(-key, axis=0, kind="stable")[:k]               # [k', nb]
    for t in range(top.shape[0]):
        c = top[t]
        ok = feas[c, np.arange(nb)]
        best[ok, t] = c[ok]
        score[ok, t] = mn[c[ok], np.arange(nb)[ok]]
    return best, score, feas.sum(axis=0).astype(np.uint32)


def check(got, want):
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(got[2], want[2])


# ---- fixtures of sequences -------------------------------------------------------------------------------------------------

def two_sides(rng, n_members, n_queries, len_lo, len_hi, max_cluster=6, max_query=4, trim=False):
    """existing clusters and query clusters around shared random centres (1..max_cluster / 1..max_query members, mutants of the
    centre), plus random query clusters -> (members, member_cluster, queries, query_cluster)"""
    members, mc, queries, qc, centres = [], [], [], [], []
    while len(members) < n_members:
        L = int(rng.integers(len_lo, len_hi + 1))
        centre = rng.integers(0, 20, size=L).astype(np.uint8)
        centres.append(centre)
        for _ in range(int(rng.integers(1, 4))):
            c = int(mc[-1]) + 1 if mc else 0
            for _ in range(int(rng.integers(1, max_cluster + 1))):
                members.append(mutate(rng, centre, int(rng.integers(0, 3)), trim))
                mc.append(c)
    while len(queries) < n_queries:
        b = int(qc[-1]) + 1 if qc else 0
        centre = centres[int(rng.integers(len(centres)))] if rng.random() < 0.8 else \
            rng.integers(0, 20, size=int(rng.integers(len_lo, len_hi + 1))).astype(np.uint8)
        for _ in range(int(rng.integers(1, max_query + 1))):
            queries.append(mutate(rng, centre, int(rng.integers(0, 2)), trim))
            qc.append(b)
    return members[:n_members], np.asarray(mc[:n_members], dtype=np.int64), queries[:n_queries], relabel(np.asarray(qc[:n_queries]))


def setup(M, queries, members, member_cluster, rng, queries_first=True):
    """one uploaded set: queries + members (or members + queries) with random member sizes; -> ctx, res, off, q-range, r-range,
    ids, member sizes"""
    nq, nm = len(queries), len(members)
    msizes = rng.integers(1, 6, size=nm).astype(np.int32)
    if queries_first:
        seqs, sizes, qr, rr = queries + members, np.concatenate([np.ones(nq, np.int32), msizes]), (0, nq), (nq, nq + nm)
    else:
        seqs, sizes, qr, rr = members + queries, np.concatenate([msizes, np.ones(nq, np.int32)]), (nm, nm + nq), (0, nm)
    res, off = hammock_amd.pack_sequences(seqs)
    ctx = hammock_amd.Context(M, device=0)
    ctx.set_sequences(residues=res, offsets=off, sizes=sizes)
    nc = int(member_cluster.max()) + 1 if nm else 0
    ids = rng.permutation(np.arange(nc) * 7 + 100).astype(np.int32)
    return ctx, res, off, qr, rr, ids, msizes


def block(coracle, M, res, off, qr, rr, scorer, a, b):
    st, blk = coracle.score_block(M, res, off, np.arange(*rr), np.arange(*qr), scorer, a, b)
    assert st == 0
    return blk


def synth_seqs(seed, n):
    res, off = synth_peptides(seed, n, 12)
    return [np.asarray(res[off[i]:off[i + 1]]) for i in range(n)]


# ---- CPU ---------------------------------------------------------------------------------------------------------------------

def test_match_symbols_in_header_symbols_and_library():
    with open(os.path.join(ROOT, "include", "hammock_hip.h")) as fh:
        header = fh.read()
    for name in NEW_SYMBOLS:
        assert f"int {name}(" in header
        assert name in N.SYMBOLS
        assert hasattr(N.lib, name)
    assert N.lib.hmk_abi_version() == 4


def _raw(ctx, q0, q1, qc, nb, r0, r1, mc, cid, k=2, fn=None):
    qc = None if qc is None else np.asarray(qc, dtype=np.uint32)
    mc = np.asarray(mc, dtype=np.uint32)
    cid = np.asarray(cid, dtype=np.int32)
    out = np.empty(64, dtype=np.uint32)
    sc = np.empty(64, dtype=np.int32)
    p32 = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint32))  # noqa: E731
    fn = fn or N.lib.hmk_match_clusters_shifted
    return fn(ctx._h, q0, q1, p32(qc), nb, r0, r1, p32(mc), cid.ctypes.data_as(C.POINTER(C.c_int32)), len(cid), 2, 0, 10, k, p32(out),
              sc.ctypes.data_as(C.POINTER(C.c_int32)), p32(out), None)


def test_match_argument_errors_on_a_host_only_context():
    ctx = hammock_amd.Context(_blosum62(), device=-1)
    ctx.set_sequences(["ACDEFGHIK", "ACDEFGHIKL", "MNPQRSTVW", "WYVACDEFG", "KLMNPQRST"])
    for fn, a, b in ((ctx.match_clusters_shifted, 2, 0), (ctx.match_clusters_local, -5, -1)):
        for q0, q1, r0, r1 in ((0, 2, 1, 4), (2, 5, 0, 3), (0, 2, 3, 6), (3, 2, 0, 1)):
            with pytest.raises(ValueError):
                fn(q0, q1, [0] * max(q1 - q0, 0), r0, r1, [0] * max(r1 - r0, 0), [1], a, b, 10)
        for k in (0, 33):
            with pytest.raises(ValueError):
                fn(0, 2, [0, 0], 2, 5, [0, 1, 1], [5, 9], a, b, 10, k)
        with pytest.raises(ValueError):          # a member_cluster value >= n_clusters
            fn(0, 2, [0, 0], 2, 5, [0, 2, 1], [5, 9], a, b, 10)
        with pytest.raises(ValueError):          # slot 1 has no member
            fn(0, 2, [0, 0], 2, 5, [0, 0, 2], [5, 9, 4], a, b, 10)
        with pytest.raises(ValueError):          # duplicate ids
            fn(0, 2, [0, 0], 2, 5, [0, 1, 2], [5, 9, 5], a, b, 10)
        with pytest.raises(ValueError):          # query slot 1 has no member (n_query_clusters = 3)
            fn(0, 2, [0, 2], 2, 5, [0, 1, 1], [5, 9], a, b, 10)
        with pytest.raises(ValueError):          # query_cluster of the wrong length
            fn(0, 2, [0], 2, 5, [0, 1, 1], [5, 9], a, b, 10)
        with pytest.raises(ValueError):          # negative query slot
            fn(0, 2, [0, -1], 2, 5, [0, 1, 1], [5, 9], a, b, 10)
    # the raw status is HMK_ERR_BAD_ARG, also for what the Python layer cannot pass
    for fn in (N.lib.hmk_match_clusters_shifted, N.lib.hmk_match_clusters_local):
        assert _raw(ctx, 0, 2, [0, 0], 1, 2, 5, [0, 1, 1], [5, 5], fn=fn) == N.HMK_ERR_BAD_ARG       # duplicate ids
        assert _raw(ctx, 0, 2, None, 1, 2, 5, [0, 1, 1], [5, 9], fn=fn) == N.HMK_ERR_BAD_ARG         # null query_cluster
        assert _raw(ctx, 0, 2, [0, 1], 1, 2, 5, [0, 1, 1], [5, 9], fn=fn) == N.HMK_ERR_BAD_ARG       # a value >= n_query_clusters
        assert _raw(ctx, 0, 2, [0, 0], 2, 2, 5, [0, 1, 1], [5, 9], fn=fn) == N.HMK_ERR_BAD_ARG       # slot 1 without a member
        assert _raw(ctx, 0, 2, [0, 0], 1, 2, 5, [0, 1, 1], [5, 9], k=0, fn=fn) == N.HMK_ERR_BAD_ARG  # k
        assert _raw(ctx, 0, 2, [0, 0], 1, 1, 4, [0, 1, 1], [5, 9], fn=fn) == N.HMK_ERR_BAD_ARG       # overlap
    # valid arguments reach the device check: no CPU fallback
    with pytest.raises(hammock_amd.DeviceError):
        ctx.match_clusters_shifted(0, 2, [0, 0], 2, 5, [0, 1, 1], [5, 9], 2, 0, 10)
    with pytest.raises(hammock_amd.DeviceError):
        ctx.match_clusters_local(3, 5, [1, 0], 0, 3, [1, 0, 1], [5, 9], -5, -1, 10, k=32)


def test_match_expectation_agrees_with_the_python_oracle():
    """the numpy expectation's rank 1 is findNearestClusterParallel(existing clusters, query cluster) with ClinkageClusterScorer,
    on small random inputs whose query clusters have several members"""
    from oracle import hammock_oracle as ho
    M = _blosum62()
    Mlist = [list(map(int, r)) for r in M]
    rng = np.random.default_rng(31)
    for trial in range(4):
        members, mc, queries, qc = two_sides(rng, 60, 40, 9, 12, max_query=4, trim=True)
        mc = relabel(mc)
        text = lambda s: "".join(ALPHABET[c] for c in s)  # noqa: E731
        mseq = [ho.UniqueSequence(text(s), {"l": int(rng.integers(1, 4))}) for s in members]
        qseq = [ho.UniqueSequence(text(s)) for s in queries]
        X, thr = 3, 28
        scorer = ho.ShiftedScorer(Mlist, 0, X)
        blk = np.array([[scorer.sequence_score(m, x) for x in qseq] for m in mseq], dtype=np.int32)
        nc, nb = int(mc.max()) + 1, int(qc.max()) + 1
        ids = rng.permutation(np.arange(nc) * 3 + 10)
        sizes = [m.size() for m in mseq]
        want = expected(blk, mc, ids, sizes, qc, thr, 3)
        clusters = [ho.Cluster([mseq[i] for i in np.nonzero(mc == c)[0]], int(ids[c])) for c in range(nc)]
        slot = {id(cl): c for c, cl in enumerate(clusters)}
        clink = ho.ClinkageClusterScorer(scorer, thr)
        assert (want[2] > 0).any() and (want[2] == 0).any() and (np.bincount(qc) > 1).any()
        for b in range(nb):
            compared = ho.Cluster([qseq[i] for i in np.nonzero(qc == b)[0]], -1 - b)
            for a in range(nc):
                s = clink.cluster_score(clusters[a], compared)
                mn = int(blk[mc == a][:, qc == b].min())
                assert s == (mn if mn >= thr else INT_MIN + 1)
            got = ho.find_nearest_cluster_parallel(clusters, compared, clink, sum(c.get_unique_size() for c in clusters))
            if got is None or got.cluster is None or got.score < thr:
                assert want[2][b] == 0 and want[0][b, 0] == NONE
            else:
                assert (slot[id(got.cluster)], got.score) == (want[0][b, 0], want[1][b, 0])


def cli(*args, **kw):
    return subprocess.run([CLI, *args], capture_output=True, text=True, **kw)


def test_cli_match_needs_clusters(tmp_path):
    f = tmp_path / "q.tsv"
    f.write_text("1\tWVTAPRSLPVLP\n")
    r = cli("match", "-i", str(f), "-d", str(tmp_path / "out"))
    assert r.returncode == 2
    assert "--clusters" in r.stderr
    assert not (tmp_path / "out").exists()


def test_cli_match_rejects_devices(tmp_path):
    f = tmp_path / "q.tsv"
    f.write_text("1\tWVTAPRSLPVLP\n")
    r = cli("match", "-i", str(f), "--clusters", str(f), "-d", str(tmp_path / "out"), "--devices", "0,1")
    assert r.returncode == 2
    assert not (tmp_path / "out").exists()


def test_cli_help_names_match():
    r = cli("--help")
    assert r.returncode == 0
    assert "hammock-hip match" in r.stderr and "--clusters" in r.stderr and "--skip_singletons" in r.stderr and "--best" in r.stderr


def test_cli_match_rejects_na_ids(tmp_path):
    good = "cluster_id\tsequence\talignment\tsum\tl1\n3\tWVTAPRSLPVLP\tNA\t3\t3\n"
    bad = good + "NA\tNYSGNRPLPGIW\tNA\t1\t1\n"
    (tmp_path / "good.tsv").write_text(good)
    (tmp_path / "bad.tsv").write_text(bad)
    for i, c in (("bad", "good"), ("good", "bad")):
        out = tmp_path / f"out_{i}"
        r = cli("match", "-i", str(tmp_path / f"{i}.tsv"), "--clusters", str(tmp_path / f"{c}.tsv"), "-d", str(out), timeout=120)
        assert r.returncode == 3, (i, r.returncode, r.stderr)
        assert "FileFormatException" in (out / "run.log").read_text()


# ---- GPU ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 5, 32])
def test_match_uniform_12mers(gpu, coracle, k):
    M = _blosum62()
    rng = np.random.default_rng(400 + k)
    members, mc, queries, qc = two_sides(rng, 3000, 2000, 12, 12)
    mc = relabel(mc)
    for queries_first in (True, False):
        ctx, res, off, qr, rr, ids, msz = setup(M, queries, members, mc, rng, queries_first)
        blk = block(coracle, M, res, off, qr, rr, 0, 3, 0)
        want = expected(blk, mc, ids, msz, qc, 30, k)
        multi = np.bincount(qc) > 1
        assert (want[2][multi] > 0).mean() > 0.2 and (want[2] == 0).any()
        if k > 1:
            assert (want[2][multi] > 1).any()
        got = ctx.match_clusters_shifted(*qr, qc, *rr, mc, ids, 3, 0, 30, k)
        check(got, want)
        st = ctx.last_match_stats
        assert st.pairs_scored == len(queries) * len(members) and st.n_edges == int((blk >= 30).sum())


@pytest.mark.gpu
def test_match_asymmetric_matrix_orientation(gpu, coracle):
    """score(seq1 = member, seq2 = query): there are query clusters whose answer differs under the swapped orientation"""
    M = asymmetric(_blosum62())
    rng = np.random.default_rng(17)
    members, mc, queries, qc = two_sides(rng, 2000, 1500, 10, 13, trim=True)
    mc = relabel(mc)
    for queries_first in (True, False):
        ctx, res, off, qr, rr, ids, msz = setup(M, queries, members, mc, rng, queries_first)
        blk = block(coracle, M, res, off, qr, rr, 0, 3, -1)
        st, swapped = coracle.score_block(M, res, off, np.arange(*qr), np.arange(*rr), 0, 3, -1)
        assert st == 0
        for k in (1, 5, 32):
            want = expected(blk, mc, ids, msz, qc, 26, k)
            other = expected(swapped.T, mc, ids, msz, qc, 26, k)
            assert (np.any(want[0] != other[0], axis=1) | (want[2] != other[2])).sum() > 0
            check(ctx.match_clusters_shifted(*qr, qc, *rr, mc, ids, 3, -1, 26, k), want)
            assert ctx.last_match_stats.symmetric == 0


@pytest.mark.gpu
@pytest.mark.parametrize("gaps,thr", [((-5, -1), 30), ((1, 1), None)], ids=["striped", "literal"])
def test_match_local(gpu, coracle, gaps, thr):
    M = _blosum62()
    rng = np.random.default_rng(500)
    members, mc, queries, qc = two_sides(rng, 1200, 800, 9, 15, trim=True)
    mc = relabel(mc)
    for queries_first in (True, False):
        ctx, res, off, qr, rr, ids, msz = setup(M, queries, members, mc, rng, queries_first)
        blk = block(coracle, M, res, off, qr, rr, 1, gaps[0], gaps[1])
        t = thr if thr is not None else int(np.percentile(blk, 97))   # (positive gap scores lift every pair)
        for k in (1, 5, 32):
            want = expected(blk, mc, ids, msz, qc, t, k)
            assert (want[2] > 0).any() and (want[2] == 0).any()
            check(ctx.match_clusters_local(*qr, qc, *rr, mc, ids, gaps[0], gaps[1], t, k), want)


@pytest.mark.gpu
def test_match_ties(gpu):
    """equal scores: the larger cluster first; equal score and size: the smaller id first -- with query clusters of copies"""
    M = _blosum62()
    x, s = "WVTAPRSLPVLP", "WVTAPRSLPVLA"
    ctx = hammock_amd.Context(M, device=0)
    sizes = [1, 1, 1, 2, 3, 3, 1, 2]            # x three times, then five copies of s
    ctx.set_sequences([x, x, x, s, s, s, s, s], sizes=sizes)
    score = int(ctx.score_pairs_shifted([3], [0], 3, 0)[0])
    blk = np.full((5, 3), score, dtype=np.int32)
    cases = [([0, 1, 2, 3, 3], [40, 30, 20, 10], [3, 2, 1, 0]),     # sizes 2, 3, 3, 3: slot 0 last, the rest by id
             ([0, 1, 2, 3, 3], [10, 20, 30, 40], [1, 2, 3, 0]),
             ([3, 2, 1, 0, 0], [40, 30, 20, 10], [2, 1, 0, 3])]
    for qc in ([0, 0, 0], [0, 1, 1], [1, 0, 2]):
        for mc, ids, want_order in cases:
            best, sc, nf = ctx.match_clusters_shifted(0, 3, qc, 3, 8, mc, ids, 3, 0, 10, 4)
            nb = max(qc) + 1
            assert (best == np.array(want_order, dtype=np.uint32)).all() and (nf == 4).all() and (sc == score).all()
            check((best, sc, nf), expected(blk, mc, ids, sizes[3:], qc, 10, 4))
            assert best.shape == (nb, 4)


@pytest.mark.gpu
def test_match_singletons_equal_assign(gpu, coracle):
    """one member per query slot: bit-identical to assign_* on the same arguments, slot b = the query sequence labelled b"""
    M = _blosum62()
    rng = np.random.default_rng(23)
    members, mc, queries, _ = two_sides(rng, 2500, 1500, 10, 13, trim=True)
    mc = relabel(mc)
    ctx, res, off, qr, rr, ids, msz = setup(M, queries, members, mc, rng)
    label = rng.permutation(len(queries))
    for k in (1, 5, 32):
        for fn, afn, a, b, thr in ((ctx.match_clusters_shifted, ctx.assign_shifted, 3, -1, 26),
                                   (ctx.match_clusters_local, ctx.assign_local, -5, -1, 30)):
            got = fn(*qr, label, *rr, mc, ids, a, b, thr, k)
            want = afn(*qr, *rr, mc, ids, a, b, thr, k)
            assert (want[2] > 0).any()
            inv = np.argsort(label)
            check(got, (want[0][inv], want[1][inv], want[2][inv]))
            got = fn(*qr, np.arange(len(queries)), *rr, mc, ids, a, b, thr, k)
            check(got, want)
            assert ctx.last_match_stats.n_edges == ctx.last_assign_stats.n_edges


@pytest.mark.gpu
def test_match_order_does_not_matter(gpu, coracle):
    """permuting the query slots and the members inside them (the uploaded order) changes only the slot labels"""
    M = _blosum62()
    rng = np.random.default_rng(29)
    members, mc, queries, qc = two_sides(rng, 2000, 1500, 12, 12)
    mc = relabel(mc)
    ctx, res, off, qr, rr, ids, msz = setup(M, queries, members, mc, rng)
    base = ctx.match_clusters_shifted(*qr, qc, *rr, mc, ids, 3, 0, 30, 5)
    assert (base[2] > 1).any()
    nb = int(qc.max()) + 1
    perm_slot = rng.permutation(nb)                 # old slot b -> new slot perm_slot[b]
    perm_seq = rng.permutation(len(queries))        # new position i holds old query perm_seq[i]
    seqs = [queries[i] for i in perm_seq] + members
    sizes = np.concatenate([np.ones(len(queries), np.int32), msz])
    r2, o2 = hammock_amd.pack_sequences(seqs)
    ctx.set_sequences(residues=r2, offsets=o2, sizes=sizes)
    got = ctx.match_clusters_shifted(*qr, perm_slot[qc[perm_seq]], *rr, mc, ids, 3, 0, 30, 5)
    check((got[0][perm_slot], got[1][perm_slot], got[2][perm_slot]), base)


def _run_stats(blk, mc, qc, thr):
    """per query member its hits and distinct clusters (level 1), per query slot its feasible records and distinct ranks (level 2)"""
    nc = int(mc.max()) + 1
    hit = blk >= thr
    hits = hit.sum(axis=0)
    per_cluster = np.zeros((nc, blk.shape[1]), dtype=np.int64)
    np.add.at(per_cluster, mc, hit.astype(np.int64))
    distinct = (per_cluster > 0).sum(axis=0)
    feas1 = per_cluster == np.bincount(mc, minlength=nc)[:, None]           # [nc, nq]
    nb = int(qc.max()) + 1
    rec2 = np.bincount(qc, weights=feas1.sum(axis=0), minlength=nb).astype(np.int64)
    any2 = np.zeros((nc, nb), dtype=bool)
    for b in range(nb):
        any2[:, b] = feas1[:, qc == b].any(axis=1)
    return hits, distinct, rec2, any2.sum(axis=0)


@pytest.mark.gpu
def test_match_table_overflow(gpu, coracle):
    """runs of at most 4,096 records (a wave each) that touch more than 384 distinct clusters -- 3/4 of the wave's 512-slot
    table -- in both levels: the clusters are taken in 2, 4, ... classes by rank, one table fill per class"""
    M = _blosum62()
    rng = np.random.default_rng(41)
    seqs = synth_seqs(41, 3040)
    queries, members = seqs[:40], seqs[40:]
    mc = relabel(np.repeat(np.arange(2000), [1 if i % 2 else 2 for i in range(2000)])[:3000])
    qc = relabel(np.arange(40) // 2)
    ctx, res, off, qr, rr, ids, msz = setup(M, queries, members, mc, rng)
    blk = block(coracle, M, res, off, qr, rr, 0, 3, 0)
    thr = int(np.percentile(blk, 40))
    hits, distinct, rec2, distinct2 = _run_stats(blk, mc, qc, thr)
    assert hits.max() <= 4096 and distinct.min() > 384
    assert rec2.max() <= 4096 and distinct2.min() > 384
    for k in (1, 32):
        want = expected(blk, mc, ids, msz, qc, thr, k)
        assert want[2].min() > 32
        check(ctx.match_clusters_shifted(*qr, qc, *rr, mc, ids, 3, 0, thr, k), want)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["few_clusters", "many_clusters"])
def test_match_long_runs(gpu, coracle, layout):
    """runs of more than 4,096 records: a workgroup each, in both levels.  many_clusters: more than 1,536 distinct clusters
    per run, 3/4 of the workgroup's 2,048-slot table, so the workgroup splits them into classes too"""
    M = _blosum62()
    rng = np.random.default_rng(42)
    seqs = synth_seqs(42, 6030)
    queries, members = seqs[:30], seqs[30:]
    per, qper = (10, 15) if layout == "few_clusters" else (2, 3)
    mc = relabel(np.arange(6000) // per)
    qc = relabel(np.arange(30) // qper)
    ctx, res, off, qr, rr, ids, msz = setup(M, queries, members, mc, rng)
    blk = block(coracle, M, res, off, qr, rr, 0, 3, 0)
    thr = int(np.percentile(blk, 5))
    hits, distinct, rec2, distinct2 = _run_stats(blk, mc, qc, thr)
    assert hits.min() > 4096 and rec2.min() > 4096
    if layout == "many_clusters":
        assert distinct.min() > 1536 and distinct2.min() > 1536
    for k in (1, 32):
        want = expected(blk, mc, ids, msz, qc, thr, k)
        if layout == "many_clusters":
            assert want[2].min() > 32
        check(ctx.match_clusters_shifted(*qr, qc, *rr, mc, ids, 3, 0, thr, k), want)


@pytest.mark.gpu
def test_match_empty_sides(gpu):
    M = _blosum62()
    res, off = synth_peptides(4, 100, 12)
    ctx = hammock_amd.Context(M, device=0)
    ctx.set_sequences(residues=res, offsets=off)
    best, sc, nf = ctx.match_clusters_shifted(0, 0, [], 10, 20, np.arange(10) // 2, np.arange(5), 3, 0, 20, 3)
    assert best.shape == (0, 3) and sc.shape == (0, 3) and nf.shape == (0,)
    best, sc, nf = ctx.match_clusters_shifted(0, 10, np.arange(10) // 3, 10, 10, [], [], 3, 0, 20, 3)
    assert (best == NONE).all() and (sc == INT_MIN).all() and (nf == 0).all() and best.shape == (4, 3)
    best, sc, nf = ctx.match_clusters_local(0, 10, np.arange(10) % 2, 50, 50, [], [], -5, -1, 20, 1)
    assert (best == NONE).all() and (nf == 0).all() and best.shape == (2, 1)


@pytest.mark.gpu
def test_match_full_size(gpu, coracle):
    """query clusters = the greedy clusters of 10^4 12-mers of seed 2; existing clusters = those of bench.py's 10^5 set (seed 1),
    all of them and the multi-member ones.  For 200 sampled query clusters, the 20 largest among them, the whole answer is
    recomputed from score_block over every existing member x the slot's members"""
    M = _blosum62()
    X, P, THR = 3, 0, 20
    n, nq = 100_000, 10_000
    res, off = synth_peptides(1, n, 12)
    ctx = hammock_amd.Context(M, device=0)
    ctx.set_sequences(residues=res, offsets=off)
    cid, _, _ = ctx.greedy_cluster(X, P, THR, int(round(n * 0.025)))
    qres, qoff = synth_peptides(2, nq, 12)
    ctx.set_sequences(residues=qres, offsets=qoff)
    qcid, _, _ = ctx.greedy_cluster(X, P, THR, int(round(nq * 0.025)))
    qids, qc = np.unique(qcid, return_inverse=True)
    qc = qc.astype(np.uint32)
    nb = len(qids)
    qsize = np.bincount(qc, minlength=nb)
    assert qsize.max() >= 4
    rng = np.random.default_rng(7)
    largest = np.argsort(-qsize, kind="stable")[:20]
    sample = np.unique(np.concatenate([largest, rng.choice(np.setdiff1d(np.arange(nb), largest), 180, replace=False)]))
    counts = np.bincount(cid, minlength=n)
    seqs = [qres[qoff[i]:qoff[i + 1]] for i in range(nq)] + [res[off[i]:off[i + 1]] for i in range(n)]
    r2, o2 = hammock_amd.pack_sequences(seqs)
    ctx.set_sequences(residues=r2, offsets=o2)
    blocks = {}
    for b in sample:
        xs = np.nonzero(qc == b)[0]
        st, blk = coracle.score_block(M, r2, o2, np.arange(nq, nq + n), xs, 0, X, P)
        assert st == 0
        blocks[b] = blk
    for candidates in ("all", "multi"):
        members = np.arange(n) if candidates == "all" else np.nonzero(counts[cid] > 1)[0]
        ids, slot = np.unique(cid[members], return_inverse=True)
        if candidates == "multi":
            seqs2 = [qres[qoff[i]:qoff[i + 1]] for i in range(nq)] + [res[off[i]:off[i + 1]] for i in members]
            r3, o3 = hammock_amd.pack_sequences(seqs2)
            ctx.set_sequences(residues=r3, offsets=o3)
        for k in (1, 5):
            best, sc, nf = ctx.match_clusters_shifted(0, nq, qc, nq, nq + len(members), slot, ids, X, P, THR, k)
            assert best.shape == (nb, k)
            matched = 0
            for b in sample:
                blk = blocks[b][members]
                w = expected(blk, slot, ids, np.ones(len(members)), np.zeros(blk.shape[1], dtype=np.int64), THR, k)
                assert np.array_equal(best[b], w[0][0]) and np.array_equal(sc[b], w[1][0]) and nf[b] == w[2][0], (candidates, k, b)
                matched += int(w[2][0] > 0)
            assert matched > 0


def _java_round(v):
    return int(math.floor(v + 0.5))


def _antibody_halves(tmp_path, n_records=8000):
    """the odd and even records of the first n_records of antibodies.fa.gz (the oracle scores every pair of the two halves)"""
    with gzip.open(os.path.join(GOLDEN, "antibodies.fa.gz"), "rt") as fh:
        lines = fh.read().splitlines()
    records, cur = [], []
    for line in lines:
        if line.startswith(">") and cur:
            records.append(cur)
            cur = []
            if len(records) == n_records:
                break
        cur.append(line)
    if cur and len(records) < n_records:
        records.append(cur)
    a, b = tmp_path / "a.fa", tmp_path / "b.fa"
    a.write_text("\n".join(l for i, r in enumerate(records) if i % 2 == 0 for l in r) + "\n")
    b.write_text("\n".join(l for i, r in enumerate(records) if i % 2 == 1 for l in r) + "\n")
    return a, b


def _match_expectation(coracle, qfile, cfile, skip, best_k):
    """the cluster_matches.tsv rows the two cluster files call for, with the CLI's defaults"""
    M = _blosum62()
    qloaded = _cluster_file_expectation(qfile)
    loaded = _cluster_file_expectation(cfile)
    mlens = [len(s) for _, s, _ in loaded]
    X = min(_java_round(sum(mlens) / len(mlens) / 4), min(mlens + [len(s) for _, s, _ in qloaded]) - 1)
    thr = _java_round(sum(mlens) / len(mlens) * 1.7)
    ids_all = list(dict.fromkeys(cid for cid, _, _ in loaded))
    uniq = {c: 0 for c in ids_all}
    for cid, _, _ in loaded:
        uniq[cid] += 1
    cids = [c for c in ids_all if not skip or uniq[c] > 1]
    slot = {c: i for i, c in enumerate(cids)}
    mem = [(slot[cid], s, sz) for cid, s, sz in loaded if cid in slot]
    qids = list(dict.fromkeys(cid for cid, _, _ in qloaded))
    qslot = {c: i for i, c in enumerate(qids)}
    qseqs = [(qslot[cid], s) for cid, s, _ in qloaded]
    seqs = [s for _, s in qseqs] + [s for _, s, _ in mem]
    res, off = hammock_amd.pack_sequences(seqs)
    nq = len(qseqs)
    st, blk = coracle.score_block(M, res, off, np.arange(nq, len(seqs)), np.arange(nq), 0, X, 0)
    assert st == 0
    mc = np.array([c for c, _, _ in mem], dtype=np.int64)
    msz = np.array([sz for _, _, sz in mem], dtype=np.int64)
    qc = np.array([b for b, _ in qseqs], dtype=np.int64)
    best, score, nf = expected(blk, mc, cids, msz, qc, thr, best_k)
    size = np.bincount(mc, weights=msz, minlength=len(cids)).astype(np.int64)
    want = ["cluster_id\trank\tmatched_cluster_id\tscore\tmatched_size\tfeasible_clusters"]
    for b, qid in enumerate(qids):
        if nf[b] == 0:
            want.append(f"{qid}\tNA\tNA\tNA\tNA\t0")
        for t in range(min(int(nf[b]), best_k)):
            c = int(best[b, t])
            want.append(f"{qid}\t{t + 1}\t{cids[c]}\t{score[b, t]}\t{size[c]}\t{nf[b]}")
    return want, X, thr, nf, np.bincount(qc)


@pytest.mark.gpu
def test_cli_match_matches_the_expectation(gpu, coracle, tmp_path):
    """greedy on the two halves of (a prefix of) antibodies.fa.gz, then the clusters of one half matched against those of the other"""
    a, b = _antibody_halves(tmp_path)
    for half, fa in (("ga", a), ("gb", b)):
        r = cli("greedy", "-i", str(fa), "-d", str(tmp_path / half), timeout=600)
        assert r.returncode == 0, r.stderr
    qfile = tmp_path / "gb" / "initial_clusters_sequences.tsv"
    cfile = tmp_path / "ga" / "initial_clusters_sequences.tsv"
    for extra, best_k in (([], 1), (["--skip_singletons", "--best", "3"], 3), (["--best", "5"], 5)):
        want, X, thr, nf, qsize = _match_expectation(coracle, qfile, cfile, "--skip_singletons" in extra, best_k)
        assert (nf[qsize > 1] > 0).sum() > 5
        out = tmp_path / ("m" + "".join(extra).replace("-", "_"))
        r = cli("match", "-i", str(qfile), "--clusters", str(cfile), "-d", str(out), *extra, timeout=600)
        assert r.returncode == 0, r.stderr
        assert "Max shift not set. Setting automatically to: " + str(X) in r.stderr
        assert "not set. Setting automatically to: " + str(thr) in r.stderr
        assert (out / "cluster_matches.tsv").read_text().splitlines() == want
        assert (out / "run.log").exists()


@pytest.mark.gpu
def test_cli_match_of_singletons_equals_assign(gpu, tmp_path):
    """an -i file of singletons: the rows of assign's assignments.tsv, with the singleton's id in place of its sequence"""
    a, b = _antibody_halves(tmp_path)
    r = cli("greedy", "-i", str(a), "-d", str(tmp_path / "ga"), timeout=600)
    assert r.returncode == 0, r.stderr
    cfile = tmp_path / "ga" / "initial_clusters_sequences.tsv"
    from oracle import hammock_oracle as ho
    news = ho.load_unique_sequences_from_fasta(str(b))[:3000]
    text = lambda u: "".join(ALPHABET[c] for c in u.sequence)  # noqa: E731
    qseqs = [text(u) for u in news]
    (tmp_path / "new.fa").write_text("".join(f">s{i}\n{s}\n" for i, s in enumerate(qseqs)))
    (tmp_path / "q.tsv").write_text("cluster_id\tsequence\tno_label\n" + "".join(f"{1000 + i}\t{s}\t1\n" for i, s in enumerate(qseqs)))
    for extra in ([], ["--skip_singletons", "--best", "4"]):
        tag = "".join(extra).replace("-", "_")
        r = cli("assign", "-i", str(tmp_path / "new.fa"), "--clusters", str(cfile), "-d", str(tmp_path / ("a" + tag)), *extra, timeout=600)
        assert r.returncode == 0, r.stderr
        r = cli("match", "-i", str(tmp_path / "q.tsv"), "--clusters", str(cfile), "-d", str(tmp_path / ("m" + tag)), *extra, timeout=600)
        assert r.returncode == 0, r.stderr
        arows = (tmp_path / ("a" + tag) / "assignments.tsv").read_text().splitlines()[1:]
        mrows = (tmp_path / ("m" + tag) / "cluster_matches.tsv").read_text().splitlines()[1:]
        id_of = {s: str(1000 + i) for i, s in enumerate(qseqs)}
        assert len(arows) == len(mrows) and sum(r.split("\t")[1] != "NA" for r in arows) > 10
        assert sorted(mrows) == sorted(id_of[r.split("\t", 1)[0]] + "\t" + r.split("\t", 1)[1] for r in arows)
