"""Continuing a greedy clustering with new sequences (hmk_greedy_continue, Context.greedy_continue): the second loop of
LimitedGreedySequenceClusterer.cluster (LimitedGreedySequenceClusterer.java:59-67) over the new sequences [q0, q1) in index order,
seeded with the clusters of the members [r0, r1) of one uploaded set.  Unlike the assignment, a new sequence that joins a cluster
is a member for every later one.  Expectations come from a restatement of :59-67 over dense score blocks from
oracle.c_oracle.score_block; a CPU test pins the restatement against the oracle's LimitedGreedySequenceClusterer seeded with its
own phase 1.  The CPU tests run anywhere; the GPU tests need an MI355X (-m gpu)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import hammock_amd
from hammock_amd import _native as N
from hammock_amd.synth import synth_peptides
from oracle import hammock_oracle as ho

INT_MAX = 2 ** 31 - 1


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


# ---- the restatement -------------------------------------------------------------------------------------------------------

def restate(blk_mn, blk_nn, member_cluster, cluster_id, member_sizes, new_sizes, thr):
    """:59-67 with actualClusters = the slots, actualSequences = the new sequences in order.  blk_mn[m, x] = score(seq1 = member m,
    seq2 = new x), blk_nn[x, y] = score(seq1 = new x, seq2 = new y) -> (joined int32[nq], member_rank int32[nq])"""
    nm, nq = blk_mn.shape
    nc = len(cluster_id)
    joined = np.full(nq, -1, np.int32)
    rank = np.full(nq, -1, np.int32)
    if nc == 0 or nq == 0:
        return joined, rank
    mc = np.asarray(member_cluster, np.int64)
    ids = np.asarray(cluster_id, np.int64)
    size = np.bincount(mc, weights=np.asarray(member_sizes, np.float64), minlength=nc).astype(np.int64)
    count = np.bincount(mc, minlength=nc).astype(np.int64)
    order = np.argsort(mc, kind="stable")
    cur = np.minimum.reduceat(np.asarray(blk_mn, np.int64)[order], np.searchsorted(mc[order], np.arange(nc)), axis=0)   # [nc, nq]
    for x in range(nq):
        col = cur[:, x]
        ok = np.nonzero(col >= thr)[0]                     # ClinkageClusterScorer: every member >= thr, the minimum
        if ok.size == 0:
            continue                                       # :64 remainingSequences
        c = int(ok[np.lexsort((ids[ok], -size[ok], -col[ok]))[0]])   # score desc, size() desc, id asc
        joined[x], rank[x] = c, count[c]                   # :61-62 insertAll
        count[c] += 1
        size[c] += int(new_sizes[x])
        cur[c] = np.minimum(cur[c], blk_nn[x])             # x is a member for every later new sequence
    return joined, rank


def blocks(coracle, M, res, off, qr, rr, a, b):
    st, mn = coracle.score_block(M, res, off, np.arange(*rr), np.arange(*qr), 0, a, b)
    assert st == 0
    st, nn = coracle.score_block(M, res, off, np.arange(*qr), np.arange(*qr), 0, a, b)
    assert st == 0
    return mn, nn


# ---- sequences -------------------------------------------------------------------------------------------------------------

def mutate(rng, p, n_sub, alphabet=20):
    q = p.copy()
    for pos in rng.choice(len(q), size=n_sub, replace=False):
        q[pos] = rng.integers(0, alphabet)
    return q


def families(rng, n_members, n_new, len_lo, len_hi, alphabet=20, max_cluster=5):
    """members in clusters around random centres, new sequences that are near copies of the centres or random ->
    (members, member_cluster, new)"""
    members, mc, new, centres = [], [], [], []
    while len(members) < n_members:
        centre = rng.integers(0, alphabet, size=int(rng.integers(len_lo, len_hi + 1))).astype(np.uint8)
        centres.append(centre)
        for _ in range(int(rng.integers(1, 3))):
            c = int(mc[-1]) + 1 if mc else 0
            for _ in range(int(rng.integers(1, max_cluster + 1))):
                members.append(mutate(rng, centre, int(rng.integers(0, 2)), alphabet))
                mc.append(c)
    members, mc = members[:n_members], np.asarray(mc[:n_members])
    _, mc = np.unique(mc, return_inverse=True)
    for _ in range(n_new):
        if rng.random() < 0.85:
            new.append(mutate(rng, centres[int(rng.integers(len(centres)))], int(rng.integers(0, 3)), alphabet))
        else:
            new.append(rng.integers(0, alphabet, size=int(rng.integers(len_lo, len_hi + 1))).astype(np.uint8))
    return members, mc.astype(np.uint32), new


def upload(M, members, new, msizes, nsizes, new_first):
    nm, nq = len(members), len(new)
    if new_first:
        seqs, sizes, qr, rr = new + members, np.concatenate([nsizes, msizes]), (0, nq), (nq, nq + nm)
    else:
        seqs, sizes, qr, rr = members + new, np.concatenate([msizes, nsizes]), (nm, nm + nq), (0, nm)
    res, off = hammock_amd.pack_sequences(seqs)
    ctx = hammock_amd.Context(M, device=0)
    ctx.set_sequences(residues=res, offsets=off, sizes=sizes.astype(np.int32))
    return ctx, res, off, qr, rr


def run_case(coracle, M, members, mc, new, ids, msizes, nsizes, X, p, thr, new_first):
    ctx, res, off, qr, rr = upload(M, members, new, msizes, nsizes, new_first)
    mn, nn = blocks(coracle, M, res, off, qr, rr, X, p)
    want = restate(mn, nn, mc, ids, msizes, nsizes, thr)
    got = ctx.greedy_continue(*qr, *rr, mc, ids, X, p, thr)
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1], want[1])
    st = ctx.last_continue_stats
    assert st.n_joined == int((want[0] >= 0).sum())
    assert st.n_edges == int((mn >= thr).sum()) + int((np.triu(nn, 1) >= thr)[np.triu_indices(len(new), 1)].sum())
    assert st.pairs_scored == len(members) * len(new) + len(new) * (len(new) - 1) // 2
    ctx.close()
    return got, st


def blosum62(matrices):
    return np.asarray(matrices["blosum62"], dtype=np.int32)


# ---- CPU ---------------------------------------------------------------------------------------------------------------------

def test_symbol_declared_exported_abi_4():
    with open(os.path.join(ROOT, "include", "hammock_hip.h")) as fh:
        header = fh.read()
    assert re.search(r"\bint hmk_greedy_continue\(", header) and "hmk_continue_stats" in header
    assert "hmk_greedy_continue" in N.SYMBOLS
    assert hasattr(N.lib, "hmk_greedy_continue")
    assert N.lib.hmk_abi_version() == 4
    assert C.sizeof(N.ContinueStats) == 48


def test_restatement_matches_oracle_second_loop(matrices):
    """the restatement, seeded with the oracle's _first_phase, gives the oracle's LimitedGreedySequenceClusterer.cluster"""
    M = blosum62(matrices)
    rng = np.random.default_rng(3)
    for trial in range(3):
        centres = [rng.integers(0, 20, size=int(rng.integers(7, 11))) for _ in range(6)]
        raw = [mutate(rng, centres[int(rng.integers(6))], int(rng.integers(0, 3))) for _ in range(70)]
        strs = sorted({"".join(ho.AMINO_ACIDS[i] for i in s) for s in raw})
        sizes = rng.integers(1, 4, size=len(strs))
        seqs = [ho.UniqueSequence(s, {"a": int(z)}) for s, z in zip(strs, sizes)]
        p, thr, maxc = (0, -1, 0)[trial % 2], (20, 25, 30)[trial], 4
        scorer = ho.ShiftedScorer(M.tolist(), p, 2)
        want = ho.LimitedGreedySequenceClusterer(scorer, thr, maxc, 1).cluster(seqs)
        g = ho.LimitedGreedySequenceClusterer(scorer, thr, maxc, 1)
        state = g._first_phase(seqs, maxc, ho.ClinkageClusterScorer(scorer, thr))
        k = next((i for i, c in enumerate(state) if c.get_unique_size() == 1), len(state))
        clusters, left = state[:k], [c.sequences[0] for c in state[k:]]
        members = [s for c in clusters for s in c.sequences]
        mc = np.asarray([i for i, c in enumerate(clusters) for _ in c.sequences], np.int64)
        ids = [c.id for c in clusters]
        mn = np.asarray([[scorer.sequence_score(m, x) for x in left] for m in members], np.int64).reshape(len(members), len(left))
        nn = np.asarray([[scorer.sequence_score(x, y) for y in left] for x in left], np.int64).reshape(len(left), len(left))
        joined, rank = restate(mn, nn, mc, ids, [s.size() for s in members], [s.size() for s in left], thr)
        where = {id(s): (ci, r) for ci, c in enumerate(want) for r, s in enumerate(c.sequences)}
        for x, s in enumerate(left):
            ci, r = where[id(s)]
            if joined[x] < 0:
                assert want[ci].get_unique_size() == 1 and ci >= k
            else:
                assert (want[ci].id, r) == (ids[joined[x]], rank[x])
        assert len(want) == k + int((joined < 0).sum())


def test_argument_errors_host_only(matrices):
    M = blosum62(matrices)
    ctx = hammock_amd.Context(M, device=-1)
    res, off = synth_peptides(1, 10, 8)
    ctx.set_sequences(residues=res, offsets=off)
    mc, ids = np.array([0, 0, 1], np.uint32), np.array([5, 6], np.int32)
    bad = [
        ((0, 11, 0, 0, [], []), "ranges"),
        ((3, 2, 5, 8, mc, ids), "ranges"),
        ((0, 4, 3, 6, mc, ids), "overlap"),
        ((0, 4, 5, 8, [0, 0, 2], ids), "not a slot"),
        ((0, 4, 5, 8, [0, 0, 0], ids), "has no member"),
        ((0, 4, 5, 8, mc, [7, 7]), "two slots"),
    ]
    for (q0, q1, r0, r1, m, i), what in bad:
        with pytest.raises(ValueError, match=what):
            ctx.greedy_continue(q0, q1, r0, r1, m, i, 2, 0, 20)
    asym = M.copy()
    asym[0, 1] += 1
    ctx2 = hammock_amd.Context(asym, device=-1)
    ctx2.set_sequences(residues=res, offsets=off)
    with pytest.raises(ValueError, match="symmetric"):
        ctx2.greedy_continue(0, 4, 5, 8, mc, ids, 2, 0, 20)
    j, r = (np.zeros(4, np.int32) for _ in range(2))
    assert N.lib.hmk_greedy_continue(ctx._h, 0, 4, 5, 8, None, None, 2, 2, 0, 20, j.ctypes.data_as(C.POINTER(C.c_int32)),
                                     r.ctypes.data_as(C.POINTER(C.c_int32)), None) == N.HMK_ERR_BAD_ARG
    ctx.close()
    ctx2.close()


# ---- GPU ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("seed,lens,X,p,thr,new_first", [
    (1, (7, 20), 2, 0, 22, True), (2, (7, 20), 3, -1, 18, False), (3, (9, 14), 1, 0, 30, False), (4, (12, 12), 3, -1, 26, True)])
def test_parity_mixed(gpu, coracle, matrices, seed, lens, X, p, thr, new_first):
    M = blosum62(matrices)
    rng = np.random.default_rng(seed)
    members, mc, new = families(rng, 600, 700, *lens)
    nc = int(mc.max()) + 1
    ids = rng.permutation(np.arange(nc) * 3 - nc).astype(np.int32)   # permuted, partly negative
    msizes = rng.integers(1, 5, size=len(members)).astype(np.int32)
    nsizes = rng.integers(1, 5, size=len(new)).astype(np.int32)
    (joined, _), _ = run_case(coracle, M, members, mc, new, ids, msizes, nsizes, X, p, thr, new_first)
    assert (joined >= 0).sum() > 20


@pytest.mark.gpu
def test_ties_low_entropy_chains(gpu, coracle, matrices):
    """two letters, equal sizes: scores and sizes tie and the id decides; near-duplicate families make long chains"""
    M = blosum62(matrices)
    rng = np.random.default_rng(11)
    for new_first in (True, False):
        members, mc, new = families(rng, 300, 900, 10, 10, alphabet=2, max_cluster=3)
        nc = int(mc.max()) + 1
        ids = rng.permutation(nc).astype(np.int32)
        ones_m, ones_n = np.ones(len(members), np.int32), np.ones(len(new), np.int32)
        (joined, _), _ = run_case(coracle, M, members, mc, new, ids, ones_m, ones_n, 1, 0, 30, new_first)
        assert (joined >= 0).sum() > 100


@pytest.mark.gpu
def test_zero_candidates_zero_joins_all_join(gpu, coracle, matrices):
    M = blosum62(matrices)
    rng = np.random.default_rng(5)
    members, mc, new = families(rng, 200, 300, 8, 12)
    nc = int(mc.max()) + 1
    ids = np.arange(nc, dtype=np.int32)
    ms, ns = rng.integers(1, 3, size=len(members)).astype(np.int32), np.ones(len(new), np.int32)
    ctx, res, off, qr, rr = upload(M, members, new, ms, ns, True)
    j, r = ctx.greedy_continue(*qr, rr[0], rr[0], [], [], 2, 0, 20)           # no candidate slot
    assert (j == -1).all() and (r == -1).all() and j.size == len(new)
    j, r = ctx.greedy_continue(*qr, *rr, mc, ids, 2, 0, 500)                  # nothing reaches the threshold
    assert (j == -1).all() and ctx.last_continue_stats.n_joined == 0
    ctx.close()
    (j, r), _ = run_case(coracle, M, members, mc, new, ids, ms, ns, 2, 0, -200, True)   # every pair: every new sequence joins
    assert (j >= 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("thr", [-300, -100])   # 8-byte adjacency entries / 4-byte entries (score - threshold fits 0..255)
def test_precheck_overflow_host_lists(gpu, coracle, matrices, thr):
    """70,000 one-member slots next to every new sequence: more clusters than k_greedy_precheck's tables take"""
    M = blosum62(matrices)
    res0, off0 = synth_peptides(9, 70010, 12)
    seqs = [res0[off0[k]:off0[k + 1]] for k in range(70010)]
    members, new = seqs[:70000], seqs[70000:]
    mc = np.arange(70000, dtype=np.uint32)
    ids = np.arange(70000, dtype=np.int32)[::-1].copy()
    ms, ns = np.ones(70000, np.int32), np.ones(10, np.int32)
    (j, _), st = run_case(coracle, M, members, mc, new, ids, ms, ns, 2, 0, thr, False)
    assert st.host_precheck == 1 and (j >= 0).all()


@pytest.mark.gpu
def test_composition(gpu, coracle, matrices):
    """continue(continue(C, A), B) == continue(C, A ++ B)"""
    M = blosum62(matrices)
    rng = np.random.default_rng(8)
    members, mc, new = families(rng, 400, 800, 8, 14)
    nc = int(mc.max()) + 1
    ids = (np.arange(nc) * 5 + 3).astype(np.int32)
    ms, ns = rng.integers(1, 4, size=len(members)).astype(np.int32), rng.integers(1, 4, size=len(new)).astype(np.int32)
    A, B = new[:500], new[500:]
    ctx, res, off, qr, rr = upload(M, members, new, ms, ns, False)
    jall, rall = ctx.greedy_continue(*qr, *rr, mc, ids, 2, -1, 24)
    ctx.close()
    ctx, res, off, qr, rr = upload(M, members, A, ms, ns[:500], False)
    ja, ra = ctx.greedy_continue(*qr, *rr, mc, ids, 2, -1, 24)
    ctx.close()
    assert np.array_equal(ja, jall[:500]) and np.array_equal(ra, rall[:500])
    # C' = C plus A's joiners, each slot's members in Cluster.getSequences() order
    order = sorted(range(500), key=lambda x: (ja[x], ra[x]))
    joiners = [x for x in order if ja[x] >= 0]
    members2 = members + [A[x] for x in joiners]
    mc2 = np.concatenate([mc, ja[joiners]]).astype(np.uint32)
    ms2 = np.concatenate([ms, ns[:500][joiners]]).astype(np.int32)
    ctx, res, off, qr, rr = upload(M, members2, B, ms2, ns[500:], True)
    jb, rb = ctx.greedy_continue(*qr, *rr, mc2, ids, 2, -1, 24)
    ctx.close()
    assert np.array_equal(jb, jall[500:]) and np.array_equal(rb, rall[500:])


def _phase1_state(M, seqs_res, off, sizes, X, p, thr, maxc, dense):
    """the oracle's _first_phase on S with a scorer that looks scores up in the dense block"""
    useqs = []
    for k in range(len(off) - 1):
        u = ho.UniqueSequence("".join(ho.AMINO_ACIDS[i] for i in seqs_res[off[k]:off[k + 1]]), {"a": int(sizes[k])})
        u.k = k
        useqs.append(u)

    class Dense:
        calls = 0

        def sequence_score(self, a, b):
            return int(dense[a.k, b.k])

    sc = Dense()
    g = ho.LimitedGreedySequenceClusterer(sc, thr, maxc, 1)
    state = g._first_phase(useqs, maxc, ho.ClinkageClusterScorer(sc, thr))
    k = next((i for i, c in enumerate(state) if c.get_unique_size() == 1), len(state))
    return state[:k], [c.sequences[0].k for c in state[k:]]


@pytest.mark.gpu
@pytest.mark.parametrize("n,maxc", [(400, 12), (2600, 25)])   # fewer / more than the greedy's 512 leftovers
def test_equivalence_with_greedy_from_phase1(gpu, coracle, matrices, n, maxc):
    """continuing the phase-1 clusters with the leftovers (orphans, then the free sequences) is hmk_greedy_cluster(S); every
    multi-member cluster is a clique"""
    M = blosum62(matrices)
    rng = np.random.default_rng(n)
    centres = [rng.integers(0, 20, size=12).astype(np.uint8) for _ in range(n // 25)]
    seqs, seen = [], set()
    while len(seqs) < n:   # (unique sequences: Cluster.insert refuses a sequence twice)
        s = mutate(rng, centres[int(rng.integers(len(centres)))], int(rng.integers(1, 4)))
        if s.tobytes() not in seen:
            seen.add(s.tobytes())
            seqs.append(s)
    res, off = hammock_amd.pack_sequences(seqs)
    sizes = rng.integers(1, 4, size=n).astype(np.int32)
    X, p, thr = 2, 0, 35
    ctx = hammock_amd.Context(M, device=0)
    ctx.set_sequences(residues=res, offsets=off, sizes=sizes)
    gcid, gorder, _ = ctx.greedy_cluster(X, p, thr, maxc)
    grank = ctx.member_rank[:n].copy()
    ctx.close()
    st, dense = coracle.score_block(M, res, off, np.arange(n), np.arange(n), 0, X, p)
    assert st == 0
    clusters, left = _phase1_state(M, res, off, sizes, X, p, thr, maxc, dense)
    members = [s.k for c in clusters for s in c.sequences]
    mc = np.asarray([i for i, c in enumerate(clusters) for _ in c.sequences], np.uint32)
    ids = np.asarray([c.id for c in clusters], np.int32)
    perm = members + left
    ctx = hammock_amd.Context(M, device=0)
    r2, o2 = hammock_amd.pack_sequences([seqs[k] for k in perm])
    ctx.set_sequences(residues=r2, offsets=o2, sizes=sizes[perm])
    nm = len(members)
    joined, rank = ctx.greedy_continue(nm, n, 0, nm, mc, ids, X, p, thr)
    ctx.close()
    cid = np.empty(n, np.int32)
    mrank = np.empty(n, np.int32)
    for ci, c in enumerate(clusters):
        for r, s in enumerate(c.sequences):
            cid[s.k], mrank[s.k] = c.id, r
    for x, k in enumerate(left):
        cid[k] = ids[joined[x]] if joined[x] >= 0 else k
        mrank[k] = rank[x] if joined[x] >= 0 else 0
    order = np.concatenate([ids, np.asarray([k for x, k in enumerate(left) if joined[x] < 0], np.int32)])
    assert len(left) > 0 and (joined >= 0).sum() > 0
    assert (len(left) < 512) == (n < 1000)   # the greedy's host loop (<= 512 leftovers) and its device loop
    assert np.array_equal(cid, gcid) and np.array_equal(mrank, grank) and np.array_equal(order, gorder)
    for c in np.unique(cid):
        idx = np.nonzero(cid == c)[0]
        if idx.size > 1:
            assert dense[np.ix_(idx, idx)][~np.eye(idx.size, dtype=bool)].min() >= thr


# ---- CLI ---------------------------------------------------------------------------------------------------------------------

CLI = os.path.join(ROOT, "hammock_amd", "bin", "hammock-hip")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def cli(*args, timeout=60):
    import subprocess
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=timeout)


def test_cli_continue_argument_errors(tmp_path):
    fa = os.path.join(GOLDEN, "musi.fa")
    r = cli("continue", "-i", fa, "-d", str(tmp_path / "a"))
    assert r.returncode == 2 and "--clusters" in r.stderr
    r = cli("continue", "--clusters", fa, "-d", str(tmp_path / "b"))
    assert r.returncode == 2 and "-i or --input" in r.stderr
    r = cli("continue", "-i", fa, "--clusters", fa, "--devices", "0,1", "-d", str(tmp_path / "c"))
    assert r.returncode == 2 and "--devices" in r.stderr
    r = cli("continue", "-i", fa, "--clusters", fa, "-f", "seq", "-d", str(tmp_path / "d"))
    assert r.returncode == 2 and "-f" in r.stderr


def read_cluster_file(path):
    """[(cluster_id, sequence, size)] in line order (the label columns summed)"""
    lines = open(path).read().splitlines()
    head = lines[0].split("\t")
    ci, si = head.index("cluster_id"), head.index("sequence")
    lab = [k for k, h in enumerate(head) if k not in (ci, si) and h not in ("alignment", "sum")]
    return [(int(f[ci]), f[si], sum(int(f[k]) for k in lab if k < len(f) and f[k] not in ("", "NA")))
            for f in (line.split("\t") for line in lines[1:])]


@pytest.mark.gpu
def test_cli_greedy_then_continue(gpu, matrices, tmp_path):
    """greedy on part of musi.fa, continue with the rest: joins equal the API's, the output loads back, duplicates are merged,
    and the output can be continued again"""
    with open(os.path.join(GOLDEN, "musi.fa")) as fh:
        lines = fh.read().splitlines()
    records = [lines[k:k + 2] for k in range(0, len(lines), 2)]
    kept, b1, b2 = tmp_path / "kept.fa", tmp_path / "b1.fa", tmp_path / "b2.fa"
    kept.write_text("\n".join(l for i, r in enumerate(records) if i % 5 for l in r) + "\n")
    dup = records[1]   # a record greedy clusters: continuing with it again merges its count
    b1.write_text("\n".join(l for i, r in enumerate(records) if i % 10 == 0 for l in r) + "\n" + "\n".join(dup) + "\n")
    b2.write_text("\n".join(l for i, r in enumerate(records) if i % 10 == 5 for l in r) + "\n")
    r = cli("greedy", "-i", str(kept), "-d", str(tmp_path / "g"), timeout=600)
    assert r.returncode == 0, r.stderr
    cfile = tmp_path / "g" / "initial_clusters_sequences.tsv"
    loaded = read_cluster_file(cfile)
    r = cli("continue", "-i", str(b1), "--clusters", str(cfile), "-d", str(tmp_path / "c1"), timeout=600)
    assert r.returncode == 0, r.stderr
    assert "1 new sequences were already in the cluster file" in r.stderr
    assert "it should be the original run's" in r.stderr
    X = int(re.search(r"Max shift not set. Setting automatically to: (\d+)", r.stderr).group(1))
    thr = int(re.search(r"threshold not set. Setting automatically to: (-?\d+)", r.stderr).group(1))
    newrows = [l.split("\t") for l in (tmp_path / "c1" / "new_sequences.tsv").read_text().splitlines()[1:]]
    new_seq = [f[0] for f in newrows]
    assert dup[1] not in new_seq
    # the API on the same inputs: the file's multi-member clusters in first-line order, the new sequences in processing order
    from collections import Counter
    held = Counter(l for i, r in enumerate(records) if i % 10 == 0 for l in r[1:])
    cids = list(dict.fromkeys(c for c, _, _ in loaded))
    uniq = Counter(c for c, _, _ in loaded)
    cand = [c for c in cids if uniq[c] > 1]
    slot = {c: k for k, c in enumerate(cand)}
    mem = [(slot[c], s, sz + (1 if s == dup[1] else 0)) for c, s, sz in loaded if c in slot]
    nsz = np.asarray([held[s] for s in new_seq], np.int32)
    assert (np.diff(nsz) <= 0).all()   # -R size: the most frequent first
    M = blosum62(matrices)
    ctx, res, off, qr, rr = upload(M, [hammock_amd.encode(s) for _, s, _ in mem], [hammock_amd.encode(s) for s in new_seq],
                                   np.asarray([z for _, _, z in mem], np.int32), nsz, False)
    joined, rank = ctx.greedy_continue(*qr, *rr, np.asarray([c for c, _, _ in mem], np.uint32), np.asarray(cand, np.int32), X, 0, thr)
    ctx.close()
    top = max(cids)
    k, want = 0, []
    for q in range(len(new_seq)):
        if joined[q] >= 0:
            want.append((cand[joined[q]], 1))
        else:
            want.append((top + 1 + k, 0))
            k += 1
    assert [(int(f[1]), int(f[2])) for f in newrows] == want
    assert sum(j >= 0 for j in joined) > 0
    out = read_cluster_file(tmp_path / "c1" / "initial_clusters_sequences.tsv")
    got = {s: (c, z) for c, s, z in out}
    for (c, j), s in zip(want, new_seq):
        assert got[s][0] == c
    before = {s: z for _, s, z in loaded}
    assert got[dup[1]][1] == before[dup[1]] + 1
    assert len(out) == len(loaded) + len(new_seq)
    # ... and it loads back and can be continued again
    r = cli("continue", "-i", str(b2), "--clusters", str(tmp_path / "c1" / "initial_clusters_sequences.tsv"), "-d", str(tmp_path / "c2"),
            "-x", str(X), "-g", str(thr), timeout=600)
    assert r.returncode == 0, r.stderr
    out2 = read_cluster_file(tmp_path / "c2" / "initial_clusters_sequences.tsv")
    assert len(out2) == len(out) + len((tmp_path / "c2" / "new_sequences.tsv").read_text().splitlines()) - 1
    assert (tmp_path / "c2" / "run.log").exists() and (tmp_path / "c2" / "initial_clusters.tsv").exists()
