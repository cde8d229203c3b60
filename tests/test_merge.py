"""Merging given clusters by complete linkage: hmk_clinkage_merge / hmk_clinkage_merge_from_edges / hmk_cluster_pairs_shifted.

CPU part (host-only context, hmk_clinkage_merge_from_edges): the chain started from given clusters against hmk_clinkage_from_edges
(singleton seeds), against a literal restatement of ClinkageSequenceClusterer.cluster with its seeding replaced (built from the
Python oracle's own parts: cluster pairs are scored member by member, no thresholded graph), properties that need no oracle, and the
argument checks.  GPU part: the device-side cluster graph (k_merge.hip) against numpy on the C oracle's score block, its four table
paths and the 8-byte CSR entries, and hmk_clinkage_merge against hmk_clinkage_merge_from_edges / hmk_clinkage_cluster.

CLI (`hammock-hip merge`): argument and file-format errors on the CPU; the run itself, the renumbering and the duplicate-sequence
rule on the GPU (test_cli_merge_two_greedy_runs, test_cli_merge_duplicate_sequences): they are not exposed through io-selftest."""
import gzip
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, random_peptides
from oracle import hammock_oracle as po
from test_assign import gpu, relabel   # noqa: F401  (gpu: the fixture that skips where no HIP device is visible)
from test_continue import cli, read_cluster_file
from test_host_greedy import oracle_edges

import hammock_amd
from hammock_amd import _native as N
from hammock_amd.synth import synth_peptides

LETTERS = "ARNDCQEGHILKMFPSTWYV"


# ---- inputs ----------------------------------------------------------------------------------------------------------------

def mutant(rng, p, n_sub, alphabet):
    q = p.copy()
    for pos in rng.choice(len(q), size=n_sub, replace=False):
        q[pos] = rng.integers(0, alphabet)
    return q


def families(rng, n_centres, len_lo, len_hi, alphabet):
    """families of mutants around random centres: 1-4 clusters per centre, 1-4 members each, 0-2 substitutions, all sequences
    distinct, members of a cluster NOT adjacent in the returned order -> (peptides, member_cluster uint32, sizes int32)"""
    peps, mc, seen = [], [], set()
    c = 0
    for _ in range(n_centres):
        centre = rng.integers(0, alphabet, size=int(rng.integers(len_lo, len_hi + 1))).astype(np.uint8)
        for _ in range(int(rng.integers(1, 5))):
            added = 0
            for _ in range(int(rng.integers(1, 5))):
                q = mutant(rng, centre, int(rng.integers(0, 3)), alphabet)
                if q.tobytes() in seen:
                    continue
                seen.add(q.tobytes())
                peps.append(q)
                mc.append(c)
                added += 1
            c += added > 0
    perm = rng.permutation(len(peps))
    peps = [peps[k] for k in perm]
    mc = relabel(np.asarray(mc)[perm])
    return peps, mc, rng.integers(1, 5, size=len(peps)).astype(np.int32)


def family_case(seed):
    """the inputs of the seeded-chain tests: 12-mers and mixed 8-12-mers, alphabets of 20 and of 4-6 letters, thresholds 14-38,
    X = 2, ids a random permutation of a CONSECUTIVE range (consecutive ids cannot pile up in one HashSet bucket)"""
    rng = np.random.default_rng(52_000 + seed)
    alphabet = 20 if seed % 2 else 4 + seed % 3
    lo = 12 if seed % 4 < 2 else 8
    peps, mc, sizes = families(rng, int(rng.integers(3, 13)), lo, 12, alphabet)
    ncl = int(mc.max()) + 1
    ids = (int(rng.integers(1, 5000)) + rng.permutation(ncl)).astype(np.int32)
    return peps, mc, sizes, ids, 2, -(seed % 3), 14 + (seed * 7) % 25


def host_ctx(M, peps, sizes=None):
    res, off = hammock_amd.pack_sequences(peps)
    ctx = hammock_amd.Context(M, device=-1)
    ctx.set_sequences(residues=res, offsets=off, sizes=sizes)
    return ctx, res, off


# ---- the literal restatement ---------------------------------------------------------------------------------------------------

class StaleStack(Exception):
    pass


def seeded_oracle(M, peps, sizes, mc, ids, X, p, thr, version):
    """ClinkageSequenceClusterer.cluster (oracle/hammock_oracle.py, :43-124) with :50-55 replaced by "the given clusters, added in slot
    order": -> (merged_id per slot, ids in list order, member_rank per member, merges).  StaleStack where the chain returns to a
    cluster that is still on its stack below stack[-2] (the reference goes on with a stale object there)."""
    old = po.JAVA_HASHSET
    po.JAVA_HASHSET = version
    try:
        seqs = [po.UniqueSequence("".join(LETTERS[r] for r in q), {"no_label": int(sizes[k])}) for k, q in enumerate(peps)]
        index_of = {id(s): k for k, s in enumerate(seqs)}
        scorer = po.CachedClusterScorer(po.ClinkageClusterScorer(po.ShiftedScorer(M.tolist(), p, X), thr), 1)
        stack, ready, active = [], po._cluster_set(), po._cluster_set()
        for c in range(len(ids)):
            active.add(po.Cluster([seqs[k] for k in np.flatnonzero(mc == c)], int(ids[c])))
        current_id = int(max(ids)) + 1
        sum_commodity = sum(c.get_unique_size() for c in active)
        merges = 0
        while len(active) > 1:
            stack.append(active.first())
            while stack:
                top = stack[-1]
                found = po._nearest_over_hash_parts(active, top, scorer, sum_commodity, 1)
                max_score, nearest = po.INT_MIN, None
                if found is not None:
                    nearest, max_score = found.cluster, found.score
                if max_score < thr:
                    stack.pop()
                    ready.add(top)
                    active.remove(top)
                    sum_commodity -= top.get_unique_size()
                    continue
                if len(stack) > 1 and stack[-2].id == nearest.id:
                    current_id += 1
                    stack.pop()
                    stack.pop()
                    active.remove(top)
                    active.remove(nearest)
                    scorer.join(top, nearest, current_id)
                    sum_commodity -= top.get_unique_size() + nearest.get_unique_size()
                    merged = top.sequences
                    merged.extend(nearest.sequences)
                    new_top = po.Cluster(merged, current_id)
                    active.add(new_top)
                    sum_commodity += new_top.get_unique_size()
                    merges += 1
                else:
                    if any(s.id == nearest.id for s in stack):
                        raise StaleStack(nearest.id)
                    stack.append(nearest)
        ready.add(active.first())
        merged_id = np.zeros(len(ids), dtype=np.int32)
        rank = np.zeros(len(peps), dtype=np.int32)
        order = []
        for cl in ready:
            order.append(cl.id)
            for pos, s in enumerate(cl.sequences):
                k = index_of[id(s)]
                merged_id[mc[k]] = cl.id
                rank[k] = pos
        return merged_id, np.asarray(order, dtype=np.int32), rank, merges
    finally:
        po.JAVA_HASHSET = old


# ---- CPU ------------------------------------------------------------------------------------------------------------------------

def test_merge_symbols():
    with open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "hammock_hip.h")) as fh:
        header = fh.read()
    for name in ("hmk_cluster_pairs_shifted", "hmk_clinkage_merge", "hmk_clinkage_merge_from_edges"):
        assert name + "(" in header and name in N.SYMBOLS and hasattr(N.lib, name)
    assert "hmk_merge_stats" in header
    assert N.lib.hmk_abi_version() == 4


@pytest.mark.parametrize("version", [8, 7, 6])
@pytest.mark.parametrize("seed", range(6))
def test_singleton_seeds_are_clinkage(blosum62, coracle, seed, version):
    """slots = the n sequences, ids 1 .. n: everything equals hmk_clinkage_from_edges on the same edges (the inputs of
    test_host_greedy.test_clinkage_from_edges_matches_oracle, same generator and seeds)"""
    rng = np.random.default_rng(900 + seed)
    n = int(rng.integers(2, 500))
    peps = random_peptides(rng, n, 9 if seed % 2 else 12, 12, alphabet=4 + seed % 3)
    sizes = rng.integers(1, 5, size=n).astype(np.int32) if seed % 3 else None
    X, p, thr = 2 + seed % 2, -(seed % 2), 12 + 2 * seed
    ctx, res, off = host_ctx(blosum62, peps, sizes)
    ctx.set_java_hashset(version)
    edges = oracle_edges(coracle, blosum62, res, off, X, p, thr, True)
    cid, order, stats = ctx.clinkage_from_edges(edges)
    rank = ctx.member_rank[:n].copy()
    merged, morder = ctx.clinkage_merge_from_edges(edges, 0, n, np.arange(n), np.arange(1, n + 1))
    assert np.array_equal(merged, cid) and np.array_equal(morder, order) and np.array_equal(ctx.member_rank, rank)
    ms = ctx.last_merge_stats
    assert (ms.merges, ms.searches, ms.n_result_clusters) == (stats.merges, stats.searches, stats.n_result_clusters)
    assert ms.n_edges == len(edges) == ms.cluster_pairs


def test_singleton_seeds_stale_stack(matrices, coracle):
    """the two stale-stack inputs of test_host_greedy.test_clinkage_from_edges_chain_returns_to_a_stacked_cluster: same error, same
    message"""
    M = matrices["blosum75"]
    four = ["TTKFVE", "DTKFVE", "QTKFVE", "ETKFVE"]
    for strings in (four, four + ["WWWWWW", "CCCCCC", "WWWWWC"]):
        res, off = coracle.pack(strings)
        ctx = hammock_amd.Context(M, device=-1)
        ctx.set_sequences(residues=res, offsets=off)
        edges = oracle_edges(coracle, M, res, off, 2, -2, 19, True)
        with pytest.raises(hammock_amd.ReferenceWouldCrash, match="still on its stack") as e1:
            ctx.clinkage_from_edges(edges)
        n = len(strings)
        with pytest.raises(hammock_amd.ReferenceWouldCrash, match="still on its stack") as e2:
            ctx.clinkage_merge_from_edges(edges, 0, n, np.arange(n), np.arange(1, n + 1))
        assert str(e1.value) == str(e2.value)


N_FAMILY_CASES = 120


def test_seeded_chain_against_the_literal_oracle(blosum62, coracle):
    """120 family inputs x the three Java orders against the restatement: partition, ids, list order, member order.  No case is
    skipped; a case in which the restatement meets the stale-stack condition counts only if the library answers
    HMK_ERR_REFERENCE_WOULD_CRASH; at least 90 % of the cases must have a merge, counted on the restatement."""
    runs = with_merge = 0
    for seed in range(N_FAMILY_CASES):
        peps, mc, sizes, ids, X, p, thr = family_case(seed)
        ctx, res, off = host_ctx(blosum62, peps, sizes)
        edges = oracle_edges(coracle, blosum62, res, off, X, p, thr, True)
        for version in (8, 7, 6):
            ctx.set_java_hashset(version)
            runs += 1
            try:
                want = seeded_oracle(blosum62, peps, sizes, mc, ids, X, p, thr, version)
            except StaleStack:
                with pytest.raises(hammock_amd.ReferenceWouldCrash, match="still on its stack"):
                    ctx.clinkage_merge_from_edges(edges, 0, len(peps), mc, ids)
                continue
            merged, order = ctx.clinkage_merge_from_edges(edges, 0, len(peps), mc, ids)
            where = f"seed {seed}, Java {version}"
            assert np.array_equal(merged, want[0]), where
            assert np.array_equal(order, want[1]), where
            assert np.array_equal(ctx.member_rank, want[2]), where
            assert ctx.last_merge_stats.merges == want[3], where
            with_merge += want[3] > 0
    assert runs == 3 * N_FAMILY_CASES
    assert with_merge >= 0.9 * runs, (with_merge, runs)


@pytest.mark.parametrize("seed", range(8))
def test_merge_properties(blosum62, coracle, seed):
    """idempotence (complete linkage is monotone: what a finished merge left apart stays apart), scores inside a slot and edges
    outside the range are ignored, members-first and members-last layouts agree"""
    peps, mc, sizes, ids, X, p, thr = family_case(1000 + seed)
    nm, ncl = len(peps), len(ids)
    rng = np.random.default_rng(seed)
    extra = random_peptides(rng, 7, 12, 12, alphabet=4)
    ctx, res, off = host_ctx(blosum62, peps + extra, np.concatenate([sizes, np.ones(7, np.int32)]))
    edges = oracle_edges(coracle, blosum62, res, off, X, p, thr, True)
    x, m, _ = hammock_amd.edge_fields(edges)
    merged, order = ctx.clinkage_merge_from_edges(edges, 0, nm, mc, ids)
    rank = ctx.member_rank.copy()
    n_merges = ctx.last_merge_stats.merges
    assert len(order) == ncl - n_merges and sorted(set(merged.tolist())) == sorted(order.tolist())
    # edges with an end outside the range, and edges inside a slot, change nothing
    inside = (x < nm) & (m < nm)
    cross = inside & (mc[np.minimum(x, nm - 1)] != mc[np.minimum(m, nm - 1)])
    for kept in (edges[inside], edges[cross]):
        got = ctx.clinkage_merge_from_edges(kept, 0, nm, mc, ids)
        assert np.array_equal(got[0], merged) and np.array_equal(got[1], order) and np.array_equal(ctx.member_rank, rank)
    # members last: the same range behind the extra sequences
    ctx2, res2, off2 = host_ctx(blosum62, extra + peps, np.concatenate([np.ones(7, np.int32), sizes]))
    edges2 = oracle_edges(coracle, blosum62, res2, off2, X, p, thr, True)
    got = ctx2.clinkage_merge_from_edges(edges2, 7, 7 + nm, mc, ids)
    assert np.array_equal(got[0], merged) and np.array_equal(got[1], order) and np.array_equal(ctx2.member_rank, rank)
    # idempotence: the result as the given clusters
    new_ids, mc2 = np.unique(merged[mc], return_inverse=True)
    again, order2 = ctx.clinkage_merge_from_edges(edges, 0, nm, mc2, new_ids)
    assert ctx.last_merge_stats.merges == 0 and np.array_equal(again, new_ids) and len(order2) == len(new_ids)


def test_idempotence_after_clinkage(blosum62, coracle):
    """the result of hmk_clinkage_from_edges fed back as the given clusters merges nothing"""
    rng = np.random.default_rng(77)
    peps = random_peptides(rng, 400, 12, 12, alphabet=5)
    ctx, res, off = host_ctx(blosum62, peps)
    edges = oracle_edges(coracle, blosum62, res, off, 2, 0, 18, True)
    cid, _, stats = ctx.clinkage_from_edges(edges)
    assert stats.merges > 0
    ids, mc = np.unique(cid, return_inverse=True)
    merged, order = ctx.clinkage_merge_from_edges(edges, 0, 400, mc, ids)
    assert ctx.last_merge_stats.merges == 0 and np.array_equal(merged, ids) and len(order) == len(ids)


def test_merge_argument_checks(blosum62, matrices):
    ctx = hammock_amd.Context(blosum62, device=-1)
    ctx.set_sequences(["WVTAPRSLPVLP", "WVTAPRSLPVLA", "RSPIVRQLPSLP", "RSPIVRQLPSLA"])
    none = np.zeros(0, dtype=np.uint64)
    calls = [
        lambda c, *a: c.clinkage_merge_from_edges(none, *a),
        lambda c, *a: c.clinkage_merge(*a, 3, 0, 20),
    ]
    for call in calls:
        for args in (
            (0, 5, [0, 0, 1, 1, 1], [1, 2]),          # range outside [0, n)
            (3, 1, [], [1]),                          # r0 > r1
            (0, 4, [0, 0, 2, 2], [1, 2, 3]),          # slot 1 without member
            (0, 4, [0, 0, 1, 3], [1, 2, 3]),          # slot that does not exist
            (0, 4, [0, 0, 1, 1], [5, 5]),             # duplicate ids
            (0, 4, [0, 0, 1, 1], [0, 5]),             # id 0
            (0, 4, [0, 0, 1, 1], [5, 2 ** 30 + 1]),   # id above 2^30
        ):
            with pytest.raises(ValueError):
                call(ctx, *args)
        with pytest.raises(hammock_amd.ReferenceWouldCrash, match="NoSuchElementException"):
            call(ctx, 2, 2, [], [])                   # zero clusters
    with pytest.raises(ValueError):
        ctx.cluster_pairs_shifted(0, 4, [0, 0, 2, 2], 3, 3, 0, 20)
    # one cluster: returned as it is (the host path needs no device)
    merged, order = ctx.clinkage_merge_from_edges(none, 0, 4, [0, 0, 0, 0], [2 ** 30])
    assert merged.tolist() == [2 ** 30] and order.tolist() == [2 ** 30] and ctx.member_rank.tolist() == [0, 1, 2, 3]
    # the device paths have no CPU fallback
    with pytest.raises(hammock_amd.DeviceError):
        ctx.clinkage_merge(0, 4, [0, 0, 1, 1], [1, 2], 3, 0, 20)
    with pytest.raises(hammock_amd.DeviceError):
        ctx.cluster_pairs_shifted(0, 4, [0, 0, 1, 1], 2, 3, 0, 20)
    asym = blosum62.copy()
    asym[0, 1] += 1
    actx = hammock_amd.Context(asym, device=-1)
    actx.set_sequences(["WVTAPRSLPVLP", "WVTAPRSLPVLA"])
    with pytest.raises(ValueError, match="symmetric"):
        actx.clinkage_merge_from_edges(none, 0, 2, [0, 1], [1, 2])
    with pytest.raises(ValueError, match="symmetric"):
        actx.clinkage_merge(0, 2, [0, 1], [1, 2], 3, 0, 20)
    with pytest.raises(ValueError, match="symmetric"):
        actx.cluster_pairs_shifted(0, 2, [0, 1], 2, 3, 0, 20)


def test_cli_merge_argument_and_format_errors(tmp_path):
    """argument and file-format errors end the program before the device is needed"""
    r = cli("merge", "-d", str(tmp_path / "a"))
    assert r.returncode == 2 and "-i or --input" in r.stderr
    na = tmp_path / "na.tsv"
    na.write_text("cluster_id\tsequence\tno_label\n1\tWVTAPRSLPVLP\t1\nNA\tWVTAPRSLPVLA\t1\n")
    r = cli("merge", "-i", str(na), "--devices", "0,1", "-d", str(tmp_path / "b"))
    assert r.returncode == 2 and "--devices" in r.stderr
    r = cli("merge", "-i", str(na), "--java_hashset", "5", "-d", str(tmp_path / "b2"))
    assert r.returncode == 2 and "--java_hashset" in r.stderr
    r = cli("merge", "-i", str(na), "-d", str(tmp_path / "c"))
    assert r.returncode == 3 and "FileFormatException" in r.stderr
    r = cli("merge", "-i", str(na), "-d", str(tmp_path / "c"))     # the directory exists now
    assert r.returncode == 2 and "Output directory exists" in r.stderr


# ---- GPU ------------------------------------------------------------------------------------------------------------------------

def expected_pairs(coracle, M, res, off, r0, r1, mc, X, p, thr):
    """the feasible slot pairs from the C oracle's score block: block minimum over both slots' members >= thr -> sorted packed pairs,
    and per slot its run length (entries of its members' rows) and the distinct slots next to it"""
    idx = np.arange(r0, r1, dtype=np.uint32)
    order = np.argsort(mc, kind="stable")
    st, blk = coracle.score_block(M, res, off, idx[order], idx[order], 0, X, p)
    assert st == 0
    blk = blk.astype(np.int64)
    np.fill_diagonal(blk, -10 ** 6)
    starts = np.searchsorted(mc[order], np.arange(int(mc.max()) + 1))
    hit = blk >= thr
    run = np.add.reduceat(hit.sum(axis=1), starts)
    near = np.add.reduceat(hit, starts, axis=0)
    near = np.add.reduceat(near, starts, axis=1) > 0
    np.fill_diagonal(near, False)
    np.fill_diagonal(blk, 10 ** 6)   # (a slot's own block does not count: only a < b is read below)
    mn = np.minimum.reduceat(np.minimum.reduceat(blk, starts, axis=0), starts, axis=1)
    a, b = np.nonzero(np.triu(mn >= thr, 1))
    return np.sort(hammock_amd.pack_edges(a, b, mn[a, b])), run, near.sum(axis=1)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["mixed_7_20", "twelve"])
def test_cluster_pairs_against_the_oracle(gpu, blosum62, coracle, shape):
    """~2,000 members in ~600 slots somewhere inside the uploaded set; twice on the resident context"""
    rng = np.random.default_rng(61)
    res, off = synth_peptides(61, 2300, 7, 20) if shape == "mixed_7_20" else synth_peptides(62, 2300, 12)
    r0, r1 = 150, 2150
    mc = relabel(rng.integers(0, 600, size=r1 - r0))
    X, p, thr = 3, (-1 if shape == "mixed_7_20" else 0), 4   # (low: ~10^3 of the 1.8 x 10^5 slot pairs are feasible)
    ctx = hammock_amd.Context(blosum62, device=0)
    ctx.set_sequences(residues=res, offsets=off)
    want, _, _ = expected_pairs(coracle, blosum62, res, off, r0, r1, mc, X, p, thr)
    assert len(want) > 100
    for _ in range(2):
        got = ctx.cluster_pairs_shifted(r0, r1, mc, int(mc.max()) + 1, X, p, thr)
        assert np.array_equal(np.sort(got), want)
        assert ctx.last_merge_stats.cluster_pairs == len(want)
    with pytest.raises(BufferError):
        ctx.cluster_pairs_shifted(r0, r1, mc, int(mc.max()) + 1, X, p, thr, capacity=len(want) - 1)


@pytest.mark.gpu
def test_cluster_pairs_agree_with_match(gpu, blosum62):
    """a two-sided input: n_feasible[b] of hmk_match_clusters_shifted = the returned pairs that join query slot b with an existing
    slot, and every best_cluster entry is one of them"""
    rng = np.random.default_rng(63)
    res, off = synth_peptides(63, 1500, 12)
    nq, nm = 300, 1200
    qc, mc = relabel(rng.integers(0, 120, size=nq)), relabel(rng.integers(0, 400, size=nm))
    nb, nc = int(qc.max()) + 1, int(mc.max()) + 1
    ctx = hammock_amd.Context(blosum62, device=0)
    ctx.set_sequences(residues=res, offsets=off)
    best, _, nf = ctx.match_clusters_shifted(0, nq, qc, nq, nq + nm, mc, np.arange(1, nc + 1), 3, 0, 6, 4)
    pairs = ctx.cluster_pairs_shifted(0, nq + nm, np.concatenate([qc, mc + nb]), nb + nc, 3, 0, 6)
    a, b, _ = hammock_amd.edge_fields(pairs)
    two_sided = (a < nb) & (b >= nb)
    assert nf.sum() > 50 and np.array_equal(np.bincount(a[two_sided], minlength=nb), nf)
    have = set(zip(a[two_sided].tolist(), (b[two_sided] - nb).tolist()))
    for q in range(nb):
        for c in best[q][: min(int(nf[q]), 4)]:
            assert (q, int(c)) in have


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["wave_and_block_overflow", "block", "eight_byte_entries"])
def test_cluster_graph_table_paths(gpu, blosum62, coracle, layout):
    """the table paths of k_merge.hip, forced with low-complexity peptides over three letters (dense rows).
    wave_and_block_overflow: single-sequence slots whose rows hold at most 4,096 entries next to more than 384 distinct slots (a wave,
    its 512-slot table split into classes), and two-member slots with more than 4,096 entries next to more than 1,536 distinct
    slots (a workgroup, its 2,048-slot table split).  block: ten-member slots, more than 4,096 entries, few distinct slots.
    eight_byte_entries: a threshold so low that score - threshold does not fit a byte (8-byte CSR entries)."""
    rng = np.random.default_rng(64)
    if layout == "eight_byte_entries":
        n = 600
        peps = random_peptides(rng, n, 10, 14, alphabet=20)
        mc = relabel(rng.integers(0, 200, size=n))
        X, p, thr = 3, 0, -200
    else:
        n = 4000
        peps = random_peptides(rng, n, 12, 12, alphabet=3)
        mc = relabel(np.concatenate([np.arange(2000), 2000 + np.arange(2000) // 2])) if layout != "block" else relabel(np.arange(n) // 10)
        X, p, thr = 3, 0, None
    res, off = hammock_amd.pack_sequences(peps)
    if thr is None:
        st, sample = coracle.score_block(blosum62, res, off, np.arange(200, dtype=np.uint32), np.arange(200, n, dtype=np.uint32), 0, X, p)
        assert st == 0
        thr = int(np.percentile(sample, 40 if layout != "block" else 5))
    want, run, near = expected_pairs(coracle, blosum62, res, off, 0, n, mc, X, p, thr)
    if layout == "wave_and_block_overflow":
        assert ((run <= 4096) & (near > 384)).sum() > 100 and ((run > 4096) & (near > 1536)).sum() > 100
    elif layout == "block":
        assert (run > 4096).all() and (near <= 1536).all()
    assert len(want) > 100
    ctx = hammock_amd.Context(blosum62, device=0)
    ctx.set_sequences(residues=res, offsets=off)
    got = ctx.cluster_pairs_shifted(0, n, mc, int(mc.max()) + 1, X, p, thr)
    assert np.array_equal(np.sort(got), want)


@pytest.mark.gpu
def test_merge_equals_merge_from_edges(gpu, blosum62):
    """hmk_clinkage_merge (device cluster graph) = hmk_clinkage_merge_from_edges (host cluster graph) on the edges
    hmk_neighbors_shifted returns: family inputs at ~3,000 members, all three Java orders"""
    for seed, (lo, alphabet) in enumerate([(12, 20), (8, 20), (12, 5)]):
        rng = np.random.default_rng(70 + seed)
        peps, mc, sizes = families(rng, 620, lo, 12, alphabet)
        assert len(peps) > 2500
        ncl = int(mc.max()) + 1
        ids = (1000 + rng.permutation(ncl)).astype(np.int32)
        res, off = hammock_amd.pack_sequences(peps)
        ctx = hammock_amd.Context(blosum62, device=0)
        ctx.set_sequences(residues=res, offsets=off, sizes=sizes)
        X, p, thr = 2, -(seed % 2), 20 + 6 * seed
        edges, _ = ctx.neighbors_shifted(X, p, thr)
        for version in (8, 7, 6):
            ctx.set_java_hashset(version)
            want = ctx.clinkage_merge_from_edges(edges, 0, len(peps), mc, ids)
            want_rank, ws = ctx.member_rank.copy(), ctx.last_merge_stats
            assert ws.merges > 50
            got = ctx.clinkage_merge(0, len(peps), mc, ids, X, p, thr)
            gs = ctx.last_merge_stats
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(ctx.member_rank, want_rank)
            assert (gs.merges, gs.searches, gs.n_result_clusters, gs.cluster_pairs, gs.n_edges) == \
                   (ws.merges, ws.searches, ws.n_result_clusters, ws.cluster_pairs, len(edges))


def _golden_set(name):
    if name == "musi":
        seqs = po.load_unique_sequences_from_fasta(os.path.join(GOLDEN, "musi.fa"))
        return [s.get_sequence_string() for s in seqs]
    seen, out = set(), []
    with gzip.open(os.path.join(GOLDEN, "antibodies.fa.gz"), "rt") as fh:
        for line in fh:
            s = line.strip()
            if not s or s.startswith(">") or s in seen:
                continue
            seen.add(s)
            out.append(s)
            if len(out) == 10_000:
                break
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["musi", "antibodies_1e4"])
def test_singleton_seeds_equal_clinkage_cluster(gpu, blosum62, name):
    """slots = the sequences, ids 1 .. n: hmk_clinkage_merge = hmk_clinkage_cluster on MUSI and on the first 10,000 unique sequences
    of the antibodies example"""
    strings = _golden_set(name)
    n = len(strings)
    res, off = hammock_amd.pack_sequences(strings)
    ctx = hammock_amd.Context(blosum62, device=0)
    ctx.set_sequences(residues=res, offsets=off)
    cid, order, stats = ctx.clinkage_cluster(3, 0, 20)
    rank = ctx.member_rank[:n].copy()
    assert stats.merges > 0
    merged, morder = ctx.clinkage_merge(0, n, np.arange(n), np.arange(1, n + 1), 3, 0, 20)
    ms = ctx.last_merge_stats
    assert np.array_equal(merged, cid) and np.array_equal(morder, order) and np.array_equal(ctx.member_rank, rank)
    assert (ms.merges, ms.searches, ms.n_edges, ms.cluster_pairs) == (stats.merges, stats.searches, stats.n_edges, stats.n_edges)


@pytest.mark.gpu
def test_merge_at_scale(gpu, blosum62):
    """greedy on 10^5 synthetic 12-mers (bench.py's set), no oracle.  (i) hmk_clinkage_merge of its multi-member clusters: idempotent
    when the result is fed back; for 200 sampled result clusters every cross pair of their source clusters scores >= threshold, for
    200 sampled pairs of different result clusters at least one cross pair is below it.  (ii) hmk_cluster_pairs_shifted over all its
    clusters: equal as a set on two calls of a resident context; 2,000 sampled slot pairs (half of them drawn from the returned
    pairs) agree with the block minimum by hmk_score_block_shifted.  HMK_ERR_REFERENCE_WOULD_CRASH in (i) fails the test."""
    X, P, THR, n = 3, 0, 20, 100_000
    rng = np.random.default_rng(80)
    res, off = synth_peptides(1, n, 12)
    ctx = hammock_amd.Context(blosum62, device=0)
    ctx.set_sequences(residues=res, offsets=off)
    cid, _, _ = ctx.greedy_cluster(X, P, THR, int(round(0.025 * n)))   # (the CLI's default limit of initial clusters, as bench.py's call)
    ids_all, mc_all, counts = np.unique(cid, return_inverse=True, return_counts=True)

    # (ii) every cluster, the whole set
    ncl = len(ids_all)
    pairs = ctx.cluster_pairs_shifted(0, n, mc_all, ncl, X, P, THR)
    again = ctx.cluster_pairs_shifted(0, n, mc_all, ncl, X, P, THR)
    assert len(pairs) > 1000 and np.array_equal(np.sort(pairs), np.sort(again))
    a, b, sc = hammock_amd.edge_fields(pairs)
    assert (a < b).all()
    members_of = np.split(np.argsort(mc_all, kind="stable"), np.cumsum(counts)[:-1])
    known = dict(zip(zip(a.tolist(), b.tolist()), sc.tolist()))
    pick = rng.choice(len(pairs), size=1000, replace=False)
    sample = [(int(a[k]), int(b[k])) for k in pick]
    while len(sample) < 2000:
        u, v = sorted(rng.integers(0, ncl, size=2).tolist())
        if u != v:
            sample.append((u, v))

    def block_min(u, v):
        worst = 10 ** 6
        for i in members_of[u]:
            for j in members_of[v]:
                worst = min(worst, int(ctx.score_block_shifted(int(i), int(i) + 1, int(j), int(j) + 1, X, P)[0, 0]))
        return worst

    for u, v in sample:
        mn = block_min(u, v)
        assert (known.get((u, v)) == mn) if mn >= THR else ((u, v) not in known), (u, v, mn)

    # (i) the multi-member clusters: move their members to the front of a second upload
    multi = np.flatnonzero(counts > 1)
    keep = np.flatnonzero(counts[mc_all] > 1)
    assert len(multi) > 1500 and len(keep) > 5000
    mc = relabel(mc_all[keep])
    ids = (1 + np.arange(len(multi))).astype(np.int32)
    sub_res = res.reshape(n, 12)[keep].ravel()
    sub_off = (np.arange(len(keep) + 1) * 12).astype(np.uint32)
    sub = hammock_amd.Context(blosum62, device=0)
    sub.set_sequences(residues=sub_res, offsets=sub_off)
    merged, order = sub.clinkage_merge(0, len(keep), mc, ids, X, P, THR)
    merges = sub.last_merge_stats.merges
    assert len(order) == len(ids) - merges   # (greedy's own multi-member clusters may well hold nothing to merge: nothing is asserted on it)
    new_ids, mc2 = np.unique(merged[mc], return_inverse=True)
    fed_back, _ = sub.clinkage_merge(0, len(keep), mc2, new_ids, X, P, THR)
    assert sub.last_merge_stats.merges == 0 and np.array_equal(fed_back, new_ids)
    sources = {}
    for slot, rid in enumerate(merged.tolist()):
        sources.setdefault(rid, []).append(slot)
    slot_members = np.split(np.argsort(mc, kind="stable"), np.cumsum(np.bincount(mc))[:-1])

    def cross_scores(u, v):
        i = np.repeat(slot_members[u], len(slot_members[v]))
        j = np.tile(slot_members[v], len(slot_members[u]))
        return sub.score_pairs_shifted(i, j, X, P)

    grown = [r for r, s in sources.items() if len(s) > 1]
    for r in (rng.choice(grown, size=min(200, len(grown)), replace=False).tolist() if grown else []):
        s = sources[r]
        for x in range(len(s)):
            for y in range(x + 1, len(s)):
                assert cross_scores(s[x], s[y]).min() >= THR
    rids = list(sources)
    for _ in range(200):
        r1, r2 = rng.choice(len(rids), size=2, replace=False).tolist()
        worst = min(cross_scores(u, v).min() for u in sources[rids[r1]] for v in sources[rids[r2]])
        assert worst < THR


# ---- CLI on the GPU ---------------------------------------------------------------------------------------------------------------

def read_merged(path):
    rows = [l.split("\t") for l in open(path).read().splitlines()]
    assert rows[0] == ["source_file", "source_cluster_id", "cluster_id", "merged"]
    return [(f[0], int(f[1]), int(f[2]), int(f[3])) for f in rows[1:]]


@pytest.mark.gpu
def test_cli_merge_two_greedy_runs(gpu, tmp_path):
    """greedy on two halves of musi.fa, merge of the two outputs: merged_clusters.tsv is consistent with the stage-1 files, the -i
    file's clusters are renumbered behind the --clusters file's, the output loads back (match of the output against itself matches
    every cluster to itself) and merging the output again merges nothing"""
    with open(os.path.join(GOLDEN, "musi.fa")) as fh:
        lines = fh.read().splitlines()
    records = [lines[k:k + 2] for k in range(0, len(lines), 2)]
    files = []
    for half in (0, 1):
        fa = tmp_path / f"h{half}.fa"
        fa.write_text("\n".join(l for i, r in enumerate(records) if i % 2 == half for l in r) + "\n")
        r = cli("greedy", "-i", str(fa), "-d", str(tmp_path / f"g{half}"), "-x", "3", "-g", "20", timeout=600)
        assert r.returncode == 0, r.stderr
        files.append(tmp_path / f"g{half}" / "initial_clusters_sequences.tsv")
    a, b = read_cluster_file(files[0]), read_cluster_file(files[1])
    shared = {s for _, s, _ in a} & {s for _, s, _ in b}
    r = cli("merge", "-i", str(files[1]), "--clusters", str(files[0]), "-d", str(tmp_path / "m"), "-x", "3", "-g", "20", timeout=600)
    assert r.returncode == 0, r.stderr
    assert f"{len(shared)} sequences of the input file were already in the cluster file" in r.stderr
    merges = int(re.search(r"merges: (\d+)", r.stderr).group(1))
    assert merges > 0
    out = read_cluster_file(tmp_path / "m" / "initial_clusters_sequences.tsv")
    rows = read_merged(tmp_path / "m" / "merged_clusters.tsv")
    ids_a = list(dict.fromkeys(c for c, _, _ in a))
    ids_b = list(dict.fromkeys(c for c, _, _ in b))
    assert [(f, i) for f, i, _, _ in rows if f == str(files[0])] == [(str(files[0]), c) for c in ids_a]
    kept_b = [c for c in ids_b if any(s not in shared for cc, s, _ in b if cc == c)]
    assert [i for f, i, _, _ in rows if f == str(files[1])] == kept_b
    # every sequence once, with the counts of both files; a given cluster's sequences sit in the cluster its row names
    assert sorted(s for _, s, _ in out) == sorted({s for _, s, _ in a} | {s for _, s, _ in b})
    size = {}
    for _, s, z in a + b:
        size[s] = size.get(s, 0) + z
    where = {s: c for c, s, _ in out}
    assert all(z == size[s] for _, s, z in out)
    top = max(ids_a)
    final = {(f, i): (c, m) for f, i, c, m in rows}
    for f, src in ((str(files[0]), a), (str(files[1]), b)):
        for c, s, _ in src:
            if f == str(files[1]) and s in shared:
                continue
            assert where[s] == final[(f, c)][0]
    assert len(set(where.values())) == len(rows) - merges
    unmerged_b = [(i, c) for f, i, c, m in rows if f == str(files[1]) and m == 0]
    assert all(c == top + 1 + ids_b.index(i) for i, c in unmerged_b)          # renumbered max + 1 + k in file order
    merged_ids = {c for _, _, c, m in rows if m}
    assert len(merged_ids) > 0 and min(merged_ids) > max([top] + [c for _, _, c, m in rows if not m])
    # loads back: every cluster matches itself and nothing else (what a finished merge leaves apart is infeasible), and a second
    # merge merges nothing
    mfile = str(tmp_path / "m" / "initial_clusters_sequences.tsv")
    r = cli("match", "-i", mfile, "--clusters", mfile, "-d", str(tmp_path / "mm"), "-x", "3", "-g", "20", timeout=600)
    assert r.returncode == 0, r.stderr
    hits = [l.split("\t") for l in (tmp_path / "mm" / "cluster_matches.tsv").read_text().splitlines()[1:]]
    assert sorted(int(f[0]) for f in hits) == sorted(set(where.values()))
    assert all(f[2] == f[0] and f[5] == "1" for f in hits)
    r = cli("merge", "-i", mfile, "-d", str(tmp_path / "m2"), "-x", "3", "-g", "20", timeout=600)
    assert r.returncode == 0 and "merges: 0," in r.stderr, r.stderr
    assert sorted(read_cluster_file(tmp_path / "m2" / "initial_clusters_sequences.tsv")) == sorted(out)


@pytest.mark.gpu
def test_cli_merge_duplicate_sequences(gpu, tmp_path):
    """a hand-made pair of files: a sequence present in both stays in its --clusters cluster with both lines' counts, leaves its -i
    cluster, and an -i cluster that becomes empty disappears; --skip_singletons writes single-sequence clusters through"""
    first, second = tmp_path / "first.tsv", tmp_path / "second.tsv"
    first.write_text("cluster_id\tsequence\tx\n3\tWVTAPRSLPVLP\t2\n3\tWVTAPRSLPVLA\t1\n9\tGGGGGGGGGGGG\t1\n")
    second.write_text("cluster_id\tsequence\ty\n1\tWVTAPRSLPVLA\t5\n2\tWVTAPRSLPVLG\t1\n2\tWVTAPRSLPVLP\t4\n7\tCCCCCCCCCCCC\t1\n")
    r = cli("merge", "-i", str(second), "--clusters", str(first), "-d", str(tmp_path / "m"), "-x", "3", "-g", "20", timeout=600)
    assert r.returncode == 0, r.stderr
    assert "2 sequences of the input file were already in the cluster file" in r.stderr and "(1 input clusters became empty)" in r.stderr
    rows = read_merged(tmp_path / "m" / "merged_clusters.tsv")
    # slots: 3, 9 of the first file; 2 -> 11 and 7 -> 12 of the second (1 -> 10 became empty); {3, 11} merge into 12 + 2
    assert rows == [(str(first), 3, 14, 1), (str(first), 9, 9, 0), (str(second), 2, 14, 1), (str(second), 7, 12, 0)]
    out = {s: (c, z) for c, s, z in read_cluster_file(tmp_path / "m" / "initial_clusters_sequences.tsv")}
    assert out == {"WVTAPRSLPVLP": (14, 6), "WVTAPRSLPVLA": (14, 6), "WVTAPRSLPVLG": (14, 1), "GGGGGGGGGGGG": (9, 1), "CCCCCCCCCCCC": (12, 1)}
    r = cli("merge", "-i", str(second), "--clusters", str(first), "--skip_singletons", "-d", str(tmp_path / "s"), "-x", "3", "-g", "20", timeout=600)
    assert r.returncode == 0, r.stderr
    # candidates: 3 (two sequences) alone -- 11 holds one sequence after the duplicate left it: nothing merges
    assert read_merged(tmp_path / "s" / "merged_clusters.tsv") == [(str(first), 3, 3, 0), (str(first), 9, 9, 0), (str(second), 2, 11, 0),
                                                                     (str(second), 7, 12, 0)]
