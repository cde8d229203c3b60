"""Assignment of new sequences to existing clusters (hmk_assign_shifted / hmk_assign_local, Context.assign_*, the CLI's `assign`
mode): new sequences [q0, q1) against the frozen clusters of the members [r0, r1) of one uploaded set, complete linkage with
score(m, x) = sequenceScore(seq1 = member, seq2 = new) -- the orientation of ClinkageSequenceClusterer.java:263, the opposite of
the search's.  Expectations come from oracle.c_oracle.score_block (rows = members = seq1, columns = new sequences) and numpy,
cross-checked on small cases against a literal restatement of NearestClusterRunner.call + findNearestClusterParallel.
The CPU tests run anywhere; the GPU tests need an MI355X (-m gpu)."""
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
NEW_SYMBOLS = ("hmk_assign_shifted", "hmk_assign_local")
ALPHABET = "ARNDCQEGHILKMFPSTWYVBZX*"
INT_MIN = -2 ** 31
NONE = 0xFFFFFFFF


def _blosum62():
    with open(os.path.join(GOLDEN, "matrices.json")) as fh:
        return np.asarray(json.load(fh)["matrices"]["blosum62"], dtype=np.int32)


def asymmetric(M):
    rng = np.random.default_rng(5)     # the matrix of test_gpu_parity.py::test_neighbors_asymmetric_matrix
    M = M.copy()
    M[np.triu_indices(24, 1)] += rng.integers(-2, 3, size=276).astype(np.int32)
    return M


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


# ---- the expectation -----------------------------------------------------------------------------------------------------

def expected(blk, member_cluster, cluster_id, member_sizes, thr, k):
    """blk[m, x] = score(seq1 = member m, seq2 = new x) -> (best_cluster uint32[nq, k], best_score int32[nq, k], n_feasible[nq]):
    cluster c feasible for x iff every member scores >= thr, its score the minimum; ranked by score desc, size desc, id asc"""
    blk = np.asarray(blk, dtype=np.int64)
    nm, nq = blk.shape
    nc = len(cluster_id)
    mc = np.asarray(member_cluster, dtype=np.int64)
    ids = np.asarray(cluster_id, dtype=np.int64)
    size = np.bincount(mc, weights=np.asarray(member_sizes, dtype=np.float64), minlength=nc).astype(np.int64)
    best = np.full((nq, k), NONE, dtype=np.uint32)
    score = np.full((nq, k), INT_MIN, dtype=np.int32)
    if nc == 0 or nq == 0:
        return best, score, np.zeros(nq, dtype=np.uint32)
    order = np.argsort(mc, kind="stable")
    starts = np.searchsorted(mc[order], np.arange(nc))
    mn = np.minimum.reduceat(blk[order], starts, axis=0)            # [nc, nq]
    feas = mn >= thr
    rank = np.empty(nc, dtype=np.int64)
    rank[np.lexsort((ids, -size))] = np.arange(nc)                   # size desc, id asc
    key = np.where(feas, mn * (nc + 1) + (nc - rank)[:, None], -2 ** 62)   # larger = better
    top = np.argsort(-key, axis=0, kind="stable")[:k]               # [k', nq]
    for t in range(top.shape[0]):
        c = top[t]
        ok = feas[c, np.arange(nq)]
        best[ok, t] = c[ok]
        score[ok, t] = mn[c[ok], np.arange(nq)[ok]]
    return best, score, feas.sum(axis=0).astype(np.uint32)


class JCluster:
    def __init__(self, members, cid, size):
        self.members, self.id, self._size = members, cid, size

    def size(self):
        return self._size


def java_nearest(clusters, x, score, thr, parts=1):
    """ClinkageClusterScorer.clusterScore(i, compared) (early exit) + NearestClusterRunner.call over `parts` parts +
    findNearestClusterParallel's fold from MIN_VALUE + 42; -> the cluster LimitedGreedy :59-66 accepts, or None"""
    def cluster_score(cl):
        result = 2 ** 31 - 1
        for m in cl.members:
            r = score(m, x)
            if r < result:
                result = r
                if result < thr:
                    return INT_MIN + 1
        return result

    def runner(part):
        max_score, nearest = INT_MIN, None
        for i in part:
            s = cluster_score(i)
            if s < max_score:
                continue
            if s > max_score:
                max_score, nearest = s, i
            elif i.size() > nearest.size() or (i.size() == nearest.size() and i.id < nearest.id):
                nearest = i
        return nearest, max_score

    if not clusters:
        return None
    max_score, nearest = INT_MIN + 42, None
    for p in range(parts):
        cur, s = runner(clusters[p::parts])
        if s < max_score:
            continue
        if s > max_score:
            nearest, max_score = cur, s
        elif cur.size() > nearest.size() or (cur.size() == nearest.size() and cur.id < nearest.id):
            nearest = cur
    if nearest is not None and max_score >= thr:
        return nearest, max_score
    return None


def cross_check(blk, member_cluster, cluster_id, member_sizes, thr, best, score, n_xs=40):
    """rank 1 of the numpy expectation against the literal restatement, on the first n_xs new sequences"""
    nc = len(cluster_id)
    mc = np.asarray(member_cluster)
    clusters = [JCluster(list(np.nonzero(mc == c)[0]), int(cluster_id[c]), int(np.asarray(member_sizes)[mc == c].sum()))
                for c in range(nc)]
    slot = {id(cl): c for c, cl in enumerate(clusters)}
    for x in range(min(n_xs, blk.shape[1])):
        for parts in (1, 3):
            got = java_nearest(clusters, x, lambda m, xx: int(blk[m, xx]), thr, parts)
            if got is None:
                assert best[x, 0] == NONE
            else:
                assert (slot[id(got[0])], got[1]) == (best[x, 0], score[x, 0])


# ---- fixtures of sequences -------------------------------------------------------------------------------------------------

def mutate(rng, p, n_sub, trim=False):
    q = p.copy()
    for pos in rng.choice(len(q), size=n_sub, replace=False):
        q[pos] = rng.integers(0, 20)
    if trim and rng.random() < 0.3:
        q = q[1:] if rng.random() < 0.5 else q[:-1]
    return q


def families(rng, n_members, n_new, len_lo, len_hi, max_cluster=6, trim=False):
    """members in clusters around random centres (several clusters per centre, 1..max_cluster members each), new sequences
    that are mutants of those centres or random -> (members, member_cluster, new)"""
    members, mc, new = [], [], []
    centres = []
    while len(members) < n_members:
        L = int(rng.integers(len_lo, len_hi + 1))
        centre = rng.integers(0, 20, size=L).astype(np.uint8)
        centres.append(centre)
        for _ in range(int(rng.integers(1, 4))):
            c = int(mc[-1]) + 1 if mc else 0
            for _ in range(int(rng.integers(1, max_cluster + 1))):
                members.append(mutate(rng, centre, int(rng.integers(0, 3)), trim))
                mc.append(c)
    for _ in range(n_new):
        if rng.random() < 0.8:
            new.append(mutate(rng, centres[int(rng.integers(len(centres)))], int(rng.integers(0, 3)), trim))
        else:
            new.append(rng.integers(0, 20, size=int(rng.integers(len_lo, len_hi + 1))).astype(np.uint8))
    return members[:n_members], np.asarray(mc[:n_members], dtype=np.int64), new


def relabel(mc):
    """cluster slots 0..nc-1 in order of first appearance (a truncated family may have dropped a slot)"""
    _, inv = np.unique(mc, return_inverse=True)
    return inv.astype(np.uint32)


def setup(M, new, members, member_cluster, rng, new_first=True):
    """one uploaded set: new + members (or members + new) with random member sizes; -> ctx, res, off, q-range, r-range, ids,
    member sizes"""
    nq, nm = len(new), len(members)
    msizes = rng.integers(1, 6, size=nm).astype(np.int32)
    if new_first:
        seqs, sizes, qr, rr = new + members, np.concatenate([np.ones(nq, np.int32), msizes]), (0, nq), (nq, nq + nm)
    else:
        seqs, sizes, qr, rr = members + new, np.concatenate([msizes, np.ones(nq, np.int32)]), (nm, nm + nq), (0, nm)
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


def check(got, want):
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(got[2], want[2])


# ---- CPU ---------------------------------------------------------------------------------------------------------------------

def test_assign_symbols_in_header_symbols_and_library():
    with open(os.path.join(ROOT, "include", "hammock_hip.h")) as fh:
        header = fh.read()
    for name in NEW_SYMBOLS:
        assert f"int {name}(" in header
        assert name in N.SYMBOLS
        assert hasattr(N.lib, name)
    assert N.lib.hmk_abi_version() == 4


def test_assign_argument_errors_on_a_host_only_context():
    ctx = hammock_amd.Context(_blosum62(), device=-1)
    ctx.set_sequences(["ACDEFGHIK", "ACDEFGHIKL", "MNPQRSTVW", "WYVACDEFG", "KLMNPQRST"])
    good = dict(member_cluster=[0, 1, 1], cluster_id=[5, 9])
    for fn, a, b in ((ctx.assign_shifted, 2, 0), (ctx.assign_local, -5, -1)):
        for q0, q1, r0, r1 in ((0, 2, 1, 4), (2, 5, 0, 3), (0, 2, 3, 6), (3, 2, 0, 1)):
            with pytest.raises(ValueError):
                fn(q0, q1, r0, r1, [0] * max(r1 - r0, 0), [1], a, b, 10)
        for k in (0, 33):
            with pytest.raises(ValueError):
                fn(0, 2, 2, 5, good["member_cluster"], good["cluster_id"], a, b, 10, k)
        with pytest.raises(ValueError):          # a member_cluster value >= n_clusters
            fn(0, 2, 2, 5, [0, 2, 1], [5, 9], a, b, 10)
        with pytest.raises(ValueError):          # slot 1 has no member
            fn(0, 2, 2, 5, [0, 0, 2], [5, 9, 4], a, b, 10)
        with pytest.raises(ValueError):          # duplicate ids
            fn(0, 2, 2, 5, [0, 1, 2], [5, 9, 5], a, b, 10)
    # the raw status is HMK_ERR_BAD_ARG
    mc = np.array([0, 1, 1], dtype=np.uint32)
    cid = np.array([5, 5], dtype=np.int32)
    out = np.empty(4, dtype=np.uint32)
    sc = np.empty(4, dtype=np.int32)
    st = N.lib.hmk_assign_shifted(ctx._h, 0, 2, 2, 5, mc.ctypes.data_as(C.POINTER(C.c_uint32)), cid.ctypes.data_as(C.POINTER(C.c_int32)), 2,
                                  2, 0, 10, 2, out.ctypes.data_as(C.POINTER(C.c_uint32)), sc.ctypes.data_as(C.POINTER(C.c_int32)),
                                  out.ctypes.data_as(C.POINTER(C.c_uint32)), None)
    assert st == N.HMK_ERR_BAD_ARG
    # valid arguments reach the device check: no CPU fallback
    with pytest.raises(hammock_amd.DeviceError):
        ctx.assign_shifted(0, 2, 2, 5, [0, 1, 1], [5, 9], 2, 0, 10)
    with pytest.raises(hammock_amd.DeviceError):
        ctx.assign_local(3, 5, 0, 3, [1, 0, 1], [5, 9], -5, -1, 10, k=32)


def cli(*args, **kw):
    return subprocess.run([CLI, *args], capture_output=True, text=True, **kw)


def test_cli_assign_needs_clusters(tmp_path):
    r = cli("assign", "-i", os.path.join(GOLDEN, "musi.fa"), "-d", str(tmp_path / "out"))
    assert r.returncode == 2
    assert "--clusters" in r.stderr
    assert not (tmp_path / "out").exists()


def test_cli_assign_rejects_devices(tmp_path):
    fa = os.path.join(GOLDEN, "musi.fa")
    r = cli("assign", "-i", fa, "--clusters", fa, "-d", str(tmp_path / "out"), "--devices", "0,1")
    assert r.returncode == 2
    assert not (tmp_path / "out").exists()


def test_cli_help_names_assign():
    r = cli("--help")
    assert r.returncode == 0
    assert "assign" in r.stderr and "--clusters" in r.stderr and "--skip_singletons" in r.stderr and "--best" in r.stderr


def _cluster_file_expectation(path):
    """the Python restatement of loadClusterDetailsFromCsv (FileIOManager.java:304-365): [(id, sequence, size)] per line"""
    with open(path) as fh:
        lines = fh.read().splitlines()
    header = lines[0].split("\t")
    ai = header.index("alignment") if "alignment" in header else -1
    if ai != -1:
        header.pop(ai)
    si = header.index("sum") if "sum" in header else -1
    if si != -1:
        header.pop(si)
    out = []
    for line in lines[1:]:
        f = line.split("\t")
        if ai != -1:
            f.pop(ai)
        if si != -1:
            f.pop(si)
        out.append((int(f[0]), f[1], sum(int(v) for v in f[2:])))
    return out


@pytest.mark.parametrize("fasta", ["manual_example.fa", "musi.fa"])
def test_cluster_file_loader_round_trip(tmp_path, fasta):
    """clusters written by the existing writers (io-selftest writers: labels, `sum` and `alignment` columns) load back with the
    same ids, members and sizes"""
    import random
    from oracle import hammock_oracle as po
    fa = os.path.join(GOLDEN, fasta)
    seqs = po.load_unique_sequences_from_fasta(fa)
    names = [s.get_sequence_string() for s in seqs]
    size_of = {s.get_sequence_string(): s.size() for s in seqs}
    rnd = random.Random(3)
    rnd.shuffle(names)
    spec, at = [], 0
    ids = rnd.sample(range(10, 100000), len(names))
    while at < len(names):
        k = rnd.randint(1, 4)
        spec.append((ids[len(spec)], names[at:at + k]))
        at += k
    (tmp_path / "clusters.tsv").write_text("".join(f"{cid}\t{','.join(m)}\n" for cid, m in spec))
    out = tmp_path / "out"
    for sub in ("serial", "side"):
        (out / sub).mkdir(parents=True)
    r = cli("io-selftest", "writers", "fasta", fa, "size", "42", str(tmp_path / "clusters.tsv"), str(out))
    assert r.returncode == 0, r.stderr
    want = sorted((cid, m, size_of[m]) for cid, members in spec for m in members)
    for name in ("initial_clusters_sequences.tsv", "initial_clusters_sequences_original_order.tsv"):
        path = out / "serial" / name
        assert "alignment" in path.read_text().splitlines()[0] and "sum" in path.read_text().splitlines()[0]
        r = cli("io-selftest", "clusters", str(path))
        assert r.returncode == 0, r.stderr
        got = [tuple(l.split("\t")) for l in r.stdout.splitlines()]
        got = sorted((int(a), b, int(c)) for a, b, c in got)
        assert got == want
        assert sorted(_cluster_file_expectation(path)) == want


def test_cluster_file_loader_rejects_malformed_and_na(tmp_path):
    good = "cluster_id\tsequence\talignment\tsum\tl1\tl2\n3\tWVTAPRSLPVLP\tNA\t3\t1\t2\n3\tGSWVVDISNVED\tNA\t1\t0\t1\n"
    (tmp_path / "good.tsv").write_text(good)
    r = cli("io-selftest", "clusters", str(tmp_path / "good.tsv"))
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines() == ["3\tWVTAPRSLPVLP\t3", "3\tGSWVVDISNVED\t1"]
    bad = {
        "na": good + "NA\tNYSGNRPLPGIW\tNA\t1\t1\t0\n",
        "count": good.replace("\t1\t2\n", "\tx\t2\n"),
        "short": good + "4\n",
        "letter": good + "5\tNYSGN1PLPGIW\tNA\t1\t1\t0\n",
    }
    for name, text in bad.items():
        p = tmp_path / f"{name}.tsv"
        p.write_text(text)
        r = cli("io-selftest", "clusters", str(p))
        assert r.returncode == 3, (name, r.returncode, r.stderr)
        out = tmp_path / f"out_{name}"
        r = cli("assign", "-i", os.path.join(GOLDEN, "musi.fa"), "--clusters", str(p), "-d", str(out), timeout=120)
        assert r.returncode == 3, (name, r.returncode, r.stderr)
        assert "FileFormatException" in (out / "run.log").read_text()


# ---- GPU ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 5, 32])
def test_assign_uniform_12mers(gpu, coracle, k):
    M = _blosum62()
    rng = np.random.default_rng(100 + k)
    members, mc, new = families(rng, 3000, 2000, 12, 12)
    mc = relabel(mc)
    for new_first in (True, False):
        ctx, res, off, qr, rr, ids, msz = setup(M, new, members, mc, rng, new_first)
        blk = block(coracle, M, res, off, qr, rr, 0, 3, 0)
        want = expected(blk, mc, ids, msz, 30, k)
        assert (want[2] > 0).mean() > 0.3 and (want[2] == 0).any()
        if k > 1:
            assert (want[2] > 1).any()
        got = ctx.assign_shifted(*qr, *rr, mc, ids, 3, 0, 30, k)
        check(got, want)
        cross_check(blk, mc, ids, msz, 30, want[0], want[1])
        st = ctx.last_assign_stats
        assert st.pairs_scored == len(new) * len(members) and st.n_edges == int((blk >= 30).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("X", [2, 3])
def test_assign_mixed_lengths(gpu, coracle, X):
    M = _blosum62()
    rng = np.random.default_rng(200 + X)
    members, mc, new = families(rng, 2500, 1500, 8, 16, trim=True)
    mc = relabel(mc)
    ctx, res, off, qr, rr, ids, msz = setup(M, new, members, mc, rng)
    blk = block(coracle, M, res, off, qr, rr, 0, X, -1)
    want = expected(blk, mc, ids, msz, 24, 4)
    assert (want[2] > 0).any()
    check(ctx.assign_shifted(*qr, *rr, mc, ids, X, -1, 24, 4), want)
    cross_check(blk, mc, ids, msz, 24, want[0], want[1])


@pytest.mark.gpu
def test_assign_asymmetric_matrix_orientation(gpu, coracle):
    """score(seq1 = member, seq2 = new): there are new sequences whose answer differs under the swapped orientation"""
    M = asymmetric(_blosum62())
    rng = np.random.default_rng(7)
    members, mc, new = families(rng, 2000, 1500, 10, 13, trim=True)
    mc = relabel(mc)
    for new_first in (True, False):
        ctx, res, off, qr, rr, ids, msz = setup(M, new, members, mc, rng, new_first)
        blk = block(coracle, M, res, off, qr, rr, 0, 3, -1)
        st, swapped = coracle.score_block(M, res, off, np.arange(*qr), np.arange(*rr), 0, 3, -1)
        assert st == 0
        want = expected(blk, mc, ids, msz, 26, 3)
        other = expected(swapped.T, mc, ids, msz, 26, 3)
        differ = np.any(want[0] != other[0], axis=1) | (want[2] != other[2])
        assert differ.sum() > 0
        got = ctx.assign_shifted(*qr, *rr, mc, ids, 3, -1, 26, 3)
        assert ctx.last_assign_stats.symmetric == 0
        check(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("gaps,thr", [((-5, -1), 30), ((1, 1), None)], ids=["striped", "literal"])
def test_assign_local(gpu, coracle, gaps, thr):
    M = _blosum62()
    rng = np.random.default_rng(300)
    members, mc, new = families(rng, 1200, 800, 9, 15, trim=True)
    mc = relabel(mc)
    for new_first in (True, False):
        ctx, res, off, qr, rr, ids, msz = setup(M, new, members, mc, rng, new_first)
        blk = block(coracle, M, res, off, qr, rr, 1, gaps[0], gaps[1])
        thr = thr if thr is not None else int(np.percentile(blk, 97))   # (positive gap scores lift every pair)
        want = expected(blk, mc, ids, msz, thr, 3)
        assert (want[2] > 0).any() and (want[2] == 0).any()
        check(ctx.assign_local(*qr, *rr, mc, ids, gaps[0], gaps[1], thr, 3), want)
        cross_check(blk, mc, ids, msz, thr, want[0], want[1])


@pytest.mark.gpu
def test_assign_ties(gpu):
    """equal scores: the larger cluster first; equal score and size: the smaller id first -- in both slot orders"""
    M = _blosum62()
    x, s = "WVTAPRSLPVLP", "WVTAPRSLPVLA"
    ctx = hammock_amd.Context(M, device=0)
    sizes = [1, 2, 3, 3, 1, 2]            # x, then five copies of s
    ctx.set_sequences([x, s, s, s, s, s], sizes=sizes)
    score = int(ctx.score_pairs_shifted([1], [0], 3, 0)[0])
    blk = np.full((5, 1), score, dtype=np.int32)
    cases = [([0, 1, 2, 3, 3], [40, 30, 20, 10], [3, 2, 1, 0]),     # sizes 2, 3, 3, 3: slot 0 last, the rest by id
             ([0, 1, 2, 3, 3], [10, 20, 30, 40], [1, 2, 3, 0]),
             ([0, 1, 2, 3, 3], [5, 9, 7, 50], [2, 1, 3, 0]),
             ([3, 2, 1, 0, 0], [10, 20, 30, 40], [0, 1, 2, 3]),     # the slot order reversed: sizes 3, 3, 3, 2
             ([3, 2, 1, 0, 0], [40, 30, 20, 10], [2, 1, 0, 3])]
    for mc, ids, want_order in cases:
        best, sc, nf = ctx.assign_shifted(0, 1, 1, 6, mc, ids, 3, 0, 10, 4)
        assert list(best[0]) == want_order and nf[0] == 4 and list(sc[0]) == [score] * 4
        want = expected(blk, mc, ids, sizes[1:], 10, 4)
        check((best, sc, nf), want)
        cross_check(blk, mc, ids, sizes[1:], 10, want[0], want[1])
        best, sc, nf = ctx.assign_shifted(0, 1, 1, 6, mc, ids, 3, 0, 10, 1)
        assert list(best[0]) == want_order[:1]


@pytest.mark.gpu
def test_assign_table_overflow(gpu, coracle):
    """runs of at most 4,096 hits (a wave each) that touch more than 384 distinct clusters -- 3/4 of the wave's 512-slot
    table: the clusters are taken in 2, 4, ... classes by rank, one table fill per class"""
    M = _blosum62()
    rng = np.random.default_rng(11)
    res0, off0 = synth_peptides(41, 3040, 12)
    seqs = [np.asarray(res0[off0[i]:off0[i + 1]]) for i in range(3040)]
    new, members = seqs[:40], seqs[40:]
    mc = np.repeat(np.arange(2000), [1 if i % 2 else 2 for i in range(2000)])[:3000]
    mc = relabel(mc)
    ctx, res, off, qr, rr, ids, msz = setup(M, new, members, mc, rng)
    blk = block(coracle, M, res, off, qr, rr, 0, 3, 0)
    thr = int(np.percentile(blk, 40))
    hits = (blk >= thr).sum(axis=0)
    distinct = np.array([len(np.unique(mc[blk[:, x] >= thr])) for x in range(len(new))])
    assert hits.max() <= 4096 and distinct.min() > 384
    for k in (1, 32):
        want = expected(blk, mc, ids, msz, thr, k)
        assert want[2].min() > 32
        check(ctx.assign_shifted(*qr, *rr, mc, ids, 3, 0, thr, k), want)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["few_clusters", "many_clusters"])
def test_assign_long_runs(gpu, coracle, layout):
    """runs of more than 4,096 hits: a workgroup each.  many_clusters: more than 1,536 distinct clusters per run, 3/4 of
    the workgroup's 2,048-slot table, so the workgroup splits them into classes too"""
    M = _blosum62()
    rng = np.random.default_rng(12)
    res0, off0 = synth_peptides(42, 6030, 12)
    seqs = [np.asarray(res0[off0[i]:off0[i + 1]]) for i in range(6030)]
    new, members = seqs[:30], seqs[30:]
    per = 10 if layout == "few_clusters" else 2
    mc = relabel(np.arange(6000) // per)
    ctx, res, off, qr, rr, ids, msz = setup(M, new, members, mc, rng)
    blk = block(coracle, M, res, off, qr, rr, 0, 3, 0)
    thr = int(np.percentile(blk, 5))
    hits = (blk >= thr).sum(axis=0)
    assert hits.min() > 4096
    if layout == "many_clusters":
        assert min(len(np.unique(mc[blk[:, x] >= thr])) for x in range(len(new))) > 1536
    for k in (1, 32):
        want = expected(blk, mc, ids, msz, thr, k)
        assert want[2].min() > 0
        check(ctx.assign_shifted(*qr, *rr, mc, ids, 3, 0, thr, k), want)


@pytest.mark.gpu
@pytest.mark.parametrize("nq,nm", [(5, 50000), (50000, 12)])
def test_assign_skewed_shapes(gpu, coracle, nq, nm):
    M = _blosum62()
    rng = np.random.default_rng(nq)
    res0, off0 = synth_peptides(21, nq + nm, 12)
    seqs = [np.asarray(res0[off0[i]:off0[i + 1]]) for i in range(nq + nm)]
    new, members = seqs[:nq], seqs[nq:]
    mc = relabel(rng.integers(0, max(nm // 3, 1), size=nm)) if nm > 100 else np.arange(nm, dtype=np.uint32) // 3
    ctx, res, off, qr, rr, ids, msz = setup(M, new, members, mc, rng)
    blk = block(coracle, M, res, off, qr, rr, 0, 3, 0)
    thr = int(np.percentile(blk, 80))
    want = expected(blk, mc, ids, msz, thr, 5)
    assert (want[2] > 0).any()
    check(ctx.assign_shifted(*qr, *rr, mc, ids, 3, 0, thr, 5), want)


@pytest.mark.gpu
def test_assign_empty_ranges(gpu):
    M = _blosum62()
    res, off = synth_peptides(4, 100, 12)
    ctx = hammock_amd.Context(M, device=0)
    ctx.set_sequences(residues=res, offsets=off)
    best, sc, nf = ctx.assign_shifted(0, 0, 10, 20, np.arange(10) // 2, np.arange(5), 3, 0, 20, 3)
    assert best.shape == (0, 3) and sc.shape == (0, 3) and nf.shape == (0,)
    best, sc, nf = ctx.assign_shifted(0, 10, 10, 10, [], [], 3, 0, 20, 3)
    assert (best == NONE).all() and (sc == INT_MIN).all() and (nf == 0).all() and best.shape == (10, 3)
    best, sc, nf = ctx.assign_local(0, 10, 50, 50, [], [], -5, -1, 20, 1)
    assert (best == NONE).all() and (nf == 0).all()


@pytest.mark.gpu
def test_assign_interleaved_with_search_and_clustering(gpu, coracle):
    M = _blosum62()
    rng = np.random.default_rng(9)
    members, mc, new = families(rng, 4000, 2000, 12, 12)
    mc = relabel(mc)
    ctx, res, off, qr, rr, ids, msz = setup(M, new, members, mc, rng)
    blk = block(coracle, M, res, off, qr, rr, 0, 3, 0)
    want = expected(blk, mc, ids, msz, 30, 2)
    a1 = ctx.assign_shifted(*qr, *rr, mc, ids, 3, 0, 30, 2)
    s1, _ = ctx.search_shifted(*qr, *rr, 3, 0, 30)
    g1 = ctx.greedy_cluster(3, 0, 30, 100)
    a2 = ctx.assign_shifted(*qr, *rr, mc, ids, 3, 0, 30, 2)
    s2, _ = ctx.search_shifted(*rr, *qr, 3, 0, 30)          # the search with the members as queries: the assignment's rectangle
    l1 = ctx.assign_local(*qr, *rr, mc, ids, -5, -1, 30, 2)
    g2 = ctx.greedy_cluster(3, 0, 30, 100)
    a3 = ctx.assign_shifted(*qr, *rr, mc, ids, 3, 0, 30, 2)
    for got in (a1, a2, a3):
        check(got, want)
    assert np.array_equal(g1[0], g2[0]) and np.array_equal(g1[1], g2[1])
    assert len(s1) == len(s2) == int((blk >= 30).sum())
    blk_l = block(coracle, M, res, off, qr, rr, 1, -5, -1)
    check(l1, expected(blk_l, mc, ids, msz, 30, 2))


@pytest.mark.gpu
def test_assign_final_singletons_of_greedy_are_unassigned(gpu):
    """no oracle: every final singleton of the greedy clustering of 10^5 synthetic 12-mers (BLOSUM62, X = 3, threshold 20)
    was rejected (LimitedGreedySequenceClusterer.java:59-66) by subsets of the final multi-member clusters, and complete
    linkage is monotone: against the final clusters it has no feasible cluster either"""
    M = _blosum62()
    n = 100000
    res, off = synth_peptides(1, n, 12)
    ctx = hammock_amd.Context(M, device=0)
    ctx.set_sequences(residues=res, offsets=off)
    cid, order, stats = ctx.greedy_cluster(3, 0, 20, int(round(n * 0.025)))
    counts = np.bincount(cid, minlength=n)
    multi = counts[cid] > 1
    members = np.nonzero(multi)[0]
    singles = np.nonzero(~multi)[0]
    assert len(members) > 1000 and len(singles) > 1000
    mids, mslot = np.unique(cid[members], return_inverse=True)
    seqs = [res[off[i]:off[i + 1]] for i in np.concatenate([singles, members])]
    r2, o2 = hammock_amd.pack_sequences(seqs)
    ctx2 = hammock_amd.Context(M, device=0)
    ctx2.set_sequences(residues=r2, offsets=o2)
    ns = len(singles)
    best, sc, nf = ctx2.assign_shifted(0, ns, ns, ns + len(members), mslot, mids, 3, 0, 20, 1)
    assert (nf == 0).all() and (best == NONE).all()
    # ... and the members themselves are not all unassigned against the other clusters' side (the call does find clusters)
    best, sc, nf = ctx2.assign_shifted(0, 200, ns, ns + len(members), mslot, mids, 3, 0, -1000, 1)
    assert (nf == len(mids)).all()


def _java_round(v):
    return int(math.floor(v + 0.5))


@pytest.mark.gpu
def test_cli_assign_matches_the_expectation(gpu, coracle, tmp_path):
    """greedy on musi.fa with every fifth record held out, then assign the held-out ones to its clusters"""
    from oracle import hammock_oracle as ho
    with open(os.path.join(GOLDEN, "musi.fa")) as fh:
        lines = fh.read().splitlines()
    records = [lines[k:k + 2] for k in range(0, len(lines), 2)]
    kept, held = tmp_path / "kept.fa", tmp_path / "held.fa"
    kept.write_text("\n".join(l for i, r in enumerate(records) if i % 5 for l in r) + "\n")
    held.write_text("\n".join(l for i, r in enumerate(records) if i % 5 == 0 for l in r) + "\n")
    r = cli("greedy", "-i", str(kept), "-d", str(tmp_path / "g"), timeout=600)
    assert r.returncode == 0, r.stderr
    cfile = tmp_path / "g" / "initial_clusters_sequences.tsv"
    loaded = _cluster_file_expectation(cfile)
    news = ho.load_unique_sequences_from_fasta(str(held))
    text = lambda u: "".join(ALPHABET[c] for c in u.sequence)  # noqa: E731
    new_str = [text(u) for u in news]
    mlens = [len(s) for _, s, _ in loaded]
    X = min(_java_round(sum(mlens) / len(mlens) / 4), min(mlens + [len(s) for s in new_str]) - 1)
    thr = _java_round(sum(mlens) / len(mlens) * 1.7)
    M = _blosum62()
    for extra, best_k in (([], 1), (["--skip_singletons", "--best", "3"], 3), (["--best", "3"], 3)):
        skip = "--skip_singletons" in extra
        ids_all = list(dict.fromkeys(cid for cid, _, _ in loaded))
        uniq = {c: len([1 for cid, _, _ in loaded if cid == c]) for c in ids_all}
        cids = [c for c in ids_all if not skip or uniq[c] > 1]
        slot = {c: i for i, c in enumerate(cids)}
        mem = [(slot[cid], s, sz) for cid, s, sz in loaded if cid in slot]
        seqs = new_str + [s for _, s, _ in mem]
        res, off = hammock_amd.pack_sequences(seqs)
        nq = len(new_str)
        st, blk = coracle.score_block(M, res, off, np.arange(nq, len(seqs)), np.arange(nq), 0, X, 0)
        assert st == 0
        mc = np.array([c for c, _, _ in mem], dtype=np.int64)
        msz = np.array([sz for _, _, sz in mem], dtype=np.int64)
        best, score, nf = expected(blk, mc, cids, msz, thr, best_k)
        size = np.bincount(mc, weights=msz, minlength=len(cids)).astype(np.int64)
        want = ["sequence\trank\tcluster_id\tscore\tcluster_size\tfeasible_clusters"]
        for q in range(nq):
            if nf[q] == 0:
                want.append(f"{new_str[q]}\tNA\tNA\tNA\tNA\t0")
            for t in range(min(int(nf[q]), best_k)):
                c = int(best[q, t])
                want.append(f"{new_str[q]}\t{t + 1}\t{cids[c]}\t{score[q, t]}\t{size[c]}\t{nf[q]}")
        assert (nf > 0).sum() > 5
        out = tmp_path / ("a" + "".join(extra).replace("-", "_"))
        r = cli("assign", "-i", str(held), "--clusters", str(cfile), "-d", str(out), *extra, timeout=600)
        assert r.returncode == 0, r.stderr
        assert "Max shift not set. Setting automatically to: " + str(X) in r.stderr
        assert "not set. Setting automatically to: " + str(thr) in r.stderr
        assert (out / "assignments.tsv").read_text().splitlines() == want
        assert (out / "run.log").exists()
