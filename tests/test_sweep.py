"""Greedy clusterings at a range of thresholds from one scoring pass: hmk_greedy_sweep (k_sweep.hip), hmk_greedy_sweep_from_edges,
hmk_greedy_sweep_from_edges_dev and `hammock-hip sweep`.

The expected answer is never the code under test: the C oracle's greedy_cluster, once per threshold, computed once per input and
shared; on the GPU also a loop of hmk_greedy_cluster calls on the same context, which the sweep must equal row for row.
CPU part (host-only context): the symbols, _from_edges against the oracle at every threshold (MUSI, random peptides, sizes, the
hand traces, an asymmetric matrix), a crash inside the range, ignored / shuffled / clamped edges, every refusal, the mode's errors.
GPU part: the scoring call against the loop and the oracle; _from_edges_dev on the pass's own edges and on synthetic lists at the
default grid and on 1 and 3 workgroups; invalid edges, the grow path, state between calls, null outputs, [0, 0], the mode's files, the mode at a --pick where the reference would throw.
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, hand_traces, random_peptides
from test_assign import gpu   # noqa: F401  (the fixture that skips where no HIP device is visible)
from test_continue import cli

import hammock_amd
from hammock_amd import _native as N
from hammock_amd.synth import synth_peptides
from oracle import c_oracle

SHARED = ("phase1_stop_index", "phase1_clusters", "phase1_orphans", "n_result_clusters", "n_multi")   # hmk_greedy_stats' fields in a level
GRID_LINE = re.compile(r"^\[hmk grid\] (\S+) (\d+) -> (\d+)$", re.M)
CRASH = N.HMK_ERR_REFERENCE_WOULD_CRASH


@functools.lru_cache(maxsize=None)
def matrix(name="blosum62"):
    import json
    with open(os.path.join(GOLDEN, "matrices.json")) as fh:
        return np.asarray(json.load(fh)["matrices"][name], dtype=np.int32)


# ---- inputs ----------------------------------------------------------------------------------------------------------------

def _sorted(res, off, sizes):
    """the greedy order (UniqueSequence.sortSequences by size) -> (res, off, sizes)"""
    perm = c_oracle.sort_order(res, off, sizes, "size")
    peps = [res[off[k]:off[k + 1]] for k in perm]
    return hammock_amd.pack_sequences(peps) + (None if sizes is None else sizes[perm],)


@functools.lru_cache(maxsize=None)
def inp(name):
    """-> dict: M, res, off, sizes, X, p, thr, hi, maxc"""
    M, sizes = matrix(), None
    if name == "musi":
        from oracle import hammock_oracle as po
        seqs = po.load_unique_sequences_from_fasta(os.path.join(GOLDEN, "musi.fa"))
        thr, X, maxc = po.greedy_defaults(seqs)
        po.sort_sequences(seqs, "size")
        res, off = c_oracle.pack([s.get_sequence_string() for s in seqs])
        assert (thr, X, maxc) == (20, 3, 61)
        X, p, thr, hi = 3, 0, 20, 40
    elif name == "random400":
        res, off = c_oracle.pack(random_peptides(np.random.default_rng(31), 400, 7, 12, alphabet=6))
        X, p, thr, hi, maxc = 2, -1, 14, 24, 20
    elif name == "sizes300":
        rng = np.random.default_rng(32)
        res, off = c_oracle.pack(random_peptides(rng, 300, 9, 12, alphabet=5))
        res, off, sizes = _sorted(res, off, rng.integers(1, 50, size=300).astype(np.int32))
        X, p, thr, hi, maxc = 2, 0, 15, 25, 12
    elif name == "asym":
        rng = np.random.default_rng(5)
        M = matrix().copy()
        M[np.triu_indices(24, 1)] += rng.integers(-2, 3, size=276).astype(np.int32)
        assert not (M == M.T).all()
        res, off = c_oracle.pack(random_peptides(rng, 200, 10, 12, alphabet=5))
        X, p, thr, hi, maxc = 3, 0, 16, 24, 10
    elif name == "crash":   # families of near-duplicates, no cluster limit: phase 1 walks to the last sequence
        rng = np.random.default_rng(4)
        res, off = synth_peptides(4, 150, 7, 12)
        peps = [res[off[k]:off[k + 1]].copy() for k in range(150)]
        for k in range(50, 150):
            src = peps[int(rng.integers(0, 50))].copy()
            for _ in range(int(rng.integers(1, 4))):
                src[int(rng.integers(len(src)))] = rng.integers(0, 20)
            peps[k] = src
        peps = list({bytes(q): q for q in peps}.values())
        res, off = hammock_amd.pack_sequences(peps)
        sizes = np.ones(len(peps), dtype=np.int32)
        pick = rng.random(len(peps)) < 0.3
        sizes[pick] = 1 + rng.integers(0, 50, int(pick.sum()))
        res, off, sizes = _sorted(res, off, sizes)
        X, p, thr, hi, maxc = 2, 0, 10, 22, len(peps)
    elif name == "synth12":
        res, off = synth_peptides(1, 3000, 12)
        X, p, thr, hi, maxc = 3, 0, 18, 30, 75
    elif name == "synth7to12":
        res, off = synth_peptides(1, 3000, 7, 12)
        X, p, thr, hi, maxc = 2, -1, 14, 22, 75
    elif name == "keyed":   # one length, max shift 3: the plan is key-sorted (HMK_NO_KEY_SORT=1 is the other order)
        res, off = synth_peptides(5, 5000, 12)
        X, p, thr, hi, maxc = 3, 0, 20, 26, 125
    elif name == "three_letters":   # a dense graph, long levels
        res, off = c_oracle.pack(random_peptides(np.random.default_rng(77), 2000, 12, 12, alphabet=3))
        X, p, thr, hi, maxc = 3, 0, 14, 18, 50
    elif name == "ends":   # the +-1,000 matrix: W/B words score 12,000 with each other, top - t crosses 255 inside the range
        from test_score_key_ends import ends_matrix
        import lane_model as lm
        M = np.array(ends_matrix())
        rng = np.random.default_rng(33)
        wb = np.array([lm.code("W"), lm.code("B")], dtype=np.uint8)
        peps = [wb[rng.integers(0, 2, size=12)] for _ in range(400)] + random_peptides(rng, 300, 12, 12)
        peps = list({bytes(q): q for q in peps}.values())
        res, off = hammock_amd.pack_sequences(peps)
        X, p, thr, hi, maxc = 0, 0, 11740, 11750, 10
    else:
        raise KeyError(name)
    for a in (res, off):
        a.setflags(write=False)
    return dict(M=M, res=res, off=off, sizes=sizes, X=X, p=p, thr=thr, hi=hi, maxc=maxc, n=len(off) - 1)


@functools.lru_cache(maxsize=None)
def oracle_levels(name, thr=None, hi=None):
    """-> per threshold (status, cluster_id, result_order, member_rank, stats) of the C oracle's greedy_cluster"""
    d = inp(name)
    out = []
    for t in range(d["thr"] if thr is None else thr, (d["hi"] if hi is None else hi) + 1):
        st, cid, order, stats = c_oracle.greedy_cluster(d["M"], d["res"], d["off"], d["sizes"], 0, d["X"], d["p"], t, d["maxc"], 1)
        assert st in (0, c_oracle.HMO_ERR_REFERENCE_WOULD_CRASH)
        out.append((st, cid, order, stats.member_rank, stats))
    return out


@functools.lru_cache(maxsize=None)
def oracle_scores(name):
    """-> (x, m, sc): ShiftedScorer.sequenceScore(seq1 = m, seq2 = x) from c_oracle.score_block over the whole square; x < m for a
    symmetric matrix, every ordered pair otherwise"""
    d = inp(name)
    n = d["n"]
    st, sc = c_oracle.score_block(d["M"], d["res"], d["off"], np.arange(n), np.arange(n), 0, d["X"], d["p"])   # [seq1][seq2]
    assert st == 0
    x, m = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    keep = x < m if symmetric(name) else x != m
    return x[keep], m[keep], sc.T[keep]


def symmetric(name):
    return bool((inp(name)["M"] == inp(name)["M"].T).all())


def oracle_edges(name, thr=None):
    x, m, sc = oracle_scores(name)
    keep = sc >= (inp(name)["thr"] if thr is None else thr)
    return hammock_amd.pack_edges(x[keep], m[keep], sc[keep])


def make_ctx(name, device=-1):
    d = inp(name)
    ctx = hammock_amd.Context(d["M"], device=device)
    ctx.set_sequences(residues=d["res"], offsets=d["off"], sizes=d["sizes"])
    return ctx


def same_as_oracle(got, want, n_edges=None, what=""):
    """got: (levels, cluster_id, result_order, member_rank) of a sweep; want: oracle_levels' list over the same range"""
    levels, cid, order, rank = got
    assert levels.size == len(want) == cid.shape[0]
    for l, (st, ocid, oorder, orank, ostats) in enumerate(want):
        lv, w = levels[l], f"{what}level {l} "
        if st:
            assert (lv["status"], lv["crash_case"], lv["crash_index"]) == (CRASH, ostats.crash_case, ostats.crash_index), w
            assert (cid[l] == -1).all() and (order[l] == -1).all() and (rank[l] == -1).all(), w
            continue
        assert (lv["status"], lv["crash_case"]) == (0, 0), w
        assert np.array_equal(cid[l], ocid), w + "cluster_id"
        assert np.array_equal(order[l, :lv["n_result_clusters"]], oorder) and (order[l, lv["n_result_clusters"]:] == -1).all(), w + "result_order"
        assert np.array_equal(rank[l], orank), w + "member_rank"
        assert [int(lv[f]) for f in SHARED] == [getattr(ostats, f) for f in SHARED], w
        size = np.bincount(ocid)
        assert (lv["n_singletons"], lv["largest"]) == ((size == 1).sum(), size.max()), w
        if n_edges is not None:
            assert lv["n_edges"] == n_edges[l], w + "n_edges"


def edge_counts(name, thr=None, hi=None):
    d = inp(name)
    sc = oracle_scores(name)[2]
    return [int((sc >= t).sum()) for t in range(d["thr"] if thr is None else thr, (d["hi"] if hi is None else hi) + 1)]


def raw(ctx, fn, head, thr, hi, maxc=10, arrays=(True, True, True), levels=True, n_levels=256):
    """the C call with NULL where an output is not wanted -> (status, levels, [cluster_id, result_order, member_rank], stats)"""
    out = [np.full((n_levels, max(ctx.n, 1)), -7, dtype=np.int32) for _ in range(3)]
    lv = np.zeros(n_levels, dtype=hammock_amd.api.GREEDY_LEVEL_DTYPE)
    stats = N.GreedySweepStats()
    st = fn(ctx._h, *head, thr, hi, maxc, *[a.ctypes.data_as(C.POINTER(C.c_int32)) if on else None for a, on in zip(out, arrays)],
            lv.ctypes.data_as(C.POINTER(N.GreedyLevel)) if levels else None, C.byref(stats))
    return st, lv, out, stats


# ---- CPU: the symbols ------------------------------------------------------------------------------------------------------

def test_symbols_are_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "hammock_hip.h")) as fh:
        header = fh.read()
    for name in ("hmk_greedy_sweep", "hmk_greedy_sweep_from_edges", "hmk_greedy_sweep_from_edges_dev"):
        assert re.search(r"\bint " + name + r"\(", header)
        assert name in N.SYMBOLS and hasattr(N.lib, name)
    assert "hmk_greedy_level" in header and "hmk_greedy_sweep_stats" in header
    assert header.count("LimitedGreedySequenceClusterer.java:22,39-69") >= 4   # hmk_greedy_cluster's and the three new entry points'
    assert re.search(r"#define HMK_ABI_VERSION 4\b", header) and N.lib.hmk_abi_version() == 4
    assert C.sizeof(N.GreedyLevel) == 56 == hammock_amd.api.GREEDY_LEVEL_DTYPE.itemsize and C.sizeof(N.GreedySweepStats) == 40
    for (name, ctype), (dname, (dtype, offset)) in zip(N.GreedyLevel._fields_, hammock_amd.api.GREEDY_LEVEL_DTYPE.fields.items()):
        assert name == dname and getattr(N.GreedyLevel, name).offset == offset and C.sizeof(ctype) == dtype.itemsize


# ---- CPU: _from_edges against the oracle -------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["musi", "random400", "sizes300", "asym"])
def test_from_edges_equals_the_oracle_at_every_threshold(name):
    d = inp(name)
    want = oracle_levels(name)
    if name == "musi":   # the known answer at the default threshold
        size = np.bincount(want[0][1])
        assert (want[0][4].phase1_stop_index, int((size > 1).sum()), int((size == 1).sum())) == (67, 61, 1755)
    assert not any(st for st, *_ in want) and len({int(w[4].n_result_clusters) for w in want}) > 1
    ctx = make_ctx(name)
    got = ctx.greedy_sweep_from_edges(oracle_edges(name), symmetric(name), d["thr"], d["hi"], d["maxc"])
    same_as_oracle(got, want, edge_counts(name))
    s = ctx.last_sweep_stats
    assert (s.n_edges, s.pairs_scored, s.n_levels, s.kernel_ms, s.deal_ms) == (edge_counts(name)[0], 0, d["hi"] - d["thr"] + 1, 0.0, 0.0)
    if name == "musi":
        lv = got[0][0]
        assert (lv["phase1_stop_index"], lv["n_multi"], lv["n_singletons"]) == (67, 61, 1755)


def test_from_edges_on_the_hand_traces_across_their_thresholds():
    ht, M = hand_traces()
    X, p = ht["max_shift"], ht["shift_penalty"]
    seen = set()
    for case in ht["greedy"]:
        res, off = c_oracle.pack(case["sequences"])
        sizes = np.asarray(case["sizes"], dtype=np.int32)
        n, t0 = len(case["sequences"]), case["threshold"]
        ii, jj = np.triu_indices(n, 1)
        st, sc = c_oracle.score_pairs(M, res, off, jj, ii, 0, X, p)
        assert st == 0
        keep = sc >= t0 - 2
        ctx = hammock_amd.Context(M, device=-1)
        ctx.set_sequences(residues=res, offsets=off, sizes=sizes)
        levels, cid, order, rank = ctx.greedy_sweep_from_edges(hammock_amd.pack_edges(ii[keep], jj[keep], sc[keep]), True, t0 - 2, t0 + 2,
                                                               case["max_clusters"])
        exp = case["expect"]   # the hand trace itself at its own threshold
        if exp["status"] == "crash":
            assert (levels[2]["status"], levels[2]["crash_case"], levels[2]["crash_index"]) == (CRASH, exp["crash_case"], exp["crash_index"])
            assert (cid[2] == -1).all()
        else:
            assert cid[2].tolist() == exp["cluster_id"] and order[2, :levels[2]["n_result_clusters"]].tolist() == exp["result_order"]
            assert rank[2].tolist() == exp["member_rank"], case["name"]
        want = []   # ... and the oracle around it
        for t in range(t0 - 2, t0 + 3):
            st, ocid, oorder, ostats = c_oracle.greedy_cluster(M, res, off, sizes, 0, X, p, t, case["max_clusters"], 1)
            want.append((st, ocid, oorder, ostats.member_rank, ostats))
            seen.add(ostats.crash_case if st else 0)
        same_as_oracle((levels, cid, order, rank), want, what=case["name"] + " ")
    assert seen == {0, 1, 2, 3}


def test_a_crash_inside_the_range_is_recorded_in_its_level_and_the_sweep_goes_on():
    d = inp("crash")
    want = oracle_levels("crash")
    status = [st != 0 for st, *_ in want]
    first = status.index(True)
    # the property of the input, from the oracle alone: a level where the reference throws, an ok level below it, an ok level above
    # it, at most half of the levels crash, and the ok levels do cluster
    assert 0 < first and not all(status[first:]) and 2 * sum(status) <= len(status)
    assert all(w[4].n_multi >= 3 for w, bad in zip(want, status) if not bad)
    ctx = make_ctx("crash")
    got = ctx.greedy_sweep_from_edges(oracle_edges("crash"), True, d["thr"], d["hi"], d["maxc"])
    same_as_oracle(got, want, edge_counts("crash"))
    assert [bool(s) for s in got[0]["status"]] == status
    st, lv, out, _ = raw(ctx, N.lib.hmk_greedy_sweep_from_edges, (oracle_edges("crash").ctypes.data_as(C.POINTER(C.c_uint64)), oracle_edges("crash").size, 1),
                         d["thr"], d["hi"], d["maxc"], n_levels=len(want))
    assert st == 0 and all((a[first] == -1).all() for a in out) and not any((a[0] == -7).any() for a in out[::2])


def test_edges_below_are_ignored_order_and_orientation_do_not_matter_and_scores_above_are_clamped():
    d = inp("random400")
    x, m, sc = oracle_scores("random400")
    ctx = make_ctx("random400")
    thr, hi, maxc = 16, 20, d["maxc"]
    want = oracle_levels("random400", thr, hi)
    counts = edge_counts("random400", thr, hi)
    keep = sc >= 10   # edges below the threshold in the list
    assert (sc[keep] < thr).sum() > 1000 and (sc > hi).sum() > 100   # ... and scores above threshold_hi: the top level's, with their score
    edges = hammock_amd.pack_edges(x[keep], m[keep], sc[keep])
    first = ctx.greedy_sweep_from_edges(edges, True, thr, hi, maxc)
    same_as_oracle(first, want, counts)
    rng = np.random.default_rng(3)
    flip = rng.random(keep.sum()) < 0.5
    other = hammock_amd.pack_edges(np.where(flip, m[keep], x[keep]), np.where(flip, x[keep], m[keep]), sc[keep])[rng.permutation(int(keep.sum()))]
    again = ctx.greedy_sweep_from_edges(other, True, thr, hi, maxc)
    for a, b in zip(first[1:], again[1:]):
        assert np.array_equal(a, b)
    for f in first[0].dtype.names:
        assert f == "tail_ms" or np.array_equal(first[0][f], again[0][f]), f
    for t in (thr, hi):   # threshold_hi == threshold: hmk_greedy_from_edges on the edges >= t
        one = ctx.greedy_sweep_from_edges(edges, True, t, t, maxc)
        cid, order, stats = ctx.greedy_from_edges(oracle_edges("random400", t), True, t, maxc)
        assert np.array_equal(one[1][0], cid) and np.array_equal(one[2][0, :stats.n_result_clusters], order)
        assert np.array_equal(one[3][0], ctx.member_rank[:d["n"]]) and one[0][0]["n_edges"] == stats.n_edges
        assert [int(one[0][0][f]) for f in SHARED] == [getattr(stats, f) for f in SHARED]
    same_as_oracle(ctx.greedy_sweep_from_edges(edges, True, thr, None, maxc), want[:1], counts[:1], "threshold_hi=None ")


# ---- CPU: the argument checks ------------------------------------------------------------------------------------------------

def test_bad_arguments_are_refused_before_the_device_is_looked_at():
    d = inp("random400")
    n = d["n"]
    edges = oracle_edges("random400")
    ctx = make_ctx("random400")
    ep = (edges.ctypes.data_as(C.POINTER(C.c_uint64)), edges.size, 1)
    heads = [(N.lib.hmk_greedy_sweep, (2, -1)), (N.lib.hmk_greedy_sweep_from_edges, ep), (N.lib.hmk_greedy_sweep_from_edges_dev, (None, 0, 1))]
    for fn, head in heads:   # the same checks in all three, on a host-only context
        assert raw(ctx, fn, head, 21, 20)[0] == N.HMK_ERR_BAD_ARG
        assert raw(ctx, fn, head, 20, 276)[0] == N.HMK_ERR_BAD_ARG
        assert raw(ctx, fn, head, -2 ** 31, 2 ** 31 - 1)[0] == N.HMK_ERR_BAD_ARG
        assert raw(ctx, fn, head, 32760, 32768)[0] == N.HMK_ERR_BAD_ARG
        assert raw(ctx, fn, head, 20, 22, arrays=(False, False, False), levels=False)[0] == N.HMK_ERR_BAD_ARG
        assert fn(None, *head, 20, 20, 10, None, None, None, None, None) == N.HMK_ERR_BAD_ARG
    assert raw(ctx, N.lib.hmk_greedy_sweep_from_edges, ep, 14, 269)[0] == 0   # 256 levels are allowed
    assert raw(ctx, N.lib.hmk_greedy_sweep_from_edges, ep, 32760, 32767)[0] == 0
    with pytest.raises(ValueError, match="threshold_hi"):
        ctx.greedy_sweep_from_edges(edges, True, 20, 19, 10)
    for x, m in ((3, n), (n, 3), (2 ** 24 - 1, 0), (5, 5)):   # an index >= n either side, a self pair, whatever its score
        for score in (25, 3):
            bad = edges.copy()
            bad[100] = hammock_amd.pack_edges(np.array([x]), np.array([m]), np.array([score]))[0]
            with pytest.raises(ValueError, match="outside"):
                ctx.greedy_sweep_from_edges(bad, True, 14, 20, 10)
    assert raw(ctx, N.lib.hmk_greedy_sweep_from_edges, (None, 5, 1), 20, 20)[0] == N.HMK_ERR_BAD_ARG
    same_as_oracle(ctx.greedy_sweep_from_edges(edges, True, d["thr"], d["hi"], d["maxc"]), oracle_levels("random400"), what="after the refusals ")
    # every combination of null outputs but the empty one
    full = raw(ctx, N.lib.hmk_greedy_sweep_from_edges, ep, 14, 18, d["maxc"])
    for mask in range(1, 16):
        on = [bool(mask >> k & 1) for k in range(4)]
        st, lv, out, _ = raw(ctx, N.lib.hmk_greedy_sweep_from_edges, ep, 14, 18, d["maxc"], arrays=on[:3], levels=on[3])
        assert st == 0
        for k in range(3):
            assert np.array_equal(out[k][:5], full[2][k][:5]) if on[k] else (out[k] == -7).all()
        assert all(f == "tail_ms" or np.array_equal(lv[f], full[1][f]) for f in lv.dtype.names) if on[3] else not lv["n_edges"].any()


def test_the_device_forms_need_a_device_and_an_empty_set_is_ok():
    ctx = make_ctx("random400")
    with pytest.raises(hammock_amd.DeviceError):
        ctx.greedy_sweep(2, -1, 14, 18, 10)
    with pytest.raises(hammock_amd.DeviceError):
        ctx.greedy_sweep_from_edges_dev(0, 0, True, 14, 18, 10)
    empty = hammock_amd.Context(matrix(), device=-1)
    levels, cid, order, rank = empty.greedy_sweep_from_edges(np.zeros(0, dtype=np.uint64), True, 20, 24, 10)
    assert cid.shape == (5, 0) and levels.size == 5 and not any(levels[f].any() for f in levels.dtype.names)
    assert empty.last_sweep_stats.n_levels == 5
    for fn, head in ((N.lib.hmk_greedy_sweep, (3, 0)), (N.lib.hmk_greedy_sweep_from_edges, (None, 0, 1)), (N.lib.hmk_greedy_sweep_from_edges_dev, (None, 0, 1))):
        assert raw(empty, fn, head, 20, 24, arrays=(False, False, False), levels=False)[0] == 0


def test_cli_sweep_argument_and_file_errors(tmp_path):
    fa = os.path.join(GOLDEN, "musi.fa")
    r = cli("sweep", "-d", str(tmp_path / "a"))
    assert r.returncode == 2 and "-i or --input" in r.stderr
    assert not (tmp_path / "a").exists()
    r = cli("sweep", "-i", fa, "--devices", "0,1", "-d", str(tmp_path / "a"))
    assert r.returncode == 2 and "--devices" in r.stderr
    r = cli("sweep", "-i", fa, "-f", "nothing", "-d", str(tmp_path / "a"))
    assert r.returncode == 2 and "-f" in r.stderr
    r = cli("sweep", "-i", fa, "-g", "26", "--scan_to", "25", "-d", str(tmp_path / "b"))
    assert r.returncode == 2 and "--scan_to" in r.stderr
    r = cli("sweep", "-i", fa, "--scan_to", "276", "-d", str(tmp_path / "c"))   # the derived threshold is 20
    assert r.returncode == 2 and "--scan_to" in r.stderr and "20 up to 275" in r.stderr
    for pick in ("19", "31"):
        r = cli("sweep", "-i", fa, "--scan_to", "30", "--pick", pick, "-d", str(tmp_path / ("p" + pick)))
        assert r.returncode == 2 and "--pick" in r.stderr and "20 up to 30" in r.stderr
        assert not (tmp_path / ("p" + pick) / "greedy_levels.tsv").exists()
    r = cli("sweep", "-i", fa, "-d", str(tmp_path / "c"))   # the directory exists now
    assert r.returncode == 2 and "Output directory exists" in r.stderr
    r = cli("sweep", "-i", str(tmp_path / "missing.fa"), "-d", str(tmp_path / "d"))
    assert r.returncode != 0
    r = cli("sweep", "-i", fa, "-l", "no_such_label", "-d", str(tmp_path / "e"))
    assert r.returncode == 3 and "No sequences" in r.stderr
    assert "hammock-hip sweep -i" in cli("--help").stderr and "--pick <int>" in cli("--help").stderr


# ---- GPU: the scoring call ---------------------------------------------------------------------------------------------------

def loop_of_greedy_cluster(ctx, d, thr, hi):
    """one hmk_greedy_cluster call per threshold on the same context -> oracle_levels' form"""
    out = []
    for t in range(thr, hi + 1):
        try:
            cid, order, stats = ctx.greedy_cluster(d["X"], d["p"], t, d["maxc"])
            out.append((0, cid.copy(), order.copy(), ctx.member_rank[:d["n"]].copy(), stats))
        except hammock_amd.ReferenceWouldCrash as e:
            stats = N.GreedyStats()
            stats.crash_case, stats.crash_index = e.case, e.index
            out.append((CRASH, None, None, None, stats))
    return out


def equal_sweeps(a, b):
    for f in a[0].dtype.names:
        assert f == "tail_ms" or np.array_equal(a[0][f], b[0][f]), f
    for u, v in zip(a[1:], b[1:]):
        assert np.array_equal(u, v)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["musi", "synth12", "synth7to12", "keyed", "three_letters", "sizes300", "crash", "asym", "ends", "random400"])
def test_greedy_sweep_equals_a_loop_of_greedy_cluster_and_the_oracle(gpu, monkeypatch, capfd, name):
    d = inp(name)
    thr, hi = d["thr"], d["hi"]
    if name == "random400":   # a range whose top levels have no edge
        top = int(oracle_scores(name)[2].max())
        thr, hi = top - 1, top + 3
    ctx = make_ctx(name, 0)
    if name == "keyed":   # the planner's timeline names the step only a key-sorted plan has
        monkeypatch.setenv("HMK_GREEDY_TIMING", "1")
        capfd.readouterr()
    got = ctx.greedy_sweep(d["X"], d["p"], thr, hi, d["maxc"])
    if name == "keyed":
        assert "[hmk plan] row-shared groups" in capfd.readouterr().err, "the plan of this case is not key-sorted"
        monkeypatch.delenv("HMK_GREEDY_TIMING")
    s = ctx.last_sweep_stats
    n = d["n"]
    assert s.pairs_scored == n * (n - 1) // 2 or not symmetric(name)
    assert (s.n_levels, s.n_edges) == (hi - thr + 1, got[0]["n_edges"][0]) and s.kernel_ms > 0 and (s.deal_ms > 0 or s.n_edges == 0)
    assert (np.diff(got[0]["n_edges"].astype(np.int64)) <= 0).all()
    same_as_oracle(got, loop_of_greedy_cluster(ctx, d, thr, hi), what="loop ")
    for t in (thr, hi):   # the levels' edge counts are the pass's own at that threshold
        assert got[0]["n_edges"][t - thr] == ctx.neighbors_shifted(d["X"], d["p"], t)[0].size
    if name in ("musi", "synth12", "synth7to12", "sizes300", "crash", "asym", "random400"):
        same_as_oracle(got, oracle_levels(name, thr, hi), what="oracle ")
    if name == "random400":
        assert got[0]["n_edges"][1] > 0 and not got[0]["n_edges"][2:].any()
    if name == "ends":   # 8-byte adjacency entries at the lower levels, 4-byte ones above, the same graph throughout
        top = 12 * 1000
        assert top - thr > 255 >= top - hi and got[0]["n_edges"][0] == got[0]["n_edges"][-1] > 10000
    if name == "crash":
        assert got[0]["status"].any() and not got[0]["status"].all()
    if name == "keyed":   # the other order of the pass: identical output
        monkeypatch.setenv("HMK_NO_KEY_SORT", "1")
        monkeypatch.setenv("HMK_GREEDY_TIMING", "1")
        other = make_ctx(name, 0)
        capfd.readouterr()
        plain = other.greedy_sweep(d["X"], d["p"], thr, hi, d["maxc"])
        err = capfd.readouterr().err
        assert "[hmk plan] device copies" in err and "row-shared groups" not in err
        monkeypatch.delenv("HMK_NO_KEY_SORT")
        monkeypatch.delenv("HMK_GREEDY_TIMING")
        equal_sweeps(plain, got)


# ---- GPU: _from_edges_dev ------------------------------------------------------------------------------------------------------

def device_edges(edges):
    import torch
    return torch.from_numpy(edges.view(np.int64).copy()).to("cuda:0")


@functools.lru_cache(maxsize=None)
def synthetic(name):
    """-> (n, packed edges, threshold, threshold_hi): edge lists for the dealing kernels"""
    rng = np.random.default_rng(99)
    if name == "repeated":   # one edge 1,000 times
        return 10, hammock_amd.pack_edges(np.full(1000, 3), np.full(1000, 7), np.full(1000, 22)), 20, 24
    if name == "none":
        return 50, np.zeros(0, dtype=np.uint64), 20, 24
    if name == "single_level":   # threshold_hi = threshold: one level, the scores below it left out, those above it clamped into it
        a, b = np.triu_indices(50, 1)
        pick = rng.choice(a.size, 600, replace=False)
        return 50, hammock_amd.pack_edges(a[pick], b[pick], 20 + np.arange(600) % 5), 22, 22
    n = 3000
    x, m = np.triu_indices(n, 1)
    if name == "one_level":   # all scores in one level
        pick = rng.choice(x.size, 40000, replace=False)
        return n, hammock_amd.pack_edges(x[pick], m[pick], np.full(40000, 23)), 20, 26
    if name == "clamped":   # 257 distinct scores (and some below the threshold) clamped into 256 levels; both orientations
        pick = rng.choice(x.size, 60000, replace=False)
        sc = 98 + np.arange(60000) % 259
        flip = rng.random(60000) < 0.5
        return n, hammock_amd.pack_edges(np.where(flip, m[pick], x[pick]), np.where(flip, x[pick], m[pick]), sc), 100, 355
    if name == "long_level":   # more than 1,024 x the largest grid (2,048 workgroups) edges of one level, a few of others
        pick = rng.choice(x.size, 2048 * 1024 + 5000, replace=False)
        sc = np.where(np.arange(pick.size) % 1000 == 0, 21 + np.arange(pick.size) % 3, 20)
        return n, hammock_amd.pack_edges(x[pick], m[pick], sc), 20, 23
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def synthetic_expect(name):
    """hmk_greedy_sweep_from_edges on a host-only context (itself tested against the oracle above)"""
    n, edges, thr, hi = synthetic(name)
    ctx = hammock_amd.Context(matrix(), device=-1)
    res, off = synth_peptides(40, n, 12)
    ctx.set_sequences(residues=res, offsets=off)
    return ctx.greedy_sweep_from_edges(edges, True, thr, hi, 40)


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [0, 1, 3])
@pytest.mark.parametrize("name", ["repeated", "none", "single_level", "one_level", "clamped", "long_level"])
def test_from_edges_dev_on_synthetic_edge_lists_at_every_grid(gpu, monkeypatch, capfd, name, cap):
    n, edges, thr, hi = synthetic(name)
    ctx = hammock_amd.Context(matrix(), device=0)
    res, off = synth_peptides(40, n, 12)
    ctx.set_sequences(residues=res, offsets=off)
    dev = device_edges(edges) if edges.size else None
    if cap:
        monkeypatch.setenv("HMK_TEST_GRID_CAP", str(cap))
    capfd.readouterr()
    got = ctx.greedy_sweep_from_edges_dev(dev.data_ptr() if edges.size else 0, edges.size, True, thr, hi, 40)
    lines = {}
    for kernel, wanted, launched in GRID_LINE.findall(capfd.readouterr().err):
        lines.setdefault(kernel, set()).add((int(wanted), int(launched)))
    if cap:
        monkeypatch.delenv("HMK_TEST_GRID_CAP")
    equal_sweeps(got, synthetic_expect(name))
    s = ctx.last_sweep_stats
    assert (s.pairs_scored, s.kernel_ms, s.n_levels) == (0, 0.0, hi - thr + 1) and (s.deal_ms > 0 or not edges.size)
    by_chunk = min(-(-edges.size // 1024), 2048)   # k_sweep.hip's launchers
    cut = {k: {(by_chunk, cap)} for k in ("k_sweep_hist", "k_sweep_deal") if cap and by_chunk > cap}
    assert {k: v for k, v in lines.items() if k.startswith("k_sweep_")} == cut
    if name == "long_level":
        assert -(-edges.size // 1024) > 2048 and got[0]["n_edges"][0] == edges.size
    if name == "single_level":
        assert hi == thr and s.n_levels == 1 and got[0]["n_edges"][0] == 360
    if name == "clamped":
        assert hi - thr == 255 and got[0]["n_edges"][0] < edges.size and got[0]["n_edges"][255] > edges.size // 259


@pytest.mark.gpu
def test_from_edges_dev_on_the_passes_own_compacted_edges(gpu):
    import torch
    d = inp("synth12")
    ctx = make_ctx("synth12", 0)
    cap = 1 << 22
    d_edges = torch.zeros(cap, dtype=torch.int64, device="cuda:0")
    d_counts = torch.zeros(N.HMK_EDGE_SHARDS, dtype=torch.int64, device="cuda:0")
    d_out = torch.zeros(cap, dtype=torch.int64, device="cuda:0")
    d_total = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    ctx.neighbors_shifted_dev(d["X"], d["p"], d["thr"], 0, 1, d_edges.data_ptr(), cap, d_counts.data_ptr())
    ctx.compact_edges_dev(d_edges.data_ptr(), cap, d_counts.data_ptr(), d_out.data_ptr(), cap, d_total.data_ptr())
    torch.cuda.synchronize()
    total = int(d_total.item())
    assert 0 < total <= cap
    got = ctx.greedy_sweep_from_edges_dev(d_out.data_ptr(), total, True, d["thr"], d["hi"], d["maxc"])
    same_as_oracle(got, oracle_levels("synth12"))
    assert got[0]["n_edges"][0] == total
    equal_sweeps(got, ctx.greedy_sweep(d["X"], d["p"], d["thr"], d["hi"], d["maxc"]))


@pytest.mark.gpu
def test_from_edges_dev_refuses_invalid_edges_and_goes_on(gpu):
    n, edges, thr, hi = synthetic("one_level")
    ctx = hammock_amd.Context(matrix(), device=0)
    res, off = synth_peptides(40, n, 12)
    ctx.set_sequences(residues=res, offsets=off)
    for x, m in ((3, n), (n + 5, 3), (2 ** 24 - 1, 2 ** 24 - 2), (5, 5)):
        bad = edges.copy()
        bad[7000] = hammock_amd.pack_edges(np.array([x]), np.array([m]), np.array([25]))[0]
        dev = device_edges(bad)
        with pytest.raises(ValueError, match="outside"):
            ctx.greedy_sweep_from_edges_dev(dev.data_ptr(), dev.numel(), True, thr, hi, 40)
        dev = device_edges(edges)
        equal_sweeps(ctx.greedy_sweep_from_edges_dev(dev.data_ptr(), dev.numel(), True, thr, hi, 40), synthetic_expect("one_level"))
    assert raw(ctx, N.lib.hmk_greedy_sweep_from_edges_dev, (None, 5, 1), 20, 20)[0] == N.HMK_ERR_BAD_ARG


@pytest.mark.gpu
def test_the_grow_path_gives_the_same(gpu, monkeypatch, capfd):
    """a first edge buffer of 2^20 entries (16,384 per segment) under 1.7 million edges: the pass is scored twice, which the
    call's timeline says"""
    d = inp("three_letters")
    monkeypatch.setenv("HMK_EDGE_GUESS", "4096")
    monkeypatch.setenv("HMK_GREEDY_TIMING", "1")
    ctx = make_ctx("three_letters", 0)   # a fresh context: no buffer grown by an earlier call
    capfd.readouterr()
    got = ctx.greedy_sweep(d["X"], d["p"], d["thr"], d["hi"], d["maxc"])
    err = capfd.readouterr().err
    monkeypatch.delenv("HMK_EDGE_GUESS")
    monkeypatch.delenv("HMK_GREEDY_TIMING")
    assert got[0]["n_edges"][0] > 2 ** 20
    assert len(re.findall(r"^\[hmk\] an edge segment overflowed \(\d+ entries for 16384\): \d+ entries next, scoring again$", err, re.M)) == 1
    equal_sweeps(got, make_ctx("three_letters", 0).greedy_sweep(d["X"], d["p"], d["thr"], d["hi"], d["maxc"]))


@pytest.mark.gpu
def test_state_between_calls_and_null_outputs(gpu):
    d = inp("musi")
    ctx = make_ctx("musi", 0)
    first = ctx.greedy_sweep(d["X"], d["p"], 20, 40, d["maxc"])
    same_as_oracle(first, oracle_levels("musi"))
    cid, order, stats = ctx.greedy_cluster(d["X"], d["p"], 33, d["maxc"])
    assert np.array_equal(cid, first[1][13]) and np.array_equal(order, first[2][13, :stats.n_result_clusters])
    same_as_oracle(ctx.greedy_sweep(d["X"], d["p"], 30, 34, d["maxc"]), oracle_levels("musi")[10:15], what="another range ")
    equal_sweeps(ctx.greedy_sweep(d["X"], d["p"], 20, 40, d["maxc"]), first)
    full = raw(ctx, N.lib.hmk_greedy_sweep, (d["X"], d["p"]), 26, 29, d["maxc"])
    assert full[0] == 0
    for mask in range(1, 16):
        on = [bool(mask >> k & 1) for k in range(4)]
        st, lv, out, _ = raw(ctx, N.lib.hmk_greedy_sweep, (d["X"], d["p"]), 26, 29, d["maxc"], arrays=on[:3], levels=on[3])
        assert st == 0
        for k in range(3):
            assert np.array_equal(out[k][:4], full[2][k][:4]) if on[k] else (out[k] == -7).all()
        assert all(f == "tail_ms" or np.array_equal(lv[f], full[1][f]) for f in lv.dtype.names) if on[3] else not lv["n_edges"].any()
    levels, *_ = ctx.greedy_sweep(d["X"], d["p"], 20, 22, d["maxc"], arrays=False)
    assert _ == [None, None, None] and np.array_equal(levels["n_multi"], first[0]["n_multi"][:3])


@pytest.mark.gpu
def test_the_device_list_runs_on_the_root(gpu):
    d = inp("synth12")
    ctx = hammock_amd.Context(matrix(), device=[0, 0])
    ctx.set_sequences(residues=d["res"], offsets=d["off"])
    same_as_oracle(ctx.greedy_sweep(d["X"], d["p"], d["thr"], d["hi"], d["maxc"]), oracle_levels("synth12"))


# ---- GPU: the mode ---------------------------------------------------------------------------------------------------------

STAGE1 = ("initial_clusters_sequences.tsv", "initial_clusters_sequences_original_order.tsv", "initial_clusters.tsv")


@pytest.mark.gpu
def test_cli_sweep_on_musi(gpu, tmp_path):
    fa = os.path.join(GOLDEN, "musi.fa")
    d = inp("musi")
    levels = make_ctx("musi", 0).greedy_sweep(d["X"], d["p"], 20, 30, d["maxc"], arrays=False)[0]
    rows = ["threshold\tedges\tstatus\tclusters\tmulti_member\tsingletons\tlargest\tphase1_stop_index"]
    for l, lv in enumerate(levels):
        assert lv["status"] == 0
        rows.append("\t".join(str(v) for v in [20 + l, int(lv["n_edges"]), "ok", int(lv["n_result_clusters"]), int(lv["n_multi"]),
                                               int(lv["n_singletons"]), int(lv["largest"]), int(lv["phase1_stop_index"])]))
    for pick in (None, 26):
        tag = "default" if pick is None else str(pick)
        r = cli("sweep", "-i", fa, "-d", str(tmp_path / ("s" + tag)), "-g", "20", "--scan_to", "30", *([] if pick is None else ["--pick", str(pick)]), timeout=600)
        assert r.returncode == 0, r.stderr
        g = cli("greedy", "-i", fa, "-d", str(tmp_path / ("g" + tag)), "-g", str(pick or 20), timeout=600)
        assert g.returncode == 0, g.stderr
        assert (tmp_path / ("s" + tag) / "greedy_levels.tsv").read_text() == "\n".join(rows) + "\n"
        for name in STAGE1:
            assert (tmp_path / ("s" + tag) / name).read_bytes() == (tmp_path / ("g" + tag) / name).read_bytes(), (tag, name)


@pytest.mark.gpu
def test_cli_sweep_at_a_pick_where_the_reference_would_throw(gpu, tmp_path):
    """AAAA has no neighbour at any of these thresholds and comes first (-R input): the reference throws at :104 (case 1, index 0).
    The levels file is written, the stage-1 files are not, the message and the exit status are greedy's."""
    fa = tmp_path / "three.fa"
    fa.write_text(">1\nAAAA\n>2\nRRRR\n>3\nRRRN\n")
    common = ["-i", str(fa), "-x", "0", "-R", "input", "--initial_clusters_limit", "2"]
    g = cli("greedy", *common, "-g", "8", "-d", str(tmp_path / "g"))
    r = cli("sweep", *common, "-g", "7", "--scan_to", "9", "--pick", "8", "-d", str(tmp_path / "s"))
    assert g.returncode == 4 == r.returncode, (g.stderr, r.stderr)
    message = [line for line in g.stderr.splitlines() if "NullPointerException" in line]
    assert message and "case 1 at index 0" in message[-1] and message == [line for line in r.stderr.splitlines() if "NullPointerException" in line]
    rows = (tmp_path / "s" / "greedy_levels.tsv").read_text().splitlines()
    assert len(rows) == 4 and all(row.startswith(f"{t}\t1\treference_would_crash:1\t") for t, row in zip((7, 8, 9), rows[1:]))
    assert not any((tmp_path / "s" / name).exists() for name in STAGE1)
