"""Complete-linkage scores inside given clusters: hmk_cluster_linkage_shifted (k_linkage.hip) and `hammock-hip check`.

CPU part (host-only context): the symbol, every argument check, DeviceError for a valid call, the mode's argument and file errors.
GPU part: all six outputs and the statistics against the C oracle's score_pairs over the enumerated pairs inside every slot,
reduced with numpy (seq1 = the pair's larger index); the oracle's side of every case is computed once and shared.  The sized
families hold one slot more than every boundary of the kernels' paths:
    LINK_FLAT_MAX = 256   slots of up to 256 members are enumerated flat, a lane per pair: slots of 256 and of 257 members
    LINK_TILE = 256       larger slots in tiles of 256 rows x 256 columns: 257 members are two row blocks, 513 are three
    64, 256               a wave and a block of the flat pair space, a wave of a tile's columns: slots of 63, 64, 65 members, and the
                          22 slots' pair counts put slot boundaries inside waves and chunks
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from conftest import GOLDEN
from test_assign import gpu   # noqa: F401  (the fixture that skips where no HIP device is visible)
from test_continue import cli, read_cluster_file

import hammock_amd
from hammock_amd import _native as N

INT32_MAX, UINT32_MAX = 2 ** 31 - 1, 2 ** 32 - 1
SIZES = [1, 2, 3, 5, 17, 63, 64, 65, 130, 257, 700]
BOUNDARY_SIZES = [256, 513]   # LINK_FLAT_MAX itself (257 is in SIZES), two tiles and one member


def _blosum62():
    import json
    with open(os.path.join(GOLDEN, "matrices.json")) as fh:
        return np.asarray(json.load(fh)["matrices"]["blosum62"], dtype=np.int32)


# ---- inputs ----------------------------------------------------------------------------------------------------------------

def sized_families(seed):
    """22 slots, two sets of SIZES members around a random centre each -- at most 2 substitutions in the first set, at most 5 in the
    second -- and one slot per BOUNDARY_SIZES (at most 2); all strings distinct, members shuffled so that no slot is contiguous.
    Even seeds: 12-mers, X = 3, p = 0, threshold 20.  Odd seeds: centres of 10-12 residues with an end residue dropped from every
    third member (lengths 9-12), X = 2, p = -1, threshold 14.  -> (peptides, member_cluster, n_clusters, X, p, threshold)"""
    rng = np.random.default_rng(88_000 + seed)
    mixed = seed % 2 == 1
    peps, mc, seen = [], [], set()
    plan = [(s, 2) for s in SIZES] + [(s, 5) for s in SIZES] + [(s, 2) for s in BOUNDARY_SIZES]
    for c, (size, max_sub) in enumerate(plan):
        centre = rng.integers(0, 20, size=int(rng.integers(10, 13)) if mixed else 12).astype(np.uint8)
        added = 0
        while added < size:
            q = centre.copy()
            for pos in rng.choice(len(q), size=int(rng.integers(0, max_sub + 1)), replace=False):
                q[pos] = rng.integers(0, 20)
            if mixed and added % 3 == 2:
                q = q[1:] if rng.integers(0, 2) else q[:-1]
            if q.tobytes() in seen:
                continue
            seen.add(q.tobytes())
            peps.append(q)
            mc.append(c)
            added += 1
    perm = rng.permutation(len(peps))
    peps = [peps[k] for k in perm]
    mc = np.asarray(mc, dtype=np.uint32)[perm]
    return (peps, mc, len(plan)) + ((2, -1, 14) if mixed else (3, 0, 20))


def inside_pairs(mc, r0=0):
    """the unordered pairs inside every slot -> (a, b, slot) with a < b, indices of the uploaded set"""
    mc = np.asarray(mc, dtype=np.int64)
    aa, bb, ss = [], [], []
    for c in np.unique(mc):
        m = np.flatnonzero(mc == c) + r0
        if m.size < 2:
            continue
        i, j = np.triu_indices(m.size, 1)
        aa.append(m[i])
        bb.append(m[j])
        ss.append(np.full(i.size, c, dtype=np.int64))
    if not aa:
        z = np.zeros(0, dtype=np.int64)
        return z, z, z
    return np.concatenate(aa), np.concatenate(bb), np.concatenate(ss)


def score_inside(coracle, M, res, off, mc, X, p, r0=0):
    a, b, slot = inside_pairs(mc, r0)
    st, sc = coracle.score_pairs(M, res, off, b, a, 0, X, p)   # seq1 = the larger index
    assert st == 0
    return a, b, slot, sc.astype(np.int64)


def reduce_scores(a, b, slot, sc, nm, ncl, thr, r0=0):
    """the six outputs and (pairs_scored, n_multi, n_violating) from the scored pairs, in numpy"""
    min_score = np.full(ncl, INT32_MAX, dtype=np.int64)
    min_a = np.full(ncl, UINT32_MAX, dtype=np.int64)
    min_b = np.full(ncl, UINT32_MAX, dtype=np.int64)
    order = np.lexsort((b, a, sc, slot))   # by slot, then score, then a, then b
    first = order[np.r_[True, slot[order][1:] != slot[order][:-1]]] if order.size else order
    min_score[slot[first]] = sc[first]
    min_a[slot[first]] = a[first]
    min_b[slot[first]] = b[first]
    low = sc < thr
    n_below = np.bincount(slot, weights=low, minlength=ncl).astype(np.int64)
    member_min = np.full(nm, INT32_MAX, dtype=np.int64)
    np.minimum.at(member_min, a - r0, sc)
    np.minimum.at(member_min, b - r0, sc)
    member_below = np.bincount(a - r0, weights=low, minlength=nm) + np.bincount(b - r0, weights=low, minlength=nm)
    stats = (int(sc.size), int(np.unique(slot).size), int((n_below > 0).sum()))
    return (min_score, min_a, min_b, n_below, member_min, member_below.astype(np.int64)), stats


def check(got, want, ctx=None, stats=None):
    for g, w, name in zip(got, want, ("min_score", "min_a", "min_b", "n_below", "member_min", "member_below")):
        if g is None:
            continue
        assert np.array_equal(np.asarray(g, dtype=np.int64), w), name
    if stats is not None:
        s = ctx.last_linkage_stats
        assert (s.pairs_scored, s.n_multi, s.n_violating) == stats


@functools.lru_cache(maxsize=None)
def sized_case(seed):
    """a sized-families input, packed, with the oracle's scores of its inside pairs (computed once per session)"""
    from oracle import c_oracle
    peps, mc, ncl, X, p, thr = sized_families(seed)
    res, off = hammock_amd.pack_sequences(peps)
    M = _blosum62()
    scored = score_inside(c_oracle, M, res, off, mc, X, p)
    for arr in (res, off, mc) + scored:
        arr.setflags(write=False)
    return M, res, off, mc, ncl, X, p, thr, scored


def device_ctx(M, res, off, device=0):
    ctx = hammock_amd.Context(M, device=device)
    ctx.set_sequences(residues=res, offsets=off)
    return ctx


# ---- CPU: the symbol, the checks -------------------------------------------------------------------------------------------

def test_symbol_is_declared_bound_and_exported():
    with open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "hammock_hip.h")) as fh:
        header = fh.read()
    assert "int hmk_cluster_linkage_shifted(hmk_ctx *ctx" in header and "} hmk_linkage_stats;" in header
    assert "hmk_cluster_linkage_shifted" in N.SYMBOLS
    assert hasattr(N.lib, "hmk_cluster_linkage_shifted")
    assert N.lib.hmk_abi_version() == 4
    assert C.sizeof(N.LinkageStats) == 32


def _raw_call(ctx, r0, r1, mc, ncl, X, p, thr, null=()):
    """the C entry point with chosen arguments null -> status"""
    nm = max(r1 - r0, 1)
    mc = None if mc is None else np.ascontiguousarray(mc, dtype=np.uint32)
    out = {"min_score": np.zeros(max(ncl, 1), np.int32), "min_a": np.zeros(max(ncl, 1), np.uint32), "min_b": np.zeros(max(ncl, 1), np.uint32),
           "n_below": np.zeros(max(ncl, 1), np.uint64), "member_min": np.zeros(nm, np.int32), "member_below": np.zeros(nm, np.uint32)}
    types = {"min_score": C.c_int32, "min_a": C.c_uint32, "min_b": C.c_uint32, "n_below": C.c_uint64, "member_min": C.c_int32,
             "member_below": C.c_uint32}
    ptr = [None if k in null else out[k].ctypes.data_as(C.POINTER(types[k])) for k in types]
    return N.lib.hmk_cluster_linkage_shifted(ctx._h, r0, r1, None if mc is None else mc.ctypes.data_as(C.POINTER(C.c_uint32)), ncl, X, p, thr,
                                             *ptr, None)


def test_host_only_context_answers_every_bad_argument(blosum62):
    rng = np.random.default_rng(5)
    peps = [rng.integers(0, 20, size=12).astype(np.uint8) for _ in range(6)]
    res, off = hammock_amd.pack_sequences(peps)
    ctx = hammock_amd.Context(blosum62, device=-1)
    ctx.set_sequences(residues=res, offsets=off)
    mc = [0, 0, 1, 1, 2, 2]
    bad = N.HMK_ERR_BAD_ARG
    # the range and slot checks of hmk_cluster_pairs_shifted
    assert _raw_call(ctx, 4, 2, mc[:2], 1, 3, 0, 20) == bad                      # r0 > r1
    assert _raw_call(ctx, 0, 7, mc + [2], 3, 3, 0, 20) == bad                    # r1 > n
    assert _raw_call(ctx, 0, 6, [0, 0, 1, 1, 3, 3], 3, 3, 0, 20) == bad          # a slot at or above n_clusters
    assert _raw_call(ctx, 0, 6, [0, 0, 1, 1, 1, 1], 3, 3, 0, 20) == bad          # a slot without a member
    assert _raw_call(ctx, 0, 6, None, 3, 3, 0, 20) == bad                        # null member_cluster, non-empty range
    for name in ("min_score", "min_a", "min_b", "n_below"):                      # a null required output
        assert _raw_call(ctx, 0, 6, mc, 3, 3, 0, 20, null=(name,)) == bad
        assert name in N.lib.hmk_last_error(ctx._h).decode() or "null output" in N.lib.hmk_last_error(ctx._h).decode()
    assert _raw_call(ctx, 0, 6, mc, 3, 3, 0, 20, null=("member_min",)) == bad    # the optional pair comes together
    with pytest.raises(ValueError):
        ctx.cluster_linkage_shifted(0, 6, [0, 0, 1, 1, 3, 3], 3, 3, 0, 20)
    # an asymmetric matrix
    A = blosum62.copy()
    A[0, 1] += 1
    actx = hammock_amd.Context(A, device=-1)
    actx.set_sequences(residues=res, offsets=off)
    with pytest.raises(ValueError, match="symmetric"):
        actx.cluster_linkage_shifted(0, 6, mc, 3, 3, 0, 20)
    # a valid call: no CPU fallback, with or without the member outputs, and for the inner range too
    assert _raw_call(ctx, 0, 6, mc, 3, 3, 0, 20) == N.HMK_ERR_DEVICE
    assert _raw_call(ctx, 0, 6, mc, 3, 3, 0, 20, null=("member_min", "member_below")) == N.HMK_ERR_DEVICE
    with pytest.raises(hammock_amd.DeviceError):
        ctx.cluster_linkage_shifted(0, 6, mc, 3, 3, 0, 20)
    with pytest.raises(hammock_amd.DeviceError):
        ctx.cluster_linkage_shifted(2, 6, [0, 0, 1, 1], 2, 3, 0, 20, members=False)


def test_cli_check_argument_and_file_errors(tmp_path):
    r = cli("check", "-d", str(tmp_path / "a"))
    assert r.returncode == 2 and "-i or --input" in r.stderr
    assert not (tmp_path / "a").exists()
    good = tmp_path / "good.tsv"
    good.write_text("cluster_id\tsequence\tno_label\n1\tWVTAPRSLPVLP\t1\n1\tWVTAPRSLPVLA\t1\n")
    r = cli("check", "-i", str(good), "--devices", "0,1", "-d", str(tmp_path / "b"))
    assert r.returncode == 2 and "--devices" in r.stderr
    na = tmp_path / "na.tsv"
    na.write_text("cluster_id\tsequence\tno_label\n1\tWVTAPRSLPVLP\t1\nNA\tWVTAPRSLPVLA\t1\n")
    r = cli("check", "-i", str(na), "-d", str(tmp_path / "c"))
    assert r.returncode == 2 and "FileFormatException" in r.stderr
    short = tmp_path / "short.tsv"
    short.write_text("cluster_id\n1\n")
    r = cli("check", "-i", str(short), "-d", str(tmp_path / "d"))
    assert r.returncode == 2 and "FileFormatException" in r.stderr
    r = cli("check", "-i", str(good), "-d", str(tmp_path / "c"))   # the directory exists now
    assert r.returncode == 2 and "Output directory exists" in r.stderr


# ---- GPU -------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2, 3, 4])   # (12-mers: 2 and 4; of the even seeds 0-12 the oracle gives 0 and 8 only 7 violating slots)
def test_sized_families_match_the_oracle(gpu, seed):
    """test 1: all six outputs and the statistics on 24 slots of 1 ... 700 members (3,383 sequences, 748,228 pairs)"""
    M, res, off, mc, ncl, X, p, thr, (a, b, slot, sc) = sized_case(seed)
    nm = mc.size
    assert nm == 2 * sum(SIZES) + sum(BOUNDARY_SIZES) and sc.size == 2 * 292_130 + 32_640 + 131_328
    assert all(np.ptp(np.flatnonzero(mc == c)) + 1 > (mc == c).sum() for c in range(ncl) if (mc == c).sum() > 1)   # no slot is contiguous
    want, stats = reduce_scores(a, b, slot, sc, nm, ncl, thr)
    # the oracle's side alone: the case cannot pass vacuously
    multi = np.bincount(mc, minlength=ncl) > 1
    assert (multi & (want[3] == 0)).sum() >= 8 and (want[3] > 0).sum() >= 8
    ties = [int((sc[slot == c] == want[0][c]).sum()) for c in range(ncl) if multi[c]]
    assert max(ties) >= 2
    assert want[0].min() < 0
    ctx = device_ctx(M, res, off)
    got = ctx.cluster_linkage_shifted(0, nm, mc, ncl, X, p, thr)
    check(got, want, ctx, stats)
    assert got[0].dtype == np.int32 and got[3].dtype == np.uint64 and got[5].dtype == np.uint32
    assert ctx.last_linkage_stats.launches == 3 and ctx.last_linkage_stats.kernel_ms > 0


@pytest.mark.gpu
def test_threshold_edge(gpu):
    """test 2: a pair scoring exactly the threshold is not below it"""
    M, res, off, mc, ncl, X, p, thr, (a, b, slot, sc) = sized_case(2)
    want, _ = reduce_scores(a, b, slot, sc, mc.size, ncl, thr)
    ctx = device_ctx(M, res, off)
    for c in (int(np.flatnonzero(np.bincount(mc) == 700)[1]), int(np.flatnonzero(np.bincount(mc) == 65)[1])):   # a tiled slot, a flat one
        lowest = int(want[0][c])
        attained = int((sc[slot == c] == lowest).sum())
        at = ctx.cluster_linkage_shifted(0, mc.size, mc, ncl, X, p, lowest)
        assert at[3][c] == 0 and at[0][c] == lowest
        check(at, reduce_scores(a, b, slot, sc, mc.size, ncl, lowest)[0])
        above = ctx.cluster_linkage_shifted(0, mc.size, mc, ncl, X, p, lowest + 1)
        assert above[3][c] == attained >= 1
        check(above, reduce_scores(a, b, slot, sc, mc.size, ncl, lowest + 1)[0])


@pytest.mark.gpu
def test_state_between_calls(gpu, coracle):
    """test 3: one context, calls with another slot assignment, another threshold and an inner range; nothing stays behind"""
    rng = np.random.default_rng(88_100)
    M = _blosum62()
    centre = rng.integers(0, 20, size=12).astype(np.uint8)
    peps, seen = [], set()
    while len(peps) < 700:
        q = centre.copy()
        for pos in rng.choice(12, size=int(rng.integers(0, 5)), replace=False):
            q[pos] = rng.integers(0, 20)
        if q.tobytes() not in seen:
            seen.add(q.tobytes())
            peps.append(q)
    res, off = hammock_amd.pack_sequences(peps)
    n = len(peps)
    ctx = device_ctx(M, res, off)

    def slots(sizes, count):
        mc = np.repeat(np.arange(len(sizes)), sizes)
        assert mc.size == count
        return rng.permutation(mc).astype(np.uint32)

    def run(r0, r1, mc, thr, **kw):
        ncl = int(mc.max()) + 1
        a, b, slot, sc = score_inside(coracle, M, res, off, mc, 3, 0, r0)
        want, stats = reduce_scores(a, b, slot, sc, r1 - r0, ncl, thr, r0)
        got = ctx.cluster_linkage_shifted(r0, r1, mc, ncl, 3, 0, thr, **kw)
        check(got, want, ctx, stats)
        return got

    mc_a = slots([300, 260, 64, 40, 20, 9, 3, 2, 1, 1], n)
    mc_b = slots([1, 350, 2, 257, 60, 30], n)
    mc_c = slots([270, 100, 1, 27, 2], 400)
    first = run(0, n, mc_a, 20)
    run(0, n, mc_b, 20)                  # a different slot assignment
    run(0, n, mc_a, 31)                  # a different threshold
    run(150, 550, mc_c, 20)              # a range in the middle of the uploaded set
    again = run(0, n, mc_a, 20)
    assert all(np.array_equal(x, y) for x, y in zip(first, again))
    perm = rng.permutation(10)
    moved = run(0, n, perm[mc_a].astype(np.uint32), 20)
    for x, y in zip(first[:4], moved[:4]):
        assert np.array_equal(x, y[perm])
    assert np.array_equal(first[4], moved[4]) and np.array_equal(first[5], moved[5])
    bare = run(0, n, mc_a, 20, members=False)
    assert bare[4] is None and bare[5] is None
    assert all(np.array_equal(x, y) for x, y in zip(first[:4], bare[:4]))


@pytest.mark.gpu
def test_halves_agree_with_cluster_pairs(gpu):
    """test 4, no oracle: a slot split into halves -- where hmk_cluster_pairs_shifted calls the halves feasible for each other
    the whole's minimum is the minimum of the halves' and the pair's, and the counts add up; where not, the whole holds more pairs
    below the threshold than the halves together"""
    M, res, off, mc, ncl, X, p, thr, _ = sized_case(2)
    nm = mc.size
    ctx = device_ctx(M, res, off)
    whole = ctx.cluster_linkage_shifted(0, nm, mc, ncl, X, p, thr)
    place = np.zeros(nm, dtype=np.int64)   # the member's place inside its slot
    for c in range(ncl):
        m = np.flatnonzero(mc == c)
        place[m] = np.arange(m.size)
    half_raw = 2 * mc.astype(np.int64) + (place % 2)
    ids, half = np.unique(half_raw, return_inverse=True)
    half = half.astype(np.uint32)
    halves = ctx.cluster_linkage_shifted(0, nm, half, ids.size, X, p, thr)
    pairs = ctx.cluster_pairs_shifted(0, nm, half, ids.size, X, p, thr)
    x, m, score = hammock_amd.edge_fields(pairs)
    between = {(int(i), int(j)): int(s) for i, j, s in zip(x, m, score)}
    slot_of = {int(raw): k for k, raw in enumerate(ids)}
    feasible = infeasible = 0
    for c in range(ncl):
        if (mc == c).sum() < 2:
            continue
        h0, h1 = slot_of[2 * c], slot_of[2 * c + 1]
        below = int(halves[3][h0]) + int(halves[3][h1])
        if (h0, h1) in between:
            feasible += 1
            assert int(whole[0][c]) == min(int(halves[0][h0]), int(halves[0][h1]), between[(h0, h1)])
            assert int(whole[3][c]) == below
        else:
            infeasible += 1
            assert int(whole[3][c]) > below
    assert feasible >= 4 and infeasible >= 4


def _musi():
    with open(os.path.join(GOLDEN, "musi.fa")) as fh:
        return [line.strip() for line in fh if line.strip() and not line.startswith(">")]


@pytest.mark.gpu
def test_clusters_of_the_clustering_calls_are_complete_linkage_clusters(gpu):
    """test 4, second half: what hmk_greedy_cluster and hmk_clinkage_cluster return passes the check at their own parameters"""
    M = _blosum62()
    seqs = list(dict.fromkeys(_musi()))
    for name, count in (("greedy", len(seqs)), ("clinkage", 1000)):
        res, off = hammock_amd.pack_sequences(seqs[:count])
        ctx = device_ctx(M, res, off)
        cid = ctx.greedy_cluster(3, 0, 20, 2 ** 31 - 1)[0] if name == "greedy" else ctx.clinkage_cluster(3, 0, 20)[0]
        _, mc = np.unique(cid, return_inverse=True)
        ncl = int(mc.max()) + 1
        got = ctx.cluster_linkage_shifted(0, count, mc, ncl, 3, 0, 20)
        multi = np.bincount(mc) > 1
        assert multi.sum() > 20, name
        assert (got[3] == 0).all() and (got[0][multi] >= 20).all(), name
        assert (got[0][~multi] == INT32_MAX).all() and (got[5] == 0).all()
        assert ctx.last_linkage_stats.n_violating == 0 and ctx.last_linkage_stats.n_multi == multi.sum()


@pytest.mark.gpu
def test_singletons_and_degenerate_inputs(gpu, coracle):
    """test 5"""
    M, res, off, mc, ncl, X, p, thr, _ = sized_case(2)
    ctx = device_ctx(M, res, off)
    # singletons only
    got = ctx.cluster_linkage_shifted(10, 60, np.arange(50), 50, X, p, thr)
    assert (got[0] == INT32_MAX).all() and (got[1] == UINT32_MAX).all() and (got[2] == UINT32_MAX).all() and (got[3] == 0).all()
    assert (got[4] == INT32_MAX).all() and (got[5] == 0).all()
    s = ctx.last_linkage_stats
    assert (s.pairs_scored, s.n_multi, s.n_violating, s.launches) == (0, 0, 0, 0)
    # an empty range
    got = ctx.cluster_linkage_shifted(7, 7, [], 0, X, p, thr)
    assert all(g.size == 0 for g in got) and ctx.last_linkage_stats.pairs_scored == 0
    got = ctx.cluster_linkage_shifted(7, 7, [], 0, X, p, thr, members=False)
    assert got[4] is None and got[0].size == 0
    # one slot holding everything, 300 members
    one = np.zeros(300, dtype=np.uint32)
    a, b, slot, sc = score_inside(coracle, M, res, off, one, X, p, 500)
    want, stats = reduce_scores(a, b, slot, sc, 300, 1, thr, 500)
    check(ctx.cluster_linkage_shifted(500, 800, one, 1, X, p, thr), want, ctx, stats)
    assert stats[0] == 300 * 299 // 2


def _java_round(v):
    import math
    return int(math.floor(v + 0.5))


@pytest.mark.gpu
def test_cli_check_on_greedy_clusters(gpu, coracle, tmp_path):
    """test 6: `check` on greedy's stage-1 file of MUSI writes what the oracle's numbers say, byte for byte; with one sequence moved
    into another cluster the report names that cluster and that sequence"""
    r = cli("greedy", "-i", os.path.join(GOLDEN, "musi.fa"), "-d", str(tmp_path / "g"), timeout=600)
    assert r.returncode == 0, r.stderr
    cfile = tmp_path / "g" / "initial_clusters_sequences.tsv"
    M = _blosum62()

    def expectation(path, skip):
        loaded = read_cluster_file(path)   # (cluster id, sequence, size) per line
        ids = list(dict.fromkeys(c for c, _, _ in loaded))
        slot = {c: k for k, c in enumerate(ids)}
        mc = np.array([slot[c] for c, _, _ in loaded], dtype=np.uint32)
        seqs = [s for _, s, _ in loaded]
        size = np.bincount(mc, weights=[z for _, _, z in loaded]).astype(np.int64)
        lens = [len(s) for s in seqs]
        X = min(_java_round(sum(lens) / len(lens) / 4), min(lens) - 1)
        thr = _java_round(sum(lens) / len(lens) * 1.7)
        res, off = hammock_amd.pack_sequences(seqs)
        a, b, sl, sc = score_inside(coracle, M, res, off, mc, X, 0)
        (mn, ma, mb, nb, mmin, mbelow), stats = reduce_scores(a, b, sl, sc, len(seqs), len(ids), thr)
        uniq = np.bincount(mc)
        link = ["cluster_id\tunique_size\tsize\tlinkage_score\tpairs_below\tworst_sequence_1\tworst_sequence_2"]
        for k, c in enumerate(ids):
            if uniq[k] == 1:
                if not skip:
                    link.append(f"{c}\t1\t{size[k]}\tNA\t0\tNA\tNA")
            else:
                link.append(f"{c}\t{uniq[k]}\t{size[k]}\t{mn[k]}\t{nb[k]}\t{seqs[ma[k]]}\t{seqs[mb[k]]}")
        memb = ["cluster_id\tsequence\tmin_score\tpairs_below"]
        memb += [f"{ids[mc[k]]}\t{seqs[k]}\t{mmin[k]}\t{mbelow[k]}" for k in range(len(seqs)) if uniq[mc[k]] > 1]
        worst = int(np.argmin(mn))   # (the first of equal minima, as the mode reports)
        last = f"{stats[2]} of {len(ids)} clusters hold a pair below the threshold {thr}; lowest linkage score {mn[worst]} (cluster {ids[worst]})"
        return "\n".join(link) + "\n", "\n".join(memb) + "\n", last, X, thr, stats

    for extra in ([], ["--skip_singletons"]):
        out = tmp_path / ("c" + str(len(extra)))
        r = cli("check", "-i", str(cfile), "-d", str(out), *extra, timeout=600)
        assert r.returncode == 0, r.stderr
        link, memb, last, X, thr, stats = expectation(cfile, bool(extra))
        assert "Max shift not set. Setting automatically to: " + str(X) in r.stderr
        assert "Check threshold not set. Setting automatically to: " + str(thr) in r.stderr
        assert (out / "cluster_linkage.tsv").read_text() == link
        assert (out / "cluster_members.tsv").read_text() == memb
        assert (out / "run.log").read_text().rstrip("\n").endswith(last)
        assert stats[2] == 0 and stats[1] > 20 and last.startswith("0 of ")

    # one sequence of the largest cluster moved into the cluster whose members it fits worst
    lines = cfile.read_text().splitlines()
    rows = [l.split("\t") for l in lines[1:]]
    counts = {}
    for f in rows:
        counts[f[0]] = counts.get(f[0], 0) + 1
    big = sorted(counts, key=lambda c: -counts[c])[:2]
    moved = next(k for k, f in enumerate(rows) if f[0] == big[0])
    moved_seq = rows[moved][1]
    rows[moved][0] = big[1]
    bad = tmp_path / "moved.tsv"
    bad.write_text("\n".join([lines[0]] + ["\t".join(f) for f in rows]) + "\n")
    link, memb, last, X, thr, stats = expectation(bad, False)
    assert stats[2] == 1   # the oracle: exactly the cluster that took the stranger breaks
    r = cli("check", "-i", str(bad), "-d", str(tmp_path / "m"), "-x", str(X), "-g", str(thr), timeout=600)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "m" / "cluster_linkage.tsv").read_text() == link
    assert (tmp_path / "m" / "cluster_members.tsv").read_text() == memb
    broken = [l.split("\t") for l in (tmp_path / "m" / "cluster_linkage.tsv").read_text().splitlines()[1:] if l.split("\t")[4] != "0"]
    assert [f[0] for f in broken] == [big[1]] and moved_seq in broken[0][5:7]
    members = [l.split("\t") for l in (tmp_path / "m" / "cluster_members.tsv").read_text().splitlines()[1:]]
    stranger = [f for f in members if f[0] == big[1] and f[1] == moved_seq]
    assert len(stranger) == 1 and int(stranger[0][3]) == int(broken[0][4]) >= 1   # every pair below the threshold is one of the stranger's
    assert all(int(f[3]) <= 1 for f in members if f[1] != moved_seq)
    assert (tmp_path / "m" / "run.log").read_text().rstrip("\n").endswith(last) and last.startswith("1 of ")
