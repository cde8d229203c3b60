"""Splitting given clusters by complete linkage: hmk_clinkage_split (k_split.hip), hmk_clinkage_split_from_edges and `hammock-hip split`.

The expected answer is the C oracle's: per slot, clinkage_cluster on the slot's members packed alone in index order, with the
HashSet order set first; split_cluster follows from n_parts and part_order by the numbering rule (slots in slot order, inside a slot
its parts in list order).  The oracle's side of the sized families is computed once per (seed, threshold, Java order) and shared.
CPU part (host-only context): the symbols, _from_edges against the oracle on every output, sizes, the degenerate slot assignments,
crash parity, every argument check, the thread count, the mode's argument and file errors.
GPU part: the device call against _from_edges on the oracle's edges and against the oracle; the families hold slots of 1, 2, 3, 256,
257, 513 and 700 members -- both sides of LINK_FLAT_MAX, a diagonal tile with one member beyond two tiles, mixed lengths.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from conftest import GOLDEN
from test_assign import gpu   # noqa: F401  (the fixture that skips where no HIP device is visible)
from test_continue import cli, read_cluster_file
from test_linkage import device_ctx, inside_pairs, score_inside, sized_case, sized_families   # noqa: F401
from test_oracle import STACKED_AGAIN

import hammock_amd
from hammock_amd import _native as N

OUTPUTS = ("split_cluster", "n_parts", "part_id", "member_rank", "part_order")


def _matrix(name):
    import json
    with open(os.path.join(GOLDEN, "matrices.json")) as fh:
        return np.asarray(json.load(fh)["matrices"][name], dtype=np.int32)


# ---- the expectation -------------------------------------------------------------------------------------------------------

def oracle_split(M, res, off, mc, ncl, X, p, thr, java=8, sizes=None, r0=0):
    """-> (split_cluster, n_parts, part_id, member_rank, part_order lists) as the call returns them, or ("crash", slot) for the
    lowest slot on which the reference's chain returns to a stacked cluster"""
    from oracle import c_oracle
    mc = np.asarray(mc, dtype=np.int64)
    nm = mc.size
    n_parts = np.zeros(ncl, dtype=np.int64)
    local = np.zeros(nm, dtype=np.int64)
    part_id = np.zeros(nm, dtype=np.int64)
    rank = np.zeros(nm, dtype=np.int64)
    orders = []
    c_oracle.set_java_hashset(java)
    try:
        for c in range(ncl):
            m = np.flatnonzero(mc == c)
            r, o = hammock_amd.pack_sequences([res[off[r0 + i]:off[r0 + i + 1]] for i in m])
            sz = None if sizes is None else np.asarray(sizes, dtype=np.int32)[r0 + m]
            st, cid, order, rk, _ = c_oracle.clinkage_cluster(M, r, o, sz, X, p, thr)
            if st == c_oracle.HMO_ERR_REFERENCE_WOULD_CRASH:
                return ("crash", c)
            assert st == 0
            n_parts[c] = order.size
            place = {int(v): k for k, v in enumerate(order)}
            local[m] = [place[int(v)] for v in cid]
            part_id[m] = cid
            rank[m] = rk
            orders.append(np.asarray(order, dtype=np.int64))
    finally:
        c_oracle.set_java_hashset(8)
    base = np.concatenate([[0], np.cumsum(n_parts)])
    return base[mc] + local, n_parts, part_id, rank, orders


def same(got, want, what=""):
    for g, w, name in zip(got, want, OUTPUTS):
        if name == "part_order":
            assert len(g) == len(w), what + name
            assert all(np.array_equal(np.asarray(x, dtype=np.int64), y) for x, y in zip(g, w)), what + name
        else:
            assert np.array_equal(np.asarray(g, dtype=np.int64), w), what + name


@functools.lru_cache(maxsize=None)
def family_expect(seed, dthr, java):
    M, res, off, mc, ncl, X, p, thr, _ = sized_case(seed)
    want = oracle_split(M, res, off, mc, ncl, X, p, thr + dthr, java)
    assert not isinstance(want[0], str)   # (no slot of the families is a crash case at these thresholds: no test leaves a slot out)
    return want


def inside_edges(scored, thr):
    a, b, _, sc = scored
    keep = sc >= thr
    return hammock_amd.pack_edges(a[keep], b[keep], sc[keep])   # x = the smaller index, m = the larger, score(seq1 = m, seq2 = x)


def numpy_stats(mc, ncl, scored, thr):
    """(pairs_scored, n_edges, n_multi, n_split) from the oracle's scores alone"""
    _, _, slot, sc = scored
    below = np.bincount(slot[sc < thr], minlength=ncl)
    return int(sc.size), int((sc >= thr).sum()), int((np.bincount(mc, minlength=ncl) > 1).sum()), int((below > 0).sum())


def host_ctx(M, res, off, sizes=None, java=8):
    ctx = hammock_amd.Context(M, device=-1)
    ctx.set_sequences(residues=res, offsets=off, sizes=sizes)
    assert N.lib.hmk_set_java_hashset(ctx._h, java) == 0
    return ctx


# ---- CPU: the symbols ------------------------------------------------------------------------------------------------------

def test_symbols_are_declared_bound_and_exported():
    with open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "hammock_hip.h")) as fh:
        header = fh.read()
    assert "int hmk_clinkage_split(hmk_ctx *ctx" in header and "int hmk_clinkage_split_from_edges(hmk_ctx *ctx" in header
    assert "} hmk_split_stats;" in header
    for name in ("hmk_clinkage_split", "hmk_clinkage_split_from_edges"):
        assert name in N.SYMBOLS and hasattr(N.lib, name)
    assert N.lib.hmk_abi_version() == 4
    assert C.sizeof(N.SplitStats) == 64


# ---- CPU: _from_edges against the oracle -----------------------------------------------------------------------------------

@pytest.mark.parametrize("java", [8, 7, 6])
@pytest.mark.parametrize("dthr", [0, 6])
@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_from_edges_equals_the_oracle(seed, dthr, java):
    """every output on 24 slots of 1 ... 700 members; edges between slots and edges with an end outside the range change nothing;
    n_parts[c] == 1 <=> the oracle's scores show no pair of slot c below the threshold"""
    M, res, off, mc, ncl, X, p, thr, scored = sized_case(seed)
    thr += dthr
    nm = mc.size
    want = family_expect(seed, dthr, java)
    rng = np.random.default_rng(90_000 + seed)
    extra = [rng.integers(0, 20, size=12).astype(np.uint8) for _ in range(5)]   # five sequences behind the range
    res2, off2 = hammock_amd.pack_sequences([res[off[i]:off[i + 1]] for i in range(nm)] + extra)
    ctx = host_ctx(M, res2, off2, java=java)
    edges = inside_edges(scored, thr)
    got = ctx.clinkage_split_from_edges(edges, 0, nm, mc, ncl)
    same(got, want)
    s = ctx.last_split_stats
    stats = numpy_stats(mc, ncl, scored, thr)
    assert (s.pairs_scored, s.n_edges, s.n_multi, s.n_split) == (0,) + stats[1:]
    assert s.n_result_clusters == int(want[1].sum()) == int(want[0].max()) + 1 and s.crash_slot == -1 and s.merges == nm - s.n_result_clusters
    # the oracle's side alone: the case cannot pass vacuously
    assert (want[1] > 1).sum() >= 4 and want[1].max() >= 10
    _, _, slot, sc = scored
    below = np.bincount(slot[sc < thr], minlength=ncl) > 0
    assert np.array_equal(want[1] == 1, ~below)
    # edges that must be ignored: ends in two slots, an end outside [0, nm)
    x = rng.integers(0, nm, size=4000)
    m = rng.integers(0, nm, size=4000)
    cross = mc[x] != mc[m]
    lo, hi = np.minimum(x, m)[cross], np.maximum(x, m)[cross]
    outside = hammock_amd.pack_edges(rng.integers(0, nm, size=200), nm + rng.integers(0, 5, size=200), np.full(200, 60))
    noisy = np.concatenate([hammock_amd.pack_edges(lo, hi, np.full(lo.size, 60)), edges, outside])
    assert cross.sum() > 1000
    same(ctx.clinkage_split_from_edges(rng.permutation(noisy), 0, nm, mc, ncl), want, "noisy ")
    assert ctx.last_split_stats.n_edges == stats[1]


@pytest.mark.parametrize("seed,size_seed,crashes", [(1, 0, False), (2, 0, True), (2, 1, False)])
def test_from_edges_with_sizes(seed, size_seed, crashes):
    """non-unit sizes reach Cluster.size(), the tie-break after the score -- which can also make a slot a crash case: with the
    first sizes, a slot of seed 2 is one in the oracle, and the call names it"""
    M, res, off, mc, ncl, X, p, thr, scored = sized_case(seed)
    sizes = np.random.default_rng(90_100 + seed + 10 * size_seed).integers(1, 6, size=mc.size).astype(np.int32)
    want = oracle_split(M, res, off, mc, ncl, X, p, thr, sizes=sizes)
    ctx = host_ctx(M, res, off, sizes=sizes)
    assert isinstance(want[0], str) == crashes
    if crashes:
        with pytest.raises(hammock_amd.ReferenceWouldCrash) as info:
            ctx.clinkage_split_from_edges(inside_edges(scored, thr), 0, mc.size, mc, ncl)
        assert info.value.index == want[1] and np.bincount(mc)[want[1]] > 256
        return
    same(ctx.clinkage_split_from_edges(inside_edges(scored, thr), 0, mc.size, mc, ncl), want)
    plain = family_expect(seed, 0, 8)
    assert not np.array_equal(plain[2], want[2]) or not np.array_equal(plain[0], want[0])   # the sizes decided something


def test_one_slot_is_clinkage_from_edges_and_singletons_are_the_identity(coracle):
    M, res, off, mc, ncl, X, p, thr, scored = sized_case(2)
    c = int(np.argmax(family_expect(2, 0, 8)[1]))   # the slot that splits into most parts
    m = np.flatnonzero(mc == c)
    place = np.full(mc.size, -1, dtype=np.int64)
    place[m] = np.arange(m.size)
    a, b, slot, sc = scored
    keep = (slot == c) & (sc >= thr)
    edges = hammock_amd.pack_edges(place[a[keep]], place[b[keep]], sc[keep])
    r, o = hammock_amd.pack_sequences([res[off[i]:off[i + 1]] for i in m])
    ctx = host_ctx(M, r, o)
    cid, order, _ = ctx.clinkage_from_edges(edges)
    cid, order, rank = cid.copy(), order.copy(), ctx.member_rank[:m.size].copy()
    split, n_parts, part_id, member_rank, part_order = ctx.clinkage_split_from_edges(edges, 0, m.size, np.zeros(m.size), 1)
    assert np.array_equal(part_id, cid) and np.array_equal(part_order[0], order) and np.array_equal(member_rank, rank)
    assert n_parts.tolist() == [order.size] and order.size > 10 and m.size > 256
    assert np.array_equal(split, [order.tolist().index(v) for v in cid])
    # one slot per sequence: the identity, whatever the edges say
    split, n_parts, part_id, member_rank, part_order = ctx.clinkage_split_from_edges(edges, 0, m.size, np.arange(m.size), m.size)
    assert np.array_equal(split, np.arange(m.size)) and (n_parts == 1).all() and (part_id == 1).all() and (member_rank == 0).all()
    assert all(x.tolist() == [1] for x in part_order)
    s = ctx.last_split_stats
    assert (s.n_edges, s.n_multi, s.n_split, s.n_result_clusters, s.merges) == (0, 0, 0, m.size, 0)
    # an empty range: nothing to do
    got = ctx.clinkage_split_from_edges(edges, 5, 5, [], 0)
    assert all(len(g) == 0 for g in got)


# ---- CPU: crash parity -----------------------------------------------------------------------------------------------------

HEALTHY_A = ["WWWWWW", "WWWWWC", "WWWCWW"]
HEALTHY_B = ["CCCCCC", "CCCCCW"]
# slots 0 and 2 healthy, 1 and 3 the four peptides of STACKED_AGAIN in their order; no slot contiguous
CRASH_LAYOUT = [(0, 0), (1, 0), (3, 0), (0, 1), (1, 1), (2, 0), (3, 1), (1, 2), (3, 2), (2, 1), (1, 3), (0, 2), (3, 3)]


def crash_case(slots_with_stack):
    source = {0: HEALTHY_A, 1: STACKED_AGAIN, 2: HEALTHY_B, 3: STACKED_AGAIN}
    keep = [(c, k) for c, k in CRASH_LAYOUT if c in (0, 2) or c in slots_with_stack]
    ids = sorted({c for c, _ in keep})
    seqs = [source[c][k] for c, k in keep]
    mc = np.array([ids.index(c) for c, _ in keep], dtype=np.uint32)
    res, off = hammock_amd.pack_sequences(seqs)
    return res, off, mc, len(ids), [ids.index(c) for c in slots_with_stack]


@pytest.mark.parametrize("stacked", [(1,), (3,), (1, 3)])
def test_crash_parity_names_the_lowest_slot(coracle, stacked):
    """the four 6-mers of tests/test_oracle.py (BLOSUM75, X = 2, p = -2, threshold 19) as one slot among healthy ones, and as two"""
    M = _matrix("blosum75")
    res, off, mc, ncl, bad = crash_case(stacked)
    assert oracle_split(M, res, off, mc, ncl, 2, -2, 19) == ("crash", bad[0])
    a, b, slot, sc = score_inside(coracle, M, res, off, mc, 2, -2)
    ctx = host_ctx(M, res, off)
    with pytest.raises(hammock_amd.ReferenceWouldCrash) as info:
        ctx.clinkage_split_from_edges(inside_edges((a, b, slot, sc), 19), 0, mc.size, mc, ncl)
    assert info.value.index == bad[0] and ("slot %d" % bad[0]) in str(info.value) and "still on its stack" in str(info.value)
    # at threshold 25 the same input succeeds: TTKFVE and DTKFVE stay alone, QTKFVE + ETKFVE merge (ids 1, 2, 6, 6)
    want = oracle_split(M, res, off, mc, ncl, 2, -2, 25)
    got = ctx.clinkage_split_from_edges(inside_edges((a, b, slot, sc), 25), 0, mc.size, mc, ncl)
    same(got, want)
    for c in bad:
        assert got[2][mc == c].tolist() == [1, 2, 6, 6]


# ---- CPU: the checks -------------------------------------------------------------------------------------------------------

def _raw(ctx, r0, r1, mc, ncl, X=3, p=0, thr=20, null=(), edges=None):
    """the C entry points with chosen arguments null -> status (edges given: hmk_clinkage_split_from_edges)"""
    nm = max(r1 - r0, 1)
    mc = None if mc is None else np.ascontiguousarray(mc, dtype=np.uint32)
    out = {"split_cluster": np.zeros(nm, np.uint32), "n_parts": np.zeros(max(ncl, 1), np.uint32), "part_id": np.zeros(nm, np.int32),
           "member_rank": np.zeros(nm, np.int32), "part_order": np.zeros(nm, np.int32), "part_start": np.zeros(ncl + 1, np.uint32)}
    types = {"split_cluster": C.c_uint32, "n_parts": C.c_uint32, "part_id": C.c_int32, "member_rank": C.c_int32, "part_order": C.c_int32,
             "part_start": C.c_uint32}
    ptr = [None if k in null else out[k].ctypes.data_as(C.POINTER(types[k])) for k in types]
    mcp = None if mc is None else mc.ctypes.data_as(C.POINTER(C.c_uint32))
    if edges is None:
        st = N.lib.hmk_clinkage_split(ctx._h, r0, r1, mcp, ncl, X, p, thr, *ptr, None)
    else:
        edges = np.ascontiguousarray(edges, dtype=np.uint64)
        st = N.lib.hmk_clinkage_split_from_edges(ctx._h, edges.ctypes.data_as(C.POINTER(C.c_uint64)), edges.size, r0, r1, mcp, ncl, *ptr, None)
    return st, out


def test_host_only_context_answers_every_bad_argument(blosum62):
    rng = np.random.default_rng(6)
    peps = [rng.integers(0, 20, size=12).astype(np.uint8) for _ in range(6)]
    res, off = hammock_amd.pack_sequences(peps)
    ctx = host_ctx(blosum62, res, off)
    mc = [0, 0, 1, 1, 2, 2]
    bad = N.HMK_ERR_BAD_ARG
    none = np.zeros(0, dtype=np.uint64)
    for edges in (None, none):   # both entry points
        assert _raw(ctx, 4, 2, mc[:2], 1, edges=edges)[0] == bad                      # r0 > r1
        assert _raw(ctx, 0, 7, mc + [2], 3, edges=edges)[0] == bad                    # r1 > n
        assert _raw(ctx, 0, 6, [0, 0, 1, 1, 3, 3], 3, edges=edges)[0] == bad          # a slot at or above n_clusters
        assert _raw(ctx, 0, 6, [0, 0, 1, 1, 1, 1], 3, edges=edges)[0] == bad          # a slot without a member
        assert _raw(ctx, 0, 6, None, 3, edges=edges)[0] == bad                        # null member_cluster, non-empty range
        for name in ("split_cluster", "n_parts"):                                     # a null required output
            assert _raw(ctx, 0, 6, mc, 3, null=(name,), edges=edges)[0] == bad
            assert "null output" in N.lib.hmk_last_error(ctx._h).decode()
        assert _raw(ctx, 0, 6, mc, 3, null=("part_order",), edges=edges)[0] == bad    # part_order and part_start come together
        assert _raw(ctx, 0, 6, mc, 3, null=("part_start",), edges=edges)[0] == bad
    with pytest.raises(ValueError):
        ctx.clinkage_split(0, 6, [0, 0, 1, 1, 3, 3], 3, 3, 0, 20)
    # the scoring parameters (the device entry): the checks of hmk_cluster_linkage_shifted
    assert _raw(ctx, 0, 6, mc, 3, X=-1)[0] == bad
    assert _raw(ctx, 0, 6, mc, 3, X=12)[0] == N.HMK_ERR_SHIFT_TOO_BIG
    assert _raw(ctx, 0, 6, mc, 3, thr=30001)[0] == bad
    with pytest.raises(hammock_amd.DataException):
        ctx.clinkage_split(0, 6, mc, 3, 12, 0, 20)
    # an asymmetric matrix; scores beyond int16 at either end (they travel as int16)
    A = blosum62.copy()
    A[0, 1] += 1
    for edges in (None, none):
        actx = host_ctx(A, res, off)
        assert _raw(actx, 0, 6, mc, 3, edges=edges)[0] == bad and "symmetric" in N.lib.hmk_last_error(actx._h).decode()
    for penalty in (6000, -6000):   # (matrix entries are bounded at hmk_create: the shift penalty reaches the ends)
        assert _raw(ctx, 0, 6, mc, 3, p=penalty)[0] == bad and "int16" in N.lib.hmk_last_error(ctx._h).decode()
    # a valid call: no CPU fallback for the device entry, optional outputs or not, inner range or not; _from_edges runs
    assert _raw(ctx, 0, 6, mc, 3)[0] == N.HMK_ERR_DEVICE
    assert _raw(ctx, 0, 6, mc, 3, null=("part_id", "member_rank", "part_order", "part_start"))[0] == N.HMK_ERR_DEVICE
    with pytest.raises(hammock_amd.DeviceError):
        ctx.clinkage_split(0, 6, mc, 3, 3, 0, 20)
    with pytest.raises(hammock_amd.DeviceError):
        ctx.clinkage_split(2, 6, [0, 0, 1, 1], 2, 3, 0, 20)
    st, out = _raw(ctx, 0, 6, mc, 3, null=("part_id", "member_rank", "part_order", "part_start"), edges=hammock_amd.pack_edges([0], [1], [30]))
    assert st == 0 and out["split_cluster"].tolist() == [0, 0, 1, 2, 3, 4] and out["n_parts"].tolist() == [1, 2, 2]


def test_more_than_2_to_30_pairs_is_refused_before_any_scoring(blosum62):
    """a slot of 46,342 members holds 1,073,767,311 pairs, just over the cap; one member fewer and only the device is missing"""
    n = 46_342
    assert n * (n - 1) // 2 == 1_073_767_311 > 2 ** 30 >= (n - 1) * (n - 2) // 2
    res = np.random.default_rng(7).integers(0, 20, size=12 * n).astype(np.uint8)
    off = (12 * np.arange(n + 1)).astype(np.uint32)
    ctx = host_ctx(blosum62, res, off)
    mc = np.zeros(n, dtype=np.uint32)
    for edges in (None, np.zeros(0, dtype=np.uint64)):
        st, _ = _raw(ctx, 0, n, mc, 1, edges=edges)
        assert st == N.HMK_ERR_BAD_ARG
        msg = N.lib.hmk_last_error(ctx._h).decode()
        assert "1073767311" in msg and "fewer slots" in msg
    with pytest.raises(ValueError, match="fewer slots"):
        ctx.clinkage_split(0, n, mc, 1, 3, 0, 20)
    mc[-1] = 1   # 46,341 and 1: under the cap
    with pytest.raises(hammock_amd.DeviceError):
        ctx.clinkage_split(0, n, mc, 2, 3, 0, 20)


# ---- CPU: the thread count -------------------------------------------------------------------------------------------------

def test_result_does_not_depend_on_the_thread_count(coracle):
    """the slots run on min(8, usable CPUs) threads, and the usable CPUs are this process's affinity mask: one CPU is one thread"""
    allowed = os.sched_getaffinity(0)
    M, res, off, mc, ncl, X, p, thr, scored = sized_case(3)
    ctx = host_ctx(M, res, off)
    edges = inside_edges(scored, thr)
    Mc = _matrix("blosum75")
    cres, coff, cmc, cncl, bad = crash_case((1, 3))
    cctx = host_ctx(Mc, cres, coff)
    cedges = inside_edges(score_inside(coracle, Mc, cres, coff, cmc, 2, -2), 19)
    results = []
    try:
        for cpus in (allowed, {min(allowed)}):
            os.sched_setaffinity(0, cpus)
            results.append(ctx.clinkage_split_from_edges(edges, 0, mc.size, mc, ncl))
            with pytest.raises(hammock_amd.ReferenceWouldCrash) as info:
                cctx.clinkage_split_from_edges(cedges, 0, cmc.size, cmc, cncl)
            assert info.value.index == bad[0]
    finally:
        os.sched_setaffinity(0, allowed)
    same(results[0], family_expect(3, 0, 8))
    same(results[1], family_expect(3, 0, 8))


# ---- CPU: the mode's argument and file errors ------------------------------------------------------------------------------

def test_cli_split_argument_and_file_errors(tmp_path):
    r = cli("split", "-d", str(tmp_path / "a"))
    assert r.returncode == 2 and "-i or --input" in r.stderr
    assert not (tmp_path / "a").exists()
    good = tmp_path / "good.tsv"
    good.write_text("cluster_id\tsequence\tno_label\n1\tWVTAPRSLPVLP\t1\n1\tWVTAPRSLPVLA\t1\n")
    r = cli("split", "-i", str(good), "--devices", "0,1", "-d", str(tmp_path / "b"))
    assert r.returncode == 2 and "--devices" in r.stderr
    r = cli("split", "-i", str(good), "--java_hashset", "5", "-d", str(tmp_path / "b"))
    assert r.returncode == 2
    na = tmp_path / "na.tsv"
    na.write_text("cluster_id\tsequence\tno_label\n1\tWVTAPRSLPVLP\t1\nNA\tWVTAPRSLPVLA\t1\n")
    r = cli("split", "-i", str(na), "-d", str(tmp_path / "c"))
    assert r.returncode == 2 and "FileFormatException" in r.stderr
    short = tmp_path / "short.tsv"
    short.write_text("cluster_id\n1\n")
    r = cli("split", "-i", str(short), "-d", str(tmp_path / "d"))
    assert r.returncode == 2 and "FileFormatException" in r.stderr
    r = cli("split", "-i", str(good), "-d", str(tmp_path / "c"))   # the directory exists now
    assert r.returncode == 2 and "Output directory exists" in r.stderr
    r = cli("--help")
    assert "hammock-hip split -i" in r.stderr


# ---- GPU -------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("dthr", [0, 6])
@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_device_call_equals_from_edges_and_the_oracle(gpu, seed, dthr):
    """test 1: 24 slots of 1 ... 700 members (3,383 sequences, 748,228 pairs), flat and tiled slots in one call"""
    M, res, off, mc, ncl, X, p, thr, scored = sized_case(seed)
    thr += dthr
    want = family_expect(seed, dthr, 8)
    ctx = device_ctx(M, res, off)
    got = ctx.clinkage_split(0, mc.size, mc, ncl, X, p, thr)
    s = ctx.last_split_stats
    same(got, want)
    assert (s.pairs_scored, s.n_edges, s.n_multi, s.n_split) == numpy_stats(mc, ncl, scored, thr)
    assert s.n_result_clusters == int(want[1].sum()) and s.crash_slot == -1 and s.kernel_ms > 0 and s.chain_ms > 0
    assert got[0].dtype == np.uint32 and got[1].dtype == np.uint32 and got[2].dtype == np.int32
    same(ctx.clinkage_split_from_edges(inside_edges(scored, thr), 0, mc.size, mc, ncl), got, "from edges ")


@pytest.mark.gpu
def test_threshold_edge(gpu):
    """test 2: a pair scoring exactly the threshold is an edge; one threshold higher it is not, and its slot splits"""
    M, res, off, mc, ncl, X, p, thr, scored = sized_case(2)
    _, _, slot, sc = scored
    ctx = device_ctx(M, res, off)
    for c in (int(np.flatnonzero(np.bincount(mc) == 700)[0]), int(np.flatnonzero(np.bincount(mc) == 65)[0])):   # a tiled slot, a flat one
        lowest = int(sc[slot == c].min())
        at = ctx.clinkage_split(0, mc.size, mc, ncl, X, p, lowest)
        assert at[1][c] == 1
        same(at, oracle_split(M, res, off, mc, ncl, X, p, lowest))
        above = ctx.clinkage_split(0, mc.size, mc, ncl, X, p, lowest + 1)
        assert above[1][c] > 1
        same(above, oracle_split(M, res, off, mc, ncl, X, p, lowest + 1))
        assert ctx.last_split_stats.n_edges == int((sc >= lowest + 1).sum())


@pytest.mark.gpu
def test_state_between_calls(gpu):
    """test 3: one context; an inner range, permuted slot numbers, another threshold and back, a repeat, other calls in between,
    the optional outputs null"""
    M, res, off, mc, ncl, X, p, thr, scored = sized_case(2)
    nm = mc.size
    ctx = device_ctx(M, res, off)
    first = ctx.clinkage_split(0, nm, mc, ncl, X, p, thr)
    same(first, family_expect(2, 0, 8))
    # an inner range: the slots that have members there, renumbered
    r0, r1 = 150, 1550
    ids, sub = np.unique(mc[r0:r1], return_inverse=True)
    sub = sub.astype(np.uint32)
    same(ctx.clinkage_split(r0, r1, sub, ids.size, X, p, thr), oracle_split(M, res, off, sub, ids.size, X, p, thr, r0=r0), "inner ")
    # permuted slot numbers
    perm = np.random.default_rng(90_200).permutation(ncl)
    moved_mc = perm[mc].astype(np.uint32)
    moved = ctx.clinkage_split(0, nm, moved_mc, ncl, X, p, thr)
    same(moved, oracle_split(M, res, off, moved_mc, ncl, X, p, thr), "moved ")
    assert np.array_equal(moved[1][perm], first[1]) and np.array_equal(moved[2], first[2]) and np.array_equal(moved[3], first[3])
    # another threshold, other calls, and back
    same(ctx.clinkage_split(0, nm, mc, ncl, X, p, thr + 6), family_expect(2, 6, 8), "raised ")
    ctx.cluster_linkage_shifted(0, nm, mc, ncl, X, p, thr)
    ctx.neighbors_shifted(X, p, thr + 10)
    again = ctx.clinkage_split(0, nm, mc, ncl, X, p, thr)
    same(again, first, "again ")
    same(ctx.clinkage_split(0, nm, mc, ncl, X, p, thr), first, "repeat ")
    # the optional outputs null
    st, out = _raw(ctx, 0, nm, mc, ncl, X, p, thr, null=("part_id", "member_rank", "part_order", "part_start"))
    assert st == 0 and np.array_equal(out["split_cluster"], first[0]) and np.array_equal(out["n_parts"], first[1])
    st, out = _raw(ctx, 0, nm, mc, ncl, X, p, thr, null=("member_rank",))
    assert st == 0 and np.array_equal(out["part_id"], first[2])
    assert np.array_equal(out["part_start"], np.concatenate([[0], np.cumsum(np.bincount(mc, minlength=ncl))]))


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2])
def test_closure(gpu, seed):
    """test 4: the new clustering passes the check, and no two parts of one source slot are feasible for each other"""
    M, res, off, mc, ncl, X, p, thr, _ = sized_case(seed)
    ctx = device_ctx(M, res, off)
    split = ctx.clinkage_split(0, mc.size, mc, ncl, X, p, thr)[0]
    parts = int(ctx.last_split_stats.n_result_clusters)
    assert parts > ncl
    ctx.cluster_linkage_shifted(0, mc.size, split, parts, X, p, thr)
    assert ctx.last_linkage_stats.n_violating == 0
    source = np.zeros(parts, dtype=np.int64)
    source[split] = mc
    x, m, _ = hammock_amd.edge_fields(ctx.cluster_pairs_shifted(0, mc.size, split, parts, X, p, thr))
    assert not (source[x] == source[m]).any()


def _musi():
    with open(os.path.join(GOLDEN, "musi.fa")) as fh:
        return [line.strip() for line in fh if line.strip() and not line.startswith(">")]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["greedy", "clinkage"])
def test_clusters_of_the_clustering_calls_come_back_whole(gpu, name):
    """test 5: what hmk_greedy_cluster and hmk_clinkage_cluster return is not split at their own parameters; at threshold + 4 the
    split equals the oracle's"""
    M = _matrix("blosum62")
    seqs = list(dict.fromkeys(_musi()))
    count = len(seqs) if name == "greedy" else 1000
    res, off = hammock_amd.pack_sequences(seqs[:count])
    ctx = device_ctx(M, res, off)
    cid = ctx.greedy_cluster(3, 0, 20, 2 ** 31 - 1)[0] if name == "greedy" else ctx.clinkage_cluster(3, 0, 20)[0]
    _, mc = np.unique(cid, return_inverse=True)
    mc = mc.astype(np.uint32)
    ncl = int(mc.max()) + 1
    got = ctx.clinkage_split(0, count, mc, ncl, 3, 0, 20)
    s = ctx.last_split_stats
    assert s.n_split == 0 and s.n_result_clusters == ncl and s.n_multi > 20 and s.n_edges == s.pairs_scored
    assert np.array_equal(got[0], mc) and (got[1] == 1).all()
    raised = ctx.clinkage_split(0, count, mc, ncl, 3, 0, 24)
    assert ctx.last_split_stats.n_split > 0
    same(raised, oracle_split(M, res, off, mc, ncl, 3, 0, 24))


@pytest.mark.gpu
def test_singletons_an_empty_range_and_one_slot_of_two(gpu):
    """test 6"""
    M, res, off, mc, ncl, X, p, thr, _ = sized_case(2)
    ctx = device_ctx(M, res, off)
    got = ctx.clinkage_split(10, 60, np.arange(50), 50, X, p, thr)
    assert np.array_equal(got[0], np.arange(50)) and (got[1] == 1).all() and (got[2] == 1).all() and (got[3] == 0).all()
    s = ctx.last_split_stats
    assert (s.pairs_scored, s.n_edges, s.n_multi, s.n_split, s.n_result_clusters, s.kernel_ms) == (0, 0, 0, 0, 50, 0.0)
    got = ctx.clinkage_split(7, 7, [], 0, X, p, thr)
    assert all(len(g) == 0 for g in got) and ctx.last_split_stats.n_result_clusters == 0
    for r0 in (0, 500):
        two = np.zeros(2, dtype=np.uint32)
        for t in (-100, 100):   # together, apart
            same(ctx.clinkage_split(r0, r0 + 2, two, 1, X, p, t), oracle_split(M, res, off, two, 1, X, p, t, r0=r0))
        assert ctx.last_split_stats.pairs_scored == 1 and ctx.last_split_stats.n_split == 1


def _java_round(v):
    import math
    return int(math.floor(v + 0.5))


def _grouped(path):
    """cluster id -> its sequences in the file's line order"""
    out = {}
    for c, s, _ in read_cluster_file(path):
        out.setdefault(c, []).append(s)
    return out


@pytest.mark.gpu
def test_cli_split_on_greedy_clusters(gpu, tmp_path):
    """test 7: `split` on greedy's stage-1 file of MUSI at a raised threshold writes what the oracle says; at the original parameters
    the clusters come back as they were read; `check` on the output finds nothing"""
    r = cli("greedy", "-i", os.path.join(GOLDEN, "musi.fa"), "-d", str(tmp_path / "g"), timeout=600)
    assert r.returncode == 0, r.stderr
    cfile = tmp_path / "g" / "initial_clusters_sequences.tsv"
    M = _matrix("blosum62")
    loaded = read_cluster_file(cfile)
    ids = list(dict.fromkeys(c for c, _, _ in loaded))
    slot = {c: k for k, c in enumerate(ids)}
    order = sorted(range(len(loaded)), key=lambda k: slot[loaded[k][0]])   # the loader groups the lines by cluster (stable)
    mc = np.array([slot[loaded[k][0]] for k in order], dtype=np.uint32)
    seqs = [loaded[k][1] for k in order]
    sizes = np.array([loaded[k][2] for k in order], dtype=np.int32)
    lens = [len(s) for s in seqs]
    X = min(_java_round(sum(lens) / len(lens) / 4), min(lens) - 1)
    thr = _java_round(sum(lens) / len(lens) * 1.7)
    res, off = hammock_amd.pack_sequences(seqs)
    raised = thr + 4
    split, n_parts, part_id, rank, part_order = oracle_split(M, res, off, mc, len(ids), X, 0, raised, sizes=sizes)
    assert (n_parts > 1).sum() >= 5
    next_id = max(ids)
    lines, members = ["source_cluster_id\tcluster_id\tunique_size\tsize\tparts"], {}
    for k, c in enumerate(ids):
        m = np.flatnonzero(mc == k)
        if n_parts[k] == 1:
            lines.append(f"{c}\t{c}\t{m.size}\t{sizes[m].sum()}\t1")
            members[c] = [seqs[i] for i in m]
            continue
        for pid in part_order[k]:
            next_id += 1
            mine = m[part_id[m] == pid]
            mine = mine[np.argsort(rank[mine])]
            lines.append(f"{c}\t{next_id}\t{mine.size}\t{sizes[mine].sum()}\t{n_parts[k]}")
            members[next_id] = [seqs[i] for i in mine]
    out = tmp_path / "s"
    r = cli("split", "-i", str(cfile), "-d", str(out), "-x", str(X), "-g", str(raised), timeout=600)
    assert r.returncode == 0, r.stderr
    assert (out / "split_clusters.tsv").read_text() == "\n".join(lines) + "\n"
    written = _grouped(out / "initial_clusters_sequences.tsv")
    assert {c: sorted(v) for c, v in written.items()} == {c: sorted(v) for c, v in members.items()}
    log = (out / "run.log").read_text()
    assert f"Clusters split: {(n_parts > 1).sum()}" in log and f"Resulting clusers: {n_parts.sum()}" in log and "pairs scored: " in log
    # the output passes the check at the same parameters
    r = cli("check", "-i", str(out / "initial_clusters_sequences.tsv"), "-d", str(tmp_path / "c"), "-x", str(X), "-g", str(raised), timeout=600)
    assert r.returncode == 0, r.stderr
    assert f"\t0 of {n_parts.sum()} clusters hold a pair below the threshold {raised};" in (tmp_path / "c" / "run.log").read_text().splitlines()[-1]
    # the original parameters (the defaults): the clusters and their member order are the input's
    same_out = tmp_path / "o"
    r = cli("split", "-i", str(cfile), "-d", str(same_out), timeout=600)
    assert r.returncode == 0, r.stderr
    assert "Max shift not set. Setting automatically to: " + str(X) in r.stderr
    assert "Split threshold not set. Setting automatically to: " + str(thr) in r.stderr
    assert "Clusters split: 0" in (same_out / "run.log").read_text()
    assert _grouped(same_out / "initial_clusters_sequences.tsv") == _grouped(cfile)
