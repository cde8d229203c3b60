"""Order stability: the greedy clustering under many orders of the set from one scoring pass -- hmk_greedy_orders (k_orders.hip),
hmk_greedy_orders_from_edges and `hammock-hip orders`.

The expected answer is never the code under test: per order the C oracle's greedy_cluster on the PERMUTED input, mapped back to
uploaded indices; the supports, partner counts and pair counts by numpy over the oracle's ids; the consensus by scipy's connected
components over those supports, and at n_valid also as the meet of the valid partitions.  One identity is asserted everywhere:
pairs_together[k] = the sum of C(members, 2) over order k's clusters.  Expectations are computed once per (input, orders) and shared.
CPU part (host-only context): the symbols and structure sizes, every refusal, _from_edges against the oracle, ignored / shuffled /
either-orientation edges, the mode's argument errors.
GPU part: the device call against the oracle and against _from_edges on the pass's own edges at the smallest shapes where the
kernels can still go wrong; capacities; grid caps; state between calls; the permuted sizes do not leak; [0, 0]; the mode's files.
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, random_peptides
from test_assign import gpu   # noqa: F401  (the fixture that skips where no HIP device is visible)
from test_continue import cli, read_cluster_file
from test_sweep import inp as sweep_inp, matrix

import hammock_amd
from hammock_amd import _native as N
from oracle import c_oracle

SHARED = ("phase1_stop_index", "phase1_clusters", "phase1_orphans", "n_result_clusters", "n_multi")   # hmk_greedy_stats' fields in an order
GRID_LINE = re.compile(r"^\[hmk grid\] (\S+) (\d+) -> (\d+)$", re.M)
CRASH = N.HMK_ERR_REFERENCE_WOULD_CRASH
P_U32, P_I32, P_U64 = C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_uint64)


# ---- inputs ----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def inp(name):
    """-> dict: M, res, off, sizes, X, p, thr, maxc, n"""
    if name in ("random400", "keyed", "sizes300", "crash", "ends", "synth12", "musi"):
        d = dict(sweep_inp(name))
        if name == "crash":   # (at this threshold some orders make the reference throw and some do not: asserted where it is used)
            d["thr"] = 10
        return d
    M, sizes = matrix(), None
    rng = np.random.default_rng(7)
    if name == "n1":
        peps, (X, p, thr, maxc) = random_peptides(rng, 1, 8, 10), (2, 0, 10, 1)
    elif name == "n2":
        peps, (X, p, thr, maxc) = random_peptides(rng, 2, 8, 10), (2, 0, -50, 2)
    elif name == "n65":
        peps, (X, p, thr, maxc) = random_peptides(rng, 65, 7, 12, alphabet=4), (2, -1, 12, 6)
    elif name == "noedge":   # no pair reaches the threshold: the first sequence of any order has no neighbour, the reference throws
        peps, (X, p, thr, maxc) = random_peptides(rng, 30, 8, 10), (2, 0, 200, 5)
    elif name in ("n40", "n40_one_cluster", "n40_no_limit"):
        peps, (X, p, thr) = random_peptides(np.random.default_rng(11), 40, 7, 12, alphabet=4), (2, -1, 12)
        maxc = {"n40": 5, "n40_one_cluster": 1, "n40_no_limit": 40}[name]
    elif name == "one_length":   # one length: one tile of the pass, so one segment of the edge buffer holds every edge
        peps, (X, p, thr, maxc) = random_peptides(rng, 14, 9, 9, alphabet=4), (2, -1, 9, 3)
    elif name == "negative":   # a tiny dense set, scores -16 .. 12, every threshold below 0
        peps, (X, p, thr, maxc) = random_peptides(rng, 24, 7, 9), (2, -2, -5, 6)
    else:
        raise KeyError(name)
    res, off = hammock_amd.pack_sequences(peps)
    for a in (res, off):
        a.setflags(write=False)
    return dict(M=M, res=res, off=off, sizes=sizes, X=X, p=p, thr=thr, maxc=maxc, n=len(off) - 1)


@functools.lru_cache(maxsize=None)
def make_orders(n, kind, k=0, seed=0):
    """-> uint32 (n_orders, n): 'id'; 'rev' (identity + reversed); 'random' (identity + k - 1 random); 'twice' (one random order twice)"""
    rng = np.random.default_rng(1000 + seed)
    ident = np.arange(n, dtype=np.uint32)
    if kind == "id":
        rows = [ident]
    elif kind == "rev":
        rows = [ident, ident[::-1]]
    elif kind == "random":
        rows = [ident] + [rng.permutation(n) for _ in range(k - 1)]
    elif kind == "twice":
        perm = rng.permutation(n)
        rows = [perm, perm]
    else:
        raise KeyError(kind)
    out = np.ascontiguousarray(np.stack(rows).astype(np.uint32))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle_rows(name, okey, unit_sizes=False):
    """-> per order (status, cluster_id, result_order, member_rank, stats) of the C oracle's greedy_cluster on the permuted input, the
    three rows mapped back to uploaded indices (clusters named by their seed's uploaded index)"""
    d = inp(name)
    n = d["n"]
    out = []
    for o in make_orders(n, *okey):
        res, off = hammock_amd.pack_sequences([d["res"][d["off"][i]:d["off"][i + 1]] for i in o])
        sizes = None if d["sizes"] is None or unit_sizes else np.ascontiguousarray(d["sizes"][o])
        st, cid, order, stats = c_oracle.greedy_cluster(d["M"], res, off, sizes, 0, d["X"], d["p"], d["thr"], d["maxc"], 1)
        assert st in (0, c_oracle.HMO_ERR_REFERENCE_WOULD_CRASH)
        if st:
            out.append((st, None, None, None, stats))
            continue
        ids, rank = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
        ids[o] = o[cid]
        rank[o] = stats.member_rank
        out.append((0, ids, o[order].astype(np.int32), rank, stats))
    return out


def pairs_of(ids):
    """the unordered pairs inside one cluster of a partition given as labels -> sorted keys i * n + j, i < j"""
    n = ids.size
    by = np.argsort(ids, kind="stable")
    cut = np.flatnonzero(np.diff(ids[by])) + 1
    keys = []
    for grp in np.split(by, cut):
        if grp.size > 1:
            a, b = np.triu_indices(grp.size, 1)
            keys.append(grp[a].astype(np.int64) * n + grp[b])   # (stable argsort: grp ascending, so i < j)
    return np.sort(np.concatenate(keys)) if keys else np.zeros(0, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def expected(name, okey, min_support=0):
    """everything the call returns, from the oracle's rows by numpy and scipy"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    n = inp(name)["n"]
    rows = oracle_rows(name, okey)
    valid = [k for k, r in enumerate(rows) if r[0] == 0]
    nv = len(valid)
    per = {k: pairs_of(rows[k][1]) for k in valid}
    for k in valid:   # the identity: pairs together = the sum of C(members, 2)
        size = np.bincount(rows[k][1], minlength=n).astype(np.int64)
        assert per[k].size == int((size * (size - 1) // 2).sum())
    keys, support = np.unique(np.concatenate([per[k] for k in valid]), return_counts=True) if nv else (np.zeros(0, np.int64), np.zeros(0, np.int64))
    x, m = keys // n, keys % n
    E = dict(rows=rows, valid=valid, n_valid=nv, keys=keys, support=support,
             together={k: per[k].size for k in valid},
             with_first={k: np.intersect1d(per[k], per[valid[0]], assume_unique=True).size for k in valid},
             ever=np.bincount(np.concatenate([x, m]), minlength=n).astype(np.uint32),
             always=np.bincount(np.concatenate([x[support == nv], m[support == nv]]), minlength=n).astype(np.uint32),
             pairs_always=int((support == nv).sum()) if nv else 0)
    level = min_support if min_support else nv
    keep = support >= level if nv else np.zeros(0, dtype=bool)
    g = coo_matrix((np.ones(int(keep.sum())), (x[keep], m[keep])), shape=(n, n))
    ncomp, lab = connected_components(g, directed=False)
    smallest = np.full(ncomp, n, dtype=np.int64)
    np.minimum.at(smallest, lab, np.arange(n))
    E["consensus"] = smallest[lab].astype(np.uint32)
    if nv and level == nv:   # the meet of the valid partitions
        _, meet = np.unique(np.stack([rows[k][1] for k in valid], axis=1), axis=0, return_inverse=True)
        meet = np.asarray(meet).reshape(-1)
        first = np.full(meet.max() + 1, n, dtype=np.int64)
        np.minimum.at(first, meet, np.arange(n))
        assert np.array_equal(E["consensus"], first[meet])
    size = np.bincount(E["consensus"], minlength=n)
    E["consensus_counts"] = (int((size > 0).sum()), int((size == 1).sum()), int(size.max()))
    return E


def oracle_edges(name, thr=None):
    d = inp(name)
    n = d["n"]
    st, sc = c_oracle.score_block(d["M"], d["res"], d["off"], np.arange(n), np.arange(n), 0, d["X"], d["p"])   # [seq1][seq2]
    assert st == 0
    x, m = np.triu_indices(n, 1)
    s = sc.T[x, m]
    keep = s >= (d["thr"] if thr is None else thr)
    return hammock_amd.pack_edges(x[keep], m[keep], s[keep])


def make_ctx(name, device=-1):
    d = inp(name)
    ctx = hammock_amd.Context(d["M"], device=device)
    ctx.set_sequences(residues=d["res"], offsets=d["off"], sizes=d["sizes"])
    return ctx


def same_as_expected(r, E, what=""):
    """r: an OrdersResult with every output; E: expected()"""
    n = r.consensus.size
    assert r.per_order.size == len(E["rows"]) == r.cluster_id.shape[0]
    for k, (st, ids, order, rank, ostats) in enumerate(E["rows"]):
        po, w = r.per_order[k], f"{what}order {k} "
        if st:
            assert (po["status"], po["crash_case"], po["crash_index"]) == (CRASH, ostats.crash_case, ostats.crash_index), w
            assert (r.cluster_id[k] == -1).all() and (r.result_order[k] == -1).all() and (r.member_rank[k] == -1).all(), w
            assert (po["pairs_together"], po["pairs_with_first"]) == (0, 0), w
            continue
        assert (po["status"], po["crash_case"]) == (0, 0), w
        assert np.array_equal(r.cluster_id[k], ids), w + "cluster_id"
        nr = po["n_result_clusters"]
        assert np.array_equal(r.result_order[k, :nr], order) and (r.result_order[k, nr:] == -1).all(), w + "result_order"
        assert np.array_equal(r.member_rank[k], rank), w + "member_rank"
        assert [int(po[f]) for f in SHARED] == [getattr(ostats, f) for f in SHARED], w
        size = np.bincount(ids, minlength=n).astype(np.int64)
        assert (po["n_singletons"], po["largest"]) == ((size == 1).sum(), size.max()), w
        assert po["pairs_together"] == E["together"][k] == (size * (size - 1) // 2).sum(), w + "pairs_together"
        assert po["pairs_with_first"] == E["with_first"][k], w + "pairs_with_first"
    s = r.stats
    assert (s.n_orders, s.n_valid) == (len(E["rows"]), E["n_valid"]), what
    assert (s.pairs_ever, s.pairs_always) == (E["keys"].size, E["pairs_always"]), what
    assert np.array_equal(r.partners_ever, E["ever"]) and np.array_equal(r.partners_always, E["always"]), what + "partners"
    assert np.array_equal(r.consensus, E["consensus"]), what + "consensus"
    assert (s.n_consensus, s.n_consensus_singletons, s.consensus_largest) == E["consensus_counts"], what
    if r.support_edges is not None:
        x, m, sup = hammock_amd.edge_fields(r.support_edges)
        assert (x < m).all() and r.support_edges.size == E["keys"].size
        by = np.argsort(x.astype(np.int64) * n + m)
        assert np.array_equal(x[by].astype(np.int64) * n + m[by], E["keys"]) and np.array_equal(sup[by], E["support"]), what + "support edges"


def same_results(a, b, what=""):
    """two OrdersResults of the same call: everything but the times and pairs_scored"""
    for f in a.per_order.dtype.names:
        assert f == "tail_ms" or np.array_equal(a.per_order[f], b.per_order[f]), what + f
    for f in ("cluster_id", "result_order", "member_rank", "partners_always", "partners_ever", "consensus"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), what + f
    assert np.array_equal(np.sort(a.support_edges), np.sort(b.support_edges)), what + "support edges"
    for f, _ in N.GreedyOrdersStats._fields_:
        assert f.endswith("_ms") or f == "pairs_scored" or getattr(a.stats, f) == getattr(b.stats, f), what + f


def raw(ctx, fn, head, orders, n_orders=None, min_support=0, outputs=True, stats=True, support=False, capacity=0):
    """the C call with NULL where an output is not wanted -> status"""
    n = max(ctx.n, 1)
    k = orders.shape[0] if n_orders is None and orders is not None else n_orders
    rows = [np.full((max(k, 1), n), -7, dtype=np.int32) for _ in range(3)]
    po = np.zeros(max(k, 1), dtype=hammock_amd.api.GREEDY_ORDER_DTYPE)
    u = [np.zeros(n, dtype=np.uint32) for _ in range(3)]
    sup = np.zeros(max(capacity, 1), dtype=np.uint64)
    need = C.c_uint64(0)
    S = N.GreedyOrdersStats()
    return fn(ctx._h, *head, orders.ctypes.data_as(P_U32) if orders is not None else None, k, min_support,
              *[a.ctypes.data_as(P_I32) if outputs else None for a in rows],
              po.ctypes.data_as(C.POINTER(N.GreedyOrder)) if outputs else None,
              *[a.ctypes.data_as(P_U32) if outputs else None for a in u],
              sup.ctypes.data_as(P_U64) if support else None, capacity, C.byref(need), C.byref(S) if stats else None)


# ---- CPU: the symbols ------------------------------------------------------------------------------------------------------

def test_symbols_are_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "hammock_hip.h")) as fh:
        header = fh.read()
    for name in ("hmk_greedy_orders", "hmk_greedy_orders_from_edges"):
        assert re.search(r"\bint " + name + r"\(", header)
        assert name in N.SYMBOLS and hasattr(N.lib, name)
    assert "} hmk_greedy_order;" in header and "} hmk_greedy_orders_stats;" in header
    assert re.search(r"#define HMK_ABI_VERSION 4\b", header) and N.lib.hmk_abi_version() == 4
    assert C.sizeof(N.GreedyOrder) == 64 == hammock_amd.api.GREEDY_ORDER_DTYPE.itemsize and C.sizeof(N.GreedyOrdersStats) == 80
    for (name, ctype), (dname, (dtype, offset)) in zip(N.GreedyOrder._fields_, hammock_amd.api.GREEDY_ORDER_DTYPE.fields.items()):
        assert name == dname and getattr(N.GreedyOrder, name).offset == offset and C.sizeof(ctype) == dtype.itemsize


# ---- CPU: _from_edges against the oracle -------------------------------------------------------------------------------------

CPU_CASES = [("musi", ("random", 5, 0)), ("random400", ("random", 10, 0)), ("sizes300", ("random", 6, 0)), ("crash", ("random", 10, 0)),
             ("n40", ("random", 9, 0)), ("noedge", ("random", 3, 0)), ("n1", ("id",)), ("negative", ("random", 5, 0))]


@pytest.mark.parametrize("name,okey", CPU_CASES)
def test_from_edges_equals_the_oracle(name, okey):
    d = inp(name)
    if name == "musi":   # the reversed order beside the random ones, as in the issue's table
        okey = ("rev",)
    E = expected(name, okey)
    orders = make_orders(d["n"], *okey)
    if name == "crash":
        assert 0 < E["n_valid"] < orders.shape[0]
    if name in ("noedge", "n1"):
        assert E["n_valid"] == 0
    if name == "random400":   # the issue's table: 285 to 482 pairs per order, none in every order, 3,148 in at least one
        assert E["n_valid"] == 10 and min(E["together"].values()) > 100 and E["pairs_always"] < E["keys"].size
    ctx = make_ctx(name)
    r = ctx.greedy_orders_from_edges(oracle_edges(name), d["thr"], d["maxc"], orders)
    same_as_expected(r, E)
    s = r.stats
    assert (s.n_edges, s.pairs_scored, s.kernel_ms, s.relabel_ms, s.support_ms) == (oracle_edges(name).size, 0, 0.0, 0.0, 0.0)
    assert ctx.last_orders_needed == E["keys"].size


def test_the_size_tie_break_decides_in_some_order():
    """the property of the weighted input, from the oracle alone: at least one order's clustering differs from the same order's with
    every size 1 -- so a tail that read the sizes in upload order, or none, cannot pass"""
    okey = ("random", 6, 0)
    with_sizes, unit = oracle_rows("sizes300", okey), oracle_rows("sizes300", okey, True)
    assert any(a[0] == 0 and b[0] == 0 and not np.array_equal(a[1], b[1]) for a, b in zip(with_sizes, unit))


@pytest.mark.parametrize("min_support", [1, 4, 9])
def test_from_edges_consensus_at_every_support_level(min_support):
    d = inp("n40")
    okey = ("random", 9, 0)
    E = expected("n40", okey, min_support)
    assert len({expected("n40", okey, s)["consensus_counts"] for s in (1, 4, 9)}) == 3   # the levels differ on this input
    r = make_ctx("n40").greedy_orders_from_edges(oracle_edges("n40"), d["thr"], d["maxc"], make_orders(d["n"], *okey), min_support=min_support)
    same_as_expected(r, E)
    if min_support == 9:
        same_results(r, make_ctx("n40").greedy_orders_from_edges(oracle_edges("n40"), d["thr"], d["maxc"], make_orders(d["n"], *okey)))


def test_edges_below_are_ignored_and_order_and_orientation_do_not_matter():
    d = inp("random400")
    okey = ("random", 4, 0)
    orders = make_orders(d["n"], *okey)
    ctx = make_ctx("random400")
    first = ctx.greedy_orders_from_edges(oracle_edges("random400"), d["thr"], d["maxc"], orders)
    low = oracle_edges("random400", 8)
    assert low.size > oracle_edges("random400").size + 1000
    x, m, sc = hammock_amd.edge_fields(low)
    rng = np.random.default_rng(3)
    flip = rng.random(low.size) < 0.5
    other = hammock_amd.pack_edges(np.where(flip, m, x), np.where(flip, x, m), sc)[rng.permutation(low.size)]
    again = ctx.greedy_orders_from_edges(other, d["thr"], d["maxc"], orders)
    same_results(first, again)
    same_as_expected(again, expected("random400", okey))


# ---- CPU: the argument checks ------------------------------------------------------------------------------------------------

def test_bad_arguments_are_refused_before_the_device_is_looked_at():
    d = inp("n40")
    n = d["n"]
    edges = oracle_edges("n40")
    ctx = make_ctx("n40")
    orders = make_orders(n, "random", 3, 0)
    heads = [(N.lib.hmk_greedy_orders, (d["X"], d["p"], d["thr"], d["maxc"])),
             (N.lib.hmk_greedy_orders_from_edges, (edges.ctypes.data_as(P_U64), edges.size, d["thr"], d["maxc"]))]
    BAD = N.HMK_ERR_BAD_ARG
    for fn, head in heads:   # the same checks in both, on a host-only context
        assert raw(ctx, fn, head, orders, n_orders=0) == BAD
        assert raw(ctx, fn, head, np.tile(orders[:1], (257, 1)), n_orders=257) == BAD
        assert raw(ctx, fn, head, None, n_orders=3) == BAD
        assert raw(ctx, fn, head, orders, stats=False) == BAD
        assert raw(ctx, fn, head, orders, min_support=4) == BAD
        assert raw(ctx, fn, head, orders, support=False, capacity=5) == BAD
        assert raw(ctx, fn, head, orders, outputs=False) == BAD
        for bad_value in (orders[1, 0], n, 2 ** 32 - 1):   # a repeated index, one past the end, far outside
            bad = orders.copy()
            bad[1, 7] = bad_value
            assert raw(ctx, fn, head, bad) == BAD and "order 1 is not a permutation" in N.lib.hmk_last_error(ctx._h).decode()
        assert fn(None, *head, orders.ctypes.data_as(P_U32), 3, 0, *[None] * 8, 0, None, None) == BAD
    fn, head = heads[1]
    assert raw(ctx, fn, head, orders) == 0 and raw(ctx, fn, head, orders, min_support=3) == 0
    assert raw(ctx, fn, head, orders, outputs=False, support=True, capacity=4096) == 0   # one output is enough
    assert raw(ctx, fn, head, np.tile(orders[:1], (256, 1))) == 0                       # 256 orders are allowed
    assert raw(ctx, fn, (None, 5, d["thr"], d["maxc"]), orders) == BAD                  # a null edge list
    for x, m in ((3, n), (n, 3), (2 ** 24 - 1, 0), (5, 5)):   # an index >= n either side, a self pair, whatever its score
        for score in (25, 3):
            bad = edges.copy()
            bad[10] = hammock_amd.pack_edges(np.array([x]), np.array([m]), np.array([score]))[0]
            with pytest.raises(ValueError, match="outside"):
                ctx.greedy_orders_from_edges(bad, d["thr"], d["maxc"], orders)
    with pytest.raises(ValueError, match="min_support"):
        ctx.greedy_orders_from_edges(edges, d["thr"], d["maxc"], orders, min_support=4)
    with pytest.raises(ValueError, match="orders must be"):
        ctx.greedy_orders_from_edges(edges, d["thr"], d["maxc"], orders[:, :-1])
    same_as_expected(ctx.greedy_orders_from_edges(edges, d["thr"], d["maxc"], orders), expected("n40", ("random", 3, 0)), "after the refusals ")


def test_an_asymmetric_matrix_is_refused():
    d = sweep_inp("asym")
    ctx = hammock_amd.Context(d["M"], device=-1)
    ctx.set_sequences(residues=d["res"], offsets=d["off"])
    orders = make_orders(d["n"], "rev")
    for call in (lambda: ctx.greedy_orders(d["X"], d["p"], d["thr"], d["maxc"], orders),
                 lambda: ctx.greedy_orders_from_edges(np.zeros(0, dtype=np.uint64), d["thr"], d["maxc"], orders)):
        with pytest.raises(ValueError, match="symmetric"):
            call()


def test_support_capacity_on_the_host_form():
    d = inp("n40")
    okey = ("random", 9, 0)
    E = expected("n40", okey)
    need = E["keys"].size
    assert need > 2
    ctx = make_ctx("n40")
    args = (oracle_edges("n40"), d["thr"], d["maxc"], make_orders(d["n"], *okey))
    for cap in (0, need - 1):
        with pytest.raises(BufferError, match=str(need)):
            ctx.greedy_orders_from_edges(*args, support_capacity=cap)
        assert ctx.last_orders_needed == need
    same_as_expected(ctx.greedy_orders_from_edges(*args, support_capacity=need), E)
    r = ctx.greedy_orders_from_edges(*args, support=False)
    assert r.support_edges is None and ctx.last_orders_needed == need
    same_as_expected(r, E)


def test_the_device_form_needs_a_device_and_an_empty_set_is_ok():
    d = inp("n40")
    ctx = make_ctx("n40")
    with pytest.raises(hammock_amd.DeviceError):
        ctx.greedy_orders(d["X"], d["p"], d["thr"], d["maxc"], make_orders(d["n"], "rev"))
    empty = hammock_amd.Context(matrix(), device=-1)
    for r in (empty.greedy_orders_from_edges(np.zeros(0, dtype=np.uint64), 20, 10, np.zeros((3, 0), dtype=np.uint32)),
              empty.greedy_orders(3, 0, 20, 10, np.zeros((3, 0), dtype=np.uint32))):
        assert r.cluster_id.shape == (3, 0) and r.consensus.size == 0 and r.support_edges.size == 0
        assert not any(r.per_order[f].any() for f in r.per_order.dtype.names)
        assert (r.stats.n_orders, r.stats.n_valid, r.stats.pairs_ever, r.stats.n_consensus) == (3, 3, 0, 0)


def test_cli_orders_argument_and_file_errors(tmp_path):
    fa = os.path.join(GOLDEN, "musi.fa")
    r = cli("orders", "-d", str(tmp_path / "a"))
    assert r.returncode == 2 and "-i or --input" in r.stderr
    r = cli("orders", "-i", fa, "--devices", "0,1", "-d", str(tmp_path / "a"))
    assert r.returncode == 2 and "--devices" in r.stderr
    for value in ("-1", "256"):
        r = cli("orders", "-i", fa, "--random_orders", value, "-d", str(tmp_path / "a"))
        assert r.returncode == 2 and "--random_orders may be 0 to 255" in r.stderr
    r = cli("orders", "-i", fa, "--random_orders", "4", "--min_support", "6", "-d", str(tmp_path / "a"))
    assert r.returncode == 2 and "--min_support" in r.stderr and "orders, 5" in r.stderr
    assert not (tmp_path / "a").exists()
    r = cli("orders", "-i", fa, "-f", "nothing", "-d", str(tmp_path / "b"))
    assert r.returncode == 2 and "-f" in r.stderr
    r = cli("orders", "-i", fa, "-d", str(tmp_path / "b"))   # the directory exists now
    assert r.returncode == 2 and "Output directory exists" in r.stderr
    r = cli("orders", "-i", str(tmp_path / "missing.fa"), "-d", str(tmp_path / "c"))
    assert r.returncode != 0
    r = cli("orders", "-i", fa, "-l", "no_such_label", "-d", str(tmp_path / "e"))
    assert r.returncode == 3 and "No sequences" in r.stderr
    usage = cli("--help").stderr
    assert "hammock-hip orders -i" in usage and "--random_orders <int>" in usage and "--min_support <int>" in usage and "--pairs\n" in usage


# ---- GPU: the device call ----------------------------------------------------------------------------------------------------

def device_call(name, okey, min_support=0, ctx=None, **kw):
    d = inp(name)
    ctx = ctx or make_ctx(name, 0)
    return ctx, ctx.greedy_orders(d["X"], d["p"], d["thr"], d["maxc"], make_orders(d["n"], *okey), min_support=min_support, **kw)


def against_both(name, okey, min_support=0):
    """the device call against the oracle and against _from_edges on the pass's own edges -> (ctx, result, expected)"""
    d = inp(name)
    E = expected(name, okey, min_support)
    ctx, r = device_call(name, okey, min_support)
    same_as_expected(r, E, "oracle: ")
    edges = ctx.neighbors_shifted(d["X"], d["p"], d["thr"])[0]
    s = r.stats
    n = d["n"]
    assert (s.n_edges, s.pairs_scored) == (edges.size, n * (n - 1) // 2) and (s.kernel_ms > 0 or n < 2)
    host = hammock_amd.Context(d["M"], device=-1)
    host.set_sequences(residues=d["res"], offsets=d["off"], sizes=d["sizes"])
    same_results(r, host.greedy_orders_from_edges(edges, d["thr"], d["maxc"], make_orders(n, *okey), min_support=min_support), "from_edges: ")
    return ctx, r, E


GPU_CASES = [("n1", ("id",)), ("n2", ("rev",)), ("n65", ("random", 5, 0)), ("noedge", ("random", 3, 0)), ("n40", ("id",)), ("n40", ("rev",)),
             ("n40", ("random", 9, 0)), ("n40", ("random", 65, 1)), ("n40", ("random", 256, 2)), ("n40", ("twice",)),
             ("n40_one_cluster", ("random", 4, 0)), ("n40_no_limit", ("random", 4, 0)), ("random400", ("random", 10, 0)),
             ("keyed", ("random", 3, 0)), ("sizes300", ("random", 6, 0)), ("negative", ("random", 5, 0)), ("ends", ("random", 3, 0)),
             ("crash", ("random", 10, 0))]


@pytest.mark.gpu
@pytest.mark.parametrize("name,okey", GPU_CASES, ids=[f"{a}-{'-'.join(str(v) for v in b)}" for a, b in GPU_CASES])
def test_greedy_orders_equals_the_oracle_and_from_edges(gpu, monkeypatch, capfd, name, okey):
    d = inp(name)
    if name == "keyed":   # the planner's timeline names the step only a key-sorted plan has
        monkeypatch.setenv("HMK_GREEDY_TIMING", "1")
        capfd.readouterr()
    ctx, r, E = against_both(name, okey)
    if name == "keyed":
        assert "[hmk plan] row-shared groups" in capfd.readouterr().err, "the plan of this case is not key-sorted"
        monkeypatch.delenv("HMK_GREEDY_TIMING")
    nv, k = E["n_valid"], len(E["rows"])
    if name in ("n1", "noedge"):   # every order throws: everybody alone, no partner, no pair
        assert nv == 0 and (r.consensus == np.arange(d["n"])).all() and not r.partners_ever.any() and r.support_edges.size == 0
        assert r.stats.n_edges == 0
    elif name in ("crash", "ends"):   # some orders throw, some do not
        assert 0 < nv < k
    else:
        assert nv == k and (r.stats.support_ms > 0) and (r.stats.relabel_ms > 0 or r.stats.n_edges == 0)
    if okey == ("id",) and name == "n40":   # the identity alone: hmk_greedy_cluster row for row, stats included
        cid, order, stats = ctx.greedy_cluster(d["X"], d["p"], d["thr"], d["maxc"])
        assert np.array_equal(r.cluster_id[0], cid) and np.array_equal(r.result_order[0, :stats.n_result_clusters], order)
        assert np.array_equal(r.member_rank[0], ctx.member_rank[:d["n"]])
        assert [int(r.per_order[0][f]) for f in SHARED] == [getattr(stats, f) for f in SHARED] and r.stats.n_edges == stats.n_edges
        assert r.per_order[0]["pairs_with_first"] == r.per_order[0]["pairs_together"] == r.stats.pairs_ever == r.stats.pairs_always
    if okey == ("twice",):   # the same order twice: every support is 2
        assert (hammock_amd.edge_fields(r.support_edges)[2] == 2).all() and r.stats.pairs_always == r.stats.pairs_ever > 0
        assert np.array_equal(r.cluster_id[0], r.cluster_id[1])
    if name == "negative":
        assert d["thr"] < 0 and (hammock_amd.edge_fields(ctx.neighbors_shifted(d["X"], d["p"], d["thr"])[0])[2] < 0).any()
    if name == "n40_no_limit":
        assert d["maxc"] == d["n"]
    if name == "ends":
        assert r.stats.n_edges > 10000


@pytest.mark.gpu
def test_the_edges_of_a_tiny_set_fall_into_one_segment(gpu):
    """the relabel's run offsets with 63 empty runs: the property of the input is read off the pass's own segment counts"""
    import torch
    d = inp("one_length")
    ctx = make_ctx("one_length", 0)
    cap = 1 << 16
    d_edges = torch.zeros(cap, dtype=torch.int64, device="cuda:0")
    d_counts = torch.zeros(N.HMK_EDGE_SHARDS, dtype=torch.int64, device="cuda:0")
    ctx.neighbors_shifted_dev(d["X"], d["p"], d["thr"], 0, 1, d_edges.data_ptr(), cap, d_counts.data_ptr())
    torch.cuda.synchronize()
    counts = d_counts.cpu().numpy()
    assert (counts > 0).sum() == 1 and counts.sum() > 20
    E = expected("one_length", ("random", 9, 0))
    assert E["n_valid"] > 1 and E["keys"].size > 0
    same_as_expected(device_call("one_length", ("random", 9, 0), ctx=ctx)[1], E)


@pytest.mark.gpu
@pytest.mark.parametrize("min_support", [0, 1, 4, 9])
def test_consensus_at_every_support_level(gpu, min_support):
    against_both("n40", ("random", 9, 0), min_support)


@pytest.mark.gpu
def test_a_support_level_above_the_valid_orders_is_reached_by_no_pair(gpu):
    E = expected("crash", ("random", 10, 0))
    ctx, r = device_call("crash", ("random", 10, 0), min_support=10)
    assert E["n_valid"] < 10 and (r.consensus == np.arange(inp("crash")["n"])).all() and r.stats.n_consensus == inp("crash")["n"]
    assert np.array_equal(r.partners_ever, E["ever"]) and r.stats.pairs_ever == E["keys"].size


@pytest.mark.gpu
def test_support_capacity(gpu):
    d = inp("n40")
    okey = ("random", 9, 0)
    E = expected("n40", okey)
    need = E["keys"].size
    ctx = make_ctx("n40", 0)
    for cap in (0, need - 1):
        with pytest.raises(BufferError, match=str(need)):
            device_call("n40", okey, ctx=ctx, support_capacity=cap)
        assert ctx.last_orders_needed == need
    same_as_expected(device_call("n40", okey, ctx=ctx, support_capacity=need)[1], E)
    r = device_call("n40", okey, ctx=ctx, support=False)[1]
    assert r.support_edges is None and ctx.last_orders_needed == need
    same_as_expected(r, E)
    r = device_call("n40", okey, ctx=ctx, arrays=False, per_order=False)[1]   # the rows not wanted: the supports need them all the same
    assert r.cluster_id is None and r.per_order is None
    assert np.array_equal(r.consensus, E["consensus"]) and np.array_equal(r.partners_ever, E["ever"]) and r.support_edges.size == need


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [1, 3])
def test_every_new_kernel_runs_its_later_iterations_on_a_capped_grid(gpu, monkeypatch, capfd, cap):
    d = inp("random400")
    okey = ("random", 4, 0)
    ctx = make_ctx("random400", 0)
    monkeypatch.setenv("HMK_TEST_GRID_CAP", str(cap))
    capfd.readouterr()
    _, r = device_call("random400", okey, ctx=ctx)
    lines = {}
    for kernel, wanted, launched in GRID_LINE.findall(capfd.readouterr().err):
        lines.setdefault(kernel, set()).add((int(wanted), int(launched)))
    monkeypatch.delenv("HMK_TEST_GRID_CAP")
    same_as_expected(r, expected("random400", okey))
    edges = ctx.neighbors_shifted(d["X"], d["p"], d["thr"])[0]
    assert edges.size > 3 * 1024
    for kernel in ("k_orders_relabel", "k_orders_support"):   # grids by chunk of 1,024 edges per segment: more than `cap` of them
        assert lines[kernel] and all(w > cap == l for w, l in lines[kernel]), (kernel, lines.get(kernel))


@pytest.mark.gpu
def test_two_calls_are_bit_identical_and_the_permuted_sizes_do_not_leak(gpu):
    d = inp("sizes300")
    okey = ("random", 6, 0)
    ctx = make_ctx("sizes300", 0)

    def others():
        cid, order, stats = ctx.greedy_cluster(d["X"], d["p"], d["thr"], d["maxc"])
        sweep = ctx.greedy_sweep(d["X"], d["p"], d["thr"], d["thr"] + 3, d["maxc"])
        return (cid.copy(), order.copy(), ctx.member_rank.copy(), np.sort(ctx.neighbors_shifted(d["X"], d["p"], d["thr"])[0]), *[a.copy() for a in sweep[1:]],
                *[sweep[0][f].copy() for f in sweep[0].dtype.names if f != "tail_ms"])

    before = others()
    _, a = device_call("sizes300", okey, ctx=ctx)
    after = others()
    _, b = device_call("sizes300", okey, ctx=ctx)
    for u, v in zip(before, after):
        assert np.array_equal(u, v)
    same_results(a, b)
    same_as_expected(b, expected("sizes300", okey))
    with pytest.raises(ValueError, match="min_support"):   # an early exit leaves the context as it was
        device_call("sizes300", okey, ctx=ctx, min_support=7)
    for u, v in zip(before, others()):
        assert np.array_equal(u, v)


@pytest.mark.gpu
def test_the_device_list_runs_on_the_root(gpu):
    d = inp("n65")
    ctx = hammock_amd.Context(matrix(), device=[0, 0])
    ctx.set_sequences(residues=d["res"], offsets=d["off"])
    same_as_expected(device_call("n65", ("random", 5, 0), ctx=ctx)[1], expected("n65", ("random", 5, 0)))


# ---- GPU: the mode ---------------------------------------------------------------------------------------------------------

STAGE1 = ("initial_clusters_sequences.tsv", "initial_clusters_sequences_original_order.tsv", "initial_clusters.tsv")


def partition(pairs):
    """[(cluster, sequence)] -> the set of clusters as sets of sequences"""
    by = {}
    for c, s in pairs:
        by.setdefault(c, set()).add(s)
    return {frozenset(v) for v in by.values()}


@pytest.mark.gpu
def test_cli_orders(gpu, tmp_path):
    """order 0 is what `hammock-hip greedy` clusters, order k what `hammock-hip greedy -R random -S seed` clusters; the consensus files
    against the definition (the meet of the valid orders' partitions); two runs byte-identical"""
    with open(os.path.join(GOLDEN, "musi.fa")) as fh:
        seqs = [line.strip() for line in fh if not line.startswith(">")][:300]
    rng = np.random.default_rng(5)
    fa = tmp_path / "in.fa"
    fa.write_text("".join(f">{k}|{int(rng.integers(1, 30))}|lab\n{s}\n" for k, s in enumerate(seqs)))
    common = ["-i", str(fa), "-g", "14", "-x", "3", "--initial_clusters_limit", "12"]
    runs = []
    for tag in ("a", "b"):
        r = cli("orders", *common, "--random_orders", "3", "-S", "41", "--pairs", "-d", str(tmp_path / tag), timeout=600)
        assert r.returncode == 0, r.stderr
        runs.append(tmp_path / tag)
    files = ("order_levels.tsv", "order_clusters.tsv", "sequence_support.tsv", "pair_support.tsv") + STAGE1
    for name in files:
        assert (runs[0] / name).read_bytes() == (runs[1] / name).read_bytes(), name
    levels = [line.split("\t") for line in (runs[0] / "order_levels.tsv").read_text().splitlines()]
    assert levels[0][:3] == ["order", "status", "clusters"] and [row[0] for row in levels[1:]] == ["size", "random:41", "random:42", "random:43"]
    table = [line.split("\t") for line in (runs[0] / "order_clusters.tsv").read_text().splitlines()]
    assert table[0] == ["sequence", "size", "random:41", "random:42", "random:43"] and len(table) == 1 + len(set(seqs))
    parts = []
    for k, extra in enumerate(([], ["-R", "random", "-S", "41"], ["-R", "random", "-S", "42"], ["-R", "random", "-S", "43"])):
        g = cli("greedy", *common, *extra, "-d", str(tmp_path / f"g{k}"), timeout=600)
        if g.returncode == 4:   # the reference throws in this order: the mode says so and leaves the order out
            assert levels[1 + k][1].startswith("reference_would_crash:") and all(row[1 + k] == "NA" for row in table[1:])
            continue
        assert g.returncode == 0 and levels[1 + k][1] == "ok", g.stderr
        want = partition((c, s) for c, s, _ in read_cluster_file(tmp_path / f"g{k}" / "initial_clusters_sequences.tsv"))
        got = partition((row[1 + k], row[0]) for row in table[1:])
        assert got == want, f"order {k}"
        assert int(levels[1 + k][2]) == len(want) and int(levels[1 + k][6]) == sum(len(c) * (len(c) - 1) // 2 for c in want)
        parts.append({s: c for c in want for s in c})
    assert len(parts) >= 2
    meet = partition((tuple(id(p[s]) for p in parts), s) for s in set(seqs))
    consensus = partition((c, s) for c, s, _ in read_cluster_file(runs[0] / "initial_clusters_sequences.tsv"))
    assert consensus == meet
    support = [line.split("\t") for line in (runs[0] / "sequence_support.tsv").read_text().splitlines()]
    assert support[0] == ["sequence", "cluster_in_order_0", "partners_always", "partners_ever", "consensus_cluster"]
    assert partition((row[4], row[0]) for row in support[1:]) == meet
    always = {s: len(c) - 1 for c in meet for s in c}
    assert all(int(row[2]) == always[row[0]] for row in support[1:])
    pairs = [line.split("\t") for line in (runs[0] / "pair_support.tsv").read_text().splitlines()][1:]
    together = {frozenset((a, b)) for p in parts for c in set(p.values()) for a in c for b in c if a < b}
    assert {frozenset(row[:2]) for row in pairs} == together and all(1 <= int(row[2]) <= len(parts) == int(row[3]) for row in pairs)
    assert "Consensus clusters:" in (runs[0] / "run.log").read_text()
