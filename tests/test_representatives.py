"""Representatives, the non-redundant subset of the set at one threshold or a range: hmk_representatives_shifted
(k_representatives.hip), hmk_representatives_from_edges, hmk_representatives_from_edges_dev and `hammock-hip representatives`.

The expected answer is never the code under test: a sequential Python loop in index order (i is a representative iff no
representative r < i is its neighbour) over the given edges for the synthetic graphs, over the C oracle's scores for peptide inputs;
covered_by and nearest follow from it with numpy.  Expectations are computed once per input and shared.  model_rounds is a numpy
model of the synchronous rounds of the device scheme (the kernel file's header describes them): the bound for n_rounds.
CPU part (host-only context): the symbols, _from_edges against the loop on every output for every synthetic graph and for MUSI's
oracle edges, every argument check, the device forms' DeviceError, the mode's argument and file errors.
GPU part: every synthetic graph through _from_edges_dev at the default grid and on 1 and 3 workgroups; the scoring call against the
loop and against _from_edges on its own edges; the grow path, state between calls, null outputs, the device list [0, 0], the
components the representatives lie in, the mode's files.
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, random_peptides
from test_assign import gpu   # noqa: F401  (the fixture that skips where no HIP device is visible)
from test_continue import cli

import hammock_amd
from hammock_amd import _native as N
from hammock_amd.synth import synth_peptides

FIELDS = ("n_edges", "n_representatives", "n_isolated", "largest")
THR = 20                     # the synthetic graphs' edges score THR + (k mod 9)
RANGES = [(20, 28), (20, 20), (23, 26)]   # all levels; a single one; edges below the threshold ignored and levels above threshold_hi clamped
EXTREME_RANGES = [(-32768, -32766), (-32768, -32768), (-6, 8)]   # the graph whose scores reach both ends of int16
GRID_LINE = re.compile(r"^\[hmk grid\] (\S+) (\d+) -> (\d+)$", re.M)
INT32_MAX = 2 ** 31 - 1


@functools.lru_cache(maxsize=None)
def matrix(name="blosum62"):
    import json
    with open(os.path.join(GOLDEN, "matrices.json")) as fh:
        return np.asarray(json.load(fh)["matrices"][name], dtype=np.int32)


# ---- the expectation -------------------------------------------------------------------------------------------------------

def sequential_level(n, x, m, sc, t):
    """the definition at one threshold -> (rep bool[n], covered_by, nearest, nearest_score, the level's counts)"""
    keep = sc >= t
    lo, hi, s = np.minimum(x[keep], m[keep]), np.maximum(x[keep], m[keep]), sc[keep]
    order = np.argsort(hi, kind="stable")
    lo_s, hi_s = lo[order], hi[order]
    start = np.searchsorted(hi_s, np.arange(n + 1))
    rep = np.ones(n, dtype=bool)
    for i in np.flatnonzero(start[1:] > start[:-1]).tolist():   # in index order: every smaller neighbour is decided
        rep[i] = not rep[lo_s[start[i]:start[i + 1]]].any()
    cov = np.arange(n, dtype=np.int64)
    near = np.arange(n, dtype=np.int64)
    nsc = np.full(n, INT32_MAX, dtype=np.int64)
    a = np.concatenate([lo, hi])   # every edge from both ends: a = the candidate representative, b = the other end
    b = np.concatenate([hi, lo])
    s2 = np.concatenate([s, s])
    pick = rep[a] & ~rep[b]
    a, b, s2 = a[pick], b[pick], s2[pick]
    low = np.full(n, n, dtype=np.int64)
    np.minimum.at(low, b, a)
    cov[~rep] = low[~rep]
    by = np.lexsort((a, -s2, b))   # per b: the largest score first, among equals the smaller index
    first = by[np.concatenate([[True], b[by][1:] != b[by][:-1]])] if by.size else by
    near[b[first]] = a[first]
    nsc[b[first]] = s2[first]
    assert (cov < n).all() and (cov[~rep] < np.flatnonzero(~rep)).all()
    touched = np.zeros(n, dtype=bool)
    touched[lo] = True
    touched[hi] = True
    counts = (int(keep.sum()), int(rep.sum()), int((~touched).sum()), int(np.bincount(near, minlength=n).max()) if n else 0)
    return rep, cov, near, nsc, counts


def sequential_levels(n, x, m, sc, thr, hi):
    """-> (covered_by, nearest, nearest_score: (levels, n) each, {field: array over thr ... hi})"""
    rows = [sequential_level(n, x, m, sc, t) for t in range(thr, hi + 1)]
    counts = {f: np.asarray([r[4][k] for r in rows], dtype=np.int64) for k, f in enumerate(FIELDS)}
    return tuple(np.stack([r[k] for r in rows]) for k in (1, 2, 3)) + (counts,)


def model_rounds(n, x, m, sc, t):
    """the synchronous rounds of the device scheme -> (rounds until no vertex is undecided, rep bool[n])"""
    keep = sc >= t
    lo, hi = np.minimum(x[keep], m[keep]), np.maximum(x[keep], m[keep])
    UND, REP, RED = 0, 1, 2
    state = np.zeros(n, dtype=np.int8)
    rounds = 0
    while True:
        rounds += 1
        sl, sh = state[lo], state[hi]
        redundant = np.zeros(n, dtype=bool)
        waits = np.zeros(n, dtype=bool)
        redundant[hi[(sl == REP) & (sh == UND)]] = True      # stamp 2r + 1
        both = (sl == UND) & (sh == UND)
        waits[hi[both]] = True                               # stamp 2r
        und = state == UND
        state[und & redundant] = RED
        state[und & ~redundant & ~waits] = REP
        lo, hi = lo[both], hi[both]
        if not (state == UND).any():
            return rounds, state == REP


def same(got, want, what="", rounds=None):
    """got = (levels, covered_by, nearest, nearest_score) of a call, each possibly None; rounds: None, 0 (the host form) or the
    model's bound per level"""
    levels, cov, near, nsc = got
    for arr, exp, kind, name in ((cov, want[0], np.uint32, "covered_by"), (near, want[1], np.uint32, "nearest"), (nsc, want[2], np.int32, "nearest_score")):
        if arr is not None:
            assert arr.dtype == kind and arr.shape == exp.shape and np.array_equal(arr.astype(np.int64), exp), what + name
    if levels is not None:
        for f in FIELDS:
            assert np.array_equal(levels[f].astype(np.int64), want[3][f]), what + f
        assert not levels["reserved"].any()
        if rounds is not None:
            assert (levels["n_rounds"] <= rounds).all() and ((levels["n_rounds"] > 0) == (np.asarray(rounds) > 0)).all(), what + "n_rounds"


def same_stats(s, want, n_levels):
    assert (s.n_edges, s.n_representatives, s.n_isolated, s.largest, s.n_levels) == tuple(int(want[3][f][0]) for f in FIELDS) + (n_levels,)


def properties(n, x, m, sc, thr, got):
    """asserted outright: no two representatives are adjacent; every other vertex has covered_by and nearest among its
    representative neighbours (nearest with the score of that edge)"""
    _, cov, near, nsc = got
    for l in range(cov.shape[0]):
        keep = sc >= thr + l
        a, b, s = x[keep].astype(np.int64), m[keep].astype(np.int64), sc[keep].astype(np.int64)
        rep = near[l] == np.arange(n)
        assert np.array_equal(rep, cov[l] == np.arange(n)) and (nsc[l][rep] == INT32_MAX).all()
        assert not (rep[a] & rep[b]).any()
        u, v, s2 = np.concatenate([a, b]), np.concatenate([b, a]), np.concatenate([s, s])
        adjacent = u * n + v                                   # the ordered pairs, and below with their scores (n < 2^24: below 2^63)
        scored = adjacent * 65536 + (s2 + 32768)
        other = np.flatnonzero(~rep)
        c, r, q = cov[l][other].astype(np.int64), near[l][other].astype(np.int64), nsc[l][other].astype(np.int64)
        assert rep[c].all() and np.isin(other * n + c, adjacent).all()
        assert rep[r].all() and np.isin((other * n + r) * 65536 + (q + 32768), scored).all()


# ---- the synthetic graphs --------------------------------------------------------------------------------------------------

def _gnm(rng, n, m):
    got = np.zeros((2, 0), dtype=np.int64)
    while got.shape[1] < m:
        a = rng.integers(0, n, size=(2, 2 * m))
        a = a[:, a[0] != a[1]]
        got = np.unique(np.concatenate([got, np.sort(a, axis=0)], axis=1), axis=1)
    return got[:, rng.permutation(got.shape[1])[:m]]


def _build(name):
    """-> (n, ends [2, E], shuffle, extra scores or None)"""
    rng = np.random.default_rng(4242)
    if name == "path_ascending":   # the deepest chain: one decision per round
        i = np.arange(1024)
        return 1025, np.stack([i, i + 1]), True, np.full(1024, THR + 3)
    if name == "path_relabelled":
        q = rng.permutation(4099)
        return 4099, np.stack([q[:-1], q[1:]]), True, None
    if name == "star_centre_last":   # every leaf is a representative, all keys contend for one word, the scores tie
        return 20000, np.stack([np.arange(19999), np.full(19999, 19999)]), True, None
    if name == "star_centre_first":   # one representative
        return 20000, np.stack([np.arange(1, 20000), np.zeros(19999, dtype=np.int64)]), True, np.full(19999, THR + 8)
    if name == "cliques":
        a, b = np.triu_indices(17, 1)
        base = np.repeat(np.arange(64) * 17, a.size)
        q = rng.permutation(64 * 17 + 500)
        return q.size, np.stack([q[base + np.tile(a, 64)], q[base + np.tile(b, 64)]]), True, None
    if name == "repeated":   # one pair 1,000 times, both orientations, different scores: its score is the maximum
        return 10, np.stack([np.full(1000, 3), np.full(1000, 7)]), True, None
    if name == "none":
        return 50, np.zeros((2, 0), dtype=np.int64), True, None
    if name.startswith("gnm_"):
        return 20000, _gnm(rng, 20000, int(name[4:])), True, None
    if name == "below_mixed":   # a third of the edges below THR: they would make many more sequences redundant
        ends = _gnm(rng, 5000, 9000)
        k = np.arange(9000)
        return 5000, ends, True, np.where(k % 3 == 0, THR - 1 - k % 5, THR + k % 9)
    if name == "extremes":   # both ends of int16 in the key's packing, and a negative threshold
        ends = _gnm(rng, 300, 900)
        return 300, ends, True, np.asarray([-32768, -32767, -32766, -5, 0, 7, 32766, 32767])[np.arange(900) % 8]
    raise KeyError(name)


GRAPHS = ["path_ascending", "path_relabelled", "star_centre_last", "star_centre_first", "cliques", "repeated", "none", "gnm_12000", "gnm_30000",
          "gnm_400000", "below_mixed", "extremes"]


def ranges(name):
    return EXTREME_RANGES if name == "extremes" else RANGES


@functools.lru_cache(maxsize=None)
def graph(name):
    """-> (n, x, m, sc, packed edges): both orientations occur, the order is shuffled with a fixed seed"""
    n, ends, shuffle, sc = _build(name)
    e = ends.shape[1]
    k = np.arange(e)
    sc = THR + k % 9 if sc is None else sc
    flip = np.random.default_rng(7).random(e) < 0.5
    x, m = np.where(flip, ends[1], ends[0]), np.where(flip, ends[0], ends[1])
    if shuffle:
        order = np.random.default_rng(8).permutation(e)
        x, m, sc = x[order], m[order], sc[order]
    return n, x, m, sc, hammock_amd.pack_edges(x, m, sc)


@functools.lru_cache(maxsize=None)
def graph_expect(name, thr, hi):
    n, x, m, sc, _ = graph(name)
    return sequential_levels(n, x, m, sc, thr, hi)


@functools.lru_cache(maxsize=None)
def graph_rounds(name, thr, hi):
    n, x, m, sc, _ = graph(name)
    out = []
    for l, t in enumerate(range(thr, hi + 1)):
        r, rep = model_rounds(n, x, m, sc, t)
        assert np.array_equal(rep, graph_expect(name, thr, hi)[1][l] == np.arange(n)), "the model of the rounds disagrees with the loop"
        out.append(r)
    return np.asarray(out)


@functools.lru_cache(maxsize=None)
def vertices(n):
    return synth_peptides(40, n, 12)   # any n distinct peptides


def graph_ctx(name, device):
    ctx = hammock_amd.Context(matrix(), device=device)
    ctx.set_sequences(residues=vertices(graph(name)[0])[0], offsets=vertices(graph(name)[0])[1])
    return ctx


# ---- peptide inputs and the oracle's scores ----------------------------------------------------------------------------------

def musi():
    with open(os.path.join(GOLDEN, "musi.fa")) as fh:
        return list(dict.fromkeys(line.strip() for line in fh if line.strip() and not line.startswith(">")))


@functools.lru_cache(maxsize=None)
def peptides(name):
    """-> (res, off, max shift, penalty, threshold, threshold_hi)"""
    if name == "musi":
        return hammock_amd.pack_sequences(musi()) + (3, 0, 20, 32)
    if name == "synth12":
        return synth_peptides(1, 3000, 12) + (3, 0, 20, 26)
    if name == "synth7to12":
        return synth_peptides(1, 3000, 7, 12) + (2, -1, 14, 20)
    if name == "keyed":   # one length, max shift 3: the plan is key-sorted (HMK_NO_KEY_SORT=1 is the other order)
        return synth_peptides(5, 5000, 12) + (3, 0, 20, 24)
    if name == "three_letters":   # dense: few representatives
        from oracle import c_oracle
        return c_oracle.pack(random_peptides(np.random.default_rng(77), 2000, 12, 12, alphabet=3)) + (3, 0, 14, 17)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def oracle_scores(name):
    """-> (n, x, m, sc) over every pair x < m with sc >= the input's threshold: ShiftedScorer.sequenceScore(seq1 = m, seq2 = x), the
    orientation of the pass's edges"""
    from oracle import c_oracle
    res, off, X, p, thr, _ = peptides(name)
    n = len(off) - 1
    x, m = np.triu_indices(n, 1)
    st, sc = c_oracle.score_pairs(matrix(), res, off, m, x, 0, X, p)
    assert st == 0
    keep = sc >= thr
    return n, x[keep], m[keep], sc[keep], int(sc.max())


@functools.lru_cache(maxsize=None)
def oracle_expect(name, thr, hi):
    n, x, m, sc, _ = oracle_scores(name)
    assert thr >= peptides(name)[4]
    return sequential_levels(n, x, m, sc, thr, hi)


def oracle_edges(name, thr):
    _, x, m, sc, _ = oracle_scores(name)
    keep = sc >= thr
    return hammock_amd.pack_edges(x[keep], m[keep], sc[keep])


def pep_ctx(name, device=0):
    res, off = peptides(name)[:2]
    ctx = hammock_amd.Context(matrix(), device=device)
    ctx.set_sequences(residues=res, offsets=off)
    return ctx


def raw(ctx, fn, head, thr, hi, covered_by=True, nearest=True, nearest_score=True, levels=True):
    """the C call with NULL where an output is not wanted -> (status, (levels, covered_by, nearest, nearest_score), stats)"""
    nl = min(max(hi - thr + 1, 1), 256)
    cov = np.zeros((nl, max(ctx.n, 1)), dtype=np.uint32)
    near = np.zeros((nl, max(ctx.n, 1)), dtype=np.uint32)
    nsc = np.zeros((nl, max(ctx.n, 1)), dtype=np.int32)
    lv = np.zeros(256, dtype=hammock_amd.api.REPRESENTATIVE_LEVEL_DTYPE)
    stats = N.RepresentativesStats()
    st = fn(ctx._h, *head, thr, hi, cov.ctypes.data_as(C.POINTER(C.c_uint32)) if covered_by else None,
            near.ctypes.data_as(C.POINTER(C.c_uint32)) if nearest else None, nsc.ctypes.data_as(C.POINTER(C.c_int32)) if nearest_score else None,
            lv.ctypes.data_as(C.POINTER(N.RepresentativeLevel)) if levels else None, C.byref(stats))
    return st, (lv[:nl] if levels else None, cov[:, :ctx.n] if covered_by else None, near[:, :ctx.n] if nearest else None,
                nsc[:, :ctx.n] if nearest_score else None), stats


# ---- CPU: the symbols ------------------------------------------------------------------------------------------------------

def test_symbols_are_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "hammock_hip.h")) as fh:
        header = fh.read()
    for name in ("hmk_representatives_shifted", "hmk_representatives_from_edges", "hmk_representatives_from_edges_dev"):
        assert re.search(r"\bint " + name + r"\(", header)
        assert name in N.SYMBOLS and hasattr(N.lib, name)
    assert "hmk_representative_level" in header and "hmk_representatives_stats" in header
    assert re.search(r"#define HMK_ABI_VERSION 4\b", header) and N.lib.hmk_abi_version() == 4
    assert C.sizeof(N.RepresentativeLevel) == 32 == hammock_amd.api.REPRESENTATIVE_LEVEL_DTYPE.itemsize and C.sizeof(N.RepresentativesStats) == 56


# ---- CPU: _from_edges against the sequential loop ------------------------------------------------------------------------------

@pytest.mark.parametrize("name", GRAPHS)
def test_from_edges_equals_the_sequential_loop_on_the_synthetic_graphs(name):
    n, x, m, sc, edges = graph(name)
    ctx = graph_ctx(name, -1)
    ep = (edges.ctypes.data_as(C.POINTER(C.c_uint64)), edges.size)
    for thr, hi in ranges(name):
        want = graph_expect(name, thr, hi)
        got = ctx.representatives_from_edges(edges, thr, hi)
        same(got, want, f"{thr}..{hi} ", rounds=np.zeros(hi - thr + 1, dtype=np.int64))
        s = ctx.last_representatives_stats
        same_stats(s, want, hi - thr + 1)
        assert (s.pairs_scored, s.kernel_ms, s.select_ms, s.rounds_total) == (0, 0.0, 0.0, 0)
        properties(n, x, m, sc, thr, got)
    thr, hi = ranges(name)[0]
    same(ctx.representatives_from_edges(edges, thr), graph_expect(name, thr, thr), "threshold_hi=None ")
    same(ctx.representatives_from_edges(edges[::-1].copy(), thr, hi), graph_expect(name, thr, hi), "reversed ")
    for k, only in enumerate(("covered_by", "nearest", "nearest_score", "levels")):   # each output alone
        st, got, _ = raw(ctx, N.lib.hmk_representatives_from_edges, ep, thr, hi, **{o: o == only for o in ("covered_by", "nearest", "nearest_score", "levels")})
        assert st == 0 and [g is not None for g in got] == [only == o for o in ("levels", "covered_by", "nearest", "nearest_score")]
        same(got, graph_expect(name, thr, hi), only + " alone ")


def test_the_reference_alone_the_inputs_are_not_degenerate():
    # the random graphs lie on both sides of n / 2 representatives; the special graphs are what their names say
    reps = [graph_expect(f"gnm_{m}", 20, 28)[3]["n_representatives"] for m in (12000, 30000, 400000)]
    assert reps[0][0] > 10000 > reps[1][0] > reps[2][0] > 1000 and reps[1][8] > 10000 > reps[2][8]
    assert all((np.diff(r) > 0).all() for r in reps)   # (here: fewer edges, more representatives)
    want = graph_expect("star_centre_last", 20, 28)
    assert want[3]["n_representatives"][0] == 19999 and want[0][0][19999] == 0
    n, x, m, sc, _ = graph("star_centre_last")
    best = np.flatnonzero(((x == 19999) | (m == 19999)) & (sc == 28))
    assert best.size > 1000 and want[1][0][19999] == np.minimum(x[best], m[best]).min() and want[2][0][19999] == 28   # a tie: the smaller index
    want = graph_expect("star_centre_first", 20, 28)
    assert (want[3]["n_representatives"] == 1).all() and (want[3]["largest"] == 20000).all()
    assert graph_expect("cliques", 20, 20)[3]["n_isolated"][0] == 500 and graph_expect("cliques", 20, 20)[3]["n_representatives"][0] == 564
    want = graph_expect("repeated", 20, 28)
    assert (want[3]["n_representatives"] == 9).all() and (want[2][:, 7] == 28).all() and (want[1][:, 7] == 3).all()
    assert want[3]["n_edges"].tolist() == [1000 - 111 * k - min(k, 1) for k in range(9)]
    assert graph_expect("path_ascending", 20, 23)[3]["n_representatives"].tolist() == [513] * 4
    assert graph_rounds("path_ascending", 20, 20)[0] == 1025 and graph_rounds("none", 20, 20)[0] == 1
    assert graph_expect("below_mixed", 20, 20)[3]["n_edges"][0] == 6000
    want = graph_expect("extremes", -32768, -32766)
    assert want[2].min() == -32768 and graph_expect("extremes", -6, 8)[2][graph_expect("extremes", -6, 8)[2] < INT32_MAX].max() == 32767


def test_from_edges_on_musi_equals_the_loop():
    n = oracle_scores("musi")[0]
    want = oracle_expect("musi", 20, 32)
    assert n == 2457 and [int(want[3]["n_representatives"][t - 20]) for t in (20, 26, 32)] == [133, 320, 707]   # (load order; the issue's figures)
    ctx = pep_ctx("musi", -1)
    got = ctx.representatives_from_edges(oracle_edges("musi", 20), 20, 32)
    same(got, want)
    _, x, m, sc, _ = oracle_scores("musi")
    keep = sc >= 30
    properties(n, x[keep], m[keep], sc[keep], 30, ctx.representatives_from_edges(oracle_edges("musi", 30), 30, 32))
    same(ctx.representatives_from_edges(oracle_edges("musi", 20), 26), oracle_expect("musi", 26, 26), "26 ")


# ---- CPU: the argument checks ------------------------------------------------------------------------------------------------

def test_bad_arguments_are_refused_before_the_device_is_looked_at():
    n, _, _, _, edges = graph("cliques")
    ctx = graph_ctx("cliques", -1)
    ep = (edges.ctypes.data_as(C.POINTER(C.c_uint64)), edges.size)
    heads = [(N.lib.hmk_representatives_shifted, (3, 0)), (N.lib.hmk_representatives_from_edges, ep), (N.lib.hmk_representatives_from_edges_dev, (None, 0))]
    nothing = dict(covered_by=False, nearest=False, nearest_score=False, levels=False)
    for fn, head in heads:   # the same checks in all three, on a host-only context
        assert raw(ctx, fn, head, 21, 20)[0] == N.HMK_ERR_BAD_ARG
        assert raw(ctx, fn, head, 20, 276)[0] == N.HMK_ERR_BAD_ARG
        assert raw(ctx, fn, head, -2 ** 31, 32767)[0] == N.HMK_ERR_BAD_ARG
        assert raw(ctx, fn, head, 32760, 32768)[0] == N.HMK_ERR_BAD_ARG
        assert raw(ctx, fn, head, 20, 22, **nothing)[0] == N.HMK_ERR_BAD_ARG
        assert fn(None, *head, 20, 20, None, None, None, None, None) == N.HMK_ERR_BAD_ARG
    assert raw(ctx, N.lib.hmk_representatives_from_edges, ep, 20, 275)[0] == 0   # 256 levels are allowed
    assert raw(ctx, N.lib.hmk_representatives_from_edges, ep, 32767, 32767)[0] == 0
    with pytest.raises(ValueError, match="threshold_hi"):
        ctx.representatives_from_edges(edges, 20, 19)
    for x, m in ((3, n), (n, 3), (2 ** 24 - 1, 0), (5, 5)):   # an index >= n either side, a self pair
        bad = edges.copy()
        bad[100] = hammock_amd.pack_edges(np.array([x]), np.array([m]), np.array([25]))[0]
        with pytest.raises(ValueError, match="outside"):
            ctx.representatives_from_edges(bad, 20, 28)
        bad[100] = hammock_amd.pack_edges(np.array([x]), np.array([m]), np.array([3]))[0]   # ... whatever its score
        with pytest.raises(ValueError, match="outside"):
            ctx.representatives_from_edges(bad, 20, 28)
    assert raw(ctx, N.lib.hmk_representatives_from_edges, (None, 5), 20, 20)[0] == N.HMK_ERR_BAD_ARG
    same(ctx.representatives_from_edges(edges, 20, 28), graph_expect("cliques", 20, 28), "after the refusals ")
    # a threshold below every score an edge can hold: score - threshold must not wrap
    far = hammock_amd.pack_edges(np.array([0, 2, 4, 6]), np.array([1, 3, 5, 7]), np.array([-32768, -2, 5, 32767]))
    for thr, hi, joined in ((-2 ** 31, -2 ** 31, 4), (-2 ** 31, -2 ** 31 + 255, 4), (32767, 32767, 1), (-40000, -39990, 4)):
        levels, cov, _, _ = ctx.representatives_from_edges(far, thr, hi)
        assert (levels["n_edges"] == joined).all() and (levels["n_representatives"] == n - joined).all() and ((cov != np.arange(n)).sum(axis=1) == joined).all()
    asym = matrix().copy()
    asym[3, 5] += 1
    actx = hammock_amd.Context(asym, device=-1)
    actx.set_sequences(residues=vertices(n)[0], offsets=vertices(n)[1])
    with pytest.raises(ValueError, match="symmetric"):
        actx.representatives_shifted(3, 0, 20)


def test_the_device_forms_need_a_device_and_an_empty_set_is_ok():
    ctx = graph_ctx("cliques", -1)
    with pytest.raises(hammock_amd.DeviceError):
        ctx.representatives_shifted(3, 0, 20, 24)
    with pytest.raises(hammock_amd.DeviceError):
        ctx.representatives_from_edges_dev(0, 0, 20, 24)
    empty = hammock_amd.Context(matrix(), device=-1)
    for call in (lambda: empty.representatives_from_edges(np.zeros(0, dtype=np.uint64), 20, 24), lambda: empty.representatives_shifted(3, 0, 20, 24),
                 lambda: empty.representatives_from_edges_dev(0, 0, 20, 24)):
        levels, cov, near, nsc = call()
        assert cov.shape == near.shape == nsc.shape == (5, 0) and levels.size == 5 and not any(levels[f].any() for f in FIELDS)
        assert empty.last_representatives_stats.n_levels == 5
    nothing = dict(covered_by=False, nearest=False, nearest_score=False, levels=False)
    assert raw(empty, N.lib.hmk_representatives_from_edges, (None, 0), 20, 24, **nothing)[0] == 0


def test_cli_representatives_argument_and_file_errors(tmp_path):
    fa = os.path.join(GOLDEN, "musi.fa")
    r = cli("representatives", "-d", str(tmp_path / "a"))
    assert r.returncode == 2 and "-i or --input" in r.stderr
    assert not (tmp_path / "a").exists()
    r = cli("representatives", "-i", fa, "--devices", "0,1", "-d", str(tmp_path / "a"))
    assert r.returncode == 2 and "--devices" in r.stderr
    r = cli("representatives", "-i", fa, "-f", "seq", "-d", str(tmp_path / "a"))
    assert r.returncode == 2 and "-f" in r.stderr
    assert not (tmp_path / "a").exists()
    r = cli("representatives", "-i", fa, "-g", "26", "--scan_to", "25", "-d", str(tmp_path / "b"))
    assert r.returncode == 2 and "--scan_to" in r.stderr
    r = cli("representatives", "-i", fa, "--scan_to", "276", "-d", str(tmp_path / "c"))   # the derived threshold is 20
    assert r.returncode == 2 and "--scan_to" in r.stderr and "20 up to 275" in r.stderr
    r = cli("representatives", "-i", fa, "-d", str(tmp_path / "c"))   # the directory exists now
    assert r.returncode == 2 and "Output directory exists" in r.stderr
    r = cli("representatives", "-i", str(tmp_path / "missing.fa"), "-d", str(tmp_path / "d"))
    assert r.returncode != 0
    r = cli("representatives", "-i", fa, "-l", "no_such_label", "-d", str(tmp_path / "e"))
    assert r.returncode == 3 and "No sequences" in r.stderr
    assert "hammock-hip representatives -i" in cli("--help").stderr


# ---- GPU: the synthetic graphs through the device kernels --------------------------------------------------------------------

def device_edges(edges):
    import torch
    return torch.from_numpy(edges.view(np.int64).copy()).to("cuda:0")


def wanted_grids(n, given, level_edges, single):
    """kernel -> the grids its launcher asks for (k_representatives.hip's and k_sweep.hip's launchers) on n vertices, `given` edges
    in the caller's block and level_edges[l] edges at level l; a launch over no edge is not made"""
    by_vertex = min(-(-n // 256), 2048)
    grids = {k: {by_vertex} for k in ("k_rep_init", "k_rep_decide", "k_rep_finish")}
    if not given:
        return grids
    if single:   # the level reads the caller's block itself
        chunks = [min(-(-given // 1024), 2048)]
    else:
        grids.update({k: {min(-(-given // 1024), 2048)} for k in ("k_sweep_hist", "k_sweep_deal")})
        chunks = [min(-(-e // 1024), 2048) for e in level_edges if e]
    if chunks:
        grids.update({k: set(chunks) for k in ("k_rep_mark_first", "k_rep_assign")})
    return grids


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [0, 1, 3])
@pytest.mark.parametrize("name", GRAPHS)
def test_from_edges_dev_equals_the_sequential_loop_on_the_synthetic_graphs(gpu, monkeypatch, capfd, name, cap):
    n, x, m, sc, edges = graph(name)
    ctx = graph_ctx(name, 0)
    d = device_edges(edges)
    if cap:
        monkeypatch.setenv("HMK_TEST_GRID_CAP", str(cap))
    for thr, hi in ranges(name):
        capfd.readouterr()
        want = graph_expect(name, thr, hi)
        bound = graph_rounds(name, thr, hi)
        got = ctx.representatives_from_edges_dev(d.data_ptr(), d.numel(), thr, hi)
        err = capfd.readouterr().err
        same(got, want, f"{thr}..{hi} ", rounds=bound)
        s = ctx.last_representatives_stats
        same_stats(s, want, hi - thr + 1)
        assert s.pairs_scored == 0 and s.kernel_ms == 0.0 and s.select_ms > 0.0 and s.rounds_total == int(got[0]["n_rounds"].sum())
        properties(n, x, m, sc, thr, got)
        lines = {}
        for kernel, wanted, launched in GRID_LINE.findall(err):
            assert int(launched) == cap
            lines.setdefault(kernel, set()).add(int(wanted))
        level_edges = [edges.size] if thr == hi else want[3]["n_edges"].tolist()
        cut = {k: {w for w in v if cap and w > cap} for k, v in wanted_grids(n, edges.size, level_edges, thr == hi).items()}
        cut = {k: v for k, v in cut.items() if v}
        # k_rep_mark, the rounds behind the second: its grid is the level's k_rep_mark_first grid.  A level that needs a third round
        # launches it; one that ends with its second round may have had the third in the queue already.
        mark = lines.pop("k_rep_mark", set())
        level_grid = [min(-(-e // 1024), 2048) for e in level_edges]
        must = {g for g, r in zip(level_grid, got[0]["n_rounds"].tolist()) if r > 2 and cap and g > cap}
        assert must <= mark <= {g for g in level_grid if cap and g > cap}
        assert {k: v for k, v in lines.items() if k.startswith(("k_rep_", "k_sweep_"))} == cut
        if name == "gnm_400000" and cap:   # here every grid-stride kernel runs its loop well beyond the first iteration
            assert set(cut) == set(wanted_grids(n, edges.size, level_edges, thr == hi)) and mark and all(w >= 2 * cap for v in cut.values() for w in v)


@pytest.mark.gpu
def test_from_edges_dev_refuses_invalid_edges_and_goes_on(gpu):
    n, _, _, _, edges = graph("gnm_12000")
    ctx = graph_ctx("gnm_12000", 0)
    for x, m in ((3, n), (n + 5, 3), (2 ** 24 - 1, 2 ** 24 - 2), (5, 5)):
        bad = edges.copy()
        bad[7000] = hammock_amd.pack_edges(np.array([x]), np.array([m]), np.array([25]))[0]
        d = device_edges(bad)
        with pytest.raises(ValueError, match="outside"):
            ctx.representatives_from_edges_dev(d.data_ptr(), d.numel(), 20, 28)
        with pytest.raises(ValueError, match="outside"):
            ctx.representatives_from_edges_dev(d.data_ptr(), d.numel(), 20)
        d = device_edges(edges)
        same(ctx.representatives_from_edges_dev(d.data_ptr(), d.numel(), 20, 28), graph_expect("gnm_12000", 20, 28), "the next call ")
    assert raw(ctx, N.lib.hmk_representatives_from_edges_dev, (None, 5), 20, 20)[0] == N.HMK_ERR_BAD_ARG


# ---- GPU: the scoring call -----------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", ["musi", "synth12", "synth7to12", "keyed", "three_letters"])
def test_representatives_shifted_equals_the_loop_on_oracle_scores_and_from_edges(gpu, monkeypatch, capfd, name):
    res, off, X, p, thr, hi = peptides(name)
    n = len(off) - 1
    ctx = pep_ctx(name)
    want = oracle_expect(name, thr, hi)
    if name == "keyed":   # the planner's timeline names the step only a key-sorted plan has
        monkeypatch.setenv("HMK_GREEDY_TIMING", "1")
        capfd.readouterr()
    got = ctx.representatives_shifted(X, p, thr, hi)
    if name == "keyed":
        assert "[hmk plan] row-shared groups" in capfd.readouterr().err, "the plan of this case is not key-sorted"
        monkeypatch.delenv("HMK_GREEDY_TIMING")
    same(got, want)
    s = ctx.last_representatives_stats
    same_stats(s, want, hi - thr + 1)
    assert s.pairs_scored == n * (n - 1) // 2 and s.kernel_ms > 0 and s.select_ms > 0 and s.rounds_total == int(got[0]["n_rounds"].sum())
    assert (got[0]["n_rounds"] >= 1).all() and (got[0]["n_rounds"] < 64).all()
    edges, _ = ctx.neighbors_shifted(X, p, thr)
    host = ctx.representatives_from_edges(edges, thr, hi)
    same(host, want, "from its own edges ")
    mid = 26 if name == "musi" else (thr + hi) // 2   # a single level: the pass's segments are read where they lie
    one = ctx.representatives_shifted(X, p, mid)
    same(one, oracle_expect(name, mid, mid), "single level ")
    for k in range(1, 4):   # ... and it is that row of the range call
        assert np.array_equal(one[k][0], got[k][mid - thr])
    assert one[0]["n_rounds"][0] == got[0]["n_rounds"][mid - thr]
    same_stats(ctx.last_representatives_stats, oracle_expect(name, mid, mid), 1)
    if name == "musi":
        assert [int(want[3]["n_representatives"][t - 20]) for t in (20, 26, 32)] == [133, 320, 707]
        x, m, sc = oracle_scores(name)[1:4]
        for l, t in enumerate(range(thr, hi + 1)):
            assert got[0]["n_rounds"][l] <= model_rounds(n, x, m, sc, t)[0]
    if name == "three_letters":
        assert want[3]["n_representatives"][0] < 100
    if name == "keyed":   # the other order of the pass: identical output
        monkeypatch.setenv("HMK_NO_KEY_SORT", "1")
        monkeypatch.setenv("HMK_GREEDY_TIMING", "1")
        other = pep_ctx(name)
        capfd.readouterr()
        plain = other.representatives_shifted(X, p, thr, hi)
        err = capfd.readouterr().err
        assert "[hmk plan] device copies" in err and "row-shared groups" not in err
        assert len(re.findall(r"^\[hmk representatives\] threshold \d+: \d+ rounds, live edges behind each:( \d+)+$", err, re.M)) == hi - thr + 1
        monkeypatch.delenv("HMK_NO_KEY_SORT")
        monkeypatch.delenv("HMK_GREEDY_TIMING")
        assert all(np.array_equal(a, b) for a, b in zip(plain[1:], got[1:])) and plain[0].tobytes() == got[0].tobytes()


@pytest.mark.gpu
def test_the_grow_path_gives_the_same(gpu, monkeypatch, capfd):
    """a first edge buffer of 2^20 entries (16,384 per segment) under 1.7 million edges: the pass is scored twice, which the
    call's timeline says"""
    res, off, X, p, thr, hi = peptides("three_letters")
    assert oracle_expect("three_letters", thr, hi)[3]["n_edges"][0] > 2 ** 20
    monkeypatch.setenv("HMK_EDGE_GUESS", "4096")
    monkeypatch.setenv("HMK_GREEDY_TIMING", "1")
    ctx = pep_ctx("three_letters")   # a fresh context: no buffer grown by an earlier call
    capfd.readouterr()
    got = ctx.representatives_shifted(X, p, thr, hi)
    err = capfd.readouterr().err
    monkeypatch.delenv("HMK_EDGE_GUESS")
    monkeypatch.delenv("HMK_GREEDY_TIMING")
    assert len(re.findall(r"^\[hmk\] an edge segment overflowed \(\d+ entries for 16384\): \d+ entries next, scoring again$", err, re.M)) == 1
    same(got, oracle_expect("three_letters", thr, hi))


@pytest.mark.gpu
def test_state_between_calls_null_outputs_and_a_threshold_above_every_score(gpu):
    res, off, X, p, thr, hi = peptides("musi")
    n = len(off) - 1
    ctx = pep_ctx("musi")
    first = ctx.representatives_shifted(X, p, 20, 32)
    same(first, oracle_expect("musi", 20, 32))
    same(ctx.representatives_shifted(X, p, 28, 31), oracle_expect("musi", 28, 31), "another range ")
    ctx.neighbors_shifted(X, p, 30)
    ctx.greedy_cluster(X, p, 26, 61)   # (the second loop of a clustering call uses the same progress word)
    again = ctx.representatives_shifted(X, p, 20, 32)
    assert all(np.array_equal(a, b) for a, b in zip(again[1:], first[1:])) and again[0].tobytes() == first[0].tobytes()
    outs = ("covered_by", "nearest", "nearest_score", "levels")
    for mask in range(1, 16):   # NULL outputs in each combination
        st, got, s = raw(ctx, N.lib.hmk_representatives_shifted, (X, p), 26, 29, **{o: bool(mask >> k & 1) for k, o in enumerate(outs)})
        assert st == 0 and [g is not None for g in got] == [bool(mask >> k & 1) for k in (3, 0, 1, 2)]
        same(got, oracle_expect("musi", 26, 29), f"outputs {mask:04b} ")
        same_stats(s, oracle_expect("musi", 26, 29), 4)
    top = oracle_scores("musi")[4]
    levels, cov, near, nsc = ctx.representatives_shifted(X, p, top, top + 2)
    assert levels["n_edges"][0] > 0 and levels["n_edges"][1] == 0
    for l in (1, 2):   # everyone is an isolated representative
        assert np.array_equal(cov[l], np.arange(n)) and np.array_equal(near[l], np.arange(n)) and (nsc[l] == INT32_MAX).all()
        assert levels[l].tolist()[:5] == (0, n, n, 1, 1)
    levels, cov, _, _ = ctx.representatives_shifted(X, p, top + 1)
    assert np.array_equal(cov[0], np.arange(n)) and levels[0].tolist()[:5] == (0, n, n, 1, 1)


@pytest.mark.gpu
def test_the_device_list_runs_on_the_root(gpu):
    res, off, X, p, thr, hi = peptides("synth12")
    ctx = hammock_amd.Context(matrix(), device=[0, 0])
    ctx.set_sequences(residues=res, offsets=off)
    same(ctx.representatives_shifted(X, p, thr, hi), oracle_expect("synth12", thr, hi))


@pytest.mark.gpu
@pytest.mark.parametrize("t", [26, 32])
def test_the_representatives_lie_in_their_sequences_components(gpu, t):
    res, off, X, p, _, _ = peptides("musi")
    n = len(off) - 1
    ctx = pep_ctx("musi")
    levels, cov, near, _ = ctx.representatives_shifted(X, p, t, t + 1)
    comp, clv = ctx.components_shifted(X, p, t, t + 1)
    assert np.array_equal(comp[cov[0]], comp) and np.array_equal(comp[near[0]], comp)
    assert np.array_equal(levels["n_isolated"], clv["n_singletons"]) and (levels["n_representatives"] >= clv["n_components"]).all()
    for k in (0, 1):
        assert int(levels["n_edges"][k]) == ctx.neighbors_shifted(X, p, t + k)[0].size


# ---- GPU: the mode ---------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_cli_representatives_on_musi(gpu, tmp_path):
    from oracle import c_oracle, hammock_oracle as po
    fa = os.path.join(GOLDEN, "musi.fa")
    seqs = po.load_unique_sequences_from_fasta(fa)
    labels = po.get_sorted_labels(seqs)
    initial = list(seqs)
    po.sort_sequences(seqs, "size")   # greedy's default order
    n = len(seqs)
    strings = [s.get_sequence_string() for s in seqs]
    res, off = c_oracle.pack(strings)
    x, m = np.triu_indices(n, 1)
    st, sc = c_oracle.score_pairs(matrix(), res, off, m, x, 0, 3, 0)
    assert st == 0
    keep = sc >= 26
    cov, near, nsc, lv = sequential_levels(n, x[keep], m[keep], sc[keep], 26, 30)
    members = {}
    for i, r in enumerate(near[0].tolist()):
        members.setdefault(r, []).append(seqs[i])
    ids = sorted(members, key=lambda r: (len(members[r]) == 1, r))   # groups of several sequences first, each part by ascending id
    clusters = [po.Cluster(list(members[r]), r + 1) for r in ids]
    exp = tmp_path / "exp"
    exp.mkdir()
    po.save_cluster_sequences_csv(clusters, str(exp / "initial_clusters_sequences.tsv"), labels)
    po.write_cluster_sequences_csv(initial, clusters, str(exp / "initial_clusters_sequences_original_order.tsv"), labels)
    po.save_clusters_csv(clusters, str(exp / "initial_clusters.tsv"), labels)
    rows = ["threshold\tedges\trepresentatives\tisolated\tlargest"]
    rows += ["\t".join(str(v) for v in [26 + k] + [int(lv[f][k]) for f in FIELDS]) for k in range(5)]
    per = ["sequence\trepresentative\tcovered_by\tnearest\tscore"]
    for i in range(n):
        rep = near[0][i] == i
        per.append("\t".join([strings[i], "1" if rep else "0", strings[cov[0][i]], strings[near[0][i]], "NA" if rep else str(int(nsc[0][i]))]))
    out = tmp_path / "out"
    r = cli("representatives", "-i", fa, "-d", str(out), "-g", "26", "--scan_to", "30", timeout=600)
    assert r.returncode == 0, r.stderr
    assert "Max shift not set. Setting automatically to: 3" in r.stderr
    assert (out / "representative_levels.tsv").read_text() == "\n".join(rows) + "\n"
    assert (out / "representatives.tsv").read_text() == "\n".join(per) + "\n"
    for name in ("initial_clusters_sequences.tsv", "initial_clusters_sequences_original_order.tsv", "initial_clusters.tsv"):
        assert (out / name).read_bytes() == (exp / name).read_bytes(), name
    log = (out / "run.log").read_text()
    assert 'Program started in mode "representatives"' in log and f"Resulting clusers: {len(clusters)}" in log and "Program successfully ended." in log
    assert f"Representatives at threshold 26: {int(lv['n_representatives'][0])}, without a neighbour: {int(lv['n_isolated'][0])}, largest group: {int(lv['largest'][0])}" in log
    # the representatives' file loads back: the same sequences in the same order, and no count is lost
    back = po.load_unique_sequences_from_fasta(str(out / "representatives.fa"))
    assert [s.get_sequence_string() for s in back] == [strings[r] for r in sorted(members)]
    assert sum(s.size() for s in back) == sum(s.size() for s in seqs)
    for s, r in zip(back, sorted(members)):
        assert s.size() == sum(q.size() for q in members[r])
    r = cli("check", "-i", str(out / "initial_clusters_sequences.tsv"), "-d", str(tmp_path / "c"), "-x", "3", "-g", "26", timeout=600)
    assert r.returncode == 0, r.stderr
    assert f" of {len(clusters)} clusters hold a pair below the threshold 26;" in (tmp_path / "c" / "run.log").read_text()
