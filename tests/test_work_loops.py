"""The work loops of the grid-stride kernels beyond their first iteration (HMK_TEST_GRID_CAP, hmk_grid.h).

At every shape the other files test, a launch of k_linkage, k_split, k_pairs, k_assign, k_match, k_merge or k_search.hip gets as many
workgroups as it has chunks, tiles or long runs: each workgroup's loop runs once, and what the loop carries into a second
iteration -- LDS counters cleared and flushed, rows restaged while other waves may still read them, a RunTable that must be empty
again, the barrier ahead of all that -- is product code for inputs of 10^6 sequences that no test has run.  The switch gives those
launches min(their own grid, n) workgroups, so the existing inputs walk the loops: n = 1, one workgroup takes everything, and n = 3,
which divides none of the counts, so that a workgroup's consecutive items belong to different slots while the other workgroups
hit the same accumulators.

Every comparison is with the oracle-side expectation the other files compute (never with an uncapped GPU result), and every case
asserts the "[hmk grid] <kernel> <wanted> -> <launched>" line of the kernels it is about, with wanted >= 2 x launched: without the
line the cap did nothing and the case would pass vacuously.  Where the wanted grid follows from the input alone it is asserted too.
The inputs are the other files' (built here as there, same seeds); two calls lower a threshold so that the segment kernels have
more than 2,048 x 2 x cap edges in some segment (they are named where they are made).
"""
import functools
import re

import numpy as np
import pytest

from conftest import random_peptides
from test_assign import gpu   # noqa: F401  (the fixture that skips where no HIP device is visible)
from test_linkage import check as check_linkage, device_ctx, reduce_scores, score_inside, sized_case
from test_split import family_expect, numpy_stats, oracle_split, same
import test_assign as A
import test_match as MA
import test_merge as ME
import test_search as S

import hammock_amd
from hammock_amd.synth import synth_peptides

pytestmark = pytest.mark.gpu

VAR = "HMK_TEST_GRID_CAP"
CAPS = [1, 3]
LINE = re.compile(r"^\[hmk grid\] (\S+) (\d+) -> (\d+)$", re.M)
LINK_FLAT_MAX = LINK_TILE = 256
SPLIT_ROWS = 64
LONG_RUN = 4096
SHARDS, SEG_EDGES = 64, 2048   # HMK_EDGE_SHARDS; edges per workgroup that seg_grid_x plans


def capped(monkeypatch, capfd, cap, call):
    """call() under HMK_TEST_GRID_CAP=cap -> (its result, {kernel: [(wanted, launched), ...]} from the call's stderr)"""
    monkeypatch.setenv(VAR, str(cap))
    capfd.readouterr()
    try:
        out = call()
    finally:
        monkeypatch.delenv(VAR)
    lines = {}
    for name, wanted, launched in LINE.findall(capfd.readouterr().err):
        lines.setdefault(name, []).append((int(wanted), int(launched)))
    return out, lines


def cut(lines, cap, kernel, wanted=None, at_least=None):
    """the kernel's launches were cut to `cap` workgroups from at least twice as many (`wanted`: from exactly that many)"""
    assert kernel in lines, (kernel, sorted(lines))
    for w, launched in lines[kernel]:
        assert launched == cap and w >= 2 * cap, (kernel, w, launched)
        if wanted is not None:
            assert w == wanted, (kernel, w, wanted)
        if at_least is not None:
            assert w >= at_least, (kernel, w, at_least)


def ceil_div(a, b):
    return -(-a // b)


def link_grids(mc, members=True):
    """(flat chunks, tiles, init workgroups, split items, split items past their slot's last row) of a slot assignment"""
    sizes = np.bincount(mc)
    flat = sum(int(s) * (int(s) - 1) // 2 for s in sizes if s <= LINK_FLAT_MAX)
    tiles = items = skipped = 0
    for s in (int(s) for s in sizes if s > LINK_FLAT_MAX):
        blocks = ceil_div(s, LINK_TILE)
        tiles += blocks * (blocks + 1) // 2
        for i in range(blocks):   # row block i has i + 1 tiles of LINK_TILE / SPLIT_ROWS quarters
            for part in range(LINK_TILE // SPLIT_ROWS):
                items += i + 1
                skipped += (i + 1) * (i * LINK_TILE + part * SPLIT_ROWS >= s)
    init = ceil_div(max(len(sizes), mc.size if members else 0), 256)
    return ceil_div(flat, 256), tiles, init, items, skipped


# ---- linkage ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("members", [True, False], ids=["members", "slots_only"])
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("seed", [1, 2])
def test_linkage_sized_families(gpu, monkeypatch, capfd, seed, cap, members):
    """mixed lengths and 12-mers, 17 flat and 5 tiled slots: 242 chunks, 24 tiles (and 14 workgroups of k_linkage_init) on 1 and 3
    workgroups -- the top-of-loop barriers, lmin / lbelow / span, rowseq / rowidx / rmin / rbelow from one item to the next"""
    Mx, res, off, mc, ncl, X, p, thr, (a, b, slot, sc) = sized_case(seed)
    nm = mc.size
    assert link_grids(mc, members)[:3] == (242, 24, 14 if members else 1)
    want, stats = reduce_scores(a, b, slot, sc, nm, ncl, thr)
    ctx = device_ctx(Mx, res, off)
    got, lines = capped(monkeypatch, capfd, cap, lambda: ctx.cluster_linkage_shifted(0, nm, mc, ncl, X, p, thr, members=members))
    check_linkage(got, want, ctx, stats)
    assert (got[4] is None) == (not members)
    cut(lines, cap, "k_linkage_flat", 242)
    cut(lines, cap, "k_linkage_tiled", 24)
    if members:
        cut(lines, cap, "k_linkage_init", 14)
    else:
        assert "k_linkage_init" not in lines   # 24 slots: one workgroup anyway


def test_linkage_threshold_edge(gpu, monkeypatch, capfd):
    """test_linkage.test_threshold_edge's pairs of calls on 3 workgroups: n_below at and one above a slot's lowest score"""
    Mx, res, off, mc, ncl, X, p, thr, (a, b, slot, sc) = sized_case(2)
    want, _ = reduce_scores(a, b, slot, sc, mc.size, ncl, thr)
    ctx = device_ctx(Mx, res, off)
    for c in (int(np.flatnonzero(np.bincount(mc) == 700)[1]), int(np.flatnonzero(np.bincount(mc) == 65)[1])):   # a tiled slot, a flat one
        lowest = int(want[0][c])
        attained = int((sc[slot == c] == lowest).sum())
        at, lines = capped(monkeypatch, capfd, 3, lambda: ctx.cluster_linkage_shifted(0, mc.size, mc, ncl, X, p, lowest))
        assert at[3][c] == 0 and at[0][c] == lowest
        check_linkage(at, reduce_scores(a, b, slot, sc, mc.size, ncl, lowest)[0])
        cut(lines, 3, "k_linkage_flat", 242)
        cut(lines, 3, "k_linkage_tiled", 24)
        above, lines = capped(monkeypatch, capfd, 3, lambda: ctx.cluster_linkage_shifted(0, mc.size, mc, ncl, X, p, lowest + 1))
        assert above[3][c] == attained >= 1
        check_linkage(above, reduce_scores(a, b, slot, sc, mc.size, ncl, lowest + 1)[0])
        cut(lines, 3, "k_linkage_flat", 242)
        cut(lines, 3, "k_linkage_tiled", 24)


def test_cap_below_one_changes_nothing(gpu, monkeypatch, capfd):
    """HMK_TEST_GRID_CAP=0: no launch is cut, no line is written"""
    Mx, res, off, mc, ncl, X, p, thr, (a, b, slot, sc) = sized_case(2)
    want, stats = reduce_scores(a, b, slot, sc, mc.size, ncl, thr)
    ctx = device_ctx(Mx, res, off)
    got, lines = capped(monkeypatch, capfd, 0, lambda: ctx.cluster_linkage_shifted(0, mc.size, mc, ncl, X, p, thr))
    check_linkage(got, want, ctx, stats)
    assert lines == {}
    got, lines = capped(monkeypatch, capfd, -3, lambda: ctx.cluster_linkage_shifted(0, mc.size, mc, ncl, X, p, thr))
    check_linkage(got, want, ctx, stats)
    assert lines == {}


# ---- split -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("seed,dthr", [(1, 0), (2, 0), (2, 6)])
def test_split_sized_families(gpu, monkeypatch, capfd, seed, dthr, cap):
    """the same families through k_split_flat (242 chunks) and k_split_tiled (96 quarter tiles, of which the workgroup skips, ahead
    of its barrier, the 27 that start past their slot's last row: 12 of them in the two 257-member slots)"""
    Mx, res, off, mc, ncl, X, p, thr, scored = sized_case(seed)
    thr += dthr
    assert link_grids(mc)[0] == 242 and link_grids(mc)[3:] == (96, 27)
    assert link_grids(np.repeat([0, 1], 257))[3:] == (24, 12)
    want = family_expect(seed, dthr, 8)
    ctx = device_ctx(Mx, res, off)
    got, lines = capped(monkeypatch, capfd, cap, lambda: ctx.clinkage_split(0, mc.size, mc, ncl, X, p, thr))
    same(got, want)
    s = ctx.last_split_stats
    assert (s.pairs_scored, s.n_edges, s.n_multi, s.n_split) == numpy_stats(mc, ncl, scored, thr)
    assert s.n_result_clusters == int(want[1].sum()) and s.crash_slot == -1
    cut(lines, cap, "k_split_flat", 242)
    cut(lines, cap, "k_split_tiled", 96)


# ---- one input for the tile loops ------------------------------------------------------------------------------------------

TILE_SIZES = [257, 320, 512, 513]
TILE_SUBS = [2, 5, 2, 5]   # substitutions at most, as test_linkage.sized_families' two sets
TILE_THR = 20


def tile_loop_case():
    """four tiled slots around one centre each, drawn as test_linkage.sized_families draws: 12-mers, X = 3, p = 0, all strings
    distinct, members shuffled.  3 + 3 + 3 + 6 = 15 tiles: one workgroup runs, back to back, a full diagonal tile, a one-row tile
    and a one-member diagonal tile (257), a 64-row tile (320), full tiles (512) and those of a third row block of one row (513)"""
    rng = np.random.default_rng(88_500)
    peps, mc, seen = [], [], set()
    for c, (size, max_sub) in enumerate(zip(TILE_SIZES, TILE_SUBS)):
        centre = rng.integers(0, 20, size=12).astype(np.uint8)
        added = 0
        while added < size:
            q = centre.copy()
            for pos in rng.choice(12, size=int(rng.integers(0, max_sub + 1)), replace=False):
                q[pos] = rng.integers(0, 20)
            if q.tobytes() in seen:
                continue
            seen.add(q.tobytes())
            peps.append(q)
            mc.append(c)
            added += 1
    perm = rng.permutation(len(peps))
    res, off = hammock_amd.pack_sequences([peps[k] for k in perm])
    return res, off, np.asarray(mc, dtype=np.uint32)[perm]


def test_tile_loops_on_one_workgroup(gpu, coracle, monkeypatch, capfd):
    """linkage and split of four slots of 257, 320, 512 and 513 members under cap 1: 15 tiles / 60 quarter tiles on one workgroup"""
    Mx = A._blosum62()
    res, off, mc = tile_loop_case()
    nm, ncl, X, p, thr = mc.size, 4, 3, 0, TILE_THR
    assert np.bincount(mc).tolist() == TILE_SIZES
    flat, tiles, init, items, skipped = link_grids(mc)
    assert (flat, tiles, init, items) == (0, 15, 7, 60) and skipped == 6 + 6 + 9
    a, b, slot, sc = score_inside(coracle, Mx, res, off, mc, X, p)
    want, stats = reduce_scores(a, b, slot, sc, nm, ncl, thr)
    want_split = oracle_split(Mx, res, off, mc, ncl, X, p, thr)
    # the oracle's side alone: slots that hold together and slots that split at this threshold
    assert (want_split[1] == 1).any() and (want_split[1] > 1).any()
    assert np.array_equal(want_split[1] == 1, want[3] == 0)
    ctx = device_ctx(Mx, res, off)
    for members in (True, False):
        got, lines = capped(monkeypatch, capfd, 1, lambda: ctx.cluster_linkage_shifted(0, nm, mc, ncl, X, p, thr, members=members))
        check_linkage(got, want, ctx, stats)
        cut(lines, 1, "k_linkage_tiled", 15)
        assert "k_linkage_flat" not in lines and ("k_linkage_init" in lines) == members
        if members:
            cut(lines, 1, "k_linkage_init", 7)
    got, lines = capped(monkeypatch, capfd, 1, lambda: ctx.clinkage_split(0, nm, mc, ncl, X, p, thr))
    same(got, want_split)
    s = ctx.last_split_stats
    assert (s.pairs_scored, s.n_edges, s.n_multi, s.n_split) == numpy_stats(mc, ncl, (a, b, slot, sc), thr)
    cut(lines, 1, "k_split_tiled", 60)
    assert "k_split_flat" not in lines


# ---- the pair probes -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cap", CAPS)
def test_pairs_shifted_and_with_shift(gpu, matrices, coracle, monkeypatch, capfd, cap):
    """test_gpu_parity.test_pairs_shifted_vs_oracle's 40,000 pairs (157 chunks) at X = 3, p = -1 through hmk_score_pairs_shifted and
    hmk_score_with_shift, the latter's score and shift against the oracle's on every pair"""
    rng = np.random.default_rng(1)
    Mx = matrices["blosum62"]
    peps = random_peptides(rng, 500, 7, 32, alphabet=24)
    res, off = hammock_amd.pack_sequences(peps)
    ctx = device_ctx(Mx, res, off)
    i = rng.integers(0, len(peps), 40000).astype(np.uint32)
    j = rng.integers(0, len(peps), 40000).astype(np.uint32)
    st, want = coracle.score_pairs(Mx, res, off, i, j, 0, 3, -1)
    assert st == 0
    got, lines = capped(monkeypatch, capfd, cap, lambda: ctx.score_pairs_shifted(i, j, 3, -1))
    assert np.array_equal(got, want)
    cut(lines, cap, "k_pairs<0>", 157)
    (score, shift), lines = capped(monkeypatch, capfd, cap, lambda: ctx.score_with_shift(i, j, 3, -1))
    cut(lines, cap, "k_pairs<0>", 157)
    each = [coracle.shifted_score(Mx, peps[x], peps[y], 3, -1) for x, y in zip(i, j)]
    assert all(st == 0 for st, _, _ in each)
    assert np.array_equal(score, [s for _, s, _ in each]) and np.array_equal(shift, [sh for _, _, sh in each])
    assert np.array_equal(score, want) and (shift > 0).any() and (shift < 0).any()


@pytest.mark.parametrize("cap", CAPS)
def test_pairs_local_and_literal_block(gpu, matrices, coracle, monkeypatch, capfd, cap):
    """test_gpu_parity.test_pairs_local_vs_oracle's 30,000 pairs (118 chunks) at gaps -5, -1, and a dense block of 100 x 400 of the
    same sequences on the literal tier (gaps 3, -1: a positive penalty), 157 chunks: k_pairs<1>'s DP rows in LDS from pair to pair"""
    rng = np.random.default_rng(2)
    Mx = matrices["blosum62"]
    peps = random_peptides(rng, 400, 1, 32, alphabet=24)
    res, off = hammock_amd.pack_sequences(peps)
    ctx = device_ctx(Mx, res, off)
    i = rng.integers(0, len(peps), 30000).astype(np.uint32)
    j = rng.integers(0, len(peps), 30000).astype(np.uint32)
    st, want = coracle.score_pairs(Mx, res, off, i, j, 1, -5, -1)
    assert st == 0
    got, lines = capped(monkeypatch, capfd, cap, lambda: ctx.score_pairs_local(i, j, -5, -1))
    assert np.array_equal(got, want)
    cut(lines, cap, "k_pairs<1>", 118)
    st, want = coracle.score_block(Mx, res, off, np.arange(100), np.arange(400), 1, 3, -1)
    assert st == 0
    got, lines = capped(monkeypatch, capfd, cap, lambda: ctx.score_block_local(0, 100, 0, 400, 3, -1))
    assert np.array_equal(got, want)
    cut(lines, cap, "k_pairs<1>", 157)


# ---- assign, match, merge: long runs on few workgroups, a run after a class-split run on the same table -------------------------

def cut_segments(lines, cap, total):
    """k_assign_count / _scatter: some segment holds at least total / 64 edges, so the grid wanted is at least that over 2,048"""
    floor = ceil_div(ceil_div(total, SHARDS), SEG_EDGES)
    assert floor >= 2 * cap, (total, floor)
    cut(lines, cap, "k_assign_count", at_least=floor)
    cut(lines, cap, "k_assign_scatter", at_least=floor)


@pytest.mark.parametrize("cap", CAPS)
def test_assign_long_runs_many_clusters(gpu, coracle, monkeypatch, capfd, cap):
    """test_assign.test_assign_long_runs[many_clusters] at k = 32: 30 runs of more than 4,096 hits next to more than 1,536 clusters
    each, so every run is walked in classes -- and the next run of the workgroup starts on the table it leaves"""
    Mx = A._blosum62()
    rng = np.random.default_rng(12)
    res0, off0 = synth_peptides(42, 6030, 12)
    seqs = [np.asarray(res0[off0[i]:off0[i + 1]]) for i in range(6030)]
    new, members = seqs[:30], seqs[30:]
    mc = A.relabel(np.arange(6000) // 2)
    ctx, res, off, qr, rr, ids, msz = A.setup(Mx, new, members, mc, rng)
    blk = A.block(coracle, Mx, res, off, qr, rr, 0, 3, 0)
    thr = int(np.percentile(blk, 5))
    hits = (blk >= thr).sum(axis=0)
    assert (hits > LONG_RUN).sum() == 30 >= 6
    assert min(len(np.unique(mc[blk[:, x] >= thr])) for x in range(len(new))) > 1536
    want = A.expected(blk, mc, ids, msz, thr, 32)
    assert want[2].min() > 32
    got, lines = capped(monkeypatch, capfd, cap, lambda: ctx.assign_shifted(*qr, *rr, mc, ids, 3, 0, thr, 32))
    A.check(got, want)
    cut(lines, cap, "k_assign_block", min(30, int(hits.sum()) // (LONG_RUN + 1)))
    cut(lines, cap, "k_assign_wave", 8)
    if cap == 1:
        cut_segments(lines, cap, int(hits.sum()))


@pytest.mark.parametrize("cap", CAPS)
def test_assign_uniform_12mers_wave_and_segment_kernels(gpu, coracle, monkeypatch, capfd, cap):
    """test_assign.test_assign_uniform_12mers' input at k = 32 (2,000 new sequences, 500 workgroups of k_assign_wave) at threshold 5
    instead of 30: the 10^6 edges it keeps put more than 10,240 into some segment, six workgroups' worth for the segment kernels"""
    Mx = A._blosum62()
    rng = np.random.default_rng(100 + 32)
    members, mc, new = A.families(rng, 3000, 2000, 12, 12)
    mc = A.relabel(mc)
    ctx, res, off, qr, rr, ids, msz = A.setup(Mx, new, members, mc, rng)
    blk = A.block(coracle, Mx, res, off, qr, rr, 0, 3, 0)
    thr = 5
    hits = (blk >= thr).sum(axis=0)
    assert hits.max() <= LONG_RUN and hits.sum() > SHARDS * SEG_EDGES * 5
    want = A.expected(blk, mc, ids, msz, thr, 32)
    assert (want[2] > 32).any() and (want[2] < 32).any()
    got, lines = capped(monkeypatch, capfd, cap, lambda: ctx.assign_shifted(*qr, *rr, mc, ids, 3, 0, thr, 32))
    A.check(got, want)
    assert ctx.last_assign_stats.n_edges == int(hits.sum())
    cut(lines, cap, "k_assign_wave", 500)
    cut_segments(lines, cap, int(hits.sum()))


@pytest.mark.parametrize("cap", CAPS)
def test_match_long_runs_many_clusters(gpu, coracle, monkeypatch, capfd, cap):
    """test_match.test_match_long_runs[many_clusters] at k = 32: 30 long runs in level 1, 10 in level 2, all walked in classes"""
    Mx = A._blosum62()
    rng = np.random.default_rng(42)
    seqs = MA.synth_seqs(42, 6030)
    queries, members = seqs[:30], seqs[30:]
    mc = A.relabel(np.arange(6000) // 2)
    qc = A.relabel(np.arange(30) // 3)
    ctx, res, off, qr, rr, ids, msz = MA.setup(Mx, queries, members, mc, rng)
    blk = MA.block(coracle, Mx, res, off, qr, rr, 0, 3, 0)
    thr = int(np.percentile(blk, 5))
    hits, distinct, rec2, distinct2 = MA._run_stats(blk, mc, qc, thr)
    assert (hits > LONG_RUN).sum() == 30 and (rec2 > LONG_RUN).sum() == 10 >= 6
    assert distinct.min() > 1536 and distinct2.min() > 1536
    want = MA.expected(blk, mc, ids, msz, qc, thr, 32)
    assert want[2].min() > 32
    got, lines = capped(monkeypatch, capfd, cap, lambda: ctx.match_clusters_shifted(*qr, qc, *rr, mc, ids, 3, 0, thr, 32))
    MA.check(got, want)
    max_long = int(hits.sum()) // (LONG_RUN + 1)
    cut(lines, cap, "k_match_feasible_block", min(30, max_long))
    cut(lines, cap, "k_match_select_block", min(10, max_long))
    cut(lines, cap, "k_match_feasible_wave", 8)
    cut(lines, cap, "k_match_copy", 8)
    if cap == 1:
        cut(lines, cap, "k_match_select_wave", 3)
        cut_segments(lines, cap, int(hits.sum()))


@pytest.mark.parametrize("cap", CAPS)
def test_match_uniform_12mers_wave_kernels(gpu, coracle, monkeypatch, capfd, cap):
    """test_match.test_match_uniform_12mers' input at k = 32: 2,000 query members in some 800 query clusters, the size at which
    k_match_count (256 members per workgroup) wants 8 workgroups and the wave kernels hundreds"""
    Mx = A._blosum62()
    rng = np.random.default_rng(400 + 32)
    members, mc, queries, qc = MA.two_sides(rng, 3000, 2000, 12, 12)
    mc = A.relabel(mc)
    nb = int(qc.max()) + 1
    ctx, res, off, qr, rr, ids, msz = MA.setup(Mx, queries, members, mc, rng)
    blk = MA.block(coracle, Mx, res, off, qr, rr, 0, 3, 0)
    want = MA.expected(blk, mc, ids, msz, qc, 30, 32)
    multi = np.bincount(qc) > 1
    assert (want[2][multi] > 0).mean() > 0.2 and (want[2] == 0).any() and (want[2][multi] > 1).any()
    got, lines = capped(monkeypatch, capfd, cap, lambda: ctx.match_clusters_shifted(*qr, qc, *rr, mc, ids, 3, 0, 30, 32))
    MA.check(got, want)
    cut(lines, cap, "k_match_count", 8)
    cut(lines, cap, "k_match_feasible_wave", 500)
    cut(lines, cap, "k_match_copy", 500)
    cut(lines, cap, "k_match_select_wave", ceil_div(nb, 4))


@functools.lru_cache(maxsize=None)
def graph_case(layout):
    """test_merge.test_cluster_graph_table_paths' input of that layout with the oracle's feasible slot pairs, run lengths and
    neighbouring slots (computed once per session, read-only)"""
    from oracle import c_oracle
    Mx = A._blosum62()
    rng = np.random.default_rng(64)
    n = 4000
    peps = random_peptides(rng, n, 12, 12, alphabet=3)
    mc = A.relabel(np.concatenate([np.arange(2000), 2000 + np.arange(2000) // 2])) if layout != "block" else A.relabel(np.arange(n) // 10)
    X, p = 3, 0
    res, off = hammock_amd.pack_sequences(peps)
    st, sample = c_oracle.score_block(Mx, res, off, np.arange(200, dtype=np.uint32), np.arange(200, n, dtype=np.uint32), 0, X, p)
    assert st == 0
    thr = int(np.percentile(sample, 40 if layout != "block" else 5))
    want, run, near = ME.expected_pairs(c_oracle, Mx, res, off, 0, n, mc, X, p, thr)
    for arr in (res, off, mc, want, run, near):
        arr.setflags(write=False)
    return Mx, res, off, mc, X, p, thr, want, run, near


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("layout", ["wave_and_block_overflow", "block", "block_eight_byte_entries"])
def test_cluster_graph_table_paths(gpu, monkeypatch, capfd, layout, cap):
    """test_merge.test_cluster_graph_table_paths' two dense layouts: hundreds of long runs on 1 and 3 workgroups of k_merge_block, in
    the first layout each split into classes; 3,000 / 400 slots over the waves of k_merge_wave and k_merge_compact.  The block layout
    once more under HMK_ADJ_8BYTE=1: the same runs through the kernels' other instantiation, k_merge_wave / _block<false>"""
    inst = "<true>"
    if layout == "block_eight_byte_entries":
        monkeypatch.setenv("HMK_ADJ_8BYTE", "1")
        layout, inst = "block", "<false>"
    Mx, res, off, mc, X, p, thr, want, run, near = graph_case(layout)
    n, ncl = mc.size, int(mc.max()) + 1
    if layout == "wave_and_block_overflow":
        assert ((run <= LONG_RUN) & (near > 384)).sum() > 100 and ((run > LONG_RUN) & (near > 1536)).sum() > 100
    else:
        assert (run > LONG_RUN).all() and (near <= 1536).all()
    assert (run > LONG_RUN).sum() >= 6 and len(want) > 100
    ctx = device_ctx(Mx, res, off)
    got, lines = capped(monkeypatch, capfd, cap, lambda: ctx.cluster_pairs_shifted(0, n, mc, ncl, X, p, thr))
    assert np.array_equal(np.sort(got), want)
    cut(lines, cap, "k_merge_block" + inst, min(ncl, int(run.sum()) // (LONG_RUN + 1), 1024))
    cut(lines, cap, "k_merge_wave" + inst, ceil_div(ncl, 4))
    assert sorted(k for k in lines if k.startswith(("k_merge_wave", "k_merge_block"))) == ["k_merge_block" + inst, "k_merge_wave" + inst]
    cut(lines, cap, "k_merge_compact", ceil_div(ncl, 4))
    cut(lines, cap, "k_merge_len", 16)


# ---- search ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cap", CAPS)
def test_search_segment_kernels(gpu, coracle, monkeypatch, capfd, cap):
    """test_search.test_search_best_k's input (300 queries, 2,200 references with duplicates) at k = 5, and the thresholded search
    of the same rectangle, at a threshold every pair passes instead of 20: 660,000 edges, more than 10,240 in some segment, which
    is what makes k_search_count / _scatter / _compact want six workgroups per segment (at 20 the input has 1,651 edges)"""
    Mx = A._blosum62()
    res, off = synth_peptides(31, 2300, 12)
    seqs = S.split_seqs(res, off)
    seqs = seqs + seqs[300:500]          # duplicate references: tied scores, the lower index first
    ctx, res, off = S.ctx_with(Mx, seqs)
    Q, n, thr = 300, len(seqs), -1000
    blk, want_edges = S.oracle_hits(coracle, Mx, res, off, np.arange(Q), np.arange(Q, n), 0, 3, 0, thr)
    total = Q * (n - Q)
    assert len(want_edges) == total == 660_000
    floor = ceil_div(ceil_div(total, SHARDS), SEG_EDGES)
    assert floor == 6 >= 2 * cap
    (idx, sc), lines = capped(monkeypatch, capfd, cap, lambda: ctx.search_best_shifted(0, Q, Q, n, 3, 0, thr, 5))
    widx, wsc = S.numpy_best(blk, np.arange(Q, n), thr, 5)
    assert np.array_equal(idx, widx) and np.array_equal(sc, wsc)
    cut(lines, cap, "k_search_count", at_least=floor)
    cut(lines, cap, "k_search_scatter", at_least=floor)
    (edges, _), lines = capped(monkeypatch, capfd, cap, lambda: ctx.search_shifted(0, Q, Q, n, 3, 0, thr))
    assert np.array_equal(np.sort(edges), want_edges)
    cut(lines, cap, "k_search_compact", at_least=floor)
