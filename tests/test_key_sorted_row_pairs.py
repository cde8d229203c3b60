"""Sixteen-row tiles of the key-sorted 12-mer pass.  A paired plan's tile holds two row groups behind ONE column
set-up: the column's fetch, its table offsets, the run words and the window's mode are worked out once per step and serve both
groups, each with its own key-table entries, its own row-shared flag and its own body.  None of this may show: the edge set
(x, m, score) of the pass with pairing forced on (HMK_KEY_ROW_PAIRS=1) must be exactly the one with it forced off
(HMK_KEY_ROW_PAIRS=0) and the one of the caller's order (HMK_NO_KEY_SORT=1), and sampled rows must match the oracle.  The cases
are the smallest that break one piece each: a second group that is absent, partial or full, the triangle's mask inside a
diagonal tile, groups of different kinds in one tile, a stage that fills between the two groups of a step, lanes at the edges
of the byte, column tiles that do not start at the tile's first column, and the planner's size rule at both ends.
The GPU tests run with -m gpu on an MI355X; the two checks of the constructed inputs need none."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

import hammock_amd
from hammock_amd.synth import synth_peptides

gpu = pytest.mark.gpu

X, P, THR = 3, 0, 20
K0, K1 = 5, 6   # the key positions of 12-mers at max shift 3
SWITCHES = ("HMK_NO_KEY_SORT", "HMK_KEY_SORT_KEYS", "HMK_NO_ROW_SHARED", "HMK_KEY_ROW_PAIRS")


@pytest.fixture(scope="module")
def M():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need an MI355X; no HIP device is visible")
    with open(os.path.join(GOLDEN, "matrices.json")) as fh:
        return np.asarray(json.load(fh)["matrices"]["blosum62"], dtype=np.int32)


def edges_under(ctx, env, thr=THR):
    """sorted edges of one pass with the given switches (read by the library at every call)"""
    keep = {k: os.environ.get(k) for k in SWITCHES}
    try:
        for k in keep:
            os.environ.pop(k, None)
        os.environ.update(env)
        e, _ = ctx.neighbors_shifted(X, P, thr)
        return np.sort(np.asarray(e, dtype=np.uint64))
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def check_rows(M, res, off, edges, thr, rows):
    """every edge of a few sampled rows, against the oracle's scores of those rows"""
    from oracle import c_oracle
    n = len(off) - 1
    x, m, s = hammock_amd.edge_fields(edges)
    rng = np.random.default_rng(11)
    for r in rng.choice(n, min(rows, n), replace=False):
        others = np.delete(np.arange(n, dtype=np.uint32), r)
        st, sc = c_oracle.score_pairs(M, res, off, others, np.full(len(others), r, dtype=np.uint32), 0, X, P)
        assert st == 0
        hit = sc >= thr
        want = sorted(zip(np.minimum(others[hit], r).tolist(), np.maximum(others[hit], r).tolist(), sc[hit].tolist()))
        sel = (x == r) | (m == r)
        got = sorted(zip(x[sel].tolist(), m[sel].tolist(), s[sel].tolist()))
        assert got == want, f"row {r}"


def same_edges(M, res, off, thr=THR, oracle_rows=24):
    """paired == unpaired == caller's order; -> (edges, the paired plan, the unpaired plan)"""
    ctx = hammock_amd.Context(M, device=0)
    ctx.set_sequences(residues=res, offsets=off)
    got = edges_under(ctx, {"HMK_KEY_ROW_PAIRS": "1"}, thr)
    plan = ctx.last_plan()
    assert np.array_equal(got, edges_under(ctx, {"HMK_KEY_ROW_PAIRS": "0"}, thr))
    plan8 = ctx.last_plan()
    assert np.array_equal(got, edges_under(ctx, {"HMK_NO_KEY_SORT": "1"}, thr))
    n = len(off) - 1
    assert plan.pairs_scored == plan8.pairs_scored == n * (n - 1) // 2
    if n > 16:
        assert plan.n_tiles < plan8.n_tiles   # the switch reached the planner
    if oracle_rows:
        check_rows(M, res, off, got, thr, oracle_rows)
    return got, plan, plan8


def tile_kinds(res, off):
    """the 16-row tiles of the key-sorted order by what their two groups are, (group 0, group 1) row-shared or not -- a group
    with rows past the end, or none at all, is not: {(True, True): ..., (True, False): ..., (False, True): ..., (False, False): ...}"""
    n = len(off) - 1
    k0, k1 = res[off[:-1] + K0].astype(np.int64), res[off[:-1] + K1].astype(np.int64)
    key = np.sort(k0 * 24 + k1, kind="stable")
    shared = [8 * g + 8 <= n and bool((key[8 * g:8 * g + 8] == key[8 * g]).all()) for g in range(2 * ((n + 15) // 16))]
    kinds = {(a, b): 0 for a in (True, False) for b in (True, False)}
    for t in range(len(shared) // 2):
        kinds[(shared[2 * t], shared[2 * t + 1])] += 1
    return kinds


def tiles_of(n, rows, cols):
    """tiles of the triangle of n rows: per row chunk its columns after the chunk's first row, cut into runs of at most `cols`"""
    return sum(-(-(n - r0 - 1) // cols) for r0 in range(0, n - 1, rows))


def equal_key_set(n):
    res, off = synth_peptides(50 + n, n, 12)
    res = res.copy()
    res[off[:-1] + K0], res[off[:-1] + K1] = 17, 3
    return res, off


def mixed_runs_set():
    # runs of equal (res[5], res[6]) in the sorted order, (key 0, key 1, length), some inside longer runs of equal res[5]: group
    # boundaries (every 8 sorted positions) fall on and off run boundaries, so row-shared groups, groups equal at position 5
    # only and groups equal at neither meet windows that share both keys, position 5 only and nothing
    runs = [(0, 0, 1), (0, 1, 7), (0, 2, 8), (0, 3, 9), (1, 0, 15), (1, 1, 16), (1, 2, 17), (2, 0, 63), (3, 0, 64), (4, 0, 65),
            (5, 0, 250), (5, 1, 700), (5, 2, 65), (6, 3, 700), (7, 0, 250), (7, 1, 64), (7, 2, 63), (8, 0, 1), (8, 1, 1), (8, 2, 1),
            (9, 0, 17), (9, 1, 16), (9, 2, 15), (9, 3, 9), (9, 4, 8), (9, 5, 7), (9, 6, 1), (10, 0, 1), (11, 0, 1), (12, 7, 250),
            (13, 0, 8), (13, 1, 8), (14, 0, 64), (15, 0, 9), (16, 1, 200), (17, 0, 27)]
    keys = [(a, b) for a, b, length in runs for _ in range(length)]
    n = len(keys)
    assert n == 3001
    res, off = synth_peptides(23, n, 12)
    place = np.random.default_rng(5).permutation(n)   # the caller's order has nothing of the sorted one
    res = res.copy()
    for k in range(n):
        res[off[place[k]] + K0], res[off[place[k]] + K1] = keys[k]
    return res, off


ENDS = [9, 15, 16, 17, 23, 24, 25, 33, 257]


# ---- the constructed inputs are what the GPU cases take them for (no GPU) ----------------------------------------------------

def test_group_kinds_of_the_constructed_inputs():
    for n in ENDS:
        res, off = equal_key_set(n)
        full, last = divmod(n, 16)
        want = {(True, True): full, (True, False): 1 if last >= 8 else 0, (False, True): 0, (False, False): 1 if 0 < last < 8 else 0}
        assert tile_kinds(res, off) == want, n
    res, off = mixed_runs_set()
    kinds = tile_kinds(res, off)
    assert sum(kinds.values()) == 188 and all(v > 0 for v in kinds.values()), kinds
    # (354 row-shared groups, 21 full ordinary ones and one with rows past the end, as the 8-row tests count them)
    assert 2 * kinds[(True, True)] + kinds[(True, False)] + kinds[(False, True)] == 354


def test_tile_count_formula():
    # 16-row chunks halve the row chunks; the columns of a chunk start after its first row
    assert tiles_of(17, 16, 4096) == 1 and tiles_of(18, 16, 4096) == 2 and tiles_of(17, 8, 4096) == 2
    # n = 9,000: the chunks with more than 8,192 columns are cut three times, those with more than 4,096 twice
    assert tiles_of(9000, 8, 4096) == sum(-(-(9000 - r0 - 1) // 4096) for r0 in range(0, 8999, 8)) == 3 * 101 + 2 * 512 + 512
    assert tiles_of(9000, 16, 4096) == 3 * 51 + 2 * 256 + 256


# ---- GPU ---------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("n", ENDS)
def test_rows_past_the_end_in_either_group(M, n):
    # every sequence has the same residues at 5 and 6: every full group is row-shared, the last tile has 1 to 16 live rows and its
    # second group is absent, partial (an ordinary body: its dead rows' entries are zero; a merged entry would not be) or full
    res, off = equal_key_set(n)
    same_edges(M, res, off, thr=14)


@gpu
def test_triangle_masking_of_the_second_group(M):
    # the columns row0 + 1 .. row0 + 15 of a diagonal tile are masked differently for the two groups (g = 0: the rows below the
    # column; g = 1: the same, counted from row0 + 8).  Threshold 12 gives random 12-mers enough hits that a pair kept or dropped
    # on the wrong side of the diagonal shows against the caller's order and the oracle (all 257 rows)
    res, off = synth_peptides(77, 257, 12)
    got, plan, _ = same_edges(M, res, off, thr=12, oracle_rows=257)
    assert plan.n_tiles == tiles_of(257, 16, 4096) == 16
    assert len(got) > 0


@gpu
def test_groups_of_different_kinds_in_one_tile(M):
    res, off = mixed_runs_set()
    kinds = tile_kinds(res, off)
    assert all(v > 0 for v in kinds.values()), kinds   # (shared, ordinary), (ordinary, shared), both, neither
    for thr in (THR, 12):   # 12: hits in most steps, scores are cut out of planes that the row-shared bodies produced
        same_edges(M, res, off, thr=thr, oracle_rows=24 if thr == THR else 6)


def family_set(seed, n, bases, mutations):
    """n 12-mers, each one of a few base peptides with some residues redrawn: hits are dense at any threshold"""
    rng = np.random.default_rng(seed)
    base_res, _ = synth_peptides(seed, bases, 12)
    base_res = base_res.reshape(bases, 12)
    rows = base_res[rng.integers(0, bases, n)].copy()
    for _ in range(mutations):
        rows[np.arange(n), rng.integers(0, 12, n)] = rng.integers(0, 20, n)
    off = (np.arange(n + 1, dtype=np.uint32) * 12).astype(np.uint32)
    return np.ascontiguousarray(rows.reshape(-1).astype(np.uint8)), off


@gpu
def test_dense_hits(M):
    # One group of a wave's step tests 64 columns x 8 rows = 512 pairs; with more than 1/16 of the pairs hits (asserted) that is
    # more than 32 records per group and step on average.  A wave's stage holds 640 records and is flushed once more than 576
    # are staged, so it fills after at most 18 group-steps, i.e. 9 steps of two groups -- and a tile of up to 2,999 columns gives
    # a wave 12 steps: every wave of a tile away from the triangle's tip flushes inside its append loop, and over 188 tiles x 4
    # waves the fill falls after group 0 (the flush then runs BETWEEN the two groups of a step, group 1 appending to an emptied
    # stage behind the same column set-up) as often as after group 1
    res, off = family_set(5, 3000, 4, 2)
    got, plan, _ = same_edges(M, res, off, thr=14, oracle_rows=6)
    assert len(got) * 16 > plan.pairs_scored


@gpu
def test_byte_lane_edges(M):
    # W at both key positions of every 12-mer (the largest cell, 11, at both): every full group is row-shared and the merged
    # entries and the key table's start values hold the largest bytes there are.  classify() proves 8-bit lanes for thresholds
    # 5 .. 80: at 80 the planes start at the bottom of the byte, at 5 a pair that scored 12 x 11 would end at 255
    rng = np.random.default_rng(9)
    rich = "WCHYPFW"
    bases = ["".join(rng.choice(list(rich), 12)) for _ in range(6)] + ["W" * 12]
    seqs = []
    for k in range(700):
        s = list(bases[k % len(bases)])
        for _ in range(k % 3):
            s[rng.integers(0, 12)] = rich[rng.integers(0, len(rich))]
        s[K0] = s[K1] = "W"
        seqs.append("".join(s))
    res, off = hammock_amd.pack_sequences(seqs)
    assert tile_kinds(res, off) == {(True, True): 43, (True, False): 1, (False, True): 0, (False, False): 0}
    for thr in (80, 5):
        got, plan, _ = same_edges(M, res, off, thr=thr, oracle_rows=12)
        assert plan.classes_rows == 1 and plan.classes_u16 == 0 and plan.classes_direct == 0
        assert len(got) > 0


@gpu
def test_more_than_one_column_tile_per_16_row_tile(M):
    # from 2 x 4,096 columns on a tile's columns are cut at least twice: both groups' merged entries, flags and key-table
    # entries in tiles that do not start at the tile's first column.  With no switch a set this small keeps its 8-row tiles
    n = 9000
    res, off = synth_peptides(43, n, 12)
    _, plan, plan8 = same_edges(M, res, off, oracle_rows=0)
    assert plan.n_tiles == tiles_of(n, 16, 4096) and plan8.n_tiles == tiles_of(n, 8, 4096)
    ctx = hammock_amd.Context(M, device=0)
    ctx.set_sequences(residues=res, offsets=off)
    edges_under(ctx, {})
    assert ctx.last_plan().n_tiles == tiles_of(n, 8, 4096)


@gpu
def test_the_rule_at_full_size(M):
    # 10^5 synthetic 12-mers: the planner pairs by itself, with 16,384 columns per tile
    n = 100000
    res, off = synth_peptides(1, n, 12)
    ctx = hammock_amd.Context(M, device=0)
    ctx.set_sequences(residues=res, offsets=off)
    got = edges_under(ctx, {})
    plan = ctx.last_plan()
    assert plan.n_tiles == tiles_of(n, 16, 16384)
    assert plan.pairs_scored == n * (n - 1) // 2
    assert np.array_equal(got, edges_under(ctx, {"HMK_KEY_ROW_PAIRS": "0"}))
    assert ctx.last_plan().n_tiles == tiles_of(n, 8, 32768)
    check_rows(M, res, off, got, THR, 4)
