"""Start values of the key-sorted 12-mer pass.  The key table's key-0 entries hold the planes' initial lanes:
a window that shares key 0 starts its planes at the entry as loaded, one that shares both keys adds the key-1 entry, any
other window starts at the class's initial lanes.  The table belongs to the plan's (max shift, penalty, threshold).  None of
this may show: the edge set (x, m, score) of the default pass must be exactly the one of the caller's order
(HMK_NO_KEY_SORT=1) and of the one-key sort (HMK_KEY_SORT_KEYS=1), and sampled rows must match the oracle.  The cases are
the smallest that break one piece each: the mode changing from step to step inside a wave, rows past the end and partial
windows, two thresholds on one context, several column tiles per row group, lanes at the edges of the byte.
Run with -m gpu on an MI355X."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

import hammock_amd
from hammock_amd.synth import synth_peptides

pytestmark = pytest.mark.gpu

X, P, THR = 3, 0, 20
SWITCHES = ("HMK_NO_KEY_SORT", "HMK_KEY_SORT_KEYS")


@pytest.fixture(scope="module")
def M():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need an MI355X; no HIP device is visible")
    with open(os.path.join(GOLDEN, "matrices.json")) as fh:
        return np.asarray(json.load(fh)["matrices"]["blosum62"], dtype=np.int32)


def edges_under(ctx, env, thr=THR):
    """sorted edges of one pass with the given key-sort switches (read by the library at every call)"""
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


def check_rows(M, res, off, edges, thr, rows=24):
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


def same_edges(M, res, off, thr=THR, oracle_rows=24, one_key=True):
    ctx = hammock_amd.Context(M, device=0)
    ctx.set_sequences(residues=res, offsets=off)
    base = edges_under(ctx, {"HMK_NO_KEY_SORT": "1"}, thr)
    both = edges_under(ctx, {}, thr)
    plan = ctx.last_plan()
    assert np.array_equal(both, base)
    if one_key:
        assert np.array_equal(edges_under(ctx, {"HMK_KEY_SORT_KEYS": "1"}, thr), base)
    if oracle_rows:
        check_rows(M, res, off, base, thr, oracle_rows)
    return base, plan


def test_mode_changes_from_step_to_step(M):
    # runs of key 0 in the sorted order (key 0 = the run's index), each cut into equal runs of key 1: a wave's windows, 256
    # columns apart and shifted by 8 from one row group to the next, share both keys, then key 0 only, then nothing, then
    # both again, and end on every run's last column
    runs = [(1, 1), (63, 1), (64, 1), (65, 1), (255, 2), (256, 1), (257, 3), (700, 20), (700, 1), (640, 2)]
    keys = []
    for a, (length, n_k1) in enumerate(runs):
        keys += [(a, 23 - (k * n_k1) // length) for k in range(length)]
    n = len(keys)
    assert n == 3001
    res, off = synth_peptides(21, n, 12)
    place = np.random.default_rng(3).permutation(n)   # the caller's order has nothing of the sorted one
    res = res.copy()
    for k in range(n):
        res[off[place[k]] + 5], res[off[place[k]] + 6] = keys[k]
    for thr in (THR, 12):   # 12: hits in most steps, the hit path runs between the prologues
        same_edges(M, res, off, thr=thr, oracle_rows=24 if thr == THR else 6)


@pytest.mark.parametrize("n", [2, 9, 63, 65, 257, 1001])
def test_rows_past_the_end_and_partial_windows(M, n):
    # n % 8 != 0 (a row group with rows past the end: their key-0 entries hold the initial lane alone), last windows with a
    # single live column, a last batch behind which keyrun ends
    res, off = synth_peptides(30 + n, n, 12)
    same_edges(M, res, off, thr=14)
    # every column in one run of both keys: no window is left out
    res = res.copy()
    for k in range(n):
        res[off[k] + 5], res[off[k] + 6] = 17, 3
    same_edges(M, res, off, thr=14)


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


def test_two_thresholds_on_one_context(M):
    # 20, 14, 20 on ONE context: the second plan's key table holds other initial lanes than the first's, and a table left
    # over from the other threshold would show.  A quarter of the pairs are hits: a wave's stage fills within a few steps and
    # the flush is called between steps
    res, off = family_set(5, 3000, 4, 2)
    ctx = hammock_amd.Context(M, device=0)
    ctx.set_sequences(residues=res, offsets=off)
    got = [edges_under(ctx, {}, thr) for thr in (20, 14, 20)]
    assert len(got[1]) > 3000 * 3000 // 16
    base = hammock_amd.Context(M, device=0)
    base.set_sequences(residues=res, offsets=off)
    want = {thr: edges_under(base, {"HMK_NO_KEY_SORT": "1"}, thr) for thr in (20, 14)}
    assert np.array_equal(got[0], want[20])
    assert np.array_equal(got[1], want[14])
    assert np.array_equal(got[2], want[20])
    check_rows(M, res, off, got[1], 14, rows=6)


def test_more_than_one_column_tile_per_row_group(M):
    # the planner's column runs are at least 4,096 columns long (hmk_plan.cpp, cols_per_tile): from 2 x 4,096 columns on a row
    # group's columns are cut at least twice, and the tile's key-table and run-word bases start at a column that is not the
    # row group's first
    n = 9000
    res, off = synth_peptides(41, n, 12)
    _, plan = same_edges(M, res, off, oracle_rows=0, one_key=False)
    # the triangle: the row group at r0 has the columns (r0, n), in runs of at most 4,096
    per_group = [-(-(n - r0 - 1) // 4096) for r0 in range(0, n - 1, 8)]
    assert max(per_group) >= 3 and plan.n_tiles == sum(per_group)


def test_byte_lane_edges(M):
    # W at both key positions of every 12-mer (the largest cell, 11, at both), the rest from residues with large cells.
    # classify() proves 8-bit lanes for any pair of 12-mers at max shift 3 for thresholds 5 .. 80 (BLOSUM62: bias 4, largest
    # cell 11; lane = 128 - thr - 4 * cells + sum of biased cells, 0 <= lane <= 255 for 12 cells): at 80 the planes start at
    # the bottom of the byte (initial lane 0 in the unshifted plane), at 5 start value + both key cells is as large as it gets
    # (75 + 15 + 15 in the unshifted plane, 123 + 11 * 12 = 255 for a row of W against itself)
    rng = np.random.default_rng(9)
    rich = "WCHYPFW"
    bases = ["".join(rng.choice(list(rich), 12)) for _ in range(6)] + ["W" * 12]
    seqs = []
    for k in range(700):
        s = list(bases[k % len(bases)])
        for _ in range(k % 3):
            s[rng.integers(0, 12)] = rich[rng.integers(0, len(rich))]
        s[5] = s[6] = "W"
        seqs.append("".join(s))
    res, off = hammock_amd.pack_sequences(seqs)
    for thr in (80, 5):
        base, plan = same_edges(M, res, off, thr=thr, oracle_rows=12)
        assert plan.classes_rows == 1 and plan.classes_u16 == 0 and plan.classes_direct == 0
        assert len(base) > 0
    # one past the upper end the class leaves the 8-bit tier (the case above stood ON the edge)
    ctx = hammock_amd.Context(M, device=0)
    ctx.set_sequences(residues=res, offsets=off)
    edges_under(ctx, {}, 81)
    assert ctx.last_plan().classes_u8 == 0
