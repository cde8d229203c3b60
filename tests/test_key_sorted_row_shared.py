"""Row-shared groups of the key-sorted 12-mer pass.  A row group whose 8 rows are all live and have the same
residue at both key positions reads ONE merged entry per column position where an ordinary group reads two (row positions 5
and 6), and each half of it goes to both accumulators of its plane.  None of this may show: the edge set (x, m, score) of the
default pass must be exactly the one with the row-shared bodies switched off (HMK_NO_ROW_SHARED=1) and the one of the caller's
order (HMK_NO_KEY_SORT=1), and sampled rows must match the oracle.  The cases are the smallest that break one piece each: row
groups of every kind against windows of every mode, rows past the end, lanes at the edges of the byte, tiles that do not
start at their row group's first column.
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
K0, K1 = 5, 6   # the key positions of 12-mers at max shift 3
SWITCHES = ("HMK_NO_KEY_SORT", "HMK_KEY_SORT_KEYS", "HMK_NO_ROW_SHARED")


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
    ctx = hammock_amd.Context(M, device=0)
    ctx.set_sequences(residues=res, offsets=off)
    got = edges_under(ctx, {}, thr)
    plan = ctx.last_plan()
    assert np.array_equal(got, edges_under(ctx, {"HMK_NO_ROW_SHARED": "1"}, thr))
    assert np.array_equal(got, edges_under(ctx, {"HMK_NO_KEY_SORT": "1"}, thr))
    if oracle_rows:
        check_rows(M, res, off, got, thr, oracle_rows)
    return got, plan


def group_kinds(res, off):
    """the row groups of the key-sorted order: (row-shared, full but not row-shared, with rows past the end)"""
    n = len(off) - 1
    k0, k1 = res[off[:-1] + K0].astype(np.int64), res[off[:-1] + K1].astype(np.int64)
    key = np.sort(k0 * 24 + k1, kind="stable")
    full = n // 8
    g = key[:full * 8].reshape(full, 8)
    shared = int(np.count_nonzero((g == g[:, :1]).all(axis=1)))
    return shared, full - shared, (n + 7) // 8 - full


def test_mixed_runs(M):
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
    shared, plain, partial = group_kinds(res, off)
    assert (shared, plain, partial) == (354, 21, 1)
    for thr in (THR, 12):   # 12: hits in most steps, scores are cut out of planes that the row-shared bodies produced
        same_edges(M, res, off, thr=thr, oracle_rows=24 if thr == THR else 6)


@pytest.mark.parametrize("n", [8, 9, 16, 23, 65, 257])
def test_rows_past_the_end(M, n):
    # every sequence has the same residues at 5 and 6: every full group is row-shared, and the last group of n % 8 != 0 has rows
    # past the end -- it must take an ordinary body (its dead rows' entries are zero; a merged entry would not be)
    res, off = synth_peptides(50 + n, n, 12)
    res = res.copy()
    res[off[:-1] + K0], res[off[:-1] + K1] = 17, 3
    assert group_kinds(res, off) == (n // 8, 0, 1 if n % 8 else 0)
    same_edges(M, res, off, thr=14)


def test_byte_lane_edges(M):
    # W at both key positions of every 12-mer (the largest cell, 11, at both): every full group is row-shared and the merged
    # entries hold the largest bytes there are.  classify() proves 8-bit lanes for thresholds 5 .. 80: at 80 the planes start at
    # the bottom of the byte, at 5 a pair that scored 12 x 11 would end at 255.  No pair of this input does: a sequence is never
    # scored against itself and under BLOSUM62 only W against W is 11, so these lanes stay below the top of the byte -- the
    # pairs that land on 0 and on 255 are test_score_field_edges.py's, which makes B an exact copy of W
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
    assert group_kinds(res, off) == (87, 0, 1)
    for thr in (80, 5):
        got, plan = same_edges(M, res, off, thr=thr, oracle_rows=12)
        assert plan.classes_rows == 1 and plan.classes_u16 == 0 and plan.classes_direct == 0
        assert len(got) > 0


def test_more_than_one_column_tile_per_row_group(M):
    # from 2 x 4,096 columns on a row group's columns are cut at least twice (hmk_plan.cpp, cols_per_tile): the merged entries
    # and the flag in tiles that do not start at the group's first column
    n = 9000
    res, off = synth_peptides(43, n, 12)
    shared, plain, _ = group_kinds(res, off)
    assert shared > 500 and plain > 50
    _, plan = same_edges(M, res, off, oracle_rows=0)
    per_group = [-(-(n - r0 - 1) // 4096) for r0 in range(0, n - 1, 8)]
    assert max(per_group) >= 3 and plan.n_tiles == sum(per_group)
