"""The tile tables of a key-sorted 12-mer plan ("Tile tables built once per plan").  The bytes a tile's table build
writes into LDS for a group of 8 sorted rows depend on the sorted residues, the matrix and the group's row-shared flag only, so the
plan builds them once (k_rows_rowtab, behind the group's key entries) and a tile copies its groups' tables instead of building them.
HMK_NO_TILE_TABLES=1 keeps the build in every tile.  None of this may show: for every input the edge set (x, m, score) with the
tables, the edge set under HMK_NO_TILE_TABLES=1 and the C oracle's edge set of ALL pairs must be one set.  The cases are the smallest
that break one piece each: a last group with dead rows (which must contribute nothing, and must not hold merged entries although its
live rows agree at both key positions), a tile whose second group does not exist, sets in which every full group is row-shared and
sets in which none is, the one-group and the paired kernel, with and without the row-shared bodies, an interior tile, two plans and a
re-plan on one context, thresholds at which every tile has hits and one at which none has.  Context.last_plan_tables() tells which
prologue the plan's tiles run -- a case that passes has compared the two.  The GPU tests run with -m gpu on an MI355X; the check that
the oracle's edge sets are what the cases take them for needs none."""
import functools
import os

import numpy as np
import pytest

import hammock_amd
from hammock_amd.synth import synth_peptides
from test_key_sorted_step_modes import (INTERIOR_COLS, INTERIOR_N, K0, K1, X, blosum62, chunk_kinds, equal_key_set, planted_set, runs,
                                        sort_order, with_keys)

gpu = pytest.mark.gpu

SWITCHES = ("HMK_NO_KEY_SORT", "HMK_KEY_SORT_KEYS", "HMK_NO_ROW_SHARED", "HMK_KEY_ROW_PAIRS", "HMK_NO_ROW_RUN_SHARE", "HMK_NO_TILE_TABLES")
GROUP_TABLE_BYTES = 12 * 24 * 8   # 12 row positions x 24 residues x 8 rows
COLS = 4096                       # columns per tile of every plan here
# 8-bit lanes hold every 12-mer pair at thresholds 5 .. 80 under BLOSUM62 (128 - threshold + 12 x 11 <= 255, 128 - threshold - 12 x 4 >= 0);
# outside that range the set does not run the key-sorted kernels at all
DENSE, USUAL, SPARSE, NONE = 6, 14, 20, 80    # hits in every tile; fewer; few (the large set); no pair of any set here reaches it
PAIRED, PAIRED_PLAIN = {"HMK_KEY_ROW_PAIRS": "1"}, {"HMK_KEY_ROW_PAIRS": "1", "HMK_NO_ROW_SHARED": "1"}
SINGLE, SINGLE_PLAIN = {"HMK_KEY_ROW_PAIRS": "0"}, {"HMK_KEY_ROW_PAIRS": "0", "HMK_NO_ROW_SHARED": "1"}
FOUR = (PAIRED, PAIRED_PLAIN, SINGLE, SINGLE_PLAIN)


# ---- the inputs --------------------------------------------------------------------------------------------------------------

def distinct_key_set(n):
    """no two sequences agree at both key positions: no group of the sorted order is row-shared"""
    assert n <= 20 * 20
    return with_keys(900 + n, [(k // 20, k % 20) for k in range(n)])


@functools.lru_cache(maxsize=None)
def input_set(name):
    kind, n = name.split(":")
    n = int(n)
    if kind == "equal":
        return equal_key_set(n)
    if kind == "distinct":
        return distinct_key_set(n)
    if kind == "interior":
        return planted_set(n, INTERIOR_COLS)
    if kind == "mixed":   # runs of the key pair shorter and longer than a group: row-shared and ordinary groups side by side
        spec = [(1, 1, 21), (1, 2, 5), (2, 0, 11), (2, 1, 30), (3, 0, 7), (3, 1, 19), (4, 4, 40), (5, 0, 9), (5, 1, 2), (6, 6, 27)]
        assert sum(length for _, _, length in spec) == n
        return with_keys(300 + n, runs(spec))
    if kind == "random":
        return synth_peptides(40 + n, n, 12)
    raise ValueError(name)


# (set, switch sets, thresholds, shift penalty).  The partial last groups run the paired kernel, as do the one-group variants of the
# same sets; NONE rides on one set of every kind of flagging.
CASES = {
    "last_group_1_live_row": ("equal:9", (PAIRED,), (DENSE,), 0),          # 16-row tile of 9 rows: group 1 has one live row
    "no_second_group": ("equal:17", (PAIRED,), (DENSE,), 0),               # last tile of 1 row: its second group does not exist
    "last_group_5_live_rows": ("equal:13", FOUR, (DENSE,), 0),            # dead rows in the half that a merged entry changes
    "all_row_shared_16": ("equal:48", FOUR, (DENSE, NONE), 0),            # n a multiple of 16: every tile run-shared
    "all_row_shared_odd": ("equal:45", FOUR, (DENSE, USUAL), 0),          # n no multiple of 8
    "nothing_flagged": ("distinct:83", FOUR, (DENSE, NONE), 0),
    "interior_tile": ("interior:%d" % INTERIOR_N, ({},) + FOUR[:1] + FOUR[2:3], (SPARSE,), 0),
    "mixed_runs": ("mixed:171", FOUR, (DENSE, USUAL), 0),
}
REPLAN = (("random:700", USUAL, 0), ("random:700", DENSE, 2), ("equal:45", DENSE, 2), ("random:700", USUAL, 0))   # (set, threshold, shift penalty)


@functools.lru_cache(maxsize=None)
def oracle_scores(name, p):
    """the oracle's score of every pair i < j of the set, computed once per (set, shift penalty)"""
    from oracle import c_oracle
    res, off = input_set(name)
    n = len(off) - 1
    ii, jj = np.triu_indices(n, 1)
    ii, jj = ii.astype(np.uint32), jj.astype(np.uint32)
    st, sc = c_oracle.score_pairs(blosum62(), res, off, jj, ii, 0, X, p)
    assert st == 0
    for a in (ii, jj, sc):
        a.setflags(write=False)
    return ii, jj, sc


def oracle_edges(name, thr, p=0):
    ii, jj, sc = oracle_scores(name, p)
    hit = sc >= thr
    return np.sort(hammock_amd.pack_edges(ii[hit], jj[hit], sc[hit]))


def groups_of(n):
    return (n + 7) // 8


def tiles_of(n, rows):
    """tiles of the triangle plan: per chunk of `rows` sorted rows the columns after its first row, in runs of at most COLS"""
    return sum(-(-(n - r0 - 1) // COLS) for r0 in range(0, n, rows) if n - r0 - 1 > 0)


# ---- the cases are what the GPU tests take them for (no GPU) ------------------------------------------------------------------

def test_oracle_edge_sets_of_the_cases():
    """every case compares something: the oracle alone gives edges at every threshold but NONE, at DENSE in every tile's rows,
    and none at NONE"""
    for case, (name, _, thrs, p) in CASES.items():
        res, off = input_set(name)
        n = len(off) - 1
        order = sort_order(res, off)
        for thr in thrs:
            e = oracle_edges(name, thr, p)
            if thr == NONE:
                assert len(e) == 0, case
                continue
            assert len(e) > 0, case
            if thr == DENSE:   # a hit in every 16-row chunk of the sorted order that has a column after it
                x, m, _ = hammock_amd.edge_fields(e)
                pos = np.empty(n, dtype=np.int64)
                pos[order] = np.arange(n)
                chunks = set((np.minimum(pos[x], pos[m]) // 16).tolist())
                assert chunks >= {r0 // 16 for r0 in range(0, n, 16) if n - r0 - 1 > 0}, case
    for name, thr, p in REPLAN:
        assert len(oracle_edges(name, thr, p)) > 0


def test_flags_of_the_constructed_inputs():
    """the planner's rule restated (test_key_sorted_step_modes.chunk_kinds): full groups of the equal-key sets are row-shared, a
    group with a dead row never is, and the distinct-key set has no row-shared group"""
    for n in (9, 13, 17, 45, 48):
        kinds = chunk_kinds(*input_set("equal:%d" % n))
        full, last = divmod(n, 16)
        assert kinds[:full] == [(True, True, True)] * full
        if last:
            assert kinds[full:] == [(last >= 8, False, False)], n
    assert all(k == (False, False, False) for k in chunk_kinds(*input_set("distinct:83")))
    mixed = chunk_kinds(*input_set("mixed:171"))
    assert any(a or b for a, b, _ in mixed) and any(not a or not b for a, b, _ in mixed)
    res, off = input_set("distinct:83")
    key = res[off[:-1] + K0].astype(np.int64) * 24 + res[off[:-1] + K1]
    assert len(set(key.tolist())) == 83


# ---- GPU ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def M():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need an MI355X; no HIP device is visible")
    return blosum62()


def pass_under(ctx, env, thr, p=0):
    """sorted edges of one pass with the given switches (read by the library at every call), and the plan's table statistics"""
    keep = {k: os.environ.get(k) for k in SWITCHES}
    try:
        for k in keep:
            os.environ.pop(k, None)
        os.environ.update(env)
        e, _ = ctx.neighbors_shifted(X, p, thr)
        return np.sort(np.asarray(e, dtype=np.uint64)), ctx.last_plan_tables(), ctx.last_plan().n_tiles
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def one_set(ctx, name, env, thr, p=0):
    """with the tables, without them, the oracle: one edge set; the plan reports the prologue its tiles ran"""
    n = len(input_set(name)[1]) - 1
    want = oracle_edges(name, thr, p)
    got, tables, n_tiles = pass_under(ctx, env, thr, p)
    assert tables == (n_tiles, groups_of(n) * GROUP_TABLE_BYTES) and n_tiles > 0, (name, env, thr)
    if "HMK_KEY_ROW_PAIRS" in env:
        assert n_tiles == tiles_of(n, 16 if env["HMK_KEY_ROW_PAIRS"] == "1" else 8)
    assert np.array_equal(got, want), (name, env, thr, "with the plan's tables")
    got, tables, n_tiles_built = pass_under(ctx, dict(env, HMK_NO_TILE_TABLES="1"), thr, p)
    assert tables == (0, 0) and n_tiles_built == n_tiles, (name, env, thr)
    assert np.array_equal(got, want), (name, env, thr, "with the tables built in every tile")


@gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_same_edges_with_and_without_the_tables(M, case):
    name, envs, thrs, p = CASES[case]
    res, off = input_set(name)
    ctx = hammock_amd.Context(M, device=0)
    ctx.set_sequences(residues=res, offsets=off)
    for env in envs:
        for thr in thrs:
            one_set(ctx, name, env, thr, p)


@gpu
def test_two_plans_and_a_replan_on_one_context(M):
    """two thresholds and a non-zero shift penalty, then another set, then the first again: every plan's tables are its own (a table
    left from the former plan would hold the other set's cells), and the statistics are the current plan's"""
    ctx = hammock_amd.Context(M, device=0)
    current = None
    for name, thr, p in REPLAN:
        if name != current:
            res, off = input_set(name)
            ctx.set_sequences(residues=res, offsets=off)
            current = name
        for env in (PAIRED, SINGLE):
            one_set(ctx, name, env, thr, p)
    # a plan that is not key-sorted has no tables: nothing stays behind from the key-sorted one before it
    got, tables, _ = pass_under(ctx, {"HMK_NO_KEY_SORT": "1"}, USUAL)
    assert tables == (0, 0) and np.array_equal(got, oracle_edges(current, USUAL))
