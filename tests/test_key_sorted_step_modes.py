"""The step of the paired key-sorted 12-mer kernel ("One mode switch per step").  On a 16-row tile the window mode
-- both keys shared, key 0 only, none -- is tested ONCE per step and both row groups run inside that branch: on a run-shared tile
the lead and its follower lie in one straight line, their row masks are literals (both groups have 8 live rows), and on an
interior tile the column words are loaded without bounds.  In-loop shapes keep the hit word's halves swapped (rows 0-3 in the
bits 8r + 3, rows 4-7 in 8r + 7).  None of this may show: for every input the edge set (x, m, score) must be the same under no
switch, under HMK_KEY_ROW_PAIRS=1, under HMK_KEY_ROW_PAIRS=1 with HMK_NO_ROW_RUN_SHARE=1, under HMK_KEY_ROW_PAIRS=0 and under
HMK_NO_KEY_SORT=1, and sampled rows must match the oracle.  The cases are the smallest that break one piece each: all three window
modes inside one flagged and one unflagged tile, two hits of one lane in both groups of one step, a stage that fills (and is
flushed) between a lead and its follower under every mode, last chunks of 1, 8, 9 and 15 rows, diagonal and ragged tiles, one
interior tile, and columns hit by all eight rows of both groups.  With at most 4,097 sequences every row chunk has ONE column tile,
which reaches the diagonal: the interior case takes the smallest n that gives an off-diagonal tile of whole 256-column batches,
4,353.  The GPU tests run with -m gpu on an MI355X; the checks of the constructed inputs need none."""
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
COLS = 4096     # columns per tile of every plan here
STAGE, WAVE = 640, 64   # records a wave stages; it is flushed before a turn once more than STAGE - WAVE are staged
SWITCHES = ("HMK_NO_KEY_SORT", "HMK_KEY_SORT_KEYS", "HMK_NO_ROW_SHARED", "HMK_KEY_ROW_PAIRS", "HMK_NO_ROW_RUN_SHARE")
FIVE = ({}, {"HMK_KEY_ROW_PAIRS": "1"}, {"HMK_KEY_ROW_PAIRS": "1", "HMK_NO_ROW_RUN_SHARE": "1"}, {"HMK_KEY_ROW_PAIRS": "0"},
        {"HMK_NO_KEY_SORT": "1"})


@pytest.fixture(scope="module")
def M():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need an MI355X; no HIP device is visible")
    return blosum62()


def blosum62():
    with open(os.path.join(GOLDEN, "matrices.json")) as fh:
        return np.asarray(json.load(fh)["matrices"]["blosum62"], dtype=np.int32)


def edges_under(ctx, env, thr):
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
    """every edge of the given rows (an int: that many sampled ones), against the oracle's scores of those rows"""
    from oracle import c_oracle
    n = len(off) - 1
    x, m, s = hammock_amd.edge_fields(edges)
    if isinstance(rows, int):
        rows = np.random.default_rng(11).choice(n, min(rows, n), replace=False)
    for r in rows:
        others = np.delete(np.arange(n, dtype=np.uint32), r)
        st, sc = c_oracle.score_pairs(M, res, off, others, np.full(len(others), r, dtype=np.uint32), 0, X, P)
        assert st == 0
        hit = sc >= thr
        want = sorted(zip(np.minimum(others[hit], r).tolist(), np.maximum(others[hit], r).tolist(), sc[hit].tolist()))
        sel = (x == r) | (m == r)
        got = sorted(zip(x[sel].tolist(), m[sel].tolist(), s[sel].tolist()))
        assert got == want, f"row {r}"


def same_edges(M, res, off, thr=THR, rows=24):
    """the five passes give one edge set, and the given rows match the oracle"""
    ctx = hammock_amd.Context(M, device=0)
    ctx.set_sequences(residues=res, offsets=off)
    got = edges_under(ctx, FIVE[1], thr)
    for env in (FIVE[0],) + FIVE[2:]:
        assert np.array_equal(got, edges_under(ctx, env, thr)), env
    check_rows(M, res, off, got, thr, rows)
    return got


# ---- the rule, restated ------------------------------------------------------------------------------------------------------

def sort_order(res, off):
    """the planner's stable sort by the two key residues: caller index of every sorted position"""
    k0, k1 = res[off[:-1] + K0].astype(np.int64), res[off[:-1] + K1].astype(np.int64)
    return np.argsort(k0 * 24 + k1, kind="stable")


def sorted_keys(res, off):
    order = sort_order(res, off)
    return res[off[:-1] + K0].astype(np.int64)[order], res[off[:-1] + K1].astype(np.int64)[order]


def chunk_kinds(res, off):
    """per 16-row chunk of the sorted order: (group 0 row-shared, group 1 row-shared, flagged run-shared).  A group with a row past
    the end is not row-shared; a tile is flagged when both groups are and their first rows agree at BOTH key positions"""
    n = len(off) - 1
    k0, k1 = sorted_keys(res, off)
    key = k0 * 24 + k1
    out = []
    for r0 in range(0, n, 16):
        sh = [r0 + 8 * g + 8 <= n and bool((key[r0 + 8 * g:r0 + 8 * g + 8] == key[r0 + 8 * g]).all()) for g in (0, 1)]
        out.append((sh[0], sh[1], sh[0] and sh[1] and key[r0] == key[r0 + 8]))
    return out


def run_ids(res, off):
    """run of key 0 / of the key pair that every sorted position lies in"""
    k0, k1 = sorted_keys(res, off)
    run0 = np.concatenate(([0], np.cumsum(k0[1:] != k0[:-1])))
    run01 = np.concatenate(([0], np.cumsum((k0[1:] != k0[:-1]) | (k1[1:] != k1[:-1]))))
    return run0, run01


def window_mode(runs, n, w0):
    """3: both keys shared, 1: key 0 only, 0: none -- the window's first and last live column lie in one run of the pair / of key 0"""
    run0, run01 = runs
    w1 = min(w0 + 63, n - 1)
    return 3 if run01[w0] == run01[w1] else 1 if run0[w0] == run0[w1] else 0


def tile_runs(n, r0):
    """(first column, columns) of the column tiles of the chunk at r0 in the triangle: the columns after r0, in equal runs of whole
    256-column batches of at most COLS, the rest in the last"""
    lo, hi = r0 + 1, n
    if lo >= hi:
        return []
    k = -(-(hi - lo) // COLS)
    run = min(COLS, (-(-(hi - lo) // k) + 255) // 256 * 256)
    return [(c0, min(run, hi - c0)) for c0 in range(lo, hi, run)]


def chunk_scores(M, res, off, order, r0, cols):
    """oracle scores of the sorted rows r0 .. r0 + 15 against the sorted columns `cols`: [16, len(cols)]"""
    from oracle import c_oracle
    out = np.zeros((16, len(cols)), dtype=np.int64)
    for r in range(16):
        st, sc = c_oracle.score_pairs(M, res, off, order[cols].astype(np.uint32), np.full(len(cols), order[r0 + r], dtype=np.uint32), 0, X, P)
        assert st == 0
        out[r] = sc
    return out


# ---- the inputs --------------------------------------------------------------------------------------------------------------

def with_keys(seed, keys):
    """random 12-mers whose sorted order has the given (residue at 5, residue at 6) list; the caller's order has nothing of it"""
    n = len(keys)
    res, off = synth_peptides(seed, n, 12)
    res = res.copy()
    place = np.random.default_rng(seed + 1).permutation(n)
    for k in range(n):
        res[off[place[k]] + K0], res[off[place[k]] + K1] = keys[k]
    return res, off


def runs(spec):
    return [(a, b) for a, b, length in spec for _ in range(length)]


def modes_set():
    # runs of 100: a key-1 boundary at 100 and a key-0 boundary at 200, both inside the first 256 columns after chunk 0 (flagged: 16
    # rows of the pair (1, 1)) and after chunk 6 (rows 96 .. 111: four of (1, 1), twelve of (1, 2): group 1 row-shared, not flagged)
    return with_keys(61, runs([(1, 1, 100), (1, 2, 100), (2, 0, 100), (3, 0, 333)]))


def family(seed, keys, bases, mutations):
    """12-mers in sorted order, each one of a few base peptides with some residues redrawn and the given key pair: hits are dense"""
    n = len(keys)
    rng = np.random.default_rng(seed)
    base_res, _ = synth_peptides(seed, bases, 12)
    base_res = base_res.reshape(bases, 12)
    rows = base_res[rng.integers(0, bases, n)].copy()
    for _ in range(mutations):
        rows[np.arange(n), rng.integers(0, 12, n)] = rng.integers(0, 20, n)
    rows[:, K0], rows[:, K1] = np.asarray(keys).T
    off = (np.arange(n + 1, dtype=np.uint32) * 12).astype(np.uint32)
    return np.ascontiguousarray(rows.reshape(-1).astype(np.uint8)), off


FLUSH_THR = 14


def flush_set():
    # runs of 304 = 19 chunks: every tile is flagged, and every tile before a boundary has one window that crosses it -- key-1
    # boundaries at 304, 912 and 1,520 (mode 1), key-0 boundaries at 608 and 1,216 (mode 0)
    return family(5, runs([(9, 4, 304), (9, 5, 304), (10, 0, 304), (10, 1, 304), (11, 0, 304), (11, 1, 304)]), 3, 2)


def equal_key_set(n, seed=0):
    return with_keys(70 + n + seed, [(17, 3)] * n)


def planted_set(n, columns):
    """one key pair for all (sorted order = the caller's, every full tile flagged).  Rows 0-7 are one peptide A and rows 8-15 a
    peptide B that differs from A in its last two residues, each row with ONE residue of its own redrawn outside the key positions:
    a column that equals A (or B) is hit by all sixteen rows -- eight turns of its lane in BOTH groups of one step -- with scores
    that tell the rows apart.  Such columns are planted at `columns`: A at the even places of the list, B at the odd ones"""
    res, off = equal_key_set(n, seed=1)
    res = res.reshape(n, 12).copy()
    rng = np.random.default_rng(n)
    a = res[0].copy()
    b = a.copy()
    b[10:] = (b[10:] + 7) % 20
    free = [0, 1, 2, 3, 4, 7, 8, 9]
    for r in range(16):
        res[r] = a if r < 8 else b
        res[r, free[r % 8]] = (res[r, free[r % 8]] + 1 + rng.integers(0, 18)) % 20
    for k, col in enumerate(columns):
        res[col] = b if k & 1 else a
    return np.ascontiguousarray(res.reshape(-1)), off


PLANTED_COLS = [40, 90]            # both in step 0 of tile 0 (columns 1 .. 256)
INTERIOR_N = 4353                  # chunk 0: columns 1 .. 2,304 (diagonal) and 2,305 .. 4,352 (2,048 columns: interior)
INTERIOR_COLS = [40, 90, 2400, 3000, 4300, 4340]
LAST_CHUNKS = [49, 40, 41, 47]     # n = 1, 8, 9, 15 (mod 16)


# ---- the constructed inputs are what the GPU cases take them for (no GPU) ----------------------------------------------------

def test_window_modes_of_the_constructed_input():
    res, off = modes_set()
    n = len(off) - 1
    kinds, rid = chunk_kinds(res, off), run_ids(res, off)
    assert kinds[0] == (True, True, True) and kinds[6] == (False, True, False)
    for c in (0, 6):
        # the four waves' windows of the tile's first step, and each wave's next one: every mode, and a change of mode between the steps
        first = [window_mode(rid, n, 16 * c + 1 + 64 * w) for w in range(4)]
        second = [window_mode(rid, n, 16 * c + 1 + 256 + 64 * w) for w in range(4)]
        assert set(first) == {0, 1, 3}, (c, first)
        assert any(a != b for a, b in zip(first, second)), (c, first, second)


def test_two_hits_in_one_lane_of_both_groups():
    M = blosum62()
    res, off = planted_set(600, PLANTED_COLS)
    assert chunk_kinds(res, off)[0] == (True, True, True) and np.array_equal(sort_order(res, off), np.arange(600))
    cols = np.arange(1, 257)   # step 0 of tile 0
    hit = (chunk_scores(M, res, off, np.arange(600), 0, cols) >= THR) & (cols[None, :] > np.arange(16)[:, None])
    per_lane = np.stack([hit[:8].sum(0), hit[8:].sum(0)])
    for col in PLANTED_COLS:   # all eight rows of BOTH groups: eight turns of one lane behind the lead and behind the follower
        assert per_lane[0, col - 1] == 8 and per_lane[1, col - 1] == 8
    # ... with scores that tell the rows apart, in rows 0-3 and in rows 4-7
    sc = chunk_scores(M, res, off, np.arange(600), 0, np.asarray(PLANTED_COLS))
    for k in range(len(PLANTED_COLS)):
        for g in (0, 1):
            eight = sc[8 * g:8 * g + 8, k]
            assert len(set(eight[:4].tolist())) >= 2 and len(set(eight[4:].tolist())) >= 2 and len(set(eight.tolist())) >= 4, eight


def test_the_interior_tile_of_the_constructed_input():
    assert tile_runs(INTERIOR_N, 0) == [(1, 2304), (2305, 2048)]   # the second: off the diagonal, whole batches
    interior = [(r0, c0, nc) for r0 in range(0, INTERIOR_N, 16) for c0, nc in tile_runs(INTERIOR_N, r0) if c0 >= r0 + 16 and nc % 256 == 0]
    assert interior == [(0, 2305, 2048)]
    assert all(len(tile_runs(n, r0)) <= 1 for n in LAST_CHUNKS + [600, 733, 1824, 4097] for r0 in range(0, n, 16))
    res, off = planted_set(INTERIOR_N, INTERIOR_COLS)
    kinds = chunk_kinds(res, off)
    assert all(k == (True, True, True) for k in kinds[:-1]) and kinds[-1] == (False, False, False)
    # all eight rows of each group hit a planted column of the interior tile
    sc = chunk_scores(blosum62(), res, off, np.arange(INTERIOR_N), 0, np.asarray(INTERIOR_COLS))
    assert (sc[:, 2:] >= THR).all() and INTERIOR_COLS[2] >= 2305


def test_last_chunks_of_the_constructed_inputs():
    for n in LAST_CHUNKS:
        kinds = chunk_kinds(*equal_key_set(n))
        full, last = divmod(n, 16)
        assert kinds[:full] == [(True, True, True)] * full and kinds[full:] == [(last >= 8, False, False)], n
    assert [n % 16 for n in LAST_CHUNKS] == [1, 8, 9, 15]


def test_stage_fills_between_lead_and_follower_in_every_mode():
    """the wave's stage, restated: before every turn of an append loop the stage is flushed once more than STAGE - WAVE records are
    staged.  Simulated with the oracle's scores for every wave of every tile until each window mode has seen a flush inside the
    LEAD's append loop (group 0) -- between a lead and its follower"""
    M = blosum62()
    res, off = flush_set()
    n = len(off) - 1
    order, kinds, rid = sort_order(res, off), chunk_kinds(res, off), run_ids(res, off)
    assert all(k == (True, True, True) for k in kinds)
    seen = {0: 0, 1: 0, 3: 0}
    for c in range(len(kinds)):
        r0, col0 = 16 * c, 16 * c + 1
        cols = np.arange(col0, n)
        if len(cols) == 0 or all(seen.values()):
            break
        hit = (chunk_scores(M, res, off, order, r0, cols) >= FLUSH_THR) & (cols[None, :] > (r0 + np.arange(16))[:, None])
        for w in range(4):
            cnt = 0
            for s in range(-(-len(cols) // 256)):
                lo = 256 * s + 64 * w
                if lo >= len(cols):
                    break
                mode = window_mode(rid, n, col0 + lo)
                for g in (0, 1):
                    per_lane = hit[8 * g:8 * g + 8, lo:lo + 64].sum(0)
                    for turn in range(int(per_lane.max(initial=0))):
                        if cnt > STAGE - WAVE:
                            seen[mode] += g == 0
                            cnt = 0
                        cnt += int((per_lane > turn).sum())
    assert all(v > 0 for v in seen.values()), seen


# ---- GPU ---------------------------------------------------------------------------------------------------------------------

@gpu
def test_all_window_modes_in_one_tile(M):
    res, off = modes_set()
    for thr in (THR, 12):   # 12: hits in most steps, scores are cut out of planes that every mode's bodies produced
        assert len(same_edges(M, res, off, thr=thr, rows=16)) > 0


@gpu
def test_two_turns_in_both_groups_and_all_eight_rows(M):
    res, off = planted_set(600, PLANTED_COLS)
    # every record's row: all edges of rows 0 .. 15 and of the planted columns
    got = same_edges(M, res, off, rows=list(range(16)) + PLANTED_COLS)
    x, m, _ = hammock_amd.edge_fields(got)
    for col in PLANTED_COLS:
        assert set(x[m == col].tolist()) >= set(range(16))


@gpu
def test_stage_flushed_between_lead_and_follower_in_every_mode(M):
    res, off = flush_set()
    assert len(same_edges(M, res, off, thr=FLUSH_THR, rows=6)) > 0


@gpu
@pytest.mark.parametrize("n", LAST_CHUNKS)
def test_partial_last_chunk(M, n):
    res, off = equal_key_set(n)
    for thr in (THR, 12):
        assert len(same_edges(M, res, off, thr=thr, rows=n)) > 0


@gpu
def test_diagonal_tiles_and_a_ragged_end(M):
    # every tile reaches the diagonal, and 732 columns after row 0 are no multiple of 256: dead lanes in every tile's last batch
    res, off = with_keys(83, runs([(2, 2, 400), (2, 3, 333)]))
    for thr in (THR, 12):
        assert len(same_edges(M, res, off, thr=thr, rows=16)) > 0


@gpu
def test_interior_tile(M):
    res, off = planted_set(INTERIOR_N, INTERIOR_COLS)
    got = same_edges(M, res, off, rows=list(range(16)) + INTERIOR_COLS[2:])
    x, m, _ = hammock_amd.edge_fields(got)
    for col in INTERIOR_COLS:
        assert set(x[m == col].tolist()) >= set(range(16))
