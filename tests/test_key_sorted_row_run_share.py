"""Run-shared tiles of the key-sorted 12-mer pass.  On a 16-row tile whose two groups are both row-shared with the
SAME two key residues, group 0 runs the lead form of the row-shared body and leaves one dword per shift plane -- the sum of the
plane's merged halves -- in registers; group 1, the follower, takes it as one operand per plane and issues no merged read.  None of
this may show: the edge set (x, m, score) must be exactly the one with the hand-over switched off (HMK_NO_ROW_RUN_SHARE=1), the one
of 8-row tiles (HMK_KEY_ROW_PAIRS=0) and the one of the caller's order (HMK_NO_KEY_SORT=1), and sampled rows must match the oracle.
Context.last_plan_shared() must report the flagged tiles that the rule, restated here, gives for the input.  The cases are the
smallest that break one piece each: a second group that is absent, partial or full, the triangle's mask in the follower, two
row-shared groups with different key pairs, tiles with one row-shared group, every window mode under a follower, a stage that fills
(and is flushed) between the lead and its follower, and the largest and smallest cells in the handed-over dwords.
The GPU tests run with -m gpu on an MI355X; the checks of the constructed inputs need none."""
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
COLS = 4096     # columns per tile of every plan here (n <= 4,097: one column tile per row chunk)
SWITCHES = ("HMK_NO_KEY_SORT", "HMK_KEY_SORT_KEYS", "HMK_NO_ROW_SHARED", "HMK_KEY_ROW_PAIRS", "HMK_NO_ROW_RUN_SHARE")


@pytest.fixture(scope="module")
def M():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need an MI355X; no HIP device is visible")
    return blosum62()


def blosum62():
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


# ---- the rule, restated ------------------------------------------------------------------------------------------------------

def sorted_keys(res, off):
    """(residue at 5, residue at 6) of every sorted position: the planner's stable sort by the two key residues"""
    k0, k1 = res[off[:-1] + K0].astype(np.int64), res[off[:-1] + K1].astype(np.int64)
    order = np.argsort(k0 * 24 + k1, kind="stable")
    return k0[order], k1[order]


def chunk_kinds(res, off):
    """per 16-row chunk of the sorted order: (group 0 row-shared, group 1 row-shared, flagged run-shared).  A group with a row past
    the end is not row-shared; a tile is flagged when both groups are and their first rows agree at BOTH key positions"""
    n = len(off) - 1
    k0, k1 = sorted_keys(res, off)
    key = k0 * 24 + k1
    out = []
    for r0 in range(0, n, 16):
        sh = [r0 + 8 * g + 8 <= n and bool((key[r0 + 8 * g:r0 + 8 * g + 8] == key[r0 + 8 * g]).all()) for g in (0, 1)]
        out.append((sh[0], sh[1], sh[0] and sh[1] and k0[r0] == k0[r0 + 8] and k1[r0] == k1[r0 + 8]))
    return out


def tiles_of(n, rows, cols):
    """tiles of the triangle of n rows: per row chunk its columns after the chunk's first row, cut into runs of at most `cols`"""
    return sum(-(-(n - r0 - 1) // cols) for r0 in range(0, n - 1, rows))


def flagged_tiles(res, off):
    """tiles the planner flags: the column tiles of every flagged chunk (a chunk of 16 live rows always has columns after its first row)"""
    n = len(off) - 1
    return sum(-(-(n - 16 * c - 1) // COLS) for c, kind in enumerate(chunk_kinds(res, off)) if kind[2])


def window_modes(res, off):
    """the modes (3: both keys shared, 1: key 0 only, 0: none) of the 64-column windows that a wave scores on FLAGGED tiles: the
    window's first and last live column lie in one run of the key pair / of key 0 / in neither.  Tile of chunk c: columns
    16 c + 1 .. n - 1 (the triangle), 256 per step, 64 per wave"""
    n = len(off) - 1
    k0, k1 = sorted_keys(res, off)
    run0 = np.concatenate(([0], np.cumsum(k0[1:] != k0[:-1])))
    run01 = np.concatenate(([0], np.cumsum((k0[1:] != k0[:-1]) | (k1[1:] != k1[:-1]))))
    modes = {0: 0, 1: 0, 3: 0}
    for c, kind in enumerate(chunk_kinds(res, off)):
        if not kind[2]:
            continue
        for w0 in range(16 * c + 1, n, 64):
            w1 = min(w0 + 63, n - 1)
            modes[3 if run01[w0] == run01[w1] else 1 if run0[w0] == run0[w1] else 0] += 1
    return modes


# ---- the inputs --------------------------------------------------------------------------------------------------------------

def with_keys(seed, keys, shuffle=True):
    """random 12-mers whose sorted order has the given (residue at 5, residue at 6) list; the caller's order has nothing of it"""
    n = len(keys)
    res, off = synth_peptides(seed, n, 12)
    res = res.copy()
    place = np.random.default_rng(seed + 1).permutation(n) if shuffle else np.arange(n)
    for k in range(n):
        res[off[place[k]] + K0], res[off[place[k]] + K1] = keys[k]
    return res, off


def runs(spec):
    return [(a, b) for a, b, length in spec for _ in range(length)]


def equal_key_set(n):
    return with_keys(50 + n, [(17, 3)] * n)


def different_pairs_set():
    # runs of exactly 8 on group boundaries: tile 0 holds (1, 2) | (1, 3) -- the same residue at 5, another at 6 --, tile 1 (2, 5) | (3, 5)
    # -- another at 5, the same at 6 --, tile 2 (4, 4) | (4, 4), tile 3 (5, 0) | (5, 1) again; the rest is one long run (flagged tiles)
    return with_keys(7, runs([(1, 2, 8), (1, 3, 8), (2, 5, 8), (3, 5, 8), (4, 4, 16), (5, 0, 8), (5, 1, 8), (6, 6, 200)]))


def mixed_flags_set():
    # group boundaries on and off run boundaries: (shared, not), (not, shared), (not, not) and flagged tiles, under windows of all kinds
    return with_keys(23, runs([(0, 0, 1), (0, 1, 7), (0, 2, 8), (0, 3, 9), (1, 0, 15), (1, 1, 16), (1, 2, 17), (2, 0, 63), (3, 0, 64), (4, 0, 65),
                               (5, 0, 250), (5, 1, 700), (5, 2, 65), (6, 3, 700), (7, 0, 250), (7, 1, 64), (7, 2, 63), (8, 0, 1), (8, 1, 1), (8, 2, 1),
                               (9, 0, 17), (9, 1, 16), (9, 2, 15), (9, 3, 9), (9, 4, 8), (9, 5, 7), (9, 6, 1), (10, 0, 1), (11, 0, 1), (12, 7, 250),
                               (13, 0, 8), (13, 1, 8), (14, 0, 64), (15, 0, 9), (16, 1, 200), (17, 0, 27)]))


def key0_runs_set():
    # two long runs of the residue at 5, cut into column runs of 63 / 64 / 65 of the residue at 6: most 64-column windows cross a
    # boundary of the pair's runs inside a run of key 0
    return with_keys(31, runs([(3, b, (63, 64, 65)[b % 3]) for b in range(9)] + [(8, b, (65, 63, 64)[b % 3]) for b in range(6)]))


def no_runs_set():
    # one flagged tile (16 rows of the pair (0, 0)) whose columns have no runs: after the 16 rows every pair of residues once, so a
    # window of 64 columns spans more than three values of the residue at 5
    return with_keys(41, [(0, 0)] * 16 + [(a, b) for a in range(20) for b in range(20) if (a, b) != (0, 0)])


def family_set(seed, n, bases, mutations):
    """n 12-mers, each one of a few base peptides with some residues redrawn and ONE key pair for all: every tile is flagged and
    hits are dense at any threshold"""
    rng = np.random.default_rng(seed)
    base_res, _ = synth_peptides(seed, bases, 12)
    base_res = base_res.reshape(bases, 12)
    rows = base_res[rng.integers(0, bases, n)].copy()
    for _ in range(mutations):
        rows[np.arange(n), rng.integers(0, 12, n)] = rng.integers(0, 20, n)
    rows[:, K0], rows[:, K1] = 9, 4
    off = (np.arange(n + 1, dtype=np.uint32) * 12).astype(np.uint32)
    return np.ascontiguousarray(rows.reshape(-1).astype(np.uint8)), off


def extreme_cells_set():
    # rows with (W, W) and rows with (D, D) at the key positions, 352 each (22 flagged tiles per pair), W-rich columns: the handed-over
    # dword of a plane holds cell(W, W) twice -- the matrix's largest, 11 -- or cell(D, W) twice -- its smallest, -4
    rng = np.random.default_rng(9)
    rich = "WDWCWNW"
    bases = ["".join(rng.choice(list(rich), 12)) for _ in range(6)] + ["W" * 12]
    seqs = []
    for k in range(704):
        s = list(bases[k % len(bases)])
        for _ in range(k % 3):
            s[rng.integers(0, 12)] = rich[rng.integers(0, len(rich))]
        s[K0] = s[K1] = "W" if k < 352 else "D"
        seqs.append("".join(s))
    return hammock_amd.pack_sequences(seqs)


ENDS = [9, 15, 16, 17, 24, 25, 31, 32, 33, 257]


# ---- the constructed inputs are what the GPU cases take them for (no GPU) ----------------------------------------------------

def test_tile_ends_of_the_constructed_inputs():
    for n in ENDS:
        res, off = equal_key_set(n)
        kinds = chunk_kinds(res, off)
        full, last = divmod(n, 16)
        assert kinds[:full] == [(True, True, True)] * full, n
        # the last tile's second group is absent (1-8 live rows) or partial (9-15): never flagged
        if last:
            assert kinds[full:] == [(last >= 8, False, False)], n
        assert flagged_tiles(res, off) == full
        assert window_modes(res, off)[1] == window_modes(res, off)[0] == 0


def test_tile_kinds_of_the_constructed_inputs():
    kinds = chunk_kinds(*different_pairs_set())
    # both groups row-shared and NOT flagged: position 6 differs, position 5 differs; then a flagged tile; then position 6 again
    assert kinds[:4] == [(True, True, False), (True, True, False), (True, True, True), (True, True, False)]
    k0, k1 = sorted_keys(*different_pairs_set())
    assert (k0[0], k1[0], k0[8], k1[8]) == (1, 2, 1, 3) and (k0[16], k1[16], k0[24], k1[24]) == (2, 5, 3, 5)
    assert all(kind == (True, True, True) for kind in kinds[4:-1]) and flagged_tiles(*different_pairs_set()) == 13

    kinds = chunk_kinds(*mixed_flags_set())
    assert len(kinds) == 188
    for want in ((True, False, False), (False, True, False), (False, False, False), (True, True, True), (True, True, False)):
        assert want in kinds, want
    assert flagged_tiles(*mixed_flags_set()) == sum(k[2] for k in kinds) > 150


def test_window_modes_of_the_constructed_inputs():
    # every mode occurs under a flagged tile -- each in the input built for it
    m = window_modes(*equal_key_set(700))
    assert m[3] > 0 and m[1] == 0 and m[0] == 0
    m = window_modes(*key0_runs_set())
    assert m[1] > 100 and m[3] > 0
    m = window_modes(*no_runs_set())
    assert m[0] == 7 and m[1] == 0 and m[3] == 0 and flagged_tiles(*no_runs_set()) == 1
    m = window_modes(*mixed_flags_set())
    assert all(v > 0 for v in m.values()), m


def test_extreme_cells_of_the_constructed_input():
    M = blosum62()
    res, off = extreme_cells_set()
    w, d = int(res[off[0] + K0]), int(res[off[352] + K0])
    assert M[w, w] == M.max() == 11 and M[d, w] == M[w, d] == M.min() == -4
    kinds = chunk_kinds(res, off)
    assert kinds == [(True, True, True)] * 44
    k0, k1 = sorted_keys(res, off)
    assert {(int(a), int(b)) for a, b in zip(k0, k1)} == {(w, w), (d, d)}
    assert np.mean(res == w) > 0.4   # W-rich columns: most merged cells are the extremes


# ---- GPU ---------------------------------------------------------------------------------------------------------------------

def same_edges(M, res, off, thr=THR, oracle_rows=24):
    """the four passes give one edge set; last_plan_shared() reports the rule's count, and none where the hand-over cannot be"""
    ctx = hammock_amd.Context(M, device=0)
    ctx.set_sequences(residues=res, offsets=off)
    n = len(off) - 1
    got = edges_under(ctx, {"HMK_KEY_ROW_PAIRS": "1"}, thr)
    plan = ctx.last_plan()
    assert ctx.last_plan_shared() == (tiles_of(n, 16, COLS), flagged_tiles(res, off))
    assert plan.n_tiles == tiles_of(n, 16, COLS) and plan.pairs_scored == n * (n - 1) // 2
    assert np.array_equal(got, edges_under(ctx, {"HMK_KEY_ROW_PAIRS": "1", "HMK_NO_ROW_RUN_SHARE": "1"}, thr))
    assert ctx.last_plan_shared() == (tiles_of(n, 16, COLS), 0)
    assert np.array_equal(got, edges_under(ctx, {"HMK_KEY_ROW_PAIRS": "0"}, thr))
    assert ctx.last_plan_shared() == (0, 0) and ctx.last_plan().n_tiles == tiles_of(n, 8, COLS)
    assert np.array_equal(got, edges_under(ctx, {"HMK_NO_KEY_SORT": "1"}, thr))
    assert ctx.last_plan_shared() == (0, 0)
    if oracle_rows:
        check_rows(M, res, off, got, thr, oracle_rows)
    return got, plan


@gpu
@pytest.mark.parametrize("n", ENDS)
def test_tile_ends(M, n):
    # one key pair for all rows: every full tile is flagged, the last has 1 to 16 live rows -- its second group absent, partial (the
    # tile is not flagged: an ordinary body, and a row-shared first group that is no lead) or full.  Every tile is a diagonal one
    # up to n = 33: the follower's triangle mask counts from row0 + 8.  Threshold 12: hits in every tile (all rows, oracle)
    res, off = equal_key_set(n)
    for thr in (THR, 12):
        got, _ = same_edges(M, res, off, thr=thr, oracle_rows=min(n, 64))
    assert len(got) > 0


@gpu
def test_different_key_pairs_in_one_tile(M):
    # both groups row-shared, another pair in each: the follower would add the lead's cells of the wrong residue at one position
    res, off = different_pairs_set()
    for thr in (THR, 12):
        got, _ = same_edges(M, res, off, thr=thr, oracle_rows=64)
    assert len(got) > 0


@gpu
def test_mixed_flags_and_all_window_modes(M):
    res, off = mixed_flags_set()
    for thr in (THR, 12):   # 12: hits in most steps, scores are cut out of planes that the lead and the follower produced
        same_edges(M, res, off, thr=thr, oracle_rows=24 if thr == THR else 6)


@gpu
@pytest.mark.parametrize("name", ["both_keys", "key0_only", "no_runs"])
def test_window_modes_under_the_follower(M, name):
    res, off = {"both_keys": lambda: equal_key_set(700), "key0_only": key0_runs_set, "no_runs": no_runs_set}[name]()
    for thr in (THR, 12):
        got, _ = same_edges(M, res, off, thr=thr, oracle_rows=16)
    assert len(got) > 0


@gpu
def test_stage_flushed_between_lead_and_follower(M):
    # One group of a wave's step tests 64 columns x 8 rows = 512 pairs.  The threshold is the oracle's: the 70th percentile of the
    # scores of 20,000 random pairs, so about 30 % of the pairs hit -- more than a quarter (asserted on the result), over 128 records
    # per group and step.  A wave's stage holds 640 records and is flushed once more than 576 are staged: after at most five
    # group-steps, inside the lead's append loop as often as inside the follower's.  Every tile is flagged (one key pair), so the
    # handed-over dwords are live across the flush call in half of them, and group 1's scores come out of them after it
    from oracle import c_oracle
    n = 2000
    res, off = family_set(5, n, 3, 2)
    assert flagged_tiles(res, off) == n // 16
    rng = np.random.default_rng(3)
    a, b = rng.integers(0, n, 20000).astype(np.uint32), rng.integers(0, n, 20000).astype(np.uint32)
    st, sc = c_oracle.score_pairs(M, res, off, a[a != b], b[a != b], 0, X, P)
    assert st == 0
    thr = int(np.quantile(sc, 0.70))
    assert 5 <= thr <= 80 and np.mean(sc >= thr) > 0.27
    got, plan = same_edges(M, res, off, thr=thr, oracle_rows=6)
    assert len(got) * 4 > plan.pairs_scored


@gpu
def test_extreme_cells_in_the_handed_over_dwords(M):
    # classify() proves 8-bit lanes for thresholds 5 .. 80: at 80 the planes start at the bottom of the byte and a dword of two
    # cells at -4 is the smallest operand there is, at 5 a pair that scored 12 x 11 would end at 255 and the dword holds 2 x 11
    res, off = extreme_cells_set()
    for thr in (80, 5):
        got, plan = same_edges(M, res, off, thr=thr, oracle_rows=12)
        assert plan.classes_rows == 1 and plan.classes_u16 == 0 and plan.classes_direct == 0
        assert len(got) > 0
