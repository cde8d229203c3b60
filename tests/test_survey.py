"""The score survey of a pair space: hmk_score_survey_shifted (k_survey.hip) and `hammock-hip survey`.

CPU part (host-only context): the symbol, every argument check, DeviceError for a valid call, the mode's usage line and its argument and
file errors, and one test of the INPUTS with the C oracle alone: that they hold what the GPU tests claim to exercise.
GPU part: the histogram, the three row outputs and every statistics field bit-exact against an expectation built from the C oracle alone
-- score_pairs over the enumerated pairs (seq1 = the larger index in a triangle, seq1 = the query in a rectangle), np.bincount, the row
maxima with the smallest-index rule, the counts.  An input's scores are computed once per session and shared.
    mixed           1,300 distinct random 7-20-mers: five tiles per side and a ragged sixth
    twelve          1,300 12-mers: one length
    three_letters   600 distinct 12-mers over three letters: few distinct scores
    copies          70 copies of one string: one bin for every pair, every row's best tied 69 ways
    asymmetric      the first 600 of mixed under a perturbed matrix: rectangles only
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
from test_linkage import _blosum62, device_ctx

import hammock_amd
from hammock_amd import _native as N

INT32_MAX, INT32_MIN, UINT32_MAX = 2 ** 31 - 1, -2 ** 31, 2 ** 32 - 1
T = 256   # LINK_TILE
SIZES = [1, 2, T - 1, T, T + 1, 2 * T + 1]
MIXED_PARAMS = [(3, -1), (2, -1), (3, 0)]
GRID_LINE = re.compile(r"^\[hmk grid\] (\S+) (\d+) -> (\d+)$", re.M)
LETTERS = hammock_amd.AMINO_ACIDS
STAT_NAMES = ("pairs_scored", "n_below", "n_above", "n_at_or_above", "score_min", "score_max", "launches", "reserved")


# ---- inputs and the oracle's side --------------------------------------------------------------------------------------------

def _asymmetric_matrix():
    A = _blosum62().copy().reshape(24, 24)
    rng = np.random.default_rng(77)
    A[:20, :20] += rng.integers(-2, 3, size=(20, 20)).astype(A.dtype)
    assert not np.array_equal(A, A.T)
    return np.ascontiguousarray(A)


@functools.lru_cache(maxsize=None)
def input_set(name):
    """-> (M, res, off, strings)"""
    M = _blosum62()
    if name == "mixed":
        peps = random_peptides(np.random.default_rng(1), 1300, 7, 20)
    elif name == "twelve":
        peps = random_peptides(np.random.default_rng(2), 1300, 12, 12)
    elif name == "three_letters":
        peps = random_peptides(np.random.default_rng(3), 600, 12, 12, alphabet=3)
    elif name == "copies":
        peps = [np.random.default_rng(4).integers(0, 20, size=11).astype(np.uint8)] * 70
    else:
        assert name == "asymmetric"
        peps = random_peptides(np.random.default_rng(1), 1300, 7, 20)[:600]
        M = _asymmetric_matrix()
    res, off = hammock_amd.pack_sequences(peps)
    for arr in (res, off):
        arr.setflags(write=False)
    return M, res, off, ["".join(LETTERS[r] for r in q) for q in peps]


@functools.lru_cache(maxsize=None)
def triangle_scores(name, X, p):
    """int64 [n, n]: entry (a, b) and (b, a), a > b, = the oracle's score(seq1 = a, seq2 = b); the diagonal is never read"""
    from oracle import c_oracle
    M, res, off, _ = input_set(name)
    n = off.size - 1
    hi, lo = np.tril_indices(n, -1)
    st, sc = c_oracle.score_pairs(M, res, off, hi, lo, 0, X, p)
    assert st == 0
    S = np.zeros((n, n), dtype=np.int64)
    S[hi, lo] = sc
    S[lo, hi] = sc
    S.setflags(write=False)
    return S


@functools.lru_cache(maxsize=None)
def rectangle_scores(name, X, p, q0, q1, r0, r1):
    """int64 [q1 - q0, r1 - r0]: the oracle's score(seq1 = q, seq2 = r)"""
    from oracle import c_oracle
    M, res, off, _ = input_set(name)
    st, block = c_oracle.score_block(M, res, off, np.arange(q0, q1), np.arange(r0, r1), 0, X, p)
    assert st == 0
    block = block.astype(np.int64)
    block.setflags(write=False)
    return block


def reduce_scores(block, valid, partner0, pair_scores, thr, lo, n_bins, rows=True):
    """block [rows, partners] with valid marking the entries that are pairs, partner index = partner0 + column; pair_scores: every
    pair once -> (hist or None, (best_score, best_index, degree) or None, the statistics without launches)"""
    sc = np.asarray(pair_scores, dtype=np.int64)
    hist = None
    below = above = 0
    if n_bins:
        inside = (sc >= lo) & (sc < lo + n_bins)
        hist = np.bincount(sc[inside] - lo, minlength=n_bins).astype(np.uint64)
        below, above = int((sc < lo).sum()), int((sc >= lo + n_bins).sum())
    out = None
    if rows:
        masked = np.where(valid, block, INT32_MIN - 1)
        has = valid.any(axis=1) if block.shape[1] else np.zeros(block.shape[0], dtype=bool)
        first = masked.argmax(axis=1) if block.shape[1] else np.zeros(block.shape[0], dtype=np.int64)   # the first of equal maxima
        best_score = np.where(has, masked[np.arange(block.shape[0]), first] if block.shape[1] else 0, INT32_MIN)
        best_index = np.where(has, partner0 + first, UINT32_MAX)
        degree = (valid & (block >= thr)).sum(axis=1) if block.shape[1] else np.zeros(block.shape[0], dtype=np.int64)
        out = (best_score.astype(np.int64), best_index.astype(np.int64), degree.astype(np.int64))
    stats = {"pairs_scored": int(sc.size), "n_below": below, "n_above": above, "n_at_or_above": int((sc >= thr).sum()),
             "score_min": int(sc.min()) if sc.size else INT32_MAX, "score_max": int(sc.max()) if sc.size else INT32_MIN, "reserved": 0}
    return hist, out, stats


def expect_triangle(name, X, p, q0, q1, thr, lo, n_bins, rows=True):
    S = triangle_scores(name, X, p)[q0:q1, q0:q1]
    s = q1 - q0
    a, b = np.tril_indices(s, -1)
    return reduce_scores(S, ~np.eye(s, dtype=bool), q0, S[a, b], thr, lo, n_bins, rows)


def expect_rectangle(name, X, p, q0, q1, r0, r1, thr, lo, n_bins, rows=True):
    block = rectangle_scores(name, X, p, q0, q1, r0, r1)
    return reduce_scores(block, np.ones(block.shape, dtype=bool), r0, block.ravel(), thr, lo, n_bins, rows)


def wanted_grids(triangle, nq, nr, n_bins, rows):
    """kernel -> the grid its launcher asks for (k_survey.hip's launchers); an empty pair space launches nothing"""
    tq, tr = -(-nq // T), -(-nr // T)
    tiles = tq * (tq + 1) // 2 if triangle else tq * tr
    pairs = nq * (nq - 1) // 2 if triangle else nq * nr
    if pairs == 0:
        return {}
    grids = {"k_survey_init": min(-(-max(n_bins, nq if rows else 0, 3) // 256), 4096), "k_survey_tiled": min(tiles, 65536)}
    if rows:
        grids["k_survey_decode"] = min(-(-nq // 256), 4096)
    return grids


def check(got, want, launches):
    hist, out, stats = got
    whist, wout, wstats = want
    assert (hist is None) == (whist is None) and (out is None) == (wout is None)
    if whist is not None:
        assert hist.dtype == np.uint64 and np.array_equal(hist, whist), "hist"
        assert int(hist.sum()) + stats.n_below + stats.n_above == stats.pairs_scored
    if wout is not None:
        assert out[0].dtype == np.int32 and out[1].dtype == np.uint32 and out[2].dtype == np.uint32
        for g, w, name in zip(out, wout, ("best_score", "best_index", "degree")):
            assert np.array_equal(g.astype(np.int64), w), name
    for name in STAT_NAMES:
        assert getattr(stats, name) == (launches if name == "launches" else wstats[name]), name
    assert stats.kernel_ms > 0 or launches == 0


def survey(ctx, capfd, cap, triangle, q0, q1, r0, r1, X, p, thr, lo, n_bins, rows=True):
    """the call, with the [hmk grid] lines of the new kernels asserted against the launchers' arithmetic -> its result"""
    capfd.readouterr()
    got = ctx.score_survey_shifted(q0, q1, r0, r1, X, p, thr, score_lo=lo, n_bins=n_bins, rows=rows)
    grids = wanted_grids(triangle, q1 - q0, r1 - r0, n_bins, rows)
    lines = {}
    for kernel, wanted, launched in GRID_LINE.findall(capfd.readouterr().err):
        assert kernel not in lines
        lines[kernel] = (int(wanted), int(launched))
    assert {k: v for k, v in lines.items() if k.startswith("k_survey_")} == {k: (w, cap) for k, w in grids.items() if cap and w > cap}
    return got, len(grids)


# ---- CPU: the symbol, the checks ---------------------------------------------------------------------------------------------

def test_symbol_is_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "hammock_hip.h")) as fh:
        header = fh.read()
    assert "int hmk_score_survey_shifted(hmk_ctx *ctx" in header and "} hmk_survey_stats;" in header
    assert "#define HMK_SURVEY_MAX_BINS 1024" in header and N.HMK_SURVEY_MAX_BINS == 1024
    assert "hmk_score_survey_shifted" in N.SYMBOLS
    assert hasattr(N.lib, "hmk_score_survey_shifted")
    assert N.lib.hmk_abi_version() == 4
    assert C.sizeof(N.SurveyStats) == 56


def _raw_call(ctx, q0, q1, r0, r1, X=3, p=0, thr=20, lo=0, n_bins=8, null=(), stats=True):
    """the C entry point with chosen arguments null -> status"""
    nq = max(q1 - q0, 1)
    hist = np.zeros(max(n_bins, 1), np.uint64)
    out = {"best_score": (np.zeros(nq, np.int32), C.c_int32), "best_index": (np.zeros(nq, np.uint32), C.c_uint32),
           "degree": (np.zeros(nq, np.uint32), C.c_uint32)}
    ptr = [None if k in null else a.ctypes.data_as(C.POINTER(t)) for k, (a, t) in out.items()]
    s = N.SurveyStats()
    return N.lib.hmk_score_survey_shifted(ctx._h, q0, q1, r0, r1, X, p, thr, lo, n_bins,
                                          None if "hist" in null else hist.ctypes.data_as(C.POINTER(C.c_uint64)), *ptr,
                                          C.byref(s) if stats else None)


def test_host_only_context_answers_every_bad_argument(blosum62):
    rng = np.random.default_rng(5)
    peps = [rng.integers(0, 20, size=12).astype(np.uint8) for _ in range(10)]
    res, off = hammock_amd.pack_sequences(peps)
    ctx = hammock_amd.Context(blosum62, device=-1)
    ctx.set_sequences(residues=res, offsets=off)
    bad, rows = N.HMK_ERR_BAD_ARG, ("best_score", "best_index", "degree")
    # the ranges
    assert _raw_call(ctx, 4, 2, 4, 2) == bad                  # q0 > q1
    assert _raw_call(ctx, 0, 4, 6, 5) == bad                  # r0 > r1
    assert _raw_call(ctx, 0, 11, 0, 11) == bad                # beyond n
    assert _raw_call(ctx, 0, 4, 6, 11) == bad
    assert _raw_call(ctx, 0, 6, 3, 10) == bad                 # overlapping in part
    assert "overlap" in N.lib.hmk_last_error(ctx._h).decode()
    assert _raw_call(ctx, 0, 6, 0, 5) == bad                  # one inside the other
    assert _raw_call(ctx, 2, 6, 0, 6) == bad
    # the bins
    assert _raw_call(ctx, 0, 10, 0, 10, n_bins=N.HMK_SURVEY_MAX_BINS + 1) == bad
    assert _raw_call(ctx, 0, 10, 0, 10, n_bins=8, null=("hist",)) == bad
    assert _raw_call(ctx, 0, 10, 0, 10, n_bins=0) == bad      # a histogram without bins
    # the row outputs: all three or none
    for k in range(1, 7):
        null = tuple(name for bit, name in enumerate(rows) if k >> bit & 1)
        if len(null) < 3:
            assert _raw_call(ctx, 0, 10, 0, 10, null=null) == bad, null
            assert "together" in N.lib.hmk_last_error(ctx._h).decode()
    assert _raw_call(ctx, 0, 10, 0, 10, n_bins=0, null=rows + ("hist",)) == bad   # nothing wanted of a non-empty pair space
    assert _raw_call(ctx, 0, 4, 4, 10, n_bins=0, null=rows + ("hist",)) == bad
    assert _raw_call(ctx, 0, 10, 0, 10, stats=False) == bad
    with pytest.raises(ValueError):
        ctx.score_survey_shifted(0, 6, 3, 10, 3, 0, 20)
    with pytest.raises(ValueError):
        ctx.score_survey_shifted(0, 10, 0, 10, 3, 0, 20, n_bins=2000)
    # an asymmetric matrix: the triangle is refused, the rectangle is not
    A = blosum62.copy()
    A[0, 1] += 1
    actx = hammock_amd.Context(A, device=-1)
    actx.set_sequences(residues=res, offsets=off)
    with pytest.raises(ValueError, match="symmetric"):
        actx.score_survey_shifted(0, 10, 0, 10, 3, 0, 20)
    with pytest.raises(hammock_amd.DeviceError):
        actx.score_survey_shifted(0, 4, 4, 10, 3, 0, 20)
    # valid calls: no CPU fallback, in every form, for an empty pair space too
    assert _raw_call(ctx, 0, 10, 0, 10) == N.HMK_ERR_DEVICE
    assert _raw_call(ctx, 0, 10, 0, 10, n_bins=0, null=("hist",)) == N.HMK_ERR_DEVICE
    assert _raw_call(ctx, 0, 10, 0, 10, null=rows) == N.HMK_ERR_DEVICE
    assert _raw_call(ctx, 6, 10, 0, 6, thr=10 ** 6) == N.HMK_ERR_DEVICE
    for call in (lambda: ctx.score_survey_shifted(0, 10, 0, 10, 3, 0, 20, score_lo=-10, n_bins=100),
                 lambda: ctx.score_survey_shifted(0, 4, 4, 10, 3, 0, 20, rows=False, n_bins=1),
                 lambda: ctx.score_survey_shifted(3, 3, 0, 10, 3, 0, 20)):
        with pytest.raises(hammock_amd.DeviceError):
            call()


def test_cli_survey_argument_and_file_errors(tmp_path):
    fa = os.path.join(GOLDEN, "musi.fa")
    r = cli("survey", "-d", str(tmp_path / "a"))
    assert r.returncode == 2 and "-i or --input" in r.stderr
    assert not (tmp_path / "a").exists()
    r = cli("survey", "-i", fa, "--devices", "0,1", "-d", str(tmp_path / "b"))
    assert r.returncode == 2 and "--devices" in r.stderr
    r = cli("survey", "-i", fa, "-f", "xml", "-d", str(tmp_path / "c"))
    assert r.returncode == 2 and "Parameter -f" in r.stderr
    (tmp_path / "d").mkdir()
    r = cli("survey", "-i", fa, "-d", str(tmp_path / "d"))
    assert r.returncode == 2 and "Output directory exists" in r.stderr
    r = cli("survey", "-i", str(tmp_path / "missing.fa"), "-d", str(tmp_path / "e"))
    assert r.returncode != 0
    r = cli("survey", "-i", fa, "--database", str(tmp_path / "missing.fa"), "-d", str(tmp_path / "f"))
    assert r.returncode != 0
    r = cli("survey", "-i", fa, "-l", "no_such_label", "-d", str(tmp_path / "g"))
    assert r.returncode == 3 and "No sequences" in r.stderr
    usage = cli("--help").stderr
    assert "hammock-hip survey -i <sequences> -d <directory> [-g <int>] [--database <sequences>]" in usage and "(survey)" in usage


def test_the_inputs_hold_what_the_gpu_tests_claim():
    """the oracle's side alone (it passes before the call exists): no GPU test below can pass vacuously"""
    _, res, off, strings = input_set("mixed")
    n = 1300
    lens = np.diff(off.astype(np.int64))
    assert len(set(strings)) == n and lens.min() == 7 and lens.max() == 20 and n == 5 * T + 20
    hist, (best, index, degree), stats = expect_triangle("mixed", 3, -1, 0, n, 20, -32, 76)
    assert (stats["pairs_scored"], stats["score_min"], stats["score_max"], stats["n_at_or_above"]) == (844_350, -32, 43, 476)
    assert stats["n_below"] == stats["n_above"] == 0 and hist[0] and hist[-1]
    S = triangle_scores("mixed", 3, -1)
    masked = np.where(np.eye(n, dtype=bool), INT32_MIN, S)
    assert ((masked == best[:, None]).sum(axis=1) > 1).sum() == 204            # rows whose best is tied
    assert (degree == 0).sum() == 745 and degree.sum() == 2 * 476
    assert 0.07 < hist.max() / 844_350 < 0.08                                    # one bin holds 7 % of the pairs
    assert (index > np.arange(n)).any() and (index < np.arange(n)).any()       # best partners on both sides of the row
    for X, p in MIXED_PARAMS[1:]:
        assert not np.array_equal(triangle_scores("mixed", X, p), S)
    # the window that cuts both tails does, and 20 is a score that occurs
    _, _, cut = expect_triangle("mixed", 3, -1, 0, n, 20, -10, 30)
    assert cut["n_below"] > 0 and cut["n_above"] > 0 and hist[20 + 32] > 0
    lens12 = np.diff(input_set("twelve")[2].astype(np.int64))
    assert lens12.size == 1300 and (lens12 == 12).all()
    _, res3, off3, strings3 = input_set("three_letters")
    assert len(set(strings3)) == 600 and res3.max() == 2 and len(set(res3.tolist())) == 3
    t3 = triangle_scores("three_letters", 3, -1)
    assert np.unique(t3[np.tril_indices(600, -1)]).size < np.unique(S[np.tril_indices(n, -1)]).size
    assert len(set(input_set("copies")[3])) == 1
    one = int(triangle_scores("copies", 3, -1)[1, 0])
    hist, (best, index, degree), stats = expect_triangle("copies", 3, -1, 0, 70, 20, one, 1)
    assert hist[0] == 70 * 69 // 2 and stats["score_min"] == stats["score_max"] == one
    assert index[0] == 1 and (index[1:] == 0).all() and (best == one).all()
    A = input_set("asymmetric")[0]
    assert not np.array_equal(A, A.T)
    fwd, back = rectangle_scores("asymmetric", 3, -1, 0, 257, 257, 600), rectangle_scores("asymmetric", 3, -1, 257, 600, 0, 257)
    assert not np.array_equal(fwd, back.T)                                       # the orientation of a rectangle's pairs matters here


# ---- GPU ---------------------------------------------------------------------------------------------------------------------

FULL = [("mixed", X, p) for X, p in MIXED_PARAMS] + [("twelve", 3, -1), ("three_letters", 3, -1), ("copies", 3, -1)]


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [0, 1, 3])
@pytest.mark.parametrize("name,X,p", FULL)
def test_full_triangles_match_the_oracle(gpu, monkeypatch, capfd, name, X, p, cap):
    """every output and every statistics field at the exact window; under HMK_TEST_GRID_CAP the tile loop, the flush and the clearing
    of the LDS histogram go beyond their first iteration, and every new kernel says so"""
    M, res, off, _ = input_set(name)
    n = off.size - 1
    S = triangle_scores(name, X, p)
    sc = S[np.tril_indices(n, -1)]
    lo, bins = int(sc.min()), int(sc.max() - sc.min()) + 1
    ctx = device_ctx(M, res, off)
    if cap:
        monkeypatch.setenv("HMK_TEST_GRID_CAP", str(cap))
    got, launches = survey(ctx, capfd, cap, True, 0, n, 0, n, X, p, 20, lo, bins)
    check(got, expect_triangle(name, X, p, 0, n, 20, lo, bins), launches)
    assert launches == 3 and got[2].n_below == got[2].n_above == 0
    assert int(got[1][2].sum()) == 2 * got[2].n_at_or_above
    if name == "copies":
        assert got[0].tolist() == [70 * 69 // 2] and got[1][1][0] == 1 and not got[1][1][1:].any()


WINDOWS = [  # (threshold, score_lo, n_bins, rows) on mixed at (3, -1): scores -32 ... 43
    (20, -32, 76, True),        # the exact window; a threshold that occurs
    (20, -10, 30, True),        # both tails cut
    (20, 3, 1, True),           # one bin
    (20, -500, 1024, True),     # HMK_SURVEY_MAX_BINS
    (20, 44, 1024, False),      # ... all of them above every score
    (20, -2000, 1024, False),   # ... all of them below
    (20, 0, 0, True),           # no histogram
    (20, -32, 76, False),       # no row outputs
    (44, -32, 76, True),        # a threshold above score_max
    (-33, -32, 76, True),       # ... below score_min
    (43, -32, 76, True),        # ... equal to score_max
    (-2 ** 31, 2 ** 31 - 1024, 1024, True),   # the ends of int
    (2 ** 31 - 1, -2 ** 31, 1024, True),
]


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [0, 3])
def test_windows_thresholds_and_forms(gpu, monkeypatch, capfd, cap):
    M, res, off, _ = input_set("mixed")
    n = off.size - 1
    ctx = device_ctx(M, res, off)
    if cap:
        monkeypatch.setenv("HMK_TEST_GRID_CAP", str(cap))
    for thr, lo, bins, rows in WINDOWS:
        got, launches = survey(ctx, capfd, cap, True, 0, n, 0, n, 3, -1, thr, lo, bins, rows)
        want = expect_triangle("mixed", 3, -1, 0, n, thr, lo, bins, rows)
        check(got, want, launches)
        assert launches == (3 if rows else 2)
        if (lo, bins) == (-10, 30):
            assert got[2].n_below > 0 and got[2].n_above > 0
        if thr in (-33, -2 ** 31):
            assert got[2].n_at_or_above == n * (n - 1) // 2 and (got[1][2] == n - 1).all()
        if thr in (44, 2 ** 31 - 1):
            assert got[2].n_at_or_above == 0 and not got[1][2].any()


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [0, 1, 3])
def test_range_sizes_as_triangles(gpu, monkeypatch, capfd, cap):
    """ranges of 1, 2, T - 1, T, T + 1 and 2 T + 1 members cut from mixed: no tile, one ragged tile, one full tile, a second block row
    of one member, three block rows"""
    M, res, off, _ = input_set("mixed")
    ctx = device_ctx(M, res, off)
    if cap:
        monkeypatch.setenv("HMK_TEST_GRID_CAP", str(cap))
    for X, p in MIXED_PARAMS[:2]:
        for s in SIZES:
            for q0 in (0, 301):
                got, launches = survey(ctx, capfd, cap, True, q0, q0 + s, q0, q0 + s, X, p, 12, -32, 90)
                check(got, expect_triangle("mixed", X, p, q0, q0 + s, 12, -32, 90), launches)
                assert launches == (0 if s == 1 else 3)
                if s == 1:
                    assert (got[1][0][0], got[1][1][0], got[1][2][0]) == (INT32_MIN, UINT32_MAX, 0) and not got[0].any()
                    assert (got[2].score_min, got[2].score_max) == (INT32_MAX, INT32_MIN)


RECTANGLES = [(1, 1), (1, 2 * T + 1), (2 * T + 1, 1), (2, T - 1), (T - 1, 2), (T, T + 1), (T + 1, T), (T - 1, T), (2, 2), (T, T),
              (T + 1, 2 * T + 1), (2 * T + 1, T + 1), (2 * T + 1, 2 * T + 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [0, 1, 3])
@pytest.mark.parametrize("name", ["mixed", "asymmetric"])
def test_rectangles_match_the_oracle(gpu, monkeypatch, capfd, name, cap):
    """every size on either side, the queries before the references and after them; under the perturbed matrix seq1 = the query is
    the only orientation that passes"""
    M, res, off, _ = input_set(name)
    ctx = device_ctx(M, res, off)
    if cap:
        monkeypatch.setenv("HMK_TEST_GRID_CAP", str(cap))
    X, p = 3, -1
    for nq, nr in RECTANGLES:
        if name == "asymmetric" and nq + nr > 600:
            continue
        for q0, r0 in ((3, 3 + nq), (5 + nr, 5)):
            got, launches = survey(ctx, capfd, cap, False, q0, q0 + nq, r0, r0 + nr, X, p, 10, -40, 100)
            check(got, expect_rectangle(name, X, p, q0, q0 + nq, r0, r0 + nr, 10, -40, 100), launches)
            assert launches == 3 and int(got[1][2].sum()) == got[2].n_at_or_above
    got, launches = survey(ctx, capfd, cap, False, 0, 257, 257, 600, X, p, 10, 0, 0)
    check(got, expect_rectangle(name, X, p, 0, 257, 257, 600, 10, 0, 0), launches)
    got, launches = survey(ctx, capfd, cap, False, 257, 600, 0, 257, X, p, 10, -40, 100, rows=False)
    check(got, expect_rectangle(name, X, p, 257, 600, 0, 257, 10, -40, 100, rows=False), launches)
    if name == "asymmetric":
        with pytest.raises(ValueError, match="symmetric"):
            ctx.score_survey_shifted(0, 600, 0, 600, X, p, 10, score_lo=-40, n_bins=100)


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [0, 3])
def test_the_other_histogram_form_agrees(gpu, monkeypatch, capfd, cap):
    """the wave-aggregated LDS histogram that tools/bench_survey.py times beside the lane-replicated one every call runs (DESIGN.md
    5.18): the same bins, on the input with one bin for all 64 lanes too"""
    form = N.lib.hmk_survey_hist_form_for_measurement
    if cap:
        monkeypatch.setenv("HMK_TEST_GRID_CAP", str(cap))
    assert form(1) == 0
    try:
        for name, hi in (("mixed", 1300), ("copies", 70)):
            M, res, off, _ = input_set(name)
            ctx = device_ctx(M, res, off)
            for lo, bins, rows in ((-32, 76, True), (-10, 30, False), (-500, 1024, True)):
                got, launches = survey(ctx, capfd, cap, True, 0, hi, 0, hi, 3, -1, 20, lo, bins, rows)
                check(got, expect_triangle(name, 3, -1, 0, hi, 20, lo, bins, rows), launches)
            got, launches = survey(ctx, capfd, cap, False, 0, 30, 30, hi, 3, -1, 20, -32, 76)
            check(got, expect_rectangle(name, 3, -1, 0, 30, 30, hi, 20, -32, 76), launches)
    finally:
        assert form(0) == 1


@pytest.mark.gpu
def test_empty_pair_spaces(gpu, capfd):
    M, res, off, _ = input_set("mixed")
    ctx = device_ctx(M, res, off)
    for q0, q1, r0, r1 in ((7, 7, 0, 1300), (0, 40, 90, 90), (0, 40, 20, 20), (9, 10, 9, 10), (5, 5, 5, 5), (1300, 1300, 0, 0)):
        got, launches = survey(ctx, capfd, 0, q0 == r0 and q1 == r1, q0, q1, r0, r1, 3, -1, 20, -5, 64)
        hist, (best, index, degree), stats = got
        assert launches == 0 and not hist.any() and hist.size == 64 and best.size == q1 - q0
        assert (best == INT32_MIN).all() and (index == UINT32_MAX).all() and not degree.any()
        assert [getattr(stats, k) for k in STAT_NAMES] == [0, 0, 0, 0, INT32_MAX, INT32_MIN, 0, 0] and stats.kernel_ms == 0
    hist, out, stats = ctx.score_survey_shifted(7, 7, 0, 1300, 3, -1, 20, rows=False)   # nothing wanted of an empty pair space
    assert hist is None and out is None and stats.pairs_scored == 0
    with pytest.raises(hammock_amd.DataException):                                       # the shift against the shortest length (7)
        ctx.score_survey_shifted(0, 1300, 0, 1300, 7, -1, 20, n_bins=8)


@pytest.mark.gpu
def test_state_between_calls(gpu, capfd):
    """one context: other parameters, ranges, windows and forms in between, then the first call again, equal to the first"""
    M, res, off, _ = input_set("mixed")
    ctx = device_ctx(M, res, off)

    def tri(X, p, q0, q1, thr, lo, bins, rows=True):
        got, launches = survey(ctx, capfd, 0, True, q0, q1, q0, q1, X, p, thr, lo, bins, rows)
        check(got, expect_triangle("mixed", X, p, q0, q1, thr, lo, bins, rows), launches)
        return got

    first = tri(3, -1, 0, 1300, 20, -32, 76)
    tri(2, -1, 0, 1300, 15, -20, 40)
    tri(3, 0, 100, 900, 25, 0, 0)
    got, launches = survey(ctx, capfd, 0, False, 0, 300, 300, 1300, 3, -1, 20, -32, 76)
    check(got, expect_rectangle("mixed", 3, -1, 0, 300, 300, 1300, 20, -32, 76), launches)
    tri(3, -1, 0, 1300, 43, -32, 76, rows=False)
    for _ in range(2):
        again = tri(3, -1, 0, 1300, 20, -32, 76)
        assert np.array_equal(first[0], again[0]) and all(np.array_equal(x, y) for x, y in zip(first[1], again[1]))
        assert all(getattr(first[2], k) == getattr(again[2], k) for k in STAT_NAMES)


@pytest.mark.gpu
def test_device_list_runs_on_the_root(gpu, capfd):
    M, res, off, _ = input_set("mixed")
    ctx = hammock_amd.Context(M, device=[0, 0])
    ctx.set_sequences(residues=res, offsets=off)
    got, launches = survey(ctx, capfd, 0, True, 0, 1300, 0, 1300, 2, -1, 20, -32, 76)
    check(got, expect_triangle("mixed", 2, -1, 0, 1300, 20, -32, 76), launches)
    got, launches = survey(ctx, capfd, 0, False, 1000, 1300, 0, 1000, 2, -1, 20, -32, 76)
    check(got, expect_rectangle("mixed", 2, -1, 1000, 1300, 0, 1000, 20, -32, 76), launches)


@pytest.mark.gpu
def test_existing_calls_agree(gpu):
    """the neighbour pass's edge count, the components scan's levels and the best-1 search on the same input"""
    M, res, off, _ = input_set("mixed")
    n, X, p = 1300, 3, -1
    ctx = device_ctx(M, res, off)
    hist, (best, index, degree), stats = ctx.score_survey_shifted(0, n, 0, n, X, p, 20, score_lo=-32, n_bins=60)   # scores up to 27 in hist
    assert stats.n_above > 0
    edges, nstats = ctx.neighbors_shifted(X, p, 20)
    assert nstats.n_edges == stats.n_at_or_above == 476
    _, levels = ctx.components_shifted(X, p, 20, 28, component=False)
    for t in range(20, 29):
        assert levels["n_edges"][t - 20] == int(hist[t + 32:].sum()) + stats.n_above, t
        assert levels["n_singletons"][t - 20] == int((best < t).sum()), t
    thr = 12
    _, (best, index, degree), stats = ctx.score_survey_shifted(0, 400, 400, n, X, p, thr)
    hit, score = ctx.search_best_shifted(0, 400, 400, n, X, p, thr, 1)
    found = best >= thr
    assert 50 < found.sum() < 400
    assert np.array_equal(hit[found, 0], index[found].astype(np.int64)) and np.array_equal(score[found, 0], best[found])
    assert (hit[~found, 0] == -1).all() and np.array_equal(found, degree > 0)


def _matrix_file(tmp_path):
    """the default matrix with W/W raised to 60: symmetric, and the first window of `survey` (ending at 20 x 60) misses every score"""
    lines = open(os.path.join(ROOT, "hammock_amd", "matrices", "blosum62.txt")).read().splitlines()
    head = next(k for k, line in enumerate(lines) if not line.startswith("#"))
    col = lines[head].split().index("W")
    row = next(k for k in range(head + 1, len(lines)) if lines[k].startswith("W"))
    lines[row] = lines[row][:1 + 3 * col] + " 60" + lines[row][1 + 3 * col + 3:]
    path = tmp_path / "w60.txt"
    path.write_text("\n".join(lines) + "\n")
    M = _blosum62().copy().reshape(24, 24)
    w = LETTERS.index("W")
    assert M[w, w] == 11
    M[w, w] = 60
    return str(path), M


def _survey_files(strings, partners, want, score_min, score_max, lo):
    """the two files from the oracle's numbers"""
    hist, (best, index, degree), _ = want
    pairs = hist[score_min - lo:score_max - lo + 1].astype(np.int64)
    has = index != UINT32_MAX
    rows_best = np.bincount(best[has] - score_min, minlength=pairs.size)
    out = ["score\tpairs\tpairs_at_or_above\tsequences_best\tsequences_best_at_or_above"]
    out += [f"{score_min + k}\t{pairs[k]}\t{pairs[k:].sum()}\t{rows_best[k]}\t{rows_best[k:].sum()}" for k in range(pairs.size)]
    nn = ["sequence\tbest_partner\tbest_score\tneighbors_at_threshold"]
    nn += [f"{s}\t{partners[index[k]] if has[k] else 'NA'}\t{best[k] if has[k] else 'NA'}\t{degree[k]}" for k, s in enumerate(strings)]
    return "\n".join(out) + "\n", "\n".join(nn) + "\n"


@pytest.mark.gpu
def test_cli_survey_files(gpu, coracle, tmp_path):
    """`survey` with and without --database writes what the oracle's numbers say, byte for byte; with a matrix whose largest cell no
    pair comes near, the first window misses and the second call's is used; a span beyond the bins is refused"""
    _, res, off, strings = input_set("mixed")
    X, p, thr = 3, -1, 18
    fa, db = tmp_path / "in.fa", tmp_path / "db.fa"
    fa.write_text("".join(f">{k}\n{s}\n" for k, s in enumerate(strings[:700])))
    db.write_text("".join(f">{k}\n{s}\n" for k, s in enumerate(strings[700:])))
    common = ["-x", str(X), "-p", str(p), "-g", str(thr)]
    # the triangle, the default matrix: one call
    r = cli("survey", "-i", str(fa), "-d", str(tmp_path / "t"), *common, timeout=600)
    assert r.returncode == 0, r.stderr
    assert "Scoring again" not in r.stderr
    want = expect_triangle("mixed", X, p, 0, 700, thr, -100, 200)
    hfile, nfile = _survey_files(strings[:700], strings, want, want[2]["score_min"], want[2]["score_max"], -100)
    assert (tmp_path / "t" / "score_histogram.tsv").read_text() == hfile
    assert (tmp_path / "t" / "nearest_neighbors.tsv").read_text() == nfile
    assert f"Pairs scored: {700 * 699 // 2}, pairs at or above the threshold: {want[2]['n_at_or_above']}, GPU kernels: " in r.stderr
    assert f"Parameters: max shift {X}, gap penalty {p}, threshold {thr}" in (tmp_path / "t" / "run.log").read_text()
    # the rectangle against a database
    r = cli("survey", "-i", str(fa), "--database", str(db), "-d", str(tmp_path / "r"), *common, timeout=600)
    assert r.returncode == 0, r.stderr
    want = expect_rectangle("mixed", X, p, 0, 700, 700, 1300, thr, -100, 200)
    hfile, nfile = _survey_files(strings[:700], strings, want, want[2]["score_min"], want[2]["score_max"], -100)
    assert (tmp_path / "r" / "score_histogram.tsv").read_text() == hfile
    assert (tmp_path / "r" / "nearest_neighbors.tsv").read_text() == nfile
    assert f"Pairs scored: {700 * 600}, pairs at or above the threshold: {want[2]['n_at_or_above']}, GPU kernels: " in r.stderr
    # W/W = 60: the first window ends at 1,200 and starts at 177, above every score
    path, M60 = _matrix_file(tmp_path)
    hi, lo = np.tril_indices(700, -1)
    st, sc = coracle.score_pairs(M60, res, off, hi, lo, 0, X, p)
    assert st == 0 and sc.max() < 177
    S = np.zeros((700, 700), dtype=np.int64)
    S[hi, lo] = sc
    S[lo, hi] = sc
    want = reduce_scores(S, ~np.eye(700, dtype=bool), 0, sc, thr, -100, 400)
    r = cli("survey", "-i", str(fa), "-m", path, "-d", str(tmp_path / "w"), *common, timeout=600)
    assert r.returncode == 0, r.stderr
    assert f"Scoring again for the scores {sc.min()} to {sc.max()}" in r.stderr
    hfile, nfile = _survey_files(strings[:700], strings, want, int(sc.min()), int(sc.max()), -100)
    assert (tmp_path / "w" / "score_histogram.tsv").read_text() == hfile
    assert (tmp_path / "w" / "nearest_neighbors.tsv").read_text() == nfile
    # a penalty that spreads the scores over more than HMK_SURVEY_MAX_BINS values
    r = cli("survey", "-i", str(fa), "-d", str(tmp_path / "s"), "-x", "3", "-p", "-200", "-g", "18", timeout=600)
    assert r.returncode == 2 and "HMK_SURVEY_MAX_BINS" in r.stderr
    # one sequence: no pair, no partner
    one = tmp_path / "one.fa"
    one.write_text(f">0\n{strings[0]}\n")
    r = cli("survey", "-i", str(one), "-d", str(tmp_path / "o"), "-x", "3", timeout=600)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "o" / "score_histogram.tsv").read_text().count("\n") == 1
    assert (tmp_path / "o" / "nearest_neighbors.tsv").read_text().splitlines()[1] == f"{strings[0]}\tNA\tNA\t0"
