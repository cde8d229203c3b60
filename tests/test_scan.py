"""Scanning peptides along long targets (hmk_set_targets, hmk_scan_shifted).

The expectation is `window_table`, a numpy restatement of ShiftedScorer.java:67-85 per window: for every offset s in [-X, d + X]
the cells M[peptide residue][target residue] over the overlap, + d p, + 2 p per residue of overhang.  Both modes' records and both
coverage arrays follow from it.  A CPU test ties it to the two oracles (maximum and first arg-max against shifted_score on every
pair of every GPU input); another asserts on it alone that the constructed inputs hold what the GPU tests rely on."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, random_peptides
from test_assign import gpu   # noqa: F401  (the fixture that skips where no HIP device is visible)

import hammock_amd
from hammock_amd import _native as N
from hammock_amd.api import SCAN_HIT_DTYPE

CHUNK = 1024            # SCAN_CHUNK of hmk_scan.h
FIRST_HITS = 1 << 16    # SCAN_FIRST_HITS
GROUP = 8               # SCAN_GROUP
GRID_KERNELS = {"k_scan_tables", "k_scan_packed", "k_scan_literal", "k_scan_pair_insert", "k_scan_pair_compact", "k_scan_cover_add",
                "k_scan_cover_scan"}
LINE = re.compile(r"^\[hmk grid\] (\S+) (\d+) -> (\d+)$", re.M)
BIG_SIZE = 2 ** 31 - 1
LOW_THR = -8             # a threshold most windows of random 12-mers stay below, and enough pass to outgrow the first scratch


# ---- matrices ---------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def matrix(name):
    import json
    with open(os.path.join(GOLDEN, "matrices.json")) as fh:
        B = np.asarray(json.load(fh)["matrices"]["blosum62"], dtype=np.int32)
    if name == "blosum62":
        return B
    if name == "asymmetric":   # M[a][b] != M[b][a] for most a != b: an index-order mistake changes the scores
        i, j = np.indices((24, 24))
        return (B + np.where(i < j, (i * 7 + j * 3) % 3, 0)).astype(np.int32)
    if name == "thousands":    # +-1,000: literal by necessity, scores beyond int16
        return np.where(np.eye(24, dtype=bool), 1000, -1000).astype(np.int32)
    raise KeyError(name)


# ---- inputs -----------------------------------------------------------------------------------------------------------------

def mutate(rng, pep, k):
    out = pep.copy()
    for pos in rng.choice(len(pep), size=k, replace=False):
        out[pos] = (out[pos] + 1 + rng.integers(0, 19)) % 20
    return out


@functools.lru_cache(maxsize=None)
def bases():
    rng = np.random.default_rng(11)
    return {L: rng.integers(0, 20, size=L, dtype=np.uint8) for L in (6, 7, 12, 13, 20, 32)}   # 13: the second 12-mer's source


def base12b():
    return bases()[13][:12].copy()


@functools.lru_cache(maxsize=None)
def plants():
    """what is planted along the targets, in turn: the base peptides and copies with one or two substitutions"""
    rng = np.random.default_rng(12)
    b = bases()
    out = [b[12], b[6], b[7], b[20], base12b(), mutate(rng, b[12], 1), mutate(rng, b[12], 2), mutate(rng, b[20], 2), mutate(rng, b[7], 1), b[32]]
    return [np.asarray(p, dtype=np.uint8) for p in out]


TARGET_LENGTHS = [33, 34, 63, 64, 65, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 100]


@functools.lru_cache(maxsize=None)
def edge_targets():
    """the boundary targets (random over 20 letters, peptides planted at offset 0, at n - m, across every lane-64, 256 and chunk
    boundary), then: one that begins with a 12-mer's suffix, one that ends with its prefix, a periodic one"""
    rng = np.random.default_rng(13)
    P = plants()
    out, turn = [], 0
    for n in TARGET_LENGTHS:
        t = rng.integers(0, 20, size=n, dtype=np.uint8)
        first, last = P[turn % 9], P[(turn + 4) % 9]
        t[:len(first)] = first
        t[n - len(last):] = last                 # (at 33 and 34 residues a 12-mer behind a 12-mer and behind a 6-mer: no overlap)
        turn += 1
        k = 1
        while 64 * k + 40 < n:
            pep = P[turn % len(P)] if n > 3 * CHUNK else P[turn % 9]   # (the 32-mer only on the longest target)
            pos = 64 * k - (3 if (k + k // 4 + k // 16) % 2 else 4)   # at max shift 3: the window is lane 0 of a wave, or lane 63 of the one before
            t[pos:pos + len(pep)] = pep
            turn += 1
            k += 1
        out.append(t)
    b12 = bases()[12]
    out.append(np.concatenate([b12[3:], rng.integers(0, 20, size=40, dtype=np.uint8)]))    # best window at s = -3
    out.append(np.concatenate([rng.integers(0, 20, size=40, dtype=np.uint8), b12[:9]]))    # best window at s = d + 3
    out.append(np.tile(base12b(), 5))                                                      # ties: every period
    return out


SUFFIX_T, PREFIX_T, PERIODIC_T = len(TARGET_LENGTHS), len(TARGET_LENGTHS) + 1, len(TARGET_LENGTHS) + 2


@functools.lru_cache(maxsize=None)
def many_targets():
    rng = np.random.default_rng(14)
    P = plants()
    out = []
    for k in range(300):
        n = 33 + (k * 7) % 48
        t = rng.integers(0, 20, size=n, dtype=np.uint8)
        if k % 3 == 0:
            pep = P[k % 9]
            pos = (k * 5) % (n - len(pep) + 1)
            t[pos:pos + len(pep)] = pep
        out.append(t)
    return out


@functools.lru_cache(maxsize=None)
def mixed_peptides():
    """-> (peptides, sizes, n_long): the planted peptides, two random ones of every length 6..32, then (from n_long on) two of every
    length 1..5.  The 12-mer and its copies carry sizes of 2^31 - 1, one peptide the antibodies example's 56,758."""
    rng = np.random.default_rng(15)
    peps = list(plants())
    for L in range(6, 33):
        peps += random_peptides(rng, 2, L, L)
    n_long = len(peps)
    for L in range(1, 6):
        peps += random_peptides(rng, 2, L, L)
    sizes = rng.integers(1, 50, size=len(peps)).astype(np.int32)
    sizes[[0, 5, 6]] = BIG_SIZE
    sizes[1] = 56758
    return peps, sizes, n_long


@functools.lru_cache(maxsize=None)
def uniform_peptides(L):
    """the planted L-mers, then 70 random ones: two runs, the second with a partial last group"""
    rng = np.random.default_rng(100 + L)
    peps = [p for p in plants() if len(p) == L] + random_peptides(rng, 70, L, L)
    return peps, rng.integers(1, 9, size=len(peps)).astype(np.int32)


INPUTS = {
    "mixed": lambda: (mixed_peptides()[0], mixed_peptides()[1], edge_targets()),
    "u6": lambda: (*uniform_peptides(6), edge_targets()),
    "u7": lambda: (*uniform_peptides(7), edge_targets()),
    "u12": lambda: (*uniform_peptides(12), edge_targets()),
    "u20": lambda: (*uniform_peptides(20), edge_targets()),
    "many": lambda: (*uniform_peptides(12), many_targets()),
}
N_LONG = mixed_peptides()[2]
# (input, matrix, query range, X, p, threshold): what the GPU tests scan
LONG = (0, N_LONG)
CASES_MIXED = [("mixed", "blosum62", None, 0, 0, 20), ("mixed", "blosum62", None, 0, -1, 18),
               ("mixed", "blosum62", LONG, 1, -1, 20), ("mixed", "blosum62", LONG, 3, 0, 20), ("mixed", "blosum62", LONG, 3, -4, 16),
               ("mixed", "blosum62", LONG, 5, 1, 24), ("mixed", "blosum62", LONG, 5, 0, 21),
               ("mixed", "asymmetric", LONG, 3, 0, 22), ("mixed", "asymmetric", LONG, 1, -1, 19),
               ("mixed", "thousands", LONG, 3, 1, 10000), ("mixed", "thousands", LONG, 5, 1, 30000)]
UNIFORM = {"u6": (1, 10), "u7": (1, 12), "u12": (3, 20), "u20": (5, 34)}   # max shift and the default threshold of the length
CASES_UNIFORM = [(name, "blosum62", None, X, p, thr + dt) for name, (X, thr) in UNIFORM.items() for p, dt in ((0, 0), (0, -1), (-1, 1))]
CASES_MANY = [("many", "blosum62", None, 3, 0, 20), ("many", "blosum62", None, 3, -1, 19)]
ALL_CASES = CASES_MIXED + CASES_UNIFORM + CASES_MANY


def case_id(c):
    return f"{c[0]}-{c[1]}-X{c[3]}-p{c[4]}-t{c[5]}"


# ---- the definition ---------------------------------------------------------------------------------------------------------

class Table:
    """every window of every (q, t) of one input: flat q, t, s, w; per pair (row q, column t) the maximum and its first offset"""
    pass


def window_scores(M, peps, target, X, p):
    """w[k, s + X] for peptides of ONE length against one target (ShiftedScorer.java:67-85, seq1 = peptide, seq2 = target)"""
    Mx = np.concatenate([np.asarray(M, dtype=np.int64), np.zeros((24, 1), dtype=np.int64)], axis=1)   # column 24: beyond the target, no cell
    P = np.asarray(peps, dtype=np.int64)
    m, n = P.shape[1], len(target)
    d = n - m
    ext = np.concatenate([np.full(X, 24), np.asarray(target, dtype=np.int64), np.full(X, 24)])
    win = np.lib.stride_tricks.sliding_window_view(ext, m)             # row s + X: the target residues under the window at offset s (:67)
    cells = Mx[P[:, None, :], win[None, :, :]].sum(axis=2)              # :69-77, the matrix index [peptide residue][target residue]
    s = np.arange(-X, d + X + 1)
    pen = d * p + 2 * p * np.maximum(-s, 0) + 2 * p * np.maximum(s - d, 0)   # :79, :80-82, :83-85
    return cells + pen[None, :], s


@functools.lru_cache(maxsize=None)
def window_table(name, mname, X, p, transpose=False):
    return make_table(*INPUTS[name](), matrix(mname).T if transpose else matrix(mname), X, p)


def make_table(peps, sizes, targets, M, X, p):
    by_len = {}
    for q, pep in enumerate(peps):
        by_len.setdefault(len(pep), []).append(q)
    Q, T, S, W = [], [], [], []
    best = np.zeros((len(peps), len(targets)), dtype=np.int64)
    arg = np.zeros((len(peps), len(targets)), dtype=np.int64)
    for t, target in enumerate(targets):
        for m, qs in by_len.items():
            if X >= m:
                continue
            w, s = window_scores(M, [peps[q] for q in qs], target, X, p)
            Q.append(np.repeat(qs, w.shape[1])); T.append(np.full(w.size, t)); S.append(np.tile(s, len(qs))); W.append(w.ravel())
            best[qs, t] = w.max(axis=1)
            arg[qs, t] = s[w.argmax(axis=1)]          # the first maximum: the strict ">" of :86-89
    tb = Table()
    tb.q, tb.t, tb.s, tb.w = (np.concatenate(a) for a in (Q, T, S, W))
    tb.best, tb.arg = best, arg
    tb.peps, tb.sizes, tb.targets = peps, sizes, targets
    return tb


def as_records(q, t, score, s):
    out = np.zeros(len(q), dtype=SCAN_HIT_DTYPE)
    out["query"], out["target"], out["score"], out["offset"] = q, t, score, s
    return np.sort(out, order=["target", "offset", "query"])


def expect_records(tb, thr, all_windows, qr=None, tr=None):
    q0, q1 = qr or (0, len(tb.peps))
    t0, t1 = tr or (0, len(tb.targets))
    if all_windows:
        k = (tb.w >= thr) & (tb.q >= q0) & (tb.q < q1) & (tb.t >= t0) & (tb.t < t1)
        return as_records(tb.q[k], tb.t[k], tb.w[k], tb.s[k])
    qq, tt = np.nonzero(tb.best[q0:q1, t0:t1] >= thr)
    return as_records(qq + q0, tt + t0, tb.best[qq + q0, tt + t0], tb.arg[qq + q0, tt + t0])


def expect_coverage(tb, recs, tr=None):
    t0, t1 = tr or (0, len(tb.targets))
    off = np.concatenate([[0], np.cumsum([len(t) for t in tb.targets])])
    cc = np.zeros(int(off[t1] - off[t0]), dtype=np.uint32)
    cs = np.zeros(cc.size, dtype=np.uint64)
    for r in recs:
        m, n = len(tb.peps[r["query"]]), len(tb.targets[r["target"]])
        base = int(off[r["target"]] - off[t0])
        a, b = max(int(r["offset"]), 0), min(int(r["offset"]) + m, n)
        cc[base + a:base + b] += 1
        cs[base + a:base + b] += np.uint64(tb.sizes[r["query"]])
    return cc, cs


def bound_limit(m, X, p, thr, d, bias, max_m):
    """the planner's class rule, restated: the largest row bound with every byte lane in [0, 255], -1 if none"""
    if m < 6 or m > 20 or X > 5 or max_m + bias > 255:
        return -1
    g = 128 - thr + d * p
    limit = 1 << 40
    for k in range(X + 1):
        if g + 2 * p * k - bias * m < 0:
            return -1
        limit = min(limit, 255 - g - 2 * p * k)
    return limit if limit >= 0 else -1


def expect_forms(M, peps, targets, qr, tr, X, p, thr, no_packed=False):
    """-> (windows_packed, windows_literal): groups of 8 consecutive peptides of one length in (length, index) order"""
    q0, q1 = qr
    bias, max_m = max(0, -int(M.min())), int(M.max())
    by_len = {}
    for q in range(q0, q1):
        by_len.setdefault(len(peps[q]), []).append(q)
    packed = total = 0
    for t in range(*tr):
        n = len(targets[t])
        for m, qs in by_len.items():
            nwin = n - m + 2 * X + 1
            total += nwin * len(qs)
            limit = -1 if no_packed else bound_limit(m, X, p, thr, n - m, bias, max_m)
            for g in range(0, len(qs), GROUP):
                bound = max(int(np.maximum(M[peps[q]].max(axis=1), 0).sum()) for q in qs[g:g + GROUP])
                if bound <= limit:
                    packed += nwin * len(qs[g:g + GROUP])
    return packed, total - packed


# ---- CPU ----------------------------------------------------------------------------------------------------------------------

def test_symbols_structures_and_abi():
    with open(os.path.join(ROOT, "include", "hammock_hip.h")) as fh:
        header = fh.read()
    for name in ("hmk_set_targets", "hmk_scan_shifted"):
        assert name + "(" in header and name in N.SYMBOLS and hasattr(N.lib, name)
    assert "#define HMK_TARGET_MAX_LEN (1u << 20)" in header and "#define HMK_SCAN_ALL_WINDOWS 1u" in header
    assert N.lib.hmk_abi_version() == 4 and "#define HMK_ABI_VERSION 4" in header
    assert C.sizeof(N.ScanHit) == 16 == SCAN_HIT_DTYPE.itemsize
    assert C.sizeof(N.ScanStats) == 56
    assert (N.HMK_TARGET_MAX_LEN, N.HMK_SCAN_ALL_WINDOWS) == (1 << 20, 1)
    with open(os.path.join(ROOT, "hammock_amd", "csrc", "hmk_scan.h")) as fh:
        text = fh.read()
    assert f"SCAN_CHUNK = {CHUNK};" in text and "SCAN_FIRST_HITS = 1u << 16;" in text and f"SCAN_GROUP = {GROUP};" in text


def host_ctx(seqs=("WVTAPRSLPVLP", "RSPIV"), targets=("A" * 40, "C" * 100)):
    ctx = hammock_amd.Context(matrix("blosum62"), device=-1)
    if seqs:
        ctx.set_sequences(list(seqs))
    if targets:
        ctx.set_targets(list(targets))
    return ctx


def raw_set_targets(ctx, residues, offsets, n, null=False):
    residues = np.ascontiguousarray(residues, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    return N.lib.hmk_set_targets(ctx._h, None if null else residues.ctypes.data_as(C.POINTER(C.c_uint8)),
                                 offsets.ctypes.data_as(C.POINTER(C.c_uint64)), n)


def test_set_targets_checks_on_a_host_only_context():
    ctx = host_ctx(targets=None)
    ok = np.zeros(100, dtype=np.uint8)
    assert raw_set_targets(ctx, ok, [0, 33, 100], 2) == N.HMK_OK
    assert raw_set_targets(ctx, ok, [0, 32, 100], 2) == N.HMK_ERR_BAD_ARG                # a 32-residue "target" is a sequence
    assert b"hmk_search_shifted" in N.lib.hmk_last_error(ctx._h)
    assert raw_set_targets(ctx, ok, [0, 60, 50], 2) == N.HMK_ERR_BAD_ARG                 # offsets do not ascend
    assert raw_set_targets(ctx, ok, [1, 50, 100], 2) == N.HMK_ERR_BAD_ARG
    bad = ok.copy(); bad[70] = 24
    assert raw_set_targets(ctx, bad, [0, 33, 100], 2) == N.HMK_ERR_BAD_ARG               # residue code >= 24
    assert raw_set_targets(ctx, ok, [0, 33, 100], 2, null=True) == N.HMK_ERR_BAD_ARG
    assert raw_set_targets(ctx, ok[:40], [0, 40, 40 + (1 << 20) + 1], 2) == N.HMK_ERR_BAD_ARG   # longer than HMK_TARGET_MAX_LEN (checked before any residue is read)
    assert raw_set_targets(ctx, ok[:40], [0, 40] + [40 + (k + 1) * (1 << 20) for k in range(2048)], 2049) == N.HMK_ERR_BAD_ARG   # 2^31 residues
    # the failed calls left the targets of the first one in place; n_targets = 0 clears them
    st = N.ScanStats()
    scan = lambda t1: N.lib.hmk_scan_shifted(ctx._h, 0, 1, 0, t1, 3, 0, 20, 0, None, 0, None, None, C.byref(st))
    assert scan(2) == N.HMK_ERR_DEVICE and scan(3) == N.HMK_ERR_BAD_ARG
    assert raw_set_targets(ctx, ok, [0], 0, null=True) == N.HMK_OK
    assert scan(1) == N.HMK_ERR_NO_SEQUENCES


def test_scan_checks_on_a_host_only_context():
    ctx = host_ctx()
    st = N.ScanStats()
    hits = (N.ScanHit * 4)()

    def scan(q0=0, q1=1, t0=0, t1=2, X=3, p=0, thr=20, flags=0, h=hits, cap=4, stats=st):
        return N.lib.hmk_scan_shifted(ctx._h, q0, q1, t0, t1, X, p, thr, flags, h, cap, None, None, C.byref(stats) if stats is not None else None)

    assert scan() == N.HMK_ERR_DEVICE                        # every check passed: no device, no result
    assert scan(stats=None) == N.HMK_ERR_BAD_ARG
    assert scan(h=None) == N.HMK_ERR_BAD_ARG and scan(h=None, cap=0) == N.HMK_ERR_DEVICE
    assert scan(flags=2) == N.HMK_ERR_BAD_ARG and scan(flags=1) == N.HMK_ERR_DEVICE
    assert scan(q1=3) == N.HMK_ERR_BAD_ARG and scan(q0=2, q1=1) == N.HMK_ERR_BAD_ARG
    assert scan(t1=3) == N.HMK_ERR_BAD_ARG and scan(t0=2, t1=1) == N.HMK_ERR_BAD_ARG
    assert scan(X=-1) == N.HMK_ERR_BAD_ARG
    assert scan(p=1023) == N.HMK_ERR_DEVICE and scan(p=1024) == N.HMK_ERR_BAD_ARG and scan(p=-1024) == N.HMK_ERR_BAD_ARG   # |p| (2^20 + 2X) + 32 * 11 against 2^30
    assert scan(X=12) == N.HMK_ERR_SHIFT_TOO_BIG and scan(X=11) == N.HMK_ERR_DEVICE
    assert scan(q1=2, X=5) == N.HMK_ERR_SHIFT_TOO_BIG and scan(q0=1, q1=2, X=4) == N.HMK_ERR_DEVICE
    assert scan(q1=2, X=5) == N.HMK_ERR_SHIFT_TOO_BIG and b"Shift too big: 4 is maximum, but 5 found" in N.lib.hmk_last_error(ctx._h)
    # an empty range on either side: HMK_OK, no records, zeroed coverage
    cc = np.full(140, 7, dtype=np.uint32)
    cs = np.full(140, 7, dtype=np.uint64)
    assert N.lib.hmk_scan_shifted(ctx._h, 1, 1, 0, 2, 3, 0, 20, 0, hits, 4, cc.ctypes.data_as(C.POINTER(C.c_uint32)),
                                  cs.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(st)) == N.HMK_OK
    assert st.n_hits == 0 and not cc.any() and not cs.any()
    assert scan(t0=1, t1=1) == N.HMK_OK and st.n_hits == 0
    got = ctx.scan_shifted(0, 0, 0, 2, 3, 0, 20, coverage=True)
    assert len(got[0]) == 0 and got[2].size == 140 and not got[2].any() and not got[3].any()
    # without a set
    no_seqs, no_targets = host_ctx(seqs=None), host_ctx(targets=None)
    assert N.lib.hmk_scan_shifted(no_seqs._h, 0, 0, 0, 1, 3, 0, 20, 0, None, 0, None, None, C.byref(st)) == N.HMK_ERR_NO_SEQUENCES
    assert N.lib.hmk_scan_shifted(no_targets._h, 0, 1, 0, 1, 3, 0, 20, 0, None, 0, None, None, C.byref(st)) == N.HMK_ERR_NO_SEQUENCES
    assert N.lib.hmk_scan_shifted(no_targets._h, 0, 1, 0, 0, 3, 0, 20, 0, None, 0, None, None, C.byref(st)) == N.HMK_OK
    with pytest.raises(hammock_amd.DeviceError):
        ctx.scan_shifted(0, 1, 0, 2, 3, 0, 20)
    with pytest.raises(hammock_amd.DataException):
        ctx.scan_shifted(0, 2, 0, 2, 5, 0, 20)


@pytest.mark.parametrize("case", ALL_CASES, ids=case_id)
def test_the_definition_is_the_oracles_score_with_shift(coracle, case):
    """maximum and first arg-max of the definition against the C oracle's shifted_score(M, peptide, target, X, p) on every pair of
    the input (score, and shift == -offset); against the Python oracle on a sample"""
    name, mname, qr, X, p, _ = case
    tb, M = window_table(name, mname, X, p), matrix(mname)
    q0, q1 = qr or (0, len(tb.peps))
    for q in range(q0, q1):
        for t, target in enumerate(tb.targets):
            st, score, shift = coracle.shifted_score(M, tb.peps[q], target, X, p)
            assert (st, score, -shift) == (0, tb.best[q, t], tb.arg[q, t]), (q, t)
    from oracle import hammock_oracle as po
    rng = np.random.default_rng(5)
    text = lambda a: "".join(po.AMINO_ACIDS[int(c)] for c in a)
    scorer = po.ShiftedScorer(M.tolist(), p, X)
    for _ in range(12):
        q, t = int(rng.integers(q0, q1)), int(rng.integers(0, min(len(tb.targets), 9)))
        score, shift = scorer.score_with_shift(po.UniqueSequence(text(tb.peps[q])), po.UniqueSequence(text(tb.targets[t])))
        assert (score, -shift) == (tb.best[q, t], tb.arg[q, t]), (q, t)


def test_the_inputs_hold_what_the_gpu_tests_claim():
    tb = window_table("mixed", "blosum62", 3, 0)
    d = lambda q, t: len(tb.targets[t]) - len(tb.peps[q])
    assert tb.arg[0, SUFFIX_T] == -3 and tb.best[0, SUFFIX_T] >= 20              # a best window at s < 0, and at s = -X
    assert tb.arg[0, PREFIX_T] == d(0, PREFIX_T) + 3 and tb.best[0, PREFIX_T] >= 20   # ... at s > d, and at s = d + X
    tb5 = window_table("mixed", "blosum62", 5, 0)
    assert tb5.arg[0, SUFFIX_T] == -3 and tb5.arg[0, PREFIX_T] == d(0, PREFIX_T) + 3  # inside the overhang range at X = 5
    # a tie between windows of one pair: the periodic target under its unit, every period at the same score, the first one kept
    k = (tb.q == 4) & (tb.t == PERIODIC_T)
    top = tb.w[k].max()
    assert list(tb.s[k][tb.w[k] == top]) == [0, 12, 24, 36, 48] and tb.arg[4, PERIODIC_T] == 0 and top >= 20
    # pairs below the threshold, pairs above
    assert (tb.best[:N_LONG] < 20).any() and (tb.best[:N_LONG] >= 20).any()
    # hits on both sides of every boundary: window indices (offset + X) just below and at / above every multiple of 64 up to the
    # longest target's last, for the packed lengths' planted peptides
    long_t = len(TARGET_LENGTHS) - 1
    k = (tb.t == long_t) & (tb.w >= 20)
    win = np.unique(tb.s[k] + 3)
    for b in range(64, 3 * CHUNK + 1, 64):        # a hit in the last lane before or the first lane behind every boundary ...
        assert b in win or b - 1 in win, b
    for step in (64, 256, CHUNK):                   # ... and on both sides for each kind of boundary
        assert any(b in win for b in range(step, 3 * CHUNK + 1, step)) and any(b - 1 in win for b in range(step, 3 * CHUNK + 1, step)), step
    for t, n in enumerate(TARGET_LENGTHS):      # offset 0 and offset n - m are hits on every boundary target
        k = (tb.t == t) & (tb.w >= 20)
        assert (tb.s[k] == 0).any(), n
        assert any(tb.s[k][j] == n - len(tb.peps[tb.q[k][j]]) for j in range(k.sum())), n
    # the three big-size peptides' windows meet on a position: a coverage_size above 2^32
    rec = expect_records(tb, 20, True, LONG)
    cc, cs = expect_coverage(tb, rec)
    assert int(cs.max()) > 2 ** 32 and int(cc.max()) >= 3
    # the asymmetric matrix: scoring with the index order swapped gives other records
    a, b = window_table("mixed", "asymmetric", 3, 0), window_table("mixed", "asymmetric", 3, 0, True)
    assert not np.array_equal(expect_records(a, 22, False, LONG), expect_records(b, 22, False, LONG))
    assert not np.array_equal(matrix("asymmetric"), matrix("asymmetric").T)
    # +-1,000: a score beyond int16
    th = window_table("mixed", "thousands", 3, 1)
    assert th.best[:N_LONG].max() > 32767
    # forms: with p = -1 the short targets' classes stay in the byte range and the long ones leave it
    peps, _, targets = INPUTS["u12"]()
    packed, literal = expect_forms(matrix("blosum62"), peps, targets, (0, len(peps)), (0, len(targets)), 3, -1, 21)
    assert packed > 0 and literal > 0
    # one result beyond the scratch's first size
    low = window_table("u12", "blosum62", 3, 0)
    assert (low.w >= LOW_THR).sum() > FIRST_HITS


# ---- GPU ------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def device_ctx(name, mname):
    peps, sizes, targets = INPUTS[name]()
    ctx = hammock_amd.Context(matrix(mname), device=0)
    ctx.set_sequences(peps, sizes=sizes)
    ctx.set_targets(targets)
    return ctx


def scan_sorted(ctx, qr, tr, X, p, thr, **kw):
    out = ctx.scan_shifted(*qr, *tr, X, p, thr, **kw)
    return (np.sort(out[0], order=["target", "offset", "query"]),) + tuple(out[1:])


def check_case(case, monkeypatch=None, coverage=True, tr=None):
    name, mname, qr, X, p, thr = case
    tb = window_table(name, mname, X, p)
    ctx = device_ctx(name, mname)
    qr = qr or (0, len(tb.peps))
    tr = tr or (0, len(tb.targets))
    forms = expect_forms(matrix(mname), tb.peps, tb.targets, qr, tr, X, p, thr)
    for all_windows in (False, True):
        want = expect_records(tb, thr, all_windows, qr, tr)
        got = scan_sorted(ctx, qr, tr, X, p, thr, all_windows=all_windows, coverage=coverage)
        stats = got[1]
        print(case_id(case), "all_windows" if all_windows else "pairs", len(want), "records;", stats.windows_packed, "packed,",
              stats.windows_literal, "literal windows;", f"{stats.kernel_ms:.3f} ms")
        assert np.array_equal(got[0], want)
        assert (stats.windows_packed, stats.windows_literal) == forms and stats.windows_scored == sum(forms)
        assert stats.n_hits == len(want) and stats.window_hits == len(expect_records(tb, thr, True, qr, tr))
        if coverage:
            cc, cs = expect_coverage(tb, want, tr)
            assert np.array_equal(got[2], cc) and np.array_equal(got[3], cs)
        if monkeypatch is not None:     # the literal form alone: the same records
            monkeypatch.setenv("HMK_NO_SCAN_PACKED", "1")
            try:
                lit = scan_sorted(ctx, qr, tr, X, p, thr, all_windows=all_windows)
            finally:
                monkeypatch.delenv("HMK_NO_SCAN_PACKED")
            assert np.array_equal(lit[0], want)
            assert (lit[1].windows_packed, lit[1].windows_literal) == (0, sum(forms))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES_MIXED, ids=case_id)
def test_mixed_lengths_on_the_boundary_targets(gpu, monkeypatch, case):
    check_case(case, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES_UNIFORM, ids=case_id)
def test_uniform_lengths_on_the_boundary_targets(gpu, monkeypatch, case):
    check_case(case, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES_MANY, ids=case_id)
def test_three_hundred_short_targets(gpu, monkeypatch, case):
    check_case(case, monkeypatch)


@pytest.mark.gpu
def test_ties_keep_the_smallest_offset_and_every_period_shows(gpu):
    ctx, tb = device_ctx("mixed", "blosum62"), window_table("mixed", "blosum62", 3, 0)
    top = int(tb.best[4, PERIODIC_T])
    pairs, _ = ctx.scan_shifted(4, 5, PERIODIC_T, PERIODIC_T + 1, 3, 0, top)
    assert [tuple(r) for r in pairs] == [(4, PERIODIC_T, top, 0)]
    wins, _ = scan_sorted(ctx, (4, 5), (PERIODIC_T, PERIODIC_T + 1), 3, 0, top, all_windows=True)
    assert [tuple(r) for r in wins] == [(4, PERIODIC_T, top, s) for s in (0, 12, 24, 36, 48)]


@pytest.mark.gpu
def test_both_forms_run_when_the_penalty_splits_the_classes(gpu):
    ctx, tb = device_ctx("u12", "blosum62"), window_table("u12", "blosum62", 3, -1)
    hits, stats = scan_sorted(ctx, (0, len(tb.peps)), (0, len(tb.targets)), 3, -1, 21)
    assert stats.windows_packed > 0 and stats.windows_literal > 0
    assert np.array_equal(hits, expect_records(tb, 21, False))


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [1, 3])
def test_work_loops_beyond_their_first_iteration(gpu, monkeypatch, capfd, cap):
    """under HMK_TEST_GRID_CAP every grid-stride kernel of k_scan.hip runs its later iterations: identical results"""
    ctx, tb = device_ctx("mixed", "blosum62"), window_table("mixed", "blosum62", 3, 0)
    thr, seen = 12, set()
    assert (tb.w[tb.q < N_LONG] >= thr).sum() > 6 * 256
    for all_windows in (False, True):
        want = expect_records(tb, thr, all_windows, LONG)
        monkeypatch.setenv("HMK_TEST_GRID_CAP", str(cap))
        capfd.readouterr()
        try:
            got = scan_sorted(ctx, LONG, (0, len(tb.targets)), 3, 0, thr, all_windows=all_windows, coverage=True)
        finally:
            monkeypatch.delenv("HMK_TEST_GRID_CAP")
        for kernel, wanted, launched in LINE.findall(capfd.readouterr().err):
            assert int(launched) == cap < int(wanted)
            seen.add(kernel)
        assert np.array_equal(got[0], want)
        cc, cs = expect_coverage(tb, want)
        assert np.array_equal(got[2], cc) and np.array_equal(got[3], cs)
    assert seen == GRID_KERNELS


@pytest.mark.gpu
def test_capacity_is_exact(gpu):
    ctx, tb = device_ctx("u12", "blosum62"), window_table("u12", "blosum62", 3, 0)
    for all_windows in (False, True):
        want = expect_records(tb, 20, all_windows)
        for cap in (0, len(want) - 1):
            st = N.ScanStats()
            buf = np.zeros(max(cap, 1), dtype=SCAN_HIT_DTYPE)
            rc = N.lib.hmk_scan_shifted(ctx._h, 0, len(tb.peps), 0, len(tb.targets), 3, 0, 20, int(all_windows),
                                        buf.ctypes.data_as(C.POINTER(N.ScanHit)), cap, None, None, C.byref(st))
            assert rc == N.HMK_ERR_CAPACITY and st.n_hits == len(want)
        with pytest.raises(BufferError):
            ctx.scan_shifted(0, len(tb.peps), 0, len(tb.targets), 3, 0, 20, all_windows=all_windows, capacity=len(want) - 1)
        got, _ = scan_sorted(ctx, (0, len(tb.peps)), (0, len(tb.targets)), 3, 0, 20, all_windows=all_windows, capacity=len(want))
        assert np.array_equal(got, want)


@pytest.mark.gpu
def test_a_result_beyond_the_scratchs_first_size(gpu):
    tb = window_table("u12", "blosum62", 3, 0)
    ctx = hammock_amd.Context(matrix("blosum62"), device=0)     # a fresh context: its scratch has the first size
    ctx.set_sequences(tb.peps, sizes=tb.sizes)
    ctx.set_targets(tb.targets)
    for all_windows in (True, False):
        want = expect_records(tb, LOW_THR, all_windows)
        got, stats = scan_sorted(ctx, (0, len(tb.peps)), (0, len(tb.targets)), 3, 0, LOW_THR, all_windows=all_windows)
        assert stats.window_hits > FIRST_HITS and np.array_equal(got, want)


@pytest.mark.gpu
def test_ranges_uploads_and_the_other_set(gpu):
    tb = window_table("mixed", "blosum62", 3, 0)
    peps, sizes, targets = tb.peps, tb.sizes, tb.targets
    nt = len(targets)
    ctx = hammock_amd.Context(matrix("blosum62"), device=0)
    ctx.set_targets(targets)                       # targets first, then the sequences
    ctx.set_sequences(peps, sizes=sizes)
    edges_before = np.sort(ctx.neighbors_shifted(0, 0, 20)[0])
    for qr, tr in (((3, 40), (0, nt)), (LONG, (5, 9)), ((10, 11), (nt - 4, nt)), ((0, 5), (11, 12))):
        for all_windows in (False, True):
            want = expect_records(tb, 20, all_windows, qr, tr)
            got = scan_sorted(ctx, qr, tr, 3, 0, 20, all_windows=all_windows, coverage=True)
            assert np.array_equal(got[0], want)
            cc, cs = expect_coverage(tb, want, tr)      # indexed from offsets[t0]
            assert np.array_equal(got[2], cc) and np.array_equal(got[3], cs)
    assert len(ctx.scan_shifted(5, 5, 0, nt, 3, 0, 20)[0]) == 0 and len(ctx.scan_shifted(0, 5, 2, 2, 3, 0, 20)[0]) == 0
    # a second and a third upload of targets: the scan sees the set of the last one
    ctx.set_targets(targets[5:9])
    want = expect_records(tb, 20, False, LONG, (5, 9))
    want["target"] -= 5
    assert np.array_equal(scan_sorted(ctx, LONG, (0, 4), 3, 0, 20)[0], np.sort(want, order=["target", "offset", "query"]))
    ctx.set_targets(targets)
    assert np.array_equal(scan_sorted(ctx, LONG, (0, nt), 3, 0, 20)[0], expect_records(tb, 20, False, LONG))
    # new sequences under the same targets
    ctx.set_sequences(peps[:N_LONG][::-1], sizes=sizes[:N_LONG][::-1])
    want = expect_records(tb, 20, True, LONG)
    want["query"] = N_LONG - 1 - want["query"]
    assert np.array_equal(scan_sorted(ctx, LONG, (0, nt), 3, 0, 20, all_windows=True)[0], np.sort(want, order=["target", "offset", "query"]))
    # an existing call is what it was before the targets came
    ctx.set_sequences(peps, sizes=sizes)
    assert np.array_equal(np.sort(ctx.neighbors_shifted(0, 0, 20)[0]), edges_before)
    plain = hammock_amd.Context(matrix("blosum62"), device=0)
    plain.set_sequences(peps, sizes=sizes)
    assert np.array_equal(np.sort(plain.neighbors_shifted(0, 0, 20)[0]), edges_before)


@pytest.mark.gpu
def test_sizes_reach_the_coverage_and_default_to_one(gpu):
    tb = window_table("u12", "blosum62", 3, 0)
    ctx = hammock_amd.Context(matrix("blosum62"), device=0)
    ctx.set_sequences(tb.peps)                     # no sizes: 1 each
    ctx.set_targets(tb.targets)
    _, _, cc, cs = ctx.scan_shifted(0, len(tb.peps), 0, len(tb.targets), 3, 0, 20, all_windows=True, coverage=True)
    assert np.array_equal(cc.astype(np.uint64), cs) and cc.any()
    _, _, cc2, cs2 = device_ctx("u12", "blosum62").scan_shifted(0, len(tb.peps), 0, len(tb.targets), 3, 0, 20, all_windows=True, coverage=True)
    assert np.array_equal(cc2, cc) and not np.array_equal(cs2, cs)
    assert np.array_equal(cs2, expect_coverage(tb, expect_records(tb, 20, True))[1])


@pytest.mark.gpu
def test_device_list_runs_on_the_root(gpu):
    tb = window_table("u12", "blosum62", 3, 0)
    ctx = hammock_amd.Context(matrix("blosum62"), device=[0, 0])
    ctx.set_sequences(tb.peps, sizes=tb.sizes)
    ctx.set_targets(tb.targets)
    assert np.array_equal(scan_sorted(ctx, (0, len(tb.peps)), (0, len(tb.targets)), 3, 0, 20)[0], expect_records(tb, 20, False))


# ---- the targets loader and the command line -------------------------------------------------------------------------------------

CLI = os.path.join(ROOT, "hammock_amd", "bin", "hammock-hip")
ALPHABET = "ARNDCQEGHILKMFPSTWYVBZX*"


def letters(a):
    return "".join(ALPHABET[int(c)] for c in a)


def test_targets_loader(tmp_path):
    import subprocess
    unit = "ACDEFGHIKLMNPQRSTVWY"
    fa = tmp_path / "t.fa"
    fa.write_text(f">sp|P1 first protein\n{unit}\n{unit.lower()}\n\n>two\tx\n{unit}{unit}\n>three\n{unit}\n{unit}BZX*\n")
    r = subprocess.run([CLI, "io-selftest", "targets", str(fa)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    # sequences span lines, names end at the first white space, equal records stay apart, all 24 letters
    assert r.stdout.splitlines() == [f"sp|P1\t40\t{unit}{unit}", f"two\t40\t{unit}{unit}", f"three\t44\t{unit}{unit}BZX*"]
    fa.write_text(f">fine\n{unit}{unit}\n>short one\n{unit}{unit[:12]}\n")
    r = subprocess.run([CLI, "io-selftest", "targets", str(fa)], capture_output=True, text=True)
    assert r.returncode != 0 and '"short"' in r.stderr and "32 residues" in r.stderr and "search" in r.stderr
    r = subprocess.run([CLI, "scan", "-i", os.path.join(GOLDEN, "musi.fa"), "--targets", str(fa), "-d", str(tmp_path / "out")],
                       capture_output=True, text=True)
    assert r.returncode == 3 and '"short"' in r.stderr      # the run stops at the file, before it asks for the device
    fa.write_text(f">bad\n{unit}J{unit}\n")
    r = subprocess.run([CLI, "io-selftest", "targets", str(fa)], capture_output=True, text=True)
    assert r.returncode != 0 and "'J'" in r.stderr and '"bad"' in r.stderr


def test_cli_scan_arguments_and_usage(tmp_path):
    import subprocess
    fa = os.path.join(GOLDEN, "musi.fa")
    r = subprocess.run([CLI, "scan", "-i", fa, "-d", str(tmp_path / "a")], capture_output=True, text=True)
    assert r.returncode == 2 and "--targets" in r.stderr
    r = subprocess.run([CLI, "scan", "-i", fa, "--targets", fa, "-d", str(tmp_path / "b"), "--devices", "0,1"], capture_output=True, text=True)
    assert r.returncode == 2 and "--devices is not available in mode scan" in r.stderr
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "hammock-hip scan -i" in r.stderr and "--targets <file>" in r.stderr and "--all_windows" in r.stderr


def test_the_host_code_under_the_sanitizers(tmp_path):
    """the targets loader and the planner's class rule in a stand-alone program (its own main, nothing loaded into this process),
    built with AddressSanitizer and UndefinedBehaviorSanitizer for the CPU"""
    import subprocess
    exe = str(tmp_path / "scan_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "tools", "scan_host_check.cpp"), "-o", exe])
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and "scan host check ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_cli_scan_files_match_the_definition(gpu, tmp_path):
    import subprocess
    rng = np.random.default_rng(21)
    b12, b12b = bases()[12], base12b()
    peps = [b12, b12b] + random_peptides(rng, 6, 12, 12)
    counts = [3, 1, 2, 1, 1, 1, 1, 1]
    T = edge_targets()
    targets = [T[SUFFIX_T], T[PERIODIC_T], T[4], rng.integers(0, 20, size=50, dtype=np.uint8), T[PREFIX_T]]
    names = ["suffix", "periodic", "sixtyfive", "nothing", "prefix"]
    pfa, tfa = tmp_path / "peptides.fa", tmp_path / "targets.fa"
    pfa.write_text("".join(f">{k}_{c}\n{letters(p)}\n" for k, (p, n) in enumerate(zip(peps, counts)) for c in range(n)))
    tfa.write_text("".join(f">{name} some description\n{letters(t[:30])}\n{letters(t[30:])}\n" for name, t in zip(names, targets)))
    tb = make_table(peps, np.asarray(counts), targets, matrix("blosum62"), 3, 0)
    for mode, extra in (("pairs", []), ("windows", ["--all_windows"])):
        outs = []
        for run in range(2):
            out = tmp_path / f"{mode}{run}"
            r = subprocess.run([CLI, "scan", "-i", str(pfa), "--targets", str(tfa), "-d", str(out), "-g", "20"] + extra,
                               capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, r.stderr
            assert "Max shift not set. Setting automatically to: 3" in r.stderr and "Gap penalty not set. Setting automatically to: 0" in r.stderr
            outs.append({f: (out / f).read_bytes() for f in ("scan_hits.tsv", "target_coverage.tsv", "target_summary.tsv")})
            log = (out / "run.log").read_text()
            assert 'Program started in mode "scan".' in log and "Program successfully ended." in log and "Windows scored: " in log
        assert outs[0] == outs[1]                                  # two runs, the same bytes
        want = expect_records(tb, 20, mode == "windows")           # sorted by (target, offset, peptide)
        rows = [l.split("\t") for l in outs[0]["scan_hits.tsv"].decode().splitlines()]
        assert rows[0] == ["peptide", "count", "target", "start", "score", "segment"]
        expect_rows = []
        for r in want:
            pep, t, s = peps[r["query"]], targets[r["target"]], int(r["offset"])
            seg = "".join(ALPHABET[t[s + i]] if 0 <= s + i < len(t) else "-" for i in range(len(pep)))
            expect_rows.append([letters(pep), str(counts[r["query"]]), names[r["target"]], str(s + 1), str(r["score"]), seg])
        assert rows[1:] == expect_rows
        assert [letters(b12), "3", "suffix", "-2", str(tb.best[0, 0]), "---" + letters(b12[3:])] in rows      # the overhang's marks
        assert [letters(b12), "3", "prefix", str(len(targets[4]) - 9 + 1), str(tb.best[0, 4]), letters(b12[:9]) + "---"] in rows
        cc, cs = expect_coverage(tb, want)
        off = np.concatenate([[0], np.cumsum([len(t) for t in targets])])
        hit_targets = sorted(set(int(r["target"]) for r in want))
        assert 3 not in hit_targets
        cov = ["target\tposition\tresidue\thits\tcount"]
        for t in hit_targets:
            cov += [f"{names[t]}\t{k + 1}\t{ALPHABET[targets[t][k]]}\t{cc[off[t] + k]}\t{cs[off[t] + k]}" for k in range(len(targets[t]))]
        assert outs[0]["target_coverage.tsv"].decode().splitlines() == cov
        summ = ["target\tlength\thits\tpeptides\tbest_score\tcovered_positions"]
        for t in range(len(targets)):
            mine = want[want["target"] == t]
            best = str(mine["score"].max()) if len(mine) else "NA"
            summ.append(f"{names[t]}\t{len(targets[t])}\t{len(mine)}\t{len(set(mine['query']))}\t{best}\t{int((cc[off[t]:off[t + 1]] > 0).sum())}")
        assert outs[0]["target_summary.tsv"].decode().splitlines() == summ
