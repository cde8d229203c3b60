"""Cluster profiles: hmk_cluster_profile (k_profile.hip) and `hammock-hip profile`.

The expectation is never the code under test: `definition` below restates the Java the header cites -- FileIOManager
getPositionLetterCounts (:1221-1247), getInformationContents / getInformationContent (:1195-1211, :1421-1439), defineMatchStates
(:1265-1300), checkConservedStates (:1172-1181); Statistics getPeptideKld / getCorrectedFrequencies (:238-300), getMeanClusterKld /
getMeanSystemKld (:178-197) -- in plain Python floats over rows it builds itself from `column`.  Sums over symbols run in symbol
order, over columns left to right, over members in index order.  It is computed once per input and parameter set.

Integer outputs (width, col_start, counts, flags, n_conserved, n_match, passes, omitted) are compared exactly.

Tolerance of ic and the KLDs: absolute, derived, u = 2^-53 (half an ulp of 1).  The device library documents log in double at 1 ulp
(2u relative), and so does the host's libm for math.log.
  ic    a column has at most 20 terms t = p * (log(p) / log(2)).  p = c / n carries u; through log that is an absolute u in log(p),
        i.e. at most u p / ln 2 < 1.45 u p per term and 1.45 u in all (the p add up to 1).  log(p): 2u; log(2): 2u; the division
        and the product: u each -- 6u |t|.  At most 20 additions into a partial sum no larger than T = the sum of |t|: 20 u T.  The
        constant log(0.05) / log(2) = 4.33 carries 2u + 2u + u, the last addition one more u of at most 4.33: 5 * 4.33 u < 22 u.
        One side: (26 T + 1.45 + 22) u; both sides round, so tol_ic = 2 (26 T + 24) u.  T <= log2 20: tol_ic <= 6.1e-14.
  KLD   a member has at most 32 columns with a term t = log(Q / b) * (s / (s + sigma)) * scale.  g is a 20-term dot product of
        positive numbers: u for fj, u for the product, 20u for the additions: 22u relative.  fi: u.  (s - 1) fi, beta g: u each,
        their sum u, the division u (the denominator is an exact integer), Q / b: u -- the argument of log carries at most 28u
        relative, an absolute 28u in the logarithm, times s / (s + sigma) * scale < scale: 28 scale u per column.  log: 2u;
        s / (s + sigma): 2u; two products: 2u -- 6u |t|.  At most 32 additions into a partial sum no larger than T = the sum of
        |t|: 32 u T.  One side: (38 T + 32 * 28 scale) u; tol_kld = 2 (38 T + 896 scale) u.  With T <= 300 and scale = 2.88539
        that is 3.1e-12.
  means a mean of n KLDs inherits the largest tol_kld of its members, and its own n additions and one division add at most
        (n + 1) u times the mean of |KLD| on each side: tol_mean = max tol_kld + 2 (n + 1) u mean|KLD|.
test_the_tolerances_stay_far_below_1e_9 asserts on the reference alone that no input gets more than 1e-9.

What makes the flags comparable: on the reference alone, every column of every compared input has |ic - min_ic| >= 1e-9
(test_the_inputs_hold_what_the_gpu_tests_claim).  The tie column of ten members (ic = 1.2 exactly, the default min_ic) is tested
apart and only for consistency.
"""
import ctypes as C
import functools
import math
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN
from test_assign import gpu   # noqa: F401  (the fixture that skips where no HIP device is visible)
from test_align import window_family
from test_linkage import _blosum62, _musi, device_ctx

import hammock_amd
from hammock_amd import _native as N

U = 2.0 ** -53
SCALE, BETA, SIGMA = 2.88539, 200.0, 10.0
LETTERS = hammock_amd.AMINO_ACIDS
GRID_LINE = re.compile(r"^\[hmk grid\] (\S+) (\d+) -> (\d+)$", re.M)
LARGE_MIN, CHUNK = 8, 1024   # PROFILE_LARGE_MIN, PROFILE_CHUNK (hmk_profile.h)
KERNELS = ("k_profile_init", "k_profile_counts_small", "k_profile_counts_large", "k_profile_columns", "k_profile_match", "k_profile_kld")
MOTIF_SIZES = [1, 2, 3, 5, 10, 10, 17, 64, 65, 257, 700, 3000,
               CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1, 255, 256, 513]
MOTIF_SIZES += [4, 6, 7, 8, 9, 11, 12, 13] * 3   # the sizes around the small/large boundary; columns for more than two blocks of the kernels
                                                 # that take a lane per column
MOTIF_SEED = 32   # most seeds put a tie (ten members: ic = 1.2 exactly) into a uniform column of a small slot; this one has 0.026 of room
FREQ_FILE = os.path.join(GOLDEN, "blosum62.freq_rownorm")


@functools.lru_cache(maxsize=None)
def frequency():
    f, letters = hammock_amd.load_frequency_matrix(FREQ_FILE)
    f.setflags(write=False)
    return f


def skewed_background():
    """a non-uniform background made here: proportional to 1 + (7 k mod 20), normalised"""
    b = np.array([1.0 + (7 * k) % 20 for k in range(20)])
    return b / b.sum()


# ---- the definition ----------------------------------------------------------------------------------------------------------

def definition(peps, mc, ncl, column, freq, bg, min_ic=1.2, max_gap=0.2, min_cons=0, allow=False, beta=BETA, sigma=SIGMA, scale=SCALE):
    """the outputs of hmk_cluster_profile from the Java lines, in plain floats -> dict; also the tolerances and what the inputs test
    counts (negative KLDs, columns skipped as only gaps, letters whose count falls to 0)"""
    nm = len(peps)
    mc = np.asarray(mc, dtype=np.int64)
    column = np.asarray(column, dtype=np.int64)
    lens = np.array([len(q) for q in peps], dtype=np.int64)
    width = np.zeros(ncl, dtype=np.int64)
    np.maximum.at(width, mc, column + lens)
    col_start = np.concatenate([[0], np.cumsum(width)])
    ncols = int(col_start[-1])
    size = np.bincount(mc, minlength=ncl)
    # rows: symbol per (member, slot column), the gap is 20
    counts = np.zeros((ncols, 21), dtype=np.int64)
    for k in range(nm):
        base = int(col_start[mc[k]])
        w = int(width[mc[k]])
        row = np.full(w, 20, dtype=np.int64)
        row[column[k]:column[k] + lens[k]] = peps[k]
        np.add.at(counts, (np.arange(base, base + w), row), 1)
    log2 = math.log(2)
    ic = np.zeros(ncols)
    ic_T = np.zeros(ncols)
    flags = np.zeros(ncols, dtype=np.int64)
    n_cons = np.zeros(ncl, dtype=np.int64)
    n_match = np.zeros(ncl, dtype=np.int64)
    for c in range(ncl):
        a, b = int(col_start[c]), int(col_start[c + 1])
        for g in range(a, b):
            gaps = int(counts[g, 20])
            if (gaps + 0.0) / int(size[c]) <= max_gap:                                 # FileIOManager.java:1204
                n = int(size[c]) - gaps
                ent = 0.0
                for s in range(20):
                    if counts[g, s]:
                        p = (int(counts[g, s]) + 0.0) / n                              # :1431
                        t = p * (math.log(p) / log2)                                   # :1436
                        ent += t
                        ic_T[g] += abs(t)
                ic[g] = -(math.log(0.05) / log2) + ent                                 # :1438
            else:
                ic[g] = -1.0                                                           # :1207
        cons = ic[a:b] >= min_ic                                                       # :1271, :1281
        n_cons[c] = int(cons.sum())
        if allow or not cons.any():
            match = cons
        else:
            at = np.flatnonzero(cons)
            match = np.zeros(b - a, dtype=bool)
            match[at[0]:at[-1] + 1] = True                                             # :1277-1297
        n_match[c] = int(match.sum())
        flags[a:b] = cons.astype(np.int64) + 2 * match.astype(np.int64)
    # a member's term in a column depends on the column and on the member's letter alone: one evaluation per (column, letter)
    term = {}
    only_gaps = zero_count = 0
    kld_all = np.zeros(nm)
    kld_match = np.zeros(nm)
    kld_T = np.zeros(nm)
    for k in range(nm):
        c = int(mc[k])
        if size[c] < 2:
            continue                                                                   # Hammock.java:684-692: left out, 0.0 here
        all_, match_ = 0.0, 0.0
        for j in range(int(lens[k])):
            g = int(col_start[c]) + int(column[k]) + j
            aa = int(peps[k][j])
            if (g, aa) not in term:
                cnt = [int(v) for v in counts[g]]
                cnt[aa] -= 1                                                           # Statistics.java:254
                s = float(sum(cnt))                                                    # :258-261
                if s == cnt[20]:                                                       # :262
                    term[g, aa] = None
                else:
                    gi = 0.0
                    for x in range(20):                                                # :283-289
                        fj = (cnt[x] + 0.0) / s
                        gi += fj * float(freq[x, aa])
                    fi = (cnt[aa] + 0.0) / s                                           # :292
                    Q = (((s - 1) * fi) + (beta * gi)) / ((s - 1) + beta)              # :296
                    t = math.log(Q / float(bg[aa])) * (s / (s + sigma))                # :267
                    term[g, aa] = (t * scale, cnt[aa] == 0)                            # :268
            t = term[g, aa]
            if t is None:
                only_gaps += 1
                continue
            zero_count += t[1]
            all_ += t[0]                                                               # :269
            kld_T[k] += abs(t[0])
            if flags[g] & 2:
                match_ += t[0]
        kld_all[k], kld_match[k] = all_, match_
    mean_match = np.zeros(ncl)
    mean_all = np.zeros(ncl)
    sys_match = sys_all = 0.0
    sys_n = 0
    for k in range(nm):                                                                # member index order
        mean_match[mc[k]] += kld_match[k]
        mean_all[mc[k]] += kld_all[k]
        if size[mc[k]] >= 2:
            sys_match += kld_match[k]
            sys_all += kld_all[k]
            sys_n += 1
    for c in range(ncl):
        mean_match[c] /= (int(size[c]) + 0.0)
        mean_all[c] /= (int(size[c]) + 0.0)
    tol_ic = 2 * (26 * ic_T + 24) * U
    tol_kld = 2 * (38 * kld_T + 896 * scale) * U
    tol_mean = np.array([tol_kld[mc == c].max() + 2 * (size[c] + 1) * U * np.abs(kld_all[mc == c]).mean() for c in range(ncl)])
    multi = size[mc] >= 2
    tol_sys = (tol_kld.max() + 2 * (sys_n + 1) * U * np.abs(kld_all[multi]).mean()) if sys_n else 0.0
    return dict(width=width, col_start=col_start, counts=counts, ic=ic, flags=flags, n_conserved=n_cons, n_match=n_match,
                passes=(n_cons >= min_cons).astype(np.int64), kld_all=kld_all, kld_match=kld_match, mean_match=mean_match, mean_all=mean_all,
                sys_match=sys_match / (sys_n + 0.0) if sys_n else math.nan, sys_all=sys_all / (sys_n + 0.0) if sys_n else math.nan,
                omitted=int((size == 1).sum()), n_multi=int((size >= 2).sum()), size=size,
                tol_ic=tol_ic, tol_kld=tol_kld, tol_mean=tol_mean, tol_sys=tol_sys,
                only_gaps=only_gaps, zero_count=int(zero_count), min_ic=min_ic)


# ---- inputs ------------------------------------------------------------------------------------------------------------------

def motif_family(seed, sizes=MOTIF_SIZES):
    """per slot a 14-position parent whose positions are, mixed, 95 % one letter, two letters at 50/50, or uniform over 20; members
    are windows of 9-12 residues at offsets 0-2, all distinct, shuffled so that no slot is contiguous.  The slot of 5 has exactly
    one member at offset 1 and the two slots of 10 exactly two and three, the others of those slots at offset 0: gap proportions
    of 0.2, 0.2 and 0.3 in column 0 -> (peptides, member_cluster, n_clusters, column)"""
    rng = np.random.default_rng(77_000 + seed)
    peps, mc, col, seen = [], [], [], set()
    tens = 0
    for c, size in enumerate(sizes):
        kinds = np.array([0, 0, 0, 0, 0, 1, 1, 1, 2, 2, 2, 2, 2, 2])
        rng.shuffle(kinds)
        lead = rng.integers(0, 20, size=14)
        other = (lead + rng.integers(1, 20, size=14)) % 20
        forced = None
        if size == 5:
            forced = [1] + [0] * 4
        elif size == 10:
            tens += 1
            forced = [1] * (1 + tens) + [0] * (9 - tens)
        added = 0
        while added < size:
            draw = rng.integers(0, 20, size=14)
            coin = rng.random(14)
            parent = np.where(kinds == 0, np.where(coin < 0.95, lead, draw), np.where(kinds == 1, np.where(coin < 0.5, lead, other), draw))
            offset = forced[added] if forced else int(rng.integers(0, 3))
            length = int(rng.integers(9, 13))
            q = parent[offset:offset + length].astype(np.uint8)
            if q.tobytes() in seen:
                continue
            seen.add(q.tobytes())
            peps.append(q)
            mc.append(c)
            col.append(offset)
            added += 1
    perm = rng.permutation(len(peps))
    return ([peps[k] for k in perm], np.asarray(mc, dtype=np.uint32)[perm], len(sizes), np.asarray(col, dtype=np.uint32)[perm])


TIE = [0, 0, 1, 2, 3, 4, 5, 6, 7, 8]   # one letter twice, eight letters once: ic = 1.2 exactly


def tie_family():
    """ten members of 9 residues at column 0; column 0 is the tie, the even columns behind it hold one letter and the odd ones two
    letters five times each (uniform draws would tie again: ten members do that often); and a slot of three beside it"""
    rng = np.random.default_rng(77_900)
    peps = []
    for k in range(10):
        q = np.array([TIE[k]] + [j + (k % 2 if j % 2 else 0) for j in range(1, 9)], dtype=np.uint8)
        peps.append(q)
    peps += [rng.integers(0, 20, size=9).astype(np.uint8) for _ in range(3)]
    return peps, np.array([0] * 10 + [1] * 3, dtype=np.uint32), 2, np.zeros(13, dtype=np.uint32)


PARAM_SETS = {
    "inner0": dict(),
    "inner1": dict(allow=True, min_cons=4),
    "skewed": dict(bg="skewed"),
    "ic25": dict(min_ic=2.5, min_cons=3),   # (not 2.0: five distinct letters in the slot of 5 have log2 20 - log2 5 = 2.0 exactly)
}


@functools.lru_cache(maxsize=None)
def motif_input():
    peps, mc, ncl, col = motif_family(MOTIF_SEED)
    res, off = hammock_amd.pack_sequences(peps)
    for arr in (res, off, mc, col):
        arr.setflags(write=False)
    return peps, mc, ncl, col, res, off


@functools.lru_cache(maxsize=None)
def motif_want(pset):
    peps, mc, ncl, col, _, _ = motif_input()
    kw = dict(PARAM_SETS[pset])
    bg = skewed_background() if kw.pop("bg", None) else np.full(20, 0.05)
    return definition(peps, mc, ncl, col, frequency(), bg, **kw)


def params_of(pset):
    kw = dict(PARAM_SETS[pset])
    bg = skewed_background() if kw.pop("bg", None) else None
    return hammock_amd.profile_params(frequency(), bg, min_ic=kw.get("min_ic", 1.2), min_conserved_positions=kw.get("min_cons", 0),
                                      allow_inner_gaps=kw.get("allow", False))


def compare(R, want, what=""):
    """a ProfileResult against the definition: integers exactly, doubles within the derived tolerances"""
    for name in ("width", "n_conserved", "n_match", "passes", "col_start"):
        assert np.array_equal(np.asarray(getattr(R, name), dtype=np.int64), want[name]), (what, name)
    if R.counts is not None:
        assert R.counts.dtype == np.uint32 and np.array_equal(R.counts.astype(np.int64), want["counts"]), (what, "counts")
    if R.col_flags is not None:
        assert np.array_equal(R.col_flags.astype(np.int64), want["flags"]), (what, "col_flags")
    if R.ic is not None:
        assert (np.abs(R.ic - want["ic"]) <= want["tol_ic"]).all(), (what, "ic", float(np.abs(R.ic - want["ic"]).max()))
        assert np.array_equal(R.ic == -1.0, want["ic"] == -1.0), (what, "ic = -1")
    for name in ("kld_all", "kld_match"):
        d = np.abs(getattr(R, name) - want[name])
        assert (d <= want["tol_kld"]).all(), (what, name, float(d.max()))
    assert (np.abs(R.kld_match_mean - want["mean_match"]) <= want["tol_mean"]).all(), (what, "kld_match_mean")
    assert (np.abs(R.kld_all_mean - want["mean_all"]) <= want["tol_mean"]).all(), (what, "kld_all_mean")
    s = R.stats
    assert (s.columns, s.n_multi, s.omitted) == (int(want["col_start"][-1]), want["n_multi"], want["omitted"]), what
    if want["n_multi"]:
        assert abs(s.system_kld_match - want["sys_match"]) <= want["tol_sys"] and abs(s.system_kld_all - want["sys_all"]) <= want["tol_sys"], what
    else:
        assert math.isnan(s.system_kld_match) and math.isnan(s.system_kld_all), what


def consistent(R, mc, min_ic, min_cons, allow):
    """what follows from the device's own decision, exactly: flags from the returned ic, the counts of the bits, passes, the means
    from the returned KLDs summed in member index order"""
    ncl = R.width.size
    cons = R.ic >= min_ic
    assert np.array_equal(R.col_flags & 1, cons.astype(np.uint8))
    for c in range(ncl):
        a, b = int(R.col_start[c]), int(R.col_start[c + 1])
        assert b - a == R.width[c]
        at = np.flatnonzero(cons[a:b])
        match = cons[a:b].copy()
        if not allow and at.size:
            match[at[0]:at[-1] + 1] = True
        assert np.array_equal((R.col_flags[a:b] >> 1) & 1, match.astype(np.uint8)), c
        assert (R.n_conserved[c], R.n_match[c], R.passes[c]) == (at.size, int(match.sum()), int(at.size >= min_cons)), c
    assert np.array_equal(R.counts.sum(axis=1), np.bincount(mc, minlength=ncl)[np.repeat(np.arange(ncl), R.width)])
    size = np.bincount(mc, minlength=ncl)
    sums = np.zeros((2, ncl))
    sys_ = [0.0, 0.0]
    n = 0
    for k in range(mc.size):
        sums[0, mc[k]] += R.kld_match[k]
        sums[1, mc[k]] += R.kld_all[k]
        if size[mc[k]] >= 2:
            sys_[0] += R.kld_match[k]
            sys_[1] += R.kld_all[k]
            n += 1
    assert np.array_equal(sums[0] / size, R.kld_match_mean) and np.array_equal(sums[1] / size, R.kld_all_mean)
    if n:
        assert (sys_[0] / n, sys_[1] / n) == (R.stats.system_kld_match, R.stats.system_kld_all)


def identical(A, B):
    for name in hammock_amd.ProfileResult.__slots__[:-1]:
        x, y = getattr(A, name), getattr(B, name)
        assert (x is None and y is None) or (x.dtype == y.dtype and x.tobytes() == y.tobytes()), name
    assert (A.stats.system_kld_match, A.stats.system_kld_all) == (B.stats.system_kld_match, B.stats.system_kld_all) or \
        (math.isnan(A.stats.system_kld_match) and math.isnan(B.stats.system_kld_match))


# ---- CPU: the symbol, the loader, the definition, the inputs, the checks -----------------------------------------------------

def test_symbol_is_declared_bound_and_exported():
    with open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "hammock_hip.h")) as fh:
        header = fh.read()
    assert "int hmk_cluster_profile(hmk_ctx *ctx" in header and "} hmk_profile_stats;" in header and "} hmk_profile_params;" in header
    assert "#define HMK_PROFILE_SYMBOLS 21" in header and "#define HMK_PROFILE_MAX_WIDTH 96" in header
    assert "hmk_cluster_profile" in N.SYMBOLS and hasattr(N.lib, "hmk_cluster_profile")
    assert N.lib.hmk_abi_version() == 4
    assert C.sizeof(N.ProfileParams) == 16 + 8 + 24 + 3200 + 160 and C.sizeof(N.ProfileStats) == 56
    assert (N.HMK_PROFILE_SYMBOLS, N.HMK_PROFILE_MAX_WIDTH) == (21, 96)


def test_frequency_file_loader(tmp_path):
    f, letters = hammock_amd.load_frequency_matrix(FREQ_FILE)
    assert letters == LETTERS[:20] and f.shape == (20, 20) and f.dtype == np.float64
    # the file's rows, read here on their own
    rows = [ln.split("\t") for ln in open(FREQ_FILE).read().splitlines() if not ln.startswith("#")]
    assert rows[0] == list(LETTERS[:20]) and len(rows) == 21
    assert all(f[j, i] == float(rows[1 + j][i]) for j in range(20) for i in range(20))
    assert (f[0, 0], f[0, 1], f[1, 0], f[19, 19], f[4, 4]) == (0.2901, 0.0310, 0.0446, 0.2689, 0.4837)   # row j, column i: not transposed
    assert np.abs(f.sum(axis=1) - 1).max() < 2e-3 and (f > 0).all()   # row-normalised, to the file's four digits
    # another letter order lands in the alphabet's order
    order = list(range(19, -1, -1))
    text = "# reversed\n" + "\t".join(LETTERS[k] for k in order) + "\n"
    text += "".join("\t".join(repr(float(f[j, i])) for i in order) + "\n" for j in order)
    (tmp_path / "rev.freq").write_text(text)
    g, rev = hammock_amd.load_frequency_matrix(str(tmp_path / "rev.freq"))
    assert rev == LETTERS[:20][::-1] and np.array_equal(g, f)
    (tmp_path / "bg").write_text("# one line\n" + " ".join(str(k + 1) for k in range(20)) + "\n")
    b = hammock_amd.load_background(str(tmp_path / "bg"), rev)
    assert np.array_equal(b, np.arange(20, 0, -1, dtype=np.float64))
    for name, bad in (("short", text.rsplit("\n", 2)[0] + "\n"), ("letters", text.replace("\tA\n", "\tB\n", 1)), ("word", text.replace("0.2901", "x"))):
        (tmp_path / name).write_text(bad)
        with pytest.raises(hammock_amd.FileFormatException):
            hammock_amd.load_frequency_matrix(str(tmp_path / name))
    (tmp_path / "bg2").write_text("1 2 3\n")
    with pytest.raises(hammock_amd.FileFormatException):
        hammock_amd.load_background(str(tmp_path / "bg2"))


def test_the_definition_against_hand_derived_values():
    """Hand derivations, in the style of tests/golden/hand_traces.md.  F = the frequency file, F[row j][column i]; uniform
    background b = 0.05; beta = 200, sigma = 10, scale = 2.88539.

    The tie column.  Ten rows, letter A twice and R N D C Q E G H once: p = 0.2 once and 0.1 eight times.
        ic = log2 20 + 0.2 log2 0.2 + 0.8 log2 0.1 = (2 + log2 5) - 0.2 log2 5 - 0.8 (1 + log2 5) = 2 - 0.8 = 1.2

    A slot of two, rows AC and AD (both at column 0).  Width 2; counts: column 0 {A: 2}, column 1 {C: 1, D: 1}; no gaps; ic of
    column 0 = log2 20 + 1 log2 1 = log2 20, of column 1 = log2 20 + 2 (0.5 log2 0.5) = log2 20 - 1 = log2 10.  Both >= 1.2.
      row AC, column 0: take A out: {A: 1}, sum = 1.  g = (1 / 1) F[A][A] = 0.2901, fi = 1, sum - 1 = 0:
                        Q = (0 * 1 + 200 * 0.2901) / (0 + 200) = 0.2901; term = ln(0.2901 / 0.05) * (1 / 11) * scale
              column 1: take C out: {C: 0, D: 1}, sum = 1.  g = F[D][C] = 0.0075, fi = 0:
                        Q = 0.0075; term = ln(0.0075 / 0.05) * (1 / 11) * scale        (negative: C lives on the pseudocount alone)
      row AD, column 1: g = F[C][D] = 0.0163; term = ln(0.0163 / 0.05) * (1 / 11) * scale

    A slot of three, rows A, A and -R (R at column 1).  Width 2; column 0 {A: 2, gap: 1}, column 1 {R: 1, gap: 2}.  Gap
    proportions 1/3 and 2/3 > 0.2: both ic = -1, no conserved column, no match state: kld_match = 0 for all three.
      row A (either), column 0: take A out: {A: 1, gap: 1}, sum = 2 (the gap stays inside sum).  g = (1 / 2) F[A][A] = 0.14505,
                        fi = 1 / 2, sum - 1 = 1: Q = (1 * 0.5 + 200 * 0.14505) / (1 + 200) = 29.51 / 201
                        term = ln((29.51 / 201) / 0.05) * (2 / 12) * scale;  column 1 is a gap of this row: nothing
      row -R, column 0: a gap of this row: nothing;  column 1: take R out: {R: 0, gap: 2}: only gaps remain: nothing.  KLD = 0.
    """
    F = frequency()
    A, R_, D, C_ = 0, 1, 3, 4
    assert (F[A, A], F[D, C_], F[C_, D]) == (0.2901, 0.0075, 0.0163)
    w = definition([np.array([TIE[k]], dtype=np.uint8) for k in range(10)], np.zeros(10, int), 1, np.zeros(10, int), F, np.full(20, 0.05))
    assert abs(w["ic"][0] - 1.2) <= 1e-15 and w["counts"][0].tolist() == [2] + [1] * 8 + [0] * 12
    peps = [np.array(q, dtype=np.uint8) for q in ([A, C_], [A, D], [A], [A], [R_])]
    w = definition(peps, [0, 0, 1, 1, 1], 2, [0, 0, 0, 0, 1], F, np.full(20, 0.05))
    assert w["width"].tolist() == [2, 2] and w["col_start"].tolist() == [0, 2, 4]
    assert w["counts"][:, [A, R_, D, C_, 20]].tolist() == [[2, 0, 0, 0, 0], [0, 0, 1, 1, 0], [2, 0, 0, 0, 1], [0, 1, 0, 0, 2]]
    assert abs(w["ic"][0] - math.log2(20)) < 1e-14 and abs(w["ic"][1] - math.log2(10)) < 1e-14 and w["ic"][2:].tolist() == [-1.0, -1.0]
    assert w["flags"].tolist() == [3, 3, 0, 0] and w["n_conserved"].tolist() == [2, 0] and w["n_match"].tolist() == [2, 0]
    k = SCALE / 11
    ac = math.log(0.2901 / 0.05) * k + math.log(0.0075 / 0.05) * k
    ad = math.log(0.2901 / 0.05) * k + math.log(0.0163 / 0.05) * k
    a3 = math.log((29.51 / 201) / 0.05) * (2 / 12) * SCALE
    assert np.abs(w["kld_all"] - [ac, ad, a3, a3, 0.0]).max() < 1e-14
    assert np.abs(w["kld_match"] - [ac, ad, 0.0, 0.0, 0.0]).max() < 1e-14
    assert math.log(0.0075 / 0.05) < 0 and w["only_gaps"] == 1 and w["zero_count"] == 2
    assert abs(w["mean_all"][1] - 2 * a3 / 3) < 1e-14 and abs(w["sys_all"] - (ac + ad + 2 * a3) / 5) < 1e-14 and w["omitted"] == 0


def test_the_inputs_hold_what_the_gpu_tests_claim():
    """the reference's side alone (it passes before the call exists): no GPU test below can pass vacuously"""
    peps, mc, ncl, col, res, off = motif_input()
    size = np.bincount(mc, minlength=ncl)
    assert size.tolist() == MOTIF_SIZES and mc.size == sum(MOTIF_SIZES) == 10489 and 512 < int(motif_want("inner0")["col_start"][-1]) < 768
    assert len({q.tobytes() for q in peps}) == mc.size
    assert {LARGE_MIN - 1, LARGE_MIN, LARGE_MIN + 1, 2 * LARGE_MIN + 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1} <= set(MOTIF_SIZES)
    assert all(np.ptp(np.flatnonzero(mc == c)) + 1 > size[c] for c in range(ncl) if size[c] > 1)   # no slot is contiguous
    w0, w1 = motif_want("inner0"), motif_want("inner1")
    for pset in PARAM_SETS:   # what makes the flags comparable
        w = motif_want(pset)
        assert np.abs(w["ic"] - w["min_ic"]).min() >= 1e-9, pset
    # the three gap cases: 1 of 5 and 2 of 10 pass at 0.2, 3 of 10 do not
    c5, (c10a, c10b) = MOTIF_SIZES.index(5), np.flatnonzero(size == 10)
    first = lambda c: int(w0["col_start"][c])   # noqa: E731
    assert [int(w0["counts"][first(c), 20]) for c in (c5, c10a, c10b)] == [1, 2, 3]
    assert w0["ic"][first(c5)] > 0 and w0["ic"][first(c10a)] > 0 and w0["ic"][first(c10b)] == -1.0
    assert (w0["ic"] == -1.0).sum() >= 20
    # the inner-gap rule changes the match states of some slots, and never the conserved columns
    changed = np.flatnonzero(w0["n_match"] != w1["n_match"])
    assert changed.size >= 6 and np.array_equal(w0["n_conserved"], w1["n_conserved"])
    assert not np.array_equal(w0["kld_match"], w1["kld_match"])
    assert (w0["passes"] == 1).all() and 0 < w1["passes"].sum() < ncl
    assert (w0["kld_all"] < 0).sum() >= 3 and w0["only_gaps"] >= 5 and w0["zero_count"] >= 300
    assert w0["omitted"] == 1 and w0["n_multi"] == ncl - 1
    assert not np.array_equal(motif_want("skewed")["kld_all"], w0["kld_all"]) and np.array_equal(motif_want("skewed")["ic"], w0["ic"])
    assert (motif_want("ic25")["flags"] != w0["flags"]).sum() >= 10
    # the tie family: the reference lands within rounding of 1.2, on whichever side
    peps, tmc, tncl, tcol = tie_family()
    w = definition(peps, tmc, tncl, tcol, frequency(), np.full(20, 0.05))
    assert abs(w["ic"][0] - 1.2) <= 1e-15 and np.abs(w["ic"][1:] - 1.2).min() > 1e-3


def test_the_tolerances_stay_far_below_1e_9():
    for pset in PARAM_SETS:
        w = motif_want(pset)
        assert max(w["tol_ic"].max(), w["tol_kld"].max(), w["tol_mean"].max(), w["tol_sys"]) < 1e-9
        assert w["tol_ic"].max() < 6.2e-14 and w["tol_kld"].max() < 3.2e-12   # the closed bounds of the derivation
        assert w["tol_ic"].min() >= 48 * U and w["tol_kld"].min() >= 2 * 896 * SCALE * U


OUTS = {"width": (np.uint32, 0), "n_conserved": (np.uint32, 0), "n_match": (np.uint32, 0), "passes": (np.uint8, 0),
        "kld_match_mean": (np.float64, 0), "kld_all_mean": (np.float64, 0), "col_start": (np.uint64, 3), "counts": (np.uint32, 2),
        "ic": (np.float64, 2), "col_flags": (np.uint8, 2), "kld_match": (np.float64, 1), "kld_all": (np.float64, 1)}
CT = {np.uint32: C.c_uint32, np.uint8: C.c_uint8, np.float64: C.c_double, np.uint64: C.c_uint64}


def _raw_call(ctx, r0, r1, mc, ncl, column, params, null=(), cap=4096, stats=True):
    """the C entry point with chosen arguments null -> (status, stats)"""
    sizes = (max(ncl, 1), max(r1 - r0, 1), cap * 21 + 1, ncl + 1)
    out = {k: np.zeros(sizes[which], dt) for k, (dt, which) in OUTS.items()}
    ptr = {k: None if k in null else out[k].ctypes.data_as(C.POINTER(CT[OUTS[k][0]])) for k in OUTS}
    u32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.uint32).ctypes.data_as(C.POINTER(C.c_uint32))   # noqa: E731
    S = N.ProfileStats()
    st = N.lib.hmk_cluster_profile(ctx._h, r0, r1, u32(mc), ncl, u32(column), None if params is None else C.byref(params),
                                   ptr["width"], ptr["n_conserved"], ptr["n_match"], ptr["passes"], ptr["kld_match_mean"], ptr["kld_all_mean"],
                                   ptr["col_start"], cap, ptr["counts"], ptr["ic"], ptr["col_flags"], ptr["kld_match"], ptr["kld_all"],
                                   C.byref(S) if stats else None)
    return st, S


def test_host_only_context_answers_every_refusal(blosum62):
    rng = np.random.default_rng(6)
    peps = [rng.integers(0, 20, size=12).astype(np.uint8) for _ in range(6)] + [np.array([0, 1, 20, 3], dtype=np.uint8)]
    res, off = hammock_amd.pack_sequences(peps)
    ctx = hammock_amd.Context(blosum62, device=-1)
    ctx.set_sequences(residues=res, offsets=off)
    mc, col = [0, 0, 1, 1, 2, 2], [0, 1, 2, 0, 0, 3]
    good = hammock_amd.profile_params(frequency())
    bad, err = N.HMK_ERR_BAD_ARG, lambda: N.lib.hmk_last_error(ctx._h).decode()   # noqa: E731
    call = lambda *a, **k: _raw_call(ctx, *a, **k)[0]   # noqa: E731
    # the range and slot checks of hmk_cluster_linkage_shifted
    assert call(4, 2, mc[:2], 1, col[:2], good) == bad                        # r0 > r1
    assert call(0, 8, mc + [2, 2], 3, col + [0, 0], good) == bad              # r1 > n
    assert call(0, 6, [0, 0, 1, 1, 3, 3], 3, col, good) == bad                # a slot at or above n_clusters
    assert call(0, 6, [0, 0, 1, 1, 1, 1], 3, col, good) == bad                # a slot without a member
    assert call(0, 6, None, 3, col, good) == bad                              # null member_cluster
    assert call(0, 6, mc, 3, None, good) == bad                               # null column
    assert call(0, 6, mc, 3, col, None) == bad                                # null params
    assert call(0, 6, mc, 3, col, good, stats=False) == bad                   # null stats
    for name in ("width", "n_conserved", "n_match", "passes", "kld_match_mean", "kld_all_mean", "col_start", "kld_match", "kld_all"):
        assert call(0, 6, mc, 3, col, good, null=(name,)) == bad, name
        assert "null" in err()
    # the placement against the width cap: 12 residues fit up to column 84
    assert call(0, 6, mc, 3, [84, 0, 0, 0, 0, 0], good) == N.HMK_ERR_DEVICE
    assert call(0, 6, mc, 3, [85, 0, 0, 0, 0, 0], good) == bad and "HMK_PROFILE_MAX_WIDTH" in err()
    assert call(0, 6, mc, 3, [0, 0, 0, 0, 0, 2 ** 32 - 1], good) == bad
    # the parameters
    def changed(**kw):
        P = hammock_amd.profile_params(frequency())
        for k, v in kw.items():
            if k in ("frequency", "background"):
                getattr(P, k)[v[0]] = v[1]
            else:
                setattr(P, k, v)
        return P
    for kw in (dict(min_ic=math.nan), dict(min_ic=math.inf), dict(max_gap_proportion=-0.01), dict(max_gap_proportion=1.01),
               dict(max_gap_proportion=math.nan), dict(min_conserved_positions=-1), dict(beta=0.0), dict(beta=math.inf), dict(sigma=-1.0),
               dict(sigma=math.nan), dict(scale=0.0), dict(frequency=(399, 0.0)), dict(frequency=(7, math.nan)), dict(frequency=(0, -0.1)),
               dict(background=(19, 0.0)), dict(background=(0, math.inf))):
        assert call(0, 6, mc, 3, col, changed(**kw)) == bad, kw
    for kw in (dict(min_ic=-3.0), dict(max_gap_proportion=0.0), dict(max_gap_proportion=1.0), dict(min_conserved_positions=0)):
        assert call(0, 6, mc, 3, col, changed(**kw)) == N.HMK_ERR_DEVICE, kw
    # a residue code outside the 20 amino acids: the reference's NullPointerException -- after the argument checks
    assert call(0, 7, mc + [2], 3, col + [0], good) == N.HMK_ERR_REFERENCE_WOULD_CRASH and "sequence 6" in err()
    assert call(0, 7, mc + [2], 3, col + [93], good) == bad
    with pytest.raises(hammock_amd.ReferenceWouldCrash):
        ctx.cluster_profile(0, 7, mc + [2], 3, col + [0], good)
    # the capacity: widths 13, 14, 15 -> 42 columns; answered with the needed count, whichever per-column array is asked for
    for null in ((), ("counts", "ic"), ("ic", "col_flags"), ("counts", "col_flags")):
        st, S = _raw_call(ctx, 0, 6, mc, 3, col, good, null=null, cap=41)
        assert st == N.HMK_ERR_CAPACITY and S.columns == 42, null
    assert call(0, 6, mc, 3, col, good, cap=42) == N.HMK_ERR_DEVICE
    assert call(0, 6, mc, 3, col, good, null=("counts", "ic", "col_flags"), cap=0) == N.HMK_ERR_DEVICE   # nothing per column is asked for
    with pytest.raises(BufferError) as e:
        ctx.cluster_profile(0, 6, mc, 3, col, good, col_capacity=10)
    assert e.value.needed == 42
    # a valid call: no CPU fallback
    with pytest.raises(hammock_amd.DeviceError):
        ctx.cluster_profile(0, 6, mc, 3, col, good)
    with pytest.raises(hammock_amd.DeviceError):
        ctx.cluster_profile(2, 6, [0, 0, 1, 1], 2, col[2:], good, counts=False, ic=False, flags=False)
    with pytest.raises(ValueError):
        ctx.cluster_profile(0, 6, mc, 3, col[:5], good)


# ---- GPU ---------------------------------------------------------------------------------------------------------------------

def wanted_grids(mc, ncl, width, large_min=LARGE_MIN):
    """kernel -> the grid its launcher asks for (k_profile.hip's launchers)"""
    size = np.bincount(mc, minlength=ncl).astype(np.int64)
    ncols = int(np.asarray(width, dtype=np.int64).sum())
    up = lambda a, b: -(-int(a) // b)   # noqa: E731
    grids = {"k_profile_init": min(up(max(ncols * 21, mc.size, ncl), 256), 4096), "k_profile_counts_small": min(up(mc.size, 256), 65536),
             "k_profile_columns": min(up(ncols, 256), 65536), "k_profile_match": min(up(ncols, 256), 65536)}
    chunks = sum(up(s, CHUNK) for s in size if s >= max(large_min, 2))
    if chunks:
        grids["k_profile_counts_large"] = min(chunks, 65536)
    if (size >= 2).any():
        grids["k_profile_kld"] = min(up(size[size >= 2].sum(), 256), 65536)
    return grids, chunks, int((size[mc] < large_min).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("pset", ["inner0", "inner1"])
def test_motif_family_matches_the_definition_under_every_grid(gpu, monkeypatch, capfd, pset):
    """all outputs against the definition with allow_inner_gaps 0 and 1; uncapped and under HMK_TEST_GRID_CAP = 1 and 3 every new
    kernel says how its grid was cut, and every output is bit-identical across the three grids and across repeated calls"""
    peps, mc, ncl, col, res, off = motif_input()
    want = motif_want(pset)
    kw = PARAM_SETS[pset]
    P = params_of(pset)
    ctx = device_ctx(_blosum62(), res, off)
    grids, chunks, small = wanted_grids(mc, ncl, want["width"])
    assert set(grids) == set(KERNELS)
    runs = []
    for cap in (0, 1, 3, 0):
        if cap:
            monkeypatch.setenv("HMK_TEST_GRID_CAP", str(cap))
        else:
            monkeypatch.delenv("HMK_TEST_GRID_CAP", raising=False)
        capfd.readouterr()
        R = ctx.cluster_profile(0, mc.size, mc, ncl, col, P)
        lines = {}
        for kernel, wanted, launched in GRID_LINE.findall(capfd.readouterr().err):
            lines.setdefault(kernel, set()).add((int(wanted), int(launched)))
        assert {k: v for k, v in lines.items() if k.startswith("k_profile_")} == {k: {(w, cap)} for k, w in grids.items() if cap and w > cap}
        if cap == 1:   # a new kernel without a line under cap 1 would not have had its work loop tested
            assert set(lines) >= set(KERNELS)
        s = R.stats
        assert (s.launches, s.large_chunks, s.small_members) == (len(grids), chunks, small) and s.kernel_ms > 0
        runs.append(R)
    compare(runs[0], want, pset)
    consistent(runs[0], mc, 1.2, kw.get("min_cons", 0), kw.get("allow", False))
    for R in runs[1:]:
        identical(runs[0], R)
    assert runs[0].match_string(MOTIF_SIZES.index(64)) == "".join("M" if f & 2 else "." for f in want["flags"][
        int(want["col_start"][MOTIF_SIZES.index(64)]):int(want["col_start"][MOTIF_SIZES.index(64) + 1])])


@pytest.mark.gpu
@pytest.mark.parametrize("pset", ["skewed", "ic25"])
def test_another_background_and_another_min_ic(gpu, pset):
    peps, mc, ncl, col, res, off = motif_input()
    ctx = device_ctx(_blosum62(), res, off)
    R = ctx.cluster_profile(0, mc.size, mc, ncl, col, params_of(pset))
    compare(R, motif_want(pset), pset)
    consistent(R, mc, PARAM_SETS[pset].get("min_ic", 1.2), PARAM_SETS[pset].get("min_cons", 0), False)


@pytest.mark.gpu
def test_both_count_forms_give_the_same_counts(gpu, monkeypatch):
    """HMK_PROFILE_LARGE_MIN moves the boundary between the two count kernels: every slot through the LDS form, every slot
    through the lane-per-member form, and the default give identical outputs"""
    peps, mc, ncl, col, res, off = motif_input()
    ctx = device_ctx(_blosum62(), res, off)
    P = params_of("inner0")
    base = ctx.cluster_profile(0, mc.size, mc, ncl, col, P)
    compare(base, motif_want("inner0"))
    for large_min in (2, 10 ** 6, 1024, 256):
        monkeypatch.setenv("HMK_PROFILE_LARGE_MIN", str(large_min))
        R = ctx.cluster_profile(0, mc.size, mc, ncl, col, P)
        _, chunks, small = wanted_grids(mc, ncl, R.width, large_min)
        assert (R.stats.large_chunks, R.stats.small_members) == (chunks, small), large_min
        identical(base, R)
    assert wanted_grids(mc, ncl, base.width, 2)[2] == 1 and wanted_grids(mc, ncl, base.width, 10 ** 6)[1] == 0


@pytest.mark.gpu
def test_optional_outputs_capacity_and_state_between_calls(gpu):
    """each optional output NULL in turn; HMK_ERR_CAPACITY with the needed count and the next call right; other slots, an inner
    range, other parameters on one context: nothing stays behind"""
    peps, mc, ncl, col, res, off = motif_input()
    ctx = device_ctx(_blosum62(), res, off)
    P = params_of("inner0")
    want = motif_want("inner0")
    full = ctx.cluster_profile(0, mc.size, mc, ncl, col, P)
    compare(full, want)
    for drop in ("counts", "ic", "flags"):
        R = ctx.cluster_profile(0, mc.size, mc, ncl, col, P, **{drop: False})
        assert getattr(R, {"flags": "col_flags"}.get(drop, drop)) is None
        compare(R, want, drop)
    R = ctx.cluster_profile(0, mc.size, mc, ncl, col, P, counts=False, ic=False, flags=False)
    assert np.array_equal(R.kld_all, full.kld_all) and np.array_equal(R.n_match, full.n_match)
    ncols = int(want["col_start"][-1])
    with pytest.raises(BufferError) as e:
        ctx.cluster_profile(0, mc.size, mc, ncl, col, P, col_capacity=ncols - 1)
    assert e.value.needed == ncols
    identical(full, ctx.cluster_profile(0, mc.size, mc, ncl, col, P, col_capacity=ncols))
    # an inner range with its own slots, placement and parameters
    rng = np.random.default_rng(77_100)
    r0, r1 = 1000, 2400
    sub_mc = rng.permutation(np.repeat(np.arange(6), [1, 2, 300, 1000, 90, 7])).astype(np.uint32)
    sub_col = rng.integers(0, 5, size=r1 - r0).astype(np.uint32)
    P2 = hammock_amd.profile_params(frequency(), skewed_background(), min_ic=0.8, max_gap_proportion=0.35, min_conserved_positions=5,
                                    allow_inner_gaps=True, beta=50.0, sigma=3.0, scale=1.5)
    w2 = definition(peps[r0:r1], sub_mc, 6, sub_col, frequency(), skewed_background(), min_ic=0.8, max_gap=0.35, min_cons=5, allow=True,
                    beta=50.0, sigma=3.0, scale=1.5)
    assert np.abs(w2["ic"] - 0.8).min() >= 1e-9
    compare(ctx.cluster_profile(r0, r1, sub_mc, 6, sub_col, P2), w2, "inner range")
    identical(full, ctx.cluster_profile(0, mc.size, mc, ncl, col, P))


@pytest.mark.gpu
def test_degenerate_inputs_and_the_widest_slot(gpu):
    peps, mc, ncl, col, res, off = motif_input()
    ctx = device_ctx(_blosum62(), res, off)
    P = params_of("inner0")
    F, bg = frequency(), np.full(20, 0.05)
    # singletons only: every column holds one letter, ic = log2 20; nothing enters the system means
    one = np.arange(50, dtype=np.uint32)
    R = ctx.cluster_profile(10, 60, one, 50, np.zeros(50, dtype=np.uint32), P)
    compare(R, definition(peps[10:60], one, 50, np.zeros(50, int), F, bg), "singletons")
    assert not R.kld_all.any() and not R.kld_match.any() and R.stats.omitted == 50 and (R.col_flags == 3).all()
    assert (R.counts.sum(axis=1) == 1).all() and not R.counts[:, 20].any()
    # an empty range
    R = ctx.cluster_profile(7, 7, [], 0, [], P)
    assert R.col_start.tolist() == [0] and R.width.size == 0 and R.kld_all.size == 0 and R.counts.shape == (0, 21) and R.stats.columns == 0
    # a slot at width exactly HMK_PROFILE_MAX_WIDTH: members spread over columns 0 .. 96 - length
    lens = np.array([len(q) for q in peps[:300]])
    wide = (np.arange(300) * 5) % (97 - lens)
    wide[7] = 96 - lens[7]
    wide = wide.astype(np.uint32)
    R = ctx.cluster_profile(0, 300, np.zeros(300, dtype=np.uint32), 1, wide, P)
    w = definition(peps[:300], np.zeros(300, int), 1, wide, F, bg)
    assert R.width.tolist() == [96] and np.abs(w["ic"] - 1.2).min() >= 1e-9
    compare(R, w, "width 96")
    wide[7] += 1
    with pytest.raises(ValueError, match="HMK_PROFILE_MAX_WIDTH"):
        ctx.cluster_profile(0, 300, np.zeros(300, dtype=np.uint32), 1, wide, P)


@pytest.mark.gpu
def test_device_list_runs_on_the_root(gpu):
    peps, mc, ncl, col, res, off = motif_input()
    ctx = hammock_amd.Context(_blosum62(), device=[0, 0])
    ctx.set_sequences(residues=res, offsets=off)
    compare(ctx.cluster_profile(0, mc.size, mc, ncl, col, params_of("inner1")), motif_want("inner1"), "device list")


@pytest.mark.gpu
def test_the_tie_column_is_decided_once(gpu):
    """ic = 1.2 in exact arithmetic: which side the device falls on is rounding, so only consistency is asserted -- the flags
    against the returned ic, the counts of the bits, and kld_match against the returned flags"""
    peps, mc, ncl, col = tie_family()
    res, off = hammock_amd.pack_sequences(peps)
    ctx = device_ctx(_blosum62(), res, off)
    F, bg = frequency(), np.full(20, 0.05)
    for allow in (False, True):
        R = ctx.cluster_profile(0, 13, mc, ncl, col, hammock_amd.profile_params(F, allow_inner_gaps=allow))
        w = definition(peps, mc, ncl, col, F, bg, allow=allow)
        assert abs(R.ic[0] - 1.2) <= w["tol_ic"][0] and (np.abs(R.ic - w["ic"]) <= w["tol_ic"]).all()
        consistent(R, mc, 1.2, 0, allow)
        # the definition with the device's decision for column 0 put in: min_ic moved just below or above 1.2
        side = 1.2 - 1e-9 if R.col_flags[0] & 1 else 1.2 + 1e-9
        w = definition(peps, mc, ncl, col, F, bg, min_ic=side, allow=allow)
        assert np.array_equal(R.col_flags.astype(np.int64), w["flags"])
        assert (np.abs(R.kld_match - w["kld_match"]) <= w["tol_kld"]).all() and (np.abs(R.kld_all - w["kld_all"]) <= w["tol_kld"]).all()


@pytest.mark.gpu
def test_columns_of_the_align_call(gpu):
    """the composition the call was made for: columns from hmk_cluster_align_shifted on the clusters of hmk_greedy_cluster on MUSI
    and on a window family, against the definition"""
    M, F, bg = _blosum62(), frequency(), np.full(20, 0.05)
    P = hammock_amd.profile_params(F, min_conserved_positions=4)
    seqs = list(dict.fromkeys(_musi()))
    res, off = hammock_amd.pack_sequences(seqs)
    ctx = device_ctx(M, res, off)
    cid = ctx.greedy_cluster(3, 0, 20, 2 ** 31 - 1)[0]
    _, mc = np.unique(cid, return_inverse=True)
    mc = mc.astype(np.uint32)
    ncl = int(mc.max()) + 1
    inputs = [("musi", ctx, [hammock_amd.encode(s) for s in seqs], mc, ncl, 3, 0)]
    peps, wmc, wncl = window_family(0)
    wres, woff = hammock_amd.pack_sequences(peps)
    inputs.append(("window", device_ctx(M, wres, woff), peps, wmc, wncl, 3, -1))
    for name, c, p, m, n, X, pen in inputs:
        _, _, width, _, _, _, column = c.cluster_align_shifted(0, m.size, m, n, X, pen, sums=False)
        w = definition(p, m, n, column, F, bg, min_cons=4)
        assert np.abs(w["ic"] - 1.2).min() >= 1e-9 and w["n_multi"] > 5, name
        R = c.cluster_profile(0, m.size, m, n, column, P)
        assert np.array_equal(R.width, width), name
        compare(R, w, name)


# ---- the mode ------------------------------------------------------------------------------------------------------------------

def test_cli_profile_argument_and_file_errors(tmp_path):
    from test_continue import cli
    good = tmp_path / "good.tsv"
    good.write_text("cluster_id\tsequence\tno_label\n1\tWVTAPRSLPVLP\t1\n1\tWVTAPRSLPVLA\t1\n")
    r = cli("profile", "-d", str(tmp_path / "a"), "--frequency_matrix", FREQ_FILE)
    assert r.returncode == 2 and "-i or --input" in r.stderr
    r = cli("profile", "-i", str(good), "-d", str(tmp_path / "a"))
    assert r.returncode == 2 and "--frequency_matrix" in r.stderr and "missing with no default" in r.stderr
    r = cli("profile", "-i", str(good), "--devices", "0,1", "-d", str(tmp_path / "a"), "--frequency_matrix", FREQ_FILE)
    assert r.returncode == 2 and "--devices" in r.stderr
    assert not (tmp_path / "a").exists()
    text = open(FREQ_FILE).read()
    for name, bad in (("rows", text.rsplit("\n", 2)[0] + "\n"), ("letters", text.replace("\tV\n", "\tB\n", 1)), ("word", text.replace("0.2901", "x"))):
        (tmp_path / name).write_text(bad)
        r = cli("profile", "-i", str(good), "-d", str(tmp_path / ("f" + name)), "--frequency_matrix", str(tmp_path / name))
        assert r.returncode == 2 and "FileFormatException" in r.stderr, name
    (tmp_path / "bg").write_text("0.1 0.2 0.3\n")
    r = cli("profile", "-i", str(good), "-d", str(tmp_path / "b"), "--frequency_matrix", FREQ_FILE, "--background", str(tmp_path / "bg"))
    assert r.returncode == 2 and "FileFormatException" in r.stderr and "background" in r.stderr
    na = tmp_path / "na.tsv"
    na.write_text("cluster_id\tsequence\tno_label\n1\tWVTAPRSLPVLP\t1\nNA\tWVTAPRSLPVLA\t1\n")
    r = cli("profile", "-i", str(na), "-d", str(tmp_path / "c"), "--frequency_matrix", FREQ_FILE)
    assert r.returncode == 2 and "FileFormatException" in r.stderr
    r = cli("profile", "-i", str(good), "-d", str(tmp_path / "c"), "--frequency_matrix", FREQ_FILE)   # the directory exists now
    assert r.returncode == 2 and "Output directory exists" in r.stderr
    usage = cli("--help").stderr
    assert "hammock-hip profile -i <clusters.tsv> -d <directory> --frequency_matrix <file>" in usage
    assert "Statistics.java:25-28" in usage and "--max_inner_gaps" in usage


def profile_files(ids, uniq, seqs, mc, R, skip):
    """the three files of the mode from the API's outputs"""
    g17 = lambda v: "%.17g" % v   # noqa: E731
    cf = ["cluster_id\tsize\twidth\tconserved\tmatch_states\tpasses\tkld_match_mean\tkld_all_mean"]
    pf = ["cluster_id\tcolumn\tgaps\tic\tflags\t" + "\t".join(LETTERS[:20])]
    mf = ["cluster_id\tsequence\tkld_match\tkld_all"]
    for k, c in enumerate(ids):
        if skip and uniq[k] == 1:
            continue
        cf.append(f"{c}\t{uniq[k]}\t{R.width[k]}\t{R.n_conserved[k]}\t{R.match_string(k)}\t{R.passes[k]}\t{g17(R.kld_match_mean[k])}\t{g17(R.kld_all_mean[k])}")
        a = int(R.col_start[k])
        for g in range(a, int(R.col_start[k + 1])):
            pf.append(f"{c}\t{g - a + 1}\t{R.counts[g, 20]}\t{g17(R.ic[g])}\t{R.col_flags[g]}\t" + "\t".join(str(v) for v in R.counts[g, :20]))
        for j in np.flatnonzero(mc == k):
            mf.append(f"{c}\t{seqs[j]}\t{g17(R.kld_match[j])}\t{g17(R.kld_all[j])}")
    return tuple("\n".join(x) + "\n" for x in (cf, pf, mf))


@pytest.mark.gpu
def test_cli_profile_on_greedy_clusters(gpu, tmp_path):
    """`profile` on greedy's stage-1 file of MUSI: the three files byte for byte against files built from the API's outputs of the
    same inputs, which are themselves compared with the definition; align's files unchanged beside align's own"""
    from test_align import _java_round
    from test_continue import cli, read_cluster_file
    r = cli("greedy", "-i", os.path.join(GOLDEN, "musi.fa"), "-d", str(tmp_path / "g"), timeout=600)
    assert r.returncode == 0, r.stderr
    cfile = tmp_path / "g" / "initial_clusters_sequences.tsv"
    loaded = read_cluster_file(cfile)   # (cluster id, sequence, size) per line
    ids = list(dict.fromkeys(c for c, _, _ in loaded))
    slot = {c: k for k, c in enumerate(ids)}
    order = sorted(range(len(loaded)), key=lambda k: slot[loaded[k][0]])   # (stable) the upload: cluster by cluster
    seqs = [loaded[k][1] for k in order]
    mc = np.array([slot[loaded[k][0]] for k in order], dtype=np.uint32)
    uniq = np.bincount(mc)
    lens = [len(s) for s in seqs]
    mean = sum(lens) / len(lens)
    X, min_cons = min(_java_round(mean / 4), min(lens) - 1), _java_round(mean / 3)
    res, off = hammock_amd.pack_sequences(seqs)
    ctx = device_ctx(_blosum62(), res, off)
    column = ctx.cluster_align_shifted(0, len(seqs), mc, len(ids), X, 0, sums=False)[6]
    peps = [hammock_amd.encode(s) for s in seqs]
    r = cli("align", "-i", str(cfile), "-d", str(tmp_path / "a"), timeout=600)
    assert r.returncode == 0, r.stderr
    bgfile = tmp_path / "bg.txt"
    bgfile.write_text("# made here\n" + "\t".join(repr(float(v)) for v in skewed_background()) + "\n")
    runs = [("p0", [], dict(), None),
            ("p1", ["--background", str(bgfile), "--max_inner_gaps", "1", "--min_ic", "2.5", "-y", "0.3", "--min_conserved_positions", "2", "--skip_singletons"],
             dict(min_ic=2.5, max_gap=0.3, min_cons=2, allow=True), skewed_background())]
    for name, extra, kw, bg in runs:
        kw.setdefault("min_cons", min_cons)
        if "min_ic" in kw:   # a second min_ic with room on the reference alone: columns of few members land on round values often
            ic = definition(peps, mc, len(ids), column, frequency(), bg, **kw)["ic"]
            kw["min_ic"] = next(v for v in (2.5, 2.47, 2.43, 2.39, 2.33) if np.abs(ic - v).min() >= 1e-9)
            extra[extra.index("--min_ic") + 1] = repr(kw["min_ic"])
        P = hammock_amd.profile_params(frequency(), bg, min_ic=kw.get("min_ic", 1.2), max_gap_proportion=kw.get("max_gap", 0.2),
                                       min_conserved_positions=kw["min_cons"], allow_inner_gaps=kw.get("allow", False))
        R = ctx.cluster_profile(0, len(seqs), mc, len(ids), column, P)
        w = definition(peps, mc, len(ids), column, frequency(), np.full(20, 0.05) if bg is None else bg, **kw)
        assert np.abs(w["ic"] - w["min_ic"]).min() >= 1e-9 and w["n_multi"] > 20 and w["omitted"] > 0
        compare(R, w, name)
        out = tmp_path / name
        r = cli("profile", "-i", str(cfile), "-d", str(out), "--frequency_matrix", FREQ_FILE, *extra, timeout=600)
        assert r.returncode == 0, r.stderr
        log = (out / "run.log").read_text()
        for text in (r.stderr, log):
            assert "Final system KLD over match state MSA positions: " + "%.17g" % R.stats.system_kld_match + "\n" in text
            assert "Final system KLD over all MSA positions: " + "%.17g" % R.stats.system_kld_all + "\n" in text
            assert f"{w['omitted']} clusters omitted from KLD calculation because each of them only contains a single unique sequence." in text
            assert ("Minimal number of match states not set. Setting automatically to: " + str(min_cons) in text) == (not extra)
        cf, pf, mf = profile_files(ids, uniq, seqs, mc, R, bool(extra))
        assert (out / "cluster_profiles.tsv").read_text() == cf
        assert (out / "position_profiles.tsv").read_text() == pf
        assert (out / "member_kld.tsv").read_text() == mf
        # what align writes, unchanged
        assert (out / "initial_clusters_sequences.tsv").read_bytes() == (tmp_path / "a" / "initial_clusters_sequences.tsv").read_bytes()
        if not extra:
            assert (out / "cluster_centers.tsv").read_bytes() == (tmp_path / "a" / "cluster_centers.tsv").read_bytes()
        files = sorted(os.listdir(out / "alignments_initial"))
        assert files == sorted(os.listdir(tmp_path / "a" / "alignments_initial")) and len(files) == w["n_multi"]
        for f in files:
            assert (out / "alignments_initial" / f).read_bytes() == (tmp_path / "a" / "alignments_initial" / f).read_bytes()
