"""A plain Python model of how the shifted-scorer path narrows a score, and builders of inputs that land on the edges of every
narrowing.  Restated from the planner, never imported from it:

  lane_path / lane_window / u8_row_limit / row_bound / allpairs_tiers   classify() and build_plan's row-bound split (hmk_plan.cpp)
  adjacency_packed                                                      hmk_sizing.h
  plane_sums                                                            ShiftedScorer's per-shift sums (the oracle's loop)

A lane of a shift plane starts at g + penalty - bias * cells (g = half - threshold) and ends at g + penalty + score of the plane; the
tier is exact only while 0 <= start and end <= lane_max for every pair the class may hold.  with_synonyms() makes ambiguity codes exact
copies of real residues, so two DISTINCT peptides score what a peptide scores against itself: the top of a lane, the row bound of a
row, the 255 of an adjacency entry can be reached exactly.  The families below are what tests/test_score_field_edges.py plants."""
import numpy as np

ALPHABET = "ARNDCQEGHILKMFPSTWYVBZX*"
SYNONYMS = (("W", "B"), ("K", "Z"), ("I", "X"))      # (original, copy)
LANES = {"u8": (255, 128, 32), "u16": (65535, 32768, 16)}    # lane_max, half, most planes
BOUND_CAP = 4095                                    # build_plan's BCAP: bounds are clamped for the counting sort


def code(ch):
    return ALPHABET.index(ch)


def word(text):
    return np.array([code(c) for c in text], dtype=np.uint8)


def java_round(v):
    """Math.round for positive doubles: half up"""
    return int(np.floor(v + 0.5))


def uniform_defaults(L):
    """the reference's defaults for a set of one length: (max shift, the threshold round(1.7 L), the threshold round(0.4 L))"""
    return min(java_round(L / 4), L - 1), java_round(1.7 * L), java_round(0.4 * L)


# ---- the predicate ------------------------------------------------------------------------------------------------------------------

def bias_of(M):
    return -int(M.min()) if M.min() < 0 else 0


def planes(la, lb, X, p):
    """the 2X + d + 1 shift planes of a (la, lb) class: [(shift, cells, penalty)]"""
    m, nl = min(la, lb), max(la, lb)
    d = nl - m
    out = []
    for t in range(2 * X + d + 1):
        s = t - X
        ncell = m + s if s <= 0 else min(m, nl - s)
        pen = d * p + (-s * 2 * p if s < 0 else 0) + ((s - d) * 2 * p if s > d else 0)
        out.append((s, ncell, pen))
    return out


def lane_fit(M, la, lb, X, p, thr, kind, row_bound=-1):
    """classify's loop for one lane width -> (fits, the row limit or -1): lanes start at g + penalty - bias * cells and must hold
    every cell at the matrix maximum (row_bound < 0) or a row's bound, for each of the 2X + d + 1 shifts"""
    lane_max, half, max_nd = LANES[kind]
    pl = planes(la, lb, X, p)
    bias = bias_of(M)
    cell_max = int(M.max()) + bias
    if len(pl) > max_nd or cell_max > 255:
        return False, -1
    g = half - thr
    ok = lower_ok = True
    limit = 1 << 40
    for _, ncell, pen in pl:
        c0 = g + pen - bias * ncell
        if c0 < 0:
            lower_ok = False
        top = g + pen + row_bound if row_bound >= 0 else c0 + ncell * cell_max
        if top > lane_max:
            ok = False
        limit = min(limit, lane_max - g - pen)
    return ok and lower_ok, (limit if lower_ok else -1)


def lane_path(M, la, lb, X, p, thr):
    """classify's rule (hmk_plan.cpp) without a row bound -> "u8" | "u16" | "direct": lanes start at g + penalty - bias * cells and
    must hold every cell at the matrix maximum, for each of the 2X + d + 1 shifts"""
    for kind in ("u8", "u16"):
        if lane_fit(M, la, lb, X, p, thr, kind)[0]:
            return kind
    return "direct"


def lane_window(M, la, lb, X, p, kind):
    """the thresholds at which `kind` lanes fit every pair of the class -> (thr_lo, thr_hi) or None.  At thr_lo the plane with the
    largest penalty + cells * max ends at lane_max when every cell is the maximum; at thr_hi the plane with the smallest
    penalty - bias * cells starts at 0.  Solved from the two inequalities, and checked against lane_fit one step to either side."""
    lane_max, half, max_nd = LANES[kind]
    pl = planes(la, lb, X, p)
    bias = bias_of(M)
    if len(pl) > max_nd or int(M.max()) + bias > 255:
        return None
    lo = half - lane_max + max(pen + ncell * int(M.max()) for _, ncell, pen in pl)
    hi = half + min(pen - bias * ncell for _, ncell, pen in pl)
    if lo > hi:
        return None
    assert lane_fit(M, la, lb, X, p, lo, kind)[0] and lane_fit(M, la, lb, X, p, hi, kind)[0]
    assert not lane_fit(M, la, lb, X, p, lo - 1, kind)[0] and not lane_fit(M, la, lb, X, p, hi + 1, kind)[0]
    return lo, hi


def u8_row_limit(M, la, lb, X, p, thr):
    """classify's *u8_row_limit: the largest row bound for which 8-bit lanes fit, or -1 if their start values never do"""
    return lane_fit(M, la, lb, X, p, thr, "u8")[1]


def best_cells(M):
    """build_plan's best[]: per residue the best non-negative cell of its row and column"""
    return np.maximum(0, np.maximum(M.max(axis=1), M.max(axis=0))).astype(np.int64)


def row_bound(M, seq):
    """no pair that holds seq scores above the sum of its residues' best cells"""
    return int(best_cells(M)[np.asarray(seq, dtype=np.int64)].sum())


def allpairs_tiers(M, seqs, X, p, thr):
    """the classes of the all-vs-all plan under a symmetric matrix (build_plan): one per (row length >= column length) present;
    if some class misses 8-bit lanes but has a row limit, every such class is split by its rows' bounds into an 8-bit range (bound
    within the limit) and the rest -> {"u8", "u16", "direct"} class counts"""
    assert (M == M.T).all()
    lens = np.array([len(s) for s in seqs])
    present = [int(v) for v in np.unique(lens)]
    count = {L: int((lens == L).sum()) for L in present}
    pairs = [(la, lb) for la in present for lb in present if lb <= la and not (la == lb and count[la] < 2)]
    every = [(la, lb) for la in present for lb in present if lb <= la]     # (the refine scan does not look at bucket sizes)
    refine = any(lane_path(M, la, lb, X, p, thr) != "u8" and u8_row_limit(M, la, lb, X, p, thr) >= 0 for la, lb in every)
    out = {"u8": 0, "u16": 0, "direct": 0}
    for la, lb in pairs:
        path = lane_path(M, la, lb, X, p, thr)
        limit = u8_row_limit(M, la, lb, X, p, thr)
        if refine and path != "u8" and limit >= 0:
            lim = min(limit, BOUND_CAP - 1)
            bounds = np.array([min(row_bound(M, s), BOUND_CAP) for s in seqs if len(s) == la])
            fit = int((bounds <= lim).sum())
            if fit and lane_fit(M, la, lb, X, p, thr, "u8", lim)[0]:
                out["u8"] += 1
            else:
                fit = 0
            if fit < len(bounds):
                out[path] += 1
        else:
            out[path] += 1
    return out


def adjacency_packed(max_len, min_len, max_m, shift_penalty, max_shift, threshold, force_8byte=False):
    """hmk_sizing.h: adjacency entries are 4 bytes (m << 8 | score - threshold) when no score can exceed threshold + 255"""
    top = max_len * max(0, max_m) + max(0, shift_penalty) * ((max_len - min_len) + 2 * max_shift)
    return top - threshold <= 255 and not force_8byte


def plane_sums(M, a, b, X, p):
    """ShiftedScorer's loop: [(shift, sum of the cells, penalty)] of one pair; its score is the first strict maximum of sum + penalty"""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    longer, shorter = (a, b) if len(a) >= len(b) else (b, a)     # ties make seq2 the shorter one
    ll, sl = len(longer), len(shorter)
    out = []
    for s, ncell, pen in planes(ll, sl, X, p):
        if s <= 0:
            cells = M[shorter[-s:sl], longer[:sl + s]]
        else:
            lim = min(sl, ll - s)
            cells = M[shorter[:lim], longer[s:s + lim]]
        assert len(cells) == ncell
        out.append((s, int(cells.sum()), pen))
    return out


def shifted_score(M, a, b, X, p):
    return max(c + pen for _, c, pen in plane_sums(M, a, b, X, p))


# ---- matrices -----------------------------------------------------------------------------------------------------------------------

def with_synonyms(M, pairs=SYNONYMS):
    """M with each copy's row and column replaced by its original's and the copy's diagonal set to the original's: original and
    copy score alike against everything, each other included.  Symmetric if M is; minimum and maximum stay what they were as long
    as no copy held them alone."""
    S = np.array(M, dtype=np.int32, copy=True)
    for orig, copy in pairs:
        o, c = code(orig), code(copy)
        S[c, :] = S[o, :]
        S[:, c] = S[:, o]
        S[c, c] = S[o, o]
    return S


def clip14(M):
    return np.clip(M, -1, 4).astype(np.int32)


# ---- families -----------------------------------------------------------------------------------------------------------------------

def top_residues(M, pairs=SYNONYMS):
    """(original, copy) codes of the first synonym pair whose cells are all the matrix maximum"""
    for orig, copy in pairs:
        o, c = code(orig), code(copy)
        if M[o, o] == M[o, c] == M[c, o] == M[c, c] == M.max():
            return o, c
    raise AssertionError("no synonym pair at the matrix maximum")


def top_words(M, L, count, rng, fixed=(), pair=None):
    """`count` DISTINCT words of length L over one synonym pair, by default the one at the matrix maximum: any two score L * max at
    shift 0.  fixed: positions that hold the ORIGINAL in every word (shared key residues)"""
    o, c = (code(pair[0]), code(pair[1])) if pair else top_residues(M)
    free = [k for k in range(L) if k not in fixed]
    assert 2 <= count <= 2 ** len(free)
    first, second = np.full(L, o, dtype=np.uint8), np.full(L, o, dtype=np.uint8)     # the original alone; the copy wherever it may be
    second[free] = c
    out = [first, second]
    seen = {w.tobytes() for w in out}
    while len(out) < count:
        w = np.full(L, o, dtype=np.uint8)
        w[free] = np.where(rng.integers(0, 2, len(free)) == 1, c, o)
        if w.tobytes() not in seen:
            seen.add(w.tobytes())
            out.append(w)
    return out


def bottom_words(M, L_row, L_col, count, rng):
    """one word a^L_row and `count` distinct words of length L_col over {y: M[a, y] == M[y, a] == min}: every cell of every plane
    of (a-word, y-word) is the matrix minimum, so every lane of the pair stays at its start value.  Real residues only."""
    o, _ = top_residues(M)          # (kept out: a word of it alone is a top word)
    real = [y for y in range(20) if y != o]
    partners = {a: [y for y in real if y != a and M[a, y] == M.min() and M[y, a] == M.min()] for a in real}
    a = max(real, key=lambda a: len(partners[a]))
    ys = partners[a]
    assert ys
    rows = [np.full(L_row, a, dtype=np.uint8)]
    seen, cols = set(), []
    count = min(count, len(ys) ** L_col)
    while len(cols) < count:
        w = np.array(ys, dtype=np.uint8)[rng.integers(0, len(ys), L_col)]
        if len(cols) == 0:
            w[:] = ys[0]
        if w.tobytes() not in seen:
            seen.add(w.tobytes())
            cols.append(w)
    return rows, cols


def bound_exact_pair(M, L, bound, pairs=SYNONYMS):
    """a row of length L whose row_bound is exactly `bound`, and a distinct partner (the row with every synonym original replaced
    by its copy) that scores `bound` against it at shift 0.  Residues whose diagonal is their best cell, at least one of them a
    synonym original; found by a table over (length, sum)."""
    best = best_cells(M)
    usable = [a for a in range(20) if M[a, a] == best[a] and best[a] > 0]
    origs = {code(o): code(c) for o, c in pairs}
    first = max((a for a in usable if a in origs), key=lambda a: best[a])
    need = bound - int(best[first])
    reach = [{0: None}] + [dict() for _ in range(L - 1)]   # reach[k][sum] = (residue, previous sum) over k residues
    for k in range(1, L):
        for s, _ in reach[k - 1].items():
            for a in sorted(usable, key=lambda a: -best[a]):
                reach[k].setdefault(s + int(best[a]), (a, s))
    assert need in reach[L - 1], (L, bound)
    row, s = [first], need
    for k in range(L - 1, 0, -1):
        a, s = reach[k][s]
        row.append(a)
    row = np.array(sorted(row, key=lambda a: -best[a]), dtype=np.uint8)
    partner = np.array([origs.get(int(a), int(a)) for a in row], dtype=np.uint8)
    assert row_bound(M, row) == bound and not np.array_equal(row, partner)
    return row, partner


def score_exact_pair(M, L, target, X, p):
    """two distinct words of length L that score exactly `target`: the largest cells first (synonym original against its copy), then
    cells of real residue pairs found by a table over (length, sum); shift 0 must win, which the caller's oracle confirms"""
    o, c = top_residues(M)
    choices = {}          # cell value -> one (x, y) that has it, the synonym pair for the maximum
    for x in range(20):
        for y in range(20):
            choices.setdefault(int(M[x, y]), (x, y))
    choices[int(M.max())] = (o, c)
    values = sorted(choices, reverse=True)
    reach = [{0: None}] + [dict() for _ in range(L)]
    for k in range(1, L + 1):
        for s in reach[k - 1]:
            for v in values:
                reach[k].setdefault(s + v, (v, s))
    assert target in reach[L], (L, target)
    cells, s = [], target
    for k in range(L, 0, -1):
        v, s = reach[k][s]
        cells.append(v)
    cells.sort(reverse=True)
    a = np.array([choices[v][0] for v in cells], dtype=np.uint8)
    b = np.array([choices[v][1] for v in cells], dtype=np.uint8)
    assert not np.array_equal(a, b) and shifted_score(M, a, b, X, p) == target, (L, target)
    return a, b


def ordinary(rng, count, lens, avoid=()):
    """`count` distinct random peptides over the 20 real residues, lengths drawn from `lens`, none of them in `avoid`"""
    seen = {np.asarray(w, dtype=np.uint8).tobytes() for w in avoid}
    out = []
    while len(out) < count:
        w = rng.integers(0, 20, int(lens[int(rng.integers(len(lens)))]), dtype=np.uint8)
        if w.tobytes() not in seen:
            seen.add(w.tobytes())
            out.append(w)
    return out


def shuffled(rng, *groups):
    """the groups' words in one random order"""
    words = [w for g in groups for w in g]
    return [words[k] for k in rng.permutation(len(words))]
