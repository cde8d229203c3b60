"""The reference of tests/test_traceback.py: the walk of hmk_align_pairs_global (include/hammock_hip.h) restated in plain Python over
the tables of global_ref's recurrence, the star merge of `align --scorer global` in plain Python, the slips a wrong walk could make,
and the inputs the GPU tests run (so that the CPU tests can show that those inputs tell every slip from the rule).  Sequences are
sequences of residue indices; M is indexed [seq1 residue][seq2 residue]; penalties are added (<= 0).  All integers, all exact."""
import functools

import numpy as np

import gapped_ends as GE
from global_ref import NEG, edit_matrix

SLIPS = ("gap_before_diagonal", "f_before_e", "open_before_extend", "swapped", "reversed")


def tables(s1, s2, M, gap_open, gap_extend):
    """H, E, F of global_ref.global_score, kept"""
    n, m = len(s1), len(s2)
    H = [[NEG] * (m + 1) for _ in range(n + 1)]
    E = [[NEG] * (m + 1) for _ in range(n + 1)]
    F = [[NEG] * (m + 1) for _ in range(n + 1)]
    H[0][0] = 0
    for j in range(1, m + 1):
        H[0][j] = E[0][j] = gap_open + (j - 1) * gap_extend
    for i in range(1, n + 1):
        H[i][0] = F[i][0] = gap_open + (i - 1) * gap_extend
    for i in range(1, n + 1):
        Mi, Hi, Hp, Ei, Fi, Fp = M[s1[i - 1]], H[i], H[i - 1], E[i], F[i], F[i - 1]
        for j in range(1, m + 1):
            e = Ei[j] = max(Ei[j - 1] + gap_extend, Hi[j - 1] + gap_open)
            f = Fi[j] = max(Fp[j] + gap_extend, Hp[j] + gap_open)
            Hi[j] = max(Hp[j - 1] + Mi[s2[j - 1]], e, f)
    return H, E, F


def walk(s1, s2, M, gap_open, gap_extend, slip=None, T=None):
    """-> (score, n_cols, gap1, gap2): the one walk from (n, m) in state H to (0, 0); columns leave right to left, column 0 is the
    leftmost.  slip: one of SLIPS, the walk a wrong implementation would make."""
    if slip == "swapped":   # (seq1 and seq2 taken for each other: the record of the other pair)
        return walk(s2, s1, M, gap_open, gap_extend)
    H, E, F = T if T is not None else tables(s1, s2, M, gap_open, gap_extend)
    n, m = len(s1), len(s2)
    i, j, state = n, m, "H"
    cols = []   # right to left: 0 a pair, 1 a gap in seq1, 2 a gap in seq2
    while i > 0 or j > 0:
        if i == 0:
            cols.append(1)
            j -= 1
            continue
        if j == 0:
            cols.append(2)
            i -= 1
            continue
        if state == "H":
            diag = H[i][j] == H[i - 1][j - 1] + M[s1[i - 1]][s2[j - 1]]
            if slip == "gap_before_diagonal":
                state = "E" if H[i][j] == E[i][j] else "F" if H[i][j] == F[i][j] else "D"
            elif slip == "f_before_e":
                state = "D" if diag else "F" if H[i][j] == F[i][j] else "E"
            else:
                state = "D" if diag else "E" if H[i][j] == E[i][j] else "F"
            if state == "D":
                cols.append(0)
                i, j, state = i - 1, j - 1, "H"
                continue
        if state == "E":
            cols.append(1)
            if slip == "open_before_extend":
                stay = E[i][j] != H[i][j - 1] + gap_open
            else:
                stay = E[i][j] == E[i][j - 1] + gap_extend
            state = "E" if stay else "H"
            j -= 1
        else:
            cols.append(2)
            if slip == "open_before_extend":
                stay = F[i][j] != H[i - 1][j] + gap_open
            else:
                stay = F[i][j] == F[i - 1][j] + gap_extend
            state = "F" if stay else "H"
            i -= 1
    if slip != "reversed":
        cols.reverse()
    gap1 = sum(1 << c for c, k in enumerate(cols) if k == 1)
    gap2 = sum(1 << c for c, k in enumerate(cols) if k == 2)
    return H[n][m], len(cols), gap1, gap2


def rescore(s1, s2, M, gap_open, gap_extend, n_cols, gap1, gap2):
    """the score of the alignment a record describes, column by column: a run of k gap columns of one kind costs gap_open +
    (k - 1) gap_extend; asserts the record's invariants on the way"""
    assert gap1 & gap2 == 0 and (gap1 | gap2) >> n_cols == 0
    assert n_cols - bin(gap1).count("1") == len(s1) and n_cols - bin(gap2).count("1") == len(s2)
    assert max(len(s1), len(s2)) <= n_cols <= len(s1) + len(s2)
    i = j = total = last = 0
    for c in range(n_cols):
        if gap1 >> c & 1:
            total += gap_extend if last == 1 else gap_open
            j, last = j + 1, 1
        elif gap2 >> c & 1:
            total += gap_extend if last == 2 else gap_open
            i, last = i + 1, 2
        else:
            total += int(M[s1[i]][s2[j]])
            i, j, last = i + 1, j + 1, 0
    return total


def gapped_rows(s1, s2, n_cols, gap1, gap2):
    """the two rows of a record, over strings"""
    a, b = iter(s1), iter(s2)
    return ("".join("-" if gap1 >> c & 1 else next(a) for c in range(n_cols)),
            "".join("-" if gap2 >> c & 1 else next(b) for c in range(n_cols)))


def star_rows(center, members, records):
    """the star merge of DESIGN.md 5.28 in plain loops -> (centre row, member rows): ins[m][p] the residues of m that stand
    against a gap of the centre before its residue p (p = L: behind the last), W[p] their largest count; m's row is per p a block of
    W[p] columns (its inserted residues right-justified for p = 0, left-justified otherwise), then its residue under p or '-'"""
    L = len(center)
    ins, under = [], []
    for s, (n_cols, gap1, gap2) in zip(members, records):
        mine, und, p, k = [[] for _ in range(L + 1)], [None] * L, 0, 0
        for c in range(n_cols):
            if gap1 >> c & 1:
                mine[p].append(s[k])
                k += 1
            elif gap2 >> c & 1:
                und[p] = "-"
                p += 1
            else:
                und[p] = s[k]
                k, p = k + 1, p + 1
        assert p == L and k == len(s)
        ins.append(mine)
        under.append(und)
    W = [0] * (L + 1)
    for mine in ins:
        for p in range(L + 1):
            W[p] = max(W[p], len(mine[p]))

    def build(mine, und):
        out = ""
        for p in range(L + 1):
            block = "".join(mine[p])
            fill = "-" * (W[p] - len(block))
            out += fill + block if p == 0 else block + fill
            if p < L:
                out += und[p]
        return out

    return build([[] for _ in range(L + 1)], list(center)), [build(a, b) for a, b in zip(ins, under)]


# ---- the GPU tests' inputs ------------------------------------------------------------------------------------------------------------

LENGTHS = (1, 2, 3, 7, 8, 9, 12, 15, 16, 17, 24, 32)


def asym_matrix():
    """blosum62 with its upper triangle lowered by (row + column) mod 3: M[a][b] != M[b][a] for most a != b"""
    M = np.array(GE.blosum62())
    a, b = np.triu_indices(24, 1)
    M[a, b] -= (a + b) % 3
    assert not (M == M.T).all()
    return M


# name -> (matrix, gap_open, gap_extend, the letters its sequences are drawn from)
@functools.lru_cache(maxsize=None)
def family(name):
    if name == "blosum":
        return GE.blosum62(), -5, -1, tuple(range(20))
    if name == "edit":
        return edit_matrix(), -1, -1, (0, 1, 2, 3)
    if name == "zero":
        return GE.blosum62(), 0, 0, tuple(range(20))
    if name == "asym":
        return asym_matrix(), -3, -3, tuple(range(20))
    if name == "lit1000":   # entries of +-1000: W / W, B / B, W / B and C against D, E, N, Q
        return GE.matrix("lit1000"), -127, -127, (GE.W, GE.B, GE.C_) + GE.LOW + (0, 10)
    raise KeyError(name)


FAMILIES = ("blosum", "edit", "zero", "asym", "lit1000")


@functools.lru_cache(maxsize=None)
def sequences(name):
    """48 sequences, four of each of LENGTHS, ordered by length: of each four the first is random, the others are the first with a
    residue changed, a block moved, or the previous length's first sequence grown at random places -- relatives, so that gaps
    and ties take part in the optima"""
    letters = np.asarray(family(name)[3], dtype=np.uint8)
    rng = np.random.default_rng(2800 + FAMILIES.index(name))
    out, prev = [], None
    for L in LENGTHS:
        base = letters[rng.integers(0, len(letters), L)]
        sub = base.copy()
        sub[int(rng.integers(0, L))] = letters[int(rng.integers(0, len(letters)))]
        cut = int(rng.integers(0, L))
        moved = np.concatenate([base[cut:], base[:cut]])
        grown = letters[rng.integers(0, len(letters), L)]
        if prev is not None:   # the previous length's first sequence with random residues let in
            keep = np.sort(rng.choice(L, len(prev), replace=False))
            grown[keep] = prev
        out += [base, sub, moved, grown]
        prev = base
    for s in out:
        s.setflags(write=False)
    return tuple(out)


CAPS = (32, 24, 16)   # the kernel has an instantiation for sets of at most 16, 24 and 32 residues


def capped(seqs, cap):
    """the same sequences, those beyond `cap` residues cut to it (32: the set itself): the pairs of two sequences within the cap are
    common to both sets"""
    return tuple(s[:cap] for s in seqs)


def all_pairs(n):
    i, j = np.divmod(np.arange(n * n, dtype=np.uint32), np.uint32(n))
    return i.astype(np.uint32), j.astype(np.uint32)


@functools.lru_cache(maxsize=None)
def _reference(name, cap):
    """one pass over all ordered pairs: the tables of a pair once, the rule's walk and (full set only) every slipped walk on them"""
    M, go, ge, _ = family(name)
    Ml = [[int(v) for v in row] for row in np.asarray(M)]
    seqs = capped(sequences(name), cap)
    sl = [[int(v) for v in s] for s in seqs]
    n = len(sl)
    rec = [[None] * n for _ in range(n)]
    differ = {slip: 0 for slip in SLIPS}
    for a in range(n):
        for b in range(n):
            T = tables(sl[a], sl[b], Ml, go, ge)
            rec[a][b] = walk(sl[a], sl[b], Ml, go, ge, None, T)
            if cap == 32:
                for slip in SLIPS:
                    if slip != "swapped" and walk(sl[a], sl[b], Ml, go, ge, slip, T) != rec[a][b]:
                        differ[slip] += 1
    differ["swapped"] = sum(1 for a in range(n) for b in range(n) if rec[a][b] != rec[b][a])   # (the slip's record of (a, b) is (b, a)'s)
    flat = [rec[a][b] for a in range(n) for b in range(n)]
    out = tuple(np.array([r[f] for r in flat], dtype=t) for f, t in enumerate((np.int32, np.uint8, np.uint64, np.uint64)))
    for arr in out:
        arr.setflags(write=False)
    return out, differ


def expected(name, cap=32):
    """the reference records (score, n_cols, gap1, gap2) of all ordered pairs (pair a * n + b: seq1 = a, seq2 = b) of sequences(name)
    cut to `cap` residues; computed once, read-only"""
    return _reference(name, cap)[0]


def slip_counts(name):
    """slip -> on how many pairs of sequences(name) the slipped walk's record differs from the rule's"""
    return dict(_reference(name, 32)[1])
