"""The reference of tests/test_global.py: GlobalAlignmentScorer (include/hammock_hip.h, hmk_score_pairs_global) restated three
ways -- plain loops over the recurrence, a brute force over every alignment (lengths <= 6), and the recurrence vectorised with
numpy over the pairs of one (la, lb) class.  Sequences are sequences of residue indices; M is indexed [seq1 residue][seq2
residue]; penalties are added (<= 0).  All integers, every comparison exact."""
import numpy as np

NEG = -(1 << 40)   # -infinity (Python / int64: nothing wraps)


def global_score(s1, s2, M, gap_open, gap_extend):
    """the recurrence, cell by cell"""
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
        for j in range(1, m + 1):
            E[i][j] = max(E[i][j - 1] + gap_extend, H[i][j - 1] + gap_open)
            F[i][j] = max(F[i - 1][j] + gap_extend, H[i - 1][j] + gap_open)
            H[i][j] = max(H[i - 1][j - 1] + int(M[s1[i - 1]][s2[j - 1]]), E[i][j], F[i][j])
    return H[n][m]


def brute_force(s1, s2, M, gap_open, gap_extend):
    """the best of ALL alignments, enumerated one by one (no table): a column pairs two residues, or puts a residue of seq1 or of
    seq2 against a gap; a run of k gap columns of one kind costs gap_open + (k - 1) gap_extend"""
    n, m = len(s1), len(s2)
    assert n <= 6 and m <= 6

    def best(i, j, last):   # last: 0 pair / start, 1 gap against seq1's residue, 2 gap against seq2's residue
        if i == n and j == m:
            return 0
        out = NEG
        if i < n and j < m:
            out = max(out, int(M[s1[i]][s2[j]]) + best(i + 1, j + 1, 0))
        if i < n:
            out = max(out, (gap_extend if last == 1 else gap_open) + best(i + 1, j, 1))
        if j < m:
            out = max(out, (gap_extend if last == 2 else gap_open) + best(i, j + 1, 2))
        return out

    return best(0, 0, 0)


def global_class(A, B, M, gap_open, gap_extend):
    """A: int array [na, la] (seq1s of one length), B: [nb, lb] (seq2s) -> int64 [na, nb] of global(seq1 = A[r], seq2 = B[c]):
    the recurrence with every cell an [na, nb] array"""
    A, B, M = np.asarray(A, dtype=np.int64), np.asarray(B, dtype=np.int64), np.asarray(M, dtype=np.int64)
    na, la = A.shape
    nb, lb = B.shape
    shape = (na, nb)
    Hprev = [np.full(shape, gap_open + (j - 1) * gap_extend if j else 0, dtype=np.int64) for j in range(lb + 1)]
    Fprev = [np.full(shape, NEG, dtype=np.int64) for _ in range(lb + 1)]
    for i in range(1, la + 1):
        Hcur = [np.full(shape, gap_open + (i - 1) * gap_extend, dtype=np.int64)]
        Fcur = [Hcur[0]]
        e = np.full(shape, NEG, dtype=np.int64)
        for j in range(1, lb + 1):
            e = np.maximum(e + gap_extend, Hcur[j - 1] + gap_open)
            f = np.maximum(Fprev[j] + gap_extend, Hprev[j] + gap_open)
            sub = M[A[:, i - 1][:, None], B[:, j - 1][None, :]]
            Hcur.append(np.maximum(Hprev[j - 1] + sub, np.maximum(e, f)))
            Fcur.append(f)
        Hprev, Fprev = Hcur, Fcur
    return Hprev[lb]


def global_table(seqs, M, gap_open, gap_extend, rows=None, cols=None):
    """int64 [len(rows), len(cols)] of global(seq1 = seqs[rows[r]], seq2 = seqs[cols[c]]), class by class (default: all x all)"""
    rows = np.arange(len(seqs)) if rows is None else np.asarray(rows)
    cols = np.arange(len(seqs)) if cols is None else np.asarray(cols)
    out = np.zeros((len(rows), len(cols)), dtype=np.int64)
    rl = np.array([len(seqs[k]) for k in rows])
    cl = np.array([len(seqs[k]) for k in cols])
    for la in np.unique(rl):
        ri = np.nonzero(rl == la)[0]
        A = np.array([seqs[rows[k]] for k in ri], dtype=np.int64).reshape(len(ri), la)
        for lb in np.unique(cl):
            ci = np.nonzero(cl == lb)[0]
            B = np.array([seqs[cols[k]] for k in ci], dtype=np.int64).reshape(len(ci), lb)
            out[np.ix_(ri, ci)] = global_class(A, B, M, gap_open, gap_extend)
    return out


def levenshtein(s1, s2):
    """the plain edit-distance DP (substitution, insertion, deletion: 1 each)"""
    n, m = len(s1), len(s2)
    D = list(range(m + 1))
    for i in range(1, n + 1):
        prev, D[0] = D[0], i
        for j in range(1, m + 1):
            cur = min(D[j] + 1, D[j - 1] + 1, prev + (s1[i - 1] != s2[j - 1]))
            prev, D[j] = D[j], cur
    return D[m]


def edit_matrix():
    """0 on the diagonal, -1 elsewhere: with penalties -1 / -1 the global score is minus the Levenshtein distance"""
    M = np.full((24, 24), -1, dtype=np.int32)
    np.fill_diagonal(M, 0)
    return M
