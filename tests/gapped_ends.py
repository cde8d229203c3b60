"""Matrices, words and sets of tests/test_gapped_ends.py: inputs that take the gapped scorers (LocalAlignmentScorer, k_local.hip;
GlobalAlignmentScorer, k_global.hip) to the ends of their score fields, of their tiers and of their strips.  Everything is built on
lane_model.with_synonyms(blosum62): B is a distinct residue that scores like W against every other residue; W / B is planted one below
W / W, so the words over {W, B} are near the top and only a word's twin (a second copy under its own index) is at it.  Nothing here is imported from the planner or the kernels; every builder is deterministic (fixed seeds) and
cached, so the tests of one module share one copy."""
import functools
import json
import os

import numpy as np

import lane_model as LM

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
W, B, C_ = LM.code("W"), LM.code("B"), LM.code("C")
LOW = tuple(LM.code(c) for c in "DENQ")   # C against each of them (both ways) holds a matrix's lowest planted entry

# name -> (W/W and B/B, W/B, B/W, C vs D, E, N, Q both ways)
ENTRIES = {
    "reg127": (127, 126, 126, -127),
    "reg127a": (127, 127, -127, -127),
    "lit128": (128, 126, 126, -127),
    "litm128": (127, 126, 126, -128),
    "lit1000": (1000, 999, 999, -1000),
    "lit1000a": (1000, 999, -1000, -1000),   # the asymmetric variant of lit1000: seq1 = W^30, seq2 = W^29 B still scores 29,999
    "enc31": (31, 30, 30, -31),
    "enc32": (32, 30, 30, -31),
    "encm32": (31, 30, 30, -32),
}


@functools.lru_cache(maxsize=None)
def blosum62():
    with open(os.path.join(GOLDEN, "matrices.json")) as fh:
        M = np.asarray(json.load(fh)["matrices"]["blosum62"], dtype=np.int32)
    M.setflags(write=False)
    return M


@functools.lru_cache(maxsize=None)
def matrix(name):
    """a read-only int32 [24, 24]; "blosum62" is the plain matrix, every other name is ENTRIES planted into with_synonyms(blosum62)"""
    if name == "blosum62":
        return blosum62()
    top, wb, bw, low = ENTRIES[name]
    M = LM.with_synonyms(blosum62())
    M[W, W] = M[B, B] = top
    M[W, B], M[B, W] = wb, bw
    for y in LOW:
        M[C_, y] = M[y, C_] = low
    assert M.max() == top and M.min() == low
    M.setflags(write=False)
    return M


def symmetric(name):
    M = matrix(name)
    return bool((M == M.T).all())


# ---- words --------------------------------------------------------------------------------------------------------------------------

def run(residue, L):
    return np.full(L, residue, dtype=np.uint8)


def w_run_b(L):
    """W^(L-1) B"""
    w = run(W, L)
    w[-1] = B
    return w


def top_words(L, count, rng):
    """distinct words over {W, B}: W^L, W^(L-1) B, then random ones (at most 2^L exist)"""
    out = [run(W, L), w_run_b(L)]
    seen = {w.tobytes() for w in out}
    while len(out) < min(count, 2 ** L):
        w = np.where(rng.integers(0, 2, L) == 1, B, W).astype(np.uint8)
        if w.tobytes() not in seen:
            seen.add(w.tobytes())
            out.append(w)
    return out[:max(count, 2)]


def bottom_words(L, count, rng):
    """C^L, D^L, then random words over {D, E, N, Q}"""
    out = [run(C_, L), run(LOW[0], L)]
    seen = {w.tobytes() for w in out}
    while len(out) < min(count, 1 + 4 ** L):
        w = np.asarray(LOW, dtype=np.uint8)[rng.integers(0, 4, L)]
        if w.tobytes() not in seen:
            seen.add(w.tobytes())
            out.append(w)
    return out


def variants(w, rng, max_len):
    """one-edit variants of w: a substitution, an insertion (if it fits max_len) and a deletion (if a residue is left), so that
    gaps take part in the optimum of (w, variant)"""
    out = []
    s = w.copy()
    pos = int(rng.integers(0, len(w)))
    s[pos] = (int(s[pos]) + 1 + int(rng.integers(0, 19))) % 20
    out.append(s)
    if len(w) < max_len:
        out.append(np.insert(w, int(rng.integers(0, len(w) + 1)), int(rng.integers(0, 20))).astype(np.uint8))
    if len(w) > 1:
        out.append(np.delete(w, int(rng.integers(0, len(w)))))
    return out


class Pool:
    """an ordered collection of words, distinct but for the twins"""

    def __init__(self):
        self.words, self.seen = [], set()

    def add(self, words, only_len=None, not_len=None):
        for w in words:
            w = np.asarray(w, dtype=np.uint8)
            if (only_len is not None and len(w) != only_len) or (not_len is not None and len(w) == not_len):
                continue
            if w.tobytes() not in self.seen:
                self.seen.add(w.tobytes())
                self.words.append(w)

    def twin(self, w):
        """a second copy of w under an index of its own: the only way a pair of two sequences scores what w scores against itself
        when no other word does (W / B is one below W / W)"""
        self.words.append(np.array(w, dtype=np.uint8))

    def count(self, L):
        return sum(1 for w in self.words if len(w) == L)


def ends_words(pool, L, rng, n_top, n_bottom, n_ord, max_len, only_len=None, not_len=None, var_from=5):
    """top, bottom and ordinary words of length L and one-edit variants of the first `var_from` of (an ordinary word, W^(L-1) B, C^L,
    D^L, W^L)"""
    tops, bottoms = top_words(L, n_top, rng), bottom_words(L, n_bottom, rng)
    ords = LM.ordinary(rng, n_ord, [L], avoid=pool.words)
    var = [v for w in (ords[0], tops[1], bottoms[0], bottoms[1], tops[0])[:var_from] for v in variants(w, rng, max_len)]
    pool.add(tops + bottoms + ords + var, only_len=only_len, not_len=not_len)


def frozen(rng, pool):
    words = [pool.words[k] for k in rng.permutation(len(pool.words))]
    for w in words:
        w.setflags(write=False)
    return tuple(words)


# ---- sets ---------------------------------------------------------------------------------------------------------------------------

N13 = 260   # 17 row chunks of 16, the last of 4 rows; one more than a 256-column batch


@functools.lru_cache(maxsize=None)
def short16():
    """every length 1..16 with at least 6 sequences each, exactly N13 13-mers, nothing longer than 16; in a shuffled order"""
    rng = np.random.default_rng(1601)
    pool = Pool()
    for L in range(1, 17):
        if L != 13:
            ends_words(pool, L, rng, 2, 2, 2, 16, not_len=13, var_from=1)
            while pool.count(L) < 6:
                pool.add(LM.ordinary(rng, 1, [L], avoid=pool.words))
    ends_words(pool, 13, rng, 40, 40, 40, 16, only_len=13)
    pool.twin(run(W, 13))
    pool.twin(run(W, 16))
    for L in (12, 14):   # their insertions / deletions that are 13-mers
        for w in [w for w in pool.words if len(w) == L][:6]:
            pool.add(variants(w, rng, 16), only_len=13)
    while pool.count(13) < N13:
        for w in [w for w in pool.words if len(w) == 13][:N13 - pool.count(13)]:
            pool.add(variants(w, rng, 16)[:1])
    words = frozen(rng, pool)
    assert max(len(w) for w in words) == 16 and sum(1 for w in words if len(w) == 13) == N13
    return words


@functools.lru_cache(maxsize=None)
def short17():
    """short16 and one 17-mer behind it: the same pairs at the same indices, on the kernel for sets longer than 16"""
    extra = w_run_b(17)
    extra.setflags(write=False)
    return short16() + (extra,)


LONG_LENGTHS = (1, 2, 3, 5, 10, 15, 20, 29, 30, 31, 32)   # la & 3 = 1, 2, 3, 1, 2, 3, 0, 1, 2, 3, 0


@functools.lru_cache(maxsize=None)
def long32():
    rng = np.random.default_rng(3201)
    pool = Pool()
    for L in LONG_LENGTHS:
        rich = L in (30, 32)
        ends_words(pool, L, rng, 6 if rich else 2, 6 if rich else 2, 6 if rich else 4, 32, var_from=5 if rich else 1)
        if rich:
            pool.twin(run(W, L))
    words = frozen(rng, pool)
    assert max(len(w) for w in words) == 32 and len(words) >= 120
    return words


LOCAL_MAX = (12, 13, 20, 21, 32)   # the local kernels' buckets are <= 12, <= 20, <= 32: each bucket's last length and the next one


@functools.lru_cache(maxsize=None)
def local_lens(longest):
    """a set whose longest sequence is exactly `longest`: the four lengths up to it (la & 3 = 1, 2, 3, 0 in some order) with top,
    bottom, ordinary and variant words, and a few short sequences"""
    rng = np.random.default_rng(4000 + longest)
    pool = Pool()
    for L in range(longest - 3, longest + 1):
        ends_words(pool, L, rng, 4, 4, 8, longest)
    for L in (1, 2, 5):
        ends_words(pool, L, rng, 2, 2, 2, longest)
    pool.twin(run(W, longest))
    words = frozen(rng, pool)
    assert max(len(w) for w in words) == longest
    assert {len(w) & 3 for w in words if len(w) > longest - 4} == {0, 1, 2, 3}
    return words


def indices_of(words, w, copies=1):
    """the indices of word w in the set: exactly `copies` of them"""
    key = np.asarray(w, dtype=np.uint8).tobytes()
    hits = [k for k, v in enumerate(words) if v.tobytes() == key]
    assert len(hits) == copies, (key, hits)
    return hits
