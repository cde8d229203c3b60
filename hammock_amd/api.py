"""Python host-side mirror of the reference's interfaces for the greedy path,
backed by libhammock_hip.so through ctypes.  Names, argument order and error
behaviour follow the Java classes (paths relative to
src/cz/krejciadam/hammock/ of the reference):

  UniqueSequence                UniqueSequence.java:19
  Cluster                       Cluster.java:21
  ShiftedScorer                 ShiftedScorer.java:12     (sequenceScore on the GPU)
  LocalAlignmentScorer          LocalAlignmentScorer.java:10
  HipGreedySequenceClusterer    drop-in for LimitedGreedySequenceClusterer.java:17
                                at Hammock.java:403

``Context`` is the thin 1:1 wrapper of the C ABI.  Nothing here computes a
score on the CPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as N

AMINO_ACIDS = "ARNDCQEGHILKMFPSTWYVBZX*"  # UniqueSequence.java:23-26
_NAME_TO_NUM = {c: i for i, c in enumerate(AMINO_ACIDS)}


class HammockException(Exception):
    """HammockException.java"""


class DataException(HammockException):
    """DataException.java -- e.g. "Shift too big" (ShiftedScorer.java:59-62)."""


class FileFormatException(HammockException):
    """FileFormatException.java"""


class DeviceError(HammockException):
    """HIP failure or no usable gfx950 device.  There is no CPU fallback."""


class ReferenceWouldCrash(HammockException):
    """The reference throws NullPointerException here
    (LimitedGreedySequenceClusterer.java:97/104/108, reported at Hammock.java:153-157)."""

    def __init__(self, msg, case=0, index=-1):
        super().__init__(msg)
        self.case = case
        self.index = index


SCAN_HIT_DTYPE = np.dtype([("query", np.uint32), ("target", np.uint32), ("score", np.int32), ("offset", np.int32)])


def _ptr(arr, ctype):
    return arr.ctypes.data_as(C.POINTER(ctype))


def encode(sequence: str) -> np.ndarray:
    """UniqueSequence.java:46-57: case-folded letters -> residue indices."""
    out = np.empty(len(sequence), dtype=np.uint8)
    for k, ch in enumerate(sequence.upper()):
        if ch not in _NAME_TO_NUM:
            raise FileFormatException(f"Error, character {sequence[k]} is not a valid letter from the amino acid alphabet code.")
        out[k] = _NAME_TO_NUM[ch]
    return out


def pack_sequences(seqs):
    """list of str / uint8 arrays -> (residues uint8, offsets uint32[n+1])."""
    arrs = [encode(s) if isinstance(s, str) else np.ascontiguousarray(s, dtype=np.uint8) for s in seqs]
    off = np.zeros(len(arrs) + 1, dtype=np.uint32)
    if arrs:
        off[1:] = np.cumsum([len(a) for a in arrs])
    res = np.concatenate(arrs).astype(np.uint8) if arrs else np.zeros(0, dtype=np.uint8)
    return np.ascontiguousarray(res), off


def edge_fields(edges: np.ndarray):
    """packed uint64 edges -> (x, m, score) arrays (HMK_EDGE_* of hammock_hip.h)."""
    e = np.asarray(edges, dtype=np.uint64)
    x = (e >> np.uint64(40)).astype(np.uint32)
    m = ((e >> np.uint64(16)) & np.uint64(0xFFFFFF)).astype(np.uint32)
    s = (e & np.uint64(0xFFFF)).astype(np.uint16).view(np.int16).astype(np.int32)
    return x, m, s


def pack_edges(x, m, score) -> np.ndarray:
    x = np.asarray(x, dtype=np.uint64)
    m = np.asarray(m, dtype=np.uint64)
    s = np.asarray(score, dtype=np.int64).astype(np.int16).view(np.uint16).astype(np.uint64)
    return (x << np.uint64(40)) | (m << np.uint64(16)) | s


def aligned_rows(seqs, column, width_of_slot):
    """The aligned rows of Context.cluster_align_shifted's result: per sequence column[k] times '-', the sequence, '-' up to
    width_of_slot[k] (the width of the sequence's slot: width[member_cluster]).  seqs: strings."""
    rows = []
    for s, c, w in zip(seqs, column, width_of_slot):
        c, w = int(c), int(w)
        if c + len(s) > w:
            raise ValueError(f"a sequence of {len(s)} residues at column {c} does not fit a width of {w}")
        rows.append("-" * c + s + "-" * (w - c - len(s)))
    return rows


def gapped_rows(s1, s2, n_cols, gap1, gap2):
    """The two aligned strings of one record of Context.align_pairs_global (seq1 = s1, seq2 = s2): column c (0 = leftmost) shows
    '-' in the first row where bit c of gap1 is set, '-' in the second where bit c of gap2 is set, else the next residue."""
    n_cols, gap1, gap2 = int(n_cols), int(gap1), int(gap2)
    if gap1 & gap2 or (gap1 | gap2) >> n_cols:
        raise ValueError("gap1 and gap2 share a column, or have a bit at or above n_cols")
    if n_cols - bin(gap1).count("1") != len(s1) or n_cols - bin(gap2).count("1") != len(s2):
        raise ValueError(f"a record of {n_cols} columns does not hold sequences of {len(s1)} and {len(s2)} residues")
    it1, it2 = iter(s1), iter(s2)
    row1 = "".join("-" if gap1 >> c & 1 else next(it1) for c in range(n_cols))
    row2 = "".join("-" if gap2 >> c & 1 else next(it2) for c in range(n_cols))
    return row1, row2


def star_rows(center, members, records):
    """The centre-star merge of gapped pair alignments: center a string of L residues, members strings, records[k] = (n_cols, gap1,
    gap2) of align_pairs_global(seq1 = center, seq2 = members[k]) -> (the centre's row, the members' rows), all of one width.
    With ins[k][p] = the columns of record k with a gap in the centre that stand before centre residue p (p = L: after the last)
    and W[p] = max over k of ins[k][p], the width is L + sum W.  A member's row is, for each p, a block of W[p] columns with its
    ins[k][p] inserted residues (right-justified for p = 0, left-justified otherwise, the rest '-'), then its residue under centre
    residue p or '-'.  The centre's row has '-' in every block."""
    L = len(center)
    blocks, under = [], []   # per member: the inserted residues before each p (L + 1 strings); the residue under each p (L)
    for s, (n_cols, gap1, gap2) in zip(members, records):
        r1, r2 = gapped_rows(center, s, n_cols, gap1, gap2)
        ins, und = [""] * (L + 1), []
        for a, b in zip(r1, r2):
            if a == "-":
                ins[len(und)] += b
            else:
                und.append(b)
        blocks.append(ins)
        under.append(und)
    W = [max([len(ins[p]) for ins in blocks], default=0) for p in range(L + 1)]

    def row(ins, und):
        out = []
        for p in range(L + 1):
            pad = "-" * (W[p] - len(ins[p]))
            out.append(pad + ins[p] if p == 0 else ins[p] + pad)
            if p < L:
                out.append(und[p])
        return "".join(out)

    return row([""] * (L + 1), list(center)), [row(i, u) for i, u in zip(blocks, under)]


def load_frequency_matrix(path):
    """A frequency matrix in the text format FileIOManager.loadFrequencyMatrix reads (FileIOManager.java:90-118): lines starting
    with '#' are comments, one header line of letters, then one tab-separated row of numbers per letter, in the header's order ->
    (frequency float64[20, 20] in the order of AMINO_ACIDS, [row letter j][column letter i]: what hmk_profile_params.frequency
    takes, and the header's letters as a string, which a background file follows)."""
    letters, rows = None, []
    with open(path) as fh:
        for raw in fh:
            line = raw.rstrip("\r\n")
            if line.startswith("#") or not line.strip():
                continue
            if letters is None:
                letters = [s.strip()[:1].upper() for s in line.split("\t")]
                continue
            try:
                rows.append([float(s) for s in line.split("\t")])
            except ValueError:
                raise FileFormatException(f"{path}: a row of the frequency matrix holds something that is not a number")
    if letters is None or sorted(letters) != sorted(AMINO_ACIDS[:20]):
        raise FileFormatException(f"{path}: the header line must name each of the 20 amino acids {AMINO_ACIDS[:20]} once")
    if len(rows) != 20 or any(len(r) != 20 for r in rows):
        raise FileFormatException(f"{path}: 20 rows of 20 numbers are expected after the header")
    pos = [_NAME_TO_NUM[c] for c in letters]
    freq = np.zeros((20, 20), dtype=np.float64)
    freq[np.ix_(pos, pos)] = np.asarray(rows, dtype=np.float64)
    return freq, "".join(letters)


def load_background(path, letters=AMINO_ACIDS[:20]):
    """One line of 20 numbers (tabs or blanks between them, '#' comment lines before it) in the order of `letters` -- the
    frequency file's header -> float64[20] in the order of AMINO_ACIDS."""
    with open(path) as fh:
        lines = [ln for ln in (raw.strip() for raw in fh) if ln and not ln.startswith("#")]
    try:
        values = [float(s) for s in lines[0].split()] if len(lines) == 1 else []
    except ValueError:
        values = []
    if len(values) != 20 or len(letters) != 20:
        raise FileFormatException(f"{path}: one line of 20 numbers is expected")
    bg = np.zeros(20, dtype=np.float64)
    bg[[_NAME_TO_NUM[c] for c in letters]] = values
    return bg


def profile_params(frequency, background=None, min_ic=1.2, max_gap_proportion=0.2, min_conserved_positions=0, allow_inner_gaps=False,
                   beta=200.0, sigma=10.0, scale=2.88539):
    """hmk_profile_params.  The defaults are the reference's (Hammock.minIc, maxGapProportion; Statistics.java:21-23) but for the
    background: None stands for 0.05 throughout, the equiprobable model the information content uses.  The reference's own table is
    Statistics.java:25-28; pass it to get Hammock's numbers."""
    P = N.ProfileParams()
    P.min_ic, P.max_gap_proportion = float(min_ic), float(max_gap_proportion)
    P.min_conserved_positions, P.allow_inner_gaps = int(min_conserved_positions), 1 if allow_inner_gaps else 0
    P.beta, P.sigma, P.scale = float(beta), float(sigma), float(scale)
    f = np.ascontiguousarray(np.asarray(frequency, dtype=np.float64).reshape(400))
    b = np.full(20, 0.05) if background is None else np.ascontiguousarray(np.asarray(background, dtype=np.float64).reshape(20))
    P.frequency[:] = f.tolist()
    P.background[:] = b.tolist()
    return P


class ProfileResult:
    """What Context.cluster_profile returns (hmk_cluster_profile): per slot width, n_conserved, n_match, passes, kld_match_mean,
    kld_all_mean, col_start[n_clusters + 1]; per column counts[columns, 21], ic, col_flags (None where not asked for); per member
    kld_match, kld_all; stats (hmk_profile_stats)."""
    __slots__ = ("width", "n_conserved", "n_match", "passes", "kld_match_mean", "kld_all_mean", "col_start", "counts", "ic", "col_flags",
                 "kld_match", "kld_all", "stats")

    def match_string(self, c):
        """slot c's match states, 'M' per match-state column and '.' per other one"""
        a, b = int(self.col_start[c]), int(self.col_start[c + 1])
        return "".join("M" if f & 2 else "." for f in self.col_flags[a:b])


# hmk_component_level, one entry per threshold of a components call
LEVEL_DTYPE = np.dtype([("n_edges", np.uint64), ("n_components", np.uint32), ("n_singletons", np.uint32), ("largest", np.uint32),
                        ("reserved", np.uint32)])

# hmk_greedy_level, one entry per threshold of a greedy sweep
GREEDY_LEVEL_DTYPE = np.dtype([("n_edges", np.uint64), ("status", np.int32), ("crash_case", np.int32), ("crash_index", np.int32),
                               ("phase1_stop_index", np.int32), ("phase1_clusters", np.int32), ("phase1_orphans", np.int32),
                               ("n_result_clusters", np.int32), ("n_multi", np.int32), ("n_singletons", np.uint32),
                               ("largest", np.uint32), ("tail_ms", np.float64)])

# hmk_greedy_order, one entry per order of a greedy orders call
GREEDY_ORDER_DTYPE = np.dtype([("status", np.int32), ("crash_case", np.int32), ("crash_index", np.int32),
                               ("phase1_stop_index", np.int32), ("phase1_clusters", np.int32), ("phase1_orphans", np.int32),
                               ("n_result_clusters", np.int32), ("n_multi", np.int32), ("n_singletons", np.uint32),
                               ("largest", np.uint32), ("pairs_together", np.uint64), ("pairs_with_first", np.uint64),
                               ("tail_ms", np.float64)])


class OrdersResult:
    """What Context.greedy_orders returns (hmk_greedy_orders): per_order (GREEDY_ORDER_DTYPE[n_orders]); cluster_id, result_order,
    member_rank (int32 (n_orders, n), by uploaded index, clusters named by their seed's uploaded index); partners_always,
    partners_ever, consensus (uint32[n]); support_edges (packed, the support in the score field); stats (hmk_greedy_orders_stats).
    None where an output was not asked for."""
    __slots__ = ("per_order", "cluster_id", "result_order", "member_rank", "partners_always", "partners_ever", "consensus",
                 "support_edges", "stats")


# hmk_representative_level, one entry per threshold of a representatives call
REPRESENTATIVE_LEVEL_DTYPE = np.dtype([("n_edges", np.uint64), ("n_representatives", np.uint32), ("n_isolated", np.uint32),
                                       ("largest", np.uint32), ("n_rounds", np.uint32), ("reserved", np.uint32, (2,))])

# hmk_density_level, one entry per threshold of a density call
DENSITY_LEVEL_DTYPE = np.dtype([("n_edges", np.uint64), ("n_core", np.uint32), ("n_border", np.uint32), ("n_noise", np.uint32),
                                ("n_clusters", np.uint32), ("largest", np.uint32), ("reserved", np.uint32)])
DENSITY_NOISE = 0xFFFFFFFF   # HMK_DENSITY_NOISE: cluster and anchor of a noise sequence


class Context:
    """1:1 wrapper of hmk_ctx.  device >= 0: HIP ordinal; -1: host-only."""

    def __init__(self, matrix, device=0):
        """device: a HIP ordinal, -1 (host only), or a list of ordinals (hmk_create_multi: the first is the root)."""
        self._h = C.c_void_p()
        self.matrix = np.ascontiguousarray(np.asarray(matrix, dtype=np.int32).reshape(24, 24))
        if isinstance(device, (list, tuple)):
            devs = (C.c_int * len(device))(*[int(d) for d in device])
            st = N.lib.hmk_create_multi(_ptr(self.matrix, C.c_int32), devs, len(device), C.byref(self._h))
            self.devices = [int(d) for d in device]
            device = self.devices[0] if self.devices else -1
        else:
            st = N.lib.hmk_create(_ptr(self.matrix, C.c_int32), int(device), C.byref(self._h))
            self.devices = [int(device)] if int(device) >= 0 else []
        if st:
            self._h = C.c_void_p()
            self._raise(st, None)
        self.device = device
        self.n = 0

    # -- errors -----------------------------------------------------------------
    def _raise(self, st, stats=None):
        msg = N.lib.hmk_last_error(self._h if self._h else None)
        msg = msg.decode() if msg else f"hmk status {st}"
        if st == N.HMK_ERR_SHIFT_TOO_BIG:
            raise DataException(msg)
        if st == N.HMK_ERR_REFERENCE_WOULD_CRASH:
            raise ReferenceWouldCrash(msg, getattr(stats, "crash_case", 0), getattr(stats, "crash_index", -1))
        if st in (N.HMK_ERR_DEVICE, N.HMK_ERR_OOM):
            raise DeviceError(msg)
        if st == N.HMK_ERR_CAPACITY:
            raise BufferError(msg)
        raise ValueError(msg)

    def last_kernel_ms(self):
        """device time of the probe kernel(s) of the last score_pairs_* / score_block_* call"""
        return float(N.lib.hmk_last_kernel_ms(self._h))

    def close(self):
        if getattr(self, "_h", None):
            N.lib.hmk_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- sequences ----------------------------------------------------------------
    def set_sequences(self, seqs=None, sizes=None, residues=None, offsets=None):
        if residues is None:
            residues, offsets = pack_sequences(seqs)
        residues = np.ascontiguousarray(residues, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint32)
        n = len(offsets) - 1
        sp = None
        if sizes is not None:
            sizes = np.ascontiguousarray(sizes, dtype=np.int32)
            sp = _ptr(sizes, C.c_int32)
        st = N.lib.hmk_set_sequences(self._h, _ptr(residues, C.c_uint8), _ptr(offsets, C.c_uint32), sp, n)
        if st:
            self._raise(st)
        self.n = n
        return self

    # -- scorers --------------------------------------------------------------------
    def _pairs(self, fn, i, j, a, b):
        i = np.ascontiguousarray(i, dtype=np.uint32)
        j = np.ascontiguousarray(j, dtype=np.uint32)
        if i.shape != j.shape:
            raise ValueError("i and j must have the same shape")
        out = np.empty(i.size, dtype=np.int32)
        st = fn(self._h, _ptr(i, C.c_uint32), _ptr(j, C.c_uint32), i.size, int(a), int(b), _ptr(out, C.c_int32))
        if st:
            self._raise(st)
        return out.reshape(i.shape)

    def score_pairs_shifted(self, i, j, max_shift, shift_penalty):
        return self._pairs(N.lib.hmk_score_pairs_shifted, i, j, max_shift, shift_penalty)

    def score_with_shift(self, i, j, max_shift, shift_penalty):
        """-> (score, shift) arrays: AligningSequenceScorer.scoreWithShift for every pair."""
        i = np.ascontiguousarray(i, dtype=np.uint32)
        j = np.ascontiguousarray(j, dtype=np.uint32)
        score = np.empty(i.size, dtype=np.int32)
        shift = np.empty(i.size, dtype=np.int32)
        st = N.lib.hmk_score_with_shift(self._h, _ptr(i, C.c_uint32), _ptr(j, C.c_uint32), i.size, int(max_shift),
                                        int(shift_penalty), _ptr(score, C.c_int32), _ptr(shift, C.c_int32))
        if st:
            self._raise(st)
        return score.reshape(i.shape), shift.reshape(i.shape)

    def score_pairs_local(self, i, j, gap_open, gap_extend):
        return self._pairs(N.lib.hmk_score_pairs_local, i, j, gap_open, gap_extend)

    def score_pairs_global(self, i, j, gap_open, gap_extend):
        """GlobalAlignmentScorer: out[k] = global(seq1 = i[k], seq2 = j[k]), Gotoh's global alignment score with the affine gap
        gap_open + (k - 1) gap_extend (penalties added; -127 <= gap_open <= gap_extend <= 0), end gaps charged."""
        return self._pairs(N.lib.hmk_score_pairs_global, i, j, gap_open, gap_extend)

    def align_pairs_global(self, i, j, gap_open, gap_extend):
        """The gapped alignments behind score_pairs_global (hmk_align_pairs_global; seq1 = i[k], seq2 = j[k]) -> (score int32,
        n_cols uint8, gap1 uint64, gap2 uint64), one entry per pair: bit c of gap1 / gap2 marks a gap in seq1 / seq2 in column c,
        column 0 the leftmost (gapped_rows builds the strings)."""
        i = np.ascontiguousarray(i, dtype=np.uint32)
        j = np.ascontiguousarray(j, dtype=np.uint32)
        if i.shape != j.shape:
            raise ValueError("i and j must have the same shape")
        score = np.empty(i.size, dtype=np.int32)
        n_cols = np.empty(i.size, dtype=np.uint8)
        gap1 = np.empty(i.size, dtype=np.uint64)
        gap2 = np.empty(i.size, dtype=np.uint64)
        st = N.lib.hmk_align_pairs_global(self._h, _ptr(i, C.c_uint32), _ptr(j, C.c_uint32), i.size, int(gap_open), int(gap_extend),
                                          _ptr(score, C.c_int32), _ptr(n_cols, C.c_uint8), _ptr(gap1, C.c_uint64), _ptr(gap2, C.c_uint64))
        if st:
            self._raise(st)
        return score.reshape(i.shape), n_cols.reshape(i.shape), gap1.reshape(i.shape), gap2.reshape(i.shape)

    def align_edges_global(self, edges, gap_open, gap_extend):
        """The alignments of the edges of neighbors_global / search_global: seq1 = the edge's m, seq2 = its x (the orientation of
        both calls' scores) -> (score, n_cols, gap1, gap2) in the edges' order.  Raises if a score differs from its edge's: the
        edges were made with other penalties, another matrix or other sequences."""
        x, m, s = edge_fields(edges)
        score, n_cols, gap1, gap2 = self.align_pairs_global(m, x, gap_open, gap_extend)
        bad = np.nonzero(score != s)[0]
        if bad.size:
            k = int(bad[0])
            raise ValueError(f"{bad.size} edge(s) carry another score than their alignment: edge {k} (m = {int(m[k])}, x = {int(x[k])}) "
                             f"has {int(s[k])}, the alignment scores {int(score[k])}")
        return score, n_cols, gap1, gap2

    def _block(self, fn, r0, r1, c0, c1, a, b):
        out = np.empty((max(r1 - r0, 0), max(c1 - c0, 0)), dtype=np.int32)
        st = fn(self._h, r0, r1, c0, c1, int(a), int(b), _ptr(out, C.c_int32))
        if st:
            self._raise(st)
        return out

    def score_block_shifted(self, r0, r1, c0, c1, max_shift, shift_penalty):
        return self._block(N.lib.hmk_score_block_shifted, r0, r1, c0, c1, max_shift, shift_penalty)

    def score_block_local(self, r0, r1, c0, c1, gap_open, gap_extend):
        return self._block(N.lib.hmk_score_block_local, r0, r1, c0, c1, gap_open, gap_extend)

    def score_block_global(self, r0, r1, c0, c1, gap_open, gap_extend):
        return self._block(N.lib.hmk_score_block_global, r0, r1, c0, c1, gap_open, gap_extend)

    # -- neighbour graph ----------------------------------------------------------------
    def _neighbors(self, fn, a, b, threshold, part, n_parts, capacity):
        """an all-vs-all pass into a host buffer, grown to the needed count on HMK_ERR_CAPACITY unless the caller fixed the capacity"""
        stats = N.NeighborStats()
        n_edges = C.c_uint64(0)
        cap = int(capacity) if capacity is not None else 1 << 20
        while True:
            buf = np.empty(max(cap, 1), dtype=np.uint64)
            st = fn(self._h, int(a), int(b), int(threshold), part, n_parts, _ptr(buf, C.c_uint64), cap, C.byref(n_edges), C.byref(stats))
            if st == N.HMK_ERR_CAPACITY and capacity is None and int(n_edges.value) > cap:
                cap = int(n_edges.value)
                continue
            if st:
                self._raise(st)
            return buf[:n_edges.value].copy(), stats

    def neighbors_shifted(self, max_shift, shift_penalty, threshold, part=0, n_parts=1, capacity=None):
        """-> (edges uint64[n_edges], NeighborStats)"""
        return self._neighbors(N.lib.hmk_neighbors_shifted, max_shift, shift_penalty, threshold, part, n_parts, capacity)

    def neighbors_local(self, gap_open, gap_extend, threshold, part=0, n_parts=1, capacity=None):
        """LocalAlignmentScorer, all ordered pairs >= threshold -> (edges uint64[n_edges], NeighborStats)"""
        return self._neighbors(N.lib.hmk_neighbors_local, gap_open, gap_extend, threshold, part, n_parts, capacity)

    def neighbors_global(self, gap_open, gap_extend, threshold, part=0, n_parts=1, capacity=None):
        """GlobalAlignmentScorer, pairs >= threshold -> (edges uint64[n_edges], NeighborStats): each unordered pair once (x < m)
        under a symmetric matrix, else all ordered pairs with score(seq1 = m, seq2 = x)"""
        return self._neighbors(N.lib.hmk_neighbors_global, gap_open, gap_extend, threshold, part, n_parts, capacity)

    # -- query-vs-reference search ------------------------------------------------------
    # Upload queries and references together once -- set_sequences(queries + references) -- and search the two index ranges:
    # only the Q x R pairs are scored (an all-vs-all pass over the union would score (Q + R)^2 / 2).  score(q, r) is
    # sequenceScore(seq1 = query, seq2 = reference); every edge comes out m = query, x = reference (edge_fields).
    def _search(self, fn, q0, q1, r0, r1, a, b, threshold, capacity):
        stats = N.NeighborStats()
        n_edges = C.c_uint64(0)
        cap = int(capacity) if capacity is not None else 1 << 20
        while True:
            buf = np.empty(max(cap, 1), dtype=np.uint64)
            st = fn(self._h, int(q0), int(q1), int(r0), int(r1), int(a), int(b), int(threshold), _ptr(buf, C.c_uint64), cap,
                    C.byref(n_edges), C.byref(stats))
            if st == N.HMK_ERR_CAPACITY and capacity is None and int(n_edges.value) > cap:
                cap = int(n_edges.value)
                continue
            if st:
                self._raise(st)
            return buf[:n_edges.value].copy(), stats

    def search_shifted(self, q0, q1, r0, r1, max_shift, shift_penalty, threshold, capacity=None):
        """Queries [q0, q1) against references [r0, r1) (disjoint ranges of the uploaded set), ShiftedScorer:
        -> (edges uint64[n_edges] with m = query, NeighborStats).  Typical use:
            ctx.set_sequences(queries + references)
            edges, stats = ctx.search_shifted(0, len(queries), len(queries), len(queries) + len(references), 3, 0, 20)"""
        return self._search(N.lib.hmk_search_shifted, q0, q1, r0, r1, max_shift, shift_penalty, threshold, capacity)

    def search_local(self, q0, q1, r0, r1, gap_open, gap_extend, threshold, capacity=None):
        """The same with LocalAlignmentScorer(seq1 = query, seq2 = reference) -> (edges uint64[n_edges], NeighborStats)"""
        return self._search(N.lib.hmk_search_local, q0, q1, r0, r1, gap_open, gap_extend, threshold, capacity)

    def search_global(self, q0, q1, r0, r1, gap_open, gap_extend, threshold, capacity=None):
        """The same with GlobalAlignmentScorer(seq1 = query, seq2 = reference) -> (edges uint64[n_edges], NeighborStats)"""
        return self._search(N.lib.hmk_search_global, q0, q1, r0, r1, gap_open, gap_extend, threshold, capacity)

    # -- scanning peptides along long targets ---------------------------------------------
    def set_targets(self, seqs=None, residues=None, offsets=None):
        """The second resident set: targets of HMK_MAX_LEN + 1 .. HMK_TARGET_MAX_LEN residues (strings or uint8 arrays, or
        concatenated residues with uint64 offsets[n + 1]).  Independent of set_sequences; an empty list clears them."""
        if residues is None:
            arrs = [encode(s) if isinstance(s, str) else np.asarray(s, dtype=np.uint8) for s in (seqs or [])]
            offsets = np.zeros(len(arrs) + 1, dtype=np.uint64)
            if arrs:
                offsets[1:] = np.cumsum([len(a) for a in arrs])
            residues = np.concatenate(arrs) if arrs else np.zeros(0, dtype=np.uint8)
        residues = np.ascontiguousarray(residues, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = max(len(offsets) - 1, 0)
        st = N.lib.hmk_set_targets(self._h, _ptr(residues, C.c_uint8) if n else None, _ptr(offsets, C.c_uint64) if n else None, n)
        if st:
            self._raise(st)
        self.n_targets = n
        self._target_offsets = offsets.copy() if n else np.zeros(1, dtype=np.uint64)
        return self

    def scan_shifted(self, q0, q1, t0, t1, max_shift, shift_penalty, threshold, all_windows=False, coverage=False, capacity=None):
        """Queries [q0, q1) slid along targets [t0, t1) as scoreWithShift(seq1 = query, seq2 = target) slides them
        -> (hits, ScanStats) or, with coverage, (hits, ScanStats, coverage_count uint32[], coverage_size uint64[]) per residue of
        the targets in the range.  hits: structured array (query, target, score, offset), one record per pair whose best window
        reaches the threshold (the smallest offset among ties) or, with all_windows, per window that does; order unspecified."""
        stats = N.ScanStats()
        off = getattr(self, "_target_offsets", np.zeros(1, dtype=np.uint64))
        total = int(off[t1] - off[t0]) if coverage and 0 <= t0 <= t1 < len(off) else 0
        cc = np.zeros(max(total, 1), dtype=np.uint32) if coverage else None
        cs = np.zeros(max(total, 1), dtype=np.uint64) if coverage else None
        cap = int(capacity) if capacity is not None else 1 << 16
        flags = N.HMK_SCAN_ALL_WINDOWS if all_windows else 0
        for attempt in (0, 1):   # at most one retry, with the count the first call reported
            buf = np.zeros(max(cap, 1), dtype=SCAN_HIT_DTYPE)
            st = N.lib.hmk_scan_shifted(self._h, int(q0), int(q1), int(t0), int(t1), int(max_shift), int(shift_penalty), int(threshold),
                                        flags, buf.ctypes.data_as(C.POINTER(N.ScanHit)), cap,
                                        _ptr(cc, C.c_uint32) if coverage else None, _ptr(cs, C.c_uint64) if coverage else None,
                                        C.byref(stats))
            if st == N.HMK_ERR_CAPACITY and capacity is None and attempt == 0 and int(stats.n_hits) > cap:
                cap = int(stats.n_hits)
                continue
            if st:
                self._raise(st, stats)
            hits = buf[:stats.n_hits].copy()
            return (hits, stats, cc[:total], cs[:total]) if coverage else (hits, stats)

    def search_best_shifted(self, q0, q1, r0, r1, max_shift, shift_penalty, threshold, k):
        """The best k (1..32) references of every query with score >= threshold, by score descending, then reference
        index ascending, selected on the device -> (index int64[nq, k] padded with -1, score int32[nq, k]); a padded
        slot's score is INT32_MIN.  The selection's device time is in last_search_stats.kernel_ms."""
        nq = max(int(q1) - int(q0), 0)
        idx = np.empty((nq, max(int(k), 1)), dtype=np.uint32)
        score = np.empty((nq, max(int(k), 1)), dtype=np.int32)
        nh = np.empty(max(nq, 1), dtype=np.uint32)
        stats = N.NeighborStats()
        st = N.lib.hmk_search_best_shifted(self._h, int(q0), int(q1), int(r0), int(r1), int(max_shift), int(shift_penalty),
                                           int(threshold), int(k), _ptr(idx, C.c_uint32), _ptr(score, C.c_int32),
                                           _ptr(nh, C.c_uint32), C.byref(stats))
        if st:
            self._raise(st)
        self.last_search_stats = stats
        out = idx.astype(np.int64)
        out[idx == np.uint32(0xFFFFFFFF)] = -1
        return out, score

    # -- assignment of new sequences to existing clusters ----------------------------------
    # Upload members and new sequences together once -- set_sequences(members + new, sizes=...) -- and classify every new
    # sequence against the frozen clusters (NearestClusterRunner / findNearestClusterParallel, ClinkageSequenceClusterer.java
    # :137-177, 243-294): score(m, x) = sequenceScore(seq1 = member, seq2 = new), the opposite of the search's orientation.
    # New sequences never see each other: two of them given the same cluster are not checked against each other.
    def _assign(self, fn, q0, q1, r0, r1, member_cluster, cluster_id, a, b, threshold, k):
        nq = max(int(q1) - int(q0), 0)
        mc = np.ascontiguousarray(np.asarray(member_cluster, dtype=np.int64).ravel())
        cid = np.ascontiguousarray(np.asarray(cluster_id, dtype=np.int64).ravel())
        if mc.size != max(int(r1) - int(r0), 0):
            raise ValueError(f"member_cluster has {mc.size} entries for the {int(r1) - int(r0)} members [r0, r1)")
        if (mc < 0).any() or (mc > 0xFFFFFFFF).any():
            raise ValueError("member_cluster holds values outside uint32")
        if (cid < -2 ** 31).any() or (cid >= 2 ** 31).any():
            raise ValueError("cluster_id holds values outside int32")
        mc = mc.astype(np.uint32)
        cid = cid.astype(np.int32)
        kk = max(int(k), 1)
        best = np.empty((nq, kk), dtype=np.uint32)
        score = np.empty((nq, kk), dtype=np.int32)
        nf = np.empty(max(nq, 1), dtype=np.uint32)
        stats = N.NeighborStats()
        st = fn(self._h, int(q0), int(q1), int(r0), int(r1), _ptr(mc, C.c_uint32), _ptr(cid, C.c_int32), int(cid.size), int(a), int(b),
                int(threshold), int(k), _ptr(best, C.c_uint32), _ptr(score, C.c_int32), _ptr(nf, C.c_uint32), C.byref(stats))
        if st:
            self._raise(st)
        self.last_assign_stats = stats
        return best, score, nf[:nq].copy()

    def assign_shifted(self, q0, q1, r0, r1, member_cluster, cluster_id, max_shift, shift_penalty, threshold, k=1):
        """New sequences [q0, q1) against the clusters of the members [r0, r1) (member r in slot member_cluster[r - r0],
        slot c with Java id cluster_id[c]), ShiftedScorer, complete linkage -> (best_cluster uint32[nq, k] = slots,
        best_score int32[nq, k], n_feasible uint32[nq]).  Feasible clusters rank by score descending, size() descending,
        cluster_id ascending; unused slots hold 0xFFFFFFFF / INT32_MIN; n_feasible counts all feasible clusters (0 =
        unassigned).  kernel_ms of last_assign_stats includes the aggregation and selection."""
        return self._assign(N.lib.hmk_assign_shifted, q0, q1, r0, r1, member_cluster, cluster_id, max_shift, shift_penalty, threshold, k)

    def assign_local(self, q0, q1, r0, r1, member_cluster, cluster_id, gap_open, gap_extend, threshold, k=1):
        """The same with LocalAlignmentScorer(seq1 = member, seq2 = new)."""
        return self._assign(N.lib.hmk_assign_local, q0, q1, r0, r1, member_cluster, cluster_id, gap_open, gap_extend, threshold, k)

    # -- match of query clusters to existing clusters -----------------------------------------
    # Upload both sides together once and rank, for every query cluster, the existing clusters every one of whose members scores at
    # or above the threshold against every query member (ClinkageClusterScorer.clusterScore(existing, query cluster),
    # ClinkageSequenceClusterer.java:263): the assignment with query clusters of any size.  Query clusters matched to the same
    # existing cluster are not checked against each other.
    def _match(self, fn, q0, q1, query_cluster, r0, r1, member_cluster, cluster_id, a, b, threshold, k):
        qc = np.ascontiguousarray(np.asarray(query_cluster, dtype=np.int64).ravel())
        if qc.size != max(int(q1) - int(q0), 0):
            raise ValueError(f"query_cluster has {qc.size} entries for the {int(q1) - int(q0)} query sequences [q0, q1)")
        if (qc < 0).any() or (qc > 0xFFFFFFFF).any():
            raise ValueError("query_cluster holds values outside uint32")
        mc = np.ascontiguousarray(np.asarray(member_cluster, dtype=np.int64).ravel())
        cid = np.ascontiguousarray(np.asarray(cluster_id, dtype=np.int64).ravel())
        if mc.size != max(int(r1) - int(r0), 0):
            raise ValueError(f"member_cluster has {mc.size} entries for the {int(r1) - int(r0)} members [r0, r1)")
        if (mc < 0).any() or (mc > 0xFFFFFFFF).any():
            raise ValueError("member_cluster holds values outside uint32")
        if (cid < -2 ** 31).any() or (cid >= 2 ** 31).any():
            raise ValueError("cluster_id holds values outside int32")
        nb = int(qc.max()) + 1 if qc.size else 0
        qc, mc, cid = qc.astype(np.uint32), mc.astype(np.uint32), cid.astype(np.int32)
        kk = max(int(k), 1)
        best = np.empty((nb, kk), dtype=np.uint32)
        score = np.empty((nb, kk), dtype=np.int32)
        nf = np.empty(max(nb, 1), dtype=np.uint32)
        stats = N.NeighborStats()
        st = fn(self._h, int(q0), int(q1), _ptr(qc, C.c_uint32), nb, int(r0), int(r1), _ptr(mc, C.c_uint32), _ptr(cid, C.c_int32), int(cid.size),
                int(a), int(b), int(threshold), int(k), _ptr(best, C.c_uint32), _ptr(score, C.c_int32), _ptr(nf, C.c_uint32), C.byref(stats))
        if st:
            self._raise(st)
        self.last_match_stats = stats
        return best, score, nf[:nb].copy()

    def match_clusters_shifted(self, q0, q1, query_cluster, r0, r1, member_cluster, cluster_id, max_shift, shift_penalty, threshold, k=1):
        """Query clusters (sequence x of [q0, q1) in query slot query_cluster[x - q0]; n_query_clusters = max + 1, every slot
        non-empty) against the clusters of the members [r0, r1) (as assign_shifted's), ShiftedScorer, complete linkage over both
        sides' members -> (best_cluster uint32[nb, k] = slots, best_score int32[nb, k], n_feasible uint32[nb]).  Ranked and padded
        as assign_shifted's, which it equals when every query slot holds one sequence.  kernel_ms of last_match_stats includes
        the pass, both aggregation levels and the selection."""
        return self._match(N.lib.hmk_match_clusters_shifted, q0, q1, query_cluster, r0, r1, member_cluster, cluster_id, max_shift,
                           shift_penalty, threshold, k)

    def match_clusters_local(self, q0, q1, query_cluster, r0, r1, member_cluster, cluster_id, gap_open, gap_extend, threshold, k=1):
        """The same with LocalAlignmentScorer(seq1 = member, seq2 = query)."""
        return self._match(N.lib.hmk_match_clusters_local, q0, q1, query_cluster, r0, r1, member_cluster, cluster_id, gap_open, gap_extend,
                           threshold, k)

    # -- continuing a greedy clustering with new sequences --------------------------------------
    # Upload members and new sequences together once -- set_sequences(members + new, sizes=...) -- and run the greedy's second loop
    # (LimitedGreedySequenceClusterer.java:59-67) over the new sequences in index order, seeded with the given clusters: a new
    # sequence that joins a cluster is a member for every later one.  New sequences never seed clusters (phase 1 does not run).
    def greedy_continue(self, q0, q1, r0, r1, member_cluster, cluster_id, max_shift, shift_penalty, threshold):
        """New sequences [q0, q1) into the clusters of the members [r0, r1) (member r in slot member_cluster[r - r0], slot c
        with Java id cluster_id[c]), ShiftedScorer, complete linkage, symmetric matrices only -> (joined int32[nq] = the slot or
        -1, member_rank int32[nq] = the position in Cluster.getSequences() or -1).  Statistics: last_continue_stats."""
        nq = max(int(q1) - int(q0), 0)
        mc = np.ascontiguousarray(np.asarray(member_cluster, dtype=np.int64).ravel())
        cid = np.ascontiguousarray(np.asarray(cluster_id, dtype=np.int64).ravel())
        if mc.size != max(int(r1) - int(r0), 0):
            raise ValueError(f"member_cluster has {mc.size} entries for the {int(r1) - int(r0)} members [r0, r1)")
        if (mc < 0).any() or (mc > 0xFFFFFFFF).any():
            raise ValueError("member_cluster holds values outside uint32")
        if (cid < -2 ** 31).any() or (cid >= 2 ** 31).any():
            raise ValueError("cluster_id holds values outside int32")
        mc = mc.astype(np.uint32)
        cid = cid.astype(np.int32)
        joined = np.empty(max(nq, 1), dtype=np.int32)
        rank = np.empty(max(nq, 1), dtype=np.int32)
        stats = N.ContinueStats()
        st = N.lib.hmk_greedy_continue(self._h, int(q0), int(q1), int(r0), int(r1), _ptr(mc, C.c_uint32), _ptr(cid, C.c_int32),
                                       int(cid.size), int(max_shift), int(shift_penalty), int(threshold), _ptr(joined, C.c_int32),
                                       _ptr(rank, C.c_int32), C.byref(stats))
        if st:
            self._raise(st)
        self.last_continue_stats = stats
        return joined[:nq].copy(), rank[:nq].copy()

    def neighbors_shifted_dev(self, max_shift, shift_penalty, threshold, part, n_parts, d_edges_ptr, capacity,
                              d_counts_ptr, stream=0):
        st = N.lib.hmk_neighbors_shifted_dev(self._h, int(max_shift), int(shift_penalty), int(threshold), part, n_parts,
                                             C.c_void_p(d_edges_ptr), int(capacity), C.c_void_p(d_counts_ptr),
                                             C.c_void_p(stream))
        if st:
            self._raise(st)

    def compact_edges_dev(self, d_edges_ptr, capacity, d_counts_ptr, d_out_ptr, out_capacity, d_total_ptr, stream=0):
        st = N.lib.hmk_compact_edges_dev(self._h, C.c_void_p(d_edges_ptr), int(capacity), C.c_void_p(d_counts_ptr),
                                         C.c_void_p(d_out_ptr), int(out_capacity), C.c_void_p(d_total_ptr),
                                         C.c_void_p(stream))
        if st:
            self._raise(st)

    def pack_rows_dev(self, d_edges_ptr, capacity, d_counts_ptr, threshold, d_row_start_ptr, d_adj_ptr, adj_capacity, stream=0):
        st = N.lib.hmk_pack_rows_dev(self._h, C.c_void_p(d_edges_ptr), int(capacity), C.c_void_p(d_counts_ptr), int(threshold),
                                     C.c_void_p(d_row_start_ptr), C.c_void_p(d_adj_ptr), int(adj_capacity), C.c_void_p(stream))
        if st:
            self._raise(st)

    def unpack_rows_dev(self, d_row_start_ptr, d_adj_ptr, threshold, d_edges_out_ptr, out_capacity, stream=0):
        st = N.lib.hmk_unpack_rows_dev(self._h, C.c_void_p(d_row_start_ptr), C.c_void_p(d_adj_ptr), int(threshold),
                                       C.c_void_p(d_edges_out_ptr), int(out_capacity), C.c_void_p(stream))
        if st:
            self._raise(st)

    def last_plan(self):
        stats = N.NeighborStats()
        st = N.lib.hmk_neighbors_last_plan(self._h, C.byref(stats))
        if st:
            self._raise(st)
        return stats

    def last_plan_shared(self):
        """-> (16-row tiles of the last plan, those whose second group takes the first group's merged key cells)"""
        paired, shared = C.c_uint32(0), C.c_uint32(0)
        st = N.lib.hmk_neighbors_last_plan_shared(self._h, C.byref(paired), C.byref(shared))
        if st:
            self._raise(st)
        return int(paired.value), int(shared.value)

    def last_plan_tables(self):
        """-> (tiles of the last plan that copy their tables from the plan, bytes of device memory those tables take)"""
        tiles, nbytes = C.c_uint32(0), C.c_uint64(0)
        st = N.lib.hmk_neighbors_last_plan_tables(self._h, C.byref(tiles), C.byref(nbytes))
        if st:
            self._raise(st)
        return int(tiles.value), int(nbytes.value)

    # -- greedy ---------------------------------------------------------------------------
    def greedy_cluster(self, max_shift, shift_penalty, threshold, max_clusters):
        """-> (cluster_id int32[n], result_order int32[n_result], GreedyStats)"""
        cid = np.full(max(self.n, 1), -1, dtype=np.int32)
        order = np.full(max(self.n, 1), -1, dtype=np.int32)
        self.member_rank = np.zeros(max(self.n, 1), dtype=np.int32)
        stats = N.GreedyStats()
        st = N.lib.hmk_greedy_cluster(self._h, int(max_shift), int(shift_penalty), int(threshold), int(max_clusters),
                                      _ptr(cid, C.c_int32), _ptr(order, C.c_int32),
                                      _ptr(self.member_rank, C.c_int32), C.byref(stats))
        if st:
            self._raise(st, stats)
        return cid[:self.n], order[:stats.n_result_clusters], stats

    def reserve(self, n_sequences):
        """hmk_reserve: sizes the buffers of a clustering call on n_sequences ahead of time (optional; the two a call needs
        last are obtained on a thread of their own and the call's CSR step waits for them)."""
        st = N.lib.hmk_reserve(self._h, int(n_sequences))
        if st:
            self._raise(st)

    def set_java_hashset(self, version):
        """hmk_set_java_hashset: 8 (default, Java 8+), 7 (JDK 7u6+) or 6 (JDK 6 / 7 before 7u6) -- whose HashSet iteration
        order the clinkage calls emulate for the chain starts and the returned list."""
        st = N.lib.hmk_set_java_hashset(self._h, int(version))
        if st:
            self._raise(st)

    def clinkage_cluster(self, max_shift, shift_penalty, threshold):
        """hmk_clinkage_cluster -> (cluster_id int32[n], result_order int32[n_result], ClinkageStats); member_rank in
        self.member_rank.  Sequences in LOAD order (clinkage mode does not sort)."""
        cid = np.full(max(self.n, 1), -1, dtype=np.int32)
        order = np.full(max(self.n, 1), -1, dtype=np.int32)
        self.member_rank = np.zeros(max(self.n, 1), dtype=np.int32)
        stats = N.ClinkageStats()
        st = N.lib.hmk_clinkage_cluster(self._h, int(max_shift), int(shift_penalty), int(threshold), _ptr(cid, C.c_int32),
                                        _ptr(order, C.c_int32), _ptr(self.member_rank, C.c_int32), C.byref(stats))
        if st == N.HMK_ERR_REFERENCE_WOULD_CRASH:
            raise ReferenceWouldCrash(N.lib.hmk_last_error(self._h).decode(), 0, -1)
        if st:
            self._raise(st)
        return cid[:self.n], order[:stats.n_result_clusters], stats

    def clinkage_from_edges(self, edges):
        """hmk_clinkage_from_edges: the nearest-neighbour chain on a given edge list (works on a host-only context)."""
        edges = np.ascontiguousarray(edges, dtype=np.uint64)
        cid = np.full(max(self.n, 1), -1, dtype=np.int32)
        order = np.full(max(self.n, 1), -1, dtype=np.int32)
        self.member_rank = np.zeros(max(self.n, 1), dtype=np.int32)
        stats = N.ClinkageStats()
        st = N.lib.hmk_clinkage_from_edges(self._h, _ptr(edges, C.c_uint64), edges.size, _ptr(cid, C.c_int32),
                                           _ptr(order, C.c_int32), _ptr(self.member_rank, C.c_int32), C.byref(stats))
        if st == N.HMK_ERR_REFERENCE_WOULD_CRASH:
            raise ReferenceWouldCrash(N.lib.hmk_last_error(self._h).decode(), 0, -1)
        if st:
            self._raise(st)
        return cid[:self.n], order[:stats.n_result_clusters], stats

    # -- merging given clusters by complete linkage ---------------------------------------
    @staticmethod
    def _merge_args(r0, r1, member_cluster, cluster_id):
        mc = np.ascontiguousarray(np.asarray(member_cluster, dtype=np.int64).ravel())
        if mc.size != max(int(r1) - int(r0), 0):
            raise ValueError(f"member_cluster has {mc.size} entries for the {int(r1) - int(r0)} members [r0, r1)")
        if (mc < 0).any() or (mc > 0xFFFFFFFF).any():
            raise ValueError("member_cluster holds values outside uint32")
        cid = None
        if cluster_id is not None:
            cid = np.ascontiguousarray(np.asarray(cluster_id, dtype=np.int64).ravel())
            if (cid < -2 ** 31).any() or (cid >= 2 ** 31).any():
                raise ValueError("cluster_id holds values outside int32")
            cid = cid.astype(np.int32)
        return mc.astype(np.uint32), cid

    def cluster_pairs_shifted(self, r0, r1, member_cluster, n_clusters, max_shift, shift_penalty, threshold, capacity=None):
        """hmk_cluster_pairs_shifted: the pairs of given clusters (members [r0, r1), member r in slot member_cluster[r - r0])
        that are feasible for each other -> packed pairs uint64[] (x = smaller slot, m = larger slot, score = the
        complete-linkage score; edge_fields unpacks them).  Statistics: last_merge_stats."""
        mc, _ = self._merge_args(r0, r1, member_cluster, None)
        cap = int(capacity) if capacity is not None else 1 << 16
        while True:
            buf = np.empty(max(cap, 1), dtype=np.uint64)
            n = C.c_uint64(0)
            stats = N.MergeStats()
            st = N.lib.hmk_cluster_pairs_shifted(self._h, int(r0), int(r1), _ptr(mc, C.c_uint32), int(n_clusters), int(max_shift),
                                                 int(shift_penalty), int(threshold), _ptr(buf, C.c_uint64), cap, C.byref(n), C.byref(stats))
            if st == N.HMK_ERR_CAPACITY and capacity is None:
                cap = int(n.value)
                continue
            if st:
                self._raise(st)
            self.last_merge_stats = stats
            return buf[:n.value].copy()

    def cluster_linkage_shifted(self, r0, r1, member_cluster, n_clusters, max_shift, shift_penalty, threshold, members=True):
        """hmk_cluster_linkage_shifted: the complete-linkage scores INSIDE given clusters (members [r0, r1), member r in slot
        member_cluster[r - r0]) -> (min_score int32[n_clusters], min_a, min_b uint32[n_clusters] -- the pair that attains it,
        min_a < min_b, indices of the uploaded set -- n_below uint64[n_clusters], member_min int32[r1 - r0], member_below
        uint32[r1 - r0]); the last two are None with members=False.  A slot is a complete-linkage cluster at these parameters
        iff its n_below is 0.  Statistics: last_linkage_stats."""
        mc, _ = self._merge_args(r0, r1, member_cluster, None)
        ncl = int(n_clusters)
        min_score = np.empty(max(ncl, 1), dtype=np.int32)
        min_a = np.empty(max(ncl, 1), dtype=np.uint32)
        min_b = np.empty(max(ncl, 1), dtype=np.uint32)
        n_below = np.empty(max(ncl, 1), dtype=np.uint64)
        member_min = np.empty(max(mc.size, 1), dtype=np.int32) if members else None
        member_below = np.empty(max(mc.size, 1), dtype=np.uint32) if members else None
        stats = N.LinkageStats()
        st = N.lib.hmk_cluster_linkage_shifted(self._h, int(r0), int(r1), _ptr(mc, C.c_uint32), ncl, int(max_shift), int(shift_penalty),
                                               int(threshold), _ptr(min_score, C.c_int32), _ptr(min_a, C.c_uint32), _ptr(min_b, C.c_uint32),
                                               _ptr(n_below, C.c_uint64), _ptr(member_min, C.c_int32) if members else None,
                                               _ptr(member_below, C.c_uint32) if members else None, C.byref(stats))
        if st:
            self._raise(st)
        self.last_linkage_stats = stats
        return (min_score[:ncl], min_a[:ncl], min_b[:ncl], n_below[:ncl],
                member_min[:mc.size] if members else None, member_below[:mc.size] if members else None)

    def cluster_align_shifted(self, r0, r1, member_cluster, n_clusters, max_shift, shift_penalty, sums=True):
        """hmk_cluster_align_shifted: a centre-star alignment of given clusters (members [r0, r1), member r in slot
        member_cluster[r - r0]) around their medoids, in the ungapped model of ShiftedScorer.scoreWithShift; not Clustal Omega's
        alignment -> (center uint32[n_clusters] -- the member with the largest sum of scores against the others, the smallest index
        among ties --, center_sum int64[n_clusters], width uint32[n_clusters], member_sum int64[r1 - r0] or None with sums=False,
        center_score int32[r1 - r0], shift int32[r1 - r0] -- scoreWithShift(seq1 = the centre, seq2 = the member); INT32_MAX and 0
        for a centre --, column uint32[r1 - r0]).  aligned_rows builds the strings.  Statistics: last_align_stats."""
        mc, _ = self._merge_args(r0, r1, member_cluster, None)
        ncl, nm = int(n_clusters), mc.size
        center = np.zeros(max(ncl, 1), dtype=np.uint32)
        center_sum = np.zeros(max(ncl, 1), dtype=np.int64)
        width = np.zeros(max(ncl, 1), dtype=np.uint32)
        member_sum = np.zeros(max(nm, 1), dtype=np.int64) if sums else None
        center_score = np.zeros(max(nm, 1), dtype=np.int32)
        shift = np.zeros(max(nm, 1), dtype=np.int32)
        column = np.zeros(max(nm, 1), dtype=np.uint32)
        stats = N.AlignStats()
        st = N.lib.hmk_cluster_align_shifted(self._h, int(r0), int(r1), _ptr(mc, C.c_uint32), ncl, int(max_shift), int(shift_penalty),
                                             _ptr(center, C.c_uint32), _ptr(center_sum, C.c_int64), _ptr(width, C.c_uint32),
                                             _ptr(member_sum, C.c_int64) if sums else None, _ptr(center_score, C.c_int32),
                                             _ptr(shift, C.c_int32), _ptr(column, C.c_uint32), C.byref(stats))
        if st:
            self._raise(st)
        self.last_align_stats = stats
        return (center[:ncl], center_sum[:ncl], width[:ncl], member_sum[:nm] if sums else None, center_score[:nm], shift[:nm], column[:nm])

    def cluster_profile(self, r0, r1, member_cluster, n_clusters, column, params, counts=True, ic=True, flags=True, col_capacity=None):
        """hmk_cluster_profile: what the reference reads from a cluster's alignment, for given clusters (members [r0, r1), member r
        in slot member_cluster[r - r0]) under the placement column[r - r0] -- cluster_align_shifted's column, or any ungapped
        placement -> ProfileResult.  params: profile_params(...).  counts / ic / flags = False: that per-column array is not
        fetched.  col_capacity=None sizes the per-column arrays from the call's own answer (a refused first call that touches no
        device); a number is passed on as it is, and BufferError then carries the needed count in .needed."""
        mc, _ = self._merge_args(r0, r1, member_cluster, None)
        ncl, nm = int(n_clusters), mc.size
        col = np.ascontiguousarray(np.asarray(column, dtype=np.int64).ravel())
        if col.size != nm:
            raise ValueError(f"column has {col.size} entries for the {nm} members [r0, r1)")
        if (col < 0).any() or (col > 0xFFFFFFFF).any():
            raise ValueError("column holds values outside uint32")
        col = col.astype(np.uint32)
        R = ProfileResult()
        R.width = np.zeros(max(ncl, 1), dtype=np.uint32)
        R.n_conserved = np.zeros(max(ncl, 1), dtype=np.uint32)
        R.n_match = np.zeros(max(ncl, 1), dtype=np.uint32)
        R.passes = np.zeros(max(ncl, 1), dtype=np.uint8)
        R.kld_match_mean = np.zeros(max(ncl, 1), dtype=np.float64)
        R.kld_all_mean = np.zeros(max(ncl, 1), dtype=np.float64)
        R.col_start = np.zeros(ncl + 1, dtype=np.uint64)
        R.kld_match = np.zeros(max(nm, 1), dtype=np.float64)
        R.kld_all = np.zeros(max(nm, 1), dtype=np.float64)
        stats = N.ProfileStats()
        want = counts or ic or flags

        def call(cap):
            R.counts = np.zeros((max(cap, 1), N.HMK_PROFILE_SYMBOLS), dtype=np.uint32) if counts else None
            R.ic = np.zeros(max(cap, 1), dtype=np.float64) if ic else None
            R.col_flags = np.zeros(max(cap, 1), dtype=np.uint8) if flags else None
            return N.lib.hmk_cluster_profile(self._h, int(r0), int(r1), _ptr(mc, C.c_uint32), ncl, _ptr(col, C.c_uint32), C.byref(params),
                                             _ptr(R.width, C.c_uint32), _ptr(R.n_conserved, C.c_uint32), _ptr(R.n_match, C.c_uint32),
                                             _ptr(R.passes, C.c_uint8), _ptr(R.kld_match_mean, C.c_double), _ptr(R.kld_all_mean, C.c_double),
                                             _ptr(R.col_start, C.c_uint64), cap, _ptr(R.counts, C.c_uint32) if counts else None,
                                             _ptr(R.ic, C.c_double) if ic else None, _ptr(R.col_flags, C.c_uint8) if flags else None,
                                             _ptr(R.kld_match, C.c_double), _ptr(R.kld_all, C.c_double), C.byref(stats))

        st = call(int(col_capacity) if col_capacity is not None else 0)
        if st == N.HMK_ERR_CAPACITY and col_capacity is None and want:
            st = call(int(stats.columns))
        if st == N.HMK_ERR_CAPACITY:
            try:
                self._raise(st)
            except BufferError as e:
                e.needed = int(stats.columns)
                raise
        if st:
            self._raise(st)
        ncols = int(stats.columns)
        for name in ("width", "n_conserved", "n_match", "passes", "kld_match_mean", "kld_all_mean"):
            setattr(R, name, getattr(R, name)[:ncl])
        R.kld_match, R.kld_all = R.kld_match[:nm], R.kld_all[:nm]
        R.counts = R.counts[:ncols] if counts else None
        R.ic = R.ic[:ncols] if ic else None
        R.col_flags = R.col_flags[:ncols] if flags else None
        R.stats = stats
        self.last_profile_stats = stats
        return R

    def score_survey_shifted(self, q0, q1, r0, r1, max_shift, shift_penalty, threshold, score_lo=None, n_bins=0, rows=True):
        """hmk_score_survey_shifted: the pair scores of the triangle inside one range ([q0, q1) == [r0, r1), seq1 = the larger index) or
        of the rectangle of two disjoint ranges (seq1 = the query), reduced on the device -> (hist uint64[n_bins] -- the pairs scoring
        score_lo + k -- or None with n_bins=0, (best_score int32[q1 - q0], best_index uint32[q1 - q0] -- the smallest partner attaining
        it --, degree uint32[q1 - q0] -- the partners at or above the threshold) or None with rows=False, stats); a row without
        partners has INT32_MIN, UINT32_MAX, 0.  score_lo=None stands for 0.  Statistics also in last_survey_stats."""
        nb, nq = int(n_bins), max(int(q1) - int(q0), 0)
        hist = np.zeros(nb, dtype=np.uint64) if nb else None
        best_score = np.zeros(max(nq, 1), dtype=np.int32) if rows else None
        best_index = np.zeros(max(nq, 1), dtype=np.uint32) if rows else None
        degree = np.zeros(max(nq, 1), dtype=np.uint32) if rows else None
        stats = N.SurveyStats()
        st = N.lib.hmk_score_survey_shifted(self._h, int(q0), int(q1), int(r0), int(r1), int(max_shift), int(shift_penalty), int(threshold),
                                            int(score_lo or 0), nb, _ptr(hist, C.c_uint64) if nb else None,
                                            _ptr(best_score, C.c_int32) if rows else None, _ptr(best_index, C.c_uint32) if rows else None,
                                            _ptr(degree, C.c_uint32) if rows else None, C.byref(stats))
        if st:
            self._raise(st)
        self.last_survey_stats = stats
        return hist, ((best_score[:nq], best_index[:nq], degree[:nq]) if rows else None), stats

    def cluster_separation_shifted(self, r0, r1, member_cluster, n_clusters, max_shift, shift_penalty, flags=True, clusters=True):
        """hmk_cluster_separation_shifted: how well given clusters (members [r0, r1), member r in slot member_cluster[r - r0]) are
        separated -> (own_sum int64[r1 - r0] -- the member's scores against the rest of its slot --, near_sum int64[r1 - r0],
        near_cluster uint32[r1 - r0] -- of the other slots the one with the largest mean score, the smallest slot among equal means,
        and the member's sum against it; 0 and UINT32_MAX with one slot --, misplaced uint8[r1 - r0] -- own mean strictly below the
        nearest mean -- or None with flags=False, cluster_misplaced uint32[n_clusters] and cluster_own_sum int64[n_clusters] or None
        with clusters=False).  Statistics: last_separation_stats."""
        mc, _ = self._merge_args(r0, r1, member_cluster, None)
        ncl, nm = int(n_clusters), mc.size
        own_sum = np.zeros(max(nm, 1), dtype=np.int64)
        near_sum = np.zeros(max(nm, 1), dtype=np.int64)
        near_cluster = np.zeros(max(nm, 1), dtype=np.uint32)
        misplaced = np.zeros(max(nm, 1), dtype=np.uint8) if flags else None
        cluster_misplaced = np.zeros(max(ncl, 1), dtype=np.uint32) if clusters else None
        cluster_own_sum = np.zeros(max(ncl, 1), dtype=np.int64) if clusters else None
        stats = N.SeparationStats()
        st = N.lib.hmk_cluster_separation_shifted(self._h, int(r0), int(r1), _ptr(mc, C.c_uint32), ncl, int(max_shift), int(shift_penalty),
                                                  _ptr(own_sum, C.c_int64), _ptr(near_sum, C.c_int64), _ptr(near_cluster, C.c_uint32),
                                                  _ptr(misplaced, C.c_uint8) if flags else None,
                                                  _ptr(cluster_misplaced, C.c_uint32) if clusters else None,
                                                  _ptr(cluster_own_sum, C.c_int64) if clusters else None, C.byref(stats))
        if st:
            self._raise(st)
        self.last_separation_stats = stats
        return (own_sum[:nm], near_sum[:nm], near_cluster[:nm], misplaced[:nm] if flags else None,
                cluster_misplaced[:ncl] if clusters else None, cluster_own_sum[:ncl] if clusters else None)

    def _merge_out(self, nm, ncl):
        merged = np.full(max(ncl, 1), -1, dtype=np.int32)
        order = np.full(max(ncl, 1), -1, dtype=np.int32)
        self.member_rank = np.zeros(max(nm, 1), dtype=np.int32)
        return merged, order, N.MergeStats()

    def clinkage_merge(self, r0, r1, member_cluster, cluster_id, max_shift, shift_penalty, threshold):
        """hmk_clinkage_merge: the reference's complete-linkage agglomeration started from the given clusters (members
        [r0, r1), member r in slot member_cluster[r - r0], slot c with Java id cluster_id[c]) -> (merged_id int32[n_clusters],
        result_order int32[n_result]); member_rank in self.member_rank[:r1 - r0], statistics in last_merge_stats."""
        mc, cid = self._merge_args(r0, r1, member_cluster, cluster_id)
        merged, order, stats = self._merge_out(mc.size, cid.size)
        st = N.lib.hmk_clinkage_merge(self._h, int(r0), int(r1), _ptr(mc, C.c_uint32), _ptr(cid, C.c_int32), int(cid.size), int(max_shift),
                                      int(shift_penalty), int(threshold), _ptr(merged, C.c_int32), _ptr(order, C.c_int32),
                                      _ptr(self.member_rank, C.c_int32), C.byref(stats))
        if st:
            self._raise(st)
        self.last_merge_stats = stats
        self.member_rank = self.member_rank[:mc.size]
        return merged[:cid.size], order[:stats.n_result_clusters]

    def clinkage_merge_from_edges(self, edges, r0, r1, member_cluster, cluster_id):
        """hmk_clinkage_merge_from_edges: the same from a sequence-level edge list (works on a host-only context)."""
        edges = np.ascontiguousarray(edges, dtype=np.uint64)
        mc, cid = self._merge_args(r0, r1, member_cluster, cluster_id)
        merged, order, stats = self._merge_out(mc.size, cid.size)
        st = N.lib.hmk_clinkage_merge_from_edges(self._h, _ptr(edges, C.c_uint64), edges.size, int(r0), int(r1), _ptr(mc, C.c_uint32),
                                                 _ptr(cid, C.c_int32), int(cid.size), _ptr(merged, C.c_int32), _ptr(order, C.c_int32),
                                                 _ptr(self.member_rank, C.c_int32), C.byref(stats))
        if st:
            self._raise(st)
        self.last_merge_stats = stats
        self.member_rank = self.member_rank[:mc.size]
        return merged[:cid.size], order[:stats.n_result_clusters]

    # -- splitting given clusters by complete linkage -------------------------------------
    def _split(self, call, r0, mc, ncl):
        """runs call(outputs..., stats) -> (split_cluster uint32[nm], n_parts uint32[ncl], part_id int32[nm], member_rank int32[nm],
        part_order: one int32 array per slot); statistics in last_split_stats"""
        nm = mc.size
        split = np.zeros(max(nm, 1), dtype=np.uint32)
        n_parts = np.zeros(max(ncl, 1), dtype=np.uint32)
        part_id = np.zeros(max(nm, 1), dtype=np.int32)
        rank = np.zeros(max(nm, 1), dtype=np.int32)
        order = np.zeros(max(nm, 1), dtype=np.int32)
        start = np.zeros(ncl + 1, dtype=np.uint32)
        stats = N.SplitStats()
        st = call(_ptr(split, C.c_uint32), _ptr(n_parts, C.c_uint32), _ptr(part_id, C.c_int32), _ptr(rank, C.c_int32), _ptr(order, C.c_int32),
                  _ptr(start, C.c_uint32), C.byref(stats))
        if st == N.HMK_ERR_REFERENCE_WOULD_CRASH:
            raise ReferenceWouldCrash(N.lib.hmk_last_error(self._h).decode(), 0, int(stats.crash_slot))
        if st:
            self._raise(st)
        self.last_split_stats = stats
        n_parts = n_parts[:ncl]
        lists = [order[int(start[c]):int(start[c]) + int(n_parts[c])].copy() for c in range(ncl)] if nm else [order[:0] for _ in range(ncl)]
        return split[:nm], n_parts, part_id[:nm], rank[:nm], lists

    def clinkage_split(self, r0, r1, member_cluster, n_clusters, max_shift, shift_penalty, threshold):
        """hmk_clinkage_split: the reference's complete-linkage clustering run INSIDE each given cluster (members [r0, r1), member r
        in slot member_cluster[r - r0]) -> (split_cluster uint32[r1 - r0] -- the new clustering's member_cluster, with
        last_split_stats.n_result_clusters slots --, n_parts uint32[n_clusters], part_id int32[r1 - r0], member_rank int32[r1 - r0],
        part_order: per slot the int32 array of its returned ids in list order).  ReferenceWouldCrash.index is the slot."""
        mc, _ = self._merge_args(r0, r1, member_cluster, None)
        ncl = int(n_clusters)
        return self._split(lambda *out: N.lib.hmk_clinkage_split(self._h, int(r0), int(r1), _ptr(mc, C.c_uint32), ncl, int(max_shift),
                                                                 int(shift_penalty), int(threshold), *out), r0, mc, ncl)

    def clinkage_split_from_edges(self, edges, r0, r1, member_cluster, n_clusters):
        """hmk_clinkage_split_from_edges: the same from a sequence-level edge list (works on a host-only context)."""
        edges = np.ascontiguousarray(edges, dtype=np.uint64)
        mc, _ = self._merge_args(r0, r1, member_cluster, None)
        ncl = int(n_clusters)
        return self._split(lambda *out: N.lib.hmk_clinkage_split_from_edges(self._h, _ptr(edges, C.c_uint64), edges.size, int(r0), int(r1),
                                                                            _ptr(mc, C.c_uint32), ncl, *out), r0, mc, ncl)

    # -- connected components of the neighbour graph ---------------------------------------
    def _components(self, call, threshold, threshold_hi, component, levels):
        """runs call(threshold, threshold_hi, component, levels, stats) -> (component uint32[n] or None, levels: structured array
        LEVEL_DTYPE[threshold_hi - threshold + 1] or None); statistics in last_components_stats"""
        thr = int(threshold)
        hi = thr if threshold_hi is None else int(threshold_hi)
        comp = np.zeros(max(self.n, 1), dtype=np.uint32) if component else None
        lv = np.zeros(min(max(hi - thr + 1, 1), 256), dtype=LEVEL_DTYPE) if levels else None
        stats = N.ComponentsStats()
        st = call(thr, hi, _ptr(comp, C.c_uint32) if component else None,
                  lv.ctypes.data_as(C.POINTER(N.ComponentLevel)) if levels else None, C.byref(stats))
        if st:
            self._raise(st)
        self.last_components_stats = stats
        return (comp[:self.n] if component else None), lv

    def components_shifted(self, max_shift, shift_penalty, threshold, threshold_hi=None, component=True, levels=True):
        """hmk_components_shifted: the connected components of the graph {ShiftedScorer score >= t} over the uploaded set, for every
        t = threshold ... threshold_hi (None: threshold alone) from one scoring pass -> (component uint32[n]: the smallest index in
        i's component at `threshold`, levels: structured array (LEVEL_DTYPE) with the fields n_edges, n_components, n_singletons,
        largest, one entry per t).  component=False / levels=False pass NULL for that output and return None for it."""
        return self._components(lambda thr, hi, *out: N.lib.hmk_components_shifted(self._h, int(max_shift), int(shift_penalty), thr, hi, *out),
                                threshold, threshold_hi, component, levels)

    def components_from_edges(self, edges, threshold, threshold_hi=None, component=True, levels=True):
        """hmk_components_from_edges: the same from packed edges, by a sequential union-find on the host (works on a host-only context)."""
        edges = np.ascontiguousarray(edges, dtype=np.uint64)
        return self._components(lambda thr, hi, *out: N.lib.hmk_components_from_edges(self._h, _ptr(edges, C.c_uint64), edges.size, thr, hi, *out),
                                threshold, threshold_hi, component, levels)

    def components_from_edges_dev(self, d_edges_ptr, n_edges, threshold, threshold_hi=None, component=True, levels=True):
        """hmk_components_from_edges_dev: the same with the packed edges in device memory, through the device kernels."""
        return self._components(lambda thr, hi, *out: N.lib.hmk_components_from_edges_dev(self._h, C.c_void_p(d_edges_ptr), int(n_edges), thr, hi, *out),
                                threshold, threshold_hi, component, levels)

    # -- greedy clusterings at a range of thresholds -----------------------------------------
    def _greedy_sweep(self, call, threshold, threshold_hi, arrays, levels):
        """runs call(threshold, threshold_hi, cluster_id, result_order, member_rank, levels, stats) ->
        (levels: structured array GREEDY_LEVEL_DTYPE[n_levels] or None, cluster_id, result_order, member_rank: int32 (n_levels, n)
        each, or None); statistics in last_sweep_stats.  A level whose status is not 0 is one where the reference would throw: its
        rows are -1.  result_order's row of a level is valid up to that level's n_result_clusters, -1 behind."""
        thr = int(threshold)
        hi = thr if threshold_hi is None else int(threshold_hi)
        nl = min(max(hi - thr + 1, 1), 256)
        out = [np.full((nl, max(self.n, 1)), -1, dtype=np.int32) if arrays else None for _ in range(3)]
        lv = np.zeros(nl, dtype=GREEDY_LEVEL_DTYPE) if levels else None
        stats = N.GreedySweepStats()
        st = call(thr, hi, *[_ptr(a, C.c_int32) if arrays else None for a in out],
                  lv.ctypes.data_as(C.POINTER(N.GreedyLevel)) if levels else None, C.byref(stats))
        if st:
            self._raise(st)
        self.last_sweep_stats = stats
        if arrays and self.n == 0:
            out = [a[:, :0] for a in out]
        return (lv, *out)

    def greedy_sweep(self, max_shift, shift_penalty, threshold, threshold_hi, max_clusters, arrays=True, levels=True):
        """hmk_greedy_sweep: the greedy clustering of the uploaded set at every t = threshold ... threshold_hi from one scoring pass
        -> (levels, cluster_id, result_order, member_rank); row t - threshold is what greedy_cluster(..., t, max_clusters) gives.
        arrays=False / levels=False pass NULL for those outputs and return None for them."""
        return self._greedy_sweep(lambda thr, hi, *out: N.lib.hmk_greedy_sweep(self._h, int(max_shift), int(shift_penalty), thr, hi,
                                                                               int(max_clusters), *out),
                                  threshold, threshold_hi, arrays, levels)

    def greedy_sweep_from_edges(self, edges, symmetric, threshold, threshold_hi, max_clusters, arrays=True, levels=True):
        """hmk_greedy_sweep_from_edges: the same from packed edges, by the host merge per threshold (works on a host-only context)."""
        edges = np.ascontiguousarray(edges, dtype=np.uint64)
        return self._greedy_sweep(lambda thr, hi, *out: N.lib.hmk_greedy_sweep_from_edges(self._h, _ptr(edges, C.c_uint64), edges.size,
                                                                                          int(bool(symmetric)), thr, hi, int(max_clusters), *out),
                                  threshold, threshold_hi, arrays, levels)

    def greedy_sweep_from_edges_dev(self, d_edges_ptr, n_edges, symmetric, threshold, threshold_hi, max_clusters, arrays=True, levels=True):
        """hmk_greedy_sweep_from_edges_dev: the same with the packed edges in device memory, through the device kernels and tails."""
        return self._greedy_sweep(lambda thr, hi, *out: N.lib.hmk_greedy_sweep_from_edges_dev(self._h, C.c_void_p(d_edges_ptr), int(n_edges),
                                                                                              int(bool(symmetric)), thr, hi, int(max_clusters), *out),
                                  threshold, threshold_hi, arrays, levels)

    # -- greedy clusterings under many orders of the set ---------------------------------------
    def _greedy_orders(self, call, orders, min_support, arrays, per_order, support, support_capacity):
        """runs call(orders, n_orders, min_support, cluster_id, result_order, member_rank, per_order, partners_always, partners_ever,
        consensus, support_edges, capacity, n_support_edges, stats) -> OrdersResult; statistics also in last_orders_stats."""
        n = self.n
        orders = np.ascontiguousarray(orders, dtype=np.uint32)
        if orders.ndim == 1:
            orders = orders.reshape(1, -1)
        if orders.ndim != 2 or orders.shape[1] != n:
            raise ValueError(f"orders must be (n_orders, {n}): one permutation of the uploaded set per row")
        k = orders.shape[0]
        rows = [np.full((k, max(n, 1)), -1, dtype=np.int32) if arrays else None for _ in range(3)]
        po = np.zeros(max(k, 1), dtype=GREEDY_ORDER_DTYPE) if per_order else None
        pa, pe, cons = (np.zeros(max(n, 1), dtype=np.uint32) for _ in range(3))
        stats = N.GreedyOrdersStats()
        need = C.c_uint64(0)
        cap = 0 if not support else max(4 * n, 1024) if support_capacity is None else int(support_capacity)
        for attempt in range(2):
            sup = np.zeros(max(cap, 1), dtype=np.uint64) if support else None
            st = call(_ptr(orders, C.c_uint32) if orders.size or k else None, k, int(min_support),
                      *[_ptr(a, C.c_int32) if arrays else None for a in rows],
                      po.ctypes.data_as(C.POINTER(N.GreedyOrder)) if per_order else None,
                      _ptr(pa, C.c_uint32), _ptr(pe, C.c_uint32), _ptr(cons, C.c_uint32),
                      _ptr(sup, C.c_uint64) if support else None, cap, C.byref(need), C.byref(stats))
            if st == N.HMK_ERR_CAPACITY and support_capacity is None and attempt == 0 and int(need.value) > cap:
                cap = int(need.value)
                continue
            break
        self.last_orders_needed = int(need.value)
        if st:
            self._raise(st)
        self.last_orders_stats = stats
        r = OrdersResult()
        r.per_order = po[:k] if per_order else None
        r.cluster_id, r.result_order, r.member_rank = [a[:, :n] if arrays else None for a in rows]
        r.partners_always, r.partners_ever, r.consensus = pa[:n], pe[:n], cons[:n]
        r.support_edges = sup[:int(need.value)] if support else None
        r.stats = stats
        return r

    def greedy_orders(self, max_shift, shift_penalty, threshold, max_clusters, orders, min_support=0, arrays=True, per_order=True,
                      support=True, support_capacity=None):
        """hmk_greedy_orders: the greedy clustering of the uploaded set under every order of `orders` (uint32 (n_orders, n): row k
        names the uploaded index standing at each position of order k) from ONE scoring pass -> OrdersResult.  Rows are indexed by
        uploaded index and name a cluster by the uploaded index of its seed; an order whose status is not 0 is one where the
        reference would throw: its rows are -1 and it takes no part in the supports.  support_edges: every pair that shares a cluster
        in at least one valid order, packed (edge_fields), the support in the score field.  consensus: the components of the pairs
        with support >= min_support (0: every valid order).  arrays=False / per_order=False / support=False pass NULL for those
        outputs; support_capacity: the exact capacity to pass (BufferError when it is too small; last_orders_needed says how many)."""
        return self._greedy_orders(lambda *tail: N.lib.hmk_greedy_orders(self._h, int(max_shift), int(shift_penalty), int(threshold),
                                                                         int(max_clusters), *tail),
                                   orders, min_support, arrays, per_order, support, support_capacity)

    def greedy_orders_from_edges(self, edges, threshold, max_clusters, orders, min_support=0, arrays=True, per_order=True, support=True,
                                 support_capacity=None):
        """hmk_greedy_orders_from_edges: the same from packed edges (each unordered pair once, either orientation), by plain host code
        (works on a host-only context)."""
        edges = np.ascontiguousarray(edges, dtype=np.uint64)
        return self._greedy_orders(lambda *tail: N.lib.hmk_greedy_orders_from_edges(self._h, _ptr(edges, C.c_uint64), edges.size,
                                                                                    int(threshold), int(max_clusters), *tail),
                                   orders, min_support, arrays, per_order, support, support_capacity)

    # -- representatives: a non-redundant subset of the set -----------------------------------
    def _representatives(self, call, threshold, threshold_hi, arrays, levels):
        """runs call(threshold, threshold_hi, covered_by, nearest, nearest_score, levels, stats) -> (levels: structured array
        REPRESENTATIVE_LEVEL_DTYPE[n_levels] or None, covered_by uint32, nearest uint32, nearest_score int32: (n_levels, n) each, or
        None); statistics in last_representatives_stats.  arrays: True, False, or one flag per array."""
        thr = int(threshold)
        hi = thr if threshold_hi is None else int(threshold_hi)
        nl = min(max(hi - thr + 1, 1), 256)
        want = (bool(arrays),) * 3 if isinstance(arrays, (bool, int)) else tuple(bool(a) for a in arrays)
        kinds = (np.uint32, np.uint32, np.int32)
        out = [np.zeros((nl, max(self.n, 1)), dtype=k) if w else None for k, w in zip(kinds, want)]
        lv = np.zeros(nl, dtype=REPRESENTATIVE_LEVEL_DTYPE) if levels else None
        stats = N.RepresentativesStats()
        st = call(thr, hi, _ptr(out[0], C.c_uint32) if want[0] else None, _ptr(out[1], C.c_uint32) if want[1] else None,
                  _ptr(out[2], C.c_int32) if want[2] else None,
                  lv.ctypes.data_as(C.POINTER(N.RepresentativeLevel)) if levels else None, C.byref(stats))
        if st:
            self._raise(st)
        self.last_representatives_stats = stats
        if self.n == 0:
            out = [a[:, :0] if a is not None else None for a in out]
        return (lv, *out)

    def representatives_shifted(self, max_shift, shift_penalty, threshold, threshold_hi=None, arrays=True, levels=True):
        """hmk_representatives_shifted: the representatives of the uploaded set (i is one iff no representative r < i is its
        neighbour in {ShiftedScorer score >= t}) at every t = threshold ... threshold_hi (None: threshold alone) from one scoring pass
        -> (levels, covered_by, nearest, nearest_score); row t - threshold: covered_by[i] = i for a representative, else its
        smallest-index representative neighbour; nearest[i], nearest_score[i] = i, INT32_MAX for a representative, else the
        representative neighbour with the largest score and that score.  arrays=False / levels=False pass NULL and return None."""
        return self._representatives(lambda thr, hi, *out: N.lib.hmk_representatives_shifted(self._h, int(max_shift), int(shift_penalty), thr, hi, *out),
                                     threshold, threshold_hi, arrays, levels)

    def representatives_from_edges(self, edges, threshold, threshold_hi=None, arrays=True, levels=True):
        """hmk_representatives_from_edges: the same from packed edges read as an undirected graph, by the sequential definition on the
        host (works on a host-only context)."""
        edges = np.ascontiguousarray(edges, dtype=np.uint64)
        return self._representatives(lambda thr, hi, *out: N.lib.hmk_representatives_from_edges(self._h, _ptr(edges, C.c_uint64), edges.size, thr, hi, *out),
                                     threshold, threshold_hi, arrays, levels)

    def representatives_from_edges_dev(self, d_edges_ptr, n_edges, threshold, threshold_hi=None, arrays=True, levels=True):
        """hmk_representatives_from_edges_dev: the same with the packed edges in device memory, through the device kernels."""
        return self._representatives(lambda thr, hi, *out: N.lib.hmk_representatives_from_edges_dev(self._h, C.c_void_p(d_edges_ptr), int(n_edges), thr, hi, *out),
                                     threshold, threshold_hi, arrays, levels)

    # -- density clustering: core, border and noise sequences ----------------------------------
    def _density(self, call, threshold, threshold_hi, min_neighbors, arrays, levels):
        """runs call(threshold, threshold_hi, min_neighbors, cluster, anchor, degree, levels, stats) -> (levels: structured array
        DENSITY_LEVEL_DTYPE[n_levels] or None, cluster, degree, anchor: uint32 (n_levels, n) each, or None); statistics in
        last_density_stats.  arrays: True, False, or one flag per returned array (cluster, degree, anchor)."""
        thr = int(threshold)
        hi = thr if threshold_hi is None else int(threshold_hi)
        nl = min(max(hi - thr + 1, 1), 256)
        want = (bool(arrays),) * 3 if isinstance(arrays, (bool, int)) else tuple(bool(a) for a in arrays)
        cluster, degree, anchor = [np.zeros((nl, max(self.n, 1)), dtype=np.uint32) if w else None for w in want]
        lv = np.zeros(nl, dtype=DENSITY_LEVEL_DTYPE) if levels else None
        stats = N.DensityStats()
        st = call(thr, hi, int(min_neighbors), *[_ptr(a, C.c_uint32) if a is not None else None for a in (cluster, anchor, degree)],
                  lv.ctypes.data_as(C.POINTER(N.DensityLevel)) if levels else None, C.byref(stats))
        if st:
            self._raise(st)
        self.last_density_stats = stats
        out = [cluster, degree, anchor]
        if self.n == 0:
            out = [a[:, :0] if a is not None else None for a in out]
        return (lv, *out)

    def density_shifted(self, max_shift, shift_penalty, threshold, threshold_hi=None, min_neighbors=3, arrays=True, levels=True):
        """hmk_density_shifted: density clustering (DBSCAN on the graph {ShiftedScorer score >= t}, independent of any order) of the
        uploaded set at every t = threshold ... threshold_hi (None: threshold alone) from one scoring pass -> (levels, cluster,
        degree, anchor); row t - threshold: degree[i] = i's neighbours; i is core iff degree[i] >= min_neighbors; cluster[i] = the
        smallest core index of i's cluster (core-core edges only), for a border sequence its anchor's cluster, DENSITY_NOISE for
        noise; anchor[i] = i for a core sequence, for a border one its core neighbour with the largest score (the smaller index
        among equal scores), DENSITY_NOISE for noise.  arrays=False / levels=False pass NULL and return None."""
        return self._density(lambda thr, hi, mn, *out: N.lib.hmk_density_shifted(self._h, int(max_shift), int(shift_penalty), thr, hi, mn, *out),
                             threshold, threshold_hi, min_neighbors, arrays, levels)

    def density_from_edges(self, edges, threshold, threshold_hi=None, min_neighbors=3, arrays=True, levels=True):
        """hmk_density_from_edges: the same from packed edges (each unordered pair once; a pair given k times counts k times
        towards both degrees), by the definition on the host (works on a host-only context)."""
        edges = np.ascontiguousarray(edges, dtype=np.uint64)
        return self._density(lambda thr, hi, mn, *out: N.lib.hmk_density_from_edges(self._h, _ptr(edges, C.c_uint64), edges.size, thr, hi, mn, *out),
                             threshold, threshold_hi, min_neighbors, arrays, levels)

    def density_from_edges_dev(self, d_edges_ptr, n_edges, threshold, threshold_hi=None, min_neighbors=3, arrays=True, levels=True):
        """hmk_density_from_edges_dev: the same with the packed edges in device memory, through the device kernels."""
        return self._density(lambda thr, hi, mn, *out: N.lib.hmk_density_from_edges_dev(self._h, C.c_void_p(d_edges_ptr), int(n_edges), thr, hi, mn, *out),
                             threshold, threshold_hi, min_neighbors, arrays, levels)

    def greedy_phases(self):
        """hmk_greedy_last_phases: per-phase milliseconds of the last greedy_cluster / greedy_from_edges_dev call."""
        ph = N.GreedyPhases()
        st = N.lib.hmk_greedy_last_phases(self._h, C.byref(ph))
        if st:
            self._raise(st)
        return ph.as_dict()

    def greedy_from_edges(self, edges, symmetric, threshold, max_clusters):
        edges = np.ascontiguousarray(edges, dtype=np.uint64)
        cid = np.full(max(self.n, 1), -1, dtype=np.int32)
        order = np.full(max(self.n, 1), -1, dtype=np.int32)
        stats = N.GreedyStats()
        self.member_rank = np.zeros(max(self.n, 1), dtype=np.int32)
        st = N.lib.hmk_greedy_from_edges(self._h, _ptr(edges, C.c_uint64), edges.size, int(bool(symmetric)),
                                         int(threshold), int(max_clusters), _ptr(cid, C.c_int32),
                                         _ptr(order, C.c_int32), _ptr(self.member_rank, C.c_int32), C.byref(stats))
        if st:
            self._raise(st, stats)
        return cid[:self.n], order[:stats.n_result_clusters], stats

    def greedy_from_edges_dev(self, d_edges_ptr, n_edges, symmetric, max_clusters):
        """hmk_greedy_from_edges_dev: packed edges in device memory -> clusters (CSR built on the device)."""
        cid = np.full(max(self.n, 1), -1, dtype=np.int32)
        order = np.full(max(self.n, 1), -1, dtype=np.int32)
        stats = N.GreedyStats()
        self.member_rank = np.zeros(max(self.n, 1), dtype=np.int32)
        st = N.lib.hmk_greedy_from_edges_dev(self._h, C.c_void_p(d_edges_ptr), int(n_edges), int(bool(symmetric)),
                                             int(max_clusters), _ptr(cid, C.c_int32), _ptr(order, C.c_int32),
                                             _ptr(self.member_rank, C.c_int32), C.byref(stats))
        if st:
            self._raise(st, stats)
        return cid[:self.n], order[:stats.n_result_clusters], stats


# -----------------------------------------------------------------------------------------
# mirrors of the reference classes
# -----------------------------------------------------------------------------------------
class UniqueSequence:
    """UniqueSequence.java:19-171."""

    def __init__(self, sequence: str, labelsMap=None):
        self.labelsMap = dict(labelsMap) if labelsMap is not None else {"no_label": 1}  # :65-68
        self.sequence = encode(sequence)

    def size(self):  # :82-88
        return int(sum(self.labelsMap.values()))

    def getSequence(self):
        return self.sequence

    def getSequenceString(self):  # :103-109
        return "".join(AMINO_ACIDS[int(i)] for i in self.sequence)

    def getLabelsMap(self):
        return self.labelsMap

    def __eq__(self, other):  # :143-153
        return isinstance(other, UniqueSequence) and np.array_equal(self.sequence, other.sequence)

    def __hash__(self):
        return hash(self.sequence.tobytes())

    def __repr__(self):
        return f"UniqueSequence({self.getSequenceString()!r}, {self.labelsMap})"


class Cluster:
    """Cluster.java:21-204 (member list, id, size)."""

    def __init__(self, sequences, id):
        self.sequences = list(sequences)
        self.id = int(id)
        self._size = sum(s.size() for s in self.sequences)

    def insert(self, sequence):  # :50-63
        if sequence in self.sequences:
            raise DataException(f"Trying to insert unique sequence {sequence.getSequenceString()} into cluster "
                                f"{self.id}, which already contains this sequence. ")
        self.sequences.append(sequence)
        self._size += sequence.size()

    def insertAll(self, sequences):  # :70-74
        for s in list(sequences):
            self.insert(s)

    def getSequences(self):
        return self.sequences

    def getId(self):
        return self.id

    def size(self):  # :156-158
        return self._size

    def getUniqueSize(self):  # :113-115
        return len(self.sequences)

    def __repr__(self):
        return f"Cluster(id={self.id}, unique={self.getUniqueSize()}, size={self._size})"


class _GpuScorer:
    def __init__(self, scoringMatrix, device=0):
        self.scoringMatrix = np.asarray(scoringMatrix, dtype=np.int32).reshape(24, 24)
        self._ctx = Context(self.scoringMatrix, device)

    def _score(self, seq1, seq2):
        self._ctx.set_sequences([seq1.sequence, seq2.sequence])
        return int(self._pairs([0], [1])[0])


class ShiftedScorer(_GpuScorer):
    """ShiftedScorer.java:12-114: ShiftedScorer(scoringMatrix, shiftPenalty, maxShift)."""

    def __init__(self, scoringMatrix, shiftPenalty, maxShift, device=0):
        super().__init__(scoringMatrix, device)
        self.shiftPenalty = int(shiftPenalty)
        self.maxShift = int(maxShift)

    def _pairs(self, i, j):
        return self._ctx.score_pairs_shifted(i, j, self.maxShift, self.shiftPenalty)

    def sequenceScore(self, seq1, seq2):  # :98-100; throws DataException (:59-62)
        return self._score(seq1, seq2)

    def scoreWithShift(self, seq1, seq2):  # :48-95 -> (score, shift), AligningScorerResult
        self._ctx.set_sequences([seq1.sequence, seq2.sequence])
        score, shift = self._ctx.score_with_shift([0], [1], self.maxShift, self.shiftPenalty)
        return int(score[0]), int(shift[0])


class LocalAlignmentScorer(_GpuScorer):
    """LocalAlignmentScorer.java:10-155: (scoringMatrix, gapOpenPenalty, gapExtendPenalty)."""

    def __init__(self, scoringMatrix, gapOpenPenalty, gapExtendPenalty, device=0):
        super().__init__(scoringMatrix, device)
        self.gapOpenPenalty = int(gapOpenPenalty)
        self.gapExtendPenalty = int(gapExtendPenalty)

    def _pairs(self, i, j):
        return self._ctx.score_pairs_local(i, j, self.gapOpenPenalty, self.gapExtendPenalty)

    def sequenceScore(self, seq1, seq2):  # :27-29
        return self._score(seq1, seq2)


class HipClinkageSequenceClusterer:
    """Drop-in for ClinkageSequenceClusterer(sequenceScorer, threshold) (ClinkageSequenceClusterer.java:29-33): same
    ``cluster(List<UniqueSequence>) -> List<Cluster>`` contract (:43-124) -- exact complete linkage, cluster ids as the
    reference assigns them (singletons index + 1, merged clusters n + 2, ... in merge order), the returned list in the
    iteration order of the reference's HashSet, members in getSequences() order."""

    def __init__(self, sequenceScorer: "ShiftedScorer", threshold):
        if not isinstance(sequenceScorer, ShiftedScorer):
            raise TypeError("the GPU clinkage path takes a ShiftedScorer (Hammock.java:458)")
        self.sequenceScorer = sequenceScorer
        self.threshold = int(threshold)
        self.stats = None

    def cluster(self, sequences):
        sc = self.sequenceScorer
        ctx = sc._ctx
        ctx.set_sequences([s.sequence for s in sequences], sizes=[s.size() for s in sequences])
        cid, order, stats = ctx.clinkage_cluster(sc.maxShift, sc.shiftPenalty, self.threshold)
        self.stats = stats
        members = {}
        for k, c in enumerate(cid.tolist()):
            members.setdefault(c, []).append(k)
        result = []
        for c in order.tolist():
            ks = sorted(members[c], key=lambda k: int(ctx.member_rank[k]))
            result.append(Cluster([sequences[k] for k in ks], c))
        return result


class HipGreedySequenceClusterer:
    """Drop-in for LimitedGreedySequenceClusterer(sequenceScorer, threshold, maxClusters)
    (LimitedGreedySequenceClusterer.java:22) -- same constructor shape, same
    ``cluster(List<UniqueSequence>) -> List<Cluster>`` contract (:39-69): clusters with
    more than one member first (in creation order, id = seed index), then the
    remaining singletons."""

    def __init__(self, sequenceScorer: ShiftedScorer, threshold, maxClusters):
        if not isinstance(sequenceScorer, ShiftedScorer):
            raise TypeError("the GPU greedy path takes a ShiftedScorer (Hammock.java:402)")
        self.sequenceScorer = sequenceScorer
        self.threshold = int(threshold)
        self.maxClusters = int(maxClusters)
        self.stats = None

    def cluster(self, sequences):
        sc = self.sequenceScorer
        ctx = sc._ctx
        ctx.set_sequences([s.sequence for s in sequences], sizes=[s.size() for s in sequences])
        cid, order, stats = ctx.greedy_cluster(sc.maxShift, sc.shiftPenalty, self.threshold, self.maxClusters)
        self.stats = stats
        members = {}
        for k, c in enumerate(cid.tolist()):
            members.setdefault(c, []).append(k)
        result = []
        for c in order.tolist():
            ks = members[c]
            ks.sort(key=lambda k: int(ctx.member_rank[k]))  # Cluster.getSequences() insertion order
            cl = Cluster([sequences[ks[0]]], c)
            for k in ks[1:]:
                cl.insert(sequences[k])
            result.append(cl)
        return result
