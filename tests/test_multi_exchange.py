"""The cross-device exchange of a multi-device clustering call (hammock_amd/csrc/hmk_multi.cpp), run on ONE GPU.

Contexts of one call that sit on the same HIP ordinal normally read each other's blocks in place; HMK_MULTI_FORCE_COPIES=1 makes
them exchange the way distinct GPUs do: every edge block is copied into its owner's inbox (SB_PEER, slot = the sender's place among the
owner's G - 1 senders), its size into SB_PEERCNT, every peer's band block into the root's SB_PEERBAND at its offset, and a block that
does not fit the inbox makes the call retry with a larger one.  The library says what it did on stderr under HMK_GREEDY_TIMING
("peer copies of G devices: ...", "attempt k retried: ..."), and every test here reads those lines: a forced-copy test that took
the shortcut after all would prove nothing.

Every result is compared with the CPU oracle (cluster ids, list order, member order), the edge count with a single-device context's,
and every call is made twice on the same context (grown buffers, cached plans).

What stays unverified on one GPU: copies over xGMI, hipDeviceEnablePeerAccess, and kernels loading from another device's memory.  The
distinct-ordinal lists of conftest.multi_device_lists() are parametrised here too and skip themselves on a one-GPU machine.

Not covered: a peer's band block larger than its band region (hmk_multi.cpp, `band_total > band_region`: the call then waits for the
whole pass).  The region is half the peer's edge buffer and the band holds 2 * max_clusters + 1024 rows of at most half the
sequences; no input that reaches it has been found.

That the tests bite: hmk_multi.cpp broken one place at a time, every copy and read still inside its buffer, this file run once each.

  band_off = 0 for every peer (the peers' band blocks overlap in the root's region): the oracle comparison fails in
      test_forced_copies_base_matrix[band_40000] at 3, 5 and 8 devices, test_multi_shapes[mixed_7_20 | adj_8byte, dev000, forced_copies]
      and test_inbox_overflow_retry.  Two devices cannot see it (the one peer's offset is 0), nor can a set without a band.
  need_inbox never grown: test_inbox_overflow_retry ends in "internal edge buffer kept overflowing"; nothing else changes.
  the last sender's edge block not copied, 0 written as its size (run on the asymmetric cases only, see below):
      test_multi_shapes[asymmetric, dev00 | dev000, forced_copies] end in the library's own "the pieces' entries do not add up to the
      edges scored".

Argued from the code, not run (each would read or write what this call never wrote, or leave a buffer):
  - two senders in one slot, or a size in another slot than its block: the owner reads one inbox under a size left by an earlier call
    (or by nobody), entries that are arbitrary ids.  Where the sizes happen to be plausible the piece's entry total still differs
    from the edges scored (asymmetric: the library's check; check_entries here).
  - slot = d instead of d - 1 above the owner: the last sender's block starts at (G - 1) * inbox_cap, the end of SB_PEER.
  - the lost block under a SYMMETRIC matrix: the row space comes from the degree slices, which still count the lost edges, so the rows
    keep slots nobody filled.  For the same reason the slices themselves are not mutated on the GPU.  They are covered by the pair
    asymmetric / symmetric_twin: the same sequences give the oracle's clustering with the slices (the twin: a CSR whose row starts
    are the summed slices, and check_entries = their total) and without them (degrees counted over the received blocks).
stats.n_edges is the senders' count and cannot see the exchange; check_entries (the owners' CSR pieces) can."""
import functools
import re

import numpy as np
import pytest

from conftest import multi_device_lists
from oracle import c_oracle

import hammock_amd
from hammock_amd.synth import synth_peptides

pytestmark = pytest.mark.gpu

COPIES = re.compile(r"\[hmk greedy\] peer copies of (\d+) devices( \(HMK_MULTI_FORCE_COPIES\))?: (\d+) edge blocks, (\d+) band blocks, "
                    r"(\d+) counts, (\d+) degree slices, (\d+) candidate regions")
PIECE = re.compile(r"\[hmk greedy\] device (\d+) of (\d+) \(HIP device \d+, rows (\d+)\.\.(\d+)\):.*? its CSR piece done at [\d.]+ \((\d+) entries\)")
RETRY = re.compile(r"\[hmk greedy\] attempt (\d+) retried: (edge segment overflow|inbox too small) on device (\d+) of (\d+) "
                   r"\(HIP device (\d+)\), needs (\d+) entries")


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need an MI355X; no HIP device is visible")
    return 0


class Call:
    """What one multi-device call printed: its peer copies by kind and the attempts it had to retry."""
    def __init__(self, err):
        lines = COPIES.findall(err)
        assert len(lines) == 1, "one 'peer copies' line per multi-device call:\n" + err[-2000:]
        g, forced, *counts = lines[0]
        self.devices, self.forced = int(g), bool(forced)
        self.edge, self.band, self.counts, self.deg, self.cand = map(int, counts)
        self.retries = [(reason, int(d), int(need)) for _, reason, d, _, _, need in RETRY.findall(err)]
        pieces = PIECE.findall(err)[-self.devices:]          # the last attempt's lines, one per device
        assert [int(d) for d, *_ in pieces] == list(range(self.devices)), err[-2000:]
        self.entries = sum(int(e) for *_, e in pieces)       # adjacency entries in the owners' CSR pieces

    def __repr__(self):
        return (f"Call(devices={self.devices}, forced={self.forced}, edge={self.edge}, band={self.band}, counts={self.counts}, "
                f"deg={self.deg}, cand={self.cand}, retries={self.retries})")


def distinct(devices):
    return len(set(devices)) == len(devices)


def check_entries(call, stats, symmetric=True):
    """stats.n_edges is what the SENDERS scored; what the OWNERS built their rows from is the sum of the CSR pieces' entries: an
    edge is an entry in the row of each end (symmetric scores), of its first end only (asymmetric).  A block that is lost, cut
    short or read twice on its way through an inbox shows here whatever it does to the clustering."""
    assert call.entries == (2 if symmetric else 1) * stats.n_edges, (call, stats.n_edges)


def check_copies(call, devices, forced, *, edge_blocks=True, band=None, symmetric=True):
    """The copies a call of G devices must have issued.  Forced (or distinct ordinals): one size per (sender, owner) pair and
    attempt, an edge block wherever the pair has edges; contexts of one ordinal without the switch: none of either."""
    G = len(devices)
    assert call.devices == G
    copying = forced or distinct(devices)
    assert call.forced == forced
    if copying:
        assert call.counts >= G * (G - 1), call
        if edge_blocks:
            assert call.edge >= G * (G - 1), call
        if band is True:
            assert call.band >= G - 1, call          # every peer's band block went into the root's gathered band
    elif len(set(devices)) == 1:
        assert (call.edge, call.band, call.counts) == (0, 0, 0), call
    if band is False:
        assert call.band == 0, call
    if not symmetric:
        assert call.deg == 0, call                   # asymmetric scores: no fused degree counters, no slices
    elif edge_blocks:
        assert call.deg >= 2 * (G - 1), call         # (an owner with no rows receives no slice)


def greedy_call(ctx, capfd, X, p, thr, maxc):
    capfd.readouterr()
    cid, order, stats = ctx.greedy_cluster(X, p, thr, maxc)
    rank = ctx.member_rank[:len(cid)].copy()
    return cid, order, rank, stats, Call(capfd.readouterr().err)


def same_as_oracle(got, want):
    cid, order, rank = got
    ocid, oorder, orank = want
    return np.array_equal(cid, ocid) and np.array_equal(order, oorder) and np.array_equal(rank, orank)


def blosum():
    import json
    import os
    from conftest import GOLDEN
    with open(os.path.join(GOLDEN, "matrices.json")) as fh:
        return np.asarray(json.load(fh)["matrices"]["blosum62"], dtype=np.int32)


def by_size(res, off, sizes):
    """The caller's side of `-R size`: sequences in the oracle's sort order."""
    perm = c_oracle.sort_order(res, off, sizes, "size")
    peps = [res[off[k]:off[k + 1]] for k in perm]
    res, off = hammock_amd.pack_sequences(peps)
    return res, off, np.ascontiguousarray(sizes[perm])


def family(rng, base, count, mutations):
    """`count` DISTINCT peptides that differ from `base` at up to `mutations` positions."""
    seen, out = set(), []
    while len(out) < count:
        q = base.copy()
        for pos in rng.choice(len(base), size=mutations, replace=False):
            q[pos] = rng.integers(0, 20)
        if q.tobytes() not in seen:
            seen.add(q.tobytes())
            out.append(q)
    return out


# ---- the inputs: name -> (matrix, residues, offsets, sizes, X, p, threshold, max_clusters, environment) --------------------
@functools.lru_cache(maxsize=None)
def greedy_input(name):
    M = blosum()
    env = {}
    if name == "band_40000":        # the set of test_greedy_multi_device_context: a band of 3,024 rows
        n = 40000
        res, off = synth_peptides(21, n, 12)
        sizes = (1 + np.random.default_rng(21).integers(0, 5, size=n)).astype(np.int32)
        res, off, sizes = by_size(res, off, sizes)
        par = (3, 0, 20, 1000)
    elif name == "no_band_12000":   # below 16,384 sequences: no band (band_state = -1 on every device)
        n = 12000
        res, off = synth_peptides(22, n, 12)
        sizes = (1 + np.random.default_rng(22).integers(0, 5, size=n)).astype(np.int32)
        res, off, sizes = by_size(res, off, sizes)
        par = (3, 0, 20, 300)
    elif name == "asymmetric":      # the construction of test_greedy_asymmetric_matrix_end_to_end, 6,000 sequences
        rng = np.random.default_rng(21)
        M = M.copy()
        M[np.triu_indices(24, 1)] += rng.integers(-2, 3, size=276).astype(np.int32)
        res, off = synth_peptides(6, 6000, 11, 13)
        res, off, sizes = by_size(res, off, rng.integers(1, 9, size=6000).astype(np.int32))
        par = (3, -1, 17, 150)
    elif name == "symmetric_twin":  # the same sequences under the symmetric matrix: the fused degree counters and their slices
        _, res, off, sizes, *_ = greedy_input("asymmetric")
        par = (3, -1, 17, 150)
    elif name == "mixed_7_20":      # per-length plans per shard, shift penalty -1
        n = 20000
        res, off = synth_peptides(23, n, 7, 20)
        sizes = (1 + np.random.default_rng(23).integers(0, 4, size=n)).astype(np.int32)
        res, off, sizes = by_size(res, off, sizes)
        par = (3, -1, 23, 500)
    elif name == "adj_8byte":       # 8-byte adjacency entries where 4 would do (forced), band present
        n = 20000
        res, off = synth_peptides(24, n, 12)
        sizes = None
        par = (3, 0, 20, 500)
        env = {"HMK_ADJ_8BYTE": "1"}
    elif name == "unpacked":        # 28..32-mers: the best score a pair can reach minus the threshold exceeds 255, 8-byte entries by choice
        n = 5000
        rng = np.random.default_rng(25)
        res, off = synth_peptides(25, n, 28, 32)
        peps = [res[off[k]:off[k + 1]].copy() for k in range(n)]
        for k in range(n // 2, n):   # near-duplicates of the first half: scores far above the threshold
            src = peps[int(rng.integers(0, n // 2))].copy()
            for _ in range(int(rng.integers(1, 6))):
                src[int(rng.integers(len(src)))] = rng.integers(0, 20)
            peps[k] = src
        peps = list({bytes(q): q for q in peps}.values())
        res, off = hammock_amd.pack_sequences(peps)
        sizes = None
        par = (3, 0, 45, 125)
    elif name.startswith("tiny_"):  # n sequences of one family: every pair is an edge
        n = int(name[5:])
        rng = np.random.default_rng(100 + n)
        res, off = hammock_amd.pack_sequences(family(rng, rng.integers(0, 20, size=12).astype(np.uint8), n, 1))
        sizes = None
        par = (3, 0, 20, 1)
    elif name == "inbox_overflow":
        # Device d owns the INPUT rows [d * rows_per, (d + 1) * rows_per): edge ends are caller indices (include/hammock_hip.h), the
        # plan's bucket order never reaches an edge.  The 16-row chunks of the pair space are dealt to the shards round robin.
        # 4,800 peptides within four substitutions of one another fill the last 5,000 of 40,000 rows (rows_per = 5,000 at G = 8:
        # device 7's).  All their 11.5 million pairs are edges; every shard scores an eighth, about 1.4 million, and all of those go to
        # device 7 -- once each, both ends live there.
        # The first guess (1,424,000 edges per shard) is too small, so attempt 0 ends in "edge segment overflow" and the edge buffer
        # grows to 16 * 1.125 * the fullest segment; the inbox, 1.5 * 2 / G of that + 65,536 per sender, to 6.75 of that segment.  A
        # sender's block is 16 MEAN segments, so the inbox retry needs the family's tiles spread evenly over the 16 segments.  In the
        # LAST rows a row chunk is one tile and the family's chunks are neighbours in the plan's tile order (37 to a shard).
        n, fam = 40000, 4800
        rng = np.random.default_rng(26)
        base = np.array([17, 4, 8, 18, 14, 17, 4, 8, 18, 14, 17, 4], dtype=np.uint8)   # W C H Y P ...: self-score 104
        head = family(rng, base, fam, 2)
        # (the reference throws where the FIRST sequence has no neighbour at all: three variants of another peptide lead the set)
        lead = family(rng, np.array([13, 9, 12, 5, 6, 2, 13, 9, 12, 5, 6, 2], dtype=np.uint8), 3, 1)
        fill, foff = synth_peptides(26, n - fam - 3, 12)
        peps = lead + [fill[foff[k]:foff[k + 1]] for k in range(n - fam - 3)] + head
        assert len({bytes(q) for q in peps}) == n
        res, off = hammock_amd.pack_sequences(peps)
        sizes = None
        par = (3, 0, 40, 1000)   # (four substitutions cost at most 60 of the self-score 104: every pair of the family is an edge)
    else:
        raise KeyError(name)
    return M, res, off, sizes, *par, env


@functools.lru_cache(maxsize=None)
def greedy_oracle(name):
    M, res, off, sizes, X, p, thr, maxc, _ = greedy_input(name)
    st, ocid, oorder, ostats = c_oracle.greedy_cluster(M, res, off, sizes, 0, X, p, thr, maxc, 8)
    assert st == 0, f"{name}: the oracle's status is {st} (a crash-parity input would void the test)"
    return ocid, oorder, np.asarray(ostats.member_rank).copy()


@functools.lru_cache(maxsize=None)
def single_device_edges(name):
    M, res, off, sizes, X, p, thr, maxc, _ = greedy_input(name)
    ctx = hammock_amd.Context(M, device=0)
    ctx.set_sequences(residues=res, offsets=off, sizes=sizes)
    return int(ctx.greedy_cluster(X, p, thr, maxc)[2].n_edges)


def multi_context(name, devices):
    M, res, off, sizes, *_ = greedy_input(name)
    ctx = hammock_amd.Context(M, device=devices)
    from hammock_amd import _native
    assert _native.lib.hmk_device_count(ctx._h) == len(devices)
    ctx.set_sequences(residues=res, offsets=off, sizes=sizes)
    return ctx


# ---- a. forced copies: the base matrix ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["band_40000", "no_band_12000"])
@pytest.mark.parametrize("devices", multi_device_lists(repeated=((0, 0), (0, 0, 0), (0,) * 5, (0,) * 8)))
def test_forced_copies_base_matrix(gpu, capfd, monkeypatch, devices, name):
    """Two, three, five and eight contexts on one GPU exchanging through copies: inbox slots and offsets for every (sender, owner)
    pair, rows_per and HMK_PRE_REGIONS / G with remainders (five), the gathered band at its per-peer offsets (40,000 sequences) and
    the call without a band (12,000).  Then one call each with the root replicating the pieces, the host's second loop, no band,
    and back."""
    *_, X, p, thr, maxc, _ = greedy_input(name)
    want = greedy_oracle(name)
    band = name == "band_40000"
    monkeypatch.setenv("HMK_GREEDY_TIMING", "1")
    monkeypatch.setenv("HMK_MULTI_FORCE_COPIES", "1")
    ctx = multi_context(name, devices)
    for _ in range(2):
        cid, order, rank, stats, call = greedy_call(ctx, capfd, X, p, thr, maxc)
        assert same_as_oracle((cid, order, rank), want)
        check_copies(call, devices, True, band=band)
        assert not call.retries, call
        assert call.cand >= len(devices) - 1, call           # the pre-check ran on the pieces: every peer's regions went to the root
        assert stats.n_edges == single_device_edges(name)    # the shards together hold every edge exactly once
        check_entries(call, stats)
    assert bool(ctx.greedy_phases()["band_bytes"]) == band
    for var, value, has_band in (("HMK_MULTI_REPLICATE", "1", band), ("HMK_SECOND_LOOP", "host", band), ("HMK_NO_BAND", "1", False)):
        monkeypatch.setenv(var, value)
        cid, order, rank, stats, call = greedy_call(ctx, capfd, X, p, thr, maxc)
        monkeypatch.delenv(var)
        assert same_as_oracle((cid, order, rank), want), var
        check_copies(call, devices, True, band=has_band)
        assert stats.n_edges == single_device_edges(name)
        check_entries(call, stats)
    cid, order, rank, stats, call = greedy_call(ctx, capfd, X, p, thr, maxc)   # and back
    assert same_as_oracle((cid, order, rank), want)
    check_copies(call, devices, True, band=band)


# ---- b. shapes the multi path had not seen --------------------------------------------------------------------------------
@pytest.mark.parametrize("forced", [False, True], ids=["in_place", "forced_copies"])
@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0]], ids=["dev00", "dev000"])
@pytest.mark.parametrize("name", ["asymmetric", "symmetric_twin", "mixed_7_20", "adj_8byte", "unpacked"])
def test_multi_shapes(gpu, capfd, monkeypatch, name, devices, forced):
    """An asymmetric matrix (no fused degree counters: the owner counts over the blocks it received, and no degree slice travels;
    its symmetric twin is the same set with them), mixed lengths with a shift penalty (per-length plans per shard), 8-byte
    adjacency entries forced and chosen.  With the switch: through inboxes; without: the blocks read in place, and no copy made."""
    M, _, off, _, X, p, thr, maxc, env = greedy_input(name)
    want = greedy_oracle(name)
    if name == "unpacked":   # (hmk_multi.cpp: 4-byte entries only while the best score any pair can reach - threshold <= 255)
        assert int(np.diff(off.astype(np.int64)).max()) * int(M.max()) - thr > 255
    monkeypatch.setenv("HMK_GREEDY_TIMING", "1")
    if forced:
        monkeypatch.setenv("HMK_MULTI_FORCE_COPIES", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ctx = multi_context(name, devices)
    for _ in range(2):
        cid, order, rank, stats, call = greedy_call(ctx, capfd, X, p, thr, maxc)
        assert same_as_oracle((cid, order, rank), want)
        check_copies(call, devices, forced, symmetric=bool((M == M.T).all()))
        assert not call.retries, call
        assert stats.n_edges == single_device_edges(name)
        check_entries(call, stats, symmetric=bool((M == M.T).all()))


@pytest.mark.parametrize("forced", [False, True], ids=["in_place", "forced_copies"])
@pytest.mark.parametrize("n,devices", [(2, [0, 0]), (3, [0, 0]), (2, [0, 0, 0]), (3, [0, 0, 0]), (3, [0] * 8), (9, [0] * 8), (10, [0, 0, 0])],
                         ids=lambda v: "dev" + "".join(map(str, v)) if isinstance(v, list) else f"n{v}")
def test_multi_tiny_sets(gpu, capfd, monkeypatch, n, devices, forced):
    """Fewer sequences than devices, and owners without a row: n = 2 on three devices gives rows_per = 1 and leaves the third
    nothing; n = 9 on eight gives rows_per = 2 and leaves devices 5-7 nothing (r0 == r1 == n); n = 10 on three leaves the last
    a short range.  Every pair of the set is an edge, so the one cluster needs every owner's rows."""
    name = f"tiny_{n}"
    *_, X, p, thr, maxc, _ = greedy_input(name)
    want = greedy_oracle(name)
    assert len(set(want[0].tolist())) == 1               # one cluster of all n
    monkeypatch.setenv("HMK_GREEDY_TIMING", "1")
    if forced:
        monkeypatch.setenv("HMK_MULTI_FORCE_COPIES", "1")
    ctx = multi_context(name, devices)
    for _ in range(2):
        cid, order, rank, stats, call = greedy_call(ctx, capfd, X, p, thr, maxc)
        assert same_as_oracle((cid, order, rank), want)
        check_copies(call, devices, forced, edge_blocks=False, band=False)
        assert stats.n_edges == n * (n - 1) // 2 == single_device_edges(name)
        check_entries(call, stats)


@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0]], ids=["dev00", "dev000"])
def test_clinkage_forced_copies(gpu, capfd, monkeypatch, devices):
    """hmk_clinkage_cluster through the same exchange: the mixed_dense case of test_clinkage_vs_oracle (lengths 7..20, shift
    penalty -1, threshold 15) under forced copies."""
    M = blosum()
    res, off = synth_peptides(4, 3000, 7, 20)
    sizes = (1 + np.random.default_rng(17).integers(0, 3, size=3000)).astype(np.int32)
    X, p, thr = 3, -1, 15
    st, ocid, oorder, orank, ostats = c_oracle.clinkage_cluster(M, res, off, sizes, X, p, thr, 8)
    assert st == 0 and ostats.merges > 0
    single = hammock_amd.Context(M, device=0)
    single.set_sequences(residues=res, offsets=off, sizes=sizes)
    sstats = single.clinkage_cluster(X, p, thr)[2]
    monkeypatch.setenv("HMK_GREEDY_TIMING", "1")
    monkeypatch.setenv("HMK_MULTI_FORCE_COPIES", "1")
    ctx = hammock_amd.Context(M, device=devices)
    ctx.set_sequences(residues=res, offsets=off, sizes=sizes)
    for _ in range(2):
        capfd.readouterr()
        cid, order, stats = ctx.clinkage_cluster(X, p, thr)
        call = Call(capfd.readouterr().err)
        assert same_as_oracle((cid, order, ctx.member_rank[:len(cid)]), (ocid, oorder, orank))
        assert (stats.merges, stats.searches, stats.n_result_clusters) == (ostats.merges, ostats.searches, ostats.n_result_clusters)
        check_copies(call, devices, True, band=False)
        assert stats.n_edges == sstats.n_edges
        check_entries(call, stats)


# ---- c. the inbox-overflow retry ------------------------------------------------------------------------------------------
def test_inbox_overflow_retry(gpu, capfd, monkeypatch):
    """Eight devices, and every above-threshold pair of a dense family inside device 7's rows (greedy_input("inbox_overflow")):
    each sender's block for device 7 is larger than the inbox device 7 keeps per sender.  The attempt must be given up
    ("inbox too small" for device 7, with the size needed), the next attempt must return the oracle's
    clustering through the grown inbox, and a second call on the same context must find the inbox in place.

    An edge whose two ends have ONE owner is dealt to it once (k_route_count), so a sender fills that owner's inbox with at most
    its own shard's edge count; an inbox is too small for that only from G = 8 on (0.375 of the edge buffer).  Here the call
    needs three attempts: edge segment overflow, inbox too small, done."""
    name = "inbox_overflow"
    *_, X, p, thr, maxc, _ = greedy_input(name)
    want = greedy_oracle(name)
    devices = [0] * 8
    G = len(devices)
    monkeypatch.setenv("HMK_GREEDY_TIMING", "1")
    monkeypatch.setenv("HMK_MULTI_FORCE_COPIES", "1")
    ctx = multi_context(name, devices)
    cid, order, rank, stats, call = greedy_call(ctx, capfd, X, p, thr, maxc)
    inbox = [r for r in call.retries if r[0] == "inbox too small"]
    assert inbox, call
    assert {d for _, d, _ in inbox} == {G - 1}, call                   # device 7 owns the family's rows: its inbox, nobody else's
    assert max(need for _, _, need in inbox) > 11_000_000 // G, call   # a sender's eighth of the family's 11.5 million pairs
    assert same_as_oracle((cid, order, rank), want)
    assert stats.n_edges == single_device_edges(name) > 11_000_000
    check_entries(call, stats)
    check_copies(call, devices, True)
    cid, order, rank, stats, call = greedy_call(ctx, capfd, X, p, thr, maxc)
    assert not call.retries, call
    assert same_as_oracle((cid, order, rank), want)
    assert stats.n_edges == single_device_edges(name)
    check_entries(call, stats)
    check_copies(call, devices, True)
