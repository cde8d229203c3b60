"""The separation of given clusters: hmk_cluster_separation_shifted (k_separation.hip) and `hammock-hip separation`.

CPU part (host-only context): the symbol, every argument check, DeviceError for a valid call, the segment sizing rule, the mode's usage
line and its argument and file errors, and tests of the INPUTS with the C oracle alone: that they hold what the GPU tests claim to
exercise, and that the oracle scores every pair of them equally in both orientations (the kernel relies on it).
GPU part: every output and every statistics field bit-exact against an expectation built from the C oracle alone -- score_pairs over
the strict lower triangle (seq1 = the larger index) into a symmetric int64 matrix, that matrix times a one-hot slot matrix for the sums
per (member, slot), the nearest slot and the flags by int64 cross-products.  An input's scores are computed once per session and shared.
    sized0, sized1      test_linkage.sized_families(0 / 1): 3,383 members in 24 slots of 1, 2, 63/64/65, 256/257 and 513/700 members
    ..._relabelled      the same with 5 % of the labels redrawn: members that sit closer to another slot than to their own
    ties                70 copies of one string in two slots of 30 and 40 among small slots of its variants: equal means, unequal sizes
    wide                69,000 + 600 + 40 copies of words under a matrix with cells of +-1,000: sums beyond 2^31, cross-products beyond 2^40
"""
import ctypes as C
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from test_assign import gpu   # noqa: F401  (the fixture that skips where no HIP device is visible)
from test_continue import cli, read_cluster_file
from test_linkage import _blosum62, device_ctx, sized_families

import hammock_amd
from hammock_amd import _native as N

UINT32_MAX = 2 ** 32 - 1
T = 256   # LINK_TILE: members per block, places per staged chunk
ITEMS, MAX_SEGMENTS, MIN_SEGMENT = 4096, 64, 256   # hmk_sizing.h
GRID_LINE = re.compile(r"^\[hmk grid\] (\S+) (\d+) -> (\d+)$", re.M)
LETTERS = hammock_amd.AMINO_ACIDS
STAT_NAMES = ("pairs_scored", "n_misplaced", "n_multi", "n_segments", "launches", "reserved")
OUT_NAMES = ("own_sum", "near_sum", "near_cluster", "misplaced", "cluster_misplaced", "cluster_own_sum")
OUT_DTYPES = (np.int64, np.int64, np.uint32, np.uint8, np.uint32, np.int64)
SIZED = ["sized0", "sized0_relabelled", "sized1", "sized1_relabelled"]


# ---- the sizing rule, stated again ---------------------------------------------------------------------------------------------

def segments(nm, forced=0):
    """-> (segment length, segments): enough segments for ITEMS work items of one member block x one segment, at most MAX_SEGMENTS,
    none shorter than MIN_SEGMENT places, all but the last of one length; a forced length is taken as it is"""
    if nm == 0:
        return 0, 0
    if forced:
        length = min(forced, nm)
    else:
        blocks = -(-nm // T)
        want = max(1, min(-(-ITEMS // blocks), MAX_SEGMENTS, nm // MIN_SEGMENT))
        length = -(-nm // want)
    return length, -(-nm // length)


# ---- inputs and the oracle's side ----------------------------------------------------------------------------------------------

def _variants(rng, centre, count, max_sub, seen):
    out = []
    while len(out) < count:
        q = centre.copy()
        for pos in rng.choice(len(q), size=int(rng.integers(1, max_sub + 1)), replace=False):
            q[pos] = rng.integers(0, 20)
        if q.tobytes() not in seen:
            seen.add(q.tobytes())
            out.append(q)
    return out


@functools.lru_cache(maxsize=None)
def input_set(name):
    """-> (M, res, off, mc, ncl, X, p, strings); every array read-only"""
    M = _blosum62()
    if name.startswith("sized"):
        peps, mc, ncl, X, p, _ = sized_families(int(name[5]))
        mc = mc.copy()
        if name.endswith("_relabelled"):
            rng = np.random.default_rng(7)
            pick = rng.choice(len(peps), size=len(peps) // 20, replace=False)
            mc[pick] = rng.integers(0, ncl, size=pick.size)
    else:
        assert name == "ties"
        rng = np.random.default_rng(31)
        centre = rng.integers(0, 20, size=12).astype(np.uint8)
        seen = {centre.tobytes()}
        plan = [(5, False), (30, True), (3, False), (40, True), (1, False), (2, False), (7, False)]   # (members, copies of the centre?)
        peps, mc = [], []
        for c, (size, copies) in enumerate(plan):
            peps += [centre] * size if copies else _variants(rng, centre, size, 2, seen)
            mc += [c] * size
        perm = rng.permutation(len(peps))
        peps, mc, ncl, X, p = [peps[k] for k in perm], np.asarray(mc, dtype=np.uint32)[perm], len(plan), 3, 0
    res, off = hammock_amd.pack_sequences(peps)
    for arr in (res, off, mc):
        arr.setflags(write=False)
    return M, res, off, mc, ncl, X, p, ["".join(LETTERS[r] for r in q) for q in peps]


def score_matrix(M, res, off, X, p, both=False):
    """int64 [n, n], symmetric, zero diagonal: entry (a, b), a > b, = the oracle's score(seq1 = a, seq2 = b); both: the other
    orientation is scored too and must agree on every pair"""
    from oracle import c_oracle
    n = off.size - 1
    hi, lo = np.tril_indices(n, -1)
    st, sc = c_oracle.score_pairs(M, res, off, hi, lo, 0, X, p)
    assert st == 0
    if both:
        st, back = c_oracle.score_pairs(M, res, off, lo, hi, 0, X, p)
        assert st == 0 and np.array_equal(sc, back)
    S = np.zeros((n, n), dtype=np.int64)
    S[hi, lo] = sc
    S[lo, hi] = sc
    S.setflags(write=False)
    return S


@functools.lru_cache(maxsize=None)
def scores(name):
    M, res, off, _, _, X, p, _ = input_set(name.replace("_relabelled", ""))
    return score_matrix(M, res, off, X, p)


def nearest(sums, sizes, mc):
    """the definition, in int64: of the slots other than the member's own the largest mean sums / sizes, the smallest slot among equal
    means -> (near_sum, near_cluster, ways the nearest mean is attained); sums [nm, ncl] (|sums| x sizes < 2^62)"""
    nm, ncl = sums.shape
    best_sum, best_size = np.zeros(nm, dtype=np.int64), np.zeros(nm, dtype=np.int64)
    best_slot, ways = np.full(nm, UINT32_MAX, dtype=np.int64), np.zeros(nm, dtype=np.int64)
    for c in range(ncl):
        other = mc != c
        left, right = sums[:, c] * best_size, best_sum * sizes[c]
        better = other & ((best_size == 0) | (left > right))
        equal = other & (best_size > 0) & (left == right)
        ways = np.where(better, 1, ways + equal)
        best_sum = np.where(better, sums[:, c], best_sum)
        best_size = np.where(better, sizes[c], best_size)
        best_slot = np.where(better, c, best_slot)
    return best_sum, best_slot, best_size, ways


def reduce_sums(sums, mc, ncl, forced=0):
    """the six outputs, the statistics and the ways of every member's nearest mean from the sums per (member, slot)"""
    mc = np.asarray(mc, dtype=np.int64)
    nm = mc.size
    sizes = np.bincount(mc, minlength=ncl).astype(np.int64)
    own = sums[np.arange(nm), mc] if nm else np.zeros(0, dtype=np.int64)
    near_sum, near_cluster, near_size, ways = nearest(sums, sizes, mc)
    mine = sizes[mc] if nm else np.zeros(0, dtype=np.int64)
    misplaced = (mine >= 2) & (near_size > 0) & (own * near_size < near_sum * (mine - 1))
    cluster_misplaced, cluster_own = np.zeros(ncl, dtype=np.int64), np.zeros(ncl, dtype=np.int64)
    np.add.at(cluster_misplaced, mc, misplaced)
    np.add.at(cluster_own, mc, own)
    stats = {"pairs_scored": nm * (nm - 1) if nm else 0, "n_misplaced": int(misplaced.sum()), "n_multi": int((sizes >= 2).sum()),
             "n_segments": segments(nm, forced)[1], "launches": 2 if nm else 0, "reserved": 0}
    return (own, near_sum, near_cluster, misplaced.astype(np.int64), cluster_misplaced, cluster_own), stats, ways, near_size


def slot_sums(S, mc, ncl, onehot=None):
    """[nm, ncl]: the score matrix times the one-hot slot matrix; beyond 64 slots the same sums with the columns sorted by slot and
    added run by run (no slot is empty), which the inputs test holds against the product"""
    mc = np.asarray(mc, dtype=np.int64)
    if ncl <= 64 if onehot is None else onehot:
        return S @ (mc[:, None] == np.arange(ncl)[None, :]).astype(np.int64)
    order = np.argsort(mc, kind="stable")
    starts = np.r_[0, np.cumsum(np.bincount(mc, minlength=ncl))[:-1]]
    return np.add.reduceat(S[:, order], starts, axis=1) if mc.size else np.zeros((0, ncl), dtype=np.int64)


def expect(S, mc, ncl, forced=0):
    """S: the score matrix of exactly the members (symmetric, zero diagonal)"""
    return reduce_sums(slot_sums(S, mc, ncl), mc, ncl, forced)


@functools.lru_cache(maxsize=None)
def expect_full(name):
    _, _, _, mc, ncl, _, _, _ = input_set(name)
    return expect(scores(name), mc, ncl)


def wanted_grids(nm, forced=0):
    """kernel -> the grid its launcher asks for (k_separation.hip's launchers); an empty range launches nothing"""
    if nm == 0:
        return {}
    return {"k_separation_walk": min(-(-nm // T) * segments(nm, forced)[1], 65536), "k_separation_merge": min(-(-nm // T), 4096)}


def check(got, want, stats):
    outs, wstats = want[0], want[1]
    for g, w, name, dt in zip(got, outs, OUT_NAMES, OUT_DTYPES):
        assert g.dtype == dt, name
        assert np.array_equal(g.astype(np.int64), w), name
    for name in STAT_NAMES:
        assert getattr(stats, name) == wstats[name], name
    assert stats.kernel_ms > 0 or wstats["launches"] == 0


def separation(ctx, capfd, cap, r0, r1, mc, ncl, X, p, forced=0):
    """the call, with the [hmk grid] lines of the new kernels asserted against the launchers' arithmetic -> (outputs, stats)"""
    capfd.readouterr()
    got = ctx.cluster_separation_shifted(r0, r1, mc, ncl, X, p)
    grids = wanted_grids(r1 - r0, forced)
    lines = {}
    for kernel, wanted, launched in GRID_LINE.findall(capfd.readouterr().err):
        assert kernel not in lines
        lines[kernel] = (int(wanted), int(launched))
    assert {k: v for k, v in lines.items() if k.startswith("k_separation_")} == {k: (w, cap) for k, w in grids.items() if cap and w > cap}
    return got, ctx.last_separation_stats


# ---- CPU: the symbol, the checks, the sizing rule --------------------------------------------------------------------------------

def test_symbol_is_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "hammock_hip.h")) as fh:
        header = fh.read()
    assert "int hmk_cluster_separation_shifted(hmk_ctx *ctx" in header and "} hmk_separation_stats;" in header
    assert "hmk_cluster_separation_shifted" in N.SYMBOLS
    assert hasattr(N.lib, "hmk_cluster_separation_shifted")
    assert N.lib.hmk_abi_version() == 4
    assert C.sizeof(N.SeparationStats) == 40
    assert [f[0] for f in N.SeparationStats._fields_] == list(STAT_NAMES) + ["kernel_ms"]


RAW_TYPES = {"own_sum": (np.int64, C.c_int64, 1), "near_sum": (np.int64, C.c_int64, 1), "near_cluster": (np.uint32, C.c_uint32, 1),
             "misplaced": (np.uint8, C.c_uint8, 1), "cluster_misplaced": (np.uint32, C.c_uint32, 0), "cluster_own_sum": (np.int64, C.c_int64, 0)}


def _raw_call(ctx, r0, r1, mc, ncl, X, p, null=(), stats=True):
    """the C entry point with chosen arguments null -> status"""
    sizes = (max(ncl, 1), max(r1 - r0, 1))
    mc = None if mc is None else np.ascontiguousarray(mc, dtype=np.uint32)
    out = {k: np.zeros(sizes[which], dt) for k, (dt, _, which) in RAW_TYPES.items()}
    ptr = [None if k in null else out[k].ctypes.data_as(C.POINTER(RAW_TYPES[k][1])) for k in RAW_TYPES]
    s = N.SeparationStats()
    return N.lib.hmk_cluster_separation_shifted(ctx._h, r0, r1, None if mc is None else mc.ctypes.data_as(C.POINTER(C.c_uint32)), ncl, X, p,
                                                *ptr, C.byref(s) if stats else None)


def test_host_only_context_answers_every_bad_argument(blosum62):
    rng = np.random.default_rng(5)
    peps = [rng.integers(0, 20, size=12).astype(np.uint8) for _ in range(6)]
    res, off = hammock_amd.pack_sequences(peps)
    ctx = hammock_amd.Context(blosum62, device=-1)
    ctx.set_sequences(residues=res, offsets=off)
    mc = [0, 0, 1, 1, 2, 2]
    bad = N.HMK_ERR_BAD_ARG
    # the range and slot checks of hmk_cluster_linkage_shifted
    assert _raw_call(ctx, 4, 2, mc[:2], 1, 3, 0) == bad                      # r0 > r1
    assert _raw_call(ctx, 0, 7, mc + [2], 3, 3, 0) == bad                    # r1 > n
    assert _raw_call(ctx, 0, 6, [0, 0, 1, 1, 3, 3], 3, 3, 0) == bad          # a slot at or above n_clusters
    assert _raw_call(ctx, 0, 6, [0, 0, 1, 1, 1, 1], 3, 3, 0) == bad          # a slot without a member
    assert _raw_call(ctx, 3, 3, None, 1, 3, 0) == bad                        # ... in an empty range too
    assert _raw_call(ctx, 0, 6, None, 3, 3, 0) == bad                        # null member_cluster, non-empty range
    for name in ("own_sum", "near_sum", "near_cluster"):                     # a null required output
        assert _raw_call(ctx, 0, 6, mc, 3, 3, 0, null=(name,)) == bad
        assert "null output" in N.lib.hmk_last_error(ctx._h).decode()
    assert _raw_call(ctx, 0, 6, mc, 3, 3, 0, stats=False) == bad             # null stats
    assert "stats" in N.lib.hmk_last_error(ctx._h).decode()
    assert _raw_call(ctx, 3, 3, None, 0, 3, 0, stats=False) == bad           # ... in an empty range too
    with pytest.raises(ValueError):
        ctx.cluster_separation_shifted(0, 6, [0, 0, 1, 1, 3, 3], 3, 3, 0)
    with pytest.raises(ValueError):
        ctx.cluster_separation_shifted(0, 6, mc[:5], 3, 3, 0)
    # an asymmetric matrix
    A = blosum62.copy()
    A[0, 1] += 1
    actx = hammock_amd.Context(A, device=-1)
    actx.set_sequences(residues=res, offsets=off)
    with pytest.raises(ValueError, match="symmetric"):
        actx.cluster_separation_shifted(0, 6, mc, 3, 3, 0)
    # a valid call: no CPU fallback, with or without the optional outputs, for an inner range and for an empty one too
    assert _raw_call(ctx, 0, 6, mc, 3, 3, 0) == N.HMK_ERR_DEVICE
    assert _raw_call(ctx, 0, 6, mc, 3, 3, 0, null=("misplaced", "cluster_misplaced", "cluster_own_sum")) == N.HMK_ERR_DEVICE
    assert _raw_call(ctx, 0, 6, [0] * 6, 1, 3, 0) == N.HMK_ERR_DEVICE
    assert _raw_call(ctx, 3, 3, None, 0, 3, 0) == N.HMK_ERR_DEVICE
    with pytest.raises(hammock_amd.DeviceError):
        ctx.cluster_separation_shifted(0, 6, mc, 3, 3, 0)
    with pytest.raises(hammock_amd.DeviceError):
        ctx.cluster_separation_shifted(2, 6, [0, 0, 1, 1], 2, 3, 0, flags=False, clusters=False)


def test_segment_sizing_rule(tmp_path):
    """hmk_sizing.h's separation_segments, built with the host compiler alone, against the rule as the issue states it"""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    probe = str(tmp_path / "separation_sizing_probe")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-o", probe, os.path.join(ROOT, "tests", "tools", "separation_sizing_probe.cpp")])
    sizes = [1, 2, 255, 256, 257, 511, 512, 513, 600, 3383, 16383, 16384, 16385, 20000, 10 ** 5, 262144, 10 ** 6, 2 ** 24]
    rows = [(nm, 0) for nm in sizes] + [(nm, f) for nm in (1, 600, 3383, 10 ** 5) for f in (1, 2, 7, 64, 255, 256, 257, 1000, 10 ** 6)]
    text = "".join(f"{nm} {f}\n" for nm, f in rows)
    out = subprocess.run([probe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert out[0] == f"limits = {ITEMS} {MAX_SEGMENTS} {MIN_SEGMENT}" and len(out) == 1 + len(rows)
    for (nm, forced), line in zip(rows, out[1:]):
        asked, got = line.split(" = ")
        assert asked == f"{nm} {forced}"
        length, count = (int(v) for v in got.split())
        assert (length, count) == segments(nm, forced), line
        # what the rule is for, whatever its arithmetic: the segments cover the places, none is empty, and without the switch there
        # are at most 64 of at least 256 places, and no more than bring the items to 4,096 -- or one, when even that is too many
        assert (count - 1) * length < nm <= count * length
        if forced:
            assert length == min(forced, nm)
        else:
            blocks = -(-nm // T)
            assert count <= MAX_SEGMENTS and (length >= MIN_SEGMENT or count == 1)
            assert count == 1 or (count - 1) * blocks < ITEMS
    assert segments(3383) == (261, 13) and segments(10 ** 5) == (9091, 11) and segments(20000) == (385, 52) and segments(255) == (255, 1)
    assert segments(2 ** 24) == (2 ** 24, 1) and segments(600, 1) == (1, 600)


def test_cli_separation_argument_and_file_errors(tmp_path):
    r = cli("separation", "-d", str(tmp_path / "a"))
    assert r.returncode == 2 and "-i or --input" in r.stderr
    assert not (tmp_path / "a").exists()
    good = tmp_path / "good.tsv"
    good.write_text("cluster_id\tsequence\tno_label\n1\tWVTAPRSLPVLP\t1\n1\tWVTAPRSLPVLA\t1\n")
    r = cli("separation", "-i", str(good), "--devices", "0,1", "-d", str(tmp_path / "b"))
    assert r.returncode == 2 and "--devices" in r.stderr
    na = tmp_path / "na.tsv"
    na.write_text("cluster_id\tsequence\tno_label\n1\tWVTAPRSLPVLP\t1\nNA\tWVTAPRSLPVLA\t1\n")
    r = cli("separation", "-i", str(na), "-d", str(tmp_path / "c"))
    assert r.returncode == 2 and "FileFormatException" in r.stderr
    short = tmp_path / "short.tsv"
    short.write_text("cluster_id\n1\n")
    r = cli("separation", "-i", str(short), "-d", str(tmp_path / "d"))
    assert r.returncode == 2 and "FileFormatException" in r.stderr
    r = cli("separation", "-i", str(good), "-d", str(tmp_path / "c"))   # the directory exists now
    assert r.returncode == 2 and "Output directory exists" in r.stderr
    r = cli("separation", "-i", str(tmp_path / "missing.tsv"), "-d", str(tmp_path / "e"))
    assert r.returncode != 0
    usage = cli("--help").stderr
    assert "hammock-hip separation -i <clusters.tsv> -d <directory> [--skip_singletons]" in usage and "(separation)" in usage


# ---- CPU: the inputs -----------------------------------------------------------------------------------------------------------

def _facts(name):
    outs, stats, ways, near_size = expect_full(name)
    near_sum = outs[1]
    return stats["n_misplaced"], int((ways > 1).sum()), int(((near_size > 0) & (near_sum < 0)).sum())


def test_the_inputs_hold_what_the_gpu_tests_claim():
    """the oracle's side alone (it passes before the call exists): no GPU test below can pass vacuously"""
    facts = {}
    for name in SIZED:
        _, _, off, mc, ncl, _, _, strings = input_set(name)
        sizes = np.bincount(mc, minlength=ncl)
        assert off.size - 1 == 3383 and ncl == 24 and len(set(strings)) == 3383
        assert sizes.min() >= 1                                                   # no slot is emptied by the relabelling
        facts[name] = _facts(name)
        print(name, "misplaced, tied nearest, negative nearest mean:", facts[name])
        assert facts[name][1] >= 1                                                # an exact tie on the nearest mean
        assert np.abs(scores(name) @ (mc[:, None] == np.arange(ncl)).astype(np.int64)).max() > 30000
    for seed in (0, 1):
        sizes = np.bincount(input_set(f"sized{seed}")[3])
        for s in (1, 2, 63, 64, 65, 256, 257, 513, 700):
            assert s in sizes
        assert facts[f"sized{seed}_relabelled"][0] >= 100                         # misplaced members
        assert not np.array_equal(input_set(f"sized{seed}")[3], input_set(f"sized{seed}_relabelled")[3])
    assert any(f[2] >= 1 for f in facts.values())                                 # a negative nearest mean
    assert facts["sized1"][2] >= 1 and facts["sized1_relabelled"][2] >= 1
    # the segments the rule gives 3,383 members, and the forced ones of the GPU tests, lie as those tests say
    cstart = np.r_[0, np.cumsum(np.bincount(input_set("sized0_relabelled")[3]))]
    for forced in (0, 255, 256, 257, 1000):
        length, count = segments(3383, forced)
        inside = []   # segments wholly inside one slot that touch neither of its ends
        for s in range(count):
            a, b = s * length, min(3383, (s + 1) * length)
            c = int(np.searchsorted(cstart, a, "right")) - 1
            if cstart[c] < a and b < cstart[c + 1]:
                inside.append((s, c))
        if forced != 1000:
            assert {c for _, c in inside} >= ({10, 23} if forced else {10}), (forced, inside)   # in a slot of 700 members and in the slot of 513
    S, sub = scores("sized0")[:300, :300], np.arange(300) % 70
    assert np.array_equal(slot_sums(S, sub, 70, onehot=True), slot_sums(S, sub, 70, onehot=False))
    # ties: the two copy slots have equal means at unequal sizes, and the first of them is every non-copy member's nearest
    _, _, _, mc, ncl, _, _, strings = input_set("ties")
    outs, stats, ways, near_size = expect_full("ties")
    copy = np.isin(mc, (1, 3))
    assert len({s for s, c in zip(strings, copy) if c}) == 1 and copy.sum() == 70 and np.bincount(mc)[[1, 3]].tolist() == [30, 40]
    assert (outs[2][~copy] == 1).all() and (ways[~copy] >= 2).all() and (near_size[~copy] == 30).all()
    one = int(scores("ties")[np.flatnonzero(copy)[0], np.flatnonzero(copy)[1]])
    assert (outs[0][mc == 1] == 29 * one).all() and (outs[2][mc == 1] == 3).all() and (outs[1][mc == 1] == 40 * one).all()
    assert (outs[0][mc == 3] == 39 * one).all() and (outs[2][mc == 3] == 1).all() and (outs[1][mc == 3] == 30 * one).all()
    assert not outs[3][copy].any()                                                # own mean == nearest mean: not misplaced


def test_the_oracle_scores_both_orientations_equally():
    """the kernel scores (partner, member) whichever index is larger: on every input of this file the oracle gives an unordered pair
    one score (a symmetric matrix; unequal lengths fix the roles by length, equal lengths map shift s to -s)"""
    for name in ("sized0", "sized1", "ties"):
        M, res, off, _, _, X, p, _ = input_set(name)
        assert np.array_equal(score_matrix(M, res, off, X, p, both=True), scores(name))
    w = wide_case()
    assert np.array_equal(score_matrix(w["M"], w["dres"], w["doff"], 0, 0, both=True), w["D"] - np.diag(np.diag(w["D"])))
    M, res, off, _ = musi_case(None)
    score_matrix(M, res, off, 3, 0, both=True)


# ---- beyond 32 bits ----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def wide_case():
    """Words of 32 residues under test_score_key_ends' matrix (W/B against W/B 1,000, C against D/E/N/Q -1,000) at (0, 0):
        slot 0   300 distinct W/B words, 230 copies of each: 69,000 members, every pair 32,000 -- a member's own sum is 2.2 x 10^9
        slot 1   30 distinct W/B words, 20 copies of each: 600 members, as near to slot 0 as to their own
        slot 2   40 distinct C words with up to 3 of D/E/N/Q: far from everything
    Members of one string are copies, so the oracle scores the 370 distinct strings against each other and themselves, and the sums
    follow with the copies' counts.  -> the matrix, the set, the slots, the distinct strings with their score matrix D"""
    from oracle import c_oracle
    from test_score_key_ends import ends_matrix
    M = ends_matrix()
    rng = np.random.default_rng(41)
    code = {ch: LETTERS.index(ch) for ch in "WBCDENQ"}
    words, seen = [], set()

    def distinct(count, make):
        out = []
        while len(out) < count:
            q = make()
            if q.tobytes() not in seen:
                seen.add(q.tobytes())
                out.append(q)
        return out

    def wb():
        return np.where(rng.integers(0, 2, size=32) == 1, code["W"], code["B"]).astype(np.uint8)

    def cs():
        q = np.full(32, code["C"], dtype=np.uint8)
        for pos in rng.choice(32, size=int(rng.integers(0, 4)), replace=False):
            q[pos] = code["DENQ"[int(rng.integers(0, 4))]]
        return q

    plan = [(distinct(300, wb), 230, 0), (distinct(30, wb), 20, 1), (distinct(40, cs), 1, 2)]
    dslot, dcount = [], []
    for group, copies, slot in plan:
        words += group
        dslot += [slot] * len(group)
        dcount += [copies] * len(group)
    dslot, dcount = np.asarray(dslot), np.asarray(dcount)
    dres, doff = hammock_amd.pack_sequences(words)
    nd = len(words)
    ii, jj = np.repeat(np.arange(nd), nd), np.tile(np.arange(nd), nd)
    st, sc = c_oracle.score_pairs(M, dres, doff, np.maximum(ii, jj), np.minimum(ii, jj), 0, 0, 0)
    assert st == 0
    D = sc.astype(np.int64).reshape(nd, nd)
    which = np.repeat(np.arange(nd), dcount)
    which = which[rng.permutation(which.size)]                  # the member -> its distinct string, no slot contiguous
    res, off = hammock_amd.pack_sequences([words[k] for k in which])
    mc = dslot[which].astype(np.uint32)
    # sums per (distinct string, slot): every copy of every string of the slot, less the member itself in its own slot
    counts = np.zeros((nd, 3), dtype=np.int64)
    counts[np.arange(nd), dslot] = dcount
    dsums = D @ counts
    dsums[np.arange(nd), dslot] -= np.diag(D)
    return {"M": M, "res": res, "off": off, "mc": mc, "ncl": 3, "dres": dres, "doff": doff, "D": D, "sums": dsums[which], "n": which.size}


def test_the_wide_input_passes_32_bits():
    """on the CPU, with the oracle, before the GPU case is trusted: sums beyond 2^31, cross-products beyond 2^40, all inside the
    header's bounds"""
    w = wide_case()
    sums, mc = w["sums"], w["mc"].astype(np.int64)
    sizes = np.bincount(mc)
    assert w["n"] == 69640 and sizes.tolist() == [69000, 600, 40]
    own = sums[np.arange(w["n"]), mc]
    assert own[mc == 0].min() == 68999 * 32000 > 2 ** 31 and (np.abs(sums) <= 2 ** 15 * sizes[None, :]).all()
    outs, stats, ways, near_size = reduce_sums(sums, mc, 3)
    # a member of slot 1 compares slot 0's 2.2 x 10^9 over 69,000 with slot 2's sum over 40, and its own 599 x 32,000 with slot 0's
    assert (outs[2][mc == 1] == 0).all() and (outs[1][mc == 1] == 69000 * 32000).all()
    assert int(outs[0][mc == 1][0]) * 69000 > 2 ** 40 and int(outs[1][mc == 1][0]) * 599 > 2 ** 40   # the two sides of `misplaced`
    assert not outs[3][mc != 2].any()                         # 32,000 on both sides: equal means, strictly
    assert (outs[1][mc == 2] < 0).all() and stats["n_misplaced"] == int(outs[3][mc == 2].sum())
    assert stats["n_segments"] == 16 and np.abs(sums).max() * 69000 < 2 ** 61


# ---- MUSI (the clustering calls' clusters; the CLI) ----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def musi_case(count):
    with open(os.path.join(GOLDEN, "musi.fa")) as fh:
        seqs = list(dict.fromkeys(line.strip() for line in fh if line.strip() and not line.startswith(">")))[:count]
    res, off = hammock_amd.pack_sequences(seqs)
    return _blosum62(), res, off, seqs


# ---- GPU -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("cap", [0, 1, 3])
@pytest.mark.parametrize("name", SIZED)
def test_sized_families_match_the_oracle(gpu, monkeypatch, capfd, name, cap):
    """every output and every statistics field; under HMK_TEST_GRID_CAP the item loop of the walk and the member loop of the merge go
    beyond their first iteration, and both kernels say so"""
    M, res, off, mc, ncl, X, p, _ = input_set(name)
    ctx = device_ctx(M, res, off)
    if cap:
        monkeypatch.setenv("HMK_TEST_GRID_CAP", str(cap))
    got, stats = separation(ctx, capfd, cap, 0, 3383, mc, ncl, X, p)
    check(got, expect_full(name), stats)
    assert stats.n_segments == 13 and stats.launches == 2


@pytest.mark.gpu
@pytest.mark.parametrize("forced", [255, 256, 257, 1000])
def test_forced_segment_lengths(gpu, monkeypatch, capfd, forced):
    """segments one place short of a staged chunk, a chunk, a chunk and one place, and four chunks less 24; at the first three the
    slots of 700 and 513 members hold whole segments, whose one open piece is first and last at once"""
    M, res, off, mc, ncl, X, p, _ = input_set("sized0_relabelled")
    ctx = device_ctx(M, res, off)
    monkeypatch.setenv("HMK_TEST_SEPARATION_SEGMENT", str(forced))
    got, stats = separation(ctx, capfd, 0, 0, 3383, mc, ncl, X, p, forced)
    want = expect(scores("sized0"), mc, ncl, forced)
    check(got, want, stats)
    assert stats.n_segments == -(-3383 // forced)
    monkeypatch.delenv("HMK_TEST_SEPARATION_SEGMENT")
    got, stats = separation(ctx, capfd, 0, 0, 3383, mc, ncl, X, p)
    check(got, expect_full("sized0_relabelled"), stats)


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [0, 3])
@pytest.mark.parametrize("forced", [1, 2, 7, 64])
def test_short_segments_on_a_sub_range(gpu, monkeypatch, capfd, forced, cap):
    """600 members from 1,001 on, their slots renumbered densely: every place, every second, ... closes a segment"""
    M, res, off, mc, _, X, p, _ = input_set("sized0_relabelled")
    r0, r1 = 1001, 1601
    _, sub = np.unique(mc[r0:r1], return_inverse=True)
    ncl = int(sub.max()) + 1
    assert ncl >= 20 and np.bincount(sub).max() > 64
    ctx = device_ctx(M, res, off)
    monkeypatch.setenv("HMK_TEST_SEPARATION_SEGMENT", str(forced))
    if cap:
        monkeypatch.setenv("HMK_TEST_GRID_CAP", str(cap))
    got, stats = separation(ctx, capfd, cap, r0, r1, sub, ncl, X, p, forced)
    check(got, expect(scores("sized0")[r0:r1, r0:r1], sub, ncl, forced), stats)
    assert stats.n_segments == -(-600 // forced)


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [0, 1])
def test_range_sizes_and_degenerate_clusterings(gpu, monkeypatch, capfd, cap):
    """ranges of 1, 2, T - 1, T, T + 1 and 2 T + 1 members at two offsets, as singletons, as one slot and as two slots"""
    M, res, off, _, _, X, p, _ = input_set("sized1")
    ctx = device_ctx(M, res, off)
    if cap:
        monkeypatch.setenv("HMK_TEST_GRID_CAP", str(cap))
    S = scores("sized1")
    for s in (1, 2, T - 1, T, T + 1, 2 * T + 1):
        for r0 in (0, 301):
            sub = S[r0:r0 + s, r0:r0 + s]
            forms = [(np.arange(s), s), (np.zeros(s, dtype=np.int64), 1)]
            if s >= 2:
                forms.append(((np.arange(s) >= s // 2).astype(np.int64), 2))
            for mc, ncl in forms:
                got, stats = separation(ctx, capfd, cap, r0, r0 + s, mc, ncl, X, p)
                check(got, expect(sub, mc, ncl), stats)
                if ncl == 1:
                    assert (got[2] == UINT32_MAX).all() and not got[1].any() and not got[3].any() and stats.n_misplaced == 0
                if ncl == s:
                    assert not got[0].any() and not got[3].any()
    with pytest.raises(hammock_amd.DataException):   # a shift as long as the longest member
        ctx.cluster_separation_shifted(0, 100, np.zeros(100), 1, 12, p)


@pytest.mark.gpu
@pytest.mark.parametrize("forced", [0, 16])
def test_exact_ties(gpu, monkeypatch, capfd, forced):
    """equal means at unequal sizes: the smaller slot index wins, and a copy whose own mean equals the other copy slot's is not
    misplaced; with every member a slot of its own, the nearest slot is the survey's best partner"""
    M, res, off, mc, ncl, X, p, _ = input_set("ties")
    n = off.size - 1
    ctx = device_ctx(M, res, off)
    if forced:
        monkeypatch.setenv("HMK_TEST_SEPARATION_SEGMENT", str(forced))
    got, stats = separation(ctx, capfd, 0, 0, n, mc, ncl, X, p, forced)
    check(got, expect(scores("ties"), mc, ncl, forced), stats)
    copy = np.isin(mc, (1, 3))
    assert (got[2][~copy] == 1).all() and (got[2][mc == 1] == 3).all() and (got[2][mc == 3] == 1).all() and not got[3][copy].any()
    for name, r0, r1 in (("ties", 0, n), ("sized0", 700, 1400)):
        M, res, off, _, _, X, p, _ = input_set(name)
        ctx = device_ctx(M, res, off)
        got, stats = separation(ctx, capfd, 0, r0, r1, np.arange(r1 - r0), r1 - r0, X, p, forced)
        check(got, expect(scores(name)[r0:r1, r0:r1], np.arange(r1 - r0), r1 - r0, forced), stats)
        _, (best, index, _), _ = ctx.score_survey_shifted(r0, r1, r0, r1, X, p, 0)
        assert np.array_equal(got[1], best.astype(np.int64)) and np.array_equal(got[2].astype(np.int64) + r0, index.astype(np.int64))


@pytest.mark.gpu
def test_sums_and_products_beyond_32_bits(gpu, capfd):
    w = wide_case()
    ctx = device_ctx(w["M"], w["res"], w["off"])
    got, stats = separation(ctx, capfd, 0, 0, w["n"], w["mc"], 3, 0, 0)
    check(got, reduce_sums(w["sums"], w["mc"], 3), stats)
    assert got[0].max() > 2 ** 31 and stats.pairs_scored == 69640 * 69639


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sized0", "sized1_relabelled"])
def test_own_sums_equal_the_align_calls_member_sums(gpu, name):
    M, res, off, mc, ncl, X, p, _ = input_set(name)
    ctx = device_ctx(M, res, off)
    for r0, r1 in ((0, 3383), (500, 2900)):
        _, sub = np.unique(mc[r0:r1], return_inverse=True)
        got = ctx.cluster_separation_shifted(r0, r1, sub, int(sub.max()) + 1, X, p, flags=False, clusters=False)
        member_sum = ctx.cluster_align_shifted(r0, r1, sub, int(sub.max()) + 1, X, p)[3]
        assert got[3] is None and got[4] is None and got[5] is None
        assert np.array_equal(got[0], member_sum) and np.abs(member_sum).max() > 10000


@pytest.mark.gpu
def test_state_between_calls(gpu, monkeypatch, capfd):
    """one context: another clustering, other ranges, parameters and segment lengths in between, then the first call again, equal to
    the first; and the same call twice in a row"""
    M, res, off, mc, ncl, X, p, _ = input_set("sized0")
    mc2 = input_set("sized0_relabelled")[3]
    ctx = device_ctx(M, res, off)
    first, stats = separation(ctx, capfd, 0, 0, 3383, mc, ncl, X, p)
    check(first, expect_full("sized0"), stats)
    kept = [getattr(stats, k) for k in STAT_NAMES]
    got, stats = separation(ctx, capfd, 0, 0, 3383, mc2, ncl, X, p)
    check(got, expect_full("sized0_relabelled"), stats)
    got, stats = separation(ctx, capfd, 0, 40, 340, np.arange(300) % 7, 7, X, p)
    check(got, expect(scores("sized0")[40:340, 40:340], np.arange(300) % 7, 7), stats)
    monkeypatch.setenv("HMK_TEST_SEPARATION_SEGMENT", "300")
    got, stats = separation(ctx, capfd, 0, 0, 3383, mc2, ncl, X, p, 300)
    check(got, expect(scores("sized0"), mc2, ncl, 300), stats)
    monkeypatch.delenv("HMK_TEST_SEPARATION_SEGMENT")
    got = ctx.cluster_separation_shifted(0, 3383, np.zeros(3383), 1, 2, -1)   # other parameters, one slot
    assert (got[2] == UINT32_MAX).all()
    for _ in range(2):
        again, stats = separation(ctx, capfd, 0, 0, 3383, mc, ncl, X, p)
        assert all(np.array_equal(a, b) for a, b in zip(first, again)) and [getattr(stats, k) for k in STAT_NAMES] == kept


@pytest.mark.gpu
def test_device_list_runs_on_the_root(gpu, capfd):
    M, res, off, mc, ncl, X, p, _ = input_set("sized1_relabelled")
    ctx = hammock_amd.Context(M, device=[0, 0])
    ctx.set_sequences(residues=res, offsets=off)
    got, stats = separation(ctx, capfd, 0, 0, 3383, mc, ncl, X, p)
    check(got, expect_full("sized1_relabelled"), stats)


def _mean(a, b):
    return "%.4f" % (a / b)


def _separation_files(seqs, ids, mc, outs):
    """the two files from the oracle's numbers; ids[c] = the cluster id of slot c"""
    own, near_sum, near, misplaced, cl_mis, cl_own = outs
    sizes = np.bincount(mc, minlength=len(ids))
    rows = ["sequence\tcluster_id\tcluster_members\town_sum\town_mean\tnearest_cluster_id\tnearest_members\tnear_sum\tnear_mean\tmargin\tmisplaced"]
    for k, s in enumerate(seqs):
        size = int(sizes[mc[k]])
        own_mean = int(own[k]) / (size - 1) if size > 1 else None
        row = [s, ids[mc[k]], size, own[k], "NA" if own_mean is None else "%.4f" % own_mean]
        if near[k] == UINT32_MAX:
            row += ["NA"] * 5
        else:
            near_mean = int(near_sum[k]) / int(sizes[near[k]])
            row += [ids[near[k]], sizes[near[k]], near_sum[k], "%.4f" % near_mean, "NA" if own_mean is None else "%.4f" % (own_mean - near_mean)]
        rows.append("\t".join(str(v) for v in row + [misplaced[k]]))
    cl = ["cluster_id\tmembers\town_mean\tmisplaced_members"]
    cl += [f"{ids[c]}\t{sizes[c]}\t{_mean(int(cl_own[c]), int(sizes[c]) * (int(sizes[c]) - 1)) if sizes[c] > 1 else 'NA'}\t{cl_mis[c]}"
           for c in range(len(ids))]
    return "\n".join(rows) + "\n", "\n".join(cl) + "\n"


@pytest.mark.gpu
def test_cli_separation_on_greedy_clusters(gpu, coracle, tmp_path):
    """`separation` on greedy's stage-1 file of MUSI writes what the oracle's numbers say, byte for byte, with the singletons and
    without them; a file of one cluster has NA in the nearest columns"""
    r = cli("greedy", "-i", os.path.join(GOLDEN, "musi.fa"), "-d", str(tmp_path / "g"), timeout=600)
    assert r.returncode == 0, r.stderr
    cfile = tmp_path / "g" / "initial_clusters_sequences.tsv"
    M = _blosum62()
    loaded = read_cluster_file(cfile)   # (cluster id, sequence, size) per line
    for skip in (False, True):
        members = {}
        for c, s, _ in loaded:
            members.setdefault(c, []).append(s)   # clusters in file order, members in line order: the loader's
        ids = [c for c in members if len(members[c]) > 1 or not skip]
        seqs = [s for c in ids for s in members[c]]
        mc = np.repeat(np.arange(len(ids)), [len(members[c]) for c in ids])
        lens = [len(s) for s in (s for _, s, _ in loaded)]
        X = min(int(np.floor(sum(lens) / len(lens) / 4 + 0.5)), min(lens) - 1)
        res, off = hammock_amd.pack_sequences(seqs)
        outs, stats, _, _ = expect(score_matrix(M, res, off, X, 0), mc, len(ids))
        assert stats["n_misplaced"] > 0 and stats["n_multi"] > 20 and (len(ids) < len(members)) == skip
        want_members, want_clusters = _separation_files(seqs, ids, mc, outs)
        out = tmp_path / ("s" + str(int(skip)))
        r = cli("separation", "-i", str(cfile), "-d", str(out), *(["--skip_singletons"] if skip else []), timeout=600)
        assert r.returncode == 0, r.stderr
        assert "Max shift not set. Setting automatically to: " + str(X) in r.stderr
        assert f"Clusters: {len(ids)}, sequences: {len(seqs)}, pairs scored: {len(seqs) * (len(seqs) - 1)}, GPU kernels: " in r.stderr
        assert f"{stats['n_misplaced']} of {len(seqs)} sequences are closer to another cluster than to their own" in r.stderr
        assert (out / "member_separation.tsv").read_text() == want_members
        assert (out / "cluster_separation.tsv").read_text() == want_clusters
    one = tmp_path / "one.tsv"
    one.write_text("cluster_id\tsequence\tno_label\n4\tWVTAPRSLPVLP\t1\n4\tWVTAPRSLPVLA\t1\n")
    r = cli("separation", "-i", str(one), "-d", str(tmp_path / "o"), "-x", "3", timeout=600)
    assert r.returncode == 0, r.stderr
    st, sc = coracle.score_pairs(M, *hammock_amd.pack_sequences(["WVTAPRSLPVLP", "WVTAPRSLPVLA"]), [1], [0], 0, 3, 0)
    assert (tmp_path / "o" / "member_separation.tsv").read_text().splitlines()[1:] == [
        f"WVTAPRSLPVLP\t4\t2\t{sc[0]}\t{sc[0]}.0000\tNA\tNA\tNA\tNA\tNA\t0", f"WVTAPRSLPVLA\t4\t2\t{sc[0]}\t{sc[0]}.0000\tNA\tNA\tNA\tNA\tNA\t0"]
    assert (tmp_path / "o" / "cluster_separation.tsv").read_text().splitlines()[1:] == [f"4\t2\t{sc[0]}.0000\t0"]
