"""Centre-star alignment of given clusters around their medoids: hmk_cluster_align_shifted (k_align.hip) and `hammock-hip align`.

CPU part (host-only context): the symbol, every argument check, DeviceError for a valid call, the mode's argument and file errors,
aligned_rows, and one test of the INPUTS with the C oracle alone: that the families hold what the GPU tests claim to exercise.
GPU part: all outputs and the statistics bit-exact against an expectation built from the C oracle alone -- score_pairs over the
enumerated inside pairs (seq1 = the larger index) summed per member in int64, arg-max with the smallest-index rule,
shifted_score(centre, member) for score and shift, column, width and rows from those.  Each input's expectation is computed once.
    sized_families (test_linkage)   slots of 256 / 257 / 513 / 700 members: the flat/tiled boundary (LINK_FLAT_MAX) and the tile
                                    boundaries (LINK_TILE); two 2-member slots (a tie on the sum by construction)
    window_family                   windows of a 16-residue parent: shifts of both signs and beyond max_shift, negative pair scores
    copies_family                   70 copies of one string: every sum ties, the smallest index is the centre
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN
from test_assign import gpu   # noqa: F401  (the fixture that skips where no HIP device is visible)
from test_continue import cli, read_cluster_file
from test_linkage import _blosum62, _musi, device_ctx, inside_pairs, sized_families

import hammock_amd
from hammock_amd import _native as N

INT32_MAX = 2 ** 31 - 1
LETTERS = hammock_amd.AMINO_ACIDS
GRID_LINE = re.compile(r"^\[hmk grid\] (\S+) (\d+) -> (\d+)$", re.M)
WINDOW_SIZES = [2, 3, 5, 17, 63, 64, 65, 130, 257, 300]
WINDOW_PARAMS = [(3, 0), (3, -1), (2, -1)]
NAMES = ("center", "center_sum", "width", "member_sum", "center_score", "shift", "column")


# ---- inputs ----------------------------------------------------------------------------------------------------------------

def window_family(seed):
    """per slot a random parent of 16 residues; each member a window of length 10-12 at offset 0-4 with 0-2 substitutions; all strings
    distinct, members shuffled -> (peptides, member_cluster, n_clusters)"""
    rng = np.random.default_rng(99_000 + seed)
    peps, mc, seen = [], [], set()
    for c, size in enumerate(WINDOW_SIZES):
        parent = rng.integers(0, 20, size=16).astype(np.uint8)
        added = 0
        while added < size:
            length, offset = int(rng.integers(10, 13)), int(rng.integers(0, 5))
            q = parent[offset:offset + length].copy()
            for pos in rng.choice(length, size=int(rng.integers(0, 3)), replace=False):
                q[pos] = rng.integers(0, 20)
            if q.tobytes() in seen:
                continue
            seen.add(q.tobytes())
            peps.append(q)
            mc.append(c)
            added += 1
    perm = rng.permutation(len(peps))
    return [peps[k] for k in perm], np.asarray(mc, dtype=np.uint32)[perm], len(WINDOW_SIZES)


def copies_family():
    """a slot of 70 copies of one string between the small slots of a window family"""
    peps, mc, _ = window_family(2)
    keep = np.flatnonzero(np.isin(mc, [0, 1, 2, 3, 5]))   # slots of 2, 3, 5, 17, 64 members
    peps = [peps[k] for k in keep]
    mc = np.unique(mc[keep], return_inverse=True)[1]
    rng = np.random.default_rng(99_500)
    one = rng.integers(0, 20, size=11).astype(np.uint8)
    at = np.sort(rng.choice(len(peps) + 70, size=70, replace=False))   # where the copies go: not contiguous
    out_p, out_c, src = [], [], 0
    for k in range(len(peps) + 70):
        if k in set(at.tolist()):
            out_p.append(one.copy())
            out_c.append(5)
        else:
            out_p.append(peps[src])
            out_c.append(int(mc[src]))
            src += 1
    return out_p, np.asarray(out_c, dtype=np.uint32), 6


def expectation(coracle, M, res, off, mc, ncl, X, p, r0=0):
    """the seven outputs and (pairs_scored, n_multi, max_width) from the C oracle alone; also the scored pairs"""
    mc = np.asarray(mc, dtype=np.int64)
    nm = mc.size
    a, b, slot = inside_pairs(mc, r0)
    st, sc = coracle.score_pairs(M, res, off, b, a, 0, X, p)   # seq1 = the larger index
    assert st == 0
    sc = sc.astype(np.int64)
    member_sum = np.zeros(nm, dtype=np.int64)
    np.add.at(member_sum, a - r0, sc)
    np.add.at(member_sum, b - r0, sc)
    seq = lambda k: res[int(off[k]):int(off[k + 1])]   # noqa: E731
    center = np.zeros(ncl, dtype=np.int64)
    center_sum = np.zeros(ncl, dtype=np.int64)
    width = np.zeros(ncl, dtype=np.int64)
    center_score = np.full(nm, INT32_MAX, dtype=np.int64)
    shift = np.zeros(nm, dtype=np.int64)
    column = np.zeros(nm, dtype=np.int64)
    lens = (off[1:].astype(np.int64) - off[:-1].astype(np.int64))[r0:r0 + nm]
    extra = n_multi = 0
    for c in range(ncl):
        m = np.flatnonzero(mc == c)
        z = int(m[np.argmax(member_sum[m])])   # the first of equal maxima: the smallest index
        center[c], center_sum[c] = z + r0, member_sum[z]
        for k in m:
            if k != z:
                st, center_score[k], shift[k] = coracle.shifted_score(M, seq(z + r0), seq(int(k) + r0), X, p)
                assert st == 0
        column[m] = shift[m] - shift[m].min()
        width[c] = (column[m] + lens[m]).max()
        if m.size > 1:
            n_multi += 1
            extra += m.size - 1
    want = (center, center_sum, width, member_sum, center_score, shift, column)
    return want, (int(sc.size) + extra, n_multi, int(width.max()) if ncl else 0), (a, b, slot, sc)


@functools.lru_cache(maxsize=None)
def case(name):
    """a named input, packed, with its expectation (computed once per session)
    -> (M, res, off, mc, ncl, X, p, want, stats, scored, strings)"""
    from oracle import c_oracle
    if name.startswith("sized"):
        peps, mc, ncl, X, p, _ = sized_families(int(name[5:]))
    elif name.startswith("window"):
        seed, X, p = (int(v) for v in name[6:].split("_"))
        peps, mc, ncl = window_family(seed)
    else:
        assert name == "copies"
        (peps, mc, ncl), X, p = copies_family(), 3, -1
    res, off = hammock_amd.pack_sequences(peps)
    M = _blosum62()
    want, stats, scored = expectation(c_oracle, M, res, off, mc, ncl, X, p)
    strings = ["".join(LETTERS[r] for r in q) for q in peps]
    for arr in (res, off, mc) + want + scored:
        arr.setflags(write=False)
    return M, res, off, mc, ncl, X, p, want, stats, scored, strings


CASES = ["sized0", "sized1"] + [f"window{seed}_{X}_{p}" for seed in (0, 1) for X, p in WINDOW_PARAMS] + ["copies"]


def check(got, want, ctx=None, stats=None):
    for g, w, name in zip(got, want, NAMES):
        if g is None:
            continue
        assert np.array_equal(np.asarray(g, dtype=np.int64), w), name
    if stats is not None:
        s = ctx.last_align_stats
        assert (s.pairs_scored, s.n_multi, s.max_width) == stats


# ---- CPU: the symbol, the checks -------------------------------------------------------------------------------------------

def test_symbol_is_declared_bound_and_exported():
    with open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "hammock_hip.h")) as fh:
        header = fh.read()
    assert "int hmk_cluster_align_shifted(hmk_ctx *ctx" in header and "} hmk_align_stats;" in header
    assert "hmk_cluster_align_shifted" in N.SYMBOLS
    assert hasattr(N.lib, "hmk_cluster_align_shifted")
    assert N.lib.hmk_abi_version() == 4
    assert C.sizeof(N.AlignStats) == 32


OUT_TYPES = {"center": (np.uint32, C.c_uint32, 0), "center_sum": (np.int64, C.c_int64, 0), "width": (np.uint32, C.c_uint32, 0),
             "member_sum": (np.int64, C.c_int64, 1), "center_score": (np.int32, C.c_int32, 1), "shift": (np.int32, C.c_int32, 1),
             "column": (np.uint32, C.c_uint32, 1)}


def _raw_call(ctx, r0, r1, mc, ncl, X, p, null=()):
    """the C entry point with chosen arguments null -> status"""
    sizes = (max(ncl, 1), max(r1 - r0, 1))
    mc = None if mc is None else np.ascontiguousarray(mc, dtype=np.uint32)
    out = {k: np.zeros(sizes[which], dt) for k, (dt, _, which) in OUT_TYPES.items()}
    ptr = [None if k in null else out[k].ctypes.data_as(C.POINTER(OUT_TYPES[k][1])) for k in OUT_TYPES]
    return N.lib.hmk_cluster_align_shifted(ctx._h, r0, r1, None if mc is None else mc.ctypes.data_as(C.POINTER(C.c_uint32)), ncl, X, p,
                                           *ptr, None)


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
    for name in ("center", "center_sum", "width", "center_score", "shift", "column"):   # a null required output
        assert _raw_call(ctx, 0, 6, mc, 3, 3, 0, null=(name,)) == bad
        assert "null output" in N.lib.hmk_last_error(ctx._h).decode()
    with pytest.raises(ValueError):
        ctx.cluster_align_shifted(0, 6, [0, 0, 1, 1, 3, 3], 3, 3, 0)
    # an asymmetric matrix
    A = blosum62.copy()
    A[0, 1] += 1
    actx = hammock_amd.Context(A, device=-1)
    actx.set_sequences(residues=res, offsets=off)
    with pytest.raises(ValueError, match="symmetric"):
        actx.cluster_align_shifted(0, 6, mc, 3, 3, 0)
    # a valid call: no CPU fallback, with or without the sums, and for the inner range too
    assert _raw_call(ctx, 0, 6, mc, 3, 3, 0) == N.HMK_ERR_DEVICE
    assert _raw_call(ctx, 0, 6, mc, 3, 3, 0, null=("member_sum",)) == N.HMK_ERR_DEVICE
    with pytest.raises(hammock_amd.DeviceError):
        ctx.cluster_align_shifted(0, 6, mc, 3, 3, 0)
    with pytest.raises(hammock_amd.DeviceError):
        ctx.cluster_align_shifted(2, 6, [0, 0, 1, 1], 2, 3, 0, sums=False)


def test_cli_align_argument_and_file_errors(tmp_path):
    r = cli("align", "-d", str(tmp_path / "a"))
    assert r.returncode == 2 and "-i or --input" in r.stderr
    assert not (tmp_path / "a").exists()
    good = tmp_path / "good.tsv"
    good.write_text("cluster_id\tsequence\tno_label\n1\tWVTAPRSLPVLP\t1\n1\tWVTAPRSLPVLA\t1\n")
    r = cli("align", "-i", str(good), "--devices", "0,1", "-d", str(tmp_path / "b"))
    assert r.returncode == 2 and "--devices" in r.stderr
    na = tmp_path / "na.tsv"
    na.write_text("cluster_id\tsequence\tno_label\n1\tWVTAPRSLPVLP\t1\nNA\tWVTAPRSLPVLA\t1\n")
    r = cli("align", "-i", str(na), "-d", str(tmp_path / "c"))
    assert r.returncode == 2 and "FileFormatException" in r.stderr
    short = tmp_path / "short.tsv"
    short.write_text("cluster_id\n1\n")
    r = cli("align", "-i", str(short), "-d", str(tmp_path / "d"))
    assert r.returncode == 2 and "FileFormatException" in r.stderr
    r = cli("align", "-i", str(good), "-d", str(tmp_path / "c"))   # the directory exists now
    assert r.returncode == 2 and "Output directory exists" in r.stderr
    assert "hammock-hip align -i" in cli("--help").stderr


def test_aligned_rows_on_a_hand_written_slot():
    # centre ACDEFGHIK; shifts +2, -1, 0 against it -> the smallest is -1, so the columns are 3, 0, 1 (the centre's)
    seqs = ["DEFGHIK", "WACDEFGH", "ACDEFGHIK", "MNPQ"]
    rows = hammock_amd.aligned_rows(seqs, [3, 0, 1, 0], [10, 10, 10, 4])
    assert rows == ["---DEFGHIK", "WACDEFGH--", "-ACDEFGHIK", "MNPQ"]
    assert all(r.replace("-", "") == s for r, s in zip(rows, seqs))
    assert hammock_amd.aligned_rows([], [], []) == []
    with pytest.raises(ValueError):
        hammock_amd.aligned_rows(["ACDEF"], [2], [6])


def test_the_inputs_hold_what_the_gpu_tests_claim():
    """the oracle's side alone (it passes before the call exists): no GPU test below can pass vacuously"""
    for seed in (0, 1):
        M, res, off, mc, ncl, X, p, want, stats, (a, b, slot, sc), _ = case(f"sized{seed}")
        center, center_sum, width, member_sum, center_score, shift, column = want
        sizes = np.bincount(mc, minlength=ncl)
        assert mc.size == 3383 and sc.size == 748_228 and {256, 257, 513, 700} <= set(sizes.tolist())
        assert stats == (748_228 + int((sizes[sizes > 1] - 1).sum()), int((sizes > 1).sum()), int(width.max()))
        for c in np.flatnonzero(sizes == 2):   # a tie on the sum by construction: the smallest index decides
            m = np.flatnonzero(mc == c)
            assert member_sum[m[0]] == member_sum[m[1]] and center[c] == m[0]
        moved = shift[center_score != INT32_MAX]
        if seed == 0:
            assert not moved.any() and (width == 12).all()
        else:
            assert moved.size == 3359 and (moved != 0).sum() == 549 and (moved >= 0).all()
            assert width[sizes > 1].min() >= 10 and width.max() == 12
    for seed in (0, 1):
        beyond = []   # a shift beyond max_shift (through the length difference): asked of every seed, over its parameter sets --
        for X, p in WINDOW_PARAMS:   # seed 0 has -4 at all three, seed 1 has -3 at max_shift 2 and +-3 at max_shift 3
            M, res, off, mc, ncl, _, _, want, stats, (a, b, slot, sc), _ = case(f"window{seed}_{X}_{p}")
            center, center_sum, width, member_sum, center_score, shift, column = want
            assert mc.size == 906 and sc.size == 92_330
            moved = shift[center_score != INT32_MAX]
            assert moved.size == 896
            assert (moved < 0).sum() >= 200 and (moved > 0).sum() >= 200
            beyond.append(int(np.abs(moved).max()) > X)
            assert width.max() >= 15
            assert sc.min() < 0
            assert (column >= 0).all() and all(column[mc == c].min() == 0 for c in range(ncl))
        assert any(beyond) and (seed or all(beyond))
    M, res, off, mc, ncl, X, p, want, stats, _, strings = case("copies")
    m = np.flatnonzero(mc == 5)
    assert m.size == 70 and len({strings[k] for k in m}) == 1 and np.ptp(m) + 1 > 70
    assert len(set(want[3][m].tolist())) == 1 and want[0][5] == m[0] and not want[5][m].any() and want[2][5] == 11


# ---- GPU -------------------------------------------------------------------------------------------------------------------

def wanted_grids(mc, ncl):
    """kernel -> the grid its launcher asks for (k_align.hip's launchers)"""
    sizes = np.bincount(mc, minlength=ncl).astype(np.int64)
    multi = sizes[sizes > 1]
    flat, big = multi[multi <= 256], multi[multi > 256]
    tiles = -(-big // 256)
    by_member = min(-(-int(multi.sum()) // 256), 65536)
    grids = {"k_align_init": min(-(-max(ncl, mc.size) // 256), 4096), "k_align_center": by_member, "k_align_shift": by_member}
    if flat.size:
        grids["k_align_sums_flat"] = min(-(-int((flat * (flat - 1) // 2).sum()) // 256), 65536)
    if big.size:
        grids["k_align_sums_tiled"] = min(int((tiles * (tiles + 1) // 2).sum()), 65536)
    return grids


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [0, 1, 3])
@pytest.mark.parametrize("name", CASES)
def test_families_match_the_oracle(gpu, monkeypatch, capfd, name, cap):
    """all outputs and the statistics, with and without the sums; under HMK_TEST_GRID_CAP every work loop goes beyond its first
    iteration, and every new kernel says so"""
    M, res, off, mc, ncl, X, p, want, stats, _, _ = case(name)
    ctx = device_ctx(M, res, off)
    if cap:
        monkeypatch.setenv("HMK_TEST_GRID_CAP", str(cap))
    capfd.readouterr()
    got = ctx.cluster_align_shifted(0, mc.size, mc, ncl, X, p)
    check(got, want, ctx, stats)
    assert got[0].dtype == np.uint32 and got[1].dtype == np.int64 and got[3].dtype == np.int64 and got[5].dtype == np.int32
    grids = wanted_grids(mc, ncl)
    s = ctx.last_align_stats
    assert s.launches == len(grids) and s.kernel_ms > 0
    bare = ctx.cluster_align_shifted(0, mc.size, mc, ncl, X, p, sums=False)
    assert bare[3] is None
    check(bare, want, ctx, stats)
    lines = {}
    for kernel, wanted, launched in GRID_LINE.findall(capfd.readouterr().err):
        lines.setdefault(kernel, set()).add((int(wanted), int(launched)))
    cut = {k: {(w, cap)} for k, w in grids.items() if cap and w > cap}
    assert {k: v for k, v in lines.items() if k.startswith("k_align_")} == cut
    if cap == 1 and name != "copies":   # a new kernel without a line under cap 1 would not have had its work loop tested
        assert set(cut) == {"k_align_init", "k_align_sums_flat", "k_align_sums_tiled", "k_align_center", "k_align_shift"}


def residue_rows(rows):
    """aligned rows of one width -> int array [rows, width], -1 where a row holds a gap"""
    index = {ch: k for k, ch in enumerate(LETTERS)}
    return np.array([[index.get(ch, -1) for ch in r] for r in rows], dtype=np.int64)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["window0_3_0", "window1_3_0", "sized0"])
def test_columns_reproduce_the_score_at_penalty_zero(gpu, name):
    """a property that does not trust the stated sign convention: at shift_penalty = 0 the matrix summed over the columns where the
    centre's row and the member's row both hold a residue is the member's center_score"""
    M, res, off, mc, ncl, X, p, _, _, _, strings = case(name)
    assert p == 0
    ctx = device_ctx(M, res, off)
    center, _, width, _, center_score, shift, column = ctx.cluster_align_shifted(0, mc.size, mc, ncl, X, p, sums=False)
    rows = hammock_amd.aligned_rows(strings, column, width[mc])
    assert all(len(r) == width[c] for r, c in zip(rows, mc))
    M2 = np.asarray(M, dtype=np.int64).reshape(24, 24)
    checked = 0
    for c in range(ncl):
        m = np.flatnonzero(mc == c)
        grid = residue_rows([rows[k] for k in m])
        zrow = grid[int(np.flatnonzero(m == center[c])[0])]
        for k, row in zip(m, grid):
            if k == center[c]:
                continue
            both = (zrow >= 0) & (row >= 0)
            assert int(M2[zrow[both], row[both]].sum()) == int(center_score[k]), (c, int(k))
            checked += 1
    assert checked == mc.size - int((np.bincount(mc, minlength=ncl) > 0).sum())


@pytest.mark.gpu
def test_member_sums_agree_with_the_linkage_call(gpu):
    """a member none of whose pairs is below t sums to at least (s - 1) t; and every member's sum is at least (s - 1) times its own
    minimum, whatever the threshold"""
    M, res, off, mc, ncl, X, p, _, _, _, _ = case("sized1")
    thr = sized_families(1)[5]
    ctx = device_ctx(M, res, off)
    link = ctx.cluster_linkage_shifted(0, mc.size, mc, ncl, X, p, thr)
    got = ctx.cluster_align_shifted(0, mc.size, mc, ncl, X, p)
    s = np.bincount(mc, minlength=ncl)[mc].astype(np.int64)
    clean = (link[5] == 0) & (s > 1)
    assert clean.sum() > 500 and (~clean & (s > 1)).sum() > 100
    assert (got[3][clean] >= (s[clean] - 1) * thr).all()
    multi = s > 1
    assert (got[3][multi] >= (s[multi] - 1) * link[4][multi].astype(np.int64)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["window0_3_-1", "sized1"])
def test_center_scores_equal_score_with_shift(gpu, name):
    M, res, off, mc, ncl, X, p, _, _, _, _ = case(name)
    ctx = device_ctx(M, res, off)
    center, _, _, _, center_score, shift, _ = ctx.cluster_align_shifted(0, mc.size, mc, ncl, X, p, sums=False)
    m = np.flatnonzero(center[mc] != np.arange(mc.size))
    assert m.size == mc.size - ncl + int((np.bincount(mc, minlength=ncl) == 0).sum())
    score, sh = ctx.score_with_shift(center[mc][m], m, X, p)
    assert np.array_equal(score, center_score[m]) and np.array_equal(sh, shift[m])
    z = np.flatnonzero(center[mc] == np.arange(mc.size))
    assert (center_score[z] == INT32_MAX).all() and not shift[z].any()


@pytest.mark.gpu
def test_state_between_calls(gpu, coracle):
    """one context; other slots, an inner range, permuted slot numbers, other parameters: nothing stays behind, a repeated call
    repeats its result"""
    peps, _, _ = window_family(3)
    rng = np.random.default_rng(99_100)
    M = _blosum62()
    res, off = hammock_amd.pack_sequences(peps)
    n = len(peps)
    ctx = device_ctx(M, res, off)

    def slots(sizes, count):
        mc = np.repeat(np.arange(len(sizes)), sizes)
        assert mc.size == count
        return rng.permutation(mc).astype(np.uint32)

    def run(r0, r1, mc, X, p, **kw):
        ncl = int(mc.max()) + 1
        want, stats, _ = expectation(coracle, M, res, off, mc, ncl, X, p, r0)
        got = ctx.cluster_align_shifted(r0, r1, mc, ncl, X, p, **kw)
        check(got, want, ctx, stats)
        return got

    mc_a = slots([300, 260, 150, 100, 64, 20, 6, 3, 2, 1], n)
    mc_b = slots([1, 400, 2, 257, 200, 46], n)
    mc_c = slots([270, 100, 1, 27, 2], 400)
    first = run(0, n, mc_a, 3, 0)
    run(0, n, mc_b, 3, 0)                  # a different slot assignment
    run(0, n, mc_a, 2, -1)                 # other parameters
    run(150, 550, mc_c, 3, -1)             # a range in the middle of the uploaded set
    for _ in range(2):
        again = run(0, n, mc_a, 3, 0)
        assert all(np.array_equal(x, y) for x, y in zip(first, again))
    perm = rng.permutation(10)
    moved = run(0, n, perm[mc_a].astype(np.uint32), 3, 0)
    for x, y in zip(first[:3], moved[:3]):
        assert np.array_equal(x, y[perm])
    assert all(np.array_equal(x, y) for x, y in zip(first[3:], moved[3:]))
    bare = run(0, n, mc_a, 3, 0, sums=False)
    assert bare[3] is None and all(np.array_equal(x, y) for x, y in zip(first[:3] + first[4:], bare[:3] + bare[4:]))


@pytest.mark.gpu
def test_clusters_of_the_clustering_calls(gpu, coracle):
    """the clusters of hmk_greedy_cluster and hmk_clinkage_cluster on MUSI"""
    M = _blosum62()
    seqs = list(dict.fromkeys(_musi()))
    for name, count in (("greedy", len(seqs)), ("clinkage", 1000)):
        res, off = hammock_amd.pack_sequences(seqs[:count])
        ctx = device_ctx(M, res, off)
        cid = ctx.greedy_cluster(3, 0, 20, 2 ** 31 - 1)[0] if name == "greedy" else ctx.clinkage_cluster(3, 0, 20)[0]
        _, mc = np.unique(cid, return_inverse=True)
        ncl = int(mc.max()) + 1
        want, stats, _ = expectation(coracle, M, res, off, mc, ncl, 3, 0)
        assert stats[1] > 20, name
        check(ctx.cluster_align_shifted(0, count, mc, ncl, 3, 0), want, ctx, stats)


@pytest.mark.gpu
def test_singletons_and_degenerate_inputs(gpu, coracle):
    M, res, off, mc, ncl, X, p, _, _, _, _ = case("window0_3_0")
    ctx = device_ctx(M, res, off)
    lens = (off[1:] - off[:-1]).astype(np.int64)
    # singletons only
    got = ctx.cluster_align_shifted(10, 60, np.arange(50), 50, X, p)
    assert np.array_equal(got[0], np.arange(10, 60)) and not got[1].any() and np.array_equal(got[2], lens[10:60])
    assert not got[3].any() and (got[4] == INT32_MAX).all() and not got[5].any() and not got[6].any()
    s = ctx.last_align_stats
    assert (s.pairs_scored, s.n_multi, s.max_width, s.launches) == (0, 0, int(lens[10:60].max()), 0)
    # an empty range
    got = ctx.cluster_align_shifted(7, 7, [], 0, X, p)
    assert all(g.size == 0 for g in got) and ctx.last_align_stats.pairs_scored == 0
    got = ctx.cluster_align_shifted(7, 7, [], 0, X, p, sums=False)
    assert got[3] is None and got[0].size == 0
    # one slot holding everything, 300 members
    one = np.zeros(300, dtype=np.uint32)
    want, stats, _ = expectation(coracle, M, res, off, one, 1, X, p, 500)
    check(ctx.cluster_align_shifted(500, 800, one, 1, X, p), want, ctx, stats)
    assert stats[0] == 300 * 299 // 2 + 299


@pytest.mark.gpu
def test_device_list_runs_on_the_root(gpu):
    M, res, off, mc, ncl, X, p, want, stats, _, _ = case("window1_2_-1")
    ctx = hammock_amd.Context(M, device=[0, 0])
    ctx.set_sequences(residues=res, offsets=off)
    check(ctx.cluster_align_shifted(0, mc.size, mc, ncl, X, p), want, ctx, stats)


def _java_round(v):
    import math
    return int(math.floor(v + 0.5))


@pytest.mark.gpu
def test_cli_align_on_greedy_clusters(gpu, coracle, tmp_path):
    """`align` on greedy's stage-1 file of MUSI writes what the oracle's numbers say, byte for byte, and `check` reads the written
    cluster file as it reads the input"""
    r = cli("greedy", "-i", os.path.join(GOLDEN, "musi.fa"), "-d", str(tmp_path / "g"), timeout=600)
    assert r.returncode == 0, r.stderr
    cfile = tmp_path / "g" / "initial_clusters_sequences.tsv"
    M = _blosum62()
    lines = cfile.read_text().splitlines()
    head = lines[0].split("\t")
    assert head[:4] == ["cluster_id", "sequence", "alignment", "sum"]
    loaded = read_cluster_file(cfile)   # (cluster id, sequence, size) per line
    ids = list(dict.fromkeys(c for c, _, _ in loaded))   # clusters in file order, members in line order: the loader's
    slot = {c: k for k, c in enumerate(ids)}
    order = sorted(range(len(loaded)), key=lambda k: slot[loaded[k][0]])   # (stable) the upload: cluster by cluster
    seqs = [loaded[k][1] for k in order]
    mc = np.array([slot[loaded[k][0]] for k in order], dtype=np.uint32)
    lens = [len(s) for s in seqs]
    X = min(_java_round(sum(lens) / len(lens) / 4), min(lens) - 1)
    res, off = hammock_amd.pack_sequences(seqs)
    (center, center_sum, width, _, _, _, column), stats, _ = expectation(coracle, M, res, off, mc, len(ids), X, 0)
    rows = hammock_amd.aligned_rows(seqs, column, width[mc])
    row_of_line = {order[k]: rows[k] for k in range(len(order))}
    uniq = np.bincount(mc)
    assert stats[1] > 20 and (column > 0).any()

    def centers(skip):
        out = ["cluster_id\tsize\tcenter\tcenter_sum\twidth"]
        out += [f"{c}\t{uniq[k]}\t{seqs[center[k]]}\t{center_sum[k]}\t{width[k]}" for k, c in enumerate(ids) if uniq[k] > 1 or not skip]
        return "\n".join(out) + "\n"

    want_seq = [lines[0]]
    for k, line in enumerate(lines[1:]):
        f = line.split("\t")
        assert f[2] == ("NA" if uniq[slot[int(f[0])]] > 1 else f[1])   # what greedy wrote
        f[2] = row_of_line[k]
        want_seq.append("\t".join(f))
    for extra in ([], ["--skip_singletons"]):
        out = tmp_path / ("a" + str(len(extra)))
        r = cli("align", "-i", str(cfile), "-d", str(out), *extra, timeout=600)
        assert r.returncode == 0, r.stderr
        assert "Max shift not set. Setting automatically to: " + str(X) in r.stderr
        assert f"pairs scored: {stats[0]}, widest alignment: {stats[2]}, GPU kernels: " in r.stderr
        assert f"Clusters of more than one sequence: {stats[1]}," in r.stderr
        assert (out / "initial_clusters_sequences.tsv").read_text() == "\n".join(want_seq) + "\n"
        assert (out / "cluster_centers.tsv").read_text() == centers(bool(extra))
        files = sorted(os.listdir(out / "alignments_initial"))
        assert files == sorted(f"{c}.aln" for k, c in enumerate(ids) if uniq[k] > 1)
        for k, c in enumerate(ids):
            if uniq[k] > 1:
                m = np.flatnonzero(mc == k)
                text = "".join(f">{c}_{t + 1}\n{rows[j]}\n" for t, j in enumerate(m))
                assert (out / "alignments_initial" / f"{c}.aln").read_text() == text
    # every other mode's loader drops the alignment column: check reads the written file as it reads the input
    for name, path in (("in", cfile), ("out", tmp_path / "a0" / "initial_clusters_sequences.tsv")):
        r = cli("check", "-i", str(path), "-d", str(tmp_path / ("c" + name)), timeout=600)
        assert r.returncode == 0, r.stderr
    for f in ("cluster_linkage.tsv", "cluster_members.tsv"):
        assert (tmp_path / "cin" / f).read_text() == (tmp_path / "cout" / f).read_text()
    assert len((tmp_path / "cin" / "cluster_linkage.tsv").read_text().splitlines()) == len(ids) + 1
