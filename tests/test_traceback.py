"""Global alignment traceback (hmk_align_pairs_global, Context.align_pairs_global / align_edges_global, gapped_rows, star_rows,
`search --scorer global --alignments`, `align --scorer global`): the alignments behind GlobalAlignmentScorer's scores.  The
expectation is tests/traceback_ref.py -- the header's walk restated in plain Python over the recurrence's tables, tied here to
global_ref's brute force over all alignments -- and every comparison is exact.  The CPU tests run anywhere; the GPU tests need an
MI355X (-m gpu)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import gapped_ends as GE
import global_ref as G
import traceback_ref as R
import hammock_amd
from hammock_amd import _native as N

CLI = os.path.join(ROOT, "hammock_amd", "bin", "hammock-hip")
BAD_PENALTIES = ((-1, -5), (0, -1), (1, 1), (-5, 1), (3, 0), (-128, -1), (-128, -128), (-200, -1))
GOOD_PENALTIES = ((-5, -1), (0, 0), (-127, -127), (-127, 0))
GRID_LINE = re.compile(r"^\[hmk grid\] (\S+) (\d+) -> (\d+)$", re.M)


@pytest.fixture(scope="module")
def gpu():
    """skips the GPU tests where no HIP device is visible"""
    try:
        import torch
        ok = torch.cuda.is_available()
    except Exception:
        ok = False
    if not ok:
        pytest.skip("needs an MI355X (no HIP device visible)")
    return 0


def cli(*args, timeout=300):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=timeout)


def ctx_with(M, seqs, device=0):
    ctx = hammock_amd.Context(M, device=device)
    res, off = hammock_amd.pack_sequences(seqs)
    ctx.set_sequences(residues=res, offsets=off)
    return ctx


def raw_call(ctx, i, j, n_pairs, go, ge, null=()):
    """hmk_align_pairs_global itself -> its status; null: the outputs passed as NULL"""
    i, j = np.ascontiguousarray(i, dtype=np.uint32), np.ascontiguousarray(j, dtype=np.uint32)
    n = max(len(i), 1)
    out = {"score": (np.zeros(n, np.int32), C.c_int32), "n_cols": (np.zeros(n, np.uint8), C.c_uint8),
           "gap1": (np.zeros(n, np.uint64), C.c_uint64), "gap2": (np.zeros(n, np.uint64), C.c_uint64)}
    ptr = [None if k in null else a.ctypes.data_as(C.POINTER(t)) for k, (a, t) in out.items()]
    return N.lib.hmk_align_pairs_global(ctx._h, i.ctypes.data_as(C.POINTER(C.c_uint32)), j.ctypes.data_as(C.POINTER(C.c_uint32)), n_pairs,
                                        go, ge, *ptr)


# ---- CPU ----------------------------------------------------------------------------------------------------------------

def test_symbol_is_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "hammock_hip.h")) as fh:
        header = fh.read()
    assert "int hmk_align_pairs_global(" in header
    assert "hmk_align_pairs_global" in N.SYMBOLS and hasattr(N.lib, "hmk_align_pairs_global")
    assert N.lib.hmk_abi_version() == 4 and "#define HMK_ABI_VERSION 4" in header
    for name in ("gapped_rows", "star_rows"):
        assert name in hammock_amd.__all__ and callable(getattr(hammock_amd, name))
    assert callable(hammock_amd.Context.align_pairs_global) and callable(hammock_amd.Context.align_edges_global)


def test_argument_errors_on_a_host_only_context():
    """the penalties are answered before the device is looked at (HMK_ERR_BAD_ARG); everything valid ends at HMK_ERR_DEVICE"""
    ctx = hammock_amd.Context(GE.blosum62(), device=-1)
    ctx.set_sequences(["ACDEFGHIK", "ACDEFGHIKL", "MNPQRSTVW", "WYVACDEFG"])
    for go, ge in BAD_PENALTIES:
        with pytest.raises(ValueError):
            ctx.align_pairs_global([0, 1], [2, 3], go, ge)
        assert raw_call(ctx, [0, 1], [2, 3], 2, go, ge) == N.HMK_ERR_BAD_ARG
        assert raw_call(ctx, [], [], 0, go, ge) == N.HMK_ERR_BAD_ARG
    for go, ge in GOOD_PENALTIES:
        with pytest.raises(hammock_amd.DeviceError):
            ctx.align_pairs_global([0, 1], [2, 3], go, ge)
        assert raw_call(ctx, [0, 1], [2, 3], 2, go, ge) == N.HMK_ERR_DEVICE
        assert raw_call(ctx, [0, 9], [2, 3], 2, go, ge) == N.HMK_ERR_DEVICE   # (the indices are looked at behind the device)
    with pytest.raises(ValueError):
        ctx.align_pairs_global([0, 1], [2], -5, -1)
    assert N.lib.hmk_align_pairs_global(None, None, None, 0, -5, -1, None, None, None, None) == N.HMK_ERR_BAD_ARG
    with pytest.raises(ValueError):   # the edges' own scores are compared only behind a successful call
        ctx.align_edges_global(hammock_amd.pack_edges([0], [1], [3]), 1, 1)


def test_reference_walk_is_optimal_for_all_lengths_up_to_six():
    """the walk ends, its alignment rescored column by column scores H[n][m], and that is the best of ALL alignments"""
    rng = np.random.default_rng(61)
    for name in ("blosum", "edit", "zero", "asym"):
        M, go, ge, letters = R.family(name)
        Ml = [[int(v) for v in row] for row in M]
        for n in range(1, 7):
            for m in range(1, 7):
                for _ in range(3):
                    s1 = [letters[k] for k in rng.integers(0, len(letters), n)]
                    s2 = [letters[k] for k in rng.integers(0, len(letters), m)]
                    score, n_cols, gap1, gap2 = R.walk(s1, s2, Ml, go, ge)
                    assert score == G.global_score(s1, s2, M, go, ge) == G.brute_force(s1, s2, M, go, ge)
                    assert R.rescore(s1, s2, Ml, go, ge, n_cols, gap1, gap2) == score


def test_reference_records_of_the_gpu_inputs_rescore_to_their_scores():
    for name in R.FAMILIES:
        M, go, ge, _ = R.family(name)
        Ml = [[int(v) for v in row] for row in M]
        for cap in R.CAPS:
            seqs = R.capped(R.sequences(name), cap)
            score, n_cols, gap1, gap2 = R.expected(name, cap)
            n = len(seqs)
            assert n == 48 and score.shape == (n * n,)
            assert sorted(len(s) for s in R.sequences(name)) == sorted(4 * list(R.LENGTHS))
            assert max(len(s) for s in seqs) == cap
            for k in range(0, n * n, 7):
                a, b = divmod(k, n)
                assert R.rescore(seqs[a], seqs[b], Ml, go, ge, int(n_cols[k]), int(gap1[k]), int(gap2[k])) == score[k]
        T = G.global_table(list(R.sequences(name)), M, go, ge)
        assert np.array_equal(T.reshape(-1), R.expected(name)[0])
    assert R.family("lit1000")[0].max() == 1000 and R.family("lit1000")[0].min() == -1000
    assert R.expected("lit1000")[0].max() > 4000   # (beyond what an int8 profile could hold per cell times its length)


@pytest.mark.parametrize("name", R.FAMILIES)
def test_the_inputs_tell_every_slip_from_the_rule(name):
    """a walk that tries a gap before the diagonal, F before E, an opening before an extension, that takes seq1 for seq2 or stores
    its columns right to left differs from the rule on at least one pair of the GPU tests' own input, in every family"""
    counts = R.slip_counts(name)
    assert set(counts) == set(R.SLIPS)
    for slip, differing in counts.items():
        assert differing >= 1, (name, slip)


def test_gapped_rows_by_hand():
    for rows_of in (hammock_amd.gapped_rows, R.gapped_rows):
        # ACDEFGHIKL / ACDFGHIKL: the E of seq1 stands against a gap in seq2 (column 3)
        assert rows_of("ACDEFGHIKL", "ACDFGHIKL", 10, 0, 1 << 3) == ("ACDEFGHIKL", "ACD-FGHIKL")
        assert rows_of("ACDFGHIKL", "ACDEFGHIKL", 10, 1 << 3, 0) == ("ACD-FGHIKL", "ACDEFGHIKL")
        assert rows_of("CDE", "WWCDE", 5, 0b00011, 0) == ("--CDE", "WWCDE")        # a leading insertion
        assert rows_of("CDE", "CDEWW", 5, 0b11000, 0) == ("CDE--", "CDEWW")        # a trailing insertion
        assert rows_of("A", "W", 2, 0b01, 0b10) == ("-A", "W-")
        assert rows_of("A", "A", 1, 0, 0) == ("A", "A")
    for bad in ((10, 1 << 3, 1 << 3), (10, 0, 0), (10, 0, 1 << 10), (9, 0, 1 << 3)):
        with pytest.raises(ValueError):
            hammock_amd.gapped_rows("ACDEFGHIKL", "ACDFGHIKL", *bad)
    # ... and the reference's walk finds exactly that alignment under BLOSUM62, -5 / -1
    M = [[int(v) for v in row] for row in GE.blosum62()]
    a, b = [int(r) for r in hammock_amd.encode("ACDEFGHIKL")], [int(r) for r in hammock_amd.encode("ACDFGHIKL")]
    assert R.walk(a, b, M, -5, -1) == (47, 10, 0, 1 << 3)
    assert R.walk(b, a, M, -5, -1) == (47, 10, 1 << 3, 0)


def test_star_rows_by_hand():
    for star in (hammock_amd.star_rows, R.star_rows):
        center = "ACDFGHIKL"
        members = ["ACDEFGHIKL",    # one inserted residue before centre residue 3
                   "WWACDFGHIKL",   # a leading insertion of two
                   "ACDFGHIKLYY",   # a trailing insertion of two
                   "CDFGHIK",       # both end residues of the centre against gaps
                   "YACDEEFGHIKL"]  # a leading insertion of one, two inserted before residue 3
        records = [(10, 1 << 3, 0), (11, 0b11, 0), (11, 0b11 << 9, 0), (9, 0, 1 | 1 << 8), (12, 1 | 0b11 << 4, 0)]
        c_row, rows = star(center, members, records)
        assert c_row == "--ACD--FGHIKL--"
        assert rows == ["--ACDE-FGHIKL--",
                        "WWACD--FGHIKL--",
                        "--ACD--FGHIKLYY",
                        "---CD--FGHIK---",
                        "-YACDEEFGHIKL--"]
        assert all(r.replace("-", "") == m for r, m in zip(rows, members))
        assert star("ACD", [], []) == ("ACD", [])                      # a slot of one member is its own row
        assert star("ACD", ["ACD"], [(3, 0, 0)]) == ("ACD", ["ACD"])


def test_cli_argument_errors_need_no_device(tmp_path):
    fa = os.path.join(GOLDEN, "musi.fa")
    out = tmp_path / "out"
    for args, word in ((["search", "--database", fa, "--alignments"], "--alignments"),
                       (["search", "--database", fa, "--scorer", "shifted", "--alignments"], "--alignments"),
                       (["greedy", "--scorer", "global", "--alignments"], "--alignments"),
                       (["align", "--scorer", "global", "--alignments"], "--alignments"),
                       (["align", "--scorer", "bogus"], "--scorer"),
                       (["align", "--scorer", "global", "-x", "3"], "-x"),
                       (["align", "--scorer", "global", "-p", "0"], "-p"),
                       (["align", "--scorer", "global", "--gap_open", "-1", "--gap_extend", "-5"], "--gap_open"),
                       (["profile", "--scorer", "global", "--frequency_matrix", fa], "profile")):
        r = cli(args[0], "-i", fa, "-d", str(out), *args[1:])
        assert r.returncode == 2, (args, r.stderr)
        assert word in r.stderr
        assert not out.exists()
    r = cli("--help")
    assert "--alignments" in r.stderr and "align -i <clusters.tsv> -d <directory> --scorer global" in r.stderr


# ---- GPU ----------------------------------------------------------------------------------------------------------------

def family_ctx(name, cap=32):
    M, go, ge, _ = R.family(name)
    seqs = R.capped(R.sequences(name), cap)
    return ctx_with(M, list(seqs)), go, ge, seqs


def assert_records(got, want, where=None):
    for g, w, field in zip(got, want, ("score", "n_cols", "gap1", "gap2")):
        w = w if where is None else w[where]
        assert g.dtype == w.dtype, field
        bad = np.nonzero(g != w)[0]
        assert bad.size == 0, (field, bad[:5], g[bad[:5]], w[bad[:5]])


@pytest.mark.gpu
@pytest.mark.parametrize("name", R.FAMILIES)
def test_all_ordered_pairs_match_the_reference(gpu, name):
    """48 sequences of 1..32 residues, all 2,304 ordered pairs with the self pairs: every record equals the reference's, the scores
    equal score_pairs_global's, a second call gives the same"""
    ctx, go, ge, seqs = family_ctx(name)
    i, j = R.all_pairs(len(seqs))
    got = ctx.align_pairs_global(i, j, go, ge)
    assert_records(got, R.expected(name))
    assert np.array_equal(got[0], ctx.score_pairs_global(i, j, go, ge))
    again = ctx.align_pairs_global(i, j, go, ge)
    assert all(np.array_equal(a, b) for a, b in zip(got, again))
    lens = np.array([len(s) for s in seqs])
    pop1 = np.array([bin(int(v)).count("1") for v in got[2]])
    pop2 = np.array([bin(int(v)).count("1") for v in got[3]])
    assert not (got[2] & got[3]).any()
    assert np.array_equal(pop1, got[1] - lens[i]) and np.array_equal(pop2, got[1] - lens[j])


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [16, 24])
@pytest.mark.parametrize("name", R.FAMILIES)
def test_sets_of_shorter_sequences_and_the_pairs_they_share(gpu, name, cap):
    """the same sequences cut to 16 or 24 residues run the kernel's smaller instantiations: exact, and the pairs of two sequences
    within the cap get the records they get in the full set"""
    ctx, go, ge, seqs = family_ctx(name, cap)
    i, j = R.all_pairs(len(seqs))
    got = ctx.align_pairs_global(i, j, go, ge)
    assert_records(got, R.expected(name, cap))
    short = np.array([len(s) <= cap for s in R.sequences(name)])
    common = np.nonzero(short[i] & short[j])[0]
    assert common.size == (36 * 36 if cap == 16 else 44 * 44)
    full = family_ctx(name)[0].align_pairs_global(i[common], j[common], go, ge)
    assert all(np.array_equal(a[common], b) for a, b in zip(got, full))


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [1, 3])
@pytest.mark.parametrize("lmax", [32, 24, 16])
def test_work_loop_longest_pairs_first(gpu, monkeypatch, capfd, cap, lmax):
    """HMK_TEST_GRID_CAP: 36 (lmax 16: 9) workgroups' worth of pairs on 1 and 3, the list ordered longest first, so that every lane's
    later, shorter pair meets the direction bits its longer one left"""
    name = "edit"
    ctx, go, ge, seqs = family_ctx(name, lmax)
    i, j = R.all_pairs(len(seqs))
    lens = np.array([len(s) for s in seqs])
    order = np.lexsort((lens[j], lens[i]))[::-1]
    assert (np.diff(lens[i][order]) <= 0).all() and lens[i][order][0] > lens[i][order][-1]
    monkeypatch.setenv("HMK_TEST_GRID_CAP", str(cap))
    capfd.readouterr()
    try:
        got = ctx.align_pairs_global(i[order], j[order], go, ge)
    finally:
        monkeypatch.delenv("HMK_TEST_GRID_CAP")
    lines = GRID_LINE.findall(capfd.readouterr().err)
    kernel, wanted = f"k_traceback_global<{lmax}>", 9 if lmax == 16 else 36
    assert (kernel, str(wanted), str(cap)) in lines, lines
    assert_records(got, R.expected(name, lmax), order)


@pytest.mark.gpu
def test_lists_beyond_one_workgroup_repeats_and_the_empty_list(gpu):
    name = "asym"
    want = R.expected(name, 16)
    ctx, go, ge, seqs = family_ctx(name, 16)
    rng = np.random.default_rng(9)
    pick = rng.integers(0, 48 * 48, 300)   # more than the 256 lanes of the small instantiation's workgroup
    pick[257] = pick[299] = pick[3]        # the same pair in two workgroups and twice in one
    i, j = np.divmod(pick, 48)
    assert_records(ctx.align_pairs_global(i, j, go, ge), want, pick)
    got2d = ctx.align_pairs_global(i.reshape(3, 100), j.reshape(3, 100), go, ge)
    assert all(a.shape == (3, 100) for a in got2d)
    assert_records([a.reshape(-1) for a in got2d], want, pick)
    empty = ctx.align_pairs_global([], [], go, ge)
    assert [a.shape for a in empty] == [(0,)] * 4
    assert [a.dtype for a in empty] == [np.int32, np.uint8, np.uint64, np.uint64]
    assert raw_call(ctx, [], [], 0, go, ge, null=("score", "n_cols", "gap1", "gap2")) == N.HMK_OK
    one = ctx.align_pairs_global([5], [5], go, ge)   # a sequence against itself under an asymmetric matrix
    assert_records(one, want, np.array([5 * 48 + 5]))


@pytest.mark.gpu
def test_bad_arguments_behind_the_device_check(gpu):
    ctx, go, ge, seqs = family_ctx("blosum", 16)
    n = len(seqs)
    assert raw_call(ctx, [0, n], [1, 2], 2, go, ge) == N.HMK_ERR_BAD_ARG
    assert raw_call(ctx, [0, 1], [1, n], 2, go, ge) == N.HMK_ERR_BAD_ARG
    for field in ("score", "n_cols", "gap1", "gap2"):
        assert raw_call(ctx, [0, 1], [1, 2], 2, go, ge, null=(field,)) == N.HMK_ERR_BAD_ARG
    assert N.lib.hmk_align_pairs_global(ctx._h, None, None, 2, go, ge, None, None, None, None) == N.HMK_ERR_BAD_ARG
    for bad_go, bad_ge in BAD_PENALTIES:
        assert raw_call(ctx, [0, 1], [1, 2], 2, bad_go, bad_ge) == N.HMK_ERR_BAD_ARG
    assert raw_call(ctx, [0, 1], [1, 2], 2, go, ge) == N.HMK_OK
    fresh = hammock_amd.Context(GE.blosum62(), device=0)
    assert raw_call(fresh, [0], [0], 1, go, ge) == N.HMK_ERR_NO_SEQUENCES


@pytest.mark.gpu
def test_align_edges_of_the_neighbour_pass_and_of_a_search(gpu):
    """seq1 = an edge's m, seq2 = its x in both calls: under a symmetric matrix (each unordered pair once, x < m) and under an
    asymmetric one (a search, m = query); an edge with another score than its alignment is refused"""
    n = 48
    ctx, go, ge, _ = family_ctx("blosum")
    edges, _ = ctx.neighbors_global(go, ge, -20)
    x, m, s = hammock_amd.edge_fields(edges)
    assert edges.size > 200 and (x < m).all()
    want = R.expected("blosum")
    got = ctx.align_edges_global(edges, go, ge)
    assert_records(got, want, m.astype(np.int64) * n + x)
    assert np.array_equal(got[0], s)
    bad = edges.copy()
    bad[7] = hammock_amd.pack_edges([x[7]], [m[7]], [s[7] + 1])[0]
    with pytest.raises(ValueError, match="edge 7"):
        ctx.align_edges_global(bad, go, ge)

    ctx, go, ge, _ = family_ctx("asym")
    edges, _ = ctx.search_global(0, 24, 24, n, go, ge, -40)
    x, m, s = hammock_amd.edge_fields(edges)
    assert edges.size > 100 and (m < 24).all() and (x >= 24).all()
    want = R.expected("asym")
    assert (want[0].reshape(n, n) != want[0].reshape(n, n).T).any()   # the orientation matters
    got = ctx.align_edges_global(edges, go, ge)
    assert_records(got, want, m.astype(np.int64) * n + x)
    swapped = ctx.align_pairs_global(x, m, go, ge)   # seq1 and seq2 taken for each other: other scores
    assert (swapped[0] != s).any()


QUERIES = ("ACDEFGHIKL", "WWCDEFG", "MNPQRSTVW")
REFERENCES = ("ACDFGHIKL", "ACDEFGHWWIKL", "CDEFG", "MNPQRRSTVWY", "HEAGAWGHEE", "A")


@pytest.mark.gpu
def test_cli_search_alignments_writes_exactly_the_reference_rows(gpu, tmp_path):
    qfa, rfa = tmp_path / "q.fa", tmp_path / "r.fa"
    qfa.write_text("".join(f">1\n{s}\n" for s in QUERIES))
    rfa.write_text("".join(f">1\n{s}\n" for s in REFERENCES))
    M = [[int(v) for v in row] for row in GE.blosum62()]
    go, ge, thr = -4, -2, -30

    def lines(best):
        out = ["query\ttarget\tscore\tquery_row\ttarget_row"]
        for q in QUERIES:
            hits = []
            for t, r in enumerate(REFERENCES):
                a, b = [int(v) for v in hammock_amd.encode(q)], [int(v) for v in hammock_amd.encode(r)]
                score, n_cols, gap1, gap2 = R.walk(a, b, M, go, ge)
                if score >= thr:
                    hits.append((-score, t, "\t".join((q, r, str(score)) + R.gapped_rows(q, r, n_cols, gap1, gap2))))
            out += [h[2] for h in sorted(hits)[:best]]
        return out

    assert len(lines(99)) > 1 + 2 * len(QUERIES) and any("-" in ln for ln in lines(99))
    assert "ACDEFGHIKL\tACDFGHIKL\t48\tACDEFGHIKL\tACD-FGHIKL" in lines(99)   # (52 for the nine pairs, one gap of one)
    for extra, best, name in (([], 99, "all"), (["--best", "2"], 2, "best")):
        out = tmp_path / name
        r = cli("search", "-i", str(qfa), "--database", str(rfa), "-d", str(out), "--scorer", "global", "--gap_open", str(go),
                "--gap_extend", str(ge), "-g", str(thr), "--alignments", *extra)
        assert r.returncode == 0, r.stderr
        assert (out / "search_hits.tsv").read_text().splitlines() == lines(best)
    # without the flag the file is what it was
    out = tmp_path / "plain"
    r = cli("search", "-i", str(qfa), "--database", str(rfa), "-d", str(out), "--scorer", "global", "--gap_open", str(go),
            "--gap_extend", str(ge), "-g", str(thr))
    assert r.returncode == 0, r.stderr
    assert (out / "search_hits.tsv").read_text().splitlines() == ["\t".join(ln.split("\t")[:3]) for ln in lines(99)]


@pytest.mark.gpu
def test_cli_align_with_the_global_scorer_on_greedy_clusters(gpu, tmp_path):
    """the greedy clusters (global scorer, -5 / -1) of the first 600 records of tests/golden/musi.fa: centres, sums, widths and every
    row equal the Python star merge over the reference's walk; a row without its '-' is its sequence"""
    with open(os.path.join(GOLDEN, "musi.fa")) as fh:
        fa_lines = fh.read().splitlines()
    fa = tmp_path / "subset.fa"
    fa.write_text("\n".join(fa_lines[:1200]) + "\n")
    r = cli("greedy", "-i", str(fa), "-d", str(tmp_path / "g"), "--scorer", "global")
    assert r.returncode == 0, r.stderr
    cfile = tmp_path / "g" / "initial_clusters_sequences.tsv"
    lines = cfile.read_text().splitlines()
    head = lines[0].split("\t")
    assert head[:3] == ["cluster_id", "sequence", "alignment"]
    loaded = [(int(f[0]), f[1]) for f in (ln.split("\t") for ln in lines[1:])]
    ids = list(dict.fromkeys(c for c, _ in loaded))   # clusters in file order, members in line order: the loader's
    members = {c: [s for cc, s in loaded if cc == c] for c in ids}
    M = GE.blosum62()
    Ml = [[int(v) for v in row] for row in M]
    go, ge = -5, -1
    row_of, centers, multi, widest = {}, ["cluster_id\tsize\tcenter\tcenter_sum\twidth"], 0, 0
    for c in ids:
        seqs = members[c]
        enc = [[int(v) for v in hammock_amd.encode(s)] for s in seqs]
        T = G.global_table(enc, M, go, ge)
        low = np.tril(T, -1)   # T[larger index][smaller index]: seq1 = the larger index
        sums = low.sum(axis=1) + low.sum(axis=0)
        z = int(np.argmax(sums))   # (the first of equal sums)
        others = [k for k in range(len(seqs)) if k != z]
        records = [R.walk(enc[z], enc[k], Ml, go, ge)[1:] for k in others]
        c_row, rows = R.star_rows(seqs[z], [seqs[k] for k in others], records)
        assert (c_row, rows) == hammock_amd.star_rows(seqs[z], [seqs[k] for k in others], records)
        for k, row in zip([z] + others, [c_row] + rows):
            assert row.replace("-", "") == seqs[k] and len(row) == len(c_row)
            row_of[(c, seqs[k])] = row
        centers.append(f"{c}\t{len(seqs)}\t{seqs[z]}\t{int(sums[z])}\t{len(c_row)}")
        multi += len(seqs) > 1
        widest = max(widest, len(c_row))
    assert multi >= 5 and any("-" in row.strip("-") for row in row_of.values())   # gaps inside peptides
    out = tmp_path / "a"
    r = cli("align", "-i", str(cfile), "-d", str(out), "--scorer", "global")
    assert r.returncode == 0, r.stderr
    assert "Scorer: global (global alignment, affine gap). Gap open penalty: -5, gap extend penalty: -1" in r.stderr
    assert "Max shift" not in r.stderr
    assert f"Clusters of more than one sequence: {multi}," in r.stderr and f"widest alignment: {widest}," in r.stderr
    assert (out / "cluster_centers.tsv").read_text() == "\n".join(centers) + "\n"
    want = [lines[0]]
    for ln in lines[1:]:
        f = ln.split("\t")
        f[2] = row_of[(int(f[0]), f[1])]
        want.append("\t".join(f))
    assert (out / "initial_clusters_sequences.tsv").read_text() == "\n".join(want) + "\n"
    assert sorted(os.listdir(out / "alignments_initial")) == sorted(f"{c}.aln" for c in ids if len(members[c]) > 1)
    for c in ids:
        if len(members[c]) > 1:
            aln = "".join(f">{c}_{t + 1}\n{row_of[(c, s)]}\n" for t, s in enumerate(members[c]))
            assert (out / "alignments_initial" / f"{c}.aln").read_text() == aln
