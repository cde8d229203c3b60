"""Connected components of the neighbour graph at one threshold or a range: hmk_components_shifted (k_components.hip),
hmk_components_from_edges, hmk_components_from_edges_dev and `hammock-hip components`.

The expected answer is never the code under test: scipy.sparse.csgraph.connected_components per level, relabelled to the smallest
index of each component -- over the C oracle's scores for peptide inputs, over the given edges for the synthetic graphs.  Oracle
scores and scipy results are computed once per input and shared.
CPU part (host-only context): the symbols, _from_edges against scipy on every output for every synthetic graph and for MUSI's
oracle edges, every argument check, the device forms' DeviceError, the mode's argument and file errors.
GPU part: every synthetic graph through _from_edges_dev at the default grid and on 1 and 3 workgroups; the scoring call against
scipy and against _from_edges on its own edges; the grow path, state between calls, null outputs, the device list [0, 0], the
other calls' clusters inside the components, the mode's files.
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

from conftest import GOLDEN, ROOT, random_peptides
from test_assign import gpu   # noqa: F401  (the fixture that skips where no HIP device is visible)
from test_continue import cli

import hammock_amd
from hammock_amd import _native as N
from hammock_amd.synth import synth_peptides

FIELDS = ("n_edges", "n_components", "n_singletons", "largest")
THR = 20                     # the synthetic graphs' edges score THR + (k mod 9)
RANGES = [(20, 28), (20, 20), (23, 26)]   # all levels; a single one; edges below the threshold ignored and levels above threshold_hi clamped
GRID_LINE = re.compile(r"^\[hmk grid\] (\S+) (\d+) -> (\d+)$", re.M)


@functools.lru_cache(maxsize=None)
def matrix(name="blosum62"):
    import json
    with open(os.path.join(GOLDEN, "matrices.json")) as fh:
        return np.asarray(json.load(fh)["matrices"][name], dtype=np.int32)


# ---- the expectation -------------------------------------------------------------------------------------------------------

def scipy_levels(n, x, m, sc, thr, hi):
    """-> (component at thr: the smallest index of each vertex's component, {field: array over thr ... hi})"""
    out = {f: [] for f in FIELDS}
    first = None
    for t in range(thr, hi + 1):
        keep = sc >= t
        pairs = np.stack([np.minimum(x[keep], m[keep]), np.maximum(x[keep], m[keep])])
        if pairs.shape[1]:
            pairs = np.unique(pairs, axis=1)   # an unordered pair once
        ncomp, lab = connected_components(coo_matrix((np.ones(pairs.shape[1], dtype=np.int8), (pairs[0], pairs[1])), shape=(n, n)), directed=False)
        size = np.bincount(lab, minlength=ncomp)
        out["n_edges"].append(int(keep.sum()))   # (the calls count the edges they are given)
        out["n_components"].append(ncomp)
        out["n_singletons"].append(int((size == 1).sum()))
        out["largest"].append(int(size.max()) if n else 0)
        if first is None:
            low = np.full(ncomp, n, dtype=np.int64)
            np.minimum.at(low, lab, np.arange(n))
            first = low[lab]
    return first, {f: np.asarray(v, dtype=np.int64) for f, v in out.items()}


def same(got, want, what=""):
    comp, levels = got
    if comp is not None:
        assert comp.dtype == np.uint32 and np.array_equal(comp.astype(np.int64), want[0]), what + "component"
    if levels is not None:
        for f in FIELDS:
            assert np.array_equal(levels[f].astype(np.int64), want[1][f]), what + f
        assert not levels["reserved"].any()


def same_stats(s, want, n_levels):
    assert (s.n_edges, s.n_components, s.n_singletons, s.largest, s.n_levels) == tuple(int(want[1][f][0]) for f in FIELDS) + (n_levels,)


# ---- the synthetic graphs --------------------------------------------------------------------------------------------------

def _gnm(rng, n, m):
    got = np.zeros((2, 0), dtype=np.int64)
    while got.shape[1] < m:
        a = rng.integers(0, n, size=(2, 2 * m))
        a = a[:, a[0] != a[1]]
        got = np.unique(np.concatenate([got, np.sort(a, axis=0)], axis=1), axis=1)
    return got[:, rng.permutation(got.shape[1])[:m]]


def _tree(rng, k):
    child = np.arange(1, k)
    return np.stack([child, (rng.random(k - 1) * child).astype(np.int64)])


def _build(name):
    """-> (n, ends [2, E], shuffle, extra scores or None)"""
    rng = np.random.default_rng(4242)
    if name == "path_relabelled":
        q = rng.permutation(4099)
        return 4099, np.stack([q[:-1], q[1:]]), True, None
    if name == "path_descending":
        i = np.arange(4097, -1, -1)
        return 4099, np.stack([i, i + 1]), False, None
    if name == "star":   # the centre is the largest index: every hook contends for parent[n - 1]
        return 20000, np.stack([np.arange(19999), np.full(19999, 19999)]), True, None
    if name == "cliques":
        a, b = np.triu_indices(17, 1)
        base = np.repeat(np.arange(64) * 17, a.size)
        q = rng.permutation(64 * 17 + 500)
        return q.size, np.stack([q[base + np.tile(a, 64)], q[base + np.tile(b, 64)]]), True, None
    if name == "two_trees":   # joined by one edge of the lowest level, placed last
        q = rng.permutation(6000)
        t0, t1 = _tree(rng, 3000), _tree(rng, 3000) + 3000
        ends = np.concatenate([t0, t1], axis=1)[:, rng.permutation(5998)]
        ends = np.concatenate([ends, [[17], [4000]]], axis=1)
        k = np.arange(5999)
        return 6000, q[ends], False, np.where(k == 5998, THR, THR + 1 + k % 8)
    if name == "repeated":
        return 10, np.stack([np.full(1000, 3), np.full(1000, 7)]), True, None
    if name == "none":
        return 50, np.zeros((2, 0), dtype=np.int64), True, None
    if name.startswith("gnm_"):
        return 20000, _gnm(rng, 20000, int(name[4:])), True, None
    if name == "below_mixed":   # a third of the edges below THR: they would join everything
        ends = _gnm(rng, 5000, 9000)
        k = np.arange(9000)
        return 5000, ends, True, np.where(k % 3 == 0, THR - 1 - k % 5, THR + k % 9)
    raise KeyError(name)


GRAPHS = ["path_relabelled", "path_descending", "star", "cliques", "two_trees", "repeated", "none", "gnm_12000", "gnm_20000", "gnm_30000",
          "below_mixed"]


@functools.lru_cache(maxsize=None)
def graph(name):
    """-> (n, x, m, sc, packed edges): both orientations occur, the order is shuffled with a fixed seed"""
    n, ends, shuffle, sc = _build(name)
    e = ends.shape[1]
    k = np.arange(e)
    sc = THR + k % 9 if sc is None else sc
    flip = np.random.default_rng(7).random(e) < 0.5
    x, m = np.where(flip, ends[1], ends[0]), np.where(flip, ends[0], ends[1])
    if shuffle:
        order = np.random.default_rng(8).permutation(e)
        x, m, sc = x[order], m[order], sc[order]
    return n, x, m, sc, hammock_amd.pack_edges(x, m, sc)


@functools.lru_cache(maxsize=None)
def graph_expect(name, thr, hi):
    n, x, m, sc, _ = graph(name)
    return scipy_levels(n, x, m, sc, thr, hi)


@functools.lru_cache(maxsize=None)
def vertices(n):
    return synth_peptides(40, n, 12)   # any n distinct peptides


def graph_ctx(name, device):
    ctx = hammock_amd.Context(matrix(), device=device)
    ctx.set_sequences(residues=vertices(graph(name)[0])[0], offsets=vertices(graph(name)[0])[1])
    return ctx


# ---- peptide inputs and the oracle's scores ----------------------------------------------------------------------------------

def musi():
    with open(os.path.join(GOLDEN, "musi.fa")) as fh:
        return list(dict.fromkeys(line.strip() for line in fh if line.strip() and not line.startswith(">")))


@functools.lru_cache(maxsize=None)
def peptides(name):
    """-> (res, off, max shift, penalty, threshold, threshold_hi)"""
    if name == "musi":
        return hammock_amd.pack_sequences(musi()) + (3, 0, 20, 40)
    if name == "synth12":
        return synth_peptides(1, 3000, 12) + (3, 0, 20, 28)
    if name == "synth7to12":
        return synth_peptides(1, 3000, 7, 12) + (2, -1, 14, 22)
    if name == "keyed":   # one length, max shift 3: the plan is key-sorted (HMK_NO_KEY_SORT=1 is the other order)
        return synth_peptides(5, 5000, 12) + (3, 0, 20, 26)
    if name == "three_letters":
        from oracle import c_oracle
        return c_oracle.pack(random_peptides(np.random.default_rng(77), 2000, 12, 12, alphabet=3)) + (3, 0, 14, 18)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def oracle_scores(name):
    """-> (n, x, m, sc) over every pair x < m: ShiftedScorer.sequenceScore(seq1 = m, seq2 = x), the orientation of the pass's edges"""
    from oracle import c_oracle
    res, off, X, p, _, _ = peptides(name)
    n = len(off) - 1
    x, m = np.triu_indices(n, 1)
    st, sc = c_oracle.score_pairs(matrix(), res, off, m, x, 0, X, p)
    assert st == 0
    return n, x, m, sc


@functools.lru_cache(maxsize=None)
def oracle_expect(name, thr, hi):
    n, x, m, sc = oracle_scores(name)
    keep = sc >= thr
    return scipy_levels(n, x[keep], m[keep], sc[keep], thr, hi)


def oracle_edges(name, thr):
    _, x, m, sc = oracle_scores(name)
    keep = sc >= thr
    return hammock_amd.pack_edges(x[keep], m[keep], sc[keep])


def pep_ctx(name, device=0):
    res, off = peptides(name)[:2]
    ctx = hammock_amd.Context(matrix(), device=device)
    ctx.set_sequences(residues=res, offsets=off)
    return ctx


def raw(ctx, fn, head, thr, hi, component=True, levels=True):
    """the C call with NULL where an output is not wanted -> (status, component, levels, stats)"""
    comp = np.zeros(max(ctx.n, 1), dtype=np.uint32)
    lv = np.zeros(256, dtype=hammock_amd.api.LEVEL_DTYPE)
    stats = N.ComponentsStats()
    st = fn(ctx._h, *head, thr, hi, comp.ctypes.data_as(C.POINTER(C.c_uint32)) if component else None,
            lv.ctypes.data_as(C.POINTER(N.ComponentLevel)) if levels else None, C.byref(stats))
    return st, comp[:ctx.n], lv[:max(hi - thr + 1, 0)], stats


# ---- CPU: the symbols ------------------------------------------------------------------------------------------------------

def test_symbols_are_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "hammock_hip.h")) as fh:
        header = fh.read()
    for name in ("hmk_components_shifted", "hmk_components_from_edges", "hmk_components_from_edges_dev"):
        assert re.search(r"\bint " + name + r"\(", header)
        assert name in N.SYMBOLS and hasattr(N.lib, name)
    assert "hmk_component_level" in header and "hmk_components_stats" in header and "ClinkageClusterScorer.java:36-48" in header
    assert re.search(r"#define HMK_ABI_VERSION 4\b", header) and N.lib.hmk_abi_version() == 4
    assert C.sizeof(N.ComponentLevel) == 24 == hammock_amd.api.LEVEL_DTYPE.itemsize and C.sizeof(N.ComponentsStats) == 48


# ---- CPU: _from_edges against scipy ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", GRAPHS)
def test_from_edges_equals_scipy_on_the_synthetic_graphs(name):
    n, _, _, _, edges = graph(name)
    ctx = graph_ctx(name, -1)
    for thr, hi in RANGES:
        want = graph_expect(name, thr, hi)
        same(ctx.components_from_edges(edges, thr, hi), want, f"{thr}..{hi} ")
        s = ctx.last_components_stats
        same_stats(s, want, hi - thr + 1)
        assert (s.pairs_scored, s.kernel_ms, s.components_ms) == (0, 0.0, 0.0)
    same(ctx.components_from_edges(edges, 20), graph_expect(name, 20, 20), "threshold_hi=None ")
    same(ctx.components_from_edges(edges[::-1].copy(), 20, 28), graph_expect(name, 20, 28), "reversed ")
    st, comp, _, _ = raw(ctx, N.lib.hmk_components_from_edges, (edges.ctypes.data_as(C.POINTER(C.c_uint64)), edges.size), 20, 28, levels=False)
    assert st == 0 and np.array_equal(comp, graph_expect(name, 20, 28)[0])
    st, _, lv, _ = raw(ctx, N.lib.hmk_components_from_edges, (edges.ctypes.data_as(C.POINTER(C.c_uint64)), edges.size), 20, 28, component=False)
    assert st == 0
    same((None, lv), graph_expect(name, 20, 28))


def test_the_random_graphs_lie_on_both_sides_of_the_giant_component():
    # all edges (level 20): m / n = 0.6, 1.0, 1.5, a giant component of a growing share; the top level keeps a ninth of them, m / n
    # far below 1 / 2, and nothing large is left
    share = [graph_expect(f"gnm_{m}", 20, 28)[1]["largest"][0] / 20000 for m in (12000, 20000, 30000)]
    assert share[0] + 0.1 < share[1] < share[2] - 0.1
    assert all(graph_expect(f"gnm_{m}", 20, 28)[1]["largest"][8] < 200 for m in (12000, 20000, 30000))
    assert graph_expect("star", 20, 28)[1]["largest"][0] == 20000 and graph_expect("cliques", 20, 20)[1]["n_singletons"][0] == 500
    two = graph_expect("two_trees", 20, 28)[1]["n_components"]
    assert two[0] == 1 and two[1] == 2   # the joining edge is the only one of the lowest level
    assert graph_expect("below_mixed", 20, 20)[1]["n_edges"][0] == 6000


def test_from_edges_on_musi_equals_scipy_and_the_scan_shows_the_structure():
    n, _, _, _ = oracle_scores("musi")
    want = oracle_expect("musi", 20, 40)
    # the reference alone: the graph falls apart over this range, into many families and not only into singletons
    assert len(set(want[1]["n_components"].tolist())) >= 4
    assert [int(want[1][f][0]) for f in FIELDS] == [303555, 6, 5, 2452]
    assert [int(want[1]["n_components"][t - 20]) for t in (26, 32, 38)] == [27, 128, 742]
    assert (want[1]["n_components"] - want[1]["n_singletons"]).max() >= 100
    ctx = pep_ctx("musi", -1)
    same(ctx.components_from_edges(oracle_edges("musi", 20), 20, 40), want)
    same(ctx.components_from_edges(oracle_edges("musi", 20), 26), oracle_expect("musi", 26, 26), "26 ")


# ---- CPU: the argument checks ------------------------------------------------------------------------------------------------

def test_bad_arguments_are_refused_before_the_device_is_looked_at():
    n, _, _, _, edges = graph("cliques")
    ctx = graph_ctx("cliques", -1)
    ep = (edges.ctypes.data_as(C.POINTER(C.c_uint64)), edges.size)
    heads = [(N.lib.hmk_components_shifted, (3, 0)), (N.lib.hmk_components_from_edges, ep), (N.lib.hmk_components_from_edges_dev, (None, 0))]
    for fn, head in heads:   # the same three checks in all three, on a host-only context
        assert raw(ctx, fn, head, 21, 20)[0] == N.HMK_ERR_BAD_ARG
        assert raw(ctx, fn, head, 20, 276)[0] == N.HMK_ERR_BAD_ARG
        assert raw(ctx, fn, head, -2 ** 31, 2 ** 31 - 1)[0] == N.HMK_ERR_BAD_ARG
        assert raw(ctx, fn, head, 20, 22, component=False, levels=False)[0] == N.HMK_ERR_BAD_ARG
        assert fn(None, *head, 20, 20, None, None, None) == N.HMK_ERR_BAD_ARG
    assert raw(ctx, N.lib.hmk_components_from_edges, ep, 20, 275)[0] == 0   # 256 levels are allowed
    with pytest.raises(ValueError, match="threshold_hi"):
        ctx.components_from_edges(edges, 20, 19)
    for x, m in ((3, n), (n, 3), (2 ** 24 - 1, 0), (5, 5)):   # an index >= n either side, a self pair
        bad = edges.copy()
        bad[100] = hammock_amd.pack_edges(np.array([x]), np.array([m]), np.array([25]))[0]
        with pytest.raises(ValueError, match="outside"):
            ctx.components_from_edges(bad, 20, 28)
        bad[100] = hammock_amd.pack_edges(np.array([x]), np.array([m]), np.array([3]))[0]   # ... whatever its score
        with pytest.raises(ValueError, match="outside"):
            ctx.components_from_edges(bad, 20, 28)
    assert raw(ctx, N.lib.hmk_components_from_edges, (None, 5), 20, 20)[0] == N.HMK_ERR_BAD_ARG
    same(ctx.components_from_edges(edges, 20, 28), graph_expect("cliques", 20, 28), "after the refusals ")
    # any int is a threshold here: score - threshold must not wrap for edges far from it, at either end
    far = hammock_amd.pack_edges(np.array([0, 2, 4, 6]), np.array([1, 3, 5, 7]), np.array([-32768, -2, 5, 32767]))
    top = 2 ** 31 - 1
    for thr, hi, joined in ((top, top, 0), (top - 255, top, 0), (-2 ** 31, -2 ** 31, 4), (-2 ** 31, -2 ** 31 + 255, 4), (32767, 32767 + 255, 1)):
        comp, levels = ctx.components_from_edges(far, thr, hi)
        assert levels["n_edges"][0] == joined and levels["n_components"][0] == n - joined and (comp != np.arange(n)).sum() == joined
        assert (levels["n_edges"][1:] == (0 if thr > 0 else 4)).all()
    asym = matrix().copy()
    asym[3, 5] += 1
    actx = hammock_amd.Context(asym, device=-1)
    actx.set_sequences(residues=vertices(n)[0], offsets=vertices(n)[1])
    with pytest.raises(ValueError, match="symmetric"):
        actx.components_shifted(3, 0, 20)


def test_the_device_forms_need_a_device_and_an_empty_set_is_ok():
    ctx = graph_ctx("cliques", -1)
    with pytest.raises(hammock_amd.DeviceError):
        ctx.components_shifted(3, 0, 20, 24)
    with pytest.raises(hammock_amd.DeviceError):
        ctx.components_from_edges_dev(0, 0, 20, 24)
    empty = hammock_amd.Context(matrix(), device=-1)
    comp, levels = empty.components_from_edges(np.zeros(0, dtype=np.uint64), 20, 24)
    assert comp.size == 0 and levels.size == 5 and not any(levels[f].any() for f in FIELDS)
    assert raw(empty, N.lib.hmk_components_from_edges, (None, 0), 20, 24, component=False, levels=False)[0] == 0


def test_cli_components_argument_and_file_errors(tmp_path):
    fa = os.path.join(GOLDEN, "musi.fa")
    r = cli("components", "-d", str(tmp_path / "a"))
    assert r.returncode == 2 and "-i or --input" in r.stderr
    assert not (tmp_path / "a").exists()
    r = cli("components", "-i", fa, "--devices", "0,1", "-d", str(tmp_path / "a"))
    assert r.returncode == 2 and "--devices" in r.stderr
    r = cli("components", "-i", fa, "-f", "seq", "-d", str(tmp_path / "a"))
    assert r.returncode == 2 and "-f" in r.stderr
    assert not (tmp_path / "a").exists()
    r = cli("components", "-i", fa, "-g", "26", "--scan_to", "25", "-d", str(tmp_path / "b"))
    assert r.returncode == 2 and "--scan_to" in r.stderr
    r = cli("components", "-i", fa, "--scan_to", "276", "-d", str(tmp_path / "c"))   # the derived threshold is 20
    assert r.returncode == 2 and "--scan_to" in r.stderr and "20 up to 275" in r.stderr
    r = cli("components", "-i", fa, "-d", str(tmp_path / "c"))   # the directory exists now
    assert r.returncode == 2 and "Output directory exists" in r.stderr
    r = cli("components", "-i", str(tmp_path / "missing.fa"), "-d", str(tmp_path / "d"))
    assert r.returncode != 0
    r = cli("components", "-i", fa, "-l", "no_such_label", "-d", str(tmp_path / "e"))
    assert r.returncode == 3 and "No sequences" in r.stderr
    assert "hammock-hip components -i" in cli("--help").stderr


# ---- GPU: the synthetic graphs through the device kernels --------------------------------------------------------------------

def device_edges(edges):
    import torch
    return torch.from_numpy(edges.view(np.int64).copy()).to("cuda:0")


def wanted_grids(n, e, single):
    """kernel -> the grid its launcher asks for (k_components.hip's launchers) on n vertices and e given edges"""
    by_vertex, by_chunk = min(-(-n // 256), 2048), min(-(-e // 1024), 4096)
    grids = {"k_cc_init": by_vertex, "k_cc_flatten": by_vertex, "k_cc_sizes": by_vertex}
    if single:
        grids["k_cc_union_edges"] = by_chunk
    else:
        grids.update({"k_cc_hist": by_chunk, "k_cc_partition": by_chunk, "k_cc_union": min(-(-e // 256), 2048)})
    return grids


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [0, 1, 3])
@pytest.mark.parametrize("name", GRAPHS)
def test_from_edges_dev_equals_scipy_on_the_synthetic_graphs(gpu, monkeypatch, capfd, name, cap):
    n, _, _, _, edges = graph(name)
    ctx = graph_ctx(name, 0)
    d = device_edges(edges)
    if cap:
        monkeypatch.setenv("HMK_TEST_GRID_CAP", str(cap))
    for thr, hi in RANGES + [(20, None)]:
        capfd.readouterr()
        if hi is None:   # a single level and no `levels`: the union straight from the edges
            st, comp, _, s = raw(ctx, N.lib.hmk_components_from_edges_dev, (d.data_ptr(), d.numel()), thr, thr, levels=False)
            assert st == 0
            want = graph_expect(name, thr, thr)
            same((comp, None), want, "single ")
            same_stats(s, want, 1)
        else:
            want = graph_expect(name, thr, hi)
            same(ctx.components_from_edges_dev(d.data_ptr(), d.numel(), thr, hi), want, f"{thr}..{hi} ")
            s = ctx.last_components_stats
            same_stats(s, want, hi - thr + 1)
            assert s.pairs_scored == 0 and s.kernel_ms == 0.0 and (s.components_ms > 0.0)
        lines = {}
        for kernel, wanted, launched in GRID_LINE.findall(capfd.readouterr().err):
            lines.setdefault(kernel, set()).add((int(wanted), int(launched)))
        cut = {k: {(w, cap)} for k, w in wanted_grids(n, edges.size, hi is None).items() if cap and w > cap}
        assert {k: v for k, v in lines.items() if k.startswith("k_cc_")} == cut
        if name == "star" and cap:   # here every grid-stride kernel runs its loop well beyond the first iteration
            assert set(cut) == set(wanted_grids(n, edges.size, hi is None)) and all(w >= 2 * cap for (w, _), in cut.values())


@pytest.mark.gpu
def test_from_edges_dev_refuses_invalid_edges_and_goes_on(gpu):
    n, _, _, _, edges = graph("gnm_12000")
    ctx = graph_ctx("gnm_12000", 0)
    for x, m in ((3, n), (n + 5, 3), (2 ** 24 - 1, 2 ** 24 - 2), (5, 5)):
        bad = edges.copy()
        bad[7000] = hammock_amd.pack_edges(np.array([x]), np.array([m]), np.array([25]))[0]
        d = device_edges(bad)
        with pytest.raises(ValueError, match="outside"):
            ctx.components_from_edges_dev(d.data_ptr(), d.numel(), 20, 28)
        st = raw(ctx, N.lib.hmk_components_from_edges_dev, (d.data_ptr(), d.numel()), 20, 20, levels=False)[0]
        assert st == N.HMK_ERR_BAD_ARG
        d = device_edges(edges)
        same(ctx.components_from_edges_dev(d.data_ptr(), d.numel(), 20, 28), graph_expect("gnm_12000", 20, 28), "the next call ")
    assert raw(ctx, N.lib.hmk_components_from_edges_dev, (None, 5), 20, 20)[0] == N.HMK_ERR_BAD_ARG


# ---- GPU: the scoring call -----------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", ["musi", "synth12", "synth7to12", "keyed", "three_letters"])
def test_components_shifted_equals_scipy_on_oracle_scores_and_from_edges(gpu, monkeypatch, capfd, name):
    res, off, X, p, thr, hi = peptides(name)
    n = len(off) - 1
    ctx = pep_ctx(name)
    want = oracle_expect(name, thr, hi)
    if name == "keyed":   # the planner's timeline names the step only a key-sorted plan has
        monkeypatch.setenv("HMK_GREEDY_TIMING", "1")
        capfd.readouterr()
    got = ctx.components_shifted(X, p, thr, hi)
    if name == "keyed":
        assert "[hmk plan] row-shared groups" in capfd.readouterr().err, "the plan of this case is not key-sorted"
        monkeypatch.delenv("HMK_GREEDY_TIMING")
    same(got, want)
    s = ctx.last_components_stats
    same_stats(s, want, hi - thr + 1)
    assert s.pairs_scored == n * (n - 1) // 2 and s.kernel_ms > 0 and s.components_ms > 0
    edges, _ = ctx.neighbors_shifted(X, p, thr)
    same(ctx.components_from_edges(edges, thr, hi), want, "from its own edges ")
    mid = 26 if name == "musi" else (thr + hi) // 2   # a single level
    same(ctx.components_shifted(X, p, mid), oracle_expect(name, mid, mid), "single level ")
    st, comp, _, s1 = raw(ctx, N.lib.hmk_components_shifted, (X, p), mid, mid, levels=False)
    assert st == 0 and np.array_equal(comp, oracle_expect(name, mid, mid)[0])
    same_stats(s1, oracle_expect(name, mid, mid), 1)
    if name == "musi":
        assert [int(want[1]["n_components"][t - 20]) for t in (20, 26, 32, 38)] == [6, 27, 128, 742]
    if name == "synth12":
        assert [int(want[1]["n_components"][t - 20]) for t in (20, 24, 28)] == [110, 1017, 2356]
    if name == "synth7to12":
        assert [int(want[1]["n_components"][t - 14]) for t in (14, 18, 22)] == [25, 529, 1896]
    if name == "three_letters":
        assert want[1]["n_components"][0] == 1
    if name == "keyed":   # the other order of the pass: identical output
        monkeypatch.setenv("HMK_NO_KEY_SORT", "1")
        monkeypatch.setenv("HMK_GREEDY_TIMING", "1")
        other = pep_ctx(name)
        capfd.readouterr()
        plain = other.components_shifted(X, p, thr, hi)
        err = capfd.readouterr().err
        assert "[hmk plan] device copies" in err and "row-shared groups" not in err
        monkeypatch.delenv("HMK_NO_KEY_SORT")
        monkeypatch.delenv("HMK_GREEDY_TIMING")
        assert np.array_equal(plain[0], got[0]) and plain[1].tobytes() == got[1].tobytes()


@pytest.mark.gpu
def test_the_grow_path_gives_the_same(gpu, monkeypatch, capfd):
    """a first edge buffer of 2^20 entries (16,384 per segment) under 1.7 million edges: the pass is scored twice, which the
    call's timeline says"""
    res, off, X, p, thr, hi = peptides("three_letters")
    assert oracle_expect("three_letters", thr, hi)[1]["n_edges"][0] > 2 ** 20
    monkeypatch.setenv("HMK_EDGE_GUESS", "4096")
    monkeypatch.setenv("HMK_GREEDY_TIMING", "1")
    ctx = pep_ctx("three_letters")   # a fresh context: no buffer grown by an earlier call
    capfd.readouterr()
    got = ctx.components_shifted(X, p, thr, hi)
    err = capfd.readouterr().err
    monkeypatch.delenv("HMK_EDGE_GUESS")
    monkeypatch.delenv("HMK_GREEDY_TIMING")
    assert len(re.findall(r"^\[hmk\] an edge segment overflowed \(\d+ entries for 16384\): \d+ entries next, scoring again$", err, re.M)) == 1
    same(got, oracle_expect("three_letters", thr, hi))


@pytest.mark.gpu
def test_state_between_calls_null_outputs_and_a_threshold_above_every_score(gpu):
    res, off, X, p, thr, hi = peptides("musi")
    n = len(off) - 1
    ctx = pep_ctx("musi")
    first = ctx.components_shifted(X, p, 20, 40)
    same(first, oracle_expect("musi", 20, 40))
    same(ctx.components_shifted(X, p, 30, 34), oracle_expect("musi", 30, 34), "another range ")
    ctx.neighbors_shifted(X, p, 33)
    again = ctx.components_shifted(X, p, 20, 40)
    assert np.array_equal(again[0], first[0]) and again[1].tobytes() == first[1].tobytes()
    comp, levels = ctx.components_shifted(X, p, 26, 34, levels=False)
    assert levels is None
    same((comp, None), oracle_expect("musi", 26, 34))
    comp, levels = ctx.components_shifted(X, p, 26, 34, component=False)
    assert comp is None
    same((None, levels), oracle_expect("musi", 26, 34))
    top = int(oracle_scores("musi")[3].max())
    comp, levels = ctx.components_shifted(X, p, top, top + 2)
    assert levels["n_edges"][0] > 0 and levels["n_edges"][1] == 0
    assert (levels["n_components"][1:] == n).all() and (levels["n_singletons"][1:] == n).all() and (levels["largest"][1:] == 1).all()
    comp, levels = ctx.components_shifted(X, p, top + 1)
    assert np.array_equal(comp, np.arange(n)) and levels[0].tolist() == (0, n, n, 1, 0)


@pytest.mark.gpu
def test_the_device_list_runs_on_the_root(gpu):
    res, off, X, p, thr, hi = peptides("synth12")
    ctx = hammock_amd.Context(matrix(), device=[0, 0])
    ctx.set_sequences(residues=res, offsets=off)
    same(ctx.components_shifted(X, p, thr, hi), oracle_expect("synth12", thr, hi))


@pytest.mark.gpu
@pytest.mark.parametrize("t", [26, 32])
def test_no_cluster_of_the_other_calls_crosses_a_component(gpu, t):
    res, off, X, p, _, _ = peptides("musi")
    n = len(off) - 1
    ctx = pep_ctx("musi")
    comp, levels = ctx.components_shifted(X, p, t, t + 1)
    same((comp, None), oracle_expect("musi", t, t))

    def inside(cid, comp):
        lo = np.full(int(cid.max()) + 1, 2 ** 32, dtype=np.int64)
        hi_ = np.full(int(cid.max()) + 1, -1, dtype=np.int64)
        np.minimum.at(lo, cid, comp.astype(np.int64))
        np.maximum.at(hi_, cid, comp.astype(np.int64))
        return bool((lo[np.unique(cid)] == hi_[np.unique(cid)]).all())

    cid = ctx.greedy_cluster(X, p, t, 61)[0]   # Hammock's default cluster limit, round(0.025 n) (without a limit the reference crashes here)
    assert np.bincount(cid).max() > 1 and inside(cid, comp)
    ccid = ctx.clinkage_cluster(X, p, t)[0]
    assert np.bincount(ccid).max() > 1 and inside(ccid, comp)
    # with the components as slots no two slots are feasible for each other: a pair between two components is below t
    _, slots = np.unique(comp, return_inverse=True)
    pairs = ctx.cluster_pairs_shifted(0, n, slots.astype(np.uint32), int(slots.max()) + 1, X, p, t)
    assert len(pairs) == 0
    for k in (0, 1):
        assert int(levels["n_edges"][k]) == ctx.neighbors_shifted(X, p, t + k)[0].size


# ---- GPU: the mode ---------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_cli_components_on_musi(gpu, tmp_path):
    from oracle import c_oracle, hammock_oracle as po
    fa = os.path.join(GOLDEN, "musi.fa")
    seqs = po.load_unique_sequences_from_fasta(fa)
    labels = po.get_sorted_labels(seqs)
    n = len(seqs)
    res, off = c_oracle.pack([s.get_sequence_string() for s in seqs])
    x, m = np.triu_indices(n, 1)
    st, sc = c_oracle.score_pairs(matrix(), res, off, m, x, 0, 3, 0)
    assert st == 0
    keep = sc >= 26
    comp, lv = scipy_levels(n, x[keep], m[keep], sc[keep], 26, 34)
    members = {}
    for i, c in enumerate(comp.tolist()):
        members.setdefault(c, []).append(seqs[i])
    ids = sorted(members, key=lambda c: (len(members[c]) == 1, c))   # multi-member components first, each group by ascending id
    clusters = [po.Cluster(list(members[c]), c + 1) for c in ids]
    exp = tmp_path / "exp"
    exp.mkdir()
    po.save_cluster_sequences_csv(clusters, str(exp / "initial_clusters_sequences.tsv"), labels)
    po.write_cluster_sequences_csv(seqs, clusters, str(exp / "initial_clusters_sequences_original_order.tsv"), labels)
    po.save_clusters_csv(clusters, str(exp / "initial_clusters.tsv"), labels)
    rows = ["threshold\tedges\tcomponents\tsingletons\tlargest"]
    rows += ["\t".join(str(v) for v in [26 + k] + [int(lv[f][k]) for f in FIELDS]) for k in range(9)]
    out = tmp_path / "out"
    r = cli("components", "-i", fa, "-d", str(out), "-g", "26", "--scan_to", "34", timeout=600)
    assert r.returncode == 0, r.stderr
    assert "Max shift not set. Setting automatically to: 3" in r.stderr
    assert (out / "component_levels.tsv").read_text() == "\n".join(rows) + "\n"
    for name in ("initial_clusters_sequences.tsv", "initial_clusters_sequences_original_order.tsv", "initial_clusters.tsv"):
        assert (out / name).read_bytes() == (exp / name).read_bytes(), name
    log = (out / "run.log").read_text()
    assert 'Program started in mode "components"' in log and f"Resulting clusers: {len(clusters)}" in log and "Program successfully ended." in log
    assert f"Components at threshold 26: {int(lv['n_components'][0])}, of one sequence: {int(lv['n_singletons'][0])}, largest: {int(lv['largest'][0])}" in log
    r = cli("check", "-i", str(out / "initial_clusters_sequences.tsv"), "-d", str(tmp_path / "c"), "-x", "3", "-g", "26", timeout=600)
    assert r.returncode == 0, r.stderr
    assert f" of {len(clusters)} clusters hold a pair below the threshold 26;" in (tmp_path / "c" / "run.log").read_text()
