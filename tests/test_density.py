"""Density clustering of the neighbour graph at one threshold or a range: hmk_density_shifted (k_density.hip),
hmk_density_from_edges, hmk_density_from_edges_dev and `hammock-hip density`.

The expected answer is never the code under test.  It is the definition in numpy and scipy, per level: bincount for the degrees,
scipy.sparse.csgraph.connected_components over the core-core edges, relabelled to the smallest core index, np.maximum.at over the
packed key (score + 32768) << 32 | (0xFFFFFFFF - core index) for the anchors -- over the C oracle's scores for peptide inputs, over
the given edges for the synthetic graphs.  Every comparison is exact equality on every output array and every level field.  Oracle
scores and expectations are computed once per input and shared (those of tests/test_components.py where the input is the same).
CPU part (host-only context): the symbols, _from_edges against the definition on every graph, range and min_neighbors, MUSI's
oracle edges with the issue's table, min_neighbors = 0 against components_from_edges, every refusal, the device forms'
DeviceError, the mode's argument and file errors.
GPU part: every graph through _from_edges_dev at the default grid and on 1 and 3 workgroups with the [hmk grid] lines; invalid
edges; the scoring call against the definition and against _from_edges on its own edges; the grow path, state between calls,
each output NULL in turn, a threshold above every score, the device list [0, 0], min_neighbors = 0 against components_shifted,
the mode's files.
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

from conftest import GOLDEN, ROOT
from test_assign import gpu   # noqa: F401  (the fixture that skips where no HIP device is visible)
from test_continue import cli
import test_components as tc
from test_components import GRID_LINE, RANGES, THR, device_edges, matrix, oracle_edges, oracle_scores, pep_ctx, peptides, vertices

import hammock_amd
from hammock_amd import _native as N

FIELDS = ("n_edges", "n_core", "n_border", "n_noise", "n_clusters", "largest")
NOISE = 0xFFFFFFFF


# ---- the expectation -------------------------------------------------------------------------------------------------------

def definition(n, x, m, sc, thr, hi, mn):
    """-> (cluster, degree, anchor: int64 [n_levels, n]; {field: array over thr ... hi})"""
    nl = hi - thr + 1
    cluster, anchor = np.full((nl, n), NOISE, dtype=np.int64), np.full((nl, n), NOISE, dtype=np.int64)
    degree = np.zeros((nl, n), dtype=np.int64)
    out = {f: [] for f in FIELDS}
    idx = np.arange(n)
    for l, t in enumerate(range(thr, hi + 1)):
        keep = sc >= t
        xs, ms, ss = x[keep], m[keep], sc[keep]
        deg = np.bincount(xs, minlength=n) + np.bincount(ms, minlength=n)   # (a pair given k times counts k times)
        core = deg >= mn
        cc = core[xs] & core[ms]
        ncomp, lab = connected_components(coo_matrix((np.ones(int(cc.sum()), dtype=np.int32), (xs[cc], ms[cc])), shape=(n, n)), directed=False)
        low = np.full(ncomp, n, dtype=np.int64)
        np.minimum.at(low, lab[core], idx[core])   # the smallest core index of each component
        cluster[l, core] = low[lab[core]]
        anchor[l, core] = idx[core]
        key = np.zeros(n, dtype=np.uint64)
        for a, b in ((xs, ms), (ms, xs)):   # a core, b not
            sel = core[a] & ~core[b]
            np.maximum.at(key, b[sel], ((ss[sel] + 32768).astype(np.uint64) << np.uint64(32)) | (NOISE - a[sel]).astype(np.uint64))
        border = ~core & (key != 0)
        anchor[l, border] = NOISE - (key[border] & np.uint64(NOISE)).astype(np.int64)
        cluster[l, border] = cluster[l, anchor[l, border]]
        degree[l] = deg
        member = cluster[l][cluster[l] != NOISE]
        out["n_edges"].append(int(keep.sum()))
        out["n_core"].append(int(core.sum()))
        out["n_border"].append(int(border.sum()))
        out["n_noise"].append(int(n - core.sum() - border.sum()))
        out["n_clusters"].append(int((cluster[l, core] == idx[core]).sum()))
        out["largest"].append(int(np.bincount(member).max()) if member.size else 0)
    return cluster, degree, anchor, {f: np.asarray(v, dtype=np.int64) for f, v in out.items()}


def same(got, want, what=""):
    levels, cluster, degree, anchor = got
    for name, g, w in (("cluster", cluster, want[0]), ("degree", degree, want[1]), ("anchor", anchor, want[2])):
        if g is not None:
            assert g.dtype == np.uint32 and g.shape == w.shape and np.array_equal(g.astype(np.int64), w), what + name
    if levels is not None:
        for f in FIELDS:
            assert np.array_equal(levels[f].astype(np.int64), want[3][f]), what + f
        assert not levels["reserved"].any()


def same_stats(s, want, n_levels, mn):
    assert (s.n_edges, s.n_core, s.n_border, s.n_noise, s.n_clusters, s.largest) == tuple(int(want[3][f][0]) for f in FIELDS), "stats"
    assert (s.n_levels, s.min_neighbors, s.reserved) == (n_levels, mn, 0)


# ---- the synthetic graphs --------------------------------------------------------------------------------------------------

def _clique(members):
    a, b = np.triu_indices(len(members), 1)
    return np.stack([np.asarray(members)[a], np.asarray(members)[b]])


def _build(name):
    """-> (n, ends [2, E], scores or None (THR + k mod 9), shuffle and flip)"""
    if name.startswith("late_core"):
        # two 4-cliques A and B at THR + 8, v joined to one member of each at THR + 8, v - w at THR: above THR v is border (and takes
        # A's member, the smaller index, at an equal score); at THR v turns core, A and B merge through v's OLD edges, w is v's border
        if name == "late_core_last":
            A, B, w, v = [0, 1, 2, 3], [4, 5, 6, 7], 8, 9
        else:
            v, A, B, w = 0, [1, 2, 3, 4], [5, 6, 7, 8], 9
        ends = np.concatenate([_clique(A), _clique(B), [[v, v, v], [A[1], B[2], w]]], axis=1)
        return 10, ends, np.asarray([THR + 8] * 14 + [THR]), True
    if name == "tie_border":
        # u = 8: core neighbours 5 (cluster B) and 2 (cluster A) at an equal best score, the larger index first in the list -> 2.
        # z = 9: 1 (A) at THR + 3, 6 (B) at THR + 6 -> 6: the score beats the index.  Listed as written: no shuffle, orientations mixed
        ends = np.concatenate([[[8, 2, 1, 6], [5, 8, 9, 9]], _clique([0, 1, 2, 3]), _clique([4, 5, 6, 7])[::-1]], axis=1)
        return 10, ends, np.asarray([THR + 5, THR + 5, THR + 3, THR + 6] + [THR + 8] * 12), False
    if name == "bridge":   # two 17-cliques joined by a path of five vertices of degree 2
        path = [16, 34, 35, 36, 37, 38, 17]
        ends = np.concatenate([_clique(range(17)), _clique(range(17, 34)), [path[:-1], path[1:]]], axis=1)
        return 39, ends, None, True
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def graph(name):
    """-> (n, x, m, sc, packed edges); the graphs tests/test_components.py has come from there"""
    try:
        n, ends, sc, mix = _build(name)
    except KeyError:
        return tc.graph(name)
    e = ends.shape[1]
    sc = THR + np.arange(e) % 9 if sc is None else sc
    x, m = ends[0].astype(np.int64), ends[1].astype(np.int64)
    if mix:
        flip = np.random.default_rng(7).random(e) < 0.5
        order = np.random.default_rng(8).permutation(e)
        x, m, sc = np.where(flip, m, x)[order], np.where(flip, x, m)[order], sc[order]
    return n, x, m, sc, hammock_amd.pack_edges(x, m, sc)


# graph -> the min_neighbors it runs with
CASES = {"late_core_last": (3,), "late_core_first": (3,), "tie_border": (3,), "bridge": (3,), "star": (3, 1), "cliques": (0, 1, 3),
         "gnm_30000": (2, 3, 4), "repeated": (3,), "none": (3,), "below_mixed": (3,), "path_descending": (2,)}
GRAPH_CASES = [(name, mn) for name, mns in CASES.items() for mn in mns]


@functools.lru_cache(maxsize=None)
def graph_expect(name, thr, hi, mn):
    n, x, m, sc, _ = graph(name)
    return definition(n, x, m, sc, thr, hi, mn)


def graph_ctx(name, device):
    ctx = hammock_amd.Context(matrix(), device=device)
    ctx.set_sequences(residues=vertices(graph(name)[0])[0], offsets=vertices(graph(name)[0])[1])
    return ctx


@functools.lru_cache(maxsize=None)
def oracle_expect(name, thr, hi, mn):
    n, x, m, sc = oracle_scores(name)
    keep = sc >= thr
    return definition(n, x[keep], m[keep], sc[keep], thr, hi, mn)


def raw(ctx, fn, head, thr, hi, mn, cluster=True, anchor=True, degree=True, levels=True):
    """the C call with NULL where an output is not wanted -> (status, (levels, cluster, degree, anchor), stats)"""
    nl = max(min(hi - thr + 1, 256), 1)
    arr = [np.zeros((nl, max(ctx.n, 1)), dtype=np.uint32) for _ in range(3)]
    lv = np.zeros(256, dtype=hammock_amd.api.DENSITY_LEVEL_DTYPE)
    stats = N.DensityStats()
    ptr = [a.ctypes.data_as(C.POINTER(C.c_uint32)) if w else None for a, w in zip(arr, (cluster, anchor, degree))]
    st = fn(ctx._h, *head, thr, hi, mn, *ptr, lv.ctypes.data_as(C.POINTER(N.DensityLevel)) if levels else None, C.byref(stats))
    return st, (lv[:nl] if levels else None, arr[0] if cluster else None, arr[2] if degree else None, arr[1] if anchor else None), stats


def ep(edges):
    return edges.ctypes.data_as(C.POINTER(C.c_uint64)), edges.size


# ---- CPU: the symbols ------------------------------------------------------------------------------------------------------

def test_symbols_are_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "hammock_hip.h")) as fh:
        header = fh.read()
    for name in ("hmk_density_shifted", "hmk_density_from_edges", "hmk_density_from_edges_dev"):
        assert re.search(r"\bint " + name + r"\(", header)
        assert name in N.SYMBOLS and hasattr(N.lib, name)
    assert "hmk_density_level" in header and "hmk_density_stats" in header and re.search(r"#define HMK_DENSITY_NOISE 0xFFFFFFFFu", header)
    assert C.sizeof(N.DensityLevel) == 32 == hammock_amd.api.DENSITY_LEVEL_DTYPE.itemsize and C.sizeof(N.DensityStats) == 64
    assert hammock_amd.api.DENSITY_NOISE == NOISE
    for method in ("density_shifted", "density_from_edges", "density_from_edges_dev"):
        assert callable(getattr(hammock_amd.Context, method))


# ---- CPU: _from_edges against the definition ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name,mn", GRAPH_CASES)
def test_from_edges_equals_the_definition_on_the_synthetic_graphs(name, mn):
    n, _, _, _, edges = graph(name)
    ctx = graph_ctx(name, -1)
    for thr, hi in RANGES:
        want = graph_expect(name, thr, hi, mn)
        same(ctx.density_from_edges(edges, thr, hi, mn), want, f"{thr}..{hi} ")
        s = ctx.last_density_stats
        same_stats(s, want, hi - thr + 1, mn)
        assert (s.pairs_scored, s.kernel_ms, s.density_ms) == (0, 0.0, 0.0)
    same(ctx.density_from_edges(edges, 20, min_neighbors=mn), graph_expect(name, 20, 20, mn), "threshold_hi=None ")
    same(ctx.density_from_edges(edges[::-1].copy(), 20, 28, mn), graph_expect(name, 20, 28, mn), "reversed ")
    for off in range(4):   # each output NULL in turn
        flags = [k != off for k in range(4)]
        st, got, _ = raw(ctx, N.lib.hmk_density_from_edges, ep(edges), 20, 28, mn, *flags)
        assert st == 0 and [g is None for g in (got[1], got[3], got[2], got[0])] == [not f for f in flags]
        same(got, graph_expect(name, 20, 28, mn), f"null output {off} ")


def test_the_synthetic_graphs_are_what_they_are_meant_to_be():
    """on the reference side alone"""
    for name, v, w, a, b in (("late_core_last", 9, 8, 1, 6), ("late_core_first", 0, 9, 2, 7)):
        cl, deg, an, lv = graph_expect(name, 20, 28, 3)
        assert deg[1, v] == 2 and deg[0, v] == 3 and an[1, v] == a
        assert lv["n_clusters"].tolist() == [1] + [2] * 8 and lv["n_core"].tolist() == [9] + [8] * 8
        assert an[0, v] == v and an[0, w] == v and cl[0, w] == cl[0, v] == cl[0].min() and lv["n_border"][0] == 1 and lv["n_noise"][0] == 0
        assert an[8, v] == a < b and cl[8, v] == cl[8, a] != cl[8, b] and an[8, w] == NOISE and lv["n_noise"][8] == 1
    cl, deg, an, lv = graph_expect("tie_border", 20, 28, 3)
    assert (an[0, 8], an[0, 9]) == (2, 6) and (cl[0, 8], cl[0, 9]) == (0, 4) and lv["n_border"][0] == 2 and lv["n_clusters"][0] == 2
    cl, deg, an, lv = graph_expect("bridge", 20, 20, 3)
    assert [int(lv[f][0]) for f in FIELDS] == [2 * 136 + 6, 34, 2, 3, 2, 18]
    assert an[0, 34] == 16 and an[0, 38] == 17 and (cl[0, 35:38] == NOISE).all()
    lv = graph_expect("star", 20, 20, 3)[3]
    assert [int(lv[f][0]) for f in FIELDS[1:]] == [1, 19999, 0, 1, 20000]
    assert (graph_expect("star", 20, 20, 3)[2][0, :19999] == 19999).all() and graph_expect("star", 20, 20, 1)[3]["n_core"][0] == 20000
    assert graph_expect("cliques", 20, 20, 1)[3]["n_noise"][0] == 500 and graph_expect("cliques", 20, 20, 0)[3]["n_clusters"][0] >= 500
    for mn in (2, 3, 4):   # the random graph does not degenerate: all three kinds occur
        lv = graph_expect("gnm_30000", 20, 28, mn)[3]
        assert min(lv["n_core"][0], lv["n_border"][0], lv["n_noise"][0]) >= 1000, (mn, [int(lv[f][0]) for f in FIELDS])
    lv = graph_expect("repeated", 20, 28, 3)[3]   # a pair given 1,000 times counts 1,000 times: both ends are core
    assert lv["n_core"][0] == 2 and lv["n_clusters"][0] == 1 and lv["n_noise"][0] == 8
    assert graph_expect("none", 20, 28, 3)[3]["n_noise"].tolist() == [50] * 9
    cl, deg, an, lv = graph_expect("path_descending", 20, 20, 2)
    assert lv["n_core"][0] == 4097 and lv["n_border"][0] == 2 and (an[0, 0], an[0, 4098]) == (1, 4097) and lv["n_noise"][0] == 0


def test_the_bridge_joins_everything_for_components():
    n, _, _, _, edges = graph("bridge")
    ctx = graph_ctx("bridge", -1)
    comp, lv = ctx.components_from_edges(edges, 20)
    assert lv["n_components"][0] == 1 and (comp == 0).all()
    lvd = ctx.density_from_edges(edges, 20, min_neighbors=3)[0]
    assert (lvd["n_clusters"][0], lvd["n_border"][0], lvd["n_noise"][0]) == (2, 2, 3)


MUSI_TABLE = {32: (17899, 2080, 222, 155, 5), 36: (8273, 1511, 343, 603, 28), 38: (6458, 1216, 308, 933, 60), 40: (5626, 1019, 206, 1232, 107),
              44: (4954, 880, 54, 1523, 117)}   # threshold -> edges, core, border, noise, clusters at min_neighbors = 3


def test_from_edges_on_musi_equals_the_definition_and_the_table():
    want = oracle_expect("musi", 32, 44, 3)
    for t, row in MUSI_TABLE.items():
        assert tuple(int(want[3][f][t - 32]) for f in FIELDS[:5]) == row, t
    ctx = pep_ctx("musi", -1)
    edges = oracle_edges("musi", 32)
    same(ctx.density_from_edges(edges, 32, 44, 3), want)
    same_stats(ctx.last_density_stats, want, 13, 3)
    same(ctx.density_from_edges(edges, 38, min_neighbors=3), oracle_expect("musi", 38, 38, 3), "38 ")


@pytest.mark.parametrize("name", sorted(CASES) + ["musi"])
def test_min_neighbors_zero_is_components(name):
    if name == "musi":
        ctx, edges, thr, hi = pep_ctx("musi", -1), oracle_edges("musi", 20), 20, 40
    else:
        ctx, edges, thr, hi = graph_ctx(name, -1), graph(name)[4], 20, 28
    comp, clv = ctx.components_from_edges(edges, thr, hi)
    lv, cluster, degree, anchor = ctx.density_from_edges(edges, thr, hi, 0)
    assert np.array_equal(cluster[0], comp) and np.array_equal(lv["n_clusters"], clv["n_components"]) and np.array_equal(lv["largest"], clv["largest"])
    assert (anchor == np.arange(ctx.n)).all() and (lv["n_core"] == ctx.n).all() and np.array_equal(lv["n_edges"], clv["n_edges"])


# ---- CPU: the argument checks ------------------------------------------------------------------------------------------------

def test_bad_arguments_are_refused_before_the_device_is_looked_at():
    n, _, _, _, edges = graph("cliques")
    ctx = graph_ctx("cliques", -1)
    heads = [(N.lib.hmk_density_shifted, (3, 0)), (N.lib.hmk_density_from_edges, ep(edges)), (N.lib.hmk_density_from_edges_dev, (None, 0))]
    for fn, head in heads:   # the same checks in all three, on a host-only context
        assert raw(ctx, fn, head, 20, 22, -1)[0] == N.HMK_ERR_BAD_ARG
        assert raw(ctx, fn, head, 21, 20, 3)[0] == N.HMK_ERR_BAD_ARG
        assert raw(ctx, fn, head, 20, 276, 3)[0] == N.HMK_ERR_BAD_ARG
        assert raw(ctx, fn, head, 32700, 32768, 3)[0] == N.HMK_ERR_BAD_ARG
        assert raw(ctx, fn, head, -2 ** 31, 2 ** 31 - 1, 3)[0] == N.HMK_ERR_BAD_ARG
        assert raw(ctx, fn, head, 20, 22, 3, False, False, False, False)[0] == N.HMK_ERR_BAD_ARG
        assert fn(None, *head, 20, 20, 3, None, None, None, None, None) == N.HMK_ERR_BAD_ARG
    assert raw(ctx, N.lib.hmk_density_from_edges, ep(edges), 20, 275, 3)[0] == 0   # 256 levels are allowed
    with pytest.raises(ValueError, match="min_neighbors"):
        ctx.density_from_edges(edges, 20, 22, -1)
    with pytest.raises(ValueError, match="threshold_hi"):
        ctx.density_from_edges(edges, 20, 19)
    for x, m in ((3, n), (n, 3), (2 ** 24 - 1, 0), (5, 5)):   # an index >= n either side, a self pair, whatever the score
        for score in (25, 3):
            bad = edges.copy()
            bad[100] = hammock_amd.pack_edges(np.array([x]), np.array([m]), np.array([score]))[0]
            with pytest.raises(ValueError, match="outside"):
                ctx.density_from_edges(bad, 20, 28)
    assert raw(ctx, N.lib.hmk_density_from_edges, (None, 5), 20, 20, 3)[0] == N.HMK_ERR_BAD_ARG
    same(ctx.density_from_edges(edges, 20, 28, 3), graph_expect("cliques", 20, 28, 3), "after the refusals ")
    asym = matrix().copy()
    asym[3, 5] += 1
    actx = hammock_amd.Context(asym, device=-1)
    actx.set_sequences(residues=vertices(n)[0], offsets=vertices(n)[1])
    with pytest.raises(ValueError, match="symmetric"):
        actx.density_shifted(3, 0, 20)


def test_the_device_forms_need_a_device_and_an_empty_set_is_ok():
    ctx = graph_ctx("cliques", -1)
    with pytest.raises(hammock_amd.DeviceError):
        ctx.density_shifted(3, 0, 20, 24)
    with pytest.raises(hammock_amd.DeviceError):
        ctx.density_from_edges_dev(0, 0, 20, 24)
    empty = hammock_amd.Context(matrix(), device=-1)
    lv, cluster, degree, anchor = empty.density_from_edges(np.zeros(0, dtype=np.uint64), 20, 24)
    assert cluster.shape == degree.shape == anchor.shape == (5, 0) and lv.size == 5 and not any(lv[f].any() for f in FIELDS)
    assert raw(empty, N.lib.hmk_density_from_edges, (None, 0), 20, 24, 3, False, False, False, False)[0] == 0
    assert raw(empty, N.lib.hmk_density_shifted, (3, 0), 20, 24, 3)[0] == 0 and raw(empty, N.lib.hmk_density_from_edges_dev, (None, 0), 20, 24, 3)[0] == 0
    assert (empty.last_density_stats.n_levels, empty.last_density_stats.min_neighbors) == (5, 3)


def test_cli_density_argument_and_file_errors(tmp_path):
    fa = os.path.join(GOLDEN, "musi.fa")
    r = cli("density", "-d", str(tmp_path / "a"))
    assert r.returncode == 2 and "-i or --input" in r.stderr
    assert not (tmp_path / "a").exists()
    r = cli("density", "-i", fa, "--devices", "0,1", "-d", str(tmp_path / "a"))
    assert r.returncode == 2 and "--devices" in r.stderr
    r = cli("density", "-i", fa, "-f", "seq", "-d", str(tmp_path / "a"))
    assert r.returncode == 2 and "-f" in r.stderr
    r = cli("density", "-i", fa, "--min_neighbors", "-1", "-d", str(tmp_path / "a"))
    assert r.returncode == 2 and "--min_neighbors" in r.stderr
    assert not (tmp_path / "a").exists()
    r = cli("density", "-i", fa, "-g", "26", "--scan_to", "25", "-d", str(tmp_path / "b"))
    assert r.returncode == 2 and "--scan_to" in r.stderr
    r = cli("density", "-i", fa, "--scan_to", "276", "-d", str(tmp_path / "c"))   # the derived threshold is 20
    assert r.returncode == 2 and "--scan_to" in r.stderr and "20 up to 275" in r.stderr
    r = cli("density", "-i", fa, "-g", "30", "--scan_to", "34", "--pick", "35", "-d", str(tmp_path / "f"))
    assert r.returncode == 2 and "--pick" in r.stderr and "30 up to 34" in r.stderr
    r = cli("density", "-i", fa, "-d", str(tmp_path / "c"))   # the directory exists now
    assert r.returncode == 2 and "Output directory exists" in r.stderr
    r = cli("density", "-i", str(tmp_path / "missing.fa"), "-d", str(tmp_path / "d"))
    assert r.returncode != 0
    r = cli("density", "-i", fa, "-l", "no_such_label", "-d", str(tmp_path / "e"))
    assert r.returncode == 3 and "No sequences" in r.stderr
    assert "hammock-hip density -i" in cli("--help").stderr


# ---- GPU: the synthetic graphs through the device kernels --------------------------------------------------------------------

def wanted_grids(n, e, n_edges, single):
    """kernel -> the grids its launcher asks for (k_density.hip's launchers) on n vertices and e given edges, n_edges[l] of them
    at level l: per level the link step takes the chunks of the prefix, the degree step those from the level's own run on"""
    by_vertex = min(-(-n // 256), 2048)
    grids = {k: {by_vertex} for k in ("k_den_init", "k_den_core", "k_den_labels", "k_den_sizes")} if n else {}
    degree, link = set(), set()
    if single:
        degree.add(min(-(-e // 1024), 2048))
        link.add(min(-(-e // 1024), 2048))
    else:
        prefix = [int(v) for v in n_edges] + [0]
        for l in range(len(n_edges)):
            chunks, first = -(-prefix[l] // 1024), prefix[l + 1] // 1024
            degree.add(min(max(chunks - first, 0), 2048))
            link.add(min(chunks, 2048))
    grids["k_den_degree"], grids["k_den_link"] = degree - {0}, link - {0}
    return grids


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [0, 1, 3])
@pytest.mark.parametrize("name,mn", GRAPH_CASES)
def test_from_edges_dev_equals_the_definition_on_the_synthetic_graphs(gpu, monkeypatch, capfd, name, mn, cap):
    n, _, _, _, edges = graph(name)
    ctx = graph_ctx(name, 0)
    d = device_edges(edges)
    host = graph_ctx(name, -1)
    if cap:
        monkeypatch.setenv("HMK_TEST_GRID_CAP", str(cap))
    for thr, hi in RANGES:
        capfd.readouterr()
        want = graph_expect(name, thr, hi, mn)
        got = ctx.density_from_edges_dev(d.data_ptr(), d.numel(), thr, hi, mn)
        err = capfd.readouterr().err
        same(got, want, f"{thr}..{hi} ")
        s = ctx.last_density_stats
        same_stats(s, want, hi - thr + 1, mn)
        assert s.pairs_scored == 0 and s.kernel_ms == 0.0 and s.density_ms > 0.0
        other = host.density_from_edges(edges, thr, hi, mn)   # the two implementations agree byte for byte
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, other))
        lines = {}
        for kernel, wanted, launched in GRID_LINE.findall(err):
            lines.setdefault(kernel, set()).add((int(wanted), int(launched)))
        cut = {k: {(w, cap) for w in ws if w > cap} for k, ws in wanted_grids(n, edges.size, want[3]["n_edges"], hi == thr).items() if cap}
        assert {k: v for k, v in lines.items() if k.startswith("k_den_")} == {k: v for k, v in cut.items() if v}
        if name in ("star", "gnm_30000") and cap and hi == thr:   # here every grid-stride kernel runs its loop well beyond the first iteration
            assert set(k for k, v in cut.items() if v) == set(wanted_grids(n, edges.size, want[3]["n_edges"], hi == thr))
            assert all(max(w for w, _ in v) >= 2 * cap for v in cut.values())


@pytest.mark.gpu
def test_from_edges_dev_refuses_invalid_edges_and_goes_on(gpu):
    n, _, _, _, edges = graph("gnm_30000")
    ctx = graph_ctx("gnm_30000", 0)
    for x, m in ((3, n), (n + 5, 3), (2 ** 24 - 1, 2 ** 24 - 2), (5, 5)):
        bad = edges.copy()
        bad[7000] = hammock_amd.pack_edges(np.array([x]), np.array([m]), np.array([25]))[0]
        d = device_edges(bad)
        with pytest.raises(ValueError, match="outside"):
            ctx.density_from_edges_dev(d.data_ptr(), d.numel(), 20, 28, 3)
        assert raw(ctx, N.lib.hmk_density_from_edges_dev, (d.data_ptr(), d.numel()), 20, 20, 3)[0] == N.HMK_ERR_BAD_ARG
        d = device_edges(edges)
        same(ctx.density_from_edges_dev(d.data_ptr(), d.numel(), 20, 28, 3), graph_expect("gnm_30000", 20, 28, 3), "the next call ")
    assert raw(ctx, N.lib.hmk_density_from_edges_dev, (None, 5), 20, 20, 3)[0] == N.HMK_ERR_BAD_ARG


@pytest.mark.gpu
def test_rows_come_back_in_several_batches(gpu):
    """The requested rows wait on the device, as many levels as fit 256 MiB (sizing::density_rows_per_batch): 256 levels of
    300,000 vertices with two arrays are 2.4 MB a level, 111 levels a batch, three batches (levels 255 ... 145, 144 ... 34, 33 ... 0).
    Every level against _from_edges, the levels on both sides of each batch boundary against the definition."""
    n, e = 300_000, 450_000
    rng = np.random.default_rng(99)
    ends = tc._gnm(rng, n, e)
    flip = rng.random(e) < 0.5
    x, m, sc = np.where(flip, ends[1], ends[0]), np.where(flip, ends[0], ends[1]), np.arange(e) % 256
    edges = hammock_amd.pack_edges(x, m, sc)
    res, off = vertices(n)
    ctx = hammock_amd.Context(matrix(), device=0)
    ctx.set_sequences(residues=res, offsets=off)
    d = device_edges(edges)
    lv, cluster, degree, anchor = ctx.density_from_edges_dev(d.data_ptr(), d.numel(), 0, 255, 2, arrays=(True, False, True))
    assert degree is None
    host = hammock_amd.Context(matrix(), device=-1)
    host.set_sequences(residues=res, offsets=off)
    hlv, hcluster, _, hanchor = host.density_from_edges(edges, 0, 255, 2, arrays=(True, False, True))
    assert lv.tobytes() == hlv.tobytes() and np.array_equal(cluster, hcluster) and np.array_equal(anchor, hanchor)
    for t in (0, 33, 34, 144, 145, 255):
        want = definition(n, x, m, sc, t, t, 2)
        same((lv[t:t + 1], cluster[t:t + 1], None, anchor[t:t + 1]), want, f"level {t} ")
        assert min(want[3]["n_core"][0], want[3]["n_border"][0], want[3]["n_noise"][0]) > 0


# ---- GPU: the scoring call -----------------------------------------------------------------------------------------------------

SCORED = [("musi", 32, 44, 3), ("musi", 20, 32, 10), ("synth12", 20, 28, 3), ("synth7to12", 14, 22, 3), ("keyed", 20, 26, 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,thr,hi,mn", SCORED)
def test_density_shifted_equals_the_definition_on_oracle_scores_and_from_edges(gpu, monkeypatch, capfd, name, thr, hi, mn):
    res, off, X, p, _, _ = peptides(name)
    n = len(off) - 1
    ctx = pep_ctx(name)
    want = oracle_expect(name, thr, hi, mn)
    if name == "keyed":   # the planner's timeline names the step only a key-sorted plan has
        monkeypatch.setenv("HMK_GREEDY_TIMING", "1")
        capfd.readouterr()
    got = ctx.density_shifted(X, p, thr, hi, mn)
    if name == "keyed":
        err = capfd.readouterr().err
        assert "[hmk plan] row-shared groups" in err, "the plan of this case is not key-sorted"
        looked = re.findall(r"^\[hmk density\] threshold (\d+): (\d+) vertices turned core, the link step looked at (\d+) of (\d+) edges$", err, re.M)
        assert [int(t) for t, _, _, _ in looked] == list(range(thr, hi + 1)) and all(int(k) <= int(e) for _, _, k, e in looked)
        assert [int(e) for _, _, _, e in looked] == want[3]["n_edges"].tolist()
        monkeypatch.delenv("HMK_GREEDY_TIMING")
    same(got, want)
    s = ctx.last_density_stats
    same_stats(s, want, hi - thr + 1, mn)
    assert s.pairs_scored == n * (n - 1) // 2 and s.kernel_ms > 0 and s.density_ms > 0
    assert min(want[3]["n_core"].max(), want[3]["n_border"].max(), want[3]["n_noise"].max()) > 0   # (the reference: all kinds occur)
    edges, _ = ctx.neighbors_shifted(X, p, thr)
    other = ctx.density_from_edges(edges, thr, hi, mn)
    same(other, want, "from its own edges ")
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, other))
    mid = (thr + hi) // 2   # a single level: the pass's segments where they lie
    same(ctx.density_shifted(X, p, mid, min_neighbors=mn), oracle_expect(name, mid, mid, mn), "single level ")
    same_stats(ctx.last_density_stats, oracle_expect(name, mid, mid, mn), 1, mn)
    if name == "musi" and mn == 3:
        for t, row in MUSI_TABLE.items():
            assert tuple(int(got[0][f][t - 32]) for f in FIELDS[:5]) == row, t
    if name == "keyed":   # the other order of the pass: identical output
        monkeypatch.setenv("HMK_NO_KEY_SORT", "1")
        monkeypatch.setenv("HMK_GREEDY_TIMING", "1")
        fresh = pep_ctx(name)
        capfd.readouterr()
        plain = fresh.density_shifted(X, p, thr, hi, mn)
        err = capfd.readouterr().err
        assert "[hmk plan] device copies" in err and "row-shared groups" not in err
        monkeypatch.delenv("HMK_NO_KEY_SORT")
        monkeypatch.delenv("HMK_GREEDY_TIMING")
        assert all(a.tobytes() == b.tobytes() for a, b in zip(plain, got))


@pytest.mark.gpu
def test_the_grow_path_gives_the_same(gpu, monkeypatch, capfd):
    """a first edge buffer of 2^20 entries (16,384 per segment) under 1.7 million edges: the pass is scored twice, which the
    call's timeline says"""
    res, off, X, p, thr, hi = peptides("three_letters")
    want = oracle_expect("three_letters", thr, hi, 1700)   # (mean degree 1,610 ... 1,877 over the range: core and border both occur)
    assert want[3]["n_edges"][0] > 2 ** 20 and min(want[3]["n_core"].max(), want[3]["n_border"].max()) > 0
    monkeypatch.setenv("HMK_EDGE_GUESS", "4096")
    monkeypatch.setenv("HMK_GREEDY_TIMING", "1")
    ctx = pep_ctx("three_letters")   # a fresh context: no buffer grown by an earlier call
    capfd.readouterr()
    got = ctx.density_shifted(X, p, thr, hi, 1700)
    err = capfd.readouterr().err
    monkeypatch.delenv("HMK_EDGE_GUESS")
    monkeypatch.delenv("HMK_GREEDY_TIMING")
    assert len(re.findall(r"^\[hmk\] an edge segment overflowed \(\d+ entries for 16384\): \d+ entries next, scoring again$", err, re.M)) == 1
    same(got, want)


@pytest.mark.gpu
def test_state_between_calls_null_outputs_and_a_threshold_above_every_score(gpu):
    res, off, X, p, _, _ = peptides("musi")
    n = len(off) - 1
    ctx = pep_ctx("musi")
    first = ctx.density_shifted(X, p, 20, 44, 3)   # a wide range, then a single level, then another min_neighbors: one context
    same(first, oracle_expect("musi", 20, 44, 3))
    same(ctx.density_shifted(X, p, 38, min_neighbors=3), oracle_expect("musi", 38, 38, 3), "a single level ")
    same(ctx.density_shifted(X, p, 20, 32, 10), oracle_expect("musi", 20, 32, 10), "another min_neighbors ")
    ctx.neighbors_shifted(X, p, 33)
    again = ctx.density_shifted(X, p, 20, 44, 3)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, first))
    want = oracle_expect("musi", 32, 44, 3)
    for off_ in range(4):   # each output NULL in turn
        flags = [k != off_ for k in range(4)]
        st, got, _ = raw(ctx, N.lib.hmk_density_shifted, (X, p), 32, 44, 3, *flags)
        assert st == 0 and [g is None for g in (got[1], got[3], got[2], got[0])] == [not f for f in flags]
        same(got, want, f"null output {off_} ")
    lv, cluster, degree, anchor = ctx.density_shifted(X, p, 32, 44, 3, arrays=(True, False, False), levels=False)
    assert lv is None and degree is None and anchor is None
    same((None, cluster, None, None), want)
    top = int(oracle_scores("musi")[3].max())
    lv, cluster, degree, anchor = ctx.density_shifted(X, p, top, top + 2, 1)
    assert lv["n_edges"][0] > 0 and lv["n_edges"][1] == 0 and (lv["n_noise"][1:] == n).all() and not lv["n_clusters"][1:].any()
    lv, cluster, degree, anchor = ctx.density_shifted(X, p, top + 1, min_neighbors=1)   # above every score: all noise
    assert (cluster == NOISE).all() and (anchor == NOISE).all() and not degree.any() and lv[0].tolist() == (0, 0, 0, n, 0, 0, 0)


@pytest.mark.gpu
def test_the_device_list_runs_on_the_root(gpu):
    res, off, X, p, thr, hi = peptides("synth12")
    ctx = hammock_amd.Context(matrix(), device=[0, 0])
    ctx.set_sequences(residues=res, offsets=off)
    same(ctx.density_shifted(X, p, thr, hi, 3), oracle_expect("synth12", thr, hi, 3))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["musi", "synth12"])
def test_min_neighbors_zero_is_components_shifted(gpu, name):
    res, off, X, p, thr, hi = peptides(name)
    ctx = pep_ctx(name)
    comp, clv = ctx.components_shifted(X, p, thr, hi)
    lv, cluster, degree, anchor = ctx.density_shifted(X, p, thr, hi, 0)
    same((lv, cluster, degree, anchor), oracle_expect(name, thr, hi, 0))
    assert np.array_equal(cluster[0], comp) and np.array_equal(lv["n_clusters"], clv["n_components"]) and np.array_equal(lv["largest"], clv["largest"])
    assert np.array_equal(lv["n_edges"], clv["n_edges"]) and (lv["n_core"] == ctx.n).all()


# ---- GPU: the mode ---------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_cli_density_on_musi(gpu, tmp_path):
    from oracle import c_oracle, hammock_oracle as po
    fa = os.path.join(GOLDEN, "musi.fa")
    seqs = po.load_unique_sequences_from_fasta(fa)
    labels = po.get_sorted_labels(seqs)
    n = len(seqs)
    strings = [s.get_sequence_string() for s in seqs]
    res, off = c_oracle.pack(strings)
    x, m = np.triu_indices(n, 1)
    st, sc = c_oracle.score_pairs(matrix(), res, off, m, x, 0, 3, 0)
    assert st == 0
    keep = sc >= 36
    cluster, degree, anchor, lv = definition(n, x[keep], m[keep], sc[keep], 36, 44, 3)
    row = 2   # --pick 38
    members = {}
    for i in range(n):
        members.setdefault(i if cluster[row, i] == NOISE else int(cluster[row, i]), []).append(seqs[i])
    ids = sorted(members, key=lambda c: (len(members[c]) == 1, c))   # clusters of several sequences first, each group by ascending id
    clusters = [po.Cluster(list(members[c]), c + 1) for c in ids]
    exp = tmp_path / "exp"
    exp.mkdir()
    po.save_cluster_sequences_csv(clusters, str(exp / "initial_clusters_sequences.tsv"), labels)
    po.write_cluster_sequences_csv(seqs, clusters, str(exp / "initial_clusters_sequences_original_order.tsv"), labels)
    po.save_clusters_csv(clusters, str(exp / "initial_clusters.tsv"), labels)
    rows = ["threshold\tedges\tcore\tborder\tnoise\tclusters\tlargest"]
    rows += ["\t".join(str(v) for v in [36 + k] + [int(lv[f][k]) for f in FIELDS]) for k in range(9)]
    mrows = ["sequence\tkind\tdegree\tcluster\tanchor"]
    for i in range(n):
        c, a = int(cluster[row, i]), int(anchor[row, i])
        kind = "noise" if c == NOISE else "core" if a == i else "border"
        mrows.append("\t".join([strings[i], kind, str(int(degree[row, i])), "NA" if c == NOISE else str(c + 1), "NA" if a == NOISE else strings[a]]))
    out = tmp_path / "out"
    r = cli("density", "-i", fa, "-d", str(out), "-g", "36", "--min_neighbors", "3", "--scan_to", "44", "--pick", "38", timeout=600)
    assert r.returncode == 0, r.stderr
    assert "Max shift not set. Setting automatically to: 3" in r.stderr
    assert (out / "density_levels.tsv").read_text() == "\n".join(rows) + "\n"
    assert (out / "density_members.tsv").read_text() == "\n".join(mrows) + "\n"
    for name in ("initial_clusters_sequences.tsv", "initial_clusters_sequences_original_order.tsv", "initial_clusters.tsv"):
        assert (out / name).read_bytes() == (exp / name).read_bytes(), name
    log = (out / "run.log").read_text()
    assert 'Program started in mode "density"' in log and f"Resulting clusers at threshold 38: {len(clusters)}" in log
    assert "At threshold 38: core 1216, border 308, noise 933, clusters 60, largest: " in log and "Program successfully ended." in log
    # the files load back through the loader behind --clusters: every sequence once, under its cluster's id
    r = cli("io-selftest", "clusters", str(out / "initial_clusters_sequences.tsv"))
    assert r.returncode == 0, r.stderr
    loaded = {line.split("\t")[1]: int(line.split("\t")[0]) for line in r.stdout.splitlines()}
    assert loaded == {strings[i]: (i if cluster[row, i] == NOISE else int(cluster[row, i])) + 1 for i in range(n)}
