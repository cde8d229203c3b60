"""Key-sorted one-length passes: a set of 12-mers is ordered by the residues at two middle positions and a
wave whose 64 columns share a key residue adds that position's cells by scalar loads.  The order is internal: the edge set
(x, m, score) must be exactly the one of the caller's order (HMK_NO_KEY_SORT=1), for windows that share both keys, one key
or none.  Sampled rows are checked against the oracle as well.  Shards and clustering calls keep the caller's order (the
planner key-sorts plain single-part passes only): their results must match all the same.  Run with -m gpu on an MI355X."""
import gzip
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

import hammock_amd
from hammock_amd.synth import synth_peptides

pytestmark = pytest.mark.gpu

X, P, THR = 3, 0, 20


@pytest.fixture(scope="module")
def M():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need an MI355X; no HIP device is visible")
    with open(os.path.join(GOLDEN, "matrices.json")) as fh:
        return np.asarray(json.load(fh)["matrices"]["blosum62"], dtype=np.int32)


def edges_under(ctx, env, thr=THR, part=0, n_parts=1):
    """edges of one pass with the given key-sort switches (read by the library at every call)"""
    keep = {k: os.environ.get(k) for k in ("HMK_NO_KEY_SORT", "HMK_KEY_SORT_KEYS")}
    try:
        for k in keep:
            os.environ.pop(k, None)
        os.environ.update(env)
        e, _ = ctx.neighbors_shifted(X, P, thr, part, n_parts)
        return np.sort(np.asarray(e, dtype=np.uint64))
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def check_rows(M, res, off, edges, thr, rows=24):
    """every edge of a few sampled rows, against the oracle's scores of those rows"""
    from oracle import c_oracle
    n = len(off) - 1
    x, m, s = hammock_amd.edge_fields(edges)
    rng = np.random.default_rng(7)
    for r in rng.choice(n, min(rows, n), replace=False):
        others = np.delete(np.arange(n, dtype=np.uint32), r)
        st, sc = c_oracle.score_pairs(M, res, off, others, np.full(len(others), r, dtype=np.uint32), 0, X, P)
        assert st == 0
        hit = sc >= thr
        want = sorted(zip(np.minimum(others[hit], r).tolist(), np.maximum(others[hit], r).tolist(), sc[hit].tolist()))
        sel = (x == r) | (m == r)
        got = sorted(zip(x[sel].tolist(), m[sel].tolist(), s[sel].tolist()))
        assert got == want, f"row {r}"


def same_edges(M, res, off, thr=THR, oracle_rows=24, shards=(1,)):
    ctx = hammock_amd.Context(M, device=0)
    ctx.set_sequences(residues=res, offsets=off)
    base = edges_under(ctx, {"HMK_NO_KEY_SORT": "1"}, thr)
    both = edges_under(ctx, {}, thr)
    one = edges_under(ctx, {"HMK_KEY_SORT_KEYS": "1"}, thr)
    assert np.array_equal(both, base)
    assert np.array_equal(one, base)
    for k in shards:
        if k > 1:
            parts = np.sort(np.concatenate([edges_under(ctx, {}, thr, q, k) for q in range(k)]))
            assert np.array_equal(parts, base), f"{k} shards"
    if oracle_rows:
        check_rows(M, res, off, base, thr, oracle_rows)
    return base


def with_keys(res, off, fn):
    """residues of key positions 5 and 6 of every 12-mer set by fn(index) -> (a, b)"""
    res = res.copy()
    for k in range(len(off) - 1):
        res[off[k] + 5], res[off[k] + 6] = fn(k)
    return res


def test_headline_set(M):
    res, off = synth_peptides(1, 100_000, 12)
    same_edges(M, res, off, oracle_rows=8, shards=(1, 2, 4))


def test_ten_thousand_and_partial_group(M):
    for n in (10_000, 10_003, 777):
        res, off = synth_peptides(3, n, 12)
        same_edges(M, res, off, shards=(1, 2))


def test_all_windows_share_both_keys(M):
    res, off = synth_peptides(5, 5_000, 12)
    same_edges(M, with_keys(res, off, lambda k: (4, 9)), off)


def test_runs_of_length_one(M):
    res, off = synth_peptides(6, 576, 12)
    same_edges(M, with_keys(res, off, lambda k: (k // 24, k % 24)), off, thr=10)


def test_range_edge_threshold(M):
    # low thresholds: lanes start near the top of the byte (g = 128 - threshold) and hits are dense
    res, off = synth_peptides(8, 3_000, 12)
    for thr in (5, 12, 40):
        same_edges(M, res, off, thr=thr, oracle_rows=6)


def test_antibodies_twelve_mers(M):
    seqs = []
    with gzip.open(os.path.join(GOLDEN, "antibodies.fa.gz"), "rt") as fh:
        for line in fh:
            line = line.strip()
            if line and not line.startswith(">") and len(line) == 12:
                seqs.append(line)
    seqs = sorted(set(seqs))
    assert len(seqs) > 1000
    res, off = hammock_amd.pack_sequences(seqs)
    same_edges(M, res, off, oracle_rows=8)


def test_clustering_call_with_band(M):
    res, off = synth_peptides(1, 20_000, 12)
    out = []
    for env in ({"HMK_NO_KEY_SORT": "1"}, {}):
        keep = os.environ.get("HMK_NO_KEY_SORT")
        os.environ.pop("HMK_NO_KEY_SORT", None)
        os.environ.update(env)
        try:
            ctx = hammock_amd.Context(M, device=0)
            ctx.set_sequences(residues=res, offsets=off)
            cid, order, _ = ctx.greedy_cluster(X, P, THR, 500)
            out.append((cid.copy(), order.copy()))
        finally:
            os.environ.pop("HMK_NO_KEY_SORT", None)
            if keep is not None:
                os.environ["HMK_NO_KEY_SORT"] = keep
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
