#!/usr/bin/env python3
"""bench_merge.py -- merging given clusters by complete linkage (hmk_clinkage_merge, hmk_cluster_pairs_shifted) on one MI355X.

BLOSUM62, max shift 3, shift penalty 0, threshold 20, greedy clusterings with the CLI's default limit of round(0.025 n) initial
clusters (hmk_greedy_cluster).  Workloads:
  (a) singleton seeds (slot = sequence, ids 1 .. n) on 10^4 synthetic 12-mers (seed 3) and on MUSI, beside hmk_clinkage_cluster
      on the same set: both walls with their min-max spread;
  (b) the multi-member clusters of the greedy on bench.py's 10^5 set (seed 1);
  (c) all clusters of that greedy (the whole set);
  (d) two greedy runs on the halves of the 10^5 set, merged, beside one greedy on the whole set.
Per workload: wall_ms of the call as Python sees it, and from hmk_merge_stats kernel_ms (the pass), graph_ms (CSR + cluster graph +
hand-over), chain_ms (host chain), the slots, members, cluster pairs and merges.  pass_ms / csr_ms of the clustering calls on the
same members: hmk_neighbors_shifted's kernel_ms and hmk_greedy_last_phases().csr_ms.  graph_over_pass = (graph_ms - csr_ms) /
pass_ms.  Medians of --steps calls after --warmup untimed ones on a resident context.  Prints one JSON line.  --only-parent: the
part that runs on a build without the merge calls (clinkage_cluster walls, pass_ms, csr_ms), for alternating runs of two builds.

    python tools/bench_merge.py [--steps 10] [--warmup 3] [--only-parent] [--skip-full-chain]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

X, P, THR = 3, 0, 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only-parent", action="store_true", help="only what a build without the merge calls can run")
    ap.add_argument("--skip-full-chain", action="store_true", help="(c): the cluster graph only, not the chain over all clusters")
    args = ap.parse_args()
    import hammock_amd
    from hammock_amd.synth import synth_peptides
    from oracle import hammock_oracle as po
    with open(os.path.join(ROOT, "tests", "golden", "matrices.json")) as fh:
        M = np.asarray(json.load(fh)["matrices"]["blosum62"], dtype=np.int32)
    ctx = hammock_amd.Context(M, device=0)

    def timed(call, pick=lambda r: 0.0):
        for _ in range(args.warmup):
            call()
        wall, picked = [], []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            r = call()
            wall.append((time.perf_counter() - t0) * 1e3)
            picked.append(pick(r))
        return {"median": float(np.median(wall)), "min": float(np.min(wall)), "max": float(np.max(wall))}, picked

    def med(rows, key):
        return float(np.median([getattr(s, key) for s in rows]))

    def merge_row(name, n, mc, ids, chain=True):
        """the uploaded set's members [0, n) in slots mc"""
        ncl = len(ids)
        row = {"workload": name, "slots": int(ncl), "members": int(n)}
        _, st = timed(lambda: ctx.neighbors_shifted(X, P, THR)[1], lambda s: s.kernel_ms)
        row["pass_ms"] = float(np.median(st))
        if args.only_parent:
            return row
        wall, st = timed(lambda: ctx.cluster_pairs_shifted(0, n, mc, ncl, X, P, THR) is None or ctx.last_merge_stats, lambda s: s)
        row.update({"pairs_wall_ms": wall, "pairs_kernel_ms": med(st, "kernel_ms"), "pairs_graph_ms": med(st, "graph_ms"),
                    "cluster_pairs": int(st[-1].cluster_pairs), "n_edges": int(st[-1].n_edges)})
        if chain:
            wall, st = timed(lambda: ctx.clinkage_merge(0, n, mc, ids, X, P, THR) is None or ctx.last_merge_stats, lambda s: s)
            row.update({"merge_wall_ms": wall, "kernel_ms": med(st, "kernel_ms"), "graph_ms": med(st, "graph_ms"), "chain_ms": med(st, "chain_ms"),
                        "merges": int(st[-1].merges), "result_clusters": int(st[-1].n_result_clusters)})
        return row

    out = {"what": "merge of given clusters, BLOSUM62, X=3, p=0, threshold 20", "runs": []}

    # (a) singleton seeds beside hmk_clinkage_cluster
    musi = [s.get_sequence_string() for s in po.load_unique_sequences_from_fasta(os.path.join(ROOT, "tests", "golden", "musi.fa"))]
    for name, (res, off) in (("a: singleton seeds, 1e4 synthetic 12-mers", synth_peptides(3, 10_000, 12)),
                             ("a: singleton seeds, MUSI", hammock_amd.pack_sequences(musi))):
        n = len(off) - 1
        ctx.set_sequences(residues=res, offsets=off)
        wall, _ = timed(lambda: ctx.clinkage_cluster(X, P, THR))
        row = merge_row(name, n, np.arange(n), np.arange(1, n + 1))
        row["clinkage_cluster_wall_ms"] = wall
        out["runs"].append(row)

    # the 10^5 greedy
    n = 100_000
    res, off = synth_peptides(1, n, 12)
    ctx.set_sequences(residues=res, offsets=off)
    wall_whole, _ = timed(lambda: ctx.greedy_cluster(X, P, THR, int(round(n * 0.025))))
    cid, _, _ = ctx.greedy_cluster(X, P, THR, int(round(n * 0.025)))
    csr_all = float(ctx.greedy_phases()["csr_ms"])
    ids_all, mc_all, counts = np.unique(cid, return_inverse=True, return_counts=True)

    # (b) its multi-member clusters
    keep = np.flatnonzero(counts[mc_all] > 1)
    sub = res.reshape(n, 12)[keep].ravel()
    ctx.set_sequences(residues=sub, offsets=(np.arange(len(keep) + 1) * 12).astype(np.uint32))
    ids_b, mc_b = np.unique(cid[keep], return_inverse=True)
    ctx.greedy_cluster(X, P, THR, int(round(len(keep) * 0.025)))
    csr_b = float(ctx.greedy_phases()["csr_ms"])
    row = merge_row("b: multi-member clusters of the 1e5 greedy", len(keep), mc_b, np.arange(1, len(ids_b) + 1))
    row["csr_ms"] = csr_b
    if "graph_ms" in row:
        row["graph_over_pass"] = (row["graph_ms"] - csr_b) / row["pass_ms"]
    out["runs"].append(row)

    # (c) all its clusters
    ctx.set_sequences(residues=res, offsets=off)
    row = merge_row("c: all clusters of the 1e5 greedy", n, mc_all, np.arange(1, len(ids_all) + 1), chain=not args.skip_full_chain)
    row["csr_ms"] = csr_all
    if "pairs_graph_ms" in row:
        row["graph_over_pass"] = (row.get("graph_ms", row["pairs_graph_ms"]) - csr_all) / row["pass_ms"]
    out["runs"].append(row)

    # (d) two greedy runs on the halves, merged
    if not args.only_parent:
        half = n // 2
        parts = []
        for lo in (0, half):
            ctx.set_sequences(residues=res[lo * 12:(lo + half) * 12], offsets=(np.arange(half + 1) * 12).astype(np.uint32))
            parts.append(ctx.greedy_cluster(X, P, THR, int(round(half * 0.025)))[0])
        _, mc0 = np.unique(parts[0], return_inverse=True)
        _, mc1 = np.unique(parts[1], return_inverse=True)
        mc_d = np.concatenate([mc0, mc1 + mc0.max() + 1])
        ctx.set_sequences(residues=res, offsets=off)
        row = merge_row("d: two greedy runs on the halves of the 1e5 set, merged", n, mc_d, np.arange(1, int(mc_d.max()) + 2),
                        chain=not args.skip_full_chain)
        row.update({"greedy_whole_wall_ms": wall_whole, "greedy_whole_clusters": int(len(ids_all)), "clusters_before": int(mc_d.max()) + 1})
        out["runs"].append(row)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
