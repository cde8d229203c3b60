#!/usr/bin/env python3
"""bench_continue.py -- continuing a greedy clustering with new sequences (hmk_greedy_continue) on one MI355X.

Every workload clusters a base set with hmk_greedy_cluster (BLOSUM62, max shift 3, shift penalty 0, threshold 20, the CLI's default
limit of round(0.025 n) initial clusters), takes its clusters of more than one member as the candidates (members in
Cluster.getSequences() order) and continues them with the new sequences; members first, new sequences behind them.
  (a) base: bench.py's 10^5 synthetic 12-mers (SplitMix64 seed 1); new: 10^4 12-mers of seed 2
  (b) tests/golden/antibodies.fa.gz as unique sequences with their counts, in greedy's size order: the first 64,000 are the
      base, the rest are new (dense families: long chains)
  (c) base: 10^6 12-mers of seed 1; new: 10^5 of seed 2
Per workload:
  wall_ms              the greedy_continue call as Python sees it
  kernel_ms            stats.kernel_ms: the two passes (members x new, new x new)
  loop_ms              stats.loop_ms: CSR, pre-check and the device loop (wall)
  greedy_base_ms       the base set's hmk_greedy_cluster call
  greedy_union_ms      a fresh hmk_greedy_cluster on base + new
Medians of --steps calls after --warmup untimed ones.  Prints one JSON line per workload.

    python tools/bench_continue.py [--steps 10] [--warmup 3] [--only a|b|c]
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


def load_antibodies():
    """unique sequences of the antibodies example with their counts, in greedy's default order (size, then string, descending)"""
    import gzip
    counts = {}
    with gzip.open(os.path.join(ROOT, "tests", "golden", "antibodies.fa.gz"), "rt") as fh:
        for line in fh:
            line = line.strip()
            if line and not line.startswith(">"):
                counts[line.upper()] = counts.get(line.upper(), 0) + 1
    seqs = sorted(counts, key=lambda t: (counts[t], t), reverse=True)
    return seqs, [counts[t] for t in seqs]


def workload(hammock_amd, M, name, base, base_sizes, new, new_sizes, args):
    n, nq = len(base), len(new)
    res, off = hammock_amd.pack_sequences(base)
    ctx = hammock_amd.Context(M, device=0)
    ctx.set_sequences(residues=res, offsets=off, sizes=np.asarray(base_sizes, np.int32))
    limit = int(round(n * 0.025))

    def median(call, pick):
        for _ in range(args.warmup):
            call()
        wall, picked = [], []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            r = call()
            wall.append((time.perf_counter() - t0) * 1e3)
            picked.append(pick(r))
        return float(np.median(wall)), np.median(np.asarray(picked), axis=0)

    gbase, _ = median(lambda: ctx.greedy_cluster(X, P, THR, limit), lambda r: 0.0)
    cid, _, _ = ctx.greedy_cluster(X, P, THR, limit)
    rank = ctx.member_rank[:n].copy()
    counts = np.bincount(cid, minlength=n)
    members = np.nonzero(counts[cid] > 1)[0]
    members = members[np.lexsort((rank[members], cid[members]))]
    ids, slot = np.unique(cid[members], return_inverse=True)
    nm = len(members)
    seqs = [base[i] for i in members] + list(new)
    sizes = np.concatenate([np.asarray(base_sizes, np.int32)[members], np.asarray(new_sizes, np.int32)])
    r2, o2 = hammock_amd.pack_sequences(seqs)
    ctx.set_sequences(residues=r2, offsets=o2, sizes=sizes)

    def cont():
        ctx.greedy_continue(nm, nm + nq, 0, nm, slot, ids, X, P, THR)
        s = ctx.last_continue_stats
        return (s.kernel_ms, s.loop_ms)
    wall, (kern, loop) = median(cont, lambda r: r)
    st = ctx.last_continue_stats
    ctx.close()
    ures, uoff = hammock_amd.pack_sequences(list(base) + list(new))
    gctx = hammock_amd.Context(M, device=0)
    gctx.set_sequences(residues=ures, offsets=uoff, sizes=np.concatenate([np.asarray(base_sizes, np.int32), np.asarray(new_sizes, np.int32)]))
    gunion, _ = median(lambda: gctx.greedy_cluster(X, P, THR, int(round((n + nq) * 0.025))), lambda r: 0.0)
    gctx.close()
    print(json.dumps({"workload": name, "n_base": n, "n_clusters": int(len(ids)), "n_members": int(nm), "n_new": nq, "wall_ms": wall,
                      "kernel_ms": float(kern), "loop_ms": float(loop), "n_edges": int(st.n_edges), "pairs_scored": int(st.pairs_scored),
                      "joins": int(st.n_joined), "loop_rounds": int(st.loop_rounds), "host_precheck": int(st.host_precheck),
                      "greedy_base_ms": gbase, "greedy_union_ms": gunion, "wall_over_greedy_base": wall / gbase,
                      "wall_over_greedy_union": wall / gunion}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=["a", "b", "c"], default=None)
    args = ap.parse_args()
    import hammock_amd
    from hammock_amd.synth import synth_peptides
    with open(os.path.join(ROOT, "tests", "golden", "matrices.json")) as fh:
        M = np.asarray(json.load(fh)["matrices"]["blosum62"], dtype=np.int32)

    def synth(seed, n):
        res, off = synth_peptides(seed, n, 12)
        return [res[off[i]:off[i + 1]] for i in range(n)]
    if args.only in (None, "a"):
        workload(hammock_amd, M, "a: 10^4 new 12-mers into the greedy clusters of 10^5", synth(1, 100_000), np.ones(100_000, np.int32),
                 synth(2, 10_000), np.ones(10_000, np.int32), args)
    if args.only in (None, "b"):
        seqs, counts = load_antibodies()
        enc = [hammock_amd.encode(t) for t in seqs]
        workload(hammock_amd, M, "b: antibodies example, the first 64,000 unique sequences, then the rest", enc[:64_000], counts[:64_000],
                 enc[64_000:], counts[64_000:], args)
    if args.only in (None, "c"):
        workload(hammock_amd, M, "c: 10^5 new 12-mers into the greedy clusters of 10^6", synth(1, 1_000_000), np.ones(1_000_000, np.int32),
                 synth(2, 100_000), np.ones(100_000, np.int32), args)


if __name__ == "__main__":
    main()
