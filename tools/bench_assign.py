#!/usr/bin/env python3
"""bench_assign.py -- assignment of new sequences to existing clusters (hmk_assign_shifted) on one MI355X.

The clusters are the greedy clustering (hmk_greedy_cluster: BLOSUM62, max shift 3, shift penalty 0, threshold 20, the CLI's
default limit of round(0.025 n) initial clusters) of bench.py's 10^5 synthetic 12-mers (SplitMix64 seed 1); the new sequences
are 10^4 or 10^2 synthetic 12-mers of another seed (2).  New sequences first, members behind them, in one uploaded set.  Two
candidate sets: every cluster, and only those of more than one member (the CLI's --skip_singletons).  Per run:
  wall_ms          the assign_shifted call as Python sees it (host checks and rank order, uploads, pass, aggregation, copies)
  kernel_ms        stats.kernel_ms of the call: the pass + the aggregation and selection (HIP events)
  pass_ms          stats.kernel_ms of hmk_search_shifted on the same rectangle with the members as queries -- the plan the
                   assignment builds, the pass alone
  agg_sel_ms       kernel_ms - pass_ms: count, scan, scatter, the per-run tables and the selection
  search_wall_ms   the hmk_search_shifted call as Python sees it (its edges copied to the host)
Medians of --steps calls after --warmup untimed ones; k = 1 (the CLI's default --best).  Prints one JSON line.

    python tools/bench_assign.py [--steps 10] [--warmup 3] [--k 1]
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
    ap.add_argument("--k", type=int, default=1)
    args = ap.parse_args()
    import hammock_amd
    from hammock_amd.synth import synth_peptides
    with open(os.path.join(ROOT, "tests", "golden", "matrices.json")) as fh:
        M = np.asarray(json.load(fh)["matrices"]["blosum62"], dtype=np.int32)
    n = 100_000
    res, off = synth_peptides(1, n, 12)
    ctx = hammock_amd.Context(M, device=0)
    ctx.set_sequences(residues=res, offsets=off)
    cid, _, gst = ctx.greedy_cluster(X, P, THR, int(round(n * 0.025)))
    counts = np.bincount(cid, minlength=n)
    new_res, new_off = synth_peptides(2, 10_000, 12)

    def median(call, pick):
        for _ in range(args.warmup):
            call()
        wall, picked = [], []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            r = call()
            wall.append((time.perf_counter() - t0) * 1e3)
            picked.append(pick(r))
        return float(np.median(wall)), float(np.median(picked))

    out = {"what": "assignment to the greedy clusters of 10^5 12-mers, BLOSUM62, X=3, p=0, threshold 20, k=%d" % args.k,
           "n_clusters_all": int((counts > 0).sum()), "n_multi": int(gst.n_multi), "runs": []}
    for candidates in ("all", "skip_singletons"):
        members = np.arange(n) if candidates == "all" else np.nonzero(counts[cid] > 1)[0]
        ids, slot = np.unique(cid[members], return_inverse=True)
        for nq in (10_000, 100):
            seqs = [new_res[new_off[i]:new_off[i + 1]] for i in range(nq)] + [res[off[i]:off[i + 1]] for i in members]
            r2, o2 = hammock_amd.pack_sequences(seqs)
            ctx.set_sequences(residues=r2, offsets=o2)
            nm = len(members)

            def assign():
                ctx.assign_shifted(0, nq, nq, nq + nm, slot, ids, X, P, THR, args.k)
                return ctx.last_assign_stats
            wall, kern = median(assign, lambda s: s.kernel_ms)
            st = ctx.last_assign_stats
            swall, spass = median(lambda: ctx.search_shifted(nq, nq + nm, 0, nq, X, P, THR)[1], lambda s: s.kernel_ms)
            _, _, nf = ctx.assign_shifted(0, nq, nq, nq + nm, slot, ids, X, P, THR, args.k)
            out["runs"].append({"candidates": candidates, "shape": f"{nq}x{nm}", "n_clusters": int(len(ids)), "wall_ms": wall,
                                "kernel_ms": kern, "pass_ms": spass, "agg_sel_ms": kern - spass,
                                "agg_sel_over_pass": (kern - spass) / spass, "search_wall_ms": swall, "wall_over_search": wall / swall,
                                "n_edges": int(st.n_edges), "assigned": int((nf > 0).sum())})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
