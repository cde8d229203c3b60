#!/usr/bin/env python3
"""bench_match.py -- match of query clusters to existing clusters (hmk_match_clusters_shifted) on one MI355X.

BLOSUM62, max shift 3, shift penalty 0, threshold 20, greedy clusterings with the CLI's default limit of round(0.025 n) initial
clusters (hmk_greedy_cluster).  Three workloads:
  (a) the greedy clusters of 10^4 synthetic 12-mers of seed 2 against every greedy cluster of bench.py's 10^5 set (seed 1);
  (b) the same queries against the multi-member clusters of that set only (the CLI's --skip_singletons);
  (c) the multi-member clusters of a 10^5 seed-2 greedy against the multi-member clusters of the 10^6 seed-1 greedy.
Queries first, members behind them, in one uploaded set.  Per workload:
  wall_ms          the match_clusters_shifted call as Python sees it (host checks, uploads, pass, both levels, copies)
  kernel_ms        stats.kernel_ms of the call: the pass + level 1 + level 2 (HIP events)
  assign_wall_ms   assign_shifted on the same members and query sequences, every query sequence on its own (a and b)
  pass_ms          stats.kernel_ms of hmk_search_shifted on the same rectangle with the members as queries -- the pass alone
  agg_ms           kernel_ms - pass_ms: both aggregation levels and the selection
Medians of --steps calls after --warmup untimed ones; k = 1 (the CLI's default --best).  Prints one JSON line.  The split of
agg_ms into level 1 (k_assign_count / k_assign_scatter / k_match_feasible_*) and level 2 (k_match_count / k_match_copy /
k_match_select_*) comes from a `rocprofv3 --kernel-trace --stats` run of this tool.

    python tools/bench_match.py [--steps 10] [--warmup 3] [--k 1] [--skip-c]
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
    ap.add_argument("--skip-c", action="store_true", help="leave out workload (c) (its 10^6 greedy)")
    args = ap.parse_args()
    import hammock_amd
    from hammock_amd.synth import synth_peptides
    with open(os.path.join(ROOT, "tests", "golden", "matrices.json")) as fh:
        M = np.asarray(json.load(fh)["matrices"]["blosum62"], dtype=np.int32)
    ctx = hammock_amd.Context(M, device=0)

    def greedy(seed, n):
        res, off = synth_peptides(seed, n, 12)
        ctx.set_sequences(residues=res, offsets=off)
        cid, _, _ = ctx.greedy_cluster(X, P, THR, int(round(n * 0.025)))
        return res, off, cid

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

    def seqs_of(res, off, idx):
        return [res[off[i]:off[i + 1]] for i in idx]

    out = {"what": "match of greedy clusters, BLOSUM62, X=3, p=0, threshold 20, k=%d" % args.k, "runs": []}

    def run(name, q, qcid, m, mcid, with_assign):
        (qres, qoff, qidx), (mres, moff, midx) = q, m
        _, qc = np.unique(qcid[qidx], return_inverse=True)
        ids, slot = np.unique(mcid[midx], return_inverse=True)
        nq, nm = len(qidx), len(midx)
        r2, o2 = hammock_amd.pack_sequences(seqs_of(qres, qoff, qidx) + seqs_of(mres, moff, midx))
        ctx.set_sequences(residues=r2, offsets=o2)

        def match():
            ctx.match_clusters_shifted(0, nq, qc, nq, nq + nm, slot, ids, X, P, THR, args.k)
            return ctx.last_match_stats
        wall, kern = median(match, lambda s: s.kernel_ms)
        st = ctx.last_match_stats
        _, spass = median(lambda: ctx.search_shifted(nq, nq + nm, 0, nq, X, P, THR)[1], lambda s: s.kernel_ms)
        _, _, nf = ctx.match_clusters_shifted(0, nq, qc, nq, nq + nm, slot, ids, X, P, THR, args.k)
        row = {"workload": name, "query_clusters": int(qc.max()) + 1, "query_sequences": nq, "n_clusters": int(len(ids)), "members": nm,
               "wall_ms": wall, "kernel_ms": kern, "pass_ms": spass, "agg_ms": kern - spass, "n_edges": int(st.n_edges),
               "matched": int((nf > 0).sum())}
        if with_assign:
            awall, _ = median(lambda: ctx.assign_shifted(0, nq, nq, nq + nm, slot, ids, X, P, THR, args.k), lambda r: 0.0)
            row.update({"assign_wall_ms": awall, "wall_over_assign": wall / awall})
        out["runs"].append(row)

    n = 100_000
    res1, off1, cid1 = greedy(1, n)
    counts1 = np.bincount(cid1, minlength=n)
    res2, off2, cid2 = greedy(2, 10_000)
    q = (res2, off2, np.arange(10_000))
    run("a: 1e4 seed-2 clusters x all 1e5 clusters", q, cid2, (res1, off1, np.arange(n)), cid1, True)
    run("b: 1e4 seed-2 clusters x multi-member 1e5 clusters", q, cid2, (res1, off1, np.nonzero(counts1[cid1] > 1)[0]), cid1, True)
    if not args.skip_c:
        res3, off3, cid3 = greedy(2, n)
        counts3 = np.bincount(cid3, minlength=n)
        big = 1_000_000
        res4, off4, cid4 = greedy(1, big)
        counts4 = np.bincount(cid4, minlength=big)
        run("c: multi-member 1e5 seed-2 clusters x multi-member 1e6 clusters", (res3, off3, np.nonzero(counts3[cid3] > 1)[0]), cid3,
            (res4, off4, np.nonzero(counts4[cid4] > 1)[0]), cid4, False)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
