#!/usr/bin/env python3
"""bench_orders.py -- the greedy clusterings under many orders of the set from one scoring pass (hmk_greedy_orders) on one MI355X,
beside the only other route to them: per order one set_sequences of the permuted set and one hmk_greedy_cluster on a resident context,
each of which uploads the set and scores the pair space again (the upload is in the figure: that route cannot avoid it).

BLOSUM62, max shift 3, shift penalty 0, threshold 20, the cluster limit round(0.025 n) (Hammock.java:398-401), 16 orders: the identity
and 15 random permutations (numpy, seeds 1 ... 15).  Workloads (--only picks some), all 12-mers:
  a   bench.py's 10^5 synthetic 12-mers (seed 1)
  b   the antibodies example (tests/golden/antibodies.fa.gz, its 74,041 distinct 12-mers)
  d   10^6 synthetic 12-mers (seed 1); the old route in --old-steps-d rounds only
The two routes alternate in one process, --steps timed rounds after --warmup untimed ones; in every round that runs both, every
order's ids, list order and member ranks of the two routes are asserted identical after mapping the old route's rows back to uploaded
indices (an order where the reference would throw: the same case and index).  Per workload the median, minimum and maximum of both
routes' wall time, of the new route's kernel_ms (the one pass), relabel_ms (all k_orders_relabel launches), support_ms (k_orders_support
and the consensus kernels) and the sum of its orders' tail_ms (relabel + tail, wall), and of the old route's summed neighbors_ms.
Prints one JSON line per workload; --out FILE keeps them under "workloads" of the JSON object in FILE.

    python tools/bench_orders.py [--steps 10] [--warmup 2] [--old-steps-d 3] [--no-old] [--only a,b,d] [--out profiles/greedy_orders_bench.json]
"""
import argparse
import gzip
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

X, P, THR, N_ORDERS = 3, 0, 20, 16


def spread(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--old-steps-d", type=int, default=3)
    ap.add_argument("--no-old", action="store_true", help="the orders call alone (a kernel trace of it)")
    ap.add_argument("--only", default="a,b,d")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    only = set(args.only.split(","))
    import hammock_amd
    from hammock_amd.synth import synth_peptides
    with open(os.path.join(ROOT, "tests", "golden", "matrices.json")) as fh:
        M = np.asarray(json.load(fh)["matrices"]["blosum62"], dtype=np.int32)

    def antibodies():
        with gzip.open(os.path.join(ROOT, "tests", "golden", "antibodies.fa.gz"), "rt") as fh:
            seqs = list(dict.fromkeys(line.strip() for line in fh if line.strip() and not line.startswith(">")))
        return hammock_amd.pack_sequences(seqs)

    workloads = [("a", lambda: synth_peptides(1, 100_000, 12)), ("b", antibodies), ("d", lambda: synth_peptides(1, 1_000_000, 12))]
    results = []
    for name, make in workloads:
        if name not in only:
            continue
        res, off = make()
        n = len(off) - 1
        assert res.size == 12 * n
        maxc = int(np.floor(n * 0.025 + 0.5))
        orders = np.stack([np.arange(n)] + [np.random.default_rng(s).permutation(n) for s in range(1, N_ORDERS)]).astype(np.uint32)
        permuted = [np.ascontiguousarray(res.reshape(n, 12)[o].reshape(-1)) for o in orders]
        ctx = hammock_amd.Context(M, device=0)
        ctx.set_sequences(residues=res, offsets=off)
        new = {"wall_ms": [], "kernel_ms": [], "relabel_ms": [], "support_ms": [], "tails_ms": []}
        old = {"wall_ms": [], "neighbors_ms": []}
        old_steps = 0 if args.no_old else min(args.steps, args.old_steps_d) if name == "d" else args.steps
        warmup = args.warmup
        old_from = max(warmup - 1, 0) if name == "d" else 0   # (d: one untimed round of the old route at the most)
        old_to = warmup + old_steps if old_steps else 0
        r = None
        for step in range(warmup + args.steps):
            t0 = time.perf_counter()
            r = ctx.greedy_orders(X, P, THR, maxc, orders, support=False)
            wall = (time.perf_counter() - t0) * 1e3
            s = r.stats
            if step >= warmup:
                new["wall_ms"].append(wall)
                new["kernel_ms"].append(s.kernel_ms)
                new["relabel_ms"].append(s.relabel_ms)
                new["support_ms"].append(s.support_ms)
                new["tails_ms"].append(float(r.per_order["tail_ms"].sum()))
            if not old_from <= step < old_to:
                continue
            t0 = time.perf_counter()
            got, nbr = [], 0.0
            for k in range(N_ORDERS):
                ctx.set_sequences(residues=permuted[k], offsets=off)
                try:
                    c, o, st = ctx.greedy_cluster(X, P, THR, maxc)
                    got.append((c.copy(), o.copy(), ctx.member_rank[:n].copy(), None))
                    nbr += st.neighbors_ms
                except hammock_amd.ReferenceWouldCrash as e:
                    got.append((None, None, None, (e.case, e.index)))
            wall = (time.perf_counter() - t0) * 1e3
            ctx.set_sequences(residues=res, offsets=off)   # (outside the figure: the new route's set is resident)
            for k, (c, o, rank, crash) in enumerate(got):   # identical rows in every order in every round
                po, perm = r.per_order[k], orders[k]
                if crash:
                    assert (int(po["crash_case"]), int(po["crash_index"])) == crash and po["status"] != 0, (name, k)
                    continue
                ids, rk = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
                ids[perm] = perm[c]
                rk[perm] = rank
                assert po["status"] == 0 and np.array_equal(r.cluster_id[k], ids) and np.array_equal(r.member_rank[k], rk), (name, k)
                assert np.array_equal(r.result_order[k, :o.size], perm[o]) and po["n_result_clusters"] == o.size, (name, k)
            if step >= warmup:
                old["wall_ms"].append(wall)
                old["neighbors_ms"].append(nbr)
        s = r.stats
        row = {"workload": name, "n": n, "max_shift": X, "threshold": THR, "max_clusters": maxc, "n_orders": N_ORDERS, "n_valid": int(s.n_valid),
               "n_edges": int(s.n_edges), "steps": args.steps, "warmup": warmup, "old_steps": len(old["wall_ms"]),
               "new": {k: spread(v) for k, v in new.items()}, "old": {k: spread(v) for k, v in old.items() if v},
               "pairs_ever": int(s.pairs_ever), "pairs_always": int(s.pairs_always), "n_consensus": int(s.n_consensus),
               "pairs_together_by_order": [int(v) for v in r.per_order["pairs_together"]],
               "clusters_by_order": [int(v) for v in r.per_order["n_result_clusters"]], "status_by_order": [int(v) for v in r.per_order["status"]],
               "tail_ms_by_order": [round(float(v), 3) for v in r.per_order["tail_ms"]]}
        if old["wall_ms"]:
            row["speedup_median"] = row["old"]["wall_ms"]["median"] / row["new"]["wall_ms"]["median"]
        results.append(row)
        print(json.dumps(row), flush=True)
        del ctx
    if args.out:
        doc = {}
        if os.path.exists(args.out):
            with open(args.out) as fh:
                doc = json.load(fh)
        kept = [r for r in doc.get("workloads", []) if r["workload"] not in {r["workload"] for r in results}]
        names = [w[0] for w in workloads]
        doc["workloads"] = sorted(kept + results, key=lambda r: names.index(r["workload"]))
        with open(args.out, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
