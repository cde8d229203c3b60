#!/usr/bin/env python3
"""bench_sweep.py -- the greedy clusterings at a range of thresholds from one scoring pass (hmk_greedy_sweep) on one MI355X, beside the
only other route to them: one hmk_greedy_cluster call per threshold on the same context, each of which scores the pair space again.

BLOSUM62, shift penalty 0, the cluster limit round(0.025 n) (Hammock.java:398-401), a resident context.  Workloads (--only picks some):
  a   bench.py's 10^5 synthetic 12-mers (seed 1), max shift 3, thresholds 20 ... 40
  b   the antibodies example (tests/golden/antibodies.fa.gz, its 74,041 distinct 12-mers), max shift 3, thresholds 20 ... 40
  c   10^5 synthetic peptides of length 7 ... 20 (seed 1), max shift and first threshold by Hammock's defaults (round(mean / 4) cut to
      the shortest length - 1, round(1.7 x mean)), 11 levels
  d   10^6 synthetic 12-mers (seed 1), max shift 3, thresholds 20 ... 30; the old route in --old-steps-d rounds only (default 1)
The two routes alternate in one process, --steps timed rounds after --warmup untimed ones; in every round that runs both, every
level's ids, list order and member ranks of the two routes are asserted identical (a level where the reference would throw: the same
case and index).  Per workload the median, minimum and maximum of both routes' wall time, of the sweep's kernel_ms (the one pass),
deal_ms (the three k_sweep kernels) and the sum of its levels' tail_ms, and of the old route's summed neighbors_ms.  Bytes over PCIe
are counted, not measured: the sweep adds one copy of 2,056 bytes (prefix[] and the flag) to what its tails move; a tail moves what
the same threshold's hmk_greedy_cluster call moves behind its pass, less the band hand-over, which the sweep's tails do not use.
Prints one JSON line per workload; --out FILE keeps them under "workloads" of the JSON object in FILE, replacing the rows of the same
name and leaving the file's other sections as they are.

    python tools/bench_sweep.py [--steps 5] [--warmup 2] [--old-steps-d 1] [--no-old] [--only a,b,c,d] [--out profiles/greedy_sweep_bench.json]
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

P = 0


def spread(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def java_round(v):
    return int(np.floor(v + 0.5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--old-steps-d", type=int, default=1)
    ap.add_argument("--no-old", action="store_true", help="the sweep alone (a kernel trace of it)")
    ap.add_argument("--only", default="a,b,c,d")
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

    workloads = [("a", lambda: synth_peptides(1, 100_000, 12), 3, 20, 40), ("b", antibodies, 3, 20, 40),
                 ("c", lambda: synth_peptides(1, 100_000, 7, 20), None, None, None), ("d", lambda: synth_peptides(1, 1_000_000, 12), 3, 20, 30)]
    results = []
    for name, make, X, thr, hi in workloads:
        if name not in only:
            continue
        res, off = make()
        n = len(off) - 1
        lengths = np.diff(off.astype(np.int64))
        if X is None:   # Hammock's defaults (Hammock.java:394-397, :803-811, :1421-1427)
            X = min(java_round(lengths.mean() / 4), int(lengths.min()) - 1)
            thr = java_round(lengths.mean() * 1.7)
            hi = thr + 10
        maxc = java_round(n * 0.025)
        ctx = hammock_amd.Context(M, device=0)
        ctx.set_sequences(residues=res, offsets=off)
        new = {"wall_ms": [], "kernel_ms": [], "deal_ms": [], "tails_ms": []}
        old = {"wall_ms": [], "neighbors_ms": []}
        old_steps = 0 if args.no_old else min(args.steps, args.old_steps_d) if name == "d" else args.steps
        warmup = args.warmup
        old_from = max(warmup - 1, 0) if name == "d" else 0   # (d: one untimed round of the old route at the most)
        old_to = warmup + old_steps if old_steps else 0
        levels = None
        for step in range(warmup + args.steps):
            t0 = time.perf_counter()
            levels, cid, order, rank = ctx.greedy_sweep(X, P, thr, hi, maxc)
            wall = (time.perf_counter() - t0) * 1e3
            s = ctx.last_sweep_stats
            if step >= warmup:
                new["wall_ms"].append(wall)
                new["kernel_ms"].append(s.kernel_ms)
                new["deal_ms"].append(s.deal_ms)
                new["tails_ms"].append(float(levels["tail_ms"].sum()))
            if not old_from <= step < old_to:
                continue
            t0 = time.perf_counter()
            got, nbr = [], 0.0
            for t in range(thr, hi + 1):
                try:
                    c, o, st = ctx.greedy_cluster(X, P, t, maxc)
                    got.append((c.copy(), o.copy(), ctx.member_rank[:n].copy(), None))
                    nbr += st.neighbors_ms
                except hammock_amd.ReferenceWouldCrash as e:
                    got.append((None, None, None, (e.case, e.index)))
            wall = (time.perf_counter() - t0) * 1e3
            for l, (c, o, r, crash) in enumerate(got):   # identical ids at every level in every round
                if crash:
                    assert (int(levels["crash_case"][l]), int(levels["crash_index"][l])) == crash and levels["status"][l] != 0, (name, l)
                    continue
                assert levels["status"][l] == 0 and np.array_equal(cid[l], c) and np.array_equal(rank[l], r), (name, l)
                assert np.array_equal(order[l, :o.size], o) and levels["n_result_clusters"][l] == o.size, (name, l)
            if step >= warmup:
                old["wall_ms"].append(wall)
                old["neighbors_ms"].append(nbr)
        row = {"workload": name, "n": n, "max_shift": X, "threshold": thr, "threshold_hi": hi, "max_clusters": maxc, "n_edges": int(levels["n_edges"][0]),
               "steps": args.steps, "warmup": warmup, "old_steps": len(old["wall_ms"]),
               "new": {k: spread(v) for k, v in new.items()}, "old": {k: spread(v) for k, v in old.items() if v},
               "sweep_extra_pcie_bytes": 2056,
               "edges_by_threshold": [int(v) for v in levels["n_edges"]], "clusters_by_threshold": [int(v) for v in levels["n_result_clusters"]],
               "status_by_threshold": [int(v) for v in levels["status"]], "tail_ms_by_threshold": [round(float(v), 3) for v in levels["tail_ms"]]}
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
