#!/usr/bin/env python3
"""bench_search.py -- query-vs-reference search (hmk_search_shifted / hmk_search_best_shifted) on one MI355X.

Synthetic 12-mers (SplitMix64, hammock_amd.synth), BLOSUM62, max shift 3, shift penalty 0, threshold 20; queries first,
references behind them in one uploaded set.  Four runs: 10^4 x 10^5, 10^2 x 10^5, 10^5 x 10^2 (threshold output) and the
best-k call (k = 5) on the first shape.  Kernel time is stats.kernel_ms (HIP events around the scoring launches; the best-k
call adds its selection kernels), median of --steps calls after --warmup untimed ones.  frac_lds_ideal uses bench.py's
roofline: 72 LDS bytes per pair (one per cell ShiftedScorer.java:67-77 adds at length 12, max shift 3) at 256 B/clk/CU x
256 CUs x 2.4 GHz.  Prints one JSON line.

    python tools/bench_search.py [--steps 10] [--warmup 3]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LDS_PEAK_GBS = 256 * 256 * 2.4   # bench.py
LDS_BYTES_PER_PAIR = 72          # bench.py: 12 * (0 + 1) + 2 * 3 * 12 - 3 * 4
X, P, THR, K = 3, 0, 20, 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import hammock_amd
    from hammock_amd.synth import synth_peptides
    with open(os.path.join(ROOT, "tests", "golden", "matrices.json")) as fh:
        M = np.asarray(json.load(fh)["matrices"]["blosum62"], dtype=np.int32)
    res, off = synth_peptides(1, 110_000, 12)
    ctx = hammock_amd.Context(M, device=0)

    def upload(n):
        ctx.set_sequences(residues=res[:int(off[n])], offsets=off[:n + 1])

    def measure(call):
        for _ in range(args.warmup):
            call()
        ms, last = [], None
        for _ in range(args.steps):
            last = call()
            ms.append(float(last.kernel_ms))
        return float(np.median(ms)), last

    out = {"what": "query-vs-reference search, 12-mers, BLOSUM62, X=3, p=0, threshold 20", "runs": []}
    for nq, nr in ((10_000, 100_000), (100, 100_000), (100_000, 100)):
        upload(nq + nr)
        med, st = measure(lambda: ctx.search_shifted(0, nq, nq, nq + nr, X, P, THR)[1])
        ideal = nq * nr * LDS_BYTES_PER_PAIR / (LDS_PEAK_GBS * 1e9) * 1e3
        out["runs"].append({"shape": f"{nq}x{nr}", "call": "search_shifted", "kernel_ms": med, "pairs_per_s": nq * nr / (med * 1e-3),
                            "frac_lds_ideal": ideal / med, "lds_ideal_ms": ideal, "n_edges": int(st.n_edges), "n_tiles": int(st.n_tiles),
                            "classes_rows": int(st.classes_rows)})
        if nq == 10_000:
            base = med

            def best():
                ctx.search_best_shifted(0, nq, nq, nq + nr, X, P, THR, K)
                return ctx.last_search_stats
            bmed, bst = measure(best)
            out["runs"].append({"shape": f"{nq}x{nr}", "call": f"search_best_shifted k={K}", "kernel_ms": bmed,
                                "pairs_per_s": nq * nr / (bmed * 1e-3), "frac_lds_ideal": ideal / bmed, "n_hits_above_threshold": int(bst.n_edges),
                                "added_over_threshold_pass": bmed / base - 1.0})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
