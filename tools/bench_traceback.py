#!/usr/bin/env python3
"""hmk_align_pairs_global against hmk_score_pairs_global over the same pairs, alternating in one process: the edge lists of
hmk_neighbors_global on 10^5 12-mers at threshold 18 and on the 10^5 mixed 7..20-mers of BASELINE config 4b at threshold 16
(BLOSUM62, open -5, extend -1; the sets and thresholds of tools/bench_global.py), each list traced back in full with seq1 = the
edge's m, seq2 = its x.  The yardstick is the same DP without the direction bits and the walk (k_pairs<2>).  Device time by HIP
events (hmk_last_kernel_ms, summed over the chunks of 2^24 pairs), medians of `reps` after `warm` with min and max; pairs per
second; the wall time of the Python call, which includes the uploads of the index lists and the 21 bytes per pair that come back
(4 for the scorer).  Product path only, no oracle.  One JSON line on stdout."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hammock_amd
from hammock_amd.synth import synth_peptides
from bench import load_blosum62

OPEN, EXTEND = -5, -1


def summary(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "all": [float(x) for x in v]}


def run_set(name, res, off, M, thr, reps, warm):
    ctx = hammock_amd.Context(M, device=0)
    ctx.set_sequences(residues=res, offsets=off)
    edges, st = ctx.neighbors_global(OPEN, EXTEND, thr, capacity=1 << 26)
    x, m, s = hammock_amd.edge_fields(edges)
    lens = np.diff(off.astype(np.int64))
    cells = float((lens[m] * lens[x]).sum())
    ms = {"align": [], "score": []}
    wall = {"align": [], "score": []}
    for r in range(warm + reps):   # alternating
        for which in ("align", "score"):
            t0 = time.perf_counter()
            if which == "align":
                score, n_cols, gap1, gap2 = ctx.align_pairs_global(m, x, OPEN, EXTEND)
            else:
                score = ctx.score_pairs_global(m, x, OPEN, EXTEND)
            t1 = time.perf_counter()
            if not np.array_equal(score, s):
                raise SystemExit(f"{name}: {which} scores differ from the edges'")
            if r >= warm:
                ms[which].append(ctx.last_kernel_ms())
                wall[which].append((t1 - t0) * 1e3)
    gapped = int(np.count_nonzero(gap1 | gap2))
    ctx.close()
    out = {"set": name, "n": len(off) - 1, "threshold": thr, "pairs": int(len(edges)), "neighbors_kernel_ms": float(st.kernel_ms),
           "dp_cells": cells, "pairs_with_a_gap": gapped, "mean_columns": float(n_cols.mean())}
    for which in ("align", "score"):
        k = summary(ms[which])
        out[which] = {"kernel_ms": k, "wall_ms": summary(wall[which]), "pairs_per_s": len(edges) / (k["median"] * 1e-3),
                      "dp_cells_per_s": cells / (k["median"] * 1e-3)}
    out["align_over_score_kernel_ms"] = out["align"]["kernel_ms"]["median"] / out["score"]["kernel_ms"]["median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()
    M = load_blosum62()
    results = []
    for name, lo, hi, thr in (("1e5 x 12", 12, 12, 18), ("1e5 x 7..20 (config 4b)", 7, 20, 16)):
        res, off = synth_peptides(1, a.n, lo, hi)
        results.append(run_set(name.replace("1e5", str(a.n)) if a.n != 100000 else name, res, off, M, thr, a.reps, a.warm))
    doc = {"bench": "align_pairs_global vs score_pairs_global", "open": OPEN, "extend": EXTEND, "results": results}
    line = json.dumps(doc)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
