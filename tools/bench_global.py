#!/usr/bin/env python3
"""hmk_neighbors_global against hmk_neighbors_local, alternating in one process, on the 10^5 mixed 7..20-mers of BASELINE config 4b
and on 10^5 12-mers: BLOSUM62, open -5, extend -1.  The local pass scores all ordered pairs at threshold 28; the global pass scores
every unordered pair once at the threshold whose hit share (from a sample of pair scores) is nearest the local pass's.  Device time
by HIP events (stats.kernel_ms), DP cells per second (cells = the sum of la x lb over the scored pairs), and the register tiles
against the literal tiles on the same set: 20 x BLOSUM62 with penalties and threshold x 20 has an entry above 127, so the same
pairs with the same hits run through global_score_literal.  Product path only, no oracle.  One JSON line on stdout."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hammock_amd
from hammock_amd.synth import synth_peptides
from bench import load_blosum62

# VALU instructions per DP cell of k_neighbors_global's column step, counted from the gfx950 ISA: a column of a
# four-line strip is 34-36 v_ instructions
GLOBAL_VALU_PER_CELL = 8.75
OPEN, EXTEND, LOCAL_THR = -5, -1, 28


def cells_of(off, ordered):
    lens = np.diff(off.astype(np.int64)).astype(np.float64)
    both = float(lens.sum()) ** 2 - float((lens * lens).sum())   # ordered pairs i != j of len_i x len_j
    return both if ordered else both / 2


def threshold_for_share(ctx, n, share, rng):
    i = rng.integers(0, n, size=400000)
    j = rng.integers(0, n, size=400000)
    keep = i != j
    s = np.sort(ctx.score_pairs_global(i[keep], j[keep], OPEN, EXTEND))
    return int(s[min(len(s) - 1, int(round(len(s) * (1.0 - share))))])


def run_set(name, res, off, M, reps, warm, literal_reps):
    n = len(off) - 1
    ctx = hammock_amd.Context(M, device=0)
    ctx.set_sequences(residues=res, offsets=off)
    edges, st = ctx.neighbors_local(OPEN, EXTEND, LOCAL_THR, capacity=1 << 26)
    local_share = len(edges) / float(st.pairs_scored)
    thr = threshold_for_share(ctx, n, local_share, np.random.default_rng(1))
    ms = {"global": [], "local": []}
    info = {}
    for r in range(warm + reps):   # alternating
        for which in ("global", "local"):
            if which == "global":
                edges, st = ctx.neighbors_global(OPEN, EXTEND, thr, capacity=1 << 26)
            else:
                edges, st = ctx.neighbors_local(OPEN, EXTEND, LOCAL_THR, capacity=1 << 26)
            if r >= warm:
                ms[which].append(float(st.kernel_ms))
            info[which] = {"pairs": int(st.pairs_scored), "edges": int(len(edges)), "share": len(edges) / float(st.pairs_scored)}
    ctx.close()
    out = {"set": name, "n": n, "global_threshold": thr, "local_threshold": LOCAL_THR}
    for which, ordered in (("global", False), ("local", True)):
        med = float(np.median(ms[which]))
        cells = cells_of(off, ordered)
        out[which] = dict(info[which], kernel_ms=med, kernel_ms_all=ms[which], dp_cells=cells, dp_cells_per_s=cells / (med * 1e-3))
    g = out["global"]
    g["valu_per_cell_isa"] = GLOBAL_VALU_PER_CELL
    g["valu_issue_frac"] = g["dp_cells"] * GLOBAL_VALU_PER_CELL / (g["kernel_ms"] * 1e-3) / (256 * 4 * 16 * 2.4e9)
    out["global_over_local_ms"] = g["kernel_ms"] / out["local"]["kernel_ms"]
    if literal_reps:
        ctx = hammock_amd.Context(M * 20, device=0)
        ctx.set_sequences(residues=res, offsets=off)
        lit = []
        for r in range(1 + literal_reps):
            edges, st = ctx.neighbors_global(OPEN * 20, EXTEND * 20, thr * 20, capacity=1 << 26)
            if r >= 1:
                lit.append(float(st.kernel_ms))
        ctx.close()
        out["global_literal"] = {"kernel_ms": float(np.median(lit)), "kernel_ms_all": lit, "edges": int(len(edges)),
                                 "same_hits_as_register": int(len(edges)) == g["edges"]}
        out["literal_over_register_ms"] = out["global_literal"]["kernel_ms"] / g["kernel_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--literal_reps", type=int, default=1, help="0: skip the literal tiles")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()
    M = load_blosum62()
    results = []
    for name, lo, hi in (("1e5 x 7..20 (config 4b)", 7, 20), ("1e5 x 12", 12, 12)):
        res, off = synth_peptides(1, a.n, lo, hi)
        results.append(run_set(name.replace("1e5", str(a.n)) if a.n != 100000 else name, res, off, M, a.reps, a.warm, a.literal_reps))
    line = json.dumps({"bench": "neighbors_global vs neighbors_local", "open": OPEN, "extend": EXTEND, "results": results})
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
