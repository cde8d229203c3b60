#!/usr/bin/env python3
"""bench_separation.py -- the separation of given clusters (hmk_cluster_separation_shifted) on one MI355X, beside the call that scores
pairs with the same scorer and staging today.

BLOSUM62, max shift 3, shift penalty 0, a resident context; synthetic 12-mers (hammock_amd.synth).  Workloads (--only picks some):
  a  20,000 12-mers (seed 3) in the clusters hmk_greedy_cluster gives them at threshold 20: 4.0 x 10^8 ordered pairs.  Beside it
     hmk_score_survey_shifted as the rectangle of the set's two halves with the row outputs and no histogram, 10^8 pairs: the literal
     scorer and the staging of the walk, with per-tile atomics in place of the running sums.  The two are compared per pair.  Also
     the same 20,000 as singletons only (every partner closes a slot) and as one slot, and the route a user has without the call:
     hmk_score_block_shifted in blocks of 2,000 rows + the sums per (row, slot) in numpy (wall time, --block-steps rounds).
  b  100,000 12-mers (seed 1) in their greedy clusters: 10^10 ordered pairs.
The routes of a workload alternate in one process, --steps timed rounds after --warmup untimed ones; per route the median, minimum
and maximum of the device time (the calls' kernel_ms, HIP events).  Prints one JSON line per workload.

    python tools/bench_separation.py [--steps 10] [--warmup 3] [--block-steps 2] [--only a,b]
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

from tools.bench_linkage import spread   # noqa: E402

X, P, THR = 3, 0, 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--block-steps", type=int, default=2)
    ap.add_argument("--only", default="a,b")
    args = ap.parse_args()
    only = set(args.only.split(","))
    import hammock_amd
    from hammock_amd.synth import synth_peptides
    with open(os.path.join(ROOT, "tests", "golden", "matrices.json")) as fh:
        M = np.asarray(json.load(fh)["matrices"]["blosum62"], dtype=np.int32)
    ctx = hammock_amd.Context(M, device=0)
    rounds = range(args.warmup + args.steps)

    def greedy_slots(n):
        cid = ctx.greedy_cluster(X, P, THR, int(round(n * 0.025)))[0]   # (the CLI's default cluster limit)
        _, mc = np.unique(cid[:n], return_inverse=True)
        return mc.astype(np.uint32), int(mc.max()) + 1

    def separation(n, mc, ncl):
        out = ctx.cluster_separation_shifted(0, n, mc, ncl, X, P)
        return out, ctx.last_separation_stats

    if "a" in only:
        n, half = 20_000, 10_000
        res, off = synth_peptides(3, n, 12)
        ctx.set_sequences(residues=res, offsets=off)
        mc, ncl = greedy_slots(n)
        forms = {"greedy": (mc, ncl), "singletons": (np.arange(n, dtype=np.uint32), n), "one_slot": (np.zeros(n, dtype=np.uint32), 1)}
        k = {name: [] for name in list(forms) + ["rectangle"]}
        kept = {}
        for step in rounds:
            for name, (slots, count) in forms.items():
                out, st = separation(n, slots, count)
                kept[name] = (out, st.n_misplaced, st.n_segments)
                if step >= args.warmup:
                    k[name].append(st.kernel_ms)
            _, _, rs = ctx.score_survey_shifted(0, half, half, n, X, P, THR)
            if step >= args.warmup:
                k["rectangle"].append(rs.kernel_ms)
        assert rs.pairs_scored == half * half and kept["one_slot"][1] == 0 and not kept["singletons"][0][0].any()
        blocks = []
        order = np.argsort(mc, kind="stable")
        starts = np.r_[0, np.cumsum(np.bincount(mc, minlength=ncl))[:-1]]
        for step in range(args.block_steps):   # what a user does today: every score across the bus, 4 bytes each
            t0 = time.perf_counter()
            own = np.zeros(n, dtype=np.int64)
            for r0 in range(0, n, 2000):
                sc = ctx.score_block_shifted(r0, r0 + 2000, 0, n, X, P).astype(np.int64)
                sc[np.arange(2000), np.arange(r0, r0 + 2000)] = 0
                sums = np.add.reduceat(sc[:, order], starts, axis=1)
                own[r0:r0 + 2000] = sums[np.arange(2000), mc[r0:r0 + 2000]]
            blocks.append((time.perf_counter() - t0) * 1e3)
            assert np.array_equal(own, kept["greedy"][0][0])
        pairs, rect_pairs = n * (n - 1), half * half
        per = {"greedy": spread(np.asarray(k["greedy"]) / pairs * 1e9), "rectangle": spread(np.asarray(k["rectangle"]) / rect_pairs * 1e9)}
        slack = (per["greedy"]["max"] - per["greedy"]["min"]) + (per["rectangle"]["max"] - per["rectangle"]["min"])
        print(json.dumps({"workload": "a: 20,000 12-mers in their greedy clusters", "ordered_pairs": pairs, "clusters": ncl,
                          "largest_cluster": int(np.bincount(mc).max()), "misplaced": int(kept["greedy"][1]), "segments": int(kept["greedy"][2]),
                          "steps": args.steps, "warmup": args.warmup,
                          "separation_kernel_ms": spread(k["greedy"]), "separation_kernel_ms_singletons": spread(k["singletons"]),
                          "separation_kernel_ms_one_slot": spread(k["one_slot"]), "rectangle_pairs": rect_pairs,
                          "rectangle_survey_kernel_ms": spread(k["rectangle"]),
                          "separation_ps_per_pair": per["greedy"], "rectangle_ps_per_pair": per["rectangle"],
                          "wanted_separation_at_most_ps_per_pair": per["rectangle"]["median"] + slack,
                          "wanted_met": bool(per["greedy"]["median"] <= per["rectangle"]["median"] + slack),
                          "per_pair_ratio_separation_over_rectangle": per["greedy"]["median"] / per["rectangle"]["median"],
                          "score_block_and_numpy_wall_ms": spread(blocks), "score_block_steps": args.block_steps,
                          "separation_pairs_per_s": pairs / (float(np.median(k["greedy"])) * 1e-3)}), flush=True)

    if "b" in only:
        n = 100_000
        res, off = synth_peptides(1, n, 12)
        ctx.set_sequences(residues=res, offsets=off)
        mc, ncl = greedy_slots(n)
        ks = []
        for step in rounds:
            _, st = separation(n, mc, ncl)
            if step >= args.warmup:
                ks.append(st.kernel_ms)
        print(json.dumps({"workload": "b: 100,000 12-mers in their greedy clusters", "ordered_pairs": n * (n - 1), "clusters": ncl,
                          "largest_cluster": int(np.bincount(mc).max()), "misplaced": int(st.n_misplaced), "segments": int(st.n_segments),
                          "steps": args.steps, "warmup": args.warmup, "separation_kernel_ms": spread(ks),
                          "separation_pairs_per_s": n * (n - 1) / (float(np.median(ks)) * 1e-3)}), flush=True)


if __name__ == "__main__":
    main()
