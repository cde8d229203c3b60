#!/usr/bin/env python3
"""bench_align.py -- centre-star alignment of given clusters (hmk_cluster_align_shifted) on one MI355X, beside (i) its yardstick,
hmk_cluster_linkage_shifted on the same slots -- the same pairs through the same scorer -- and (ii) the only other route to the same
numbers: hmk_score_pairs_shifted over the enumerated pairs inside every cluster, a numpy reduction to the members' sums and the
slots' medoids, then hmk_score_with_shift of every member against its medoid.

BLOSUM62, max shift 3, shift penalty 0 (linkage: threshold 20), a resident context.  Workloads (--only picks some) are those of
tools/bench_linkage.py:
  a  the multi-member clusters of the greedy (limit round(0.025 n)) on bench.py's 10^5 synthetic 12-mers (seed 1)
  b  the clinkage clusters of MUSI (tests/golden/musi.fa), singletons included
  c  10^4 slots of 10 members (10^5 synthetic 12-mers, seed 2, members dealt at random)
  d  one slot of 20,000 synthetic 12-mers (seed 3): 2 x 10^8 pairs through the tiled kernel
The three routes alternate in one process, --steps timed rounds after --warmup untimed ones; per route the median, minimum and
maximum of the device time (align: hmk_align_stats.kernel_ms with and without the sums' copy; linkage: hmk_linkage_stats.kernel_ms
with and without the per-member outputs; (ii): hmk_last_kernel_ms of its two calls added) and of the wall time (the pair list of
(ii) is enumerated once, outside the timing, which favours (ii)).  Prints one JSON line per workload.

    python tools/bench_align.py [--steps 10] [--warmup 3] [--only a,b,c,d]
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

from tools.bench_linkage import inside_pairs, spread   # noqa: E402

X, P, THR = 3, 0, 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="a,b,c,d")
    args = ap.parse_args()
    only = set(args.only.split(","))
    import hammock_amd
    from hammock_amd.synth import synth_peptides
    with open(os.path.join(ROOT, "tests", "golden", "matrices.json")) as fh:
        M = np.asarray(json.load(fh)["matrices"]["blosum62"], dtype=np.int32)
    ctx = hammock_amd.Context(M, device=0)

    def run(name, n, mc):
        """the uploaded set's members [0, n) in slots mc: the three routes, alternating"""
        mc = np.asarray(mc, dtype=np.int64)
        ncl = int(mc.max()) + 1
        a, b, first, slots = inside_pairs(mc)
        order = np.argsort(mc, kind="stable")   # members by slot, ascending inside a slot
        starts = np.concatenate([[0], np.cumsum(np.bincount(mc, minlength=ncl))])[:-1]
        al_k, al_w, bare_k, li_k, li_w, li_bare_k, old_k, old_w = [], [], [], [], [], [], [], []
        for step in range(args.warmup + args.steps):
            t0 = time.perf_counter()
            sc = ctx.score_pairs_shifted(b, a, X, P)   # seq1 = the larger index
            k_old = ctx.last_kernel_ms()
            sums = np.bincount(a, weights=sc, minlength=n) + np.bincount(b, weights=sc, minlength=n)   # (exact: |sum| < 2^53)
            by_slot = sums[order]
            best = np.maximum.reduceat(by_slot, starts)
            is_best = by_slot == np.repeat(best, np.diff(np.concatenate([starts, [n]])))
            centre = np.full(ncl, n, dtype=np.int64)
            np.minimum.at(centre, mc[order][is_best], order[is_best])   # among equal sums the smallest index
            others = np.flatnonzero(centre[mc] != np.arange(n))
            old_score, old_shift = ctx.score_with_shift(centre[mc][others], others, X, P)
            k_old += ctx.last_kernel_ms()
            t1 = time.perf_counter()
            got = ctx.cluster_align_shifted(0, n, mc, ncl, X, P)
            t2 = time.perf_counter()
            st = ctx.last_align_stats
            k_al, pairs, launches, widest = st.kernel_ms, int(st.pairs_scored), int(st.launches), int(st.max_width)
            ctx.cluster_align_shifted(0, n, mc, ncl, X, P, sums=False)
            k_bare = ctx.last_align_stats.kernel_ms
            t3 = time.perf_counter()
            ctx.cluster_linkage_shifted(0, n, mc, ncl, X, P, THR)
            t4 = time.perf_counter()
            k_li = ctx.last_linkage_stats.kernel_ms
            ctx.cluster_linkage_shifted(0, n, mc, ncl, X, P, THR, members=False)
            k_li_bare = ctx.last_linkage_stats.kernel_ms
            if step == 0:   # the routes say the same
                assert np.array_equal(got[3], sums.astype(np.int64)) and np.array_equal(got[0].astype(np.int64), centre)
                assert np.array_equal(got[4][others], old_score) and np.array_equal(got[5][others], old_shift)
                assert pairs == a.size + others.size
            if step >= args.warmup:
                old_w.append((t1 - t0) * 1e3)
                old_k.append(k_old)
                al_w.append((t2 - t1) * 1e3)
                al_k.append(k_al)
                bare_k.append(k_bare)
                li_w.append((t4 - t3) * 1e3)
                li_k.append(k_li)
                li_bare_k.append(k_li_bare)
        return {"workload": name, "slots": ncl, "multi_member_slots": int(slots.size), "members": int(n), "inside_pairs": int(a.size),
                "pairs_scored": pairs, "largest_slot": int(np.bincount(mc).max()), "widest_alignment": widest, "launches": launches,
                "steps": args.steps, "warmup": args.warmup,
                "align_kernel_ms": spread(al_k), "align_kernel_ms_without_sums_copy": spread(bare_k),
                "linkage_kernel_ms": spread(li_k), "linkage_kernel_ms_without_member_outputs": spread(li_bare_k),
                "pairs_route_kernel_ms": spread(old_k),
                "align_wall_ms": spread(al_w), "linkage_wall_ms": spread(li_w), "pairs_route_wall_ms": spread(old_w),
                "kernel_ms_align_minus_linkage": float(np.median(al_k) - np.median(li_k)),
                "kernel_ratio_align_over_linkage": float(np.median(al_k) / np.median(li_k)),
                "wall_ratio_pairs_route_over_align": float(np.median(old_w) / np.median(al_w)),
                "align_pairs_per_s": float(pairs / (np.median(al_k) * 1e-3))}

    n5 = 100_000
    res5, off5 = synth_peptides(1, n5, 12)
    if "a" in only:
        ctx.set_sequences(residues=res5, offsets=off5)
        cid, _, _ = ctx.greedy_cluster(X, P, THR, int(round(n5 * 0.025)))
        _, mc_all, counts = np.unique(cid, return_inverse=True, return_counts=True)
        keep = np.flatnonzero(counts[mc_all] > 1)
        ctx.set_sequences(residues=res5.reshape(n5, 12)[keep].ravel(), offsets=(np.arange(len(keep) + 1) * 12).astype(np.uint32))
        _, mc = np.unique(cid[keep], return_inverse=True)
        print(json.dumps(run("a: multi-member clusters of the 1e5 greedy", len(keep), mc)), flush=True)
    if "b" in only:
        with open(os.path.join(ROOT, "tests", "golden", "musi.fa")) as fh:
            musi = list(dict.fromkeys(line.strip() for line in fh if line.strip() and not line.startswith(">")))
        res, off = hammock_amd.pack_sequences(musi)
        ctx.set_sequences(residues=res, offsets=off)
        cid, _, _ = ctx.clinkage_cluster(X, P, THR)
        _, mc = np.unique(cid, return_inverse=True)
        print(json.dumps(run("b: clinkage clusters of MUSI", len(musi), mc)), flush=True)
    if "c" in only:
        res, off = synth_peptides(2, n5, 12)
        ctx.set_sequences(residues=res, offsets=off)
        mc = np.random.default_rng(7).permutation(np.repeat(np.arange(n5 // 10), 10))
        print(json.dumps(run("c: 1e4 slots of 10 members", n5, mc)), flush=True)
    if "d" in only:
        n = 20_000
        res, off = synth_peptides(3, n, 12)
        ctx.set_sequences(residues=res, offsets=off)
        print(json.dumps(run("d: one slot of 20,000 12-mers", n, np.zeros(n, dtype=np.int64))), flush=True)


if __name__ == "__main__":
    main()
