#!/usr/bin/env python3
"""bench_linkage.py -- complete-linkage scores inside given clusters (hmk_cluster_linkage_shifted) on one MI355X, beside the only
other route to the same numbers: hmk_score_pairs_shifted over the enumerated pairs inside every cluster, reduced on the host.

BLOSUM62, max shift 3, shift penalty 0, threshold 20, a resident context.  Workloads (--only picks some):
  a  the multi-member clusters of the greedy (limit round(0.025 n)) on bench.py's 10^5 synthetic 12-mers (seed 1)
  b  the clinkage clusters of MUSI (tests/golden/musi.fa), singletons included
  c  10^4 slots of 10 members (10^5 synthetic 12-mers, seed 2, members dealt at random)
  d  one slot of 20,000 synthetic 12-mers (seed 3): 2 x 10^8 pairs through the tiled kernel
The two routes alternate in one process, --steps timed rounds after --warmup untimed ones; per route the median, minimum and
maximum of the device time (new: hmk_linkage_stats.kernel_ms, with and without the per-member outputs; old: hmk_last_kernel_ms)
and of the wall time (new: the call; old: the call plus a numpy reduction of the scores to min_score, the pair that attains it
and n_below per slot -- the pair list itself is enumerated once, outside the timing, and the per-member numbers are left out of
the old route's reduction: both favour the old route).  d also reports pairs per second of the new call beside the all-vs-all
pass (hmk_neighbors_shifted, 10^5 set, threshold 20).  Prints one JSON line per workload.

    python tools/bench_linkage.py [--steps 10] [--warmup 3] [--only a,b,c,d]
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


def inside_pairs(mc):
    """the pairs inside every slot, slot by slot -> (a uint32, b uint32, first pair of every multi-member slot, those slots)"""
    order = np.argsort(mc, kind="stable")
    counts = np.bincount(mc)
    starts = np.concatenate([[0], np.cumsum(counts)])
    aa, bb, first, slots, at = [], [], [], [], 0
    tri = {}   # (the triangle's index pairs per member count: 10^4 slots share one)
    for c in np.flatnonzero(counts > 1):
        s = int(counts[c])
        if s not in tri:
            tri.clear()
            i, j = np.triu_indices(s, 1)
            tri[s] = (i.astype(np.uint32), j.astype(np.uint32))
        m = order[starts[c]:starts[c + 1]].astype(np.uint32)   # (ascending: the sort is stable)
        aa.append(m[tri[s][0]])
        bb.append(m[tri[s][1]])
        first.append(at)
        slots.append(c)
        at += s * (s - 1) // 2
    if len(aa) == 1:
        return aa[0], bb[0], np.asarray(first, dtype=np.int64), np.asarray(slots, dtype=np.int64)
    return np.concatenate(aa), np.concatenate(bb), np.asarray(first, dtype=np.int64), np.asarray(slots, dtype=np.int64)


def spread(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


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
        """the uploaded set's members [0, n) in slots mc: both routes, alternating"""
        mc = np.asarray(mc, dtype=np.int64)
        ncl = int(mc.max()) + 1
        a, b, first, slots = inside_pairs(mc)
        new_k, new_w, bare_k, old_k, old_w = [], [], [], [], []
        for step in range(args.warmup + args.steps):
            t0 = time.perf_counter()
            sc = ctx.score_pairs_shifted(b, a, X, P)   # seq1 = the larger index
            key = (sc.astype(np.int64) + 32768).astype(np.uint64) << np.uint64(48) | a.astype(np.uint64) << np.uint64(24) | b.astype(np.uint64)
            old_key = np.minimum.reduceat(key, first)
            old_below = np.add.reduceat((sc < THR).astype(np.int64), first)
            t1 = time.perf_counter()
            k_old = ctx.last_kernel_ms()
            t2 = time.perf_counter()
            got = ctx.cluster_linkage_shifted(0, n, mc, ncl, X, P, THR)
            t3 = time.perf_counter()
            st = ctx.last_linkage_stats
            k_new, pairs, launches = st.kernel_ms, int(st.pairs_scored), int(st.launches)
            ctx.cluster_linkage_shifted(0, n, mc, ncl, X, P, THR, members=False)
            k_bare = ctx.last_linkage_stats.kernel_ms
            if step == 0:   # the two routes say the same
                assert np.array_equal(got[0][slots], (old_key >> np.uint64(48)).astype(np.int64) - 32768)
                assert np.array_equal(got[1][slots], (old_key >> np.uint64(24)).astype(np.int64) & 0xFFFFFF)
                assert np.array_equal(got[2][slots], old_key.astype(np.int64) & 0xFFFFFF)
                assert np.array_equal(got[3][slots].astype(np.int64), old_below)
                assert pairs == a.size
            if step >= args.warmup:
                old_w.append((t1 - t0) * 1e3)
                old_k.append(k_old)
                new_w.append((t3 - t2) * 1e3)
                new_k.append(k_new)
                bare_k.append(k_bare)
        row = {"workload": name, "slots": ncl, "multi_member_slots": int(slots.size), "members": int(n), "pairs": int(a.size),
               "largest_slot": int(np.bincount(mc).max()), "launches": launches, "steps": args.steps, "warmup": args.warmup,
               "new_kernel_ms": spread(new_k), "new_kernel_ms_without_member_outputs": spread(bare_k), "old_kernel_ms": spread(old_k),
               "new_wall_ms": spread(new_w), "old_wall_ms": spread(old_w),
               "kernel_ratio_new_over_old": float(np.median(new_k) / np.median(old_k)),
               "new_pairs_per_s": float(a.size / (np.median(new_k) * 1e-3))}
        return row

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
        ctx.set_sequences(residues=res5, offsets=off5)
        rates = []
        for step in range(args.warmup + args.steps):
            _, st = ctx.neighbors_shifted(X, P, THR)
            if step >= args.warmup:
                rates.append(st.pairs_scored / (st.kernel_ms * 1e-3))
        n = 20_000
        res, off = synth_peptides(3, n, 12)
        ctx.set_sequences(residues=res, offsets=off)
        row = run("d: one slot of 20,000 12-mers", n, np.zeros(n, dtype=np.int64))
        row["all_vs_all_pairs_per_s_1e5"] = float(np.median(rates))
        row["share_of_all_vs_all_rate"] = row["new_pairs_per_s"] / row["all_vs_all_pairs_per_s_1e5"]
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
