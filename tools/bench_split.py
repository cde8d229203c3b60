#!/usr/bin/env python3
"""bench_split.py -- splitting given clusters by complete linkage (hmk_clinkage_split) on one MI355X, beside the only other route
to the scores it needs: hmk_score_pairs_shifted over the enumerated pairs inside every cluster.

BLOSUM62, max shift 3, shift penalty 0, a resident context.  Workloads (--only picks some):
  a20, a26  the multi-member clusters of the greedy (limit round(0.025 n), threshold 20) on bench.py's 10^5 synthetic 12-mers
            (seed 1), split at threshold 20 and at 26
  b         the clinkage clusters of MUSI (tests/golden/musi.fa, threshold 20), singletons included, split at threshold 26
  c         10^4 slots of 10 members (10^5 synthetic 12-mers, seed 2, members dealt at random), threshold 20
  d         one slot of 20,000 distinct 12-mers around one centre (at most 4 substitutions), threshold 20: 2 x 10^8 pairs through
            the tiled kernel, and one long chain on the host
The two routes alternate in one process, --steps timed rounds after --warmup untimed ones.  Per workload the median, minimum and
maximum of: the new call's kernel_ms, copy_ms and chain_ms (hmk_split_stats) and its wall time; the pair kernel's device time
(hmk_last_kernel_ms) and the old route's wall time for the scores alone (the pair list is enumerated once, outside the timing, and
the old route's chains -- one hmk_clinkage_from_edges call per slot -- are not run at all: both favour the old route).  Bytes over
PCIe per call on both routes are counted, not measured.  Prints one JSON line per workload.

    python tools/bench_split.py [--steps 10] [--warmup 3] [--only a20,a26,b,c,d]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_linkage import inside_pairs, spread   # noqa: E402

X, P = 3, 0
LINK_FLAT_MAX = 256


def table_bytes(mc):
    """the bytes of the tables the new call uploads (hmk_linkage.h: LinkTables)"""
    counts = np.bincount(mc)
    nf = int(((counts >= 2) & (counts <= LINK_FLAT_MAX)).sum())
    nb = int((counts > LINK_FLAT_MAX).sum())
    words = int(counts[counts >= 2].sum()) + nf + (nf + 1) + nb + 2 * (nb + 1)
    words = (words + 1) & ~1
    return 4 * (words + 2 * (nf + 1) + 2 * (nb + 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="a20,a26,b,c,d")
    args = ap.parse_args()
    only = set(args.only.split(","))
    import hammock_amd
    from hammock_amd.synth import synth_peptides
    with open(os.path.join(ROOT, "tests", "golden", "matrices.json")) as fh:
        M = np.asarray(json.load(fh)["matrices"]["blosum62"], dtype=np.int32)
    ctx = hammock_amd.Context(M, device=0)

    def run(name, n, mc, thr):
        """the uploaded set's members [0, n) in slots mc: both routes, alternating"""
        mc = np.asarray(mc, dtype=np.int64)
        ncl = int(mc.max()) + 1
        a, b, first, slots = inside_pairs(mc)
        cols = {k: [] for k in ("new_kernel_ms", "new_copy_ms", "new_chain_ms", "new_wall_ms", "old_kernel_ms", "old_wall_ms")}
        for step in range(args.warmup + args.steps):
            t0 = time.perf_counter()
            sc = ctx.score_pairs_shifted(b, a, X, P)   # seq1 = the larger index
            t1 = time.perf_counter()
            k_old = ctx.last_kernel_ms()
            t2 = time.perf_counter()
            got = ctx.clinkage_split(0, n, mc, ncl, X, P, thr)
            t3 = time.perf_counter()
            st = ctx.last_split_stats
            if step == 0:   # the two routes saw the same scores
                assert int(st.pairs_scored) == a.size and int(st.n_edges) == int((sc >= thr).sum())
                below = np.add.reduceat((sc < thr).astype(np.int64), first) if a.size else np.zeros(0, dtype=np.int64)
                assert np.array_equal(got[1][slots] > 1, below > 0)
            if step >= args.warmup:
                for k, v in (("new_kernel_ms", st.kernel_ms), ("new_copy_ms", st.copy_ms), ("new_chain_ms", st.chain_ms),
                             ("new_wall_ms", (t3 - t2) * 1e3), ("old_kernel_ms", k_old), ("old_wall_ms", (t1 - t0) * 1e3)):
                    cols[k].append(v)
        row = {"workload": name, "threshold": thr, "slots": ncl, "multi_member_slots": int(slots.size), "members": int(n), "pairs": int(a.size),
               "largest_slot": int(np.bincount(mc).max()), "edges": int(st.n_edges), "slots_split": int(st.n_split),
               "resulting_clusters": int(st.n_result_clusters), "steps": args.steps, "warmup": args.warmup}
        row.update({k: spread(v) for k, v in cols.items()})
        row["kernel_ratio_new_over_old"] = float(np.median(cols["new_kernel_ms"]) / np.median(cols["old_kernel_ms"]))
        row["new_pcie_bytes"] = {"up": table_bytes(mc), "down": 2 * int(a.size)}
        row["old_pcie_bytes"] = {"up": 8 * int(a.size), "down": 4 * int(a.size)}
        return row

    n5 = 100_000
    if "a20" in only or "a26" in only:
        res5, off5 = synth_peptides(1, n5, 12)
        ctx.set_sequences(residues=res5, offsets=off5)
        cid, _, _ = ctx.greedy_cluster(X, P, 20, int(round(n5 * 0.025)))
        _, mc_all, counts = np.unique(cid, return_inverse=True, return_counts=True)
        keep = np.flatnonzero(counts[mc_all] > 1)
        ctx.set_sequences(residues=res5.reshape(n5, 12)[keep].ravel(), offsets=(np.arange(len(keep) + 1) * 12).astype(np.uint32))
        _, mc = np.unique(cid[keep], return_inverse=True)
        for thr in (20, 26):
            if "a%d" % thr in only:
                print(json.dumps(run("a: multi-member clusters of the 1e5 greedy", len(keep), mc, thr)), flush=True)
    if "b" in only:
        with open(os.path.join(ROOT, "tests", "golden", "musi.fa")) as fh:
            musi = list(dict.fromkeys(line.strip() for line in fh if line.strip() and not line.startswith(">")))
        res, off = hammock_amd.pack_sequences(musi)
        ctx.set_sequences(residues=res, offsets=off)
        cid, _, _ = ctx.clinkage_cluster(X, P, 20)
        _, mc = np.unique(cid, return_inverse=True)
        print(json.dumps(run("b: clinkage clusters of MUSI", len(musi), mc, 26)), flush=True)
    if "c" in only:
        res, off = synth_peptides(2, n5, 12)
        ctx.set_sequences(residues=res, offsets=off)
        mc = np.random.default_rng(7).permutation(np.repeat(np.arange(n5 // 10), 10))
        print(json.dumps(run("c: 1e4 slots of 10 members", n5, mc, 20)), flush=True)
    if "d" in only:
        n = 20_000
        rng = np.random.default_rng(11)
        centre = rng.integers(0, 20, size=12).astype(np.uint8)
        seen, peps = set(), []
        while len(peps) < n:
            q = centre.copy()
            for pos in rng.choice(12, size=int(rng.integers(1, 5)), replace=False):
                q[pos] = rng.integers(0, 20)
            if q.tobytes() not in seen:
                seen.add(q.tobytes())
                peps.append(q)
        ctx.set_sequences(residues=np.concatenate(peps), offsets=(np.arange(n + 1) * 12).astype(np.uint32))
        print(json.dumps(run("d: one slot of 20,000 12-mers around one centre", n, np.zeros(n, dtype=np.int64), 20)), flush=True)


if __name__ == "__main__":
    main()
