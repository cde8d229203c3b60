#!/usr/bin/env python3
"""bench_profile.py -- cluster profiles (hmk_cluster_profile) on one MI355X, beside (i) hmk_cluster_align_shifted on the same slots,
the call it follows and whose columns it takes, and (ii) the only other route to the same numbers: the placement on the host and the
definition there, vectorised with numpy (counts by bincount, ic and the leave-one-out KLD terms as array expressions over all
(member, residue) places at once; numpy sums pairwise, so its doubles agree with the call's to rounding, which step 0 asserts).

BLOSUM62, max shift 3, shift penalty 0, the frequency table of tests/golden/blosum62.freq_rownorm, a uniform background, the
reference's defaults, a resident context.  Workloads (--only picks some) are those of tools/bench_align.py:
  a  the multi-member clusters of the greedy (limit round(0.025 n)) on bench.py's 10^5 synthetic 12-mers (seed 1)
  b  the clinkage clusters of MUSI (tests/golden/musi.fa), singletons included
  c  10^4 slots of 10 members (10^5 synthetic 12-mers, seed 2, members dealt at random)
  d  one slot of 20,000 synthetic 12-mers (seed 3)
The routes alternate in one process, --steps timed rounds after --warmup untimed ones; per route the median, minimum and maximum of
the device time (hmk_profile_stats.kernel_ms with and without the per-column arrays' copies; hmk_align_stats.kernel_ms) and of the
wall time.  Then where the two count forms cross: 65,536 synthetic 12-mers in equal slots of 2 ... 8,192 members, every slot
through the lane-per-member form (HMK_PROFILE_LARGE_MIN above the slot size) and through the LDS form (HMK_PROFILE_LARGE_MIN=2), the
call's device time of each.  Writes profiles/profile_bench.json and prints it.

    python tools/bench_profile.py [--steps 10] [--warmup 3] [--only a,b,c,d,x]
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
BETA, SIGMA, SCALE, MIN_IC, MAX_GAP = 200.0, 10.0, 2.88539, 1.2, 0.2


def host_route(res, off, mc, ncl, column, F, bg):
    """the definition on the host with numpy -> (counts, ic, flags, kld_all, kld_match)"""
    lens = (off[1:] - off[:-1]).astype(np.int64)
    n = mc.size
    width = np.zeros(ncl, dtype=np.int64)
    np.maximum.at(width, mc, column + lens)
    cstart = np.concatenate([[0], np.cumsum(width)])
    size = np.bincount(mc, minlength=ncl)
    member = np.repeat(np.arange(n), lens)                       # one entry per (member, residue) place
    k = np.arange(member.size) - np.repeat(off[:-1].astype(np.int64), lens)
    g = cstart[mc[member]] + column[member] + k
    a = res.astype(np.int64)
    counts = np.bincount(g * 21 + a, minlength=int(cstart[-1]) * 21).reshape(-1, 21)
    slot_of_col = np.repeat(np.arange(ncl), width)
    counts[:, 20] = size[slot_of_col] - counts[:, :20].sum(axis=1)
    nongap = counts[:, :20].sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        p = counts[:, :20] / nongap[:, None]
        ent = np.where(counts[:, :20] > 0, p * (np.log(p) / np.log(2)), 0.0).sum(axis=1)
    ic = np.where(counts[:, 20] / size[slot_of_col] <= MAX_GAP, -(np.log(0.05) / np.log(2)) + ent, -1.0)
    cons = ic >= MIN_IC
    rel = np.arange(cons.size) - cstart[slot_of_col]
    first = np.full(ncl, 1 << 30)
    last = np.full(ncl, -1)
    np.minimum.at(first, slot_of_col[cons], rel[cons])
    np.maximum.at(last, slot_of_col[cons], rel[cons])
    match = (rel >= first[slot_of_col]) & (rel <= last[slot_of_col])
    s = (size[mc[member]] - 1).astype(np.float64)
    cnt = counts[g, :20].astype(np.float64)
    cnt[np.arange(member.size), a] -= 1
    with np.errstate(divide="ignore", invalid="ignore"):
        gi = ((cnt / s[:, None]) * F[:, a].T).sum(axis=1)
        fi = cnt[np.arange(member.size), a] / s
        Q = ((s - 1) * fi + BETA * gi) / ((s - 1) + BETA)
        term = np.log(Q / bg[a]) * (s / (s + SIGMA)) * SCALE
    term[(s < 1) | (counts[g, 20] == s)] = 0.0                   # a slot of one member; only gaps remain
    kld_all = np.bincount(member, weights=term, minlength=n)
    kld_match = np.bincount(member, weights=np.where(match[g], term, 0.0), minlength=n)
    return counts, ic, cons.astype(np.uint8) + 2 * match.astype(np.uint8), kld_all, kld_match


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="a,b,c,d,x")
    args = ap.parse_args()
    only = set(args.only.split(","))
    import hammock_amd
    from hammock_amd.synth import synth_peptides
    with open(os.path.join(ROOT, "tests", "golden", "matrices.json")) as fh:
        M = np.asarray(json.load(fh)["matrices"]["blosum62"], dtype=np.int32)
    F, _ = hammock_amd.load_frequency_matrix(os.path.join(ROOT, "tests", "golden", "blosum62.freq_rownorm"))
    bg = np.full(20, 0.05)
    params = hammock_amd.profile_params(F)
    ctx = hammock_amd.Context(M, device=0)
    results = []

    def run(name, res, off, mc):
        mc = np.asarray(mc, dtype=np.int64)
        n, ncl = mc.size, int(mc.max()) + 1
        res = np.asarray(res)
        pr_k, pr_w, bare_k, al_k, al_w, host_w = [], [], [], [], [], []
        for step in range(args.warmup + args.steps):
            t0 = time.perf_counter()
            column = ctx.cluster_align_shifted(0, n, mc, ncl, X, P, sums=False)[6].astype(np.int64)
            t1 = time.perf_counter()
            k_al = ctx.last_align_stats.kernel_ms
            R = ctx.cluster_profile(0, n, mc, ncl, column, params, col_capacity=None if step == 0 else cap)
            t2 = time.perf_counter()
            cap = int(R.stats.columns)
            k_pr, launches, chunks, small = R.stats.kernel_ms, int(R.stats.launches), int(R.stats.large_chunks), int(R.stats.small_members)
            k_bare = ctx.cluster_profile(0, n, mc, ncl, column, params, counts=False, ic=False, flags=False).stats.kernel_ms
            t3 = time.perf_counter()
            counts, ic, flags, kld_all, kld_match = host_route(res, off, mc, ncl, column, F, bg)
            t4 = time.perf_counter()
            if step == 0:   # the routes say the same
                assert np.array_equal(counts, R.counts) and np.abs(ic - R.ic).max() < 1e-9
                if np.abs(ic - MIN_IC).min() >= 1e-9:
                    assert np.array_equal(flags, R.col_flags) and np.abs(kld_match - R.kld_match).max() < 1e-9
                assert np.abs(kld_all - R.kld_all).max() < 1e-9
            if step >= args.warmup:
                al_w.append((t1 - t0) * 1e3)
                al_k.append(k_al)
                pr_w.append((t2 - t1) * 1e3)
                pr_k.append(k_pr)
                bare_k.append(k_bare)
                host_w.append((t4 - t3) * 1e3)
        out = {"workload": name, "slots": ncl, "members": n, "columns": cap, "largest_slot": int(np.bincount(mc).max()), "launches": launches,
               "large_chunks": chunks, "small_members": small, "steps": args.steps, "warmup": args.warmup,
               "profile_kernel_ms": spread(pr_k), "profile_kernel_ms_without_column_copies": spread(bare_k), "align_kernel_ms": spread(al_k),
               "profile_wall_ms": spread(pr_w), "align_wall_ms": spread(al_w), "host_numpy_route_wall_ms": spread(host_w),
               "kernel_ratio_profile_over_align": float(np.median(pr_k) / np.median(al_k)),
               "wall_ratio_host_route_over_profile": float(np.median(host_w) / np.median(pr_w)),
               "system_kld_match": R.stats.system_kld_match, "system_kld_all": R.stats.system_kld_all}
        results.append(out)
        print(json.dumps(out), flush=True)

    n5 = 100_000
    if "a" in only:
        res5, off5 = synth_peptides(1, n5, 12)
        ctx.set_sequences(residues=res5, offsets=off5)
        cid, _, _ = ctx.greedy_cluster(X, P, THR, int(round(n5 * 0.025)))
        _, mc_all, counts = np.unique(cid, return_inverse=True, return_counts=True)
        keep = np.flatnonzero(counts[mc_all] > 1)
        res = res5.reshape(n5, 12)[keep].ravel()
        off = (np.arange(len(keep) + 1) * 12).astype(np.uint32)
        ctx.set_sequences(residues=res, offsets=off)
        _, mc = np.unique(cid[keep], return_inverse=True)
        run("a: multi-member clusters of the 1e5 greedy", res, off, mc)
    if "b" in only:
        with open(os.path.join(ROOT, "tests", "golden", "musi.fa")) as fh:
            musi = list(dict.fromkeys(line.strip() for line in fh if line.strip() and not line.startswith(">")))
        res, off = hammock_amd.pack_sequences(musi)
        ctx.set_sequences(residues=res, offsets=off)
        cid, _, _ = ctx.clinkage_cluster(X, P, THR)
        _, mc = np.unique(cid, return_inverse=True)
        run("b: clinkage clusters of MUSI", res, off, mc)
    if "c" in only:
        res, off = synth_peptides(2, n5, 12)
        ctx.set_sequences(residues=res, offsets=off)
        run("c: 1e4 slots of 10 members", res, off, np.random.default_rng(7).permutation(np.repeat(np.arange(n5 // 10), 10)))
    if "d" in only:
        n = 20_000
        res, off = synth_peptides(3, n, 12)
        ctx.set_sequences(residues=res, offsets=off)
        run("d: one slot of 20,000 12-mers", res, off, np.zeros(n, dtype=np.int64))
    if "x" in only:   # where the two count forms cross
        n = 65_536
        res, off = synth_peptides(4, n, 12)
        ctx.set_sequences(residues=res, offsets=off)
        column = np.random.default_rng(8).integers(0, 3, size=n)
        rows = []
        for s in (2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 8192):
            mc = np.random.default_rng(9).permutation(np.repeat(np.arange(n // s), s))
            row = {"slot_size": s, "slots": n // s}
            for form, large_min in (("lane_per_member", 10 ** 6), ("lds_chunks", 2)):
                os.environ["HMK_PROFILE_LARGE_MIN"] = str(large_min)
                ms = []
                for step in range(args.warmup + args.steps):
                    st = ctx.cluster_profile(0, n, mc, n // s, column, params, counts=False, ic=False, flags=False).stats
                    if step >= args.warmup:
                        ms.append(st.kernel_ms)
                row[form + "_kernel_ms"] = spread(ms)
                row[form + "_chunks"] = int(st.large_chunks)
            del os.environ["HMK_PROFILE_LARGE_MIN"]
            rows.append(row)
        out = {"workload": "x: 65,536 12-mers in equal slots, both count forms", "steps": args.steps, "warmup": args.warmup, "sizes": rows}
        results.append(out)
        print(json.dumps(out), flush=True)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "profile_bench.json"), "w") as fh:
        json.dump(results, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
