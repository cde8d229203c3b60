#!/usr/bin/env python3
"""bench_survey.py -- the score survey (hmk_score_survey_shifted) on one MI355X, beside the calls that score the same pairs today.

BLOSUM62, max shift 3, shift penalty 0, threshold 20, a resident context; synthetic 12-mers (hammock_amd.synth).  Workloads (--only
picks some):
  a  the triangle of 20,000 12-mers (seed 3; 2.0 x 10^8 pairs) beside hmk_cluster_linkage_shifted on the same 20,000 as one slot: the
     same pairs, scorer and tile walk.  Also the forms without the histogram (n_bins = 0) and without the row outputs (rows=False), and
     the route a user has without the call: hmk_score_block_shifted in blocks of 2,000 rows + np.bincount (wall time, --block-steps
     rounds).
  b  the triangle of 10^5 12-mers (seed 1; 5.0 x 10^9 pairs) beside hmk_neighbors_shifted at threshold 20 on the same set: the
     literal scorer against the byte-lane pass.
  c  the rectangle of 10^4 queries x 10^5 references (seeds 4, 1) beside hmk_search_shifted at threshold 20.
  d  the two forms of the workgroup's LDS histogram -- lane-replicated copies (what every call runs) and one add per distinct bin of
     a wave-instruction -- on (a) and on 20,000 copies of one 12-mer, where all 64 lanes of every wave-instruction hit one bin.  The
     second form is reached through the library's measurement hook, which is not part of the ABI.
The routes of a workload alternate in one process, --steps timed rounds after --warmup untimed ones; per route the median, minimum
and maximum of the device time (the calls' kernel_ms, HIP events) and of the wall time.  Prints one JSON line per workload.

    python tools/bench_survey.py [--steps 10] [--warmup 3] [--block-steps 3] [--only a,b,c,d]
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

X, P, THR, LO, BINS = 3, 0, 20, -120, 256   # 12-mers under BLOSUM62 at penalty 0: every score lies in [-48, 132]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--block-steps", type=int, default=3)
    ap.add_argument("--only", default="a,b,c,d")
    args = ap.parse_args()
    only = set(args.only.split(","))
    import hammock_amd
    from hammock_amd import _native as N
    from hammock_amd.synth import synth_peptides
    with open(os.path.join(ROOT, "tests", "golden", "matrices.json")) as fh:
        M = np.asarray(json.load(fh)["matrices"]["blosum62"], dtype=np.int32)
    ctx = hammock_amd.Context(M, device=0)
    rounds = range(args.warmup + args.steps)

    def timed(fn):
        t0 = time.perf_counter()
        out = fn()
        return out, (time.perf_counter() - t0) * 1e3

    def survey(q0, q1, r0, r1, **kw):
        kw = {"score_lo": LO, "n_bins": BINS, **kw}
        return ctx.score_survey_shifted(q0, q1, r0, r1, X, P, THR, **kw)

    n = 20_000
    res3, off3 = synth_peptides(3, n, 12)
    if "a" in only:
        ctx.set_sequences(residues=res3, offsets=off3)
        one = np.zeros(n, dtype=np.uint32)
        k = {name: [] for name in ("survey", "no_hist", "no_rows", "linkage", "linkage_bare")}
        w = {name: [] for name in ("survey", "linkage")}
        for step in rounds:
            (hist, rows, st), ws = timed(lambda: survey(0, n, 0, n))
            _, _, st0 = survey(0, n, 0, n, n_bins=0)
            _, _, st1 = survey(0, n, 0, n, rows=False)
            link, wl = timed(lambda: ctx.cluster_linkage_shifted(0, n, one, 1, X, P, THR))
            kl = ctx.last_linkage_stats.kernel_ms
            n_below_thr = int(link[3][0])
            ctx.cluster_linkage_shifted(0, n, one, 1, X, P, THR, members=False)
            klb = ctx.last_linkage_stats.kernel_ms
            if step == 0:   # the routes say the same
                assert st.n_below == st.n_above == 0 and int(hist.sum()) == st.pairs_scored == n * (n - 1) // 2
                assert st.pairs_scored - st.n_at_or_above == n_below_thr and st.score_min == int(link[0][0])
                assert np.array_equal(rows[2], n - 1 - link[5]) and st0.n_at_or_above == st1.n_at_or_above == st.n_at_or_above
            if step >= args.warmup:
                for name, v in (("survey", st.kernel_ms), ("no_hist", st0.kernel_ms), ("no_rows", st1.kernel_ms), ("linkage", kl),
                                ("linkage_bare", klb)):
                    k[name].append(v)
                w["survey"].append(ws)
                w["linkage"].append(wl)
        blocks = []
        for step in range(args.block_steps):   # what a user does today: every score across the bus, 4 bytes each
            def route():
                h = np.zeros(BINS, dtype=np.int64)
                for r0 in range(0, n, 2000):
                    sc = ctx.score_block_shifted(r0, r0 + 2000, 0, r0 + 2000, X, P)
                    keep = np.arange(r0, r0 + 2000)[:, None] > np.arange(r0 + 2000)[None, :]
                    h += np.bincount(sc[keep] - LO, minlength=BINS)
                return h
            h, wb = timed(route)
            assert np.array_equal(h.astype(np.uint64), hist)
            blocks.append(wb)
        sp = {name: spread(v) for name, v in k.items()}
        slack = (sp["survey"]["max"] - sp["survey"]["min"]) + (sp["linkage"]["max"] - sp["linkage"]["min"])
        print(json.dumps({"workload": "a: triangle of 20,000 12-mers", "pairs": n * (n - 1) // 2, "steps": args.steps, "warmup": args.warmup,
                          "survey_kernel_ms": sp["survey"], "survey_kernel_ms_n_bins_0": sp["no_hist"], "survey_kernel_ms_rows_false": sp["no_rows"],
                          "linkage_kernel_ms": sp["linkage"], "linkage_kernel_ms_without_member_outputs": sp["linkage_bare"],
                          "survey_wall_ms": spread(w["survey"]), "linkage_wall_ms": spread(w["linkage"]),
                          "wanted_survey_at_most_ms": sp["linkage"]["median"] + slack,
                          "wanted_met": bool(sp["survey"]["median"] <= sp["linkage"]["median"] + slack),
                          "kernel_ratio_survey_over_linkage": sp["survey"]["median"] / sp["linkage"]["median"],
                          "score_block_and_bincount_wall_ms": spread(blocks), "score_block_steps": args.block_steps,
                          "survey_pairs_per_s": n * (n - 1) / 2 / (sp["survey"]["median"] * 1e-3)}), flush=True)

    if "d" in only:
        form = N.lib.hmk_survey_hist_form_for_measurement
        copies = np.tile(res3[:12], n)
        out = {"workload": "d: the two LDS histogram forms", "steps": args.steps, "warmup": args.warmup}
        for name, res in (("20000_random", res3), ("20000_copies", copies)):
            ctx.set_sequences(residues=res, offsets=off3)
            k = {0: [], 1: [], "rows_only": []}
            hists = {}
            for step in rounds:
                for f in (0, 1):
                    form(f)
                    try:
                        hists[f], _, st = survey(0, n, 0, n)
                    finally:
                        form(0)
                    if step >= args.warmup:
                        k[f].append(st.kernel_ms)
                _, _, st = survey(0, n, 0, n, n_bins=0)
                if step >= args.warmup:
                    k["rows_only"].append(st.kernel_ms)
            assert np.array_equal(hists[0], hists[1])
            out[name] = {"lane_replicated_copies_kernel_ms": spread(k[0]), "wave_aggregated_kernel_ms": spread(k[1]),
                         "no_histogram_kernel_ms": spread(k["rows_only"]), "largest_bin_share": float(hists[0].max() / hists[0].sum())}
        print(json.dumps(out), flush=True)

    n5 = 100_000
    res1, off1 = synth_peptides(1, n5, 12)
    if "b" in only:
        ctx.set_sequences(residues=res1, offsets=off1)
        ks, kn = [], []
        cap = len(ctx.neighbors_shifted(X, P, THR)[0])   # (sizes the host buffer: no timed round scores twice)
        for step in rounds:
            hist, rows, st = survey(0, n5, 0, n5)
            _, ns = ctx.neighbors_shifted(X, P, THR, capacity=cap)
            if step == 0:
                assert ns.n_edges == st.n_at_or_above and ns.pairs_scored == st.pairs_scored
            if step >= args.warmup:
                ks.append(st.kernel_ms)
                kn.append(ns.kernel_ms)
        print(json.dumps({"workload": "b: triangle of 100,000 12-mers", "pairs": int(st.pairs_scored), "pairs_at_or_above_20": int(st.n_at_or_above),
                          "steps": args.steps, "warmup": args.warmup, "survey_kernel_ms": spread(ks), "neighbors_kernel_ms": spread(kn),
                          "kernel_ratio_survey_over_neighbors": float(np.median(ks) / np.median(kn)),
                          "survey_pairs_per_s": float(st.pairs_scored / (np.median(ks) * 1e-3))}), flush=True)

    if "c" in only:
        nq = 10_000
        res4, _ = synth_peptides(4, nq, 12)
        ctx.set_sequences(residues=np.concatenate([res4, res1]), offsets=(np.arange(nq + n5 + 1) * 12).astype(np.uint32))
        ks, kn = [], []
        cap = len(ctx.search_shifted(0, nq, nq, nq + n5, X, P, THR)[0])
        for step in rounds:
            hist, rows, st = survey(0, nq, nq, nq + n5)
            _, ss = ctx.search_shifted(0, nq, nq, nq + n5, X, P, THR, capacity=cap)
            if step == 0:
                assert ss.n_edges == st.n_at_or_above and int(rows[2].sum()) == st.n_at_or_above
            if step >= args.warmup:
                ks.append(st.kernel_ms)
                kn.append(ss.kernel_ms)
        print(json.dumps({"workload": "c: rectangle of 10,000 x 100,000 12-mers", "pairs": int(st.pairs_scored),
                          "pairs_at_or_above_20": int(st.n_at_or_above), "steps": args.steps, "warmup": args.warmup,
                          "survey_kernel_ms": spread(ks), "search_kernel_ms": spread(kn),
                          "kernel_ratio_survey_over_search": float(np.median(ks) / np.median(kn))}), flush=True)


if __name__ == "__main__":
    main()
