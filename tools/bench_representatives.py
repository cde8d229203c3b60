#!/usr/bin/env python3
"""bench_representatives.py -- the representatives of a set (hmk_representatives_shifted) on one MI355X, beside the only other route
to them: hmk_neighbors_shifted to the host, then hmk_representatives_from_edges (the sequential definition) per wanted threshold;
and beside hmk_components_shifted on the same input, the other call that walks the same edges on the device.

BLOSUM62, max shift 3, shift penalty 0, a resident context.  Workloads (--only picks some):
  a     bench.py's 10^5 synthetic 12-mers (seed 1), threshold 20, a single level
  b     the same, levels 20 ... 40
  c1/c  the antibodies example (tests/golden/antibodies.fa.gz, its 74,041 distinct 12-mers), a single level at 20 / levels 20 ... 40
  d     17,000 peptides over three letters at threshold 14: about 94 % of the pairs are neighbours, very few representatives
  e1    10^6 synthetic 12-mers (seed 1), a single level at 20
The routes alternate in one process, --steps timed rounds after --warmup untimed ones: the new call, hmk_components_shifted, and in
--old-steps of the rounds (after --old-warmup untimed ones; 0: not at all) the old route, which scores once and runs the host
selection once per threshold.  Per workload the median, minimum and maximum of the new call's kernel_ms, select_ms and wall time,
components_ms of the components call, the old route's pass and wall time; rounds_total; for every level of the last call the live
edges behind each round, read off the call's HMK_GREEDY_TIMING lines in one extra untimed call (`live_edges`: level -> counts; the
edges all rounds together read are n_edges + their sum, `edges_read_ratio` relates that to n_edges).  The bytes over PCIe per call on
both routes are counted, not measured.  Prints one JSON line per workload; --out FILE keeps them under "workloads" of the JSON object
in FILE, replacing the rows of the same name and leaving the file's other sections as they are.

    python tools/bench_representatives.py [--steps 10] [--warmup 3] [--old-steps 3] [--old-warmup 1] [--no-old] [--only a,b,c1,c,d,e1]
                                          [--out profiles/representatives_bench.json]
"""
import argparse
import gzip
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

X, P = 3, 0
HEAVY = {"b", "c", "d", "e1"}   # the old route of these takes seconds per round: --old-steps rounds of it
TRACE = re.compile(r"^\[hmk representatives\] threshold (-?\d+): (\d+) rounds, live edges behind each:((?: \d+)*)$", re.M)


def spread(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def stderr_of(call):
    """what the library writes to file descriptor 2 during call()"""
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            call()
        finally:
            os.dup2(keep, 2)
            os.close(keep)
        tmp.seek(0)
        return tmp.read().decode()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--old-steps", type=int, default=3)
    ap.add_argument("--old-warmup", type=int, default=1)
    ap.add_argument("--no-old", action="store_true", help="the new route alone (a kernel trace of it)")
    ap.add_argument("--only", default="a,b,c1,c,d,e1")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    only = set(args.only.split(","))
    import hammock_amd
    from hammock_amd.synth import synth_peptides
    with open(os.path.join(ROOT, "tests", "golden", "matrices.json")) as fh:
        M = np.asarray(json.load(fh)["matrices"]["blosum62"], dtype=np.int32)

    def synthetic(n):
        return lambda: synth_peptides(1, n, 12)

    def antibodies():
        with gzip.open(os.path.join(ROOT, "tests", "golden", "antibodies.fa.gz"), "rt") as fh:
            seqs = list(dict.fromkeys(line.strip() for line in fh if line.strip() and not line.startswith(">")))
        return hammock_amd.pack_sequences(seqs)

    def three_letters():
        rng = np.random.default_rng(77)   # (tools/bench_components.py's generator)
        seen, out = set(), []
        while len(out) < 17000:
            pep = rng.integers(0, 3, size=12, dtype=np.uint8)
            if pep.tobytes() not in seen:
                seen.add(pep.tobytes())
                out.append(pep)
        return np.concatenate(out), (np.arange(17001) * 12).astype(np.uint32)

    sets = {"1e5": synthetic(100_000), "antibodies": antibodies, "three_letters": three_letters, "1e6": synthetic(1_000_000)}
    workloads = [("a", "1e5", 20, 20), ("b", "1e5", 20, 40), ("c1", "antibodies", 20, 20), ("c", "antibodies", 20, 40),
                 ("d", "three_letters", 14, 14), ("e1", "1e6", 20, 20)]
    results, loaded = [], (None, None)
    for name, make, thr, hi in workloads:
        if name not in only:
            continue
        if loaded[0] != make:   # consecutive workloads on one set share the context
            res, off = sets[make]()
            ctx = hammock_amd.Context(M, device=0)
            ctx.set_sequences(residues=res, offsets=off)
            loaded = (make, ctx)
        ctx = loaded[1]
        n = len(off) - 1
        nl = hi - thr + 1
        new = {"kernel_ms": [], "select_ms": [], "wall_ms": []}
        comp = {"kernel_ms": [], "components_ms": []}
        old = {"kernel_ms": [], "host_select_ms": [], "wall_ms": []}
        warmup = args.warmup
        # the rounds [old_from, old_to) run the old route too; the timed ones among them are those from `warmup` on
        old_steps = 0 if args.no_old else min(args.steps, args.old_steps) if name in HEAVY else args.steps
        old_from = warmup - min(warmup, args.old_warmup) if name in HEAVY else 0
        old_from, old_to = (0, 0) if old_steps == 0 else (old_from, warmup + old_steps)
        for step in range(warmup + args.steps):
            t0 = time.perf_counter()
            levels, cov, near, nsc = ctx.representatives_shifted(X, P, thr, hi)
            wall = (time.perf_counter() - t0) * 1e3
            s = ctx.last_representatives_stats   # (the old route's host call replaces it)
            n_edges, rounds_total = int(s.n_edges), int(s.rounds_total)
            if step >= warmup:
                new["kernel_ms"].append(s.kernel_ms)
                new["select_ms"].append(s.select_ms)
                new["wall_ms"].append(wall)
            ctx.components_shifted(X, P, thr, hi, levels=nl > 1)
            if step >= warmup:
                comp["kernel_ms"].append(ctx.last_components_stats.kernel_ms)
                comp["components_ms"].append(ctx.last_components_stats.components_ms)
            if not old_from <= step < old_to:
                continue
            t0 = time.perf_counter()
            edges, ns = ctx.neighbors_shifted(X, P, thr, capacity=n_edges)
            t1 = time.perf_counter()
            for t in range(thr, hi + 1):   # the host selection once per wanted threshold
                _, ocov, onear, onsc = ctx.representatives_from_edges(edges, t)
                assert np.array_equal(ocov[0], cov[t - thr]) and np.array_equal(onear[0], near[t - thr]) and np.array_equal(onsc[0], nsc[t - thr])
                if n >= 500_000:   # (a long round: a sign of life)
                    print(f"[bench_representatives] {name}: old route, round {step}, threshold {t}: {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
            t2 = time.perf_counter()
            del edges
            if step >= warmup:
                old["kernel_ms"].append(ns.kernel_ms)
                old["host_select_ms"].append((t2 - t1) * 1e3)
                old["wall_ms"].append((t2 - t0) * 1e3)
        os.environ["HMK_GREEDY_TIMING"] = "1"
        try:
            text = stderr_of(lambda: ctx.representatives_shifted(X, P, thr, hi))
        finally:
            del os.environ["HMK_GREEDY_TIMING"]
        live = {int(t): [int(v) for v in counts.split()] for t, _, counts in TRACE.findall(text)}
        read = sum(int(e) + sum(live.get(thr + l, [])) for l, e in enumerate(levels["n_edges"]))
        row = {"workload": name, "n": n, "threshold": thr, "threshold_hi": hi, "n_edges": n_edges,
               "n_representatives": int(levels["n_representatives"][0]), "n_isolated": int(levels["n_isolated"][0]), "largest": int(levels["largest"][0]),
               "rounds_total": rounds_total, "rounds_by_threshold": [int(v) for v in levels["n_rounds"]],
               "representatives_by_threshold": [int(v) for v in levels["n_representatives"]],
               "steps": args.steps, "warmup": warmup, "old_steps": len(old["wall_ms"]), "old_warmup": warmup - old_from if old_to else 0,
               "new": {k: spread(v) for k, v in new.items()}, "components": {k: spread(v) for k, v in comp.items()},
               "old": {k: spread(v) for k, v in old.items() if v},
               "live_edges": {str(t): v for t, v in sorted(live.items())},
               "edges_read_ratio": read / max(int(levels["n_edges"].sum()), 1),
               "new_pcie_bytes": 12 * n * nl, "old_pcie_bytes": 8 * n_edges}
        results.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        doc = {}
        if os.path.exists(args.out):
            with open(args.out) as fh:
                doc = json.load(fh)
        kept = [r for r in doc.get("workloads", []) if r["workload"] not in {r["workload"] for r in results}]
        order = [w[0] for w in workloads]
        doc["workloads"] = sorted(kept + results, key=lambda r: order.index(r["workload"]))
        with open(args.out, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
