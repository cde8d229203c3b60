#!/usr/bin/env python3
"""bench_components.py -- connected components of the neighbour graph (hmk_components_shifted) on one MI355X, beside the only
other route to them: hmk_neighbors_shifted to the host, then hmk_components_from_edges (a host union-find) per wanted threshold.

BLOSUM62, max shift 3, shift penalty 0, a resident context.  Workloads (--only picks some):
  a     bench.py's 10^5 synthetic 12-mers (seed 1), threshold 20, a single level
  b     the same, levels 20 ... 40
  c1/c  the antibodies example (tests/golden/antibodies.fa.gz, its 74,041 distinct 12-mers), a single level at 20 / levels 20 ... 40
  d     17,000 peptides over three letters at threshold 14: about 94 % of the pairs are neighbours, one component, every find()
        ends at one root
  e1/e  10^6 synthetic 12-mers (seed 1), a single level at 20 / levels 20 ... 40
The two routes alternate in one process, --steps timed rounds after --warmup untimed ones.  The old route of b, c, d, e1 and e takes
seconds to minutes per round (21 host union-finds, or 1 to 10 GB over PCIe): it runs in --old-warmup untimed and --old-steps timed
rounds only (0: not at all), each right behind a call of the new route.  The old route of a level scan scores once and runs the
host union-find once per threshold.  Per workload the median, minimum and maximum of the new call's kernel_ms, components_ms and wall time, the old
route's pass (kernel_ms of hmk_neighbors_shifted) and wall time; the bytes over PCIe per call on both routes are counted, not
measured.  Prints one JSON line per workload; --out FILE keeps them under "workloads" of the JSON object in FILE, replacing the
rows of the same name and leaving the file's other sections (DESIGN.md 5.16 says where they come from) as they are.

    python tools/bench_components.py [--steps 10] [--warmup 3] [--old-steps 3] [--old-warmup 1] [--no-old] [--only a,b,c1,c,d,e1,e]
                                     [--out profiles/components_bench.json]
"""
import argparse
import gzip
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

X, P = 3, 0
HEAVY = {"b", "c", "d", "e1", "e"}   # the old route of these takes seconds per round: --old-steps rounds of it


def spread(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--old-steps", type=int, default=3)
    ap.add_argument("--old-warmup", type=int, default=1)
    ap.add_argument("--no-old", action="store_true", help="the new route alone (a kernel trace of it)")
    ap.add_argument("--only", default="a,b,c1,c,d,e1,e")
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
        rng = np.random.default_rng(77)   # (tests/test_gpu_parity.py: test_greedy_band_rows_beyond_the_intersection_table's generator)
        seen, out = set(), []
        while len(out) < 17000:
            pep = rng.integers(0, 3, size=12, dtype=np.uint8)
            if pep.tobytes() not in seen:
                seen.add(pep.tobytes())
                out.append(pep)
        return np.concatenate(out), (np.arange(17001) * 12).astype(np.uint32)

    sets = {"1e5": synthetic(100_000), "antibodies": antibodies, "three_letters": three_letters, "1e6": synthetic(1_000_000)}
    workloads = [("a", "1e5", 20, 20), ("b", "1e5", 20, 40), ("c1", "antibodies", 20, 20), ("c", "antibodies", 20, 40),
                 ("d", "three_letters", 14, 14), ("e1", "1e6", 20, 20), ("e", "1e6", 20, 40)]
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
        single = hi == thr
        new = {"kernel_ms": [], "components_ms": [], "wall_ms": []}
        old = {"kernel_ms": [], "wall_ms": []}
        warmup = args.warmup
        # the rounds [old_from, old_to) run the old route too; the timed ones among them are those from `warmup` on
        old_steps = 0 if args.no_old else min(args.steps, args.old_steps) if name in HEAVY else args.steps
        old_from = warmup - min(warmup, args.old_warmup) if name in HEAVY else 0
        old_from, old_to = (0, 0) if old_steps == 0 else (old_from, warmup + old_steps)
        n_edges, levels, comp = 0, None, None
        for step in range(warmup + args.steps):
            t0 = time.perf_counter()
            comp, levels = ctx.components_shifted(X, P, thr, hi, levels=not single)
            wall = (time.perf_counter() - t0) * 1e3
            s = ctx.last_components_stats   # (the old route's host call replaces it)
            n_edges = int(s.n_edges)
            if step >= warmup:
                new["kernel_ms"].append(s.kernel_ms)
                new["components_ms"].append(s.components_ms)
                new["wall_ms"].append(wall)
            if not old_from <= step < old_to:
                continue
            t0 = time.perf_counter()
            edges, ns = ctx.neighbors_shifted(X, P, thr, capacity=n_edges)
            ocomp = None
            for t in range(thr, hi + 1):   # the host union-find once per wanted threshold
                c, _ = ctx.components_from_edges(edges, t)
                ocomp = c if ocomp is None else ocomp
                if n >= 500_000:   # (minutes per round: a sign of life)
                    print(f"[bench_components] {name}: old route, round {step}, threshold {t}: {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
            wall = (time.perf_counter() - t0) * 1e3
            assert np.array_equal(ocomp, comp)
            del edges
            if step >= warmup:
                old["kernel_ms"].append(ns.kernel_ms)
                old["wall_ms"].append(wall)
        row = {"workload": name, "n": n, "threshold": thr, "threshold_hi": hi, "n_edges": n_edges, "n_components": int(s.n_components),
               "n_singletons": int(s.n_singletons), "largest": int(s.largest), "steps": args.steps, "warmup": warmup, "old_steps": len(old["wall_ms"]), "old_warmup": warmup - old_from if old_to else 0,
               "new": {k: spread(v) for k, v in new.items()}, "old": {k: spread(v) for k, v in old.items() if v},
               "new_pcie_bytes": 4 * n + (0 if single else 24 * (hi - thr + 1)), "old_pcie_bytes": 8 * n_edges}
        if levels is not None:
            row["components_by_threshold"] = [int(v) for v in levels["n_components"]]
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
