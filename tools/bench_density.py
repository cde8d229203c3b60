#!/usr/bin/env python3
"""bench_density.py -- density clustering (hmk_density_shifted) on one MI355X, beside the only other route to it:
hmk_neighbors_shifted to the host, then hmk_density_from_edges (the definition) per wanted threshold; and beside
hmk_components_shifted over the same range, the closest existing call: the difference is the degree step and the link step's
re-reads of the prefix.

BLOSUM62, max shift 3, shift penalty 0, min_neighbors 3, a resident context.  Workloads (--only picks some), those of DESIGN.md 5.16:
  a     bench.py's 10^5 synthetic 12-mers (seed 1), threshold 20, a single level
  b     the same, levels 20 ... 40
  c     the antibodies example (tests/golden/antibodies.fa.gz, its 74,041 distinct 12-mers), levels 20 ... 40
  d     17,000 peptides over three letters at threshold 14: about 94 % of the pairs are neighbours
  e1    10^6 synthetic 12-mers (seed 1), a single level at 20
The routes alternate in one process, --steps timed rounds after --warmup untimed ones: the new call, hmk_components_shifted, and in
--old-steps of the rounds (after --old-warmup untimed ones; 0: not at all) the old route, which scores once and runs the host
definition once per threshold; every output array of the two routes is asserted equal.  Per workload the median, minimum and maximum
of the new call's kernel_ms, density_ms and wall time, components_ms of the components call, the old route's pass and wall time;
per level the vertices that turned core and the edges the link step looked at against the edges >= t, read off the call's
HMK_GREEDY_TIMING lines in one extra untimed call (`link_looked_ratio` relates their sums).  The bytes over PCIe per call on both
routes are counted, not measured.  Prints one JSON line per workload; --out FILE keeps them under "workloads" of the JSON object in
FILE with the command that made them, replacing the rows of the same name and leaving the file's other sections as they are.

    python tools/bench_density.py [--steps 10] [--warmup 3] [--old-steps 3] [--old-warmup 1] [--no-old] [--only a,b,c,d,e1]
                                  [--min-neighbors 3] [--out profiles/density_bench.json]
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
TRACE = re.compile(r"^\[hmk density\] threshold (-?\d+): (\d+) vertices turned core, the link step looked at (\d+) of (\d+) edges$", re.M)


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
    ap.add_argument("--only", default="a,b,c,d,e1")
    ap.add_argument("--min-neighbors", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    only = set(args.only.split(","))
    mn = args.min_neighbors
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
    workloads = [("a", "1e5", 20, 20), ("b", "1e5", 20, 40), ("c", "antibodies", 20, 40), ("d", "three_letters", 14, 14), ("e1", "1e6", 20, 20)]
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
        new = {"kernel_ms": [], "density_ms": [], "wall_ms": []}
        comp = {"kernel_ms": [], "components_ms": []}
        old = {"kernel_ms": [], "host_density_ms": [], "wall_ms": []}
        warmup = args.warmup
        # the rounds [old_from, old_to) run the old route too; the timed ones among them are those from `warmup` on
        old_steps = 0 if args.no_old else min(args.steps, args.old_steps) if name in HEAVY else args.steps
        old_from = warmup - min(warmup, args.old_warmup) if name in HEAVY else 0
        old_from, old_to = (0, 0) if old_steps == 0 else (old_from, warmup + old_steps)
        for step in range(warmup + args.steps):
            t0 = time.perf_counter()
            levels, cluster, degree, anchor = ctx.density_shifted(X, P, thr, hi, mn)
            wall = (time.perf_counter() - t0) * 1e3
            s = ctx.last_density_stats   # (the old route's host call replaces it)
            n_edges = int(s.n_edges)
            if step >= warmup:
                new["kernel_ms"].append(s.kernel_ms)
                new["density_ms"].append(s.density_ms)
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
            for t in range(thr, hi + 1):   # the host definition once per wanted threshold
                _, ocl, odeg, oan = ctx.density_from_edges(edges, t, min_neighbors=mn)
                assert np.array_equal(ocl[0], cluster[t - thr]) and np.array_equal(odeg[0], degree[t - thr]) and np.array_equal(oan[0], anchor[t - thr])
                if n >= 500_000:   # (a long round: a sign of life)
                    print(f"[bench_density] {name}: old route, round {step}, threshold {t}: {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
            t2 = time.perf_counter()
            del edges
            if step >= warmup:
                old["kernel_ms"].append(ns.kernel_ms)
                old["host_density_ms"].append((t2 - t1) * 1e3)
                old["wall_ms"].append((t2 - t0) * 1e3)
        os.environ["HMK_GREEDY_TIMING"] = "1"
        try:
            text = stderr_of(lambda: ctx.density_shifted(X, P, thr, hi, mn))
        finally:
            del os.environ["HMK_GREEDY_TIMING"]
        trace = sorted((int(t), int(c), int(k), int(e)) for t, c, k, e in TRACE.findall(text))
        row = {"workload": name, "n": n, "threshold": thr, "threshold_hi": hi, "min_neighbors": mn, "n_edges": n_edges,
               "by_threshold": {f: [int(v) for v in levels[f]] for f in ("n_edges", "n_core", "n_border", "n_noise", "n_clusters", "largest")},
               "steps": args.steps, "warmup": warmup, "old_steps": len(old["wall_ms"]), "old_warmup": warmup - old_from if old_to else 0,
               "new": {k: spread(v) for k, v in new.items()}, "components": {k: spread(v) for k, v in comp.items()},
               "old": {k: spread(v) for k, v in old.items() if v},
               "turned_core": [c for _, c, _, _ in trace], "link_looked": [k for _, _, k, _ in trace], "prefix": [e for _, _, _, e in trace],
               "link_looked_ratio": sum(k for _, _, k, _ in trace) / max(sum(e for _, _, _, e in trace), 1),
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
        for r in results:
            r["command"] = "python tools/bench_density.py " + " ".join(sys.argv[1:])
        doc["workloads"] = sorted(kept + results, key=lambda r: order.index(r["workload"]))
        with open(args.out, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
