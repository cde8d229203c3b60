#!/usr/bin/env python3
"""bench_scan.py -- peptides scanned along long targets (hmk_scan_shifted) on one MI355X.  The product path only, no oracle.

BLOSUM62, max shift 3, shift penalty 0, threshold 20, pair mode.  Every call is made with capacity 0, so nothing but the counters
travels back: stats.kernel_ms (HIP events around scoring + reduction) is what is timed, median of --steps calls after --warmup untimed
ones, with the spread (min, max).  Cases:
  a   10^5 synthetic 12-mers x one 1,000-residue target
  b   10^4 12-mers x 2 x 10^4 targets of about 500 residues (10^7 residues, 10^11 windows)
  c   the antibodies example's unique peptides x a's target
  b'  10^4 12-mers x 4 x 10^6 target residues, against what the library could do before: the interior windows cut into 12-mers on
      the host, uploaded as sequences, hmk_search_shifted at max shift 0 over them.  With p = 0 both give the same interior window
      hits, which is asserted; the two calls alternate.
Each of a, b, c also runs under HMK_NO_SCAN_PACKED=1 (the literal form for everything; fewer steps, it is slow).
frac_lds_ideal: m bytes of LDS per window (one 8-byte table read per position serves 8 peptides) over 256 B/clk/CU x 256 CUs x
2.4 GHz.  LDS is the bound taken because the table reads are the only per-window traffic: the target's residues are read once per
window and 64 peptides, the tables once per 1,024 windows.  Prints one JSON line.

    python tools/bench_scan.py [--steps 10] [--warmup 3] [--cases a,b,c,bp]
"""
import argparse
import collections
import ctypes as C
import gzip
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LDS_PEAK_BS = 256 * 256 * 2.4e9
X, P, THR = 3, 0, 20
ALPHABET = "ARNDCQEGHILKMFPSTWYVBZX*"


def antibodies():
    counts = collections.Counter()
    with gzip.open(os.path.join(ROOT, "tests", "golden", "antibodies.fa.gz"), "rt") as fh:
        for line in fh:
            line = line.strip().upper()
            if line and not line.startswith(">") and len(line) <= 32 and all(ch in ALPHABET for ch in line):
                counts[line] += 1
    seqs = list(counts)
    return seqs, np.asarray([counts[s] for s in seqs], dtype=np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", default="a,b,c,bp")
    args = ap.parse_args()
    cases = set(args.cases.split(","))
    import hammock_amd
    from hammock_amd import _native as N
    from hammock_amd.synth import synth_peptides
    with open(os.path.join(ROOT, "tests", "golden", "matrices.json")) as fh:
        M = np.asarray(json.load(fh)["matrices"]["blosum62"], dtype=np.int32)
    ctx = hammock_amd.Context(M, device=0)
    rng = np.random.default_rng(3)

    def targets_of(lengths):
        off = np.zeros(len(lengths) + 1, dtype=np.uint64)
        off[1:] = np.cumsum(lengths)
        return rng.integers(0, 20, size=int(off[-1]), dtype=np.uint8), off

    def scan_counters(nq, nt, x=X, flags=0):
        st = N.ScanStats()
        rc = N.lib.hmk_scan_shifted(ctx._h, 0, nq, 0, nt, x, P, THR, flags, None, 0, None, None, C.byref(st))
        if rc not in (N.HMK_OK, N.HMK_ERR_CAPACITY):
            ctx._raise(rc)
        return st

    def measure(call, steps, warmup):
        for _ in range(warmup):
            call()
        ms, last = [], None
        for _ in range(steps):
            last = call()
            ms.append(float(last.kernel_ms))
        return {"kernel_ms": float(np.median(ms)), "min_ms": min(ms), "max_ms": max(ms)}, last

    def scan_case(name, nq, nt, mean_m):
        run = {"case": name, "queries": nq, "targets": nt}
        for form, env, steps, warmup in (("packed", None, args.steps, args.warmup), ("literal", "1", max(2, args.steps // 4), 1)):
            if env:
                os.environ["HMK_NO_SCAN_PACKED"] = env
            try:
                t, st = measure(lambda: scan_counters(nq, nt), steps, warmup)
            finally:
                os.environ.pop("HMK_NO_SCAN_PACKED", None)
            ideal_ms = st.windows_scored * mean_m / LDS_PEAK_BS * 1e3
            t.update({"windows": int(st.windows_scored), "windows_packed": int(st.windows_packed), "windows_per_s": st.windows_scored / (t["kernel_ms"] * 1e-3),
                      "window_hits": int(st.window_hits), "hits": int(st.n_hits), "lds_ideal_ms": ideal_ms, "frac_lds_ideal": ideal_ms / t["kernel_ms"],
                      "launches": int(st.launches)})
            run[form] = t
        run["packed_faster_than_literal"] = run["packed"]["kernel_ms"] < run["literal"]["kernel_ms"]
        return run

    out = {"what": f"scan of peptides along targets, BLOSUM62, X={X}, p={P}, threshold {THR}, pair mode", "runs": []}
    res, off = synth_peptides(1, 100_000, 12)
    one_res, one_off = targets_of([1000])
    if "a" in cases:
        ctx.set_sequences(residues=res, offsets=off)
        ctx.set_targets(residues=one_res, offsets=one_off)
        out["runs"].append(scan_case("a", 100_000, 1, 12))
    if "b" in cases:
        ctx.set_sequences(residues=res[:int(off[10_000])], offsets=off[:10_001])
        many_res, many_off = targets_of(rng.integers(400, 601, size=20_000))
        ctx.set_targets(residues=many_res, offsets=many_off)
        out["runs"].append(scan_case("b", 10_000, 20_000, 12))
    if "c" in cases:
        seqs, sizes = antibodies()
        ctx.set_sequences(seqs, sizes=sizes)
        ctx.set_targets(residues=one_res, offsets=one_off)
        out["runs"].append(scan_case("c", len(seqs), 1, float(np.mean([len(s) for s in seqs]))))
    if "bp" in cases:
        nq, m = 10_000, 12
        lengths = rng.integers(400, 601, size=8_000)
        tres, toff = targets_of(lengths)
        ctx.set_targets(residues=tres, offsets=toff)
        # the interior windows as sequences: target t's window s is sequence nq + first[t] + s
        nwin = lengths - m + 1
        first = np.concatenate([[0], np.cumsum(nwin)])
        starts = np.concatenate([int(toff[t]) + np.arange(nwin[t]) for t in range(len(lengths))])
        cut = tres[starts[:, None] + np.arange(m)[None, :]].ravel()
        all_res = np.concatenate([res[:int(off[nq])], cut])
        all_off = np.concatenate([off[:nq + 1], int(off[nq]) + m * np.arange(1, len(starts) + 1, dtype=np.uint64)]).astype(np.uint32)
        n = nq + len(starts)
        ctx.set_sequences(residues=all_res, offsets=all_off)

        def search_counters():
            st = N.NeighborStats()
            ne = C.c_uint64(0)
            rc = N.lib.hmk_search_shifted(ctx._h, 0, nq, nq, n, 0, P, THR, None, 0, C.byref(ne), C.byref(st))
            if rc not in (N.HMK_OK, N.HMK_ERR_CAPACITY):
                ctx._raise(rc)
            return st

        for _ in range(args.warmup):
            scan_counters(nq, len(lengths))
            search_counters()
        scan_ms, search_ms = [], []
        for _ in range(args.steps):   # the two alternate
            scan_ms.append(float(scan_counters(nq, len(lengths)).kernel_ms))
            search_ms.append(float(search_counters().kernel_ms))
        # the same interior window hits
        hits, st = ctx.scan_shifted(0, nq, 0, len(lengths), X, P, THR, all_windows=True)
        d = lengths[hits["target"]] - m
        inner = hits[(hits["offset"] >= 0) & (hits["offset"] <= d)]
        mine = np.sort(hammock_amd.pack_edges(nq + first[inner["target"]] + inner["offset"], inner["query"], inner["score"]))
        edges, _ = ctx.search_shifted(0, nq, nq, n, 0, P, THR)
        assert np.array_equal(mine, np.sort(edges)), "the scan's interior window hits differ from the materialised search's"
        spread = (max(scan_ms) - min(scan_ms)) + (max(search_ms) - min(search_ms))
        out["runs"].append({"case": "b'", "queries": nq, "target_residues": int(toff[-1]), "materialised_sequences": int(len(starts)),
                            "scan": {"kernel_ms": float(np.median(scan_ms)), "min_ms": min(scan_ms), "max_ms": max(scan_ms)},
                            "materialised_search": {"kernel_ms": float(np.median(search_ms)), "min_ms": min(search_ms), "max_ms": max(search_ms)},
                            "interior_window_hits": int(len(inner)), "equal": True,
                            "scan_not_above_search": float(np.median(scan_ms)) <= float(np.median(search_ms)) + spread})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
