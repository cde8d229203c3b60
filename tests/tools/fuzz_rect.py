#!/usr/bin/env python3
"""Long randomized sweep of the rectangle and triangle plans against the oracle (tests/test_rect_parity.py runs 48 trials of the
same generator, sweep_trial; this runs as many as asked): per trial search_shifted, search_best_shifted, the triangle through
cluster_pairs_shifted at singleton slots when the matrix is symmetric, and every fourth trial search_local (under every matrix
kind: the tagged-max, plain striped and literal kernels are counted in the summary).
Usage: python tests/tools/fuzz_rect.py [trials] [seed] [first_trial]   (trials before first_trial only advance the random
stream; HMK_FUZZ_VERBOSE=1 prints every trial's parameters before it runs).  Exit status 1 with the failing trial's parameters."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import c_oracle  # noqa: E402
import test_rect_parity as T  # noqa: E402

trials = int(sys.argv[1]) if len(sys.argv) > 1 else 200
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
first = int(sys.argv[3]) if len(sys.argv) > 3 else 0
verbose = os.environ.get("HMK_FUZZ_VERBOSE") == "1"
with open(os.path.join(ROOT, "tests", "golden", "matrices.json")) as fh:
    matrices = {k: np.asarray(v, dtype=np.int32) for k, v in json.load(fh)["matrices"].items()}
rng = np.random.default_rng(seed)

used = {"u8": 0, "u16": 0, "direct": 0, "rows": 0}
ran = {"rectangles": 0, "triangles": 0, "local": 0, "local_kernels": {"tagged": 0, "plain": 0, "literal": 0}}
for trial in range(trials):
    t = T.sweep_trial(rng, trial, matrices, c_oracle)
    if trial < first:
        continue
    if verbose:
        print(json.dumps(T.sweep_describe(t)), flush=True)
    try:
        st = T.sweep_run(t, c_oracle)
    except Exception as e:   # a result that differs from the oracle's, or an error where the generator cannot produce one
        print(json.dumps({"FAIL": trial, "seed": seed, **T.sweep_describe(t), "error": type(e).__name__, "what": str(e)[:2000]}), flush=True)
        sys.exit(1)
    used["u8"] += st.classes_u8
    used["u16"] += st.classes_u16
    used["direct"] += st.classes_direct
    used["rows"] += st.classes_rows
    ran["rectangles"] += 1
    ran["triangles"] += t["symmetric"]
    ran["local"] += t["local"]
    if t["local"]:
        ran["local_kernels"][T.sweep_local_kernel(t)] += 1
    if trial % 25 == 24:
        print(f"trial {trial + 1}/{trials} ok, classes so far {used}", flush=True)
print(json.dumps({"trials": trials, "seed": seed, "first_trial": first, "all_equal": True, "classes": used, **ran}))
