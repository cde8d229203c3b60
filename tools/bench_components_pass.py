#!/usr/bin/env python3
"""bench_components_pass.py -- the scoring pass inside hmk_components_shifted beside hmk_neighbors_shifted's, on bench.py's 10^5
synthetic 12-mers (seed 1, BLOSUM62, max shift 3, penalty 0, threshold 20): kernel_ms (HIP events) of 10 calls after 3, both calls
alternating on one resident context.  TREE is the root of a built checkout, this one by default; a build of another commit (one
without the components call reports hmk_neighbors_shifted alone) is measured by naming its root, in a process of its own:

    python tools/bench_components_pass.py [TREE] [LABEL]      # one JSON line
"""
import json
import os
import sys

import numpy as np

root = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
import hammock_amd   # noqa: E402
from hammock_amd.synth import synth_peptides   # noqa: E402

with open(os.path.join(root, "tests", "golden", "matrices.json")) as fh:
    M = np.asarray(json.load(fh)["matrices"]["blosum62"], dtype=np.int32)
res, off = synth_peptides(1, 100_000, 12)
ctx = hammock_amd.Context(M, device=0)
ctx.set_sequences(residues=res, offsets=off)
cap = None
out = {"tree": sys.argv[2] if len(sys.argv) > 2 else root, "neighbors_kernel_ms": [], "components_kernel_ms": []}
for step in range(13):
    edges, stats = ctx.neighbors_shifted(3, 0, 20, capacity=cap)
    cap = edges.size
    if step >= 3:
        out["neighbors_kernel_ms"].append(stats.kernel_ms)
    if hasattr(ctx, "components_shifted"):
        ctx.components_shifted(3, 0, 20, levels=False)
        if step >= 3:
            out["components_kernel_ms"].append(ctx.last_components_stats.kernel_ms)
print(json.dumps(out))
