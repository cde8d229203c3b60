"""The argument checks of the five calls that answer "at one threshold or a range of them" from one neighbour pass -- components,
greedy sweep, representatives, density, orders -- in every form each call has: the scoring call, the host `_from_edges` form and
the `_from_edges_dev` form (orders has no device-edges form and no range).  Everything runs on a host-only context (device = -1),
through the C ABI, so every refusal here is one the library makes before it looks at a device, and the pointers handed to the
device forms are never read.

Each case is (call, form, situation) -> (status, hmk_last_error text).  The expected values below were recorded from the library
as it stood before the calls' shared checks moved into hmk_levels.cpp; the test asserts them exactly, so a check that changes its
wording, or its place in the order of a call's checks, fails here.  Where a call succeeds only the status is compared (the text
of the last error is then whatever an earlier call left).
"""
import ctypes as C

import numpy as np
import pytest

from conftest import GOLDEN  # noqa: F401  (conftest puts the repository on sys.path)

import hammock_amd
from hammock_amd import _native as N
from hammock_amd.synth import synth_peptides
from test_components import matrix

OK, BAD_ARG, DEVICE = 0, N.HMK_ERR_BAD_ARG, N.HMK_ERR_DEVICE
N_SEQ = 10
P_U32, P_I32, P_U64 = C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_uint64)
DUMMY = 4096   # a non-null address that no check may read

CALLS = ("components", "sweep", "representatives", "density", "orders")
FORMS = {"components": ("pass", "host", "dev"), "sweep": ("pass", "host", "dev"), "representatives": ("pass", "host", "dev"),
         "density": ("pass", "host", "dev"), "orders": ("pass", "host")}
FUNCTIONS = {
    "components": ("hmk_components_shifted", "hmk_components_from_edges", "hmk_components_from_edges_dev"),
    "sweep": ("hmk_greedy_sweep", "hmk_greedy_sweep_from_edges", "hmk_greedy_sweep_from_edges_dev"),
    "representatives": ("hmk_representatives_shifted", "hmk_representatives_from_edges", "hmk_representatives_from_edges_dev"),
    "density": ("hmk_density_shifted", "hmk_density_from_edges", "hmk_density_from_edges_dev"),
    "orders": ("hmk_greedy_orders", "hmk_greedy_orders_from_edges"),
}


def context(kind):
    """kind: "set" (N_SEQ peptides), "empty" (no sequences), "asym" (N_SEQ peptides under an asymmetric matrix); all host-only"""
    M = matrix().copy()
    if kind == "asym":
        M[3, 5] += 1
    ctx = hammock_amd.Context(M, device=-1)
    if kind != "empty":
        res, off = synth_peptides(40, N_SEQ, 12)
        ctx.set_sequences(residues=res, offsets=off)
    return ctx


def run(call, form, ctx, thr, hi, edges=None, n_edges=0, outputs=True):
    """One C call -> (status, last error text or None).  edges: a uint64 array (host form), an address (device form) or None."""
    n, rows = max(ctx.n, 1), 256
    fn = getattr(N.lib, FUNCTIONS[call][("pass", "host", "dev").index(form)])
    keep = []   # the buffers stay alive until the call has returned

    def u32(count):
        keep.append(np.zeros(count, dtype=np.uint32))
        return keep[-1].ctypes.data_as(P_U32) if outputs else None

    def i32(count):
        keep.append(np.zeros(count, dtype=np.int32))
        return keep[-1].ctypes.data_as(P_I32) if outputs else None

    def records(kind):
        keep.append((kind * rows)())
        return keep[-1] if outputs else None

    if form == "pass":
        head = [3, 0]
    elif form == "host":
        head = [edges.ctypes.data_as(P_U64) if edges is not None else None, n_edges]
    else:
        head = [C.c_void_p(edges) if edges is not None else None, n_edges]
    if call == "components":
        stats = N.ComponentsStats()
        st = fn(ctx._h, *head, thr, hi, u32(n), records(N.ComponentLevel), C.byref(stats))
    elif call == "sweep":
        stats = N.GreedySweepStats()
        sym = [] if form == "pass" else [1]
        st = fn(ctx._h, *head, *sym, thr, hi, 10, i32(rows * n), i32(rows * n), i32(rows * n), records(N.GreedyLevel), C.byref(stats))
    elif call == "representatives":
        stats = N.RepresentativesStats()
        st = fn(ctx._h, *head, thr, hi, u32(rows * n), u32(rows * n), i32(rows * n), records(N.RepresentativeLevel), C.byref(stats))
    elif call == "density":
        stats = N.DensityStats()
        st = fn(ctx._h, *head, thr, hi, 3, u32(rows * n), u32(rows * n), u32(rows * n), records(N.DensityLevel), C.byref(stats))
    else:   # orders: one threshold, two orders (the identity twice)
        stats = N.GreedyOrdersStats()
        orders = np.tile(np.arange(ctx.n, dtype=np.uint32), 2)
        need = C.c_uint64(0)
        st = fn(ctx._h, *head, thr, 10, orders.ctypes.data_as(P_U32), 2, 0, i32(2 * n), i32(2 * n), i32(2 * n), records(N.GreedyOrder),
                u32(n), u32(n), u32(n), None, 0, C.byref(need), C.byref(stats))
    text = N.lib.hmk_last_error(ctx._h).decode() if st != OK else None
    return st, text


def bad_edge():
    return hammock_amd.pack_edges(np.asarray([0]), np.asarray([N_SEQ + 5]), np.asarray([25]))


def situations(call, form):
    """-> {situation: (status, text)} of one call and form"""
    out = {}
    ranged = call != "orders"
    edged = form != "pass"
    one = hammock_amd.pack_edges(np.asarray([0]), np.asarray([1]), np.asarray([25])) if form == "host" else DUMMY
    if ranged:
        out["hi_below_thr"] = run(call, form, context("set"), 20, 19)
        out["257_levels"] = run(call, form, context("set"), 0, 256)
        out["hi_32768"] = run(call, form, context("set"), 32768 - 255, 32768)
        out["hi_below_thr_before_null_outputs"] = run(call, form, context("set"), 20, 19, outputs=False)
        out["257_levels_before_asymmetric"] = run(call, form, context("asym"), 0, 256)
    out["null_outputs"] = run(call, form, context("set"), 20, 24, outputs=False)
    out["null_outputs_empty_set"] = run(call, form, context("empty"), 20, 24, outputs=False)
    out["asymmetric"] = run(call, form, context("asym"), 20, 24)
    out["asymmetric_after_null_outputs"] = run(call, form, context("asym"), 20, 24, outputs=False)
    out["set_no_edges"] = run(call, form, context("set"), 20, 24)
    out["empty_set"] = run(call, form, context("empty"), 20, 24)
    if edged:
        out["null_edges"] = run(call, form, context("set"), 20, 24, None, 1)
        out["null_edges_empty_set"] = run(call, form, context("empty"), 20, 24, None, 1)
        out["null_edges_after_range"] = run(call, form, context("set"), 20, 19, None, 1) if ranged else None
        out["set_with_edges_given"] = run(call, form, context("set"), 20, 24, one, 1)
    if form == "dev":
        out["above_2^41_edges"] = run(call, form, context("set"), 20, 24, DUMMY, (1 << 41) + 1)
        out["2^41_edges"] = run(call, form, context("set"), 20, 24, DUMMY, 1 << 41)
        out["above_2^41_edges_empty_set"] = run(call, form, context("empty"), 20, 24, DUMMY, (1 << 41) + 1)
        out["edges_given_empty_set"] = run(call, form, context("empty"), 20, 24, DUMMY, 1)
    if form == "host":
        out["bad_edge"] = run(call, form, context("set"), 20, 24, bad_edge(), 1)
        out["bad_edge_empty_set"] = run(call, form, context("empty"), 20, 24, bad_edge(), 1)
    return {k: v for k, v in out.items() if v is not None}


RANGE_LO = "threshold_hi is below threshold"
RANGE_256 = "at most 256 levels per call: threshold_hi - threshold <= 255"
RANGE_I16 = "threshold_hi is above 32767, the highest score an edge holds"
NO_GPU = "this context has no GPU (created with device = -1); scoring has no CPU fallback"
NULL_LIST, NULL_BUFFER, TOO_MANY = "null edge list", "null edge buffer", "more than 2^41 edges"
BAD_EDGE = "edge list references a sequence outside [0, n) or a self pair"
NULL_OUT = {
    "components": "null outputs (component and levels)",
    "sweep": "null outputs (levels, cluster_id, result_order and member_rank)",
    "representatives": "null outputs (levels, covered_by, nearest and nearest_score)",
    "density": "null outputs (levels, cluster, anchor and degree)",
    "orders": "null outputs (the rows, per_order, the partner counts, consensus and support_edges)",
}
ASYM = {
    "components": "components need a symmetric scoring matrix: a ~ b must not depend on which of the two is seq1",
    "representatives": "representatives need a symmetric scoring matrix: a ~ b must not depend on which of the two is seq1",
    "density": "density clustering needs a symmetric scoring matrix: a ~ b must not depend on which of the two is seq1",
    "orders": "orders need a symmetric scoring matrix: the pass scores one orientation of a pair, and which of the two is seq1 would "
              "depend on the order",
}

EXPECTED = {}   # filled below: (call, form) -> {situation: (status, text)}


def _expect():
    ok, gpu = (OK, None), (DEVICE, NO_GPU)
    for call in CALLS:
        for form in FORMS[call]:
            e = {}
            host, dev, scoring = form == "host", form == "dev", form == "pass"
            needs_gpu = ok if host else gpu
            if call != "orders":
                e["hi_below_thr"] = e["hi_below_thr_before_null_outputs"] = (BAD_ARG, RANGE_LO)
                e["257_levels"] = e["257_levels_before_asymmetric"] = (BAD_ARG, RANGE_256)
                e["hi_32768"] = needs_gpu if call == "components" else (BAD_ARG, RANGE_I16)
            e["null_outputs"] = e["asymmetric_after_null_outputs"] = (BAD_ARG, NULL_OUT[call])
            # the refusal of an asymmetric matrix: the scoring call of components, representatives and density; both forms of orders
            e["asymmetric"] = (BAD_ARG, ASYM[call]) if call == "orders" or (scoring and call != "sweep") else needs_gpu
            e["set_no_edges"] = needs_gpu
            # no sequences: components asks for the device first, the others answer first; no outputs are needed for no sequences
            e["empty_set"] = e["null_outputs_empty_set"] = gpu if call == "components" and not host else ok
            if not scoring:
                null = (BAD_ARG, NULL_LIST if host else NULL_BUFFER)
                e["null_edges"] = e["null_edges_empty_set"] = null
                if call != "orders":
                    e["null_edges_after_range"] = (BAD_ARG, RANGE_LO)
                e["set_with_edges_given"] = needs_gpu
            if dev:
                e["above_2^41_edges"] = e["above_2^41_edges_empty_set"] = (BAD_ARG, TOO_MANY)
                e["2^41_edges"] = gpu
                e["edges_given_empty_set"] = gpu if call == "components" else ok
            if host:
                e["bad_edge"] = (BAD_ARG, BAD_EDGE)
                # no sequences and an edge that names one: sweep answers for the empty set first, the others read the edges first
                e["bad_edge_empty_set"] = ok if call == "sweep" else (BAD_ARG, BAD_EDGE)
            EXPECTED[(call, form)] = e


_expect()


@pytest.mark.parametrize("call,form", [(c, f) for c in CALLS for f in FORMS[c]], ids=lambda v: v)
def test_every_check_of_every_form_gives_its_status_and_text(call, form):
    got, want = situations(call, form), EXPECTED[(call, form)]
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], f"{call} {form} {name}"


def test_the_cases_cover_what_they_are_meant_to():
    """every range call refuses the three range mistakes in every form (components accepts threshold_hi = 32768); every form with
    an edge argument refuses a null one; every device-edges form refuses more than 2^41 edges; the four calls with a refusal of
    an asymmetric matrix make it; the empty set is answered by every form, with or without a device as the call has it"""
    for call in CALLS:
        for form in FORMS[call]:
            e = EXPECTED[(call, form)]
            if call != "orders":
                assert e["hi_below_thr"][1] == RANGE_LO and e["257_levels"][1] == RANGE_256
                assert (e["hi_32768"][1] == RANGE_I16) == (call != "components")
            assert e["null_outputs"][1] == NULL_OUT[call]
            if form != "pass":
                assert e["null_edges"][1] == (NULL_LIST if form == "host" else NULL_BUFFER)
            if form == "dev":
                assert e["above_2^41_edges"][1] == TOO_MANY
            assert "empty_set" in e
    assert sorted(c for c in CALLS if EXPECTED[(c, "pass")]["asymmetric"][0] == BAD_ARG) == sorted(ASYM)
