"""The argument checks of the calls that take clusters as "members [r0, r1) with a slot per member" -- the linkage, the split (its
scoring form and its `_from_edges` form), the separation, the alignment and the profile of given clusters, and the pairs between
given clusters (hmk_cluster_pairs_shifted, which takes no cluster ids either).  Everything runs on a host-only context
(device = -1), through the C ABI, so every refusal here is one the library makes before it looks at a device.

Each case is (call, situation) -> (status, hmk_last_error text).  The expected values below were recorded from the library as it
stood before the calls' shared host steps moved into hmk_slots.cpp; the test asserts them exactly, so a check that changes its
wording, or its place in the order of a call's checks, fails here.  The situations with two faults at once pin that order: the
answer names the check that comes first.  Where a call succeeds only the status is compared (the text of the last error is then
whatever an earlier call left).
"""
import ctypes as C
import math

import numpy as np
import pytest

from conftest import GOLDEN  # noqa: F401  (conftest puts the repository on sys.path)

import hammock_amd
from hammock_amd import _native as N
from hammock_amd.synth import synth_peptides
from test_components import matrix

N_SEQ = 10
MC = [0, 0, 2, 1, 2, 2, 0, 2, 0, 2]   # three slots: of four, of one and of five members
N_BIG = 46400                         # one slot of that many members holds more than 2^30 pairs
CALLS = ("linkage", "split", "split_from_edges", "separation", "align", "profile", "pairs")
FUNCTIONS = {"linkage": "hmk_cluster_linkage_shifted", "split": "hmk_clinkage_split", "split_from_edges": "hmk_clinkage_split_from_edges",
             "separation": "hmk_cluster_separation_shifted", "align": "hmk_cluster_align_shifted", "profile": "hmk_cluster_profile",
             "pairs": "hmk_cluster_pairs_shifted"}
CTYPES = {"u8": (np.uint8, C.c_uint8), "u32": (np.uint32, C.c_uint32), "i32": (np.int32, C.c_int32), "u64": (np.uint64, C.c_uint64),
          "i64": (np.int64, C.c_int64), "f64": (np.float64, C.c_double)}
# the calls' output arrays in argument order: (name, element type); every array is made large enough for members and slots alike
OUTPUTS = {
    "linkage": (("min_score", "i32"), ("min_a", "u32"), ("min_b", "u32"), ("n_below", "u64"), ("member_min", "i32"), ("member_below", "u32")),
    "split": (("split_cluster", "u32"), ("n_parts", "u32"), ("part_id", "i32"), ("member_rank", "i32"), ("part_order", "i32"),
              ("part_start", "u32")),
    "separation": (("own_sum", "i64"), ("near_sum", "i64"), ("near_cluster", "u32"), ("misplaced", "u8"), ("cluster_misplaced", "u32"),
                   ("cluster_own_sum", "i64")),
    "align": (("center", "u32"), ("center_sum", "i64"), ("width", "u32"), ("member_sum", "i64"), ("center_score", "i32"), ("shift", "i32"),
              ("column", "u32")),
    "profile": (("width", "u32"), ("n_conserved", "u32"), ("n_match", "u32"), ("passes", "u8"), ("kld_match_mean", "f64"),
                ("kld_all_mean", "f64"), ("col_start", "u64"), ("counts", "u32"), ("ic", "f64"), ("col_flags", "u8"), ("kld_match", "f64"),
                ("kld_all", "f64")),
    "pairs": (("pairs", "u64"), ("n_pairs", "u64")),
}
OUTPUTS["split_from_edges"] = OUTPUTS["split"]
STATS = {"linkage": N.LinkageStats, "split": N.SplitStats, "split_from_edges": N.SplitStats, "separation": N.SeparationStats,
         "align": N.AlignStats, "profile": N.ProfileStats, "pairs": N.MergeStats}
# the group of outputs each call asks for first
FIRST_GROUP = {"linkage": ("min_score",), "split": ("split_cluster",), "split_from_edges": ("split_cluster",), "separation": ("own_sum",),
               "align": ("center",), "profile": ("width",), "pairs": ("n_pairs",)}


def context(kind):
    """kind: "set" (N_SEQ 12-mers), "asym" (the same under an asymmetric matrix), "odd" (the set and one peptide that holds a residue
    outside the 20 amino acids), "big" (N_BIG 12-mers); all host-only"""
    M = matrix().copy()
    if kind == "asym":
        M[3, 5] += 1
    ctx = hammock_amd.Context(M, device=-1)
    res, off = synth_peptides(40, N_BIG if kind == "big" else N_SEQ, 12)
    if kind == "odd":
        peps = [res[off[i]:off[i + 1]] for i in range(N_SEQ)] + [np.array([0, 1, 20, 3], dtype=np.uint8)]
        res, off = hammock_amd.pack_sequences(peps)
    ctx.set_sequences(residues=res, offsets=off)
    return ctx


def profile_params(**changed):
    P = hammock_amd.profile_params(np.full((20, 20), 0.0025))
    for k, v in changed.items():
        if k in ("frequency", "background"):
            getattr(P, k)[v[0]] = v[1]
        else:
            setattr(P, k, v)
    return P


def run(call, kind="set", r0=0, r1=N_SEQ, mc=MC, ncl=3, X=3, p=0, thr=20, null=(), column=0, params=True, stats=True, cap=64,
        null_edges=False, **changed):
    """One C call -> (status name, last error text or None).  null: the outputs passed as null pointers ("all": every one);
    column: the profile's placement (a number for every member, a list, or None); changed: the profile's parameters that differ."""
    ctx = context(kind)
    nm = max(r1 - r0, 0)
    count = max(nm, ncl + 1, cap, 16)
    keep = []   # the buffers stay alive until the call has returned

    def array(values, kind_):
        if values is None:
            return None
        keep.append(np.ascontiguousarray(values, dtype=CTYPES[kind_][0]))
        return keep[-1].ctypes.data_as(C.POINTER(CTYPES[kind_][1]))

    out = [None if null == "all" or name in null else array(np.zeros(count * (21 if name == "counts" else 1)), kind_)
           for name, kind_ in OUTPUTS[call]]
    S = STATS[call]()
    tail = [C.byref(S) if stats else None]
    head = [ctx._h, r0, r1, array(mc, "u32"), ncl]
    if call == "linkage" or call == "split":
        args = head + [X, p, thr] + out + tail
    elif call == "pairs":
        args = head + [X, p, thr, out[0], count, out[1]] + tail
    elif call == "split_from_edges":
        args = [ctx._h, None if null_edges else array(np.zeros(1), "u64"), 1 if null_edges else 0] + head[1:] + out + tail
    elif call == "profile":
        col = None if column is None else array(column if isinstance(column, list) else np.full(max(nm, 1), column), "u32")
        P = profile_params(**changed)
        args = head + [col, C.byref(P) if params else None] + out[:7] + [cap] + out[7:] + tail
    else:
        args = head + [X, p] + out + tail
    st = getattr(N.lib, FUNCTIONS[call])(*args)
    names = {getattr(N, k): k[8:] for k in dir(N) if k.startswith("HMK_ERR_")}
    return (names[st], N.lib.hmk_last_error(ctx._h).decode()) if st else ("OK", None)


def situations(call):
    """-> {situation: the arguments of run() that make it}"""
    bad_slot, first = MC[:4] + [3] + MC[5:], FIRST_GROUP[call]
    s = {
        "r0_above_r1": dict(r0=5, r1=3, mc=MC[:2]),
        "r1_above_n": dict(r1=N_SEQ + 1, mc=MC + [0]),
        "null_member_cluster": dict(mc=None),
        "slot_at_n_clusters": dict(mc=bad_slot),
        "slot_without_member": dict(mc=[0 if c == 1 else c for c in MC]),
        "null_first_outputs": dict(null=first),
        "null_stats": dict(stats=False),
        "asymmetric": dict(kind="asym"),
        "valid": dict(),
        "empty_range": dict(r0=4, r1=4, mc=[], ncl=0),
        "empty_range_null_outputs": dict(r0=4, r1=4, mc=None, ncl=0, null="all"),
        "empty_range_asymmetric": dict(kind="asym", r0=4, r1=4, mc=[], ncl=0),
        # two faults at once: which check comes first
        "r0_above_r1_and_null_member_cluster": dict(r0=5, r1=3, mc=None),
        "bad_slot_and_null_outputs": dict(mc=bad_slot, null=first),
        "null_outputs_and_asymmetric": dict(kind="asym", null=first),
        "null_stats_and_asymmetric": dict(kind="asym", stats=False),
        "null_outputs_and_null_stats": dict(null=first, stats=False),
    }
    if call != "profile":   # (the profile scores nothing)
        s.update({
            "negative_shift": dict(X=-1),
            "shift_too_big": dict(X=12),
            "scores_below_int16": dict(p=-6000),
            "asymmetric_and_scores_below_int16": dict(kind="asym", p=-6000),
            "null_outputs_and_negative_shift": dict(null=first, X=-1),
        })
    if call in ("linkage", "split", "pairs"):
        s["threshold_too_high"] = dict(thr=30001)
    if call == "linkage":
        s.update({
            "member_min_without_member_below": dict(null=("member_below",)),
            "member_below_without_member_min": dict(null=("member_min",)),
            "neither_member_array": dict(null=("member_min", "member_below")),
            "null_n_below": dict(null=("n_below",)),
            "one_member_array_and_asymmetric": dict(kind="asym", null=("member_min",)),
            "null_outputs_and_one_member_array": dict(null=("min_a", "member_min")),
        })
    if call in ("split", "split_from_edges"):
        s.update({
            "null_n_parts": dict(null=("n_parts",)),
            "part_order_without_part_start": dict(null=("part_start",)),
            "part_start_without_part_order": dict(null=("part_order",)),
            "neither_part_array": dict(null=("part_order", "part_start", "part_id", "member_rank")),
            "one_part_array_and_asymmetric": dict(kind="asym", null=("part_order",)),
            "null_outputs_and_one_part_array": dict(null=("n_parts", "part_start")),
            "more_than_2^30_pairs": dict(kind="big", r1=N_BIG, mc=np.zeros(N_BIG), ncl=1),
            "more_than_2^30_pairs_and_negative_shift": dict(kind="big", r1=N_BIG, mc=np.zeros(N_BIG), ncl=1, X=-1),
            "one_part_array_and_more_than_2^30_pairs": dict(kind="big", r1=N_BIG, mc=np.zeros(N_BIG), ncl=1, null=("part_order",)),
        })
    if call == "split_from_edges":
        s.update({
            "null_edges": dict(null_edges=True),
            "null_edges_and_asymmetric": dict(kind="asym", null_edges=True),
            "null_edges_empty_range": dict(null_edges=True, r0=4, r1=4, mc=[], ncl=0),
        })
    if call == "separation":
        s.update({
            "null_near_cluster": dict(null=("near_cluster",)),
            "only_required_outputs": dict(null=("misplaced", "cluster_misplaced", "cluster_own_sum")),
            "empty_range_null_stats": dict(r0=4, r1=4, mc=[], ncl=0, stats=False),
        })
    if call == "align":
        s.update({
            "null_width": dict(null=("width",)),
            "null_member_outputs": dict(null=("center_score",)),
            "null_column": dict(null=("column",)),
            "null_slot_and_member_outputs": dict(null=("center_sum", "shift")),
            "null_member_outputs_and_asymmetric": dict(kind="asym", null=("shift",)),
            "no_member_sum": dict(null=("member_sum",)),
        })
    if call == "profile":
        s.update({
            "null_params": dict(params=False),
            "null_col_start": dict(null=("col_start",)),
            "null_passes": dict(null=("passes",)),
            "null_column": dict(column=None),
            "null_kld_all": dict(null=("kld_all",)),
            "null_params_and_bad_slot": dict(params=False, mc=bad_slot),
            "null_params_and_null_outputs": dict(params=False, null=first),
            "null_slot_and_member_outputs": dict(null=("n_match", "kld_match")),
            "null_column_and_bad_parameter": dict(column=None, min_ic=math.nan),
            "min_ic_not_finite": dict(min_ic=math.nan),
            "max_gap_proportion_above_1": dict(max_gap_proportion=1.5),
            "negative_min_conserved_positions": dict(min_conserved_positions=-1),
            "beta_zero": dict(beta=0.0),
            "sigma_infinite": dict(sigma=math.inf),
            "scale_negative": dict(scale=-1.0),
            "frequency_zero": dict(frequency=(47, 0.0)),
            "background_not_finite": dict(background=(19, math.nan)),
            "column_beyond_max_width": dict(column=[0, 0, 0, 85, 0, 0, 0, 0, 0, 0]),
            "bad_parameter_and_column_beyond_max_width": dict(column=85, min_ic=math.inf),
            "residue_outside_amino_acids": dict(kind="odd", r1=N_SEQ + 1, mc=MC + [1]),
            "column_beyond_max_width_and_residue_outside": dict(kind="odd", r1=N_SEQ + 1, mc=MC + [1], column=93),
            "capacity_below_columns": dict(cap=35),
            "capacity_exact": dict(cap=36),
            "no_column_arrays_no_capacity": dict(cap=0, null=("counts", "ic", "col_flags")),
            "capacity_below_columns_and_null_stats": dict(cap=35, stats=False),
        })
    return s


NO_GPU = "this context has no GPU (created with device = -1); scoring has no CPU fallback"
NULL_MC, BAD_SLOT, NO_MEMBER = "null member_cluster", "member_cluster[4] = 3 is not a slot below n_clusters = 3", "cluster slot 1 has no member"
RANGE = "%s ranges must lie within [0, n) with q0 <= q1 and r0 <= r1 (n = 10)"
CLINKAGE = ("clinkage needs a symmetric scoring matrix: the reference caches cluster scores by unordered pair "
            "(CachedClusterScorer.java:43-53), so its result depends on the evaluation order otherwise")
ASYM = {
    "linkage": "the linkage of a cluster needs a symmetric scoring matrix: the score of an unordered pair must not depend on which "
               "member comes first (ClinkageClusterScorer.java:30-49 scores each pair once)",
    "split": CLINKAGE,
    "split_from_edges": CLINKAGE,
    "pairs": CLINKAGE,
    "separation": "the separation of clusters needs a symmetric scoring matrix: a member's sum of scores must not depend on which "
                  "sequence of a pair comes first",
    "align": "the alignment of a cluster needs a symmetric scoring matrix: a member's sum of scores must not depend on which sequence "
             "of a pair comes first",
}
NULL_OUT = {
    "linkage": "null output (min_score, min_a, min_b, n_below)",
    "split": "null output (split_cluster, n_parts)",
    "split_from_edges": "null output (split_cluster, n_parts)",
    "separation": "null output (own_sum, near_sum, near_cluster)",
    "align": "null output (center, center_sum, width)",
    "profile": "null output (width, n_conserved, n_match, passes, kld_match_mean, kld_all_mean)",
    "pairs": "null n_pairs",
}
ALIGN_MEMBERS = "null output (center_score, shift, column)"
MEMBER_PAIR = "member_min and member_below are given together or not at all"
PART_PAIR = "part_order and part_start are given together or not at all"
NULL_STATS = "stats must not be null"
TOO_MANY_PAIRS = ("1076456800 pairs inside the slots of this call, more than 2^30: pass fewer slots per call (slots are split "
                  "independently of each other)")
SCORE_CHECKS = {   # what check_link_scores answers where a call reaches it without a device: the split alone
    "negative_shift": ("BAD_ARG", "max_shift must be >= 0"),
    "shift_too_big": ("SHIFT_TOO_BIG", "Shift too big: 11 is maximum, but 12 found"),
    "scores_below_int16": ("BAD_ARG", "scores down to -36048 are possible with this matrix / shift penalty: they do not fit the int16 "
                                      "score of a slot's key"),
    "threshold_too_high": ("BAD_ARG", "threshold outside [-30000, 30000]"),
}
PROFILE_NULL, PROFILE_MEMBERS = "null params, stats or col_start", "null column, kld_match or kld_all"
PROFILE_POSITIVE = "beta, sigma and scale must be finite and > 0"
EXPECTED = {}   # filled below: call -> {situation: (status, text)}


def _expect():
    for call in CALLS:
        bad = lambda text: ("BAD_ARG", text)   # noqa: E731
        # where every check has passed: the split from edges runs on the host, every other call asks for the device
        end = ("OK", None) if call == "split_from_edges" else ("DEVICE", NO_GPU)
        asym = bad(ASYM[call]) if call != "profile" else end
        stats = bad(NULL_STATS) if call == "separation" else bad(PROFILE_NULL) if call == "profile" else end
        what = {"split_from_edges": "split", "pairs": "merge"}.get(call, call)
        e = {
            "r0_above_r1": bad(RANGE % what), "r1_above_n": bad(RANGE % what), "r0_above_r1_and_null_member_cluster": bad(RANGE % what),
            "null_member_cluster": bad(NULL_MC),
            "slot_at_n_clusters": bad(BAD_SLOT), "bad_slot_and_null_outputs": bad(BAD_SLOT),
            "slot_without_member": bad(NO_MEMBER),
            "null_first_outputs": bad(NULL_OUT[call]), "null_outputs_and_asymmetric": bad(NULL_OUT[call]),
            # the profile asks for params, stats and col_start before its outputs, the separation for its stats after them
            "null_outputs_and_null_stats": bad(PROFILE_NULL if call == "profile" else NULL_OUT[call]),
            "null_stats": stats,
            "null_stats_and_asymmetric": stats if stats[0] == "BAD_ARG" else asym,
            "asymmetric": asym, "empty_range_asymmetric": asym,
            "valid": end, "empty_range": end,
            "empty_range_null_outputs": bad(PROFILE_NULL) if call == "profile" else end,
        }
        if call != "profile":
            for name in ("negative_shift", "shift_too_big", "scores_below_int16"):
                e[name] = SCORE_CHECKS[name] if call == "split" else end
            e["asymmetric_and_scores_below_int16"] = asym
            e["null_outputs_and_negative_shift"] = bad(NULL_OUT[call])
        if call == "pairs":   # its one required output is asked for after the matrix, and with or without members
            e["null_outputs_and_asymmetric"] = asym
            e["empty_range_null_outputs"] = bad(NULL_OUT[call])
            e["threshold_too_high"] = end
        if call == "linkage":
            e["threshold_too_high"] = end   # (the device is asked for first)
            e["member_min_without_member_below"] = e["member_below_without_member_min"] = e["one_member_array_and_asymmetric"] = bad(MEMBER_PAIR)
            e["neither_member_array"] = end
            e["null_n_below"] = e["null_outputs_and_one_member_array"] = bad(NULL_OUT[call])
        if call == "split":
            e["threshold_too_high"] = SCORE_CHECKS["threshold_too_high"]
        if call in ("split", "split_from_edges"):
            e["null_n_parts"] = e["null_outputs_and_one_part_array"] = bad(NULL_OUT[call])
            e["part_order_without_part_start"] = e["part_start_without_part_order"] = e["one_part_array_and_asymmetric"] = bad(PART_PAIR)
            e["one_part_array_and_more_than_2^30_pairs"] = bad(PART_PAIR)
            e["neither_part_array"] = end
            e["more_than_2^30_pairs"] = e["more_than_2^30_pairs_and_negative_shift"] = bad(TOO_MANY_PAIRS)
        if call == "split_from_edges":
            e["null_edges"] = e["null_edges_empty_range"] = bad("null edge list")
            e["null_edges_and_asymmetric"] = asym
        if call == "separation":
            e["null_near_cluster"] = bad(NULL_OUT[call])
            e["only_required_outputs"] = end
            e["empty_range_null_stats"] = bad(NULL_STATS)
        if call == "align":
            e["null_width"] = e["null_slot_and_member_outputs"] = bad(NULL_OUT[call])
            e["null_member_outputs"] = e["null_column"] = e["null_member_outputs_and_asymmetric"] = bad(ALIGN_MEMBERS)
            e["no_member_sum"] = end
        if call == "profile":
            e["null_params"] = e["null_col_start"] = e["null_params_and_null_outputs"] = bad(PROFILE_NULL)
            e["capacity_below_columns_and_null_stats"] = bad(PROFILE_NULL)
            e["null_params_and_bad_slot"] = bad(BAD_SLOT)
            e["null_passes"] = e["null_slot_and_member_outputs"] = bad(NULL_OUT[call])
            e["null_column"] = e["null_kld_all"] = e["null_column_and_bad_parameter"] = bad(PROFILE_MEMBERS)
            e["min_ic_not_finite"] = e["bad_parameter_and_column_beyond_max_width"] = bad("min_ic is not finite")
            e["max_gap_proportion_above_1"] = bad("max_gap_proportion outside [0, 1]")
            e["negative_min_conserved_positions"] = bad("negative min_conserved_positions")
            e["beta_zero"] = e["sigma_infinite"] = e["scale_negative"] = bad(PROFILE_POSITIVE)
            e["frequency_zero"] = bad("frequency[2][7] is not finite and > 0")
            e["background_not_finite"] = bad("background[19] is not finite and > 0")
            e["column_beyond_max_width"] = bad("member 3: column + length = 97 exceeds HMK_PROFILE_MAX_WIDTH")
            e["column_beyond_max_width_and_residue_outside"] = bad("member 0: column + length = 105 exceeds HMK_PROFILE_MAX_WIDTH")
            e["residue_outside_amino_acids"] = ("REFERENCE_WOULD_CRASH", "sequence 10 holds a residue outside the 20 amino acids: "
                                                                         "frequencyMatrix.get() is null for it (Statistics.java:286)")
            e["capacity_below_columns"] = ("CAPACITY", "the per-column arrays hold 35 columns, the slots have 36")
            e["capacity_exact"] = e["no_column_arrays_no_capacity"] = end
        EXPECTED[call] = e


_expect()


@pytest.mark.parametrize("call", CALLS)
def test_every_check_gives_its_status_and_text(call):
    cases, want = situations(call), EXPECTED[call]
    assert sorted(cases) == sorted(want)
    for name, kw in cases.items():
        assert run(call, **kw) == want[name], f"{call} {name}"


def test_the_cases_cover_what_they_are_meant_to():
    """every call refuses the five mistakes of a range and its slots, a null group of its required outputs and -- the profile
    aside, which scores nothing -- an asymmetric matrix; a valid call ends at the missing device, but for the split from edges,
    which a host-only context runs; the empty range is answered; the split reaches every refusal of the score checks"""
    for call in CALLS:
        e = EXPECTED[call]
        for name in ("r0_above_r1", "r1_above_n", "null_member_cluster", "slot_at_n_clusters", "slot_without_member", "null_first_outputs"):
            assert e[name][0] == "BAD_ARG", (call, name)
        assert len({e[name][1] for name in ("r0_above_r1", "null_member_cluster", "slot_at_n_clusters", "slot_without_member")}) == 4
        assert (e["asymmetric"][0] == "BAD_ARG") == (call != "profile")
        assert e["valid"] == (("OK", None) if call == "split_from_edges" else ("DEVICE", NO_GPU))
        assert "empty_range" in e
    split = EXPECTED["split"]
    assert split["shift_too_big"][0] == "SHIFT_TOO_BIG" and "2^30" in split["more_than_2^30_pairs"][1]
    assert len({split[name][1] for name in ("negative_shift", "shift_too_big", "threshold_too_high", "scores_below_int16")}) == 4
    assert EXPECTED["linkage"]["negative_shift"] == ("DEVICE", NO_GPU)   # the linkage asks for the device first, the split afterwards
