"""ctypes binding of libhammock_hip.so (include/hammock_hip.h).

The library is built in-tree by ``__graft_entry__.build()`` /
``make -C hammock_amd/csrc``.  There is no fallback of any kind: if the shared
object is missing, importing this module raises.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libhammock_hip.so")

HMK_OK = 0
HMK_ERR_BAD_ARG = 1
HMK_ERR_SHIFT_TOO_BIG = 2
HMK_ERR_DEVICE = 3
HMK_ERR_OOM = 4
HMK_ERR_REFERENCE_WOULD_CRASH = 5
HMK_ERR_CAPACITY = 6
HMK_ERR_NO_SEQUENCES = 7
HMK_EDGE_SHARDS = 64
HMK_MAX_LEN = 32
HMK_SURVEY_MAX_BINS = 1024
HMK_PROFILE_SYMBOLS = 21
HMK_PROFILE_MAX_WIDTH = 96
HMK_TARGET_MAX_LEN = 1 << 20
HMK_SCAN_ALL_WINDOWS = 1

# every symbol include/hammock_hip.h declares
SYMBOLS = [
    "hmk_abi_version", "hmk_last_kernel_ms", "hmk_create", "hmk_create_multi", "hmk_device_count", "hmk_destroy", "hmk_last_error", "hmk_set_sequences",
    "hmk_score_pairs_shifted", "hmk_score_with_shift", "hmk_score_pairs_local", "hmk_score_block_shifted", "hmk_score_block_local",
    "hmk_score_pairs_global", "hmk_score_block_global", "hmk_neighbors_global", "hmk_search_global", "hmk_align_pairs_global",
    "hmk_neighbors_shifted", "hmk_neighbors_local", "hmk_neighbors_shifted_dev", "hmk_compact_edges_dev", "hmk_pack_rows_dev", "hmk_unpack_rows_dev",
    "hmk_neighbors_last_plan", "hmk_neighbors_last_plan_shared", "hmk_neighbors_last_plan_tables", "hmk_search_shifted", "hmk_search_local", "hmk_search_best_shifted",
    "hmk_assign_shifted", "hmk_assign_local", "hmk_match_clusters_shifted", "hmk_match_clusters_local", "hmk_greedy_continue",
    "hmk_greedy_cluster", "hmk_greedy_from_edges", "hmk_greedy_from_edges_dev", "hmk_greedy_last_phases",
    "hmk_clinkage_cluster", "hmk_clinkage_from_edges", "hmk_set_java_hashset", "hmk_reserve",
    "hmk_cluster_pairs_shifted", "hmk_clinkage_merge", "hmk_clinkage_merge_from_edges",
    "hmk_cluster_linkage_shifted", "hmk_clinkage_split", "hmk_clinkage_split_from_edges",
    "hmk_components_shifted", "hmk_components_from_edges", "hmk_components_from_edges_dev",
    "hmk_cluster_align_shifted", "hmk_score_survey_shifted", "hmk_cluster_separation_shifted",
    "hmk_greedy_sweep", "hmk_greedy_sweep_from_edges", "hmk_greedy_sweep_from_edges_dev",
    "hmk_greedy_orders", "hmk_greedy_orders_from_edges",
    "hmk_representatives_shifted", "hmk_representatives_from_edges", "hmk_representatives_from_edges_dev",
    "hmk_density_shifted", "hmk_density_from_edges", "hmk_density_from_edges_dev",
    "hmk_cluster_profile", "hmk_set_targets", "hmk_scan_shifted",
]


class NeighborStats(C.Structure):
    _fields_ = [
        ("n_edges", C.c_uint64), ("pairs_scored", C.c_uint64), ("n_tiles", C.c_uint32),
        ("symmetric", C.c_uint32), ("classes_u8", C.c_uint32), ("classes_u16", C.c_uint32),
        ("classes_direct", C.c_uint32), ("classes_rows", C.c_uint32), ("kernel_ms", C.c_double),
    ]


class ContinueStats(C.Structure):
    """hmk_continue_stats"""
    _fields_ = [
        ("n_edges", C.c_uint64), ("pairs_scored", C.c_uint64), ("n_joined", C.c_uint32), ("loop_rounds", C.c_uint32),
        ("host_precheck", C.c_uint32), ("reserved", C.c_uint32), ("kernel_ms", C.c_double), ("loop_ms", C.c_double),
    ]


class GreedyStats(C.Structure):
    _fields_ = [
        ("n_edges", C.c_uint64), ("phase1_stop_index", C.c_int32), ("phase1_clusters", C.c_int32),
        ("phase1_orphans", C.c_int32), ("crash_case", C.c_int32), ("crash_index", C.c_int32),
        ("n_result_clusters", C.c_int32), ("n_multi", C.c_int32), ("reserved", C.c_int32),
        ("neighbors_ms", C.c_double), ("greedy_ms", C.c_double),
    ]


class ClinkageStats(C.Structure):
    _fields_ = [("n_edges", C.c_uint64), ("merges", C.c_int32), ("searches", C.c_int32), ("n_result_clusters", C.c_int32),
                ("reserved", C.c_int32), ("neighbors_ms", C.c_double), ("chain_ms", C.c_double)]


class MergeStats(C.Structure):
    """hmk_merge_stats"""
    _fields_ = [("n_edges", C.c_uint64), ("pairs_scored", C.c_uint64), ("cluster_pairs", C.c_uint64), ("merges", C.c_int32),
                ("searches", C.c_int32), ("n_result_clusters", C.c_int32), ("reserved", C.c_int32), ("kernel_ms", C.c_double),
                ("graph_ms", C.c_double), ("chain_ms", C.c_double)]


class LinkageStats(C.Structure):
    """hmk_linkage_stats"""
    _fields_ = [("pairs_scored", C.c_uint64), ("n_multi", C.c_uint32), ("n_violating", C.c_uint32), ("launches", C.c_uint32),
                ("reserved", C.c_uint32), ("kernel_ms", C.c_double)]


class SplitStats(C.Structure):
    """hmk_split_stats"""
    _fields_ = [("pairs_scored", C.c_uint64), ("n_edges", C.c_uint64), ("n_multi", C.c_uint32), ("n_split", C.c_uint32),
                ("n_result_clusters", C.c_uint32), ("merges", C.c_uint32), ("crash_slot", C.c_int32), ("reserved", C.c_int32),
                ("kernel_ms", C.c_double), ("chain_ms", C.c_double), ("copy_ms", C.c_double)]


class ComponentLevel(C.Structure):
    """hmk_component_level"""
    _fields_ = [("n_edges", C.c_uint64), ("n_components", C.c_uint32), ("n_singletons", C.c_uint32), ("largest", C.c_uint32),
                ("reserved", C.c_uint32)]


class ComponentsStats(C.Structure):
    """hmk_components_stats"""
    _fields_ = [("n_edges", C.c_uint64), ("pairs_scored", C.c_uint64), ("n_levels", C.c_uint32), ("n_components", C.c_uint32),
                ("n_singletons", C.c_uint32), ("largest", C.c_uint32), ("kernel_ms", C.c_double), ("components_ms", C.c_double)]


class AlignStats(C.Structure):
    """hmk_align_stats"""
    _fields_ = [("pairs_scored", C.c_uint64), ("n_multi", C.c_uint32), ("max_width", C.c_uint32), ("launches", C.c_uint32),
                ("reserved", C.c_uint32), ("kernel_ms", C.c_double)]


class SurveyStats(C.Structure):
    """hmk_survey_stats"""
    _fields_ = [("pairs_scored", C.c_uint64), ("n_below", C.c_uint64), ("n_above", C.c_uint64), ("n_at_or_above", C.c_uint64),
                ("score_min", C.c_int32), ("score_max", C.c_int32), ("launches", C.c_uint32), ("reserved", C.c_uint32),
                ("kernel_ms", C.c_double)]


class SeparationStats(C.Structure):
    """hmk_separation_stats"""
    _fields_ = [("pairs_scored", C.c_uint64), ("n_misplaced", C.c_uint32), ("n_multi", C.c_uint32), ("n_segments", C.c_uint32),
                ("launches", C.c_uint32), ("reserved", C.c_uint32), ("kernel_ms", C.c_double)]


class ProfileParams(C.Structure):
    """hmk_profile_params"""
    _fields_ = [("min_ic", C.c_double), ("max_gap_proportion", C.c_double), ("min_conserved_positions", C.c_int32),
                ("allow_inner_gaps", C.c_int32), ("beta", C.c_double), ("sigma", C.c_double), ("scale", C.c_double),
                ("frequency", C.c_double * 400), ("background", C.c_double * 20)]


class ProfileStats(C.Structure):
    """hmk_profile_stats"""
    _fields_ = [("columns", C.c_uint64), ("n_multi", C.c_uint32), ("omitted", C.c_uint32), ("small_members", C.c_uint32),
                ("large_chunks", C.c_uint32), ("launches", C.c_uint32), ("reserved", C.c_uint32), ("system_kld_match", C.c_double),
                ("system_kld_all", C.c_double), ("kernel_ms", C.c_double)]


class ScanHit(C.Structure):
    """hmk_scan_hit"""
    _fields_ = [("query", C.c_uint32), ("target", C.c_uint32), ("score", C.c_int32), ("offset", C.c_int32)]


class ScanStats(C.Structure):
    """hmk_scan_stats"""
    _fields_ = [("n_hits", C.c_uint64), ("windows_scored", C.c_uint64), ("window_hits", C.c_uint64), ("windows_packed", C.c_uint64),
                ("windows_literal", C.c_uint64), ("n_tiles", C.c_uint32), ("launches", C.c_uint32), ("kernel_ms", C.c_double)]


class GreedyLevel(C.Structure):
    """hmk_greedy_level"""
    _fields_ = [("n_edges", C.c_uint64), ("status", C.c_int32), ("crash_case", C.c_int32), ("crash_index", C.c_int32),
                ("phase1_stop_index", C.c_int32), ("phase1_clusters", C.c_int32), ("phase1_orphans", C.c_int32),
                ("n_result_clusters", C.c_int32), ("n_multi", C.c_int32), ("n_singletons", C.c_uint32), ("largest", C.c_uint32),
                ("tail_ms", C.c_double)]


class GreedySweepStats(C.Structure):
    """hmk_greedy_sweep_stats"""
    _fields_ = [("n_edges", C.c_uint64), ("pairs_scored", C.c_uint64), ("n_levels", C.c_uint32), ("reserved", C.c_uint32),
                ("kernel_ms", C.c_double), ("deal_ms", C.c_double)]


class GreedyOrder(C.Structure):
    """hmk_greedy_order"""
    _fields_ = [("status", C.c_int32), ("crash_case", C.c_int32), ("crash_index", C.c_int32),
                ("phase1_stop_index", C.c_int32), ("phase1_clusters", C.c_int32), ("phase1_orphans", C.c_int32),
                ("n_result_clusters", C.c_int32), ("n_multi", C.c_int32), ("n_singletons", C.c_uint32), ("largest", C.c_uint32),
                ("pairs_together", C.c_uint64), ("pairs_with_first", C.c_uint64), ("tail_ms", C.c_double)]


class GreedyOrdersStats(C.Structure):
    """hmk_greedy_orders_stats"""
    _fields_ = [("n_edges", C.c_uint64), ("pairs_scored", C.c_uint64), ("n_orders", C.c_uint32), ("n_valid", C.c_uint32),
                ("pairs_ever", C.c_uint64), ("pairs_always", C.c_uint64), ("n_consensus", C.c_uint32),
                ("n_consensus_singletons", C.c_uint32), ("consensus_largest", C.c_uint32), ("reserved", C.c_uint32),
                ("kernel_ms", C.c_double), ("relabel_ms", C.c_double), ("support_ms", C.c_double)]


class RepresentativeLevel(C.Structure):
    """hmk_representative_level"""
    _fields_ = [("n_edges", C.c_uint64), ("n_representatives", C.c_uint32), ("n_isolated", C.c_uint32), ("largest", C.c_uint32),
                ("n_rounds", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class RepresentativesStats(C.Structure):
    """hmk_representatives_stats"""
    _fields_ = [("n_edges", C.c_uint64), ("pairs_scored", C.c_uint64), ("n_levels", C.c_uint32), ("n_representatives", C.c_uint32),
                ("n_isolated", C.c_uint32), ("largest", C.c_uint32), ("rounds_total", C.c_uint32), ("reserved", C.c_uint32),
                ("kernel_ms", C.c_double), ("select_ms", C.c_double)]


class DensityLevel(C.Structure):
    """hmk_density_level"""
    _fields_ = [("n_edges", C.c_uint64), ("n_core", C.c_uint32), ("n_border", C.c_uint32), ("n_noise", C.c_uint32),
                ("n_clusters", C.c_uint32), ("largest", C.c_uint32), ("reserved", C.c_uint32)]


class DensityStats(C.Structure):
    """hmk_density_stats"""
    _fields_ = [("n_edges", C.c_uint64), ("pairs_scored", C.c_uint64), ("n_levels", C.c_uint32), ("min_neighbors", C.c_uint32),
                ("n_core", C.c_uint32), ("n_border", C.c_uint32), ("n_noise", C.c_uint32), ("n_clusters", C.c_uint32),
                ("largest", C.c_uint32), ("reserved", C.c_uint32), ("kernel_ms", C.c_double), ("density_ms", C.c_double)]


class GreedyPhases(C.Structure):
    """hmk_greedy_phases: where the time of the last greedy call went (milliseconds)."""
    _fields_ = [(k, C.c_double) for k in ("plan_ms", "score_ms", "csr_ms", "wait_rows_ms", "phase1_ms", "precheck_ms", "exchange_ms",
                                          "device_loop_ms", "host_precheck_ms", "sequential_ms", "total_ms")] + \
               [("cand_entries", C.c_uint64), ("band_bytes", C.c_uint64), ("loop_rounds", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C hammock_amd/csrc`.  hammock_amd has no CPU fallback.")
    # One HIP runtime per process: PyTorch wheels bundle their own libamdhip64.so
    # (same SONAME, libamdhip64.so.7).  If torch is importable, load it FIRST so that
    # our NEEDED libamdhip64.so.7 resolves to the copy torch uses; two copies in one
    # process cannot both open the GPU ("no ROCm-capable device is detected").
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    vp, i32, u32, u64 = C.c_void_p, C.c_int, C.c_uint32, C.c_uint64
    p_i32, p_u32, p_u64, p_u8 = (C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                                 C.POINTER(C.c_uint8))
    L.hmk_abi_version.restype = i32
    L.hmk_last_kernel_ms.argtypes = [vp]
    L.hmk_last_kernel_ms.restype = C.c_double
    L.hmk_create.argtypes = [p_i32, i32, C.POINTER(vp)]
    L.hmk_create_multi.argtypes = [p_i32, C.POINTER(C.c_int), i32, C.POINTER(vp)]
    L.hmk_device_count.argtypes = [vp]
    L.hmk_destroy.argtypes = [vp]
    L.hmk_destroy.restype = None
    L.hmk_last_error.argtypes = [vp]
    L.hmk_last_error.restype = C.c_char_p
    L.hmk_set_sequences.argtypes = [vp, p_u8, p_u32, p_i32, u32]
    L.hmk_score_pairs_shifted.argtypes = [vp, p_u32, p_u32, u64, i32, i32, p_i32]
    L.hmk_score_pairs_local.argtypes = [vp, p_u32, p_u32, u64, i32, i32, p_i32]
    L.hmk_score_pairs_global.argtypes = [vp, p_u32, p_u32, u64, i32, i32, p_i32]
    L.hmk_align_pairs_global.argtypes = [vp, p_u32, p_u32, u64, i32, i32, p_i32, p_u8, p_u64, p_u64]
    L.hmk_score_with_shift.argtypes = [vp, p_u32, p_u32, u64, i32, i32, p_i32, p_i32]
    L.hmk_score_block_shifted.argtypes = [vp, u32, u32, u32, u32, i32, i32, p_i32]
    L.hmk_score_block_local.argtypes = [vp, u32, u32, u32, u32, i32, i32, p_i32]
    L.hmk_score_block_global.argtypes = [vp, u32, u32, u32, u32, i32, i32, p_i32]
    L.hmk_neighbors_shifted.argtypes = [vp, i32, i32, i32, u32, u32, p_u64, u64, p_u64, C.POINTER(NeighborStats)]
    L.hmk_neighbors_local.argtypes = [vp, i32, i32, i32, u32, u32, p_u64, u64, p_u64, C.POINTER(NeighborStats)]
    L.hmk_neighbors_global.argtypes = [vp, i32, i32, i32, u32, u32, p_u64, u64, p_u64, C.POINTER(NeighborStats)]
    L.hmk_neighbors_shifted_dev.argtypes = [vp, i32, i32, i32, u32, u32, vp, u64, vp, vp]
    L.hmk_compact_edges_dev.argtypes = [vp, vp, u64, vp, vp, u64, vp, vp]
    L.hmk_pack_rows_dev.argtypes = [vp, vp, u64, vp, i32, vp, vp, u64, vp]
    L.hmk_unpack_rows_dev.argtypes = [vp, vp, vp, i32, vp, u64, vp]
    L.hmk_neighbors_last_plan.argtypes = [vp, C.POINTER(NeighborStats)]
    L.hmk_neighbors_last_plan_shared.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.hmk_neighbors_last_plan_tables.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    L.hmk_search_shifted.argtypes = [vp, u32, u32, u32, u32, i32, i32, i32, p_u64, u64, p_u64, C.POINTER(NeighborStats)]
    L.hmk_search_local.argtypes = [vp, u32, u32, u32, u32, i32, i32, i32, p_u64, u64, p_u64, C.POINTER(NeighborStats)]
    L.hmk_search_global.argtypes = [vp, u32, u32, u32, u32, i32, i32, i32, p_u64, u64, p_u64, C.POINTER(NeighborStats)]
    L.hmk_search_best_shifted.argtypes = [vp, u32, u32, u32, u32, i32, i32, i32, u32, p_u32, p_i32, p_u32, C.POINTER(NeighborStats)]
    L.hmk_assign_shifted.argtypes = [vp, u32, u32, u32, u32, p_u32, p_i32, u32, i32, i32, i32, u32, p_u32, p_i32, p_u32,
                                     C.POINTER(NeighborStats)]
    L.hmk_assign_local.argtypes = [vp, u32, u32, u32, u32, p_u32, p_i32, u32, i32, i32, i32, u32, p_u32, p_i32, p_u32,
                                   C.POINTER(NeighborStats)]
    L.hmk_match_clusters_shifted.argtypes = [vp, u32, u32, p_u32, u32, u32, u32, p_u32, p_i32, u32, i32, i32, i32, u32, p_u32, p_i32, p_u32,
                                             C.POINTER(NeighborStats)]
    L.hmk_match_clusters_local.argtypes = [vp, u32, u32, p_u32, u32, u32, u32, p_u32, p_i32, u32, i32, i32, i32, u32, p_u32, p_i32, p_u32,
                                           C.POINTER(NeighborStats)]
    L.hmk_greedy_continue.argtypes = [vp, u32, u32, u32, u32, p_u32, p_i32, u32, i32, i32, i32, p_i32, p_i32, C.POINTER(ContinueStats)]
    L.hmk_greedy_cluster.argtypes = [vp, i32, i32, i32, i32, p_i32, p_i32, p_i32, C.POINTER(GreedyStats)]
    L.hmk_greedy_from_edges_dev.argtypes = [vp, vp, u64, i32, i32, p_i32, p_i32, p_i32, C.POINTER(GreedyStats)]
    L.hmk_greedy_from_edges.argtypes = [vp, p_u64, u64, i32, i32, i32, p_i32, p_i32, p_i32, C.POINTER(GreedyStats)]
    L.hmk_greedy_last_phases.argtypes = [vp, C.POINTER(GreedyPhases)]
    L.hmk_set_java_hashset.argtypes = [vp, i32]
    L.hmk_reserve.argtypes = [vp, u32]
    L.hmk_clinkage_cluster.argtypes = [vp, i32, i32, i32, p_i32, p_i32, p_i32, C.POINTER(ClinkageStats)]
    L.hmk_clinkage_from_edges.argtypes = [vp, p_u64, u64, p_i32, p_i32, p_i32, C.POINTER(ClinkageStats)]
    L.hmk_cluster_pairs_shifted.argtypes = [vp, u32, u32, p_u32, u32, i32, i32, i32, p_u64, u64, p_u64, C.POINTER(MergeStats)]
    L.hmk_clinkage_merge.argtypes = [vp, u32, u32, p_u32, p_i32, u32, i32, i32, i32, p_i32, p_i32, p_i32, C.POINTER(MergeStats)]
    L.hmk_clinkage_merge_from_edges.argtypes = [vp, p_u64, u64, u32, u32, p_u32, p_i32, u32, p_i32, p_i32, p_i32, C.POINTER(MergeStats)]
    L.hmk_cluster_linkage_shifted.argtypes = [vp, u32, u32, p_u32, u32, i32, i32, i32, p_i32, p_u32, p_u32, p_u64, p_i32, p_u32,
                                              C.POINTER(LinkageStats)]
    L.hmk_clinkage_split.argtypes = [vp, u32, u32, p_u32, u32, i32, i32, i32, p_u32, p_u32, p_i32, p_i32, p_i32, p_u32, C.POINTER(SplitStats)]
    L.hmk_clinkage_split_from_edges.argtypes = [vp, p_u64, u64, u32, u32, p_u32, u32, p_u32, p_u32, p_i32, p_i32, p_i32, p_u32,
                                                C.POINTER(SplitStats)]
    L.hmk_components_shifted.argtypes = [vp, i32, i32, i32, i32, p_u32, C.POINTER(ComponentLevel), C.POINTER(ComponentsStats)]
    L.hmk_components_from_edges.argtypes = [vp, p_u64, u64, i32, i32, p_u32, C.POINTER(ComponentLevel), C.POINTER(ComponentsStats)]
    L.hmk_components_from_edges_dev.argtypes = [vp, vp, u64, i32, i32, p_u32, C.POINTER(ComponentLevel), C.POINTER(ComponentsStats)]
    p_i64 = C.POINTER(C.c_int64)
    L.hmk_cluster_align_shifted.argtypes = [vp, u32, u32, p_u32, u32, i32, i32, p_u32, p_i64, p_u32, p_i64, p_i32, p_i32, p_u32,
                                            C.POINTER(AlignStats)]
    L.hmk_score_survey_shifted.argtypes = [vp, u32, u32, u32, u32, i32, i32, i32, i32, u32, p_u64, p_i32, p_u32, p_u32,
                                           C.POINTER(SurveyStats)]
    L.hmk_cluster_separation_shifted.argtypes = [vp, u32, u32, p_u32, u32, i32, i32, p_i64, p_i64, p_u32, p_u8, p_u32, p_i64,
                                                 C.POINTER(SeparationStats)]
    sweep_out = [p_i32, p_i32, p_i32, C.POINTER(GreedyLevel), C.POINTER(GreedySweepStats)]
    L.hmk_greedy_sweep.argtypes = [vp, i32, i32, i32, i32, i32] + sweep_out
    L.hmk_greedy_sweep_from_edges.argtypes = [vp, p_u64, u64, i32, i32, i32, i32] + sweep_out
    L.hmk_greedy_sweep_from_edges_dev.argtypes = [vp, vp, u64, i32, i32, i32, i32] + sweep_out
    orders_tail = [p_u32, u32, u32, p_i32, p_i32, p_i32, C.POINTER(GreedyOrder), p_u32, p_u32, p_u32, p_u64, u64, p_u64,
                   C.POINTER(GreedyOrdersStats)]
    L.hmk_greedy_orders.argtypes = [vp, i32, i32, i32, i32] + orders_tail
    L.hmk_greedy_orders_from_edges.argtypes = [vp, p_u64, u64, i32, i32] + orders_tail
    rep_out = [p_u32, p_u32, p_i32, C.POINTER(RepresentativeLevel), C.POINTER(RepresentativesStats)]
    L.hmk_representatives_shifted.argtypes = [vp, i32, i32, i32, i32] + rep_out
    L.hmk_representatives_from_edges.argtypes = [vp, p_u64, u64, i32, i32] + rep_out
    L.hmk_representatives_from_edges_dev.argtypes = [vp, vp, u64, i32, i32] + rep_out
    den_out = [p_u32, p_u32, p_u32, C.POINTER(DensityLevel), C.POINTER(DensityStats)]
    L.hmk_density_shifted.argtypes = [vp, i32, i32, i32, i32, i32] + den_out
    L.hmk_density_from_edges.argtypes = [vp, p_u64, u64, i32, i32, i32] + den_out
    L.hmk_density_from_edges_dev.argtypes = [vp, vp, u64, i32, i32, i32] + den_out
    p_f64 = C.POINTER(C.c_double)
    L.hmk_cluster_profile.argtypes = [vp, u32, u32, p_u32, u32, p_u32, C.POINTER(ProfileParams), p_u32, p_u32, p_u32, p_u8, p_f64, p_f64,
                                      p_u64, u64, p_u32, p_f64, p_u8, p_f64, p_f64, C.POINTER(ProfileStats)]
    L.hmk_set_targets.argtypes = [vp, p_u8, p_u64, u32]
    L.hmk_scan_shifted.argtypes = [vp, u32, u32, u32, u32, i32, i32, i32, u32, C.POINTER(ScanHit), u64, p_u32, p_u64, C.POINTER(ScanStats)]
    for name in SYMBOLS:
        fn = getattr(L, name)
        if name not in ("hmk_destroy", "hmk_last_error", "hmk_last_kernel_ms"):
            fn.restype = i32
    return L


lib = _load()
