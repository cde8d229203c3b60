"""hammock_amd -- MI355X-native drop-in for the greedy initial-clustering hot
path of krejciadam/hammock (pairwise ShiftedScorer / LocalAlignmentScorer
scoring + LimitedGreedySequenceClusterer), behind the C ABI of
include/hammock_hip.h.  See DESIGN.md and INTEGRATION.md."""
from .api import (AMINO_ACIDS, Cluster, Context, DataException, DeviceError, FileFormatException,
                  HammockException, HipClinkageSequenceClusterer, HipGreedySequenceClusterer, LocalAlignmentScorer, ProfileResult,
                  ReferenceWouldCrash, ShiftedScorer, UniqueSequence, aligned_rows, edge_fields, encode, load_background,
                  load_frequency_matrix, pack_edges, pack_sequences, profile_params, gapped_rows, star_rows)

__all__ = ["AMINO_ACIDS", "Cluster", "Context", "DataException", "DeviceError", "FileFormatException",
           "HammockException", "HipClinkageSequenceClusterer", "HipGreedySequenceClusterer", "LocalAlignmentScorer", "ProfileResult",
           "ReferenceWouldCrash", "ShiftedScorer", "UniqueSequence", "aligned_rows", "edge_fields", "encode", "load_background",
           "load_frequency_matrix", "pack_edges", "pack_sequences", "profile_params", "gapped_rows", "star_rows"]
