"""libsbn_amd -- MI355X-native phylogenetic likelihood + gradient engine behind
libsbn's Engine / FatBeagle API.  The compute path is libmi_phylo.so (hand-written
HIP for gfx950, C ABI in include/mi_phylo.h); this package is a thin ctypes mirror
of the reference's Engine interface.  No CPU fallback exists."""
from .engine import (AncestralStates, BranchModelSample, BranchOptResult, Engine, NniSearchResult, PairwiseDistances, PhyloGradient, Placement,  # noqa: F401
                     PhyloModelSpecification, PspTable, RellResult, SbnSupport, SplitTable, SprSearchResult, SprScan, StartingTrees, TopologyTests, consensus_tree, nni_neighbour, rell_weights, site_pattern_compress_device,
                     lognormal_mode_match, psp_strings, VariationalFit, ViState, GeneralizedPruning, GpBranchDerivatives, GpHybridMarginals, GpHybridRequests, GpLikelihoods, GpOptimizeResult, GpStructure, GpTreeIndex, GpTrees, GpBranchDraw, RootedVariationalFit, DerootedTrees, gp_hybrid_request_count, sbn_rooted_representations, sbn_strings, split_strings, spr_neighbour)
from .instance import rooted_instance, unrooted_instance  # noqa: F401

__all__ = ["AncestralStates", "BranchOptResult", "Engine", "NniSearchResult", "PairwiseDistances", "PhyloGradient", "Placement", "PhyloModelSpecification", "RellResult", "SplitTable", "SprScan", "SprSearchResult", "StartingTrees", "unrooted_instance",
           "rooted_instance", "nni_neighbour", "spr_neighbour", "rell_weights", "site_pattern_compress_device", "consensus_tree", "split_strings",
           "SbnSupport", "sbn_strings", "sbn_rooted_representations", "BranchModelSample", "PspTable", "psp_strings",
           "lognormal_mode_match", "VariationalFit", "ViState",
           "GeneralizedPruning", "GpBranchDerivatives", "GpHybridMarginals", "GpHybridRequests", "GpLikelihoods", "GpOptimizeResult", "GpStructure", "GpTreeIndex", "GpTrees", "GpBranchDraw", "RootedVariationalFit", "DerootedTrees", "gp_hybrid_request_count",
           "TopologyTests"]
