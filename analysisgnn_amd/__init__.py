"""analysisgnn_amd — MI355X-native (gfx950) hot path of manoskary/analysisgnn.

Only the heterogeneous message-passing encoder path is here: hand-written HIP
kernels behind a C-ABI (`include/agnn.h`, `analysisgnn_amd/csrc/`), and the Python host side
that mirrors the reference's encoder / operator interface.  There is no CPU fallback: every
compute entry point raises if the HIP library or a GPU is missing.
"""
__version__ = "0.1.0"

_PRETRAIN = ("PreEncoder", "pretrain_objective", "PretrainMetrics", "LinkPlan", "link_plan", "link_plans", "link_bce", "link_candidates")
_EDGE_LOSS = ("EdgeDecoder", "EdgePlan", "edge_plan", "edge_consistency_loss")
_SCORE_GRAPH = ("DeviceScoreGraph", "build_score_graph", "sort_notes")
_DESCRIPTORS = ("note_features", "VOICE_FEATURES", "CADENCE_FEATURES")
_PITCH_SPELLING = ("PKSpell", "HierarchicalHeteroGraphSage", "PitchSpellingGNN", "PitchSpellingNeighborGNN", "GraphNorm", "GraphSegments",
                   "graph_norm", "graph_segments", "clear_segment_cache", "pitch_spelling_loss")

# (cadence.HierarchicalHeteroGraphSage, a different class from the pitch-spelling one, is reached through its module)
_CADENCE = ("GNN", "SMOTE", "CadenceGNNNeighbor", "CadenceGNNPytorch", "JoinNorm", "JoinIndex", "join_index", "pool_norm", "cad_clf",
            "run_cad_clf", "balanced_cross_entropy", "cadence_training_loss", "cadence_validation_loss", "cadence_metrics")


def __getattr__(name):
    """The public names of the pretraining stage (analysisgnn_amd/pretrain.py), of the edge-consistency term
    (analysisgnn_amd/edge_loss.py), of score graph construction (analysisgnn_amd/score_graph.py) and of the note descriptors
    (analysisgnn_amd/descriptors.py), resolved on first use: importing the package stays as light as before."""
    if name in _PRETRAIN:
        from . import pretrain
        return getattr(pretrain, name)
    if name in _EDGE_LOSS:
        from . import edge_loss
        return getattr(edge_loss, name)
    if name in _SCORE_GRAPH:
        from . import score_graph
        return getattr(score_graph, name)
    if name in _DESCRIPTORS:
        from . import descriptors
        return getattr(descriptors, name)
    if name in _PITCH_SPELLING:
        from . import pitch_spelling
        return getattr(pitch_spelling, name)
    if name in _CADENCE:
        from . import cadence
        return getattr(cadence, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
