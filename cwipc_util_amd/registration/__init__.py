"""Registration tooling on the MI355X path (reference python/cwipc/registration/).

Only the analyzers exist here: `analyze.RegistrationAnalyzer` and `analyze.RegistrationAnalyzerSymmetric`, whose per-point
work (cross-cloud nearest distances, the Gaussian KDE of those distances) runs on the GPU.  The per-point helpers the rest of the
reference's tooling calls (cwipc_tilefilter_masked, cwipc_transform, get_tiles_used, cwipc_downsample_pertile,
cwipc_direction_filter) live in cwipc_util_amd.util.
"""
from .abstract import AnalysisResults, AnalysisAlgorithm   # noqa: F401
from .analyze import (RegistrationAnalyzer, RegistrationAnalyzerSymmetric, DEFAULT_ANALYZER_ALGORITHM,   # noqa: F401
                      ALL_ANALYZER_ALGORITHMS)
