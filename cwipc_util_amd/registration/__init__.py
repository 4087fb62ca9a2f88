"""Registration tooling on the MI355X path (reference python/cwipc/registration/).

The analyzers (`analyze.RegistrationAnalyzer`, `analyze.RegistrationAnalyzerSymmetric`, `analyze.OverlapAnalyzer`) and the fine
aligners (`fine.RegistrationComputer`, `fine.RegistrationComputer_ICP_Point2Point`, `fine.RegistrationComputer_ICP_Point2Plane`,
`fine.RegistrationComputer_ICP_Generalized`):
their per-point work (cross-cloud nearest distances and correspondences, the Gaussian KDE of the distances, the clouds'
normals and covariances, the sums of a rigid fit, of a plane fit and of a generalized fit) runs on the GPU.  The per-point helpers
the rest of the reference's tooling calls (cwipc_tilefilter_masked, cwipc_transform, get_tiles_used, cwipc_downsample_pertile,
cwipc_direction_filter) live in cwipc_util_amd.util.
"""
from .abstract import AnalysisResults, AnalysisAlgorithm, OverlapAnalysisResults   # noqa: F401
from .analyze import (RegistrationAnalyzer, RegistrationAnalyzerSymmetric, OverlapAnalyzer, DEFAULT_ANALYZER_ALGORITHM,   # noqa: F401
                      ALL_ANALYZER_ALGORITHMS)
from .fine import (RegistrationComputer, RegistrationComputer_ICP_Point2Point, RegistrationComputer_ICP_Point2Plane,   # noqa: F401
                   RegistrationComputer_ICP_Generalized, DEFAULT_FINE_ALIGNMENT_ALGORITHM, ALL_FINE_ALIGNMENT_ALGORITHMS)
