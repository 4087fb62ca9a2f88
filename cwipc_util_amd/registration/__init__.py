"""Registration tooling on the MI355X path (reference python/cwipc/registration/).

The analyzers (`analyze.RegistrationAnalyzer`, `analyze.RegistrationAnalyzerSymmetric`, `analyze.OverlapAnalyzer`) and the fine
aligners (`fine.RegistrationComputer`, `fine.RegistrationComputer_ICP_Point2Point`, `fine.RegistrationComputer_ICP_Point2Plane`,
`fine.RegistrationComputer_ICP_Generalized`):
their per-point work (cross-cloud nearest distances and correspondences, the Gaussian KDE of the distances, the clouds'
normals and covariances, the sums of a rigid fit, of a plane fit and of a generalized fit) runs on the GPU.  The per-point helpers
the rest of the reference's tooling calls (cwipc_tilefilter_masked, cwipc_transform, get_tiles_used, cwipc_downsample_pertile,
cwipc_direction_filter) live in cwipc_util_amd.util.

The multi-camera algorithms (`multicamera.MultiCameraIterative`, the default, `multicamera.MultiCameraOneToAllOthers`,
`multicamera.MultiCameraToFloor`, `multicamera.MultiCameraToGroundTruth`) loop over those pieces and give one transformation per
camera of a tiled capture; their per-camera analyses run as one batch (`analyze.run_analyzers_batched`, one tile-aware search over
one grid: cwipc_hip_nn_distance_jobs).  The transformation helpers are in `util`.

The step in front of them, from cameras that each have their own coordinates to a rough alignment, is `multicoarse.MultiCameraCoarse`
and `multicoarse.MultiCameraCoarseAruco`: markers with known corners, found in an image of each camera's tile.  The image comes from
`render` (`PinholeView`, `render_pointcloud`: a colour, depth and point-index image of a cloud on the GPU, cwipc_hip_render, where the
reference opens a window), and `deproject` takes image corners back to 3D.  The markers themselves are found by `markers`
(`MarkerDictionary`, `detect_markers`, `gpu_marker_detector`: square 5 x 5 binary fiducials on the GPU, cwipc_hip_detect_markers, where the
reference calls cv2.aruco); with `MultiCameraCoarseAruco.set_marker_dictionary` render and detection are one call and no image leaves the
GPU (cwipc_hip_render_detect_markers).  The user supplies the dictionary's bit patterns.  `multicoarse.MultiCameraCoarseArucoRgb` looks for
the markers in the cameras' own colour and depth images instead, which a grabber (`cwipc_util_amd.rgbd.RgbdSource`) attaches to the cloud.

Without any marker, `floor.find_floor` and `floor.level_to_floor` find the floor as the dominant near-horizontal plane of the cloud on the
GPU and move the cloud so that it lies at y = 0, which is what cwipc_floor_filter and `MultiCameraToFloor` assume.
"""
from .abstract import (AnalysisResults, AnalysisAlgorithm, OverlapAnalysisResults, AlignmentAlgorithm, MulticamAlgorithm,   # noqa: F401
                       MulticamAlignmentAlgorithm)
from .analyze import (RegistrationAnalyzer, RegistrationAnalyzerSymmetric, OverlapAnalyzer, DEFAULT_ANALYZER_ALGORITHM,   # noqa: F401
                      ALL_ANALYZER_ALGORITHMS, run_analyzers_batched, build_analyzer_jobs)
from .fine import (RegistrationComputer, RegistrationComputer_ICP_Point2Point, RegistrationComputer_ICP_Point2Plane,   # noqa: F401
                   RegistrationComputer_ICP_Generalized, DEFAULT_FINE_ALIGNMENT_ALGORITHM, ALL_FINE_ALIGNMENT_ALGORITHMS)
from .util import (transformation_identity, transformation_invert, transformation_frompython, transformation_topython,   # noqa: F401
                   transformation_get_translation, transformation_compare, BaseMulticamAlgorithm)
from .multicamera import (BaseMulticamAlignmentAlgorithm, MultiCameraOneToAllOthers, MultiCameraToFloor, MultiCameraToGroundTruth,   # noqa: F401
                          MultiCameraIterative, DEFAULT_MULTICAMERA_ALGORITHM, ALL_MULTICAMERA_ALGORITHMS, DEFAULT_MULTICAMERA_ALIGNER)
from .render import PinholeView, default_view, look_at, render_pointcloud, deproject, deproject_depth, mean_depth   # noqa: F401
from .markers import MarkerDictionary, detect_markers, gpu_marker_detector   # noqa: F401
from .multicoarse import MultiCameraCoarse, MultiCameraCoarseAruco, MultiCameraCoarseArucoRgb, MarkerPosition, MarkerPositions   # noqa: F401
from .floor import find_floor, level_to_floor   # noqa: F401
