"""One transformation per camera of a tiled capture (reference python/cwipc/registration/multicamera.py).

A tiled cloud holds one tile per camera.  The algorithms here loop over pieces this package already has -- an analyzer per camera
(registration/analyze.py) to order the cameras and to judge a step, a fine aligner per camera (registration/fine.py) to move it --
and multiply each camera's new matrix to the left of the one it had:

  * MultiCameraOneToAllOthers  every camera, best correspondence first, against all the others        (reference :308-349)
  * MultiCameraToFloor         every camera against the frame projected onto y = 0                     (reference :351-407)
  * MultiCameraToGroundTruth   every camera against a cloud the caller supplies                        (reference :409-460)
  * MultiCameraIterative       the default: the best camera stays, the others join it one by one, a step
                               that makes things worse is taken back                                   (reference :462-741)

Where this differs from the reference, and why:
  * The per-camera analyses of _pre_analyse and _post_analyse look at subsets of ONE pair of clouds, so they CAN run as one batch
    (analyze.run_analyzers_batched: one search call per direction instead of two compactions, two floor crops, a grid and a search
    per camera and direction), with the same results bit for bit: `batch_analysis = True`.  It is off by default, because it
    measured SLOWER on an MI355X (20.2 against 17.8 ms per pass of a 72 k frame, 922 against 312 ms at
    600 k): in the one grid over the whole frame a camera's query has to read through its own camera's points, which the
    per-camera grid does not hold.  _pre_step_analyse (a direction filter per camera on the reference) and _post_step_analyse
    (per-step clouds) run one by one either way.
  * The floor-only analyses name the floor by a setting (set_source_floor_only), not by a lambda: a batch can read a setting.
  * The default aligner is RegistrationComputer_ICP_Generalized, the reference's default, named here: fine.DEFAULT_FINE_ALIGNMENT_ALGORITHM
    is still the point-to-point class, because an existing test pins it.
  * MultiCameraToFloor makes its floor cloud on the device (cwipc_hip_flatten_y), no download.
  * functools.reduce(cwipc_join) is cwipc_join_multi.
  * randomize_floor takes `floor_seed` (None: a fresh one), so that a run can be repeated.
  * The todo list carries each camera's INDEX (from its tile number); the reference carries the camera's rank in the sorted
    analysis results under that name and files the matrix there (:198-204, :343-346).
  * Nothing is printed unless `verbose`; what the reference prints is kept in attributes (change, tile_occupancy).  show_plot is
    accepted and ignored with one log line; MultiCameraIterativeInteractive (stdin, matplotlib, a window) is not here.
"""
import copy
import logging
import math
from abc import abstractmethod
from typing import Any, List, Optional, Tuple

import numpy as np

from ..util import cwipc_pointcloud_wrapper, cwipc_join, cwipc_join_multi, cwipc_hip_flatten_y
from .abstract import AnalysisResults, MulticamAlignmentAlgorithm, RegistrationTransformation, Vector3
from .analyze import RegistrationAnalyzer, DEFAULT_ANALYZER_ALGORITHM, run_analyzers_batched, FLOOR_Y
from .fine import RegistrationComputer_ICP_Generalized
from .util import (BaseMulticamAlgorithm, transformation_identity, transformation_get_translation, transformation_compare,
                   cwipc_randomize_floor, cwipc_direction_filter, cwipc_downsample_pertile, cwipc_compute_tile_occupancy)

__all__ = ['BaseMulticamAlignmentAlgorithm', 'MultiCameraOneToAllOthers', 'MultiCameraToFloor', 'MultiCameraToGroundTruth',
           'MultiCameraIterative', 'DEFAULT_MULTICAMERA_ALGORITHM', 'ALL_MULTICAMERA_ALGORITHMS', 'DEFAULT_MULTICAMERA_ALIGNER']

_log = logging.getLogger(__name__)

#: (camera index, tile number, correspondence, fraction of the distances at or under it)
OrderedCameraList = List[Tuple[int, int, float, float]]

#: the reference's default fine aligner (fine.DEFAULT_FINE_ALIGNMENT_ALGORITHM cannot name it: an existing test pins that one)
DEFAULT_MULTICAMERA_ALIGNER = RegistrationComputer_ICP_Generalized


class BaseMulticamAlignmentAlgorithm(MulticamAlignmentAlgorithm, BaseMulticamAlgorithm):
    """What the multi-camera alignment algorithms share (reference multicamera.py:26-306)."""

    #: run the analyses of _pre_analyse and _post_analyse as one batch (False: one analyzer at a time).  Same results; the batch
    #: measured slower (see the module's docstring), so it is off until the search kernel makes it pay
    batch_analysis = False

    def __init__(self) -> None:
        MulticamAlignmentAlgorithm.__init__(self)
        BaseMulticamAlgorithm.__init__(self)
        self.transformations: List[RegistrationTransformation] = []
        self.original_transformations: List[RegistrationTransformation] = []
        self.camera_positions: List[Vector3] = []
        self.pre_analysis_results: List[AnalysisResults] = []
        self.results: List[AnalysisResults] = []
        self.aligner_class = DEFAULT_MULTICAMERA_ALIGNER
        self.is_interactive = False
        self.verbose = False
        self.show_plot = False
        self.change: List[Tuple[Vector3, Vector3]] = []
        self.proposed_cellsize_factor: float = math.sqrt(2)
        self.proposed_cellsize_method: str = "max"
        self.proposed_cellsize: float = 0
        #: (tile number, point count) after voxelizing with proposed_cellsize, from _compute_new_tiles
        self.tile_occupancy: List[Tuple[int, int]] = []
        self.correspondence: Optional[float] = None
        self.randomize_floor = False
        #: seed of the floor's permutation (None: a fresh one per run)
        self.floor_seed: Optional[int] = None

    def _say(self, text: str) -> None:
        if self.verbose:
            print(f"{self.__class__.__name__}: {text}")

    def set_max_correspondence(self, max_correspondence: float) -> None:
        self.correspondence = max_correspondence

    def set_tiled_pointcloud(self, pc: cwipc_pointcloud_wrapper) -> None:
        if self.randomize_floor:
            pc = cwipc_randomize_floor(pc, seed=self.floor_seed)
        super().set_tiled_pointcloud(pc)

    def _prepare_analyze(self) -> Any:
        if not self.analyzer_class:
            self.analyzer_class = DEFAULT_ANALYZER_ALGORITHM
        self._say(f"Use analyzer class {self.analyzer_class.__name__}")
        analyzer = self.analyzer_class()
        analyzer.verbose = self.verbose
        return analyzer

    def _prepare_aligner(self) -> Any:
        if not self.aligner_class:
            self.aligner_class = DEFAULT_MULTICAMERA_ALIGNER
        self._say(f"Use aligner class {self.aligner_class.__name__}")
        aligner = self.aligner_class()
        aligner.verbose = self.verbose
        return aligner

    def set_original_transform(self, cam_index: int, matrix: RegistrationTransformation) -> None:
        assert self.original_pointcloud
        if len(self.transformations) == 0:
            self.transformations = [transformation_identity() for _ in range(self.camera_count())]
        self.transformations[cam_index] = matrix

    def _init_transformations(self) -> None:
        """Identity for every camera the caller gave no matrix; a camera's position is its matrix's translation."""
        if self.show_plot:
            _log.warning("%s: show_plot is not supported and is ignored", self.__class__.__name__)
        if len(self.transformations) == 0:
            self.transformations = [transformation_identity() for _ in range(self.camera_count())]
        self.original_transformations = copy.deepcopy(self.transformations)
        assert len(self.camera_positions) == 0
        for i in range(self.camera_count()):
            self.camera_positions.append(transformation_get_translation(self.transformations[i]))

    def _run_analyzers(self, analyzers: List[Any]) -> None:
        if self.batch_analysis:
            run_analyzers_batched(analyzers)
        else:
            for analyzer in analyzers:
                analyzer.run()

    def _pre_analyse(self, toSelf: bool = False, toReference: Optional[cwipc_pointcloud_wrapper] = None, onlyFloor: bool = False,
                     ignoreFloor: bool = False, sortBy: str = 'corr', target_dirfilter: Optional[float] = None) -> None:
        """One analysis per camera into pre_analysis_results (reference :125-196).  toSelf: the camera's own nearest-point distances
        (how precise its capture is); toReference: against that cloud; otherwise against all other cameras.  ignoreFloor: without the
        points at y <= 0.1.  sortBy: 'corr' lowest correspondence first, 'corrcount' most points under it first, 'sourcecount' most
        source points first, 'none'.  target_dirfilter: the reference cloud cut down to the points facing the camera first (this
        takes the analyses off the batched path)."""
        assert self.original_pointcloud
        assert self.camera_count() > 1
        analyzers = []
        label = ""
        for camnum in range(self.camera_count()):
            tilemask = self.tilemask_for_camera_index(camnum)
            othertilemask = 0xff ^ tilemask
            if toSelf or toReference is not None:
                analyzer = RegistrationAnalyzer()
                analyzer.verbose = self.verbose
            else:
                analyzer = self._prepare_analyze()
            analyzer.set_source_pointcloud(self.original_pointcloud, tilemask)
            if toReference is not None:
                analyzer.set_reference_pointcloud(toReference)
                if onlyFloor:
                    analyzer.set_source_floor_only(FLOOR_Y)
                    analyzer.set_correspondence_measure('q=95')
                    label = "flooronly(q=95)"
                else:
                    analyzer.set_correspondence_measure('median')
                    label = "toreference(median)"
            elif toSelf:
                analyzer.set_reference_pointcloud(self.original_pointcloud, tilemask)
                analyzer.set_ignore_nearest(1)
                analyzer.set_correspondence_measure('median')
                label = "precision(median)"
            else:
                analyzer.set_reference_pointcloud(self.original_pointcloud, othertilemask)
                analyzer.set_correspondence_measure('2mode')
                label = "correspondence(2mode)"
            if ignoreFloor:
                analyzer.set_ignore_floor(True)
            if target_dirfilter is not None:
                direction, threshold = self.camera_positions[camnum], target_dirfilter
                analyzer.apply_reference_filter(lambda pc, direction=direction, threshold=threshold: cwipc_direction_filter(pc, direction, threshold))
                label += f" (dirfilter={target_dirfilter})"
            analyzers.append(analyzer)
        self._run_analyzers(analyzers)
        self.pre_analysis_results = [analyzer.get_results() for analyzer in analyzers]
        if sortBy == 'corr':
            self.pre_analysis_results.sort(key=lambda r: r.minCorrespondence)
        elif sortBy == 'corrcount':
            self.pre_analysis_results.sort(key=lambda r: r.minCorrespondenceCount, reverse=True)
        elif sortBy == 'sourcecount':
            self.pre_analysis_results.sort(key=lambda r: r.sourcePointCount, reverse=True)
        else:
            assert sortBy == 'none', f"Unknown sortBy={sortBy}"
        if self.verbose:
            self._print_correspondences(f"{self.__class__.__name__}: Before:  Per-camera capture {label}", self.pre_analysis_results)

    def _todo_from_pre_analysis_results(self) -> OrderedCameraList:
        rv: OrderedCameraList = []
        for r in self.pre_analysis_results:
            assert type(r.tilemask) == int
            rv.append((self.camera_index_for_tilemask(r.tilemask), r.tilemask, r.minCorrespondence, r.minCorrespondenceCount / r.sourcePointCount))
        return rv

    @abstractmethod
    def run(self) -> bool: ...

    def _post_analyse(self, toReference: Optional[cwipc_pointcloud_wrapper] = None, onlyFloor: bool = False) -> bool:
        """One analysis per camera of the aligned cloud into results, and the cell size they suggest (reference :211-256)."""
        assert self.original_pointcloud
        assert self.original_pointcloud.count() > 0
        assert self.camera_count() > 0
        analyzers = []
        label = ""
        for camnum in range(self.camera_count()):
            tilemask = self.tilemask_for_camera_index(camnum)
            othertilemask = 0xff ^ tilemask
            analyzer = self._prepare_analyze()
            analyzer.set_source_pointcloud(self.original_pointcloud, tilemask)
            if toReference:
                analyzer.set_reference_pointcloud(toReference)
                if onlyFloor:
                    analyzer.set_source_floor_only(FLOOR_Y)
                    analyzer.set_correspondence_measure('q=95')
                    label = "flooronly(q=95)"
                else:
                    analyzer.set_correspondence_measure('median')
                    label = "toreference(median)"
            else:
                analyzer.set_reference_pointcloud(self.original_pointcloud, othertilemask)
                analyzer.set_correspondence_measure('mode')
                label = "correspondence(mode)"
            analyzers.append(analyzer)
        self._run_analyzers(analyzers)
        self.results = [analyzer.get_results() for analyzer in analyzers]
        if self.verbose:
            self._print_correspondences(f"{self.__class__.__name__}: After:  Per-camera {label}", self.results)
        correspondences = [r.minCorrespondence for r in self.results]
        if self.proposed_cellsize_method == "max":
            correspondence = max(correspondences)
        elif self.proposed_cellsize_method == "min":
            correspondence = min(correspondences)
        else:
            assert self.proposed_cellsize_method == "avg", f"Unknown proposed_cellsize_method={self.proposed_cellsize_method}"
            correspondence = sum(correspondences) / len(correspondences)
        self.proposed_cellsize = correspondence * self.proposed_cellsize_factor
        self._compute_change()
        self._compute_new_tiles()
        return True

    def _compute_change(self) -> None:
        """Per camera what leads from the matrix it had to the one it has now: (translation, rotation vector in degrees)."""
        self._say("Change in matrices after alignment:")
        for cam_index in range(len(self.transformations)):
            translation, rotation = transformation_compare(self.original_transformations[cam_index], self.transformations[cam_index])
            if self.verbose:
                tile = self.tilemask_for_camera_index(cam_index)
                print(f"\ttile={tile}, distance={np.linalg.norm(translation):.4f}, angle={np.linalg.norm(rotation):.1f}, "
                      f"translation={translation}, rotation={rotation}")
            self.change.append((translation, rotation))

    def _compute_new_tiles(self) -> bool:
        """How many points each combination of cameras holds once the cloud is voxelized with the proposed cell size."""
        assert self.original_pointcloud
        if self.proposed_cellsize == 0:
            self._say("Warning: proposed_cellsize==0. Cannot compute new tiles.")
            return False
        self.tile_occupancy = cwipc_compute_tile_occupancy(self.original_pointcloud, cellsize=self.proposed_cellsize, filterfloor=True)
        if self.verbose:
            self._say(f"Pointcounts per tile, after voxelizing with {self.proposed_cellsize}:")
            for tile, pointcount in self.tile_occupancy:
                print(f"\ttile {tile}: {pointcount} ({bin(tile).count('1')} contributors)")
        return True

    def get_result_transformations(self) -> List[RegistrationTransformation]:
        return self.transformations

    def get_result_pointcloud_full(self) -> cwipc_pointcloud_wrapper:
        assert self.original_pointcloud
        return self.original_pointcloud

    def _print_correspondences(self, label: str, results: List[AnalysisResults]) -> None:
        print(f"{label}:")
        for r in results:
            print(f"\tcamnum={r.tilemask}, reference={r.referenceTilemask}, {r.tostr()}")

    def _apply_step(self, camnum: int, aligner: Any) -> None:
        """The aligner's transformation goes to the LEFT of the camera's old one."""
        self.transformations[camnum] = np.matmul(aligner.get_result_transformation(), self.transformations[camnum])


class MultiCameraOneToAllOthers(BaseMulticamAlignmentAlgorithm):
    """Align multiple cameras.  Every step, one camera is aligned to all others, the camera with the best correspondence first."""

    def run(self) -> bool:
        assert self.original_pointcloud
        assert self.camera_count() > 0
        self._init_transformations()
        self._pre_analyse(toSelf=False)
        for camnum, tilemask, corr, _fraction in self._todo_from_pre_analysis_results():
            aligner = self._prepare_aligner()
            aligner.set_source_pointcloud(self.original_pointcloud, tilemask)
            aligner.set_reference_pointcloud(self.original_pointcloud, 0xff ^ tilemask)
            aligner.set_correspondence(corr if self.correspondence is None else self.correspondence)
            aligner.run()
            # the next camera is aligned to the cloud with this one moved
            self.original_pointcloud = aligner.get_result_pointcloud_full()
            self._apply_step(camnum, aligner)
        return self._post_analyse()


class _MultiCameraToCloud(BaseMulticamAlignmentAlgorithm):
    """Every camera on its own against one cloud that does not change; the moved cameras joined are the result."""

    def _align_each_to(self, target: cwipc_pointcloud_wrapper) -> None:
        aligned: List[cwipc_pointcloud_wrapper] = []
        for camnum, tilemask, corr, _fraction in self._todo_from_pre_analysis_results():
            aligner = self._prepare_aligner()
            aligner.set_source_pointcloud(self.original_pointcloud, tilemask)
            aligner.set_reference_pointcloud(target)
            aligner.set_correspondence(corr if self.correspondence is None else self.correspondence)
            aligner.run()
            aligned.append(aligner.get_result_pointcloud())
            self._apply_step(camnum, aligner)
        self.original_pointcloud = cwipc_join_multi(aligned)

    def _compute_new_tiles(self) -> bool:
        return False


class MultiCameraToFloor(_MultiCameraToCloud):
    """Align multiple cameras to the floor at Y=0.  Requires enough floor to be visible for each camera.  A synthetic floor is made by
    projecting all points to Y=0; each camera's floor points are then aligned to it."""

    def __init__(self) -> None:
        super().__init__()
        self.floor_pointcloud: Optional[cwipc_pointcloud_wrapper] = None

    def run(self) -> bool:
        assert self.original_pointcloud
        assert self.camera_count() > 0
        self._init_transformations()
        self._prepare_floor()
        assert self.floor_pointcloud
        self._pre_analyse(toSelf=False, toReference=self.floor_pointcloud, onlyFloor=True, sortBy='none')
        self._align_each_to(self.floor_pointcloud)
        return self._post_analyse(toReference=self.floor_pointcloud, onlyFloor=True)

    def _prepare_floor(self) -> None:
        """On the device: x, z, colour and tile kept, y = +0.0, timestamp 0, cellsize 0 (the reference goes through numpy, :399-403)."""
        assert self.original_pointcloud
        self.floor_pointcloud = cwipc_hip_flatten_y(self.original_pointcloud)


class MultiCameraToGroundTruth(_MultiCameraToCloud):
    """Align multiple cameras to a ground truth, which needs to be given with set_groundtruth().  Floors are left out of the analysis
    that sets each camera's correspondence."""

    def __init__(self) -> None:
        super().__init__()
        self.groundtruth_pointcloud: Optional[cwipc_pointcloud_wrapper] = None

    def set_groundtruth(self, pc: cwipc_pointcloud_wrapper) -> None:
        self.groundtruth_pointcloud = pc

    def run(self) -> bool:
        assert self.original_pointcloud
        assert self.groundtruth_pointcloud
        assert self.camera_count() > 0
        self._init_transformations()
        self._pre_analyse(toSelf=False, toReference=self.groundtruth_pointcloud, ignoreFloor=True, sortBy='none')
        self._align_each_to(self.groundtruth_pointcloud)
        return self._post_analyse(toReference=self.groundtruth_pointcloud)


def accept_step(corr_improvement: float, corr_count_improvement: float) -> Tuple[bool, str]:
    """Is a step that changed the correspondence by the first factor (old / new: above 1 is better) and the number of points under
    it by the second (new / old) kept?  (reference :573-596)"""
    product = corr_improvement * corr_count_improvement
    if corr_improvement >= 0.99 and corr_count_improvement >= 0.99:
        return True, "very good, accept"
    if corr_improvement >= 0.8 and corr_count_improvement >= 0.8 and product >= 1:
        return True, "good overall, accept"
    if corr_improvement >= 2 and product >= 2:
        return True, "great (but at cost of count), accept"
    if corr_improvement >= 1.5 and product >= 1.5:
        return True, "borderline, accept"
    return False, "bad, reject"


class MultiCameraIterative(BaseMulticamAlignmentAlgorithm):
    """Align multiple cameras.  The camera with the best correspondence to all others is kept as it is: it is the destination set.
    Then, again and again, the camera that matches the destination set best is aligned to it and joins it, until none is left."""

    def __init__(self) -> None:
        super().__init__()
        self.current_step_target_pointcloud: Optional[cwipc_pointcloud_wrapper] = None
        self.current_step_in_pointcloud: Optional[cwipc_pointcloud_wrapper] = None
        self.current_step_out_pointcloud: Optional[cwipc_pointcloud_wrapper] = None
        self.current_step_results: List[AnalysisResults] = []
        self.remaining_results: List[AnalysisResults] = []
        #: tile numbers in the order they joined the destination set (the first one unmoved), and those merged unaligned at the end
        self.accepted_tiles: List[int] = []
        self.merged_tiles: List[int] = []
        self.orientation_filter: Optional[float] = -0.3
        self.select_target_tile = False
        self.randomize_floor = True
        self.candidate_measure = "2mode"

    def _direction_filter_for(self, tilemask: int) -> Any:
        threshold = self.orientation_filter
        direction = self.camera_positions[self.camera_index_for_tilemask(tilemask)]
        return lambda pc: cwipc_direction_filter(pc, direction, threshold)

    def _pre_step_analyse(self, stepnum: int) -> None:
        """The cameras still to do against the destination set, best first (reference :487-522).  One analyzer at a time: each has
        its own direction filter on the reference."""
        assert self.original_pointcloud
        assert self.current_step_target_pointcloud
        assert self.remaining_results
        remaining_results: List[AnalysisResults] = []
        for rr in self.remaining_results:
            tilemask = rr.tilemask
            assert type(tilemask) == int
            analyzer = self._prepare_analyze()
            analyzer.set_ignore_floor(True)
            analyzer.set_source_pointcloud(self.original_pointcloud, tilemask)
            analyzer.set_reference_pointcloud(self.current_step_target_pointcloud)
            analyzer.set_correspondence_measure(self.candidate_measure, "tmean", "mean")
            if self.orientation_filter is not None:
                analyzer.apply_reference_filter(self._direction_filter_for(tilemask))
            analyzer.run()
            remaining_results.append(analyzer.get_results())
        remaining_results.sort(key=lambda rr: rr.minCorrespondence)
        if self.verbose:
            self._print_correspondences(f"{self.__class__.__name__}: Step {stepnum}:  Per-tile correspondence to target", remaining_results)
        self.remaining_results = remaining_results

    def _post_step_analyse(self, stepnum: int, camnum: int) -> List[AnalysisResults]:
        """The camera against the destination set before and after the step (reference :530-571)."""
        assert self.current_step_target_pointcloud and self.current_step_in_pointcloud and self.current_step_out_pointcloud
        rv: List[AnalysisResults] = []
        for pc, when in ((self.current_step_in_pointcloud, "before"), (self.current_step_out_pointcloud, "after")):
            analyzer = self._prepare_analyze()
            analyzer.set_source_pointcloud(pc)
            analyzer.set_reference_pointcloud(self.current_step_target_pointcloud)
            analyzer.set_ignore_floor(True)
            analyzer.set_correspondence_measure("2mode", "tmean", "median")
            analyzer.run()
            results = analyzer.get_results()
            results.tilemask = f"{results.tilemask} {when}"
            rv.append(results)
        if self.verbose:
            self._print_correspondences(f"{self.__class__.__name__}: Step {stepnum}: camnum {camnum}: Pre/post correspondences", rv)
        return rv

    def _accept_step(self, step: int, aligner: Any) -> Tuple[bool, bool]:
        """(keep the step, give up altogether); subclasses may decide otherwise."""
        old_rr, new_rr = self.current_step_results
        corr_improvement = old_rr.minCorrespondence / new_rr.minCorrespondence
        corr_count_improvement = new_rr.minCorrespondenceCount / old_rr.minCorrespondenceCount
        accept, verdict = accept_step(corr_improvement, corr_count_improvement)
        self._say(f"Step {step}: {verdict}, tile={old_rr.tilemask}, improvement={corr_improvement:.2f}, count_improvement={corr_count_improvement:.2f}")
        return accept, False

    def _done_step(self, step: int, tilemask: int) -> bool:
        for i in range(len(self.remaining_results)):
            if self.remaining_results[i].tilemask == tilemask:
                del self.remaining_results[i]
                self.accepted_tiles.append(tilemask)
                return True
        assert False, f"Tilemask {tilemask} not in self.remaining_results"

    def _select_first_step(self) -> int:
        rr = self.pre_analysis_results[0]
        assert type(rr.tilemask) == int
        self._say(f"Step 0: tile={rr.tilemask}")
        return rr.tilemask

    def _select_next_step(self, step: int) -> Tuple[int, float, Optional[int]]:
        rr = self.remaining_results[0]
        assert type(rr.tilemask) == int
        self._say(f"Step {step}: tile={rr.tilemask}, corr={rr.minCorrespondence:.4f}")
        return rr.tilemask, rr.minCorrespondence, None

    def _still_to_do(self) -> List[int]:
        return [rr.tilemask for rr in self.remaining_results]   # type: ignore

    def _downsample_size(self) -> float:
        return 0

    def _optional_apply_floor_filter(self) -> None:
        pass

    def run(self) -> bool:
        assert self.original_pointcloud
        assert self.camera_count() > 0
        self._init_transformations()
        self._pre_analyse(toSelf=True, ignoreFloor=True, sortBy='corr')
        self._pre_analyse(toSelf=False, ignoreFloor=True, sortBy='corr')
        cellsize = self._downsample_size()
        if cellsize > 0:
            self.original_pointcloud = cwipc_downsample_pertile(self.original_pointcloud, cellsize)
            self._pre_analyse(toSelf=True, ignoreFloor=True, sortBy='corr')
            self._pre_analyse(toSelf=False, ignoreFloor=True, sortBy='corr')
        # the first camera stays as it is: the destination set
        first_tilemask = self._select_first_step()
        self.remaining_results = copy.copy(self.pre_analysis_results)
        self._done_step(0, first_tilemask)
        self.current_step_target_pointcloud = self.get_pc_for_tilemask(first_tilemask)
        step = 0
        give_up = False
        failures_this_step = 0
        need_new_analysis = True
        while self.remaining_results and not give_up:
            assert self.current_step_target_pointcloud
            assert self.current_step_target_pointcloud.count() > 0
            step += 1
            if need_new_analysis:
                self._pre_step_analyse(step)
            tilemask, corr, targettile = self._select_next_step(step)
            if self.correspondence is not None:
                corr = self.correspondence
            self.current_step_in_pointcloud = self.get_pc_for_tilemask(tilemask)
            self._optional_apply_floor_filter()
            aligner = self._prepare_aligner()
            aligner.set_source_pointcloud(self.current_step_in_pointcloud)
            aligner.set_reference_pointcloud(self.current_step_target_pointcloud, targettile)
            aligner.set_correspondence(corr)
            if self.orientation_filter is not None:
                aligner.apply_reference_filter(self._direction_filter_for(tilemask))
            aligner.run()
            self.current_step_out_pointcloud = aligner.get_result_pointcloud()
            self.current_step_results = self._post_step_analyse(step, tilemask)
            if self.verbose:
                translation, rotation = transformation_compare(None, aligner.get_result_transformation())
                self._say(f"Step {step}: change: distance={np.linalg.norm(translation):.4f}, angle={np.linalg.norm(rotation):.1f}, "
                          f"translation={translation}, rotation={rotation}")
            accept, give_up = self._accept_step(step, aligner)
            if accept:
                failures_this_step = 0
                need_new_analysis = True
                self._say(f"Step {step}: accepted alignment for camnum={tilemask}")
                self._done_step(step, tilemask)
                self.current_step_target_pointcloud = aligner.get_result_pointcloud_full()
                self.current_step_in_pointcloud = None
                self.current_step_out_pointcloud = None
                self._apply_step(self.camera_index_for_tilemask(tilemask), aligner)
            elif not give_up:
                failures_this_step += 1
                need_new_analysis = False
                self._say(f"Step {step}: failed for camnum={tilemask}")
                self.current_step_in_pointcloud = None
                self.current_step_out_pointcloud = None
                # everything has been tried: give up
                if failures_this_step > len(self.remaining_results) + 1:
                    self._say(f"failed {failures_this_step} times.")
                    give_up = True
                # try another camera next
                self.remaining_results.append(self.remaining_results.pop(0))
        # the cameras that were given up on join the result as they are
        self.merged_tiles = self._still_to_do()
        for tilemask in self.merged_tiles:
            self.current_step_target_pointcloud = cwipc_join(self.current_step_target_pointcloud, self.get_pc_for_tilemask(tilemask))
        assert self.current_step_target_pointcloud
        assert self.current_step_target_pointcloud.count() > 0
        self.original_pointcloud = self.current_step_target_pointcloud
        self.current_step_target_pointcloud = None
        return self._post_analyse()


DEFAULT_MULTICAMERA_ALGORITHM = MultiCameraIterative

ALL_MULTICAMERA_ALGORITHMS = [MultiCameraOneToAllOthers, MultiCameraToFloor, MultiCameraIterative, MultiCameraToGroundTruth]
