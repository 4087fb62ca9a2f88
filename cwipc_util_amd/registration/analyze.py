"""How well are two point clouds registered?  (reference python/cwipc/registration/analyze.py: RegistrationAnalyzer,
RegistrationAnalyzerSymmetric -- the default analyzer of cwipc_register, cwipc_analyze_registration, cwipc_find_transform and of
every step of registration/multicamera.py)

Per point of the source cloud the distance to its (ignore_nearest + 1)-th nearest point of the reference cloud (the symmetric
analyzer: both ways round, concatenated), points without one under max_correspondence_distance left out; then a histogram of those
distances -- a Gaussian kernel density estimate at the bin edges by default -- and the measures read off the array and the curve.

Where it runs: the clouds stay on the device (tile mask and floor filter are device compactions); the distances
(cwipc_hip_nn_distance) and the density estimate (cwipc_hip_gaussian_kde) are GPU kernels; only the distances come back.  The
reductions over them -- mean, std, median, trimmed mean, percentile, count -- are numpy on the host on purpose: the array is bit for
bit the one the reference gets from scipy's KD-tree, so the same numpy calls give the same numbers.  scipy is not needed.

The clouds an analyzer is given are masked when they are first asked for, not when they are set, and filters can be applied to them
(apply_source_filter, apply_reference_filter: reference registration/util.py:367-395).  run_analyzers_batched runs a list of analyzers
that look at subsets of ONE pair of clouds -- every camera of a frame against the others, as registration/multicamera.py asks -- with
one cwipc_hip_nn_distance_jobs call per direction: no tile compaction, no floor crop, one grid; the distances are the per-analyzer
path's bit for bit, so the results are too.

OverlapAnalyzer, the reference's third analyzer (open3d's evaluate_registration there), is one correspondence search and two sums
on the device (cwipc_hip_icp_sums at the identity): the fraction of source points with a reference point within the
correspondence, and the root mean square of their distances.
"""
import math
from typing import Any, Callable, List, Optional, Sequence, Tuple

import numpy as np

from ..util import (cwipc_pointcloud_wrapper, cwipc_tilefilter_masked, cwipc_crop, cwipc_floor_filter, cwipc_hip_nn_distance,
                    cwipc_hip_nn_distance_jobs, NNJob, cwipc_hip_gaussian_kde, cwipc_hip_icp_sums)
from .abstract import AnalysisAlgorithm, AnalysisResults, OverlapAnalysisResults

__all__ = ['RegistrationAnalyzer', 'RegistrationAnalyzerSymmetric', 'OverlapAnalyzer', 'DEFAULT_ANALYZER_ALGORITHM',
           'ALL_ANALYZER_ALGORITHMS', 'trim_mean', 'FLOOR_Y', 'run_analyzers_batched', 'build_analyzer_jobs']

PointCloudFilter = Callable[[cwipc_pointcloud_wrapper], cwipc_pointcloud_wrapper]

#: the floor filter keeps a point iff its float32 y > 0.1
FLOOR_Y = 0.1


def trim_mean(a: np.ndarray, proportiontocut: float) -> float:
    """scipy.stats.trim_mean for a one-dimensional array: the mean of what is left when int(proportiontocut * n) values are cut from
    each end -- the same numpy.partition call and the same numpy.mean over the same slice, hence the same bits."""
    a = np.asarray(a)
    if a.size == 0:
        return float('nan')
    nobs = a.shape[0]
    lowercut = int(proportiontocut * nobs)
    uppercut = nobs - lowercut
    if lowercut > uppercut:
        raise ValueError("Proportion too big.")
    part = np.partition(a, (lowercut, uppercut - 1), 0)
    return np.mean(part[lowercut:uppercut], axis=0)


def _floor_filter(pc: cwipc_pointcloud_wrapper) -> cwipc_pointcloud_wrapper:
    """The points with float32 y > 0.1, on the device: a crop whose only finite face is the next float32 above 0.1 (the box is
    half-open: miny <= y)."""
    inf = math.inf
    miny = float(np.nextafter(np.float32(FLOOR_Y), np.float32(np.inf)))
    return cwipc_crop(pc, (-inf, inf, miny, inf, -inf, inf))


class _BaseRegistrationAnalyzer(AnalysisAlgorithm):
    def __init__(self) -> None:
        # per side: the cloud as it was given, the masked cloud (made when first asked for), the cloud after the applied filters
        self._source_given: Optional[cwipc_pointcloud_wrapper] = None
        self._reference_given: Optional[cwipc_pointcloud_wrapper] = None
        self._source_pointcloud: Optional[cwipc_pointcloud_wrapper] = None
        self._reference_pointcloud: Optional[cwipc_pointcloud_wrapper] = None
        self._filtered_source_pointcloud: Optional[cwipc_pointcloud_wrapper] = None
        self._filtered_reference_pointcloud: Optional[cwipc_pointcloud_wrapper] = None
        self._filters_applied = 0
        self.source_tilemask: Optional[int] = None
        self.reference_tilemask: Optional[int] = None
        #: a floor level: only the source points with y < level take part (set_source_floor_only)
        self.source_floor_only: Optional[float] = None
        self.verbose = False
        self.histogram_bincount = 400
        self.max_correspondence_distance: float = np.inf
        self.histogram_binsize: float = 0.0
        self.correspondence_measure: str = "mean"
        self.all_measures: List[str] = []
        self.results = AnalysisResults()
        self.gaussian_bw_method: Any = None
        self.ignore_nearest: int = 0
        self.ignore_floor: bool = False
        self.use_kde = True
        self.variants: List[str] = []

    # ---- the clouds ----
    def _masked(self, which: str, pc: cwipc_pointcloud_wrapper, tilemask: Optional[int]) -> cwipc_pointcloud_wrapper:
        name = self.__class__.__name__
        before = pc.count()
        if tilemask is None:
            if self.verbose:
                print(f"{name}: Setting {which} point cloud with {before} points")
            return pc
        if tilemask != 0:
            pc = cwipc_tilefilter_masked(pc, tilemask)
        after = pc.count()
        if after == 0:
            print(f"{name}: set_{which}_pointcloud: Warning: tilemask={tilemask}, post_count={after}")
        if self.verbose:
            print(f"{name}: Setting {which} point cloud with {after} (of {before}) points using tilemask {tilemask:#x}")
        return pc

    def _given(self, which: str, pc: cwipc_pointcloud_wrapper) -> cwipc_pointcloud_wrapper:
        if pc.count() == 0:
            print(f"{self.__class__.__name__}: set_{which}_pointcloud: Warning: pre_count=0")
        return pc

    def set_source_pointcloud(self, pc: cwipc_pointcloud_wrapper, tilemask: Optional[int] = None) -> None:
        """The tile mask is applied when the cloud is first asked for: a batched run (run_analyzers_batched) never asks."""
        self._source_given = self._given("source", pc)
        self._source_pointcloud = None
        self._filtered_source_pointcloud = None
        self.source_tilemask = tilemask

    def set_reference_pointcloud(self, pc: cwipc_pointcloud_wrapper, tilemask: Optional[int] = None) -> None:
        self._reference_given = self._given("reference", pc)
        self._reference_pointcloud = None
        self._filtered_reference_pointcloud = None
        self.reference_tilemask = tilemask

    def get_source_pointcloud(self) -> cwipc_pointcloud_wrapper:
        if self._source_pointcloud is None:
            assert self._source_given is not None
            self._source_pointcloud = self._masked("source", self._source_given, self.source_tilemask)
        return self._source_pointcloud

    def get_reference_pointcloud(self) -> cwipc_pointcloud_wrapper:
        if self._reference_pointcloud is None:
            assert self._reference_given is not None
            self._reference_pointcloud = self._masked("reference", self._reference_given, self.reference_tilemask)
        return self._reference_pointcloud

    # ---- filters (reference registration/util.py:367-395) ----
    def get_filtered_source_pointcloud(self) -> cwipc_pointcloud_wrapper:
        if self._filtered_source_pointcloud is not None:
            return self._filtered_source_pointcloud
        return self.get_source_pointcloud()

    def get_filtered_reference_pointcloud(self) -> cwipc_pointcloud_wrapper:
        if self._filtered_reference_pointcloud is not None:
            return self._filtered_reference_pointcloud
        return self.get_reference_pointcloud()

    def apply_source_filter(self, filter: PointCloudFilter) -> None:
        """The distances are taken from the filtered cloud; filters applied one after the other stack."""
        self._filtered_source_pointcloud = filter(self.get_filtered_source_pointcloud())
        self._filters_applied += 1

    def apply_reference_filter(self, filter: PointCloudFilter) -> None:
        self._filtered_reference_pointcloud = filter(self.get_filtered_reference_pointcloud())
        self._filters_applied += 1

    def set_source_floor_only(self, level: Optional[float] = FLOOR_Y) -> None:
        """Only the source points on the floor (y < level) take part: apply_source_filter(lambda pc: cwipc_floor_filter(pc, keep=True))
        as a setting -- a batched run can read a setting, it cannot read a lambda.  None: off."""
        self.source_floor_only = level

    # ---- settings ----
    def set_correspondence_measure(self, method: str, *other_methods: str) -> None:
        self.correspondence_measure = method
        self.all_measures = list(other_methods)
        if method not in self.all_measures:
            self.all_measures.append(method)

    def set_min_correspondence_distance(self, correspondence: float) -> None:
        """The smallest distance that means something: the width of a histogram bin."""
        self.histogram_binsize = correspondence

    def set_max_correspondence_distance(self, correspondence: float) -> None:
        """Points further than this from every point of the other cloud are not matched."""
        self.max_correspondence_distance = correspondence

    def set_ignore_nearest(self, ignore_nearest: int) -> None:
        """Skip this many nearest points (1 when a cloud is compared with itself)."""
        self.ignore_nearest = ignore_nearest
        self.variants.append(f"ignore_nearest={ignore_nearest}")

    def set_ignore_floor(self, ignoreFloor: bool) -> None:
        self.ignore_floor = ignoreFloor
        self.variants.append("ignore_floor")

    def get_results(self) -> AnalysisResults:
        assert self.results
        return self.results

    # ---- one run ----
    def _new_results(self) -> None:
        self.results = AnalysisResults()
        self.results.algorithm = self.__class__.__name__
        self.results.tilemask = self.source_tilemask
        self.results.referenceTilemask = self.reference_tilemask
        if self.variants:
            self.results.variant = ",".join(self.variants)

    def _prepare(self) -> Tuple[cwipc_pointcloud_wrapper, cwipc_pointcloud_wrapper, List[cwipc_pointcloud_wrapper]]:
        """A fresh result record and the two clouds the distances are taken between, still on the device; the third value lists
        the clouds made here, for the caller to free."""
        self._new_results()
        made: List[cwipc_pointcloud_wrapper] = []
        clouds = []
        source = self.get_filtered_source_pointcloud()
        if self.source_floor_only is not None:
            source = cwipc_floor_filter(source, self.source_floor_only, keep=True)
            made.append(source)
        for pc in (source, self.get_filtered_reference_pointcloud()):
            if self.ignore_floor:
                kept = _floor_filter(pc)
                made.append(kept)
                if self.verbose:
                    print(f"\t\tFloor filter kept {kept.count()} of {pc.count()} points")
                pc = kept
            clouds.append(pc)
        self.results.sourcePointCount = clouds[0].count()
        self.results.referencePointCount = clouds[1].count()
        return clouds[0], clouds[1], made

    def _distances(self, source: cwipc_pointcloud_wrapper, reference: cwipc_pointcloud_wrapper) -> np.ndarray:
        return cwipc_hip_nn_distance(source, reference, self.ignore_nearest, self.max_correspondence_distance)

    def _compute_histogram_parameters(self, distances: np.ndarray) -> bool:
        """Bin width and bin count, one from the other; False when all distances are the same."""
        max_distance = np.max(distances)
        min_distance = np.min(distances)
        if min_distance == max_distance:
            return False
        if min_distance > 0:
            min_distance = 0
        span = max_distance - min_distance
        if self.histogram_binsize > 0:
            self.histogram_bincount = int(span / self.histogram_binsize)
            if self.verbose:
                print(f"\t\tmin={min_distance}, max={max_distance}, bincount={self.histogram_bincount} (based on min_correspondence_distance={self.histogram_binsize})")
        else:
            assert self.histogram_bincount > 0, "Either histogram_binsize or histogram_bincount must be set"
            self.histogram_binsize = span / self.histogram_bincount
            if self.verbose:
                print(f"\t\tmin={min_distance}, max={max_distance}, min_correspondence_distance={self.histogram_binsize} (based on bincount={self.histogram_bincount})")
        mismatch = span - self.histogram_bincount * self.histogram_binsize
        assert abs(mismatch) <= self.histogram_binsize, f"Mismatch in histogram parameters: mismatch={mismatch} (max={max_distance}, min={min_distance}, bincount={self.histogram_bincount}, binsize={self.histogram_binsize})"
        return True

    def _compute_histogram(self, distances: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        assert self.histogram_bincount > 0 and self.histogram_binsize > 0
        if self.use_kde:
            edges = np.linspace(0, np.max(distances), self.histogram_bincount + 1)
            values = cwipc_hip_gaussian_kde(distances, edges[1:], self.gaussian_bw_method)
            if self.verbose:
                print(f"\t\tgaussian_kde: nPoint={len(distances)}")
            return values, edges
        return np.histogram(distances, bins=self.histogram_bincount)

    def _compute_correspondence_errors(self, distances: np.ndarray) -> None:
        r = self.results
        if not self.all_measures:
            self.all_measures = [self.correspondence_measure]
        wanted = self.all_measures
        r.median = float(np.median(distances)) if "median" in wanted else None
        r.mean = float(np.mean(distances)) if "mean" in wanted else None
        r.stddev = float(np.std(distances)) if "mean" in wanted else None
        r.tmean = float(trim_mean(distances, 0.1)) if "tmean" in wanted else None
        r.mode = None
        if "mode" in wanted or "2mode" in wanted:
            # the upper edge of the highest bin
            r.mode = r.histogramEdges[np.argmax(r.histogram) + 1]
        measure = self.correspondence_measure
        if measure in ("mean", "tmean", "median", "mode"):
            value = getattr(r, measure)
            assert value is not None
        elif measure == "2mode":
            assert r.mode is not None
            value = 2 * r.mode
        elif measure.startswith("q="):
            value = float(np.percentile(distances, int(measure[2:])))
        else:
            assert False, f"Unknown correspondence_method '{measure}'"
        r.minCorrespondence = value
        r.minCorrespondenceCount = np.count_nonzero(distances <= value)
        if self.verbose:
            total = r.sourcePointCount
            print(f"\t\tresult: tilemask={r.tilemask}, corr={r.minCorrespondence}, nPoint={r.minCorrespondenceCount} of {total}, fraction={r.minCorrespondenceCount / total}")

    def _analyze(self, distances: np.ndarray) -> bool:
        distances = distances[np.isfinite(distances)]
        if not self._compute_histogram_parameters(distances):
            print("Warning: all distances are the same")
            value = distances[0]
            self.results.minCorrespondence = value
            self.results.minCorrespondenceCount = distances.shape[0]
            self.results.histogram = np.array([value])
            self.results.histogramEdges = np.array([value, value])
            return False
        self.results.histogram, self.results.histogramEdges = self._compute_histogram(distances)
        self._compute_correspondence_errors(distances)
        return True


class RegistrationAnalyzer(_BaseRegistrationAnalyzer):
    """Distances from every source point to the reference cloud."""
    directions = 1

    def run(self) -> bool:
        source, reference, made = self._prepare()
        try:
            distances = self._distances(source, reference)
        finally:
            for pc in made:
                pc.free()
        return self._finish([distances])

    def _finish(self, rows: Sequence[np.ndarray]) -> bool:
        """From the distances (one array per direction of `directions`) to the results; the point counts are set already."""
        return self._analyze(rows[0])


class RegistrationAnalyzerSymmetric(_BaseRegistrationAnalyzer):
    """Distances both ways round -- source points to the reference cloud, reference points to the source cloud -- as one set."""
    directions = 2

    def run(self) -> bool:
        source, reference, made = self._prepare()
        try:
            rows = [self._distances(source, reference), self._distances(reference, source)]
        finally:
            for pc in made:
                pc.free()
        return self._finish(rows)

    def _finish(self, rows: Sequence[np.ndarray]) -> bool:
        if not self._analyze(np.concatenate((rows[0], rows[1]))):
            return False
        # both counts become the number of points that took part
        total = self.results.sourcePointCount + self.results.referencePointCount
        self.results.sourcePointCount = total
        self.results.referencePointCount = total
        return True


class OverlapAnalyzer:
    """How much of the source cloud overlaps the reference cloud: fitness = the fraction of source points that have a reference
    point closer than the correspondence, rmse = the root mean square of those points' distances to their nearest reference point."""

    def __init__(self) -> None:
        self._source_pointcloud: Optional[cwipc_pointcloud_wrapper] = None
        self._reference_pointcloud: Optional[cwipc_pointcloud_wrapper] = None
        self.source_tilemask: Optional[int] = None
        self.reference_tilemask: Optional[int] = None
        self.verbose = False
        self._filtered_source_pointcloud: Optional[cwipc_pointcloud_wrapper] = None
        self._filtered_reference_pointcloud: Optional[cwipc_pointcloud_wrapper] = None
        self.correspondence: float = np.inf
        self.results: Optional[OverlapAnalysisResults] = None

    def _masked(self, pc: cwipc_pointcloud_wrapper, tilemask: Optional[int]) -> cwipc_pointcloud_wrapper:
        return cwipc_tilefilter_masked(pc, tilemask) if tilemask else pc

    def set_source_pointcloud(self, pc: cwipc_pointcloud_wrapper, tilemask: Optional[int] = None) -> None:
        self._source_pointcloud = self._masked(pc, tilemask)
        self._filtered_source_pointcloud = None
        self.source_tilemask = tilemask

    def set_reference_pointcloud(self, pc: cwipc_pointcloud_wrapper, tilemask: Optional[int] = None) -> None:
        self._reference_pointcloud = self._masked(pc, tilemask)
        self._filtered_reference_pointcloud = None
        self.reference_tilemask = tilemask

    def get_source_pointcloud(self) -> cwipc_pointcloud_wrapper:
        assert self._source_pointcloud is not None
        return self._source_pointcloud

    def get_reference_pointcloud(self) -> cwipc_pointcloud_wrapper:
        assert self._reference_pointcloud is not None
        return self._reference_pointcloud

    def get_filtered_source_pointcloud(self) -> cwipc_pointcloud_wrapper:
        return self._filtered_source_pointcloud if self._filtered_source_pointcloud is not None else self.get_source_pointcloud()

    def get_filtered_reference_pointcloud(self) -> cwipc_pointcloud_wrapper:
        return self._filtered_reference_pointcloud if self._filtered_reference_pointcloud is not None else self.get_reference_pointcloud()

    def apply_source_filter(self, filter: PointCloudFilter) -> None:
        self._filtered_source_pointcloud = filter(self.get_filtered_source_pointcloud())

    def apply_reference_filter(self, filter: PointCloudFilter) -> None:
        self._filtered_reference_pointcloud = filter(self.get_filtered_reference_pointcloud())

    def set_correspondence(self, correspondence: float) -> None:
        """The largest distance between two points that still counts as a match."""
        self.correspondence = correspondence

    def run(self) -> bool:
        source, reference = self.get_filtered_source_pointcloud(), self.get_filtered_reference_pointcloud()
        count = source.count()
        n, sums = cwipc_hip_icp_sums(source, reference, None, self.correspondence)
        r = OverlapAnalysisResults()
        r.fitness = n / count if count else 0.0
        r.rmse = math.sqrt(sums[15] / n) if n else 0.0
        r.sourcePointCount = count
        r.referencePointCount = reference.count()
        r.tilemask = self.source_tilemask
        r.referenceTilemask = self.reference_tilemask
        self.results = r
        if self.verbose:
            print(f"{self.__class__.__name__}: fitness={r.fitness}, rmse={r.rmse}, {n} of {count} points")
        return True

    def get_results(self) -> OverlapAnalysisResults:
        assert self.results
        return self.results


# ---- a list of analyzers over one pair of clouds, as one batch ----
MAX_BATCH_JOBS = 64


def _job_mask(tilemask: Optional[int]) -> Optional[int]:
    """The job's mask byte for an analyzer's tile mask (None and 0: every tile, a job's 0), or None for a mask a byte cannot hold."""
    if tilemask is None:
        return 0
    if not isinstance(tilemask, (int, np.integer)) or tilemask < 0 or tilemask > 255:
        return None
    return int(tilemask)


def build_analyzer_jobs(analyzers: Sequence[Any]) -> Optional[Tuple[List[NNJob], List[NNJob], List[int]]]:
    """The jobs that run `analyzers` as one batch: (forward jobs, one per analyzer, for the call on (source, reference); backward jobs
    for the call on (reference, source); which analyzer each backward job belongs to -- the symmetric ones, in order).  None when
    the list does not qualify: every analyzer must be a RegistrationAnalyzer or RegistrationAnalyzerSymmetric with its own run(), all
    must have been given the same source cloud object and the same reference cloud object, none may have had a filter callable applied,
    and masks, ignore_nearest and max_correspondence_distance must be what a job can hold.  What may differ: the tile masks, the floor
    settings (ignore_floor, source_floor_only), and whatever does not touch the search (measures, histogram settings)."""
    if not analyzers:
        return None
    first = analyzers[0]
    forward: List[NNJob] = []
    backward: List[NNJob] = []
    owners: List[int] = []
    for i, a in enumerate(analyzers):
        if type(a) not in (RegistrationAnalyzer, RegistrationAnalyzerSymmetric):
            return None
        if a._source_given is None or a._reference_given is None:
            return None
        if a._source_given is not first._source_given or a._reference_given is not first._reference_given:
            return None
        if a._filters_applied:
            return None
        smask, rmask = _job_mask(a.source_tilemask), _job_mask(a.reference_tilemask)
        if smask is None or rmask is None:
            return None
        nth, bound = a.ignore_nearest, a.max_correspondence_distance
        if not isinstance(nth, (int, np.integer)) or nth < 0 or nth > 31 or not (bound > 0):
            return None
        inf = math.inf
        floor_lo = NNJob.ignore_floor(FLOOR_Y)[0] if a.ignore_floor else -inf
        source_y = (floor_lo, NNJob.floor_only(a.source_floor_only)[1] if a.source_floor_only is not None else inf)
        reference_y = (floor_lo, inf)
        forward.append(NNJob(source_mask=smask, reference_mask=rmask, nth=nth, max_distance=bound, source_y=source_y, reference_y=reference_y))
        if a.directions == 2:
            backward.append(NNJob(source_mask=rmask, reference_mask=smask, nth=nth, max_distance=bound, source_y=reference_y, reference_y=source_y))
            owners.append(i)
    return forward, backward, owners


def _reference_count(a: Any, cache: dict) -> int:
    """How many reference points take part in a one-directional analyzer's run: through the very filters of its _prepare, once per
    distinct (mask, floor) of the batch."""
    key = (a.reference_tilemask, a.ignore_floor)
    if key not in cache:
        pc = a.get_reference_pointcloud()
        if a.ignore_floor:
            kept = _floor_filter(pc)
            cache[key] = kept.count()
            kept.free()
        else:
            cache[key] = pc.count()
    return cache[key]


def run_analyzers_batched(analyzers: Sequence[Any]) -> List[bool]:
    """run() for every analyzer of the list; what each run() would have returned.  A list that qualifies (build_analyzer_jobs) makes
    one cwipc_hip_nn_distance_jobs call per direction -- forward for all, backward for the symmetric analyzers -- in place of two
    compactions, two floor crops, a grid and a search per analyzer and direction; any other list is run one by one.  Either way the
    AnalysisResults are the same, bit for bit: a job's row IS the array the per-analyzer search returns.  Fewer launches is not
    less time: on an MI355X the batch measured slower than the analyzers one by one."""
    analyzers = list(analyzers)
    built = build_analyzer_jobs(analyzers)
    if built is None:
        return [a.run() for a in analyzers]
    forward, backward, owners = built
    source, reference = analyzers[0]._source_given, analyzers[0]._reference_given

    def rows_of(src: cwipc_pointcloud_wrapper, ref: cwipc_pointcloud_wrapper, jobs: List[NNJob]) -> List[np.ndarray]:
        rows: List[np.ndarray] = []
        for at in range(0, len(jobs), MAX_BATCH_JOBS):
            rows.extend(cwipc_hip_nn_distance_jobs(src, ref, jobs[at:at + MAX_BATCH_JOBS]))
        return rows

    forward_rows = rows_of(source, reference, forward)
    backward_rows = dict(zip(owners, rows_of(reference, source, backward)))
    counts: dict = {}
    rv = []
    for i, a in enumerate(analyzers):
        a._new_results()
        a.results.sourcePointCount = int(forward_rows[i].shape[0])
        if a.directions == 2:
            a.results.referencePointCount = int(backward_rows[i].shape[0])
            rv.append(a._finish([forward_rows[i], backward_rows[i]]))
        else:
            same_side = (source is reference and forward[i].source_mask == forward[i].reference_mask and
                         tuple(forward[i].source_y) == tuple(forward[i].reference_y))
            a.results.referencePointCount = a.results.sourcePointCount if same_side else _reference_count(a, counts)
            rv.append(a._finish([forward_rows[i]]))
    return rv


DEFAULT_ANALYZER_ALGORITHM = RegistrationAnalyzerSymmetric

ALL_ANALYZER_ALGORITHMS = [RegistrationAnalyzer, RegistrationAnalyzerSymmetric, OverlapAnalyzer]
