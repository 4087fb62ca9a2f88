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

OverlapAnalyzer, the reference's third analyzer (open3d's evaluate_registration there), is one correspondence search and two sums
on the device (cwipc_hip_icp_sums at the identity): the fraction of source points with a reference point within the
correspondence, and the root mean square of their distances.
"""
import math
from typing import Any, List, Optional, Tuple

import numpy as np

from ..util import (cwipc_pointcloud_wrapper, cwipc_tilefilter_masked, cwipc_crop, cwipc_hip_nn_distance,
                    cwipc_hip_gaussian_kde, cwipc_hip_icp_sums)
from .abstract import AnalysisAlgorithm, AnalysisResults, OverlapAnalysisResults

__all__ = ['RegistrationAnalyzer', 'RegistrationAnalyzerSymmetric', 'OverlapAnalyzer', 'DEFAULT_ANALYZER_ALGORITHM',
           'ALL_ANALYZER_ALGORITHMS', 'trim_mean', 'FLOOR_Y']

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
        self._source_pointcloud: Optional[cwipc_pointcloud_wrapper] = None
        self._reference_pointcloud: Optional[cwipc_pointcloud_wrapper] = None
        self.source_tilemask: Optional[int] = None
        self.reference_tilemask: Optional[int] = None
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
        if before == 0:
            print(f"{name}: set_{which}_pointcloud: Warning: pre_count={before}")
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

    def set_source_pointcloud(self, pc: cwipc_pointcloud_wrapper, tilemask: Optional[int] = None) -> None:
        self._source_pointcloud = self._masked("source", pc, tilemask)
        self.source_tilemask = tilemask

    def set_reference_pointcloud(self, pc: cwipc_pointcloud_wrapper, tilemask: Optional[int] = None) -> None:
        self._reference_pointcloud = self._masked("reference", pc, tilemask)
        self.reference_tilemask = tilemask

    def get_source_pointcloud(self) -> cwipc_pointcloud_wrapper:
        assert self._source_pointcloud
        return self._source_pointcloud

    def get_reference_pointcloud(self) -> cwipc_pointcloud_wrapper:
        assert self._reference_pointcloud
        return self._reference_pointcloud

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
    def _prepare(self) -> Tuple[cwipc_pointcloud_wrapper, cwipc_pointcloud_wrapper, List[cwipc_pointcloud_wrapper]]:
        """A fresh result record and the two clouds the distances are taken between, still on the device; the third value lists
        the clouds made here, for the caller to free."""
        self.results = AnalysisResults()
        self.results.algorithm = self.__class__.__name__
        self.results.tilemask = self.source_tilemask
        self.results.referenceTilemask = self.reference_tilemask
        if self.variants:
            self.results.variant = ",".join(self.variants)
        made: List[cwipc_pointcloud_wrapper] = []
        clouds = []
        for pc in (self.get_source_pointcloud(), self.get_reference_pointcloud()):
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

    def run(self) -> bool:
        source, reference, made = self._prepare()
        try:
            distances = self._distances(source, reference)
        finally:
            for pc in made:
                pc.free()
        return self._analyze(distances)


class RegistrationAnalyzerSymmetric(_BaseRegistrationAnalyzer):
    """Distances both ways round -- source points to the reference cloud, reference points to the source cloud -- as one set."""

    def run(self) -> bool:
        source, reference, made = self._prepare()
        try:
            distances = np.concatenate((self._distances(source, reference), self._distances(reference, source)))
        finally:
            for pc in made:
                pc.free()
        if not self._analyze(distances):
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
        self.correspondence: float = np.inf
        self.results: Optional[OverlapAnalysisResults] = None

    def _masked(self, pc: cwipc_pointcloud_wrapper, tilemask: Optional[int]) -> cwipc_pointcloud_wrapper:
        return cwipc_tilefilter_masked(pc, tilemask) if tilemask else pc

    def set_source_pointcloud(self, pc: cwipc_pointcloud_wrapper, tilemask: Optional[int] = None) -> None:
        self._source_pointcloud = self._masked(pc, tilemask)
        self.source_tilemask = tilemask

    def set_reference_pointcloud(self, pc: cwipc_pointcloud_wrapper, tilemask: Optional[int] = None) -> None:
        self._reference_pointcloud = self._masked(pc, tilemask)
        self.reference_tilemask = tilemask

    def set_correspondence(self, correspondence: float) -> None:
        """The largest distance between two points that still counts as a match."""
        self.correspondence = correspondence

    def run(self) -> bool:
        assert self._source_pointcloud is not None and self._reference_pointcloud is not None
        source, reference = self._source_pointcloud, self._reference_pointcloud
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


DEFAULT_ANALYZER_ALGORITHM = RegistrationAnalyzerSymmetric

ALL_ANALYZER_ALGORITHMS = [RegistrationAnalyzer, RegistrationAnalyzerSymmetric, OverlapAnalyzer]
