"""Result record and interface of the registration analyzers (the surface of reference python/cwipc/registration/abstract.py that
the analyzers use: AnalysisResults, AnalysisAlgorithm)."""
from abc import ABC, abstractmethod
from typing import Optional, Union

import numpy

from ..util import cwipc_pointcloud_wrapper

__all__ = ['AnalysisResults', 'AnalysisAlgorithm', 'OverlapAnalysisResults']


class AnalysisResults:
    """What an analyzer found out about one pair of clouds."""

    def __init__(self) -> None:
        #: the correspondence the chosen measure gives, and how many distances lie at or under it
        self.minCorrespondence: float = 0
        self.minCorrespondenceCount: int = 0
        #: the measures that were asked for (None otherwise)
        self.mean: Optional[float] = None
        self.stddev: Optional[float] = None
        self.tmean: Optional[float] = None
        self.mode: Optional[float] = None
        self.median: Optional[float] = None
        #: points that took part (the symmetric analyzer: both clouds together, in both fields)
        self.sourcePointCount: int = 0
        self.referencePointCount: int = 0
        self.tilemask: Union[None, int, str] = None
        self.referenceTilemask: Optional[int] = None
        #: the distances' histogram, or their kernel density estimate at the upper bin edges, and the bin edges
        self.histogram: Optional[numpy.ndarray] = None
        self.histogramEdges: Optional[numpy.ndarray] = None
        self.algorithm: str = ""
        self.variant: Optional[str] = None

    def tostr(self) -> str:
        """One line for a person to read."""
        percentage = (self.minCorrespondenceCount / self.sourcePointCount) * 100
        parts = [f"correspondence: {self.minCorrespondence:.4f}", f"count: {self.minCorrespondenceCount}", f"percentage: {percentage:.0f}%"]
        for name in ("mean", "stddev", "tmean", "mode", "median"):
            value = getattr(self, name)
            if value is not None:
                parts.append(f"{name}={value:.4f}")
        return ", ".join(parts)


class OverlapAnalysisResults:
    """What the overlap analyzer found out about one pair of clouds."""

    def __init__(self) -> None:
        #: matched source points / source points: higher is better
        self.fitness: float = 0.0
        #: root mean square of the matched points' distances: lower is better
        self.rmse: float = 0.0
        self.sourcePointCount: int = 0
        self.referencePointCount: int = 0
        self.tilemask: Optional[int] = None
        self.referenceTilemask: Optional[int] = None


class AnalysisAlgorithm(ABC):
    """An algorithm that looks at a source and a reference cloud and says how well they are registered."""
    verbose: bool

    @abstractmethod
    def set_source_pointcloud(self, pc: cwipc_pointcloud_wrapper, tilemask: Optional[int] = None) -> None: ...

    @abstractmethod
    def set_reference_pointcloud(self, pc: cwipc_pointcloud_wrapper, tilemask: Optional[int] = None) -> None: ...

    @abstractmethod
    def set_correspondence_measure(self, method: str, *other_methods: str) -> None: ...

    @abstractmethod
    def set_max_correspondence_distance(self, correspondence: float) -> None: ...

    @abstractmethod
    def set_min_correspondence_distance(self, correspondence: float) -> None: ...

    @abstractmethod
    def set_ignore_nearest(self, ignore_nearest: int) -> None: ...

    @abstractmethod
    def set_ignore_floor(self, ignoreFloor: bool) -> None: ...

    @abstractmethod
    def run(self) -> bool: ...

    @abstractmethod
    def get_results(self) -> AnalysisResults: ...
