"""Result records and interfaces of the registration tooling (the surface of reference python/cwipc/registration/abstract.py that
the analyzers, the aligners and the multi-camera algorithms use: AnalysisResults, AnalysisAlgorithm, AlignmentAlgorithm,
MulticamAlgorithm, MulticamAlignmentAlgorithm)."""
from abc import ABC, abstractmethod
from typing import Any, List, Optional, Type, Union

import numpy

from ..util import cwipc_pointcloud_wrapper

__all__ = ['AnalysisResults', 'AnalysisAlgorithm', 'OverlapAnalysisResults', 'AlignmentAlgorithm', 'MulticamAlgorithm',
           'MulticamAlignmentAlgorithm', 'RegistrationTransformation', 'Vector3']

#: a 4x4 float64 matrix; three floats
RegistrationTransformation = numpy.ndarray
Vector3 = Any


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


class AlignmentAlgorithm(ABC):
    """An algorithm that looks for the best alignment of one tile: a new matrix for that tile only (reference abstract.py:226-247).
    The fine aligners of registration/fine.py have this surface; they are used through it, not derived from it."""
    verbose: bool

    @abstractmethod
    def set_source_pointcloud(self, pc: cwipc_pointcloud_wrapper, tilemask: Optional[int] = None) -> None: ...

    @abstractmethod
    def set_reference_pointcloud(self, pc: cwipc_pointcloud_wrapper, tilemask: Optional[int] = None) -> None: ...

    @abstractmethod
    def set_correspondence(self, correspondence: float) -> None:
        """The largest distance between two points that may be "the same" point."""

    @abstractmethod
    def run(self) -> bool: ...

    @abstractmethod
    def get_result_transformation(self) -> RegistrationTransformation:
        """After run(): the transformation applied to the tile under test."""

    @abstractmethod
    def get_result_pointcloud(self) -> cwipc_pointcloud_wrapper:
        """After run(): the tile under test, moved."""

    @abstractmethod
    def get_result_pointcloud_full(self) -> cwipc_pointcloud_wrapper:
        """After run(): all tiles together, the moved one among them."""


class MulticamAlgorithm(ABC):
    """Anything that works on a tiled cloud, one tile per camera (reference abstract.py:251-288): the cloud, the mapping between a
    camera's index in the results and its tile number in the cloud, and run()."""
    verbose: bool

    @abstractmethod
    def set_tiled_pointcloud(self, pc: cwipc_pointcloud_wrapper) -> None:
        """The cloud whose tiles are the cameras."""

    @abstractmethod
    def camera_count(self) -> int: ...

    @abstractmethod
    def tilemask_for_camera_index(self, cam_index: int) -> int:
        """The tile number (in the cloud) of this index (in the results)."""

    @abstractmethod
    def camera_index_for_tilemask(self, tilenum: int) -> int:
        """... and back."""

    @abstractmethod
    def run(self) -> bool:
        """False: it failed."""


class MulticamAlignmentAlgorithm(MulticamAlgorithm):
    """An algorithm that aligns all tiles (reference abstract.py:293-326): which analyzer and which aligner it uses, and its results."""

    def __init__(self) -> None:
        self.analyzer_class: Optional[Type[Any]] = None
        self.aligner_class: Optional[Type[Any]] = None

    def set_analyzer_class(self, analyzer_class: Type[Any]) -> None:
        self.analyzer_class = analyzer_class

    def set_aligner_class(self, aligner_class: Type[Any]) -> None:
        self.aligner_class = aligner_class

    def set_max_correspondence(self, max_correspondence: float) -> None:
        """Overrides the distance within which matching points are looked for."""
        assert False, f"{self.__class__.__name__} does not implement set_max_correspondence()"

    def set_original_transform(self, cam_index: int, matrix: RegistrationTransformation) -> None:
        """The matrix a camera has before the run."""
        assert False, f"{self.__class__.__name__} does not implement set_original_transform()"

    @abstractmethod
    def get_result_transformations(self) -> List[RegistrationTransformation]:
        """After run(): one transformation per tile."""

    @abstractmethod
    def get_result_pointcloud_full(self) -> cwipc_pointcloud_wrapper:
        """After run(): all tiles together, moved."""
