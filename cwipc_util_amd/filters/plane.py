"""plane filter: find the dominant plane of the cloud and remove it, keep it or put it first (no reference counterpart;
include/cwipc_util_amd/hip_ext.h, RULE S)."""
from .abstract import _TimedFilter
from ..util import cwipc_find_plane, cwipc_plane_filter, cwipc_pointcloud_wrapper


class PlaneFilter(_TimedFilter):
    """
    plane - Find the plane with the most points close to it (random-sample consensus) and remove its points.
        Arguments:
            distance: how far from the plane a point still belongs to it (float, the cloud's units)
            keep: 'rest' removes the plane's points (default), 'inliers' keeps only them, 'both' puts them first
            iterations: how many random triples are tried (default: 1024)
            seed: the seed of the draws (default: 0); the same seed and cloud give the same result
    """
    filtername = "plane"

    def __init__(self, distance: float, keep: str = "rest", iterations: int = 1024, seed: int = 0):
        super().__init__()
        self.distance = distance
        self.keep = keep
        self.iterations = iterations
        self.seed = seed
        self.last_plane = None

    def _plane(self, pc: cwipc_pointcloud_wrapper) -> cwipc_pointcloud_wrapper:
        self.last_plane = cwipc_find_plane(pc, self.distance, self.iterations, self.seed)
        # no plane found: a plane so far away that no point is near it -- nothing is removed, nothing counts as the plane
        plane = self.last_plane.plane if self.last_plane.found else (0.0, 1.0, 0.0, 1e300)
        return cwipc_plane_filter(pc, plane, self.distance, keep=self.keep)

    def filter(self, pc: cwipc_pointcloud_wrapper) -> cwipc_pointcloud_wrapper:
        return self._run(pc, self._plane)


CustomFilter = PlaneFilter
