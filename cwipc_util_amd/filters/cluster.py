"""cluster filter: keep the big Euclidean clusters (no reference counterpart; include/cwipc_util_amd/hip_ext.h, RULE K)."""
from .abstract import _TimedFilter
from ..util import cwipc_cluster_filter, cwipc_pointcloud_wrapper


class ClusterFilter(_TimedFilter):
    """
    cluster - Cut the cloud into connected components at a radius and keep the big ones.
        Arguments:
            radius: two points closer than this are in one cluster (float)
            min_points: clusters with fewer points are dropped (default: 1, keep all)
            max_clusters: keep only this many of the largest clusters (default: 0, no limit)
            same_tile: If true only points of the same tile are linked (default: false)
    """
    filtername = "cluster"

    def __init__(self, radius: float, min_points: int = 1, max_clusters: int = 0, same_tile: bool = False):
        super().__init__()
        self.radius = radius
        self.min_points = min_points
        self.max_clusters = max_clusters
        self.same_tile = same_tile

    def filter(self, pc: cwipc_pointcloud_wrapper) -> cwipc_pointcloud_wrapper:
        return self._run(pc, lambda p: cwipc_cluster_filter(p, self.radius, self.min_points, self.max_clusters, self.same_tile))


CustomFilter = ClusterFilter
