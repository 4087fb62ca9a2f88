"""radius_outliers filter: drop the points with too few neighbours inside a radius (no reference counterpart;
include/cwipc_util_amd/hip_ext.h, RULE N)."""
from .abstract import _TimedFilter
from ..util import cwipc_radius_outlier_filter, cwipc_pointcloud_wrapper


class RadiusOutliersFilter(_TimedFilter):
    """
    radius_outliers - Count each point's neighbours inside a radius and drop the lonely points.
        Arguments:
            radius: a neighbour is another point closer than this (float, the cloud's units)
            min_neighbours: points with fewer neighbours are dropped (default: 1)
            same_tile: If true only points of the same tile count as neighbours (default: false)
    """
    filtername = "radius_outliers"

    def __init__(self, radius: float, min_neighbours: int = 1, same_tile: bool = False):
        super().__init__()
        self.radius = radius
        self.min_neighbours = min_neighbours
        self.same_tile = same_tile

    def filter(self, pc: cwipc_pointcloud_wrapper) -> cwipc_pointcloud_wrapper:
        return self._run(pc, lambda p: cwipc_radius_outlier_filter(p, self.radius, self.min_neighbours, self.same_tile))


CustomFilter = RadiusOutliersFilter
