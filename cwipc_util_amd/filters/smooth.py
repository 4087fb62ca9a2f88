"""smooth filter: move every point onto the plane fitted to its neighbourhood (no reference counterpart;
include/cwipc_util_amd/hip_ext.h, RULE N)."""
from .abstract import _TimedFilter
from ..util import cwipc_smooth, cwipc_pointcloud_wrapper


class SmoothFilter(_TimedFilter):
    """
    smooth - Flatten depth noise: each point is moved onto the plane fitted to the points inside a radius around it.
        Arguments:
            radius: the neighbourhood's radius (float, the cloud's units)
            min_neighbours: points with fewer neighbours stay where they are (default: 2, which is also the least possible)
            iterations: how many times the smoothing is applied (default: 1)
            same_tile: If true only points of the same tile are neighbours (default: false)
    """
    filtername = "smooth"

    def __init__(self, radius: float, min_neighbours: int = 2, iterations: int = 1, same_tile: bool = False):
        super().__init__()
        self.radius = radius
        self.min_neighbours = min_neighbours
        self.iterations = iterations
        self.same_tile = same_tile

    def _smooth(self, pc: cwipc_pointcloud_wrapper) -> cwipc_pointcloud_wrapper:
        # each further pass takes the pass before it, still on the device, as its input
        out = cwipc_smooth(pc, self.radius, self.min_neighbours, self.same_tile)
        for _ in range(1, max(int(self.iterations), 1)):
            nxt = cwipc_smooth(out, self.radius, self.min_neighbours, self.same_tile)
            out.free()
            out = nxt
        return out

    def filter(self, pc: cwipc_pointcloud_wrapper) -> cwipc_pointcloud_wrapper:
        return self._run(pc, self._smooth)


CustomFilter = SmoothFilter
