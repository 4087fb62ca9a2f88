"""direction filter (reference python/cwipc/filters/direction.py:6-64)."""
from .abstract import _TimedFilter
from ..util import cwipc_direction_filter, cwipc_pointcloud_wrapper


class DirectionFilter(_TimedFilter):
    """
    direction - Filter point cloud to points that are approximately oriented in a certain direction.
        Arguments:
            x, y, z: Direction vector
            threshold: float between -1.0 and 1.0. 1.0 is fully aligned with direction, -1.0 is opposite. Default 0.0.
        For each point a normal is computed, based on a surface with adjacent points.
        The dot product between these normals and the direction vector is computed, and any point
        that does not satisfy the threshold is discarded.
        The direction vector is relative to the center of the point cloud.
    """
    filtername = "direction"

    def __init__(self, x: float, y: float, z: float, threshold: float = 0.0):
        super().__init__()
        self.direction = (x, y, z)
        self.threshold = threshold

    def filter(self, pc: cwipc_pointcloud_wrapper) -> cwipc_pointcloud_wrapper:
        return self._run(pc, lambda p: cwipc_direction_filter(p, self.direction, self.threshold))

    def statistics(self) -> None:
        print(f"direction: count={self.count}")
        super().statistics()


CustomFilter = DirectionFilter
