"""transform44 filter (reference python/cwipc/filters/transform44.py:7-54)."""
from typing import List

from .abstract import _TimedFilter
from ..util import cwipc_transform, cwipc_pointcloud_wrapper
from ..registration.util import transformation_frompython


class Transform44Filter(_TimedFilter):
    """
    transform - Adjust coordinate system of the point clouds.
        Arguments:
            matrix: 4x4 transformation matrix as a list of lists.
    """
    filtername = "transform"

    def __init__(self, matrix: List[List[float]]):
        super().__init__()
        self.transform = transformation_frompython(matrix)

    def filter(self, pc: cwipc_pointcloud_wrapper) -> cwipc_pointcloud_wrapper:
        return self._run(pc, lambda p: cwipc_transform(p, self.transform))

    def statistics(self) -> None:
        print(f"transform44: count={self.count}")
        if self.times:
            self.print1stat('duration', self.times)


CustomFilter = Transform44Filter
