"""randomize_floor filter (reference python/cwipc/filters/randomize_floor.py:7-55)."""
import time
from typing import Optional

from .abstract import _TimedFilter
from ..util import cwipc_pointcloud_wrapper, cwipc_randomize_floor


class RandomizeFloorFilter(_TimedFilter):
    """
    randomize_floor - Find all points that are considered to represent the floor. Randomize the tile of each of these points.
        Argument:
            level: The Y value for floor threshold. Default 0.1.
            seed: seed of the permutation (an extension: the reference takes numpy's global generator). Default: a fresh one per frame.
        This filter may be useful when aligning point clouds that have large sections of floor visible, but
        different sections of floor for each camera.
    """
    filtername = "randomize_floor"

    def __init__(self, level: float = 0.1, seed: Optional[int] = None):
        super().__init__()
        self.level = level
        self.seed = seed

    def filter(self, pc: cwipc_pointcloud_wrapper) -> cwipc_pointcloud_wrapper:
        self.count += 1
        t1 = time.time()
        newpc = cwipc_randomize_floor(pc, self.level, seed=self.seed)
        self.times.append(time.time() - t1)
        return newpc

    def statistics(self) -> None:
        print(f"{self.filtername}: count={self.count}")
        if self.times:
            self.print1stat('duration', self.times)


CustomFilter = RandomizeFloorFilter
