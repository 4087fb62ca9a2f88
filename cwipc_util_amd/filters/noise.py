"""noise filter (reference python/cwipc/filters/noise.py:9-70)."""
from typing import Optional

from .abstract import _TimedFilter
from ..util import cwipc_hip_noise, cwipc_pointcloud_wrapper


class NoiseFilter(_TimedFilter):
    """
    noise - Add noise to the point coordinates.
        Arguments:
            distance: Each point will be moved along a random vector with length up to this distance.
            seed: seed of the random vectors (an extension: the reference takes numpy's global generator). Frame f of this
                  filter uses seed + f. Default: a fresh one per frame.
    """
    filtername = "noise"

    def __init__(self, distance: float, seed: Optional[int] = None):
        super().__init__()
        self.distance = distance
        self.seed = seed

    def filter(self, pc: cwipc_pointcloud_wrapper) -> cwipc_pointcloud_wrapper:
        # (a stream of frames must not repeat one noise field: the frame number goes into the seed)
        seed = None if self.seed is None else self.seed + self.count
        return self._run(pc, lambda p: cwipc_hip_noise(p, self.distance, seed))


CustomFilter = NoiseFilter
