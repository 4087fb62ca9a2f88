"""simulatecams filter (reference python/cwipc/filters/simulatecams.py:9-80)."""
from typing import Optional

import numpy

from .abstract import _TimedFilter
from ..util import cwipc_hip_simulatecams, cwipc_hip_simulatecams_soft, cwipc_pointcloud_wrapper


class SimulatecamsFilter(_TimedFilter):
    """
    simulatecams - Turn point cloud into multiple tiles by simulating cameras.
        Arguments:
            ncam: The number of cameras, spaced equidistantly on a circle around x=z=0.
            hard: If False or not specified, each point is assigned to the camera with the highest dot product
                  or the second highest dot product, with a probability proportional to the dot products.
                  If True, each point is assigned to the camera with the highest dot product.
            skew: If hard=False a skew > 1 will skew the distribution to the closest camera.
            seed: If hard=False, the seed of the draws (an extension: the reference takes numpy's global generator). Frame f of this
                  filter uses seed + f. Default: a fresh one per frame.
    """
    filtername = "simulatecams"

    def __init__(self, ncamera: int, hard: Optional[bool] = False, skew: Optional[float] = 1.0, seed: Optional[int] = None):
        super().__init__()
        self.ncamera = ncamera
        self.camera_vectors = numpy.zeros((ncamera, 3), dtype=float)
        for i in range(ncamera):
            angle = 2 * numpy.pi * i / ncamera
            self.camera_vectors[i, 0] = numpy.cos(angle)
            self.camera_vectors[i, 2] = numpy.sin(angle)
        self.hard = hard
        self.skew = skew
        self.seed = seed

    def filter(self, pc: cwipc_pointcloud_wrapper) -> cwipc_pointcloud_wrapper:
        if not self.hard and self.ncamera < 2:
            # (the reference raises IndexError here: there is no second camera to draw against)
            raise ValueError("simulatecams: hard=False needs at least two cameras")
        return self._run(pc, self._assign)

    def _assign(self, pc: cwipc_pointcloud_wrapper) -> cwipc_pointcloud_wrapper:
        # the centroid exactly as the reference forms it (:42-45): numpy's float32 mean over the rows of the N x 7 matrix
        point_matrix = pc.get_numpy_matrix()
        centroid = numpy.mean(point_matrix[:, :3], axis=0)
        centroid[1] = 0.0
        if self.hard:
            # the per-point loop (:47-58, :70) is one kernel: tile = 1 << camera with the largest dot product
            return cwipc_hip_simulatecams(pc, self.camera_vectors, centroid)
        # hard = False (:60-69) is a kernel too: the same rule on the library's seeded draws -- the same distribution, not the random
        # stream of the reference's numpy.random calls.  (self.count is already this frame's number + 1.)
        seed = None if self.seed is None else self.seed + self.count - 1
        return cwipc_hip_simulatecams_soft(pc, self.camera_vectors, centroid, self.skew, seed=seed)


CustomFilter = SimulatecamsFilter
