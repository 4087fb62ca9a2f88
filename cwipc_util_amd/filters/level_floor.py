"""level_floor filter: find the floor of a cloud that is not level yet and move the cloud so that the floor is y = 0 (no reference
counterpart; include/cwipc_util_amd/hip_ext.h, RULE S; cwipc_util_amd/registration/floor.py)."""
from .abstract import _TimedFilter
from ..util import cwipc_pointcloud_wrapper, cwipc_transform


class LevelFloorFilter(_TimedFilter):
    """
    level_floor - Find the floor (the largest plane within max_angle of horizontal) and rotate and shift the cloud so that it lies at y = 0.
        Arguments:
            distance: how far from the floor plane a point still belongs to it (float, the cloud's units)
            max_angle: how far the floor's normal may be from the Y axis, in degrees (default: 15)
            iterations: how many random triples are tried (default: 4096)
            seed: the seed of the draws (default: 0)
            remove: If true the floor and everything under it is removed (default: false)
        A cloud in which no floor is found passes unchanged.
    """
    filtername = "level_floor"

    def __init__(self, distance: float, max_angle: float = 15.0, iterations: int = 4096, seed: int = 0, remove: bool = False):
        super().__init__()
        self.distance = distance
        self.max_angle = max_angle
        self.iterations = iterations
        self.seed = seed
        self.remove = remove
        self.last_plane = None
        self.last_matrix = None

    def _level(self, pc: cwipc_pointcloud_wrapper) -> cwipc_pointcloud_wrapper:
        from ..registration.floor import level_to_floor
        levelled, self.last_matrix, self.last_plane = level_to_floor(pc, self.distance, self.max_angle, self.iterations, self.seed, remove=self.remove)
        if levelled is None:
            return cwipc_transform(pc, [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
        return levelled

    def filter(self, pc: cwipc_pointcloud_wrapper) -> cwipc_pointcloud_wrapper:
        return self._run(pc, self._level)


CustomFilter = LevelFloorFilter
