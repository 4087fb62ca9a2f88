"""The floor of a cloud that no marker has levelled yet (no reference counterpart; include/cwipc_util_amd/hip_ext.h, RULE S).

The reference's floor helpers (cwipc_floor_filter, cwipc_randomize_floor, cwipc_compute_radius, cwipc_limit_floor_to_radius,
MultiCameraToFloor) define the floor as y < level, which holds only after a marker alignment has put the floor at y = 0.  find_floor
looks for the dominant plane whose normal lies within max_angle of `up` on the GPU; level_to_floor moves the cloud so that this plane
becomes y = 0 with everything else above it, after which those helpers apply.  The cloud stays on the device.
"""
from typing import Any, Optional, Tuple

import numpy

from ..util import (cwipc_pointcloud_wrapper, cwipc_plane_result, cwipc_find_plane, cwipc_hip_plane_level_matrix, cwipc_transform,
                    cwipc_plane_filter)

DEFAULT_FLOOR_DISTANCE = 0.02
DEFAULT_FLOOR_MAX_ANGLE = 15.0
DEFAULT_FLOOR_ITERATIONS = 4096


def find_floor(pc: cwipc_pointcloud_wrapper, distance: float = DEFAULT_FLOOR_DISTANCE, max_angle: float = DEFAULT_FLOOR_MAX_ANGLE,
               iterations: int = DEFAULT_FLOOR_ITERATIONS, seed: int = 0, up: Any = (0.0, 1.0, 0.0)) -> cwipc_plane_result:
    """The plane with the most points within `distance` among those whose normal is within max_angle degrees of `up`; its normal
    points to the side of `up`.  result.found is False when the cloud has no such plane."""
    return cwipc_find_plane(pc, distance, iterations, seed, axis=up, max_angle=max_angle, refine=True)


def level_to_floor(pc: cwipc_pointcloud_wrapper, distance: float = DEFAULT_FLOOR_DISTANCE, max_angle: float = DEFAULT_FLOOR_MAX_ANGLE,
                   iterations: int = DEFAULT_FLOOR_ITERATIONS, seed: int = 0, up: Any = (0.0, 1.0, 0.0),
                   remove: bool = False) -> Tuple[Optional[cwipc_pointcloud_wrapper], Optional[numpy.ndarray], cwipc_plane_result]:
    """(levelled cloud, 4x4 matrix, plane): the cloud moved so that its floor is y = 0 and `up` is +Y as nearly as the floor allows;
    remove: without the floor and what lies under it.  (None, None, plane) when no floor was found."""
    plane = find_floor(pc, distance, max_angle, iterations, seed, up)
    if not plane.found:
        return None, None, plane
    matrix = cwipc_hip_plane_level_matrix(plane.plane)
    if remove:
        above = cwipc_plane_filter(pc, plane.plane, distance, keep="rest", below=True)
        levelled = cwipc_transform(above, matrix)
        above.free()
    else:
        levelled = cwipc_transform(pc, matrix)
    return levelled, matrix, plane
