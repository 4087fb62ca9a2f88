"""Helpers of the registration tooling (reference python/cwipc/registration/util.py): 4x4 transformations as numpy matrices
(:29-82) and BaseMulticamAlgorithm, the tiled cloud and the camera numbering every multi-camera algorithm shares (:397-449).  The
per-point helpers of that module run on the GPU and live in cwipc_util_amd.util; they are re-exported here under the names the
reference's callers import from this module."""
import math
from typing import List, Optional, Tuple

import numpy as np

from ..util import (cwipc_pointcloud_wrapper, cwipc_tilefilter, cwipc_tilefilter_masked, cwipc_transform, get_tiles_used,   # noqa: F401
                    cwipc_downsample_pertile, cwipc_direction_filter, cwipc_center, cwipc_floor_filter, cwipc_randomize_floor,
                    cwipc_compute_tile_occupancy, cwipc_compute_radius, cwipc_limit_floor_to_radius, cwipc_join, cwipc_join_multi)
from .abstract import MulticamAlgorithm, RegistrationTransformation, Vector3

__all__ = ['transformation_identity', 'transformation_invert', 'transformation_frompython', 'transformation_topython',
           'transformation_get_translation', 'transformation_compare', 'BaseMulticamAlgorithm',
           'cwipc_tilefilter_masked', 'cwipc_transform', 'get_tiles_used', 'cwipc_downsample_pertile', 'cwipc_direction_filter', 'cwipc_center',
           'cwipc_floor_filter', 'cwipc_randomize_floor', 'cwipc_compute_tile_occupancy', 'cwipc_compute_radius', 'cwipc_limit_floor_to_radius']


def transformation_identity() -> RegistrationTransformation:
    return np.identity(4, dtype=float)


def transformation_invert(orig_transform: RegistrationTransformation) -> RegistrationTransformation:
    """The inverse of a RIGID transformation: the rotation transposed (it preserves lengths), the translation turned back by it."""
    inv_matrix = orig_transform[:3, :3].T
    transform = np.empty((4, 4))
    transform[:3, :3] = inv_matrix
    transform[:3, 3] = -inv_matrix @ orig_transform[:3, 3]
    transform[3, :] = [0, 0, 0, 1]
    return transform


def transformation_frompython(trafo: List[List[float]]) -> RegistrationTransformation:
    rv = np.array(trafo)
    assert rv.shape == (4, 4)
    return rv


def transformation_topython(matrix: RegistrationTransformation) -> List[List[float]]:
    rv = matrix.tolist()
    assert len(rv) == 4 and len(rv[0]) == 4
    return rv


def transformation_get_translation(matrix: RegistrationTransformation) -> Vector3:
    return matrix[0:3, 3]


def _rotation_vector_degrees(rot: np.ndarray) -> np.ndarray:
    """Axis times angle (degrees) of a 3x3 rotation matrix, by way of its unit quaternion (the reference asks scipy's
    Rotation.as_rotvec(degrees=True); scipy is not needed here): q = (w, v), angle = 2 atan2(|v|, w), axis = v / |v|."""
    m = np.asarray(rot, dtype=float)
    # the largest of w^2, x^2, y^2, z^2 picks the branch: no division by a small number
    diag = np.array([m[0, 0] + m[1, 1] + m[2, 2], m[0, 0], m[1, 1], m[2, 2]])
    k = int(np.argmax(diag))
    if k == 0:
        q = np.array([1.0 + diag[0], m[2, 1] - m[1, 2], m[0, 2] - m[2, 0], m[1, 0] - m[0, 1]])
    else:
        i = k - 1
        j, l = (i + 1) % 3, (i + 2) % 3
        q = np.empty(4)
        q[0] = m[l, j] - m[j, l]
        q[1 + i] = 1.0 + m[i, i] - m[j, j] - m[l, l]
        q[1 + j] = m[j, i] + m[i, j]
        q[1 + l] = m[l, i] + m[i, l]
    q = q / np.linalg.norm(q)
    if q[0] < 0:
        q = -q
    vnorm = float(np.linalg.norm(q[1:]))
    if vnorm == 0.0:
        return np.zeros(3)
    angle = 2.0 * math.atan2(vnorm, float(q[0]))
    return q[1:] / vnorm * math.degrees(angle)


def transformation_compare(old: Optional[RegistrationTransformation], new: Optional[RegistrationTransformation]) -> Tuple[Vector3, Vector3]:
    """What leads from old to new (None: the identity): its translation and its rotation as a rotation vector in degrees."""
    if old is None:
        old = transformation_identity()
    if new is None:
        new = transformation_identity()
    diff = new @ np.linalg.inv(old)
    return diff[:3, 3].copy(), _rotation_vector_degrees(diff[:3, :3])


class BaseMulticamAlgorithm(MulticamAlgorithm):
    """The tiled cloud and the camera numbering: camera i is the i-th tile number that occurs in the cloud, ascending."""

    def __init__(self) -> None:
        self.per_camera_tilenum: List[int] = []
        self.original_pointcloud: Optional[cwipc_pointcloud_wrapper] = None
        self.verbose = False

    def set_tiled_pointcloud(self, pc: cwipc_pointcloud_wrapper) -> None:
        self.original_pointcloud = pc
        for tilemask in get_tiles_used(pc):
            self.per_camera_tilenum.append(tilemask)

    def tilemask_for_camera_index(self, cam_index: int) -> int:
        return self.per_camera_tilenum[cam_index]

    def camera_index_for_tilemask(self, tilenum: int) -> int:
        for i, t in enumerate(self.per_camera_tilenum):
            if t == tilenum:
                return i
        assert False, f"Tilenum {tilenum} not known"

    def camera_count(self) -> int:
        return len(self.per_camera_tilenum)

    def get_pc_for_tilemask(self, tilemask: int) -> cwipc_pointcloud_wrapper:
        """The points of one tile number."""
        assert self.original_pointcloud
        pc = cwipc_tilefilter(self.original_pointcloud, tilemask)
        if not pc:
            raise ValueError(f"Tilemask {tilemask} has no point cloud")
        return pc

    def get_pc_for_camnum(self, camnum: int) -> cwipc_pointcloud_wrapper:
        return self.get_pc_for_tilemask(self.tilemask_for_camera_index(camnum))
