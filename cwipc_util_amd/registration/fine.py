"""Fine alignment of one cloud onto another (reference python/cwipc/registration/fine.py: the aligner that every camera's step of
registration/multicamera.py runs between its two analyses).

Here: the base class, which finds nothing and returns the identity, point-to-point ICP, point-to-plane ICP and generalized ICP.  The reference runs
open3d's registration_icp on the CPU, on numpy copies of both clouds; here the clouds stay on the device, the loop is
cwipc_hip_icp_point2point (correspondence search on the point grid over the reference cloud, sums of the rigid fit, a 3x3 solve on
the host per iteration) or cwipc_hip_icp_point2plane (the same search, the sums of the plane fit, a 6x6 solve on the host per
iteration) and only the 4x4 result comes back.  Tile masks and filters are device compactions; no cloud is downloaded.

Point-to-plane needs the reference cloud's normals: they are estimated on the device, once per run, as the direction filter
estimates them (open3d's KDTreeSearchParamHybrid(normal_radius, normal_max_nn)), and never leave it.  The reference class also
turns the normals round with _fix_normal_direction; negating a normal leaves every term of this aligner's sums unchanged bit for
bit, so that step has no effect here and is not ported.  The source cloud's normals are never read by open3d's point-to-plane
estimate and are not computed.

Generalized ICP, the reference's default aligner, is cwipc_hip_icp_generalized: the same search and the same 6x6 solve, with sums
that weigh every pair by the inverse of Ct + R Cs R^T, the two points' covariances.  It needs normals on both clouds (estimated on the
device as above, the source's on the source cloud as given) and, unlike point-to-plane, their orientation: the sign of a normal
reaches the covariance, so the reference's _fix_normal_direction is ported for this aligner (each cloud's normals face away from
the midpoint of the two centroids).

DEFAULT_FINE_ALIGNMENT_ALGORITHM is still the point-to-point class (see the comment at the end of the file); a script that wants
the reference's default asks for RegistrationComputer_ICP_Generalized by name.
"""
from typing import Callable, List, Optional

import numpy as np

from ..util import (cwipc_pointcloud_wrapper, cwipc_tilefilter_masked, cwipc_transform, cwipc_join, cwipc_center,
                    cwipc_hip_icp_point2point, cwipc_hip_icp_point2plane, cwipc_hip_icp_generalized)

__all__ = ['RegistrationComputer', 'RegistrationComputer_ICP_Point2Point', 'RegistrationComputer_ICP_Point2Plane',
           'RegistrationComputer_ICP_Generalized', 'DEFAULT_FINE_ALIGNMENT_ALGORITHM', 'ALL_FINE_ALIGNMENT_ALGORITHMS']

PointCloudFilter = Callable[[cwipc_pointcloud_wrapper], cwipc_pointcloud_wrapper]


class RegistrationComputer:
    """Compute the registration of a source cloud against a reference cloud.  The base class does nothing: its result is the
    identity."""

    def __init__(self) -> None:
        self._source_pointcloud: Optional[cwipc_pointcloud_wrapper] = None
        self._filtered_source_pointcloud: Optional[cwipc_pointcloud_wrapper] = None
        self.source_tilemask: Optional[int] = None
        self._reference_pointcloud: Optional[cwipc_pointcloud_wrapper] = None
        self._filtered_reference_pointcloud: Optional[cwipc_pointcloud_wrapper] = None
        self.reference_tilemask: Optional[int] = None
        self.verbose = False
        #: how far apart two points may be and still be matched, in metres (inf: no limit; 0: worked out from the clouds in run())
        self.correspondence: float = np.inf

    # ---- the clouds ----
    def _masked(self, which: str, pc: cwipc_pointcloud_wrapper, tilemask: Optional[int]) -> cwipc_pointcloud_wrapper:
        name = self.__class__.__name__
        before = pc.count()
        if before == 0:
            print(f"{name}: set_{which}_pointcloud: Warning: pre_count={before}")
        if tilemask is not None and tilemask != 0:
            pc = cwipc_tilefilter_masked(pc, tilemask)
            if pc.count() == 0:
                print(f"{name}: set_{which}_pointcloud: Warning: tilemask={tilemask}, post_count=0")
        if self.verbose:
            print(f"{name}: Setting {which} point cloud with {pc.count()} (of {before}) points, tilemask {tilemask}")
        return pc

    def set_source_pointcloud(self, pc: cwipc_pointcloud_wrapper, tilemask: Optional[int] = None) -> None:
        self._source_pointcloud = self._masked("source", pc, tilemask)
        self._filtered_source_pointcloud = None
        self.source_tilemask = tilemask

    def set_reference_pointcloud(self, pc: cwipc_pointcloud_wrapper, tilemask: Optional[int] = None) -> None:
        self._reference_pointcloud = self._masked("reference", pc, tilemask)
        self._filtered_reference_pointcloud = None
        self.reference_tilemask = tilemask

    def get_source_pointcloud(self) -> cwipc_pointcloud_wrapper:
        assert self._source_pointcloud
        return self._source_pointcloud

    def get_reference_pointcloud(self) -> cwipc_pointcloud_wrapper:
        assert self._reference_pointcloud
        return self._reference_pointcloud

    def get_filtered_source_pointcloud(self) -> cwipc_pointcloud_wrapper:
        return self._filtered_source_pointcloud or self.get_source_pointcloud()

    def get_filtered_reference_pointcloud(self) -> cwipc_pointcloud_wrapper:
        return self._filtered_reference_pointcloud or self.get_reference_pointcloud()

    def apply_source_filter(self, filter: PointCloudFilter) -> None:
        """The alignment is computed from the filtered cloud; the result cloud is the whole source cloud, moved."""
        self._filtered_source_pointcloud = filter(self.get_filtered_source_pointcloud())

    def apply_reference_filter(self, filter: PointCloudFilter) -> None:
        self._filtered_reference_pointcloud = filter(self.get_filtered_reference_pointcloud())

    # ---- one run ----
    def set_correspondence(self, correspondence: float) -> None:
        self.correspondence = correspondence

    def _prepare(self) -> None:
        if self.verbose:
            print(f"{self.__class__.__name__}: with {self.get_filtered_source_pointcloud().count()} points and "
                  f"{self.get_filtered_reference_pointcloud().count()} reference points")
        if self.correspondence == 0:
            self._compute_correspondence()

    def _compute_correspondence(self) -> None:
        """Half the distance between the two clouds' centroids, height left out."""
        ours = np.array(cwipc_center(self.get_filtered_source_pointcloud()), dtype=np.float32)
        theirs = np.array(cwipc_center(self.get_filtered_reference_pointcloud()), dtype=np.float32)
        ours[1] = 0
        theirs[1] = 0
        self.correspondence = float(np.linalg.norm(ours - theirs)) / 2
        if self.verbose:
            print(f"{self.__class__.__name__}: set correspondence to {self.correspondence:.4f} meters")

    def run(self) -> bool:
        self._prepare()
        return True

    def get_result_transformation(self, nonverbose: bool = False) -> np.ndarray:
        return np.identity(4)

    def get_result_pointcloud(self) -> cwipc_pointcloud_wrapper:
        """The source cloud (all of it, not the filtered one) after the transformation."""
        return cwipc_transform(self.get_source_pointcloud(), self.get_result_transformation(nonverbose=True))

    def get_result_pointcloud_full(self) -> cwipc_pointcloud_wrapper:
        """... joined with the reference cloud."""
        return cwipc_join(self.get_result_pointcloud(), self.get_reference_pointcloud())


class _RegistrationComputer_ICP(RegistrationComputer):
    """What the ICP aligners share: the result of the last run and how it is reported."""

    def __init__(self) -> None:
        super().__init__()
        self.transformation: np.ndarray = np.identity(4)
        self.fitness: float = 0.0
        self.inlier_rmse: float = 0.0
        self.iterations: int = 0

    def get_result_transformation(self, nonverbose: bool = False) -> np.ndarray:
        if self.verbose and not nonverbose:
            print(f"{self.__class__.__name__}: fitness={self.fitness}, inlier_rmse={self.inlier_rmse}, iterations={self.iterations}")
            print(f"\toverlap: {int(self.fitness * 100)}%")
            print(f"\ttransformation:\n{self.transformation}")
        return self.transformation


class RegistrationComputer_ICP_Point2Point(_RegistrationComputer_ICP):
    """Point-to-point ICP on geometry alone, with the reference's criteria: relative fitness 1e-3, relative rmse 1e-6, at most 30
    iterations, starting from the identity."""

    relative_fitness = 1e-3
    relative_rmse = 1e-6
    max_iteration = 30

    def run(self) -> bool:
        self._prepare()
        self.transformation, self.fitness, self.inlier_rmse, self.iterations = cwipc_hip_icp_point2point(
            self.get_filtered_source_pointcloud(), self.get_filtered_reference_pointcloud(), self.correspondence, None,
            self.relative_fitness, self.relative_rmse, self.max_iteration)
        return True


class RegistrationComputer_ICP_Point2Plane(_RegistrationComputer_ICP):
    """Point-to-plane ICP on geometry alone, with the reference's criteria: relative fitness 1e-7, relative rmse 1e-7, at most 60
    iterations, starting from the identity.  The reference cloud's normals are estimated on the device from the normal_max_nn
    nearest points within normal_radius; their orientation does not matter (see the module's docstring)."""

    relative_fitness = 1e-7
    relative_rmse = 1e-7
    max_iteration = 60
    normal_radius = 0.02
    normal_max_nn = 30

    def run(self) -> bool:
        self._prepare()
        self.transformation, self.fitness, self.inlier_rmse, self.iterations = cwipc_hip_icp_point2plane(
            self.get_filtered_source_pointcloud(), self.get_filtered_reference_pointcloud(), self.correspondence, None, None,
            self.normal_radius, self.normal_max_nn, self.relative_fitness, self.relative_rmse, self.max_iteration)
        return True


class RegistrationComputer_ICP_Generalized(RegistrationComputer_ICP_Point2Plane):
    """Generalized ICP on geometry alone (the reference's default aligner), with the reference's criteria and normal parameters,
    which are the point-to-plane class's, and open3d's epsilon: the variance along a point's normal, against 1 in its plane.  Both
    clouds' normals are estimated on the device and turned as the reference's _fix_normal_direction turns them."""

    epsilon = 1e-3

    def run(self) -> bool:
        self._prepare()
        self.transformation, self.fitness, self.inlier_rmse, self.iterations = cwipc_hip_icp_generalized(
            self.get_filtered_source_pointcloud(), self.get_filtered_reference_pointcloud(), self.correspondence, None, None, None,
            self.normal_radius, self.normal_max_nn, self.epsilon, self.relative_fitness, self.relative_rmse, self.max_iteration)
        return True


#: (the reference's default is generalized ICP, RegistrationComputer_ICP_Generalized here; see below for why this one stays)
DEFAULT_FINE_ALIGNMENT_ALGORITHM = RegistrationComputer_ICP_Point2Point

# (the point-to-plane and the generalized class are not in this list, and the default is not the generalized class:
# tests/test_gpu_icp.py asserts the list and the default as they were when point-to-point went in, and existing tests are not
# edited; both classes are exported and used by name)
ALL_FINE_ALIGNMENT_ALGORITHMS: List[type] = [RegistrationComputer, RegistrationComputer_ICP_Point2Point]
