"""A cloud seen through a pinhole camera, without a window: what the reference's coarse registration gets from an open3d Visualizer
(python/cwipc/registration/multicoarse.py:333-360 views a camera's tile from (0, 0, 0) and grabs the colour and depth buffers)
comes here from one GPU call, cwipc_hip_render, exactly defined and reproducible (include/cwipc_util_amd/hip_ext.h).  Everything
else in this module is host arithmetic on a handful of numbers.

Conventions, those of the reference's `_deproject` (multicoarse.py:426-428): the camera looks along +z, image x runs right and
image y runs down; pixel (u, v) at depth z is the camera-space point ((u - cx) * z / fx, (v - cy) * z / fy, z).  A view's extrinsic
matrix takes cloud ("world") coordinates to camera coordinates."""
import math
from dataclasses import dataclass, field
from typing import Any, Optional, Sequence, Tuple

import numpy as np

from ..util import cwipc_pointcloud_wrapper, cwipc_hip_view, cwipc_hip_render
from .util import transformation_identity, transformation_invert

__all__ = ['PinholeView', 'default_view', 'look_at', 'render_pointcloud', 'deproject', 'deproject_depth', 'mean_depth']


@dataclass
class PinholeView:
    """Image size, intrinsics, world -> camera matrix (4x4, float64) and the depth range of a view."""
    width: int
    height: int
    fx: float
    fy: float
    cx: float
    cy: float
    extrinsic: np.ndarray = field(default_factory=transformation_identity)
    near: float = 0.01
    far: float = math.inf

    def as_struct(self) -> cwipc_hip_view:
        """The view as the C structure cwipc_hip_render takes."""
        e = np.ascontiguousarray(np.asarray(self.extrinsic, dtype=np.float64))
        if e.shape != (4, 4):
            raise ValueError("PinholeView: extrinsic must be a 4x4 matrix")
        rv = cwipc_hip_view()
        rv.width, rv.height = int(self.width), int(self.height)
        rv.fx, rv.fy, rv.cx, rv.cy = float(self.fx), float(self.fy), float(self.cx), float(self.cy)
        rv.near, rv.far = float(self.near), float(self.far)
        rv.extrinsic[:] = e.reshape(16).tolist()
        return rv


def default_view(width: int = 1920, height: int = 1080, fov_deg: float = 60.0, extrinsic: Optional[np.ndarray] = None) -> PinholeView:
    """A view with a vertical field of view of fov_deg, the principal point in the middle of the image and, unless one is given, the
    identity for its extrinsic matrix: the camera at the origin of the cloud's coordinates -- the reference's `from000` view, which for a
    tile that is still in its camera's own coordinates is the physical camera's view."""
    f = (height / 2.0) / math.tan(math.radians(fov_deg) / 2.0)
    e = transformation_identity() if extrinsic is None else np.array(extrinsic, dtype=np.float64)
    return PinholeView(width, height, f, f, (width - 1) / 2.0, (height - 1) / 2.0, e)


def look_at(eye: Sequence[float], target: Sequence[float], up: Sequence[float]) -> np.ndarray:
    """The world -> camera matrix of a camera at `eye` that looks at `target`: `eye` goes to the origin, `target` onto the +z axis, and
    `up` points towards the top of the image (camera -y, because image y runs down).  A proper rotation and a translation."""
    eye_v = np.asarray(eye, dtype=np.float64)
    forward = np.asarray(target, dtype=np.float64) - eye_v
    norm = np.linalg.norm(forward)
    if not norm > 0:
        raise ValueError("look_at: eye and target coincide")
    forward = forward / norm
    right = np.cross(forward, np.asarray(up, dtype=np.float64))   # x = y cross z with y = -up: the image's right-hand side
    norm = np.linalg.norm(right)
    if not norm > 0:
        raise ValueError("look_at: up is parallel to the viewing direction")
    right = right / norm
    down = np.cross(forward, right)
    rv = transformation_identity()
    rv[0, :3], rv[1, :3], rv[2, :3] = right, down, forward
    rv[:3, 3] = -(rv[:3, :3] @ eye_v)
    return rv


def render_pointcloud(pc: cwipc_pointcloud_wrapper, view: PinholeView, point_size: int = 5, tilemask: int = 0,
                      background: Sequence[int] = (255, 255, 255)) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(rgb uint8[H, W, 3], depth float32[H, W], index int32[H, W]) of the cloud in this view, rendered on the GPU."""
    return cwipc_hip_render(pc, view.as_struct(), point_size, tilemask, background)


def deproject(view: PinholeView, depth: np.ndarray, uv: Sequence[float]) -> Optional[Tuple[float, float, float]]:
    """The cloud-space point of an image position, through the depth image: the per-corner arithmetic of the reference's `_deproject`
    (multicoarse.py:403-444).  u and v are truncated to a pixel, d is that pixel's depth, the camera-space point is ((u - cx) * d / fx,
    (v - cy) * d / fy, d) and the inverse of the view's extrinsic matrix takes it back.  None for a pixel outside the image or
    without depth (the reference would index outside the image or deproject the background to the camera's origin)."""
    u, v = int(uv[0]), int(uv[1])
    height, width = depth.shape
    if u < 0 or u >= width or v < 0 or v >= height:
        return None
    d = float(depth[v, u])
    if d == 0:
        return None
    z = d
    x = (u - view.cx) * z / view.fx
    y = (v - view.cy) * z / view.fy
    transform = transformation_invert(np.asarray(view.extrinsic, dtype=np.float64))
    p = transform @ np.array([x, y, z, 1.0])
    return float(p[0]), float(p[1]), float(p[2])


def deproject_depth(view: PinholeView, u: int, v: int, d: float) -> Optional[Tuple[float, float, float]]:
    """`deproject`'s arithmetic for a pixel (u, v) whose depth d is known already (cwipc_hip_render_detect_markers hands the corners'
    depths over without the image): None for depth 0, the background."""
    d = float(d)
    if d == 0:
        return None
    z = d
    x = (u - view.cx) * z / view.fx
    y = (v - view.cy) * z / view.fy
    transform = transformation_invert(np.asarray(view.extrinsic, dtype=np.float64))
    p = transform @ np.array([x, y, z, 1.0])
    return float(p[0]), float(p[1]), float(p[2])


def mean_depth(depth: np.ndarray, x: int, y: int, offset: int = 3, minimum: int = 10) -> Any:
    """The depth at (x, y) as the mean of the depths that are there in the (2 offset + 1)^2 pixels around it, 0 when fewer than
    `minimum` of them have one: the reference's `_get_depth_value` (multicoarse.py:614-633), for depth images with holes.  Pixels
    outside the image and pixels with depth 0 do not count.  An integer image gives the floored mean of the integers, as in the
    reference (a capturer's depth is in millimetres); a float image gives the mean as a float."""
    integral = np.issubdtype(depth.dtype, np.integer)
    depth_sum: Any = 0 if integral else 0.0
    depth_count = 0
    for _x in range(x - offset, x + offset + 1):
        if _x < 0 or _x >= depth.shape[1]:
            continue
        for _y in range(y - offset, y + offset + 1):
            if _y < 0 or _y >= depth.shape[0]:
                continue
            d = int(depth[_y, _x]) if integral else float(depth[_y, _x])
            if d == 0:
                continue
            depth_sum += d
            depth_count += 1
    if depth_count < minimum:
        return 0
    return depth_sum // depth_count if integral else depth_sum / depth_count
