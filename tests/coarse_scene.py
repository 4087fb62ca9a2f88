"""A synthetic capture for the coarse registration tests (test infrastructure): a white board in the plane y = 0 with two markers whose
corners are painted in colours of their own, seen by cameras that look down at it, and a stand-in marker detector that finds those
colours in a rendered image.

The world: the board is 1.6 m x 0.8 m, sampled every 2 mm in x and z (801 x 401 points, in an order shuffled by a seeded generator).
Marker 0 has its corners where MultiCameraCoarseAruco knows them, marker 1 has the same shape 0.9 m further along x.  The board
points within 6 mm of a marker corner have the colour CORNER_COLOURS[marker][corner].

Camera k's tile (tile number 1 << k) is the whole world cloud in that camera's coordinates: its world -> camera matrix applied in
float64, stored as float32.  A camera's tile seen from the origin (the identity view) is what the physical camera saw."""
import math

import numpy as np

from cwipc_util_amd.registration.render import look_at
from cwipc_util_amd.util import cwipc_point_numpy_dtype

SPACING = 0.002
PATCH_RADIUS = 0.006
BOARD_X = (-0.35, 1.25)
BOARD_Z = (-0.4, 0.4)
MARKER_OFFSET = 0.9

MARKERS = {
    0: [(+0.087, 0.0, +0.087), (-0.087, 0.0, +0.087), (-0.087, 0.0, -0.087), (+0.087, 0.0, -0.087)],
}
MARKERS[1] = [(x + MARKER_OFFSET, y, z) for x, y, z in MARKERS[0]]

#: no two alike, none white (the board and the renderer's default background)
CORNER_COLOURS = {
    0: [(230, 20, 20), (20, 20, 230), (230, 20, 230), (230, 230, 20)],
    1: [(20, 160, 60), (20, 220, 220), (120, 60, 20), (90, 20, 160)],
}

#: (eye, target, up); the image's vertical axis, the short one, runs along the board's long side
CAMERAS = [
    ((-0.45, 1.30, 0.15), (-0.30, 0.0, 0.00), (1.0, 0.0, 0.0)),     # A: marker 0 only
    ((0.40, 1.45, -0.10), (0.45, 0.0, 0.02), (1.0, 0.0, 0.1)),      # B: both markers
    ((1.30, 1.25, 0.05), (1.20, 0.0, -0.03), (-1.0, 0.0, 0.2)),     # C: marker 1 only
    ((-0.90, 1.20, 0.00), (-1.00, 0.0, 0.05), (1.0, 0.0, 0.0)),     # D: the board's bare end, no marker
]
#: which markers each camera sees (asserted by the tests from the geometry, not taken on trust)
EXPECTED_VISIBLE = [{0}, {0, 1}, {1}, set()]


def world_to_camera(k):
    eye, target, up = CAMERAS[k]
    return look_at(eye, target, up)


def board(seed=20240):
    """The world cloud: a structured array of points, tile 0."""
    nx = int(round((BOARD_X[1] - BOARD_X[0]) / SPACING)) + 1
    nz = int(round((BOARD_Z[1] - BOARD_Z[0]) / SPACING)) + 1
    x = BOARD_X[0] + SPACING * np.arange(nx)
    z = BOARD_Z[0] + SPACING * np.arange(nz)
    gx, gz = np.meshgrid(x, z, indexing='ij')
    gx, gz = gx.reshape(-1), gz.reshape(-1)
    colour = np.full((len(gx), 3), 255, dtype=np.uint8)
    for m, corners in MARKERS.items():
        for c, (cx, _cy, cz) in enumerate(corners):
            near = (gx - cx) ** 2 + (gz - cz) ** 2 <= PATCH_RADIUS ** 2
            colour[near] = CORNER_COLOURS[m][c]
    order = np.random.default_rng(seed).permutation(len(gx))
    pts = np.zeros(len(gx), dtype=cwipc_point_numpy_dtype)
    pts['x'], pts['z'] = gx[order], gz[order]
    pts['r'], pts['g'], pts['b'] = colour[order, 0], colour[order, 1], colour[order, 2]
    return pts


def camera_tile(world_pts, k):
    """The world cloud in camera k's coordinates, tile number 1 << k."""
    m = world_to_camera(k)
    p = np.stack([world_pts[f].astype(np.float64) for f in ('x', 'y', 'z')], axis=1) @ m[:3, :3].T + m[:3, 3]
    tile = world_pts.copy()
    tile['x'], tile['y'], tile['z'] = p[:, 0], p[:, 1], p[:, 2]
    tile['tile'] = 1 << k
    return tile


def capture(ncameras=3):
    """The tiles of the first ncameras cameras, joined."""
    world = board()
    return np.concatenate([camera_tile(world, k) for k in range(ncameras)])


def true_corners_in_camera(k, marker):
    """The marker's corners in camera k's coordinates (4 x 3, float64)."""
    m = world_to_camera(k)
    return np.asarray(MARKERS[marker], dtype=np.float64) @ m[:3, :3].T + m[:3, 3]


def project(view, cam_points):
    """(u, v) of camera-space points in an identity view."""
    p = np.asarray(cam_points, dtype=np.float64)
    return np.stack([view.fx * (p[:, 0] / p[:, 2]) + view.cx, view.fy * (p[:, 1] / p[:, 2]) + view.cy], axis=1)


def visibility(view, k, marker, margin=20.0):
    """'in': all four corners are inside the image by more than margin pixels; 'out': all four are outside by more than that (no pixel
    of a corner's patch, a few pixels wide, can be in the image); None: neither, the pose is no good for these tests."""
    cam = true_corners_in_camera(k, marker)
    if (cam[:, 2] <= view.near).any():
        return None
    uv = project(view, cam)
    inside = (uv[:, 0] > margin) & (uv[:, 0] < view.width - 1 - margin) & (uv[:, 1] > margin) & (uv[:, 1] < view.height - 1 - margin)
    outside = (uv[:, 0] < -margin) | (uv[:, 0] > view.width - 1 + margin) | (uv[:, 1] < -margin) | (uv[:, 1] > view.height - 1 + margin)
    if inside.all():
        return 'in'
    if outside.all():
        return 'out'
    return None


def corner_bound(view, point_size, ncameras=3):
    """e, the bound on one deprojected corner, from the scene's geometry alone: the patch radius (the centroid of a corner's pixels
    lies within the patch's image, grown by the splats), 2 (h + 1) pixels at the largest corner depth (the rounded centroid pixel, the
    splat's half width h on either side of a patch's outline, and the half pixel _deproject leaves out when it takes a pixel's number
    for its position), and the sample spacing (the patch is made of samples, not of the disc)."""
    h = (point_size - 1) // 2
    z_max = max(true_corners_in_camera(k, m)[:, 2].max() for k in range(ncameras) for m in EXPECTED_VISIBLE[k])
    f = min(view.fx, view.fy)
    return PATCH_RADIUS + 2 * (h + 1) * z_max / f + SPACING


def make_detector(point_size):
    """The stand-in detector: for every (marker, corner) colour that at least point_size^2 pixels have exactly, the corner is the
    rounded centroid of those pixels; a marker is reported when all four of its corners were found."""
    def detect(rgb):
        areas, ids = [], []
        packed = (rgb[:, :, 0].astype(np.uint32) << 16) | (rgb[:, :, 1].astype(np.uint32) << 8) | rgb[:, :, 2].astype(np.uint32)
        for m in sorted(CORNER_COLOURS):
            corners = []
            for r, g, b in CORNER_COLOURS[m]:
                rows, cols = np.nonzero(packed == ((r << 16) | (g << 8) | b))
                if len(rows) < point_size ** 2:
                    break
                corners.append((float(math.floor(cols.mean() + 0.5)), float(math.floor(rows.mean() + 0.5))))
            if len(corners) == 4:
                areas.append(corners)
                ids.append(m)
        return areas, ids
    return detect
