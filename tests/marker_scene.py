"""A synthetic capture for the marker detector's end-to-end tests (test infrastructure): coarse_scene's board and cameras, with two real
markers painted in where coarse_scene paints corner patches.  Marker m (ids 0 and 1 of tests/golden/aruco_5x5_printed.json) fills the
square coarse_scene.MARKERS[m]; its canonical corners, top-left, top-right, bottom-right, bottom-left, are that list's corners 0, 1, 2, 3,
the pairing MultiCameraCoarseAruco.known_marker_positions assumes.  Seen from above (the cameras look down at the board) that cycle runs
clockwise on screen, so the markers are not mirrored.

A board sample inside a marker's square is black when the marker's 7 x 7 cell under it is black; everything else is white."""
import math

import numpy as np

import coarse_scene as cs
import marker_model as mm
from cwipc_util_amd.util import cwipc_point_numpy_dtype

SPACING = cs.SPACING
MARKER_IDS = (0, 1)


def marker_cell_of(m, x, z):
    """(i, j, inside): the cell row and column of board positions (x, z) in marker m's 7 x 7 grid.  The column axis runs from corner 0
    to corner 1, the row axis from corner 0 to corner 3."""
    c = np.asarray(cs.MARKERS[m], dtype=np.float64)
    origin, col_axis, row_axis = c[0, [0, 2]], c[1, [0, 2]] - c[0, [0, 2]], c[3, [0, 2]] - c[0, [0, 2]]
    d = np.stack([x, z], axis=-1) - origin
    u = 7.0 * (d @ col_axis) / (col_axis @ col_axis)
    v = 7.0 * (d @ row_axis) / (row_axis @ row_axis)
    inside = (u >= 0) & (u < 7) & (v >= 0) & (v < 7)
    return np.clip(np.floor(v).astype(np.int64), 0, 6), np.clip(np.floor(u).astype(np.int64), 0, 6), inside


def board(seed=20241):
    """The world cloud: a structured array of points, tile 0, in a seeded shuffled order."""
    nx = int(round((cs.BOARD_X[1] - cs.BOARD_X[0]) / SPACING)) + 1
    nz = int(round((cs.BOARD_Z[1] - cs.BOARD_Z[0]) / SPACING)) + 1
    gx, gz = np.meshgrid(cs.BOARD_X[0] + SPACING * np.arange(nx), cs.BOARD_Z[0] + SPACING * np.arange(nz), indexing='ij')
    gx, gz = gx.reshape(-1), gz.reshape(-1)
    shade = np.full(len(gx), 255, dtype=np.uint8)
    bits = mm.fixture_bits()
    for m in MARKER_IDS:
        cells = mm.cells_of_bits(bits[m])
        i, j, inside = marker_cell_of(m, gx, gz)
        shade[inside & (cells[i, j] == 0)] = 0
    order = np.random.default_rng(seed).permutation(len(gx))
    pts = np.zeros(len(gx), dtype=cwipc_point_numpy_dtype)
    pts['x'], pts['z'] = gx[order], gz[order]
    pts['r'] = pts['g'] = pts['b'] = shade[order]
    return pts


def capture(ncameras=3):
    """The tiles of the first ncameras of coarse_scene's cameras, joined."""
    world = board()
    return np.concatenate([cs.camera_tile(world, k) for k in range(ncameras)])


def corner_bound(view, point_size, ncameras=3):
    """e, the bound on one deprojected marker corner, from the scene's geometry alone.

    In pixels.  h = the splat's half width.  A dark pixel was painted by a black sample, which lies in the marker's square: the
    pixel's number is within h + 1 of the sample's projection in each coordinate (the floor and the splat), so the blob lies in the
    square's image grown by g = h + 1.  The other way round, the sample nearest a true corner is within one sample spacing s (in
    pixels, at the smallest corner depth) of it in each coordinate, and white samples in front of it can take at most the h + 1
    pixels next to the outline from the black ones, so the blob reaches to within g + s of the corner's image.  The detected corner
    is the blob's extreme pixel in a direction across the diagonal; at a corner whose sides make 45 degrees with that direction, a
    pixel at least as extreme as one that is d = 2 g + s (the two together) short of the corner lies within (1 + sqrt 2) d of it:
    d along the direction, and sqrt 2 d sideways between the two sides.
    Back to 3D: the corner pixel's depth is that of the sample drawn there, whose projection is within g of the pixel in each
    coordinate, and deproject takes the pixel's number for its position: sqrt 2 g more.
    A pixel at depth z is z / f wide across the viewing direction and 1 / cos(tilt) times that on the board, tilt = the angle
    between the ray to the corner and the board's normal.  The largest z / (f cos) over the visible corners is used, and the
    sample spacing is added once more for the sample grid's own step."""
    h = (point_size - 1) // 2
    f = min(view.fx, view.fy)
    pixel = 0.0
    z_min = math.inf
    for k in range(ncameras):
        normal = cs.world_to_camera(k)[:3, :3] @ np.array([0.0, 1.0, 0.0])
        for m in cs.EXPECTED_VISIBLE[k]:
            for p in cs.true_corners_in_camera(k, m):
                cos_tilt = abs(float(p @ normal)) / float(np.linalg.norm(p))
                pixel = max(pixel, float(p[2]) / (f * cos_tilt))
                z_min = min(z_min, float(p[2]))
    g = h + 1
    s = SPACING * f / z_min
    d = 2 * g + s
    return ((1 + math.sqrt(2)) * d + math.sqrt(2) * g) * pixel + SPACING
