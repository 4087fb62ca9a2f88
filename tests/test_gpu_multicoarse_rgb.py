"""Coarse registration from the cameras' own images, end to end (registration/multicoarse.py: MultiCameraCoarseArucoRgb): the scene of
tests/coarse_scene.py; each camera's tile rendered from the origin is that camera's colour and depth image, the depth quantised to Z16
millimetres; the frames go through an RgbdSource whose matrices are the identity, and its cloud, images attached, goes into the
algorithm with the scene's stand-in detector.  One test runs on the CPU: it shows on the renderer's numpy model that the scene, not
luck, gives every marker corner its depth."""
import math

import numpy as np
import pytest

import coarse_scene as cs
import render_model
from conftest import make_cloud
from cwipc_util_amd.registration import MultiCameraCoarseAruco, MultiCameraCoarseArucoRgb, default_view, render_pointcloud, mean_depth
from cwipc_util_amd.rgbd import RgbdCamera, RgbdSource

POINT_SIZE = 5
WINDOW = 3          # mean_depth's 7 x 7
MINIMUM = 10
DEPTH_SCALE = 0.001


def to_z16(depth):
    """A rendered depth image (float32 metres, 0: nothing) as Z16 millimetres, rounded to the nearest."""
    return np.floor(depth.astype(np.float64) * 1000.0 + 0.5).astype(np.uint16)


def board_plane(k):
    """The board's plane in camera k's coordinates, n . p = c, and the largest camera depth of any board point."""
    m = cs.world_to_camera(k)
    n = m[:3, :3] @ np.array([0.0, 1.0, 0.0])
    c = float(n @ m[:3, 3])
    ends = np.array([[x, 0.0, z] for x in cs.BOARD_X for z in cs.BOARD_Z]) @ m[:3, :3].T + m[:3, 3]
    assert (ends[:, 2] > 0).all()      # the whole board is in front of the camera: depth, linear on it, is largest at one of its ends
    return n, c, float(ends[:, 2].max())


def corner_bound_rgb(view, point_size, ncameras=3):
    """e', the bound on one corner as MultiCameraCoarseArucoRgb measures it, from the scene's geometry alone.

    e = coarse_scene.corner_bound bounds |P(u, v, z0) - corner|: the corner pixel (u, v) taken to 3D with its own depth z0 =
    depth[v, u], which is what MultiCameraCoarseAruco does.  Here the same pixel is taken to 3D with another depth, zm: the floored
    integer mean of the Z16 values in the 7 x 7 window, times 0.001.  P(u, v, z) = z * ((u - cx) / fx, (v - cy) / fy, 1), so the two
    points lie on the pixel's ray and |P(zm) - P(z0)| = |zm - z0| * rho(u, v), rho <= sqrt(1 + (W / 2 fx)^2 + (H / 2 fy)^2) anywhere
    in the image.  |zm - z0| has three parts:
      * every Z16 value is its depth rounded to the nearest millimetre: 0.5 mm; the mean of the values is as near the mean of the
        depths;
      * the integer mean is floored: less than 1 mm (the float32 rounding of the matrix product, 1e-7 m, is left out);
      * the mean of the window's depths against z0.  Every depth in the image is the board's depth at some point whose own pixel lies
        within h = (point_size - 1) / 2 pixels of the pixel that shows it, and a point's image position within 1 pixel of its own
        pixel; so the window's depths are board depths at image positions within 3 + h + 1 pixels of (u, v) along either axis, z0 is
        one within h + 1, and any two of them are at most 3 + 2 (h + 1) pixels apart along either axis.  On the plane n . p = c the
        depth at image position (a, b) is z = c / (n_x (a - cx) / fx + n_y (b - cy) / fy + n_z), so dz/da = -(z^2 / c) n_x / fx and
        dz/db alike: over the board, where z <= z_hi (its largest depth in that view), depths that far apart differ by at most
        (3 + 2 (h + 1)) (z_hi^2 / |c|) (|n_x| / fx + |n_y| / fy).  The mean differs from z0 by no more than its farthest member.
    e' = e + rho * (0.0015 + the slope term), the worst camera's.  26 mm here, of which 17.5 mm are e."""
    h = (point_size - 1) // 2
    rho = math.sqrt(1.0 + (view.width / (2.0 * view.fx)) ** 2 + (view.height / (2.0 * view.fy)) ** 2)
    slope = 0.0
    for k in range(ncameras):
        n, c, z_hi = board_plane(k)
        slope = max(slope, (3 + 2 * (h + 1)) * (z_hi ** 2 / abs(c)) * (abs(n[0]) / view.fx + abs(n[1]) / view.fy))
    return cs.corner_bound(view, point_size, ncameras) + rho * (0.0015 + slope)


def valid_in_window(depth16, u, v):
    return int((depth16[max(v - WINDOW, 0): v + WINDOW + 1, max(u - WINDOW, 0): u + WINDOW + 1] != 0).sum())


def test_every_corner_window_has_depth_in_the_model():
    """On the CPU, from tests/render_model.py (whose images the GPU's equal byte for byte, tests/test_gpu_render.py): every corner
    the stand-in detector reports for a visible marker has at least 10 valid depths in its 7 x 7 window -- all 49, the board being
    dense -- and mean_depth on the Z16 image is positive there."""
    world = cs.board()
    view = default_view()
    detect = cs.make_detector(POINT_SIZE)
    for k in range(3):
        rgb, depth, _index, _covered = render_model.render_model(cs.camera_tile(world, k), view, POINT_SIZE)
        depth16 = to_z16(depth)
        areas, ids = detect(rgb)
        assert set(ids) == cs.EXPECTED_VISIBLE[k]
        for area in areas:
            for u, v in area:
                assert valid_in_window(depth16, int(u), int(v)) == 49 >= MINIMUM
                assert mean_depth(depth16, int(u), int(v), WINDOW, MINIMUM) > 0


@pytest.fixture(scope="module")
def frames(gpu):
    """Per camera (all four) its (depth Z16, colour RGB8) images: its tile rendered from the origin."""
    world = cs.board()
    view = default_view()
    out = []
    for k in range(4):
        rgb, depth, _index = render_pointcloud(make_cloud(gpu, cs.camera_tile(world, k)), view, POINT_SIZE)
        out.append((to_z16(depth), np.ascontiguousarray(rgb)))
    return out


def source_for(frame, metadata=True):
    view = default_view()
    cams = [RgbdCamera(view.width, view.height, view.fx, view.fy, view.cx, view.cy, DEPTH_SCALE, np.identity(4), 1 << k, "serial%d" % k)
            for k in range(len(frame))]
    src = RgbdSource(cams, [frame])
    if metadata:
        src.request_metadata("rgb")
        src.request_metadata("depth")
    return src


def algorithm(src, pc, detector=None):
    algo = MultiCameraCoarseArucoRgb()
    algo.set_marker_detector(detector if detector is not None else cs.make_detector(POINT_SIZE))
    algo.set_grabber(src)
    algo.set_tiled_pointcloud(pc)
    return algo


def worst_residual(algo, ncameras):
    worst = 0.0
    for k in range(ncameras):
        T = algo.get_result_transformations()[algo.camera_index_for_tilemask(1 << k)]
        for m in cs.EXPECTED_VISIBLE[k]:
            moved = cs.true_corners_in_camera(k, m) @ T[:3, :3].T + T[:3, 3]
            worst = max(worst, float(np.linalg.norm(moved - np.asarray(cs.MARKERS[m]), axis=1).max()))
    return worst


@pytest.mark.gpu
def test_four_cameras_from_their_images(gpu, frames):
    """Cameras A and B register through marker 0, camera C through marker 1, which camera B taught; camera D sees no marker.  The
    residual bound is test_three_cameras's argument (tests/test_gpu_multicoarse.py: a fitted matrix moves a true corner at most 3 e
    from its place) with e' of corner_bound_rgb in place of e."""
    src = source_for(frames)
    pc = src.get()
    assert gpu.get_tiles_used(pc) == [1, 2, 4, 8] and pc.access_metadata().count() == 8
    algo = algorithm(src, pc)
    assert algo.serial_for_tilenum == {1: "serial0", 2: "serial1", 4: "serial2", 8: "serial3"}
    assert algo.run() is False
    assert [set(m) for m in algo.markers] == cs.EXPECTED_VISIBLE
    assert all(len(area) == 4 for markers in algo.markers for area in markers.values())
    got = algo.get_result_transformations()
    assert algo._get_unregistered_tiles() == [3] and np.array_equal(got[3], np.identity(4))
    assert sorted(algo.known_marker_positions) == [0, 1]          # marker 1 was learnt
    assert not np.array_equal(got[2], np.identity(4))               # ... and camera C, which never sees marker 0, is registered
    view = default_view()
    e = corner_bound_rgb(view, POINT_SIZE)
    assert cs.corner_bound(view, POINT_SIZE) < e < 0.030
    worst_corner = max(float(np.linalg.norm(np.asarray(algo.markers[k][m]) - cs.true_corners_in_camera(k, m), axis=1).max())
                       for k in range(3) for m in cs.EXPECTED_VISIBLE[k])
    worst = worst_residual(algo, 3)
    print("worst corner %.2f mm, e' = %.2f mm; worst residual %.2f mm, 3 e' = %.2f mm" % (worst_corner * 1000, e * 1000, worst * 1000, 3 * e * 1000))
    assert worst_corner <= e
    assert np.linalg.norm(np.asarray(algo.known_marker_positions[1]) - np.asarray(cs.MARKERS[1]), axis=1).max() <= 4 * e
    assert worst <= 3 * e


@pytest.mark.gpu
def test_corner_without_depth_skips_its_marker(gpu, frames):
    """A hole round corner 2 of marker 1 in camera B's depth image leaves fewer than 10 depths in its window: the corner list ends
    there, run() skips the marker, nobody learns marker 1 -- cameras A and B still register through marker 0, camera C cannot."""
    depth_b, rgb_b = frames[1]
    areas, ids = cs.make_detector(POINT_SIZE)(rgb_b)
    u, v = (int(c) for c in areas[ids.index(1)][2])
    holed = depth_b.copy()
    holed[v - WINDOW: v + WINDOW + 1, u - WINDOW: u + WINDOW + 1] = 0
    holed[v - WINDOW, u - WINDOW: u + WINDOW + 1] = depth_b[v - WINDOW, u - WINDOW: u + WINDOW + 1]          # 7 valid depths stay ...
    holed[v + WINDOW, u - WINDOW: u - WINDOW + 2] = depth_b[v + WINDOW, u - WINDOW: u - WINDOW + 2]          # ... and 2 more: 9
    assert valid_in_window(holed, u, v) == MINIMUM - 1
    src = source_for([frames[0], (holed, rgb_b), frames[2]])
    pc = src.get()
    algo = algorithm(src, pc)
    assert algo.run() is False
    assert len(algo.markers[1][1]) == 2 and len(algo.markers[1][0]) == 4 and len(algo.markers[2][1]) == 4
    assert algo._get_unregistered_tiles() == [2] and sorted(algo.known_marker_positions) == [0]
    assert worst_residual(algo, 2) <= 3 * corner_bound_rgb(default_view(), POINT_SIZE)


@pytest.mark.gpu
def test_duplicate_id_keeps_the_nearer_marker(gpu, frames):
    """A detector that calls both of camera B's markers 0: the one whose first corner is nearer the camera stays, in either order."""
    real = cs.make_detector(POINT_SIZE)
    nearer = min((0, 1), key=lambda m: float(np.linalg.norm(cs.true_corners_in_camera(1, m)[0])))
    gap = abs(float(np.linalg.norm(cs.true_corners_in_camera(1, 0)[0])) - float(np.linalg.norm(cs.true_corners_in_camera(1, 1)[0])))
    assert gap > 2 * corner_bound_rgb(default_view(), POINT_SIZE)     # (the measured distances order as the true ones)
    src = source_for(frames[:3])
    pc = src.get()
    for flip in (False, True):
        def twice(rgb):
            areas, ids = real(rgb)
            if len(ids) < 2:
                return areas, ids
            return (areas[::-1] if flip else areas), [0, 0]
        algo = algorithm(src, pc, twice)
        algo._prepare()
        found = algo._find_markers(0, 1)
        assert list(found) == [0] and len(found[0]) == 4
        err = np.linalg.norm(np.asarray(found[0]) - cs.true_corners_in_camera(1, nearer), axis=1).max()
        assert err <= corner_bound_rgb(default_view(), POINT_SIZE)


@pytest.mark.gpu
def test_cloud_without_metadata_takes_the_rendered_path(gpu, frames):
    """No images on the cloud: every camera falls back to MultiCameraCoarseAruco's rendering and the result is that class's, exactly."""
    world = cs.board()
    pc = make_cloud(gpu, np.concatenate([cs.camera_tile(world, k) for k in range(3)]))
    assert pc.access_metadata().count() == 0
    src = source_for(frames[:3], metadata=False)
    algo = algorithm(src, pc)
    assert algo.run() is True
    parent = MultiCameraCoarseAruco()
    parent.set_marker_detector(cs.make_detector(POINT_SIZE))
    parent.set_tiled_pointcloud(pc)
    assert parent.run() is True
    assert algo.markers == parent.markers and algo.known_marker_positions == parent.known_marker_positions
    for a, b in zip(algo.get_result_transformations(), parent.get_result_transformations()):
        assert np.array_equal(a, b)
