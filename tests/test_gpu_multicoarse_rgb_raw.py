"""Coarse registration from RAW camera images, end to end: the scene of tests/test_gpu_multicoarse_rgb.py, but every camera has a
separate colour sensor 32 mm to the side of its depth sensor, behind the mild Brown lens.  A camera's depth image is its tile rendered
from the origin (Z16 millimetres); its colour image is the tile rendered from the colour sensor's place and then bent by the lens
(every pixel of the bent image takes the nearest pixel of the pinhole image at its undistorted position).  The frames go through an
RgbdRigSource, which registers the colour onto the depth grid, and its cloud, images attached, goes into MultiCameraCoarseArucoRgb
unchanged, with the scene's stand-in detector."""
import math

import numpy as np
import pytest

import coarse_scene as cs
import rgbd_lens_model as lm
from conftest import make_cloud
from test_gpu_multicoarse_rgb import DEPTH_SCALE, POINT_SIZE, board_plane, to_z16, worst_residual
from cwipc_util_amd.registration import MultiCameraCoarseArucoRgb, default_view, render_pointcloud
from cwipc_util_amd.rgbd import RgbdRigSource, RgbdSensor

pytestmark = pytest.mark.gpu

MILD_BROWN = (-0.1, 0.05, 1e-3, -5e-4, 0.0, 0.0, 0.0, 0.0)
BASELINE = 0.032
NCAMERAS = 3


def depth_to_colour():
    m = np.identity(4)
    m[0, 3] = -BASELINE        # the colour sensor sits 32 mm along the depth camera's +x
    return m


def lens_stretch(view):
    """How far apart, in pinhole pixels, two points can be that are one pixel apart in the bent image: the largest 1 / |eigenvalue|
    of distort's (symmetric) Jacobian over the image, on the model's analytic terms at a grid of undistorted positions that covers it."""
    xs = np.linspace(-view.cx / view.fx, (view.width - 1 - view.cx) / view.fx, 65) * 1.1
    ys = np.linspace(-view.cy / view.fy, (view.height - 1 - view.cy) / view.fy, 37) * 1.1
    x, y = np.meshgrid(xs, ys)
    j00, j01, _j10, j11, _det = lm._jacobian(MILD_BROWN, lm._radial(MILD_BROWN, x, y), x, y)
    mean, half = (j00 + j11) / 2, np.sqrt(((j00 - j11) / 2) ** 2 + j01 ** 2)
    smallest = np.minimum(np.abs(mean - half), np.abs(mean + half))
    assert (smallest > 0.5).all()
    return float((1.0 / smallest).max())


def corner_bound_raw(view, point_size, ncameras=NCAMERAS):
    """e'', the bound on one corner as MultiCameraCoarseArucoRgb measures it on a raw rig's images, from the scene's geometry alone.
    All pixel distances are per axis; h = (point_size - 1) / 2 is a splat's half width; "position" is a point's exact projection.

    Which depth pixels get a corner's colour.  Depth pixel p has the depth of a board sample S' whose position lies within h + 1 of p
    (the splat, and a position within 1 pixel of its own pixel).  Its point P is on p's ray at that depth (rounded to the millimetre).
    Both sensors have the view's intrinsics and the colour sensor is b to the side, so a point with depth-image position a and depth
    z has the pinhole colour position a + (f b / z, 0).  P's pinhole colour position is bent by the lens, rounded to the nearest
    pixel q of the bent image (0.5 in each axis of the bent image: at most 0.5 sqrt(2) * stretch in the pinhole image,
    lens_stretch()), q's colour is that of the pinhole pixel nearest its undistorted position (0.5), and that pixel shows a sample
    S whose position lies within h + 1 of it.  So P's and S's pinhole colour positions differ by at most
        R = (h + 1) + 0.5 + 0.5 sqrt(2) stretch,
    and their depth-image positions by at most X = R + f b |1/z(S) - 1/z(P)| <= R + kappa |z(S) - z(P)|, kappa = f b / z_lo^2 with
    z_lo the board's smallest depth.  z(P) is z(S') to 0.5 mm; S and S' are on the board, their positions at most X + h + 1 apart,
    and the board's depth changes by at most g per pixel, g = (z_hi^2 / |c|)(|n_x| / fx + |n_y| / fy) (the plane n . p = c,
    tests/test_gpu_multicoarse_rgb.py: corner_bound_rgb).  X <= R + kappa (g (X + h + 1) + 0.0005) gives
        X <= (R + kappa (g (h + 1) + 0.0005)) / (1 - kappa g).
    Every depth pixel with the corner's colour lies within X of the position of a sample of the corner's patch.

    The corner pixel (u, v) is the rounded centroid of those pixels: within X + 0.5 of the convex hull of the patch samples'
    positions, X + 1 with the half pixel between a pixel's number and its position.  Its own depth z0 is that of a sample S'' whose
    position lies within h + 1 of (u, v), so the point of (u, v) at z0 is within sqrt(2) (h + 1) z_hi / f + 0.0005 rho of S''
    (rho: corner_bound_rgb's bound on a ray's length per unit depth), and S'' is a board point whose position is within
    m = (X + 1) + (h + 1) of that of a point H of the hull, which lies on the board within PATCH_RADIUS of the corner (SPACING more,
    as in coarse_scene.corner_bound, for the patch being samples).  Two board points whose positions are m apart in each axis are at
    most sqrt(2) m (z_hi / f) sec apart, sec = 1 / min |n . r| over the image's unit rays r: the plane's foreshortening.
        e_raw = PATCH_RADIUS + SPACING + sqrt(2) m (z_hi / f) sec + sqrt(2) (h + 1) z_hi / f + 0.0005 rho
    and e'' = e_raw + rho (0.0015 + (3 + 2 (h + 1)) g) for the mean depth of the 7 x 7 window in place of z0, as corner_bound_rgb
    derives it (its window argument holds for the attached depth image: inside the colour image it is the depth image)."""
    h = (point_size - 1) // 2
    f = min(view.fx, view.fy)
    rho = math.sqrt(1.0 + (view.width / (2.0 * view.fx)) ** 2 + (view.height / (2.0 * view.fy)) ** 2)
    g = z_hi = sec = 0.0
    z_lo = math.inf
    us, vs = np.meshgrid(np.linspace(0, view.width - 1, 33), np.linspace(0, view.height - 1, 19))
    rays = np.stack([(us - view.cx) / view.fx, (vs - view.cy) / view.fy, np.ones_like(us)], axis=-1)
    rays /= np.linalg.norm(rays, axis=-1, keepdims=True)
    for k in range(ncameras):
        n, c, hi = board_plane(k)
        m = cs.world_to_camera(k)
        ends = np.array([[x, 0.0, z] for x in cs.BOARD_X for z in cs.BOARD_Z]) @ m[:3, :3].T + m[:3, 3]
        z_lo, z_hi = min(z_lo, float(ends[:, 2].min())), max(z_hi, hi)
        g = max(g, (hi ** 2 / abs(c)) * (abs(n[0]) / view.fx + abs(n[1]) / view.fy))
        sec = max(sec, float(1.0 / np.abs(rays @ n).min()))
    assert z_lo > 0
    kappa = max(view.fx, view.fy) * BASELINE / z_lo ** 2
    assert kappa * g < 0.5
    reach = (h + 1) + 0.5 + 0.5 * math.sqrt(2.0) * lens_stretch(view)
    x = (reach + kappa * (g * (h + 1) + 0.0005)) / (1.0 - kappa * g)
    m_px = (x + 1) + (h + 1)
    e_raw = cs.PATCH_RADIUS + cs.SPACING + math.sqrt(2.0) * m_px * (z_hi / f) * sec + math.sqrt(2.0) * (h + 1) * z_hi / f + 0.0005 * rho
    return e_raw + rho * (0.0015 + (3 + 2 * (h + 1)) * g)


def bend(view, pinhole_rgb, undistorted):
    """The colour image behind the lens: bent pixel (uc, vc) shows the pinhole image's nearest pixel at its undistorted position,
    white where that is outside."""
    x, y = undistorted
    u = np.floor(view.fx * x + view.cx + 0.5)
    v = np.floor(view.fy * y + view.cy + 0.5)
    inside = (u >= 0) & (u < view.width) & (v >= 0) & (v < view.height)
    out = np.full_like(pinhole_rgb, 255)
    out[inside] = pinhole_rgb[v[inside].astype(np.int64), u[inside].astype(np.int64)]
    return out


@pytest.fixture(scope="module")
def raw_frames(gpu):
    """Per camera its (depth Z16 from the depth sensor's place, colour RGB8 from the colour sensor's place, bent)."""
    world = cs.board()
    view = default_view()
    side = default_view(extrinsic=depth_to_colour())
    vc, uc = np.meshgrid(np.arange(view.height), np.arange(view.width), indexing='ij')
    undistorted = lm.undistort(MILD_BROWN, (uc - view.cx) / view.fx, (vc - view.cy) / view.fy)
    assert not np.isnan(undistorted[0]).any()
    out = []
    for k in range(NCAMERAS):
        tile = make_cloud(gpu, cs.camera_tile(world, k))
        _rgb, depth, _index = render_pointcloud(tile, view, POINT_SIZE)
        rgb_side, _depth, _index = render_pointcloud(tile, side, POINT_SIZE)
        out.append((to_z16(depth), bend(view, rgb_side, undistorted)))
    return out


def test_three_raw_cameras_register(gpu, raw_frames):
    view = default_view()
    sensors = [RgbdSensor(view.width, view.height, view.fx, view.fy, view.cx, view.cy, view.width, view.height, view.fx, view.fy, view.cx, view.cy,
                          colour_coeffs=MILD_BROWN, depth_to_colour=depth_to_colour(), depth_scale=DEPTH_SCALE, tile=1 << k, serial="serial%d" % k)
               for k in range(NCAMERAS)]
    src = RgbdRigSource(sensors, [raw_frames])
    src.request_metadata("rgb")
    src.request_metadata("depth")
    pc = src.get()
    assert gpu.get_tiles_used(pc) == [1, 2, 4] and pc.access_metadata().count() == 6
    # the registered image is not the bent one: where they differ most, a corner's colour sits on another pixel
    images = pc.access_metadata().get_all_images("serial1")
    assert images["rgb."].shape == (view.height, view.width, 3) and not np.array_equal(images["rgb."][:, :, ::-1], raw_frames[1][1])
    algo = MultiCameraCoarseArucoRgb()
    algo.set_marker_detector(cs.make_detector(POINT_SIZE))
    algo.set_grabber(src)
    algo.set_tiled_pointcloud(pc)
    assert algo.serial_for_tilenum == {1: "serial0", 2: "serial1", 4: "serial2"}
    assert algo.run() is True                                          # all cameras register
    assert [set(m) for m in algo.markers] == cs.EXPECTED_VISIBLE[:NCAMERAS]
    assert all(len(area) == 4 for markers in algo.markers for area in markers.values())
    assert algo._get_unregistered_tiles() == [] and sorted(algo.known_marker_positions) == [0, 1]
    e = corner_bound_raw(view, POINT_SIZE)
    worst_corner = max(float(np.linalg.norm(np.asarray(algo.markers[k][m]) - cs.true_corners_in_camera(k, m), axis=1).max())
                       for k in range(NCAMERAS) for m in cs.EXPECTED_VISIBLE[k])
    worst = worst_residual(algo, NCAMERAS)
    print("worst corner %.2f mm, e'' = %.2f mm; worst residual %.2f mm, 3 e'' = %.2f mm" % (worst_corner * 1000, e * 1000, worst * 1000, 3 * e * 1000))
    assert cs.corner_bound(view, POINT_SIZE) < e < 0.070
    assert worst_corner <= e
    assert worst <= 3 * e
    src.free()
