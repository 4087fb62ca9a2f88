"""The occlusion test end to end on a scene that needs no model to judge: a red board 0.4 m in front of a green wall, both facing a
sensor pair whose colour sensor sits 32 mm beside the depth sensor, behind the mild Brown lens of tests/test_gpu_multicoarse_rgb_raw.py
and with twice the depth sensor's resolution.  Both images are cast, not sampled: a depth pixel has the depth of what the ray through
its centre hits, a colour pixel the colour of what the ray through its undistorted centre hits from the colour sensor's place.

Left of the board the depth sensor sees a strip of wall that the board hides from the colour sensor.  Without the occlusion test the
points of that strip are red; with it they are gone, every board point is kept, and no wall point is lost outside the strip's bound,
which shadow_band() derives from the geometry.  The model alone is held to the same on the CPU first."""
import math

import numpy as np
import pytest

import coarse_scene as cs
import rgbd_lens_model as lm
import rgbd_occlusion_model as om
from test_gpu_multicoarse_rgb_raw import BASELINE, MILD_BROWN, depth_to_colour, lens_stretch
from cwipc_util_amd.registration import default_view
from cwipc_util_amd.rgbd import RgbdOcclusion, RgbdRig, RgbdSensor

Z_BOARD, Z_WALL = 0.6, 1.0
BOARD_X, BOARD_Y = (-0.15, 0.17), (-0.11, 0.12)      # the board's extent in the depth camera's coordinates, metres
RED, GREEN = (220, 30, 30), (30, 200, 40)
STEEPEST = 1.0                                       # the slope (metres of depth per metre across) the margin is to keep: 45 degrees
NOISE = 0.002                                        # ... on top of the depth's own resolution and noise, metres


def views():
    depth = default_view(320, 240)
    return depth, default_view(640, 480, extrinsic=depth_to_colour())


def rule_of_thumb(depth_view, colour_view, z_far):
    """DESIGN 3.19.  splat: ceil(max(colour_fx / fx, colour_fy / fy)) - 1 closes the gaps between a surface's samples in the finer
    colour grid; one more closes the last fraction of a depth pixel along a silhouette, where the foreground's outermost sample lies up
    to one depth pixel, that ratio in colour pixels, inside its outline.  margin: a sample's neighbours within the splat and the two
    roundings, (splat + 1) colour pixels or (splat + 1) z / f metres across, are nearer by the slope times that."""
    ratio = max(colour_view.fx / depth_view.fx, colour_view.fy / depth_view.fy)
    splat = math.ceil(ratio)
    margin = STEEPEST * (splat + 1) * z_far / min(colour_view.fx, colour_view.fy) + NOISE
    return RgbdOcclusion(splat, margin)


def scene():
    """(sensor, model, frame) -- CPU only."""
    dv, cv = views()
    d2c = depth_to_colour()
    sensor = RgbdSensor(dv.width, dv.height, dv.fx, dv.fy, dv.cx, dv.cy, cv.width, cv.height, cv.fx, cv.fy, cv.cx, cv.cy, colour_coeffs=MILD_BROWN,
                        depth_to_colour=d2c, tile=1, serial="scene")
    model = lm.Sensor(dv.width, dv.height, dv.fx, dv.fy, dv.cx, dv.cy, lm.PINHOLE, 0.001, (cv.width, cv.height), 3, (cv.fx, cv.fy, cv.cx, cv.cy), MILD_BROWN,
                      d2c, np.identity(4), 1)
    # the depth image: the ray through pixel (u, v)'s centre meets the board's plane at ((u - cx) / fx, (v - cy) / fy) * Z_BOARD
    v, u = np.meshgrid(np.arange(dv.height), np.arange(dv.width), indexing='ij')
    x, y = (u - dv.cx) / dv.fx * Z_BOARD, (v - dv.cy) / dv.fy * Z_BOARD
    on_board = (x >= BOARD_X[0]) & (x <= BOARD_X[1]) & (y >= BOARD_Y[0]) & (y <= BOARD_Y[1])
    depth = np.where(on_board, round(Z_BOARD * 1000), round(Z_WALL * 1000)).astype(np.uint16)
    # the colour image: the colour sensor sits at (BASELINE, 0, 0); the ray of a pixel of the bent image is its undistorted position
    vc, uc = np.meshgrid(np.arange(cv.height), np.arange(cv.width), indexing='ij')
    xn, yn = lm.undistort(MILD_BROWN, (uc - cv.cx) / cv.fx, (vc - cv.cy) / cv.fy)
    assert not np.isnan(xn).any()
    x, y = BASELINE + xn * Z_BOARD, yn * Z_BOARD
    on_board = (x >= BOARD_X[0]) & (x <= BOARD_X[1]) & (y >= BOARD_Y[0]) & (y <= BOARD_Y[1])
    colour = np.where(on_board[..., None], np.uint8(RED), np.uint8(GREEN)).astype(np.uint8)
    return sensor, model, [(depth, np.ascontiguousarray(colour))]


def shadow_band(splat):
    """The wall pixels of the depth image that may be lost, from the geometry alone: a mask over the depth image.

    Both planes face the sensors and depth_to_colour is a shift along x, so Pz = z and only a board pixel q can hide a wall pixel p:
    when |uc(q) - uc(p)| <= splat and |vc(q) - vc(p)| <= splat.  uc and vc are bent positions rounded to the nearest pixel, so the bent
    positions are at most splat + 1 apart in each axis, sqrt(2) (splat + 1) in all, and the pinhole colour positions at most
    R = stretch sqrt(2) (splat + 1), stretch = lens_stretch().  The colour sensor has twice the focal lengths and is b to the side: the
    pinhole colour position of depth pixel (u, v) at depth z is (2 u + 0.5 - 2 f b / z, 2 v + 0.5), f the depth sensor's.  So
        |u(p) - (u(q) - S)| <= R / 2,  |v(p) - v(q)| <= R / 2,   S = f b (1 / Z_BOARD - 1 / Z_WALL):
    p lies within R / 2 of the board's pixels shifted S to the left -- the parallax shadow of the board's left edge, widened by the
    splat and the two roundings.  The board's pixels are those whose centres lie inside the projection of its corners (cs.project)."""
    dv, cv = views()
    corners = cs.project(dv, [(BOARD_X[0], BOARD_Y[0], Z_BOARD), (BOARD_X[1], BOARD_Y[1], Z_BOARD)])
    (u0, v0), (u1, v1) = corners
    shift = dv.fx * BASELINE * (1.0 / Z_BOARD - 1.0 / Z_WALL)
    reach = lens_stretch(cv) * math.sqrt(2.0) * (splat + 1) / 2.0
    v, u = np.meshgrid(np.arange(dv.height), np.arange(dv.width), indexing='ij')
    return (u >= u0 - shift - reach) & (u <= u1 - shift + reach) & (v >= v0 - reach) & (v <= v1 + reach), shift, reach


def judge(depth, plain_depth, plain_rgb, occluded_depth, occluded_rgb, splat):
    """What the test asks, on the images a cloud is made from (one point per pixel with depth, with the registered colour).  Returns the
    figures it printed."""
    wall, board = depth == round(Z_WALL * 1000), depth == round(Z_BOARD * 1000)
    red = lambda rgb: (rgb == np.uint8(RED)).all(axis=-1)   # noqa: E731
    band, shift, reach = shadow_band(splat)
    leaked_plain = int((wall & (plain_depth != 0) & red(plain_rgb)).sum())
    leaked = int((wall & (occluded_depth != 0) & red(occluded_rgb)).sum())
    board_plain, board_kept = int((board & (plain_depth != 0)).sum()), int((board & (occluded_depth != 0)).sum())
    lost = wall & (plain_depth != 0) & (occluded_depth == 0)
    outside = int((lost & ~band).sum())
    print("shadow %.2f px wide, reach %.2f px; red wall points %d -> %d; board points %d -> %d; wall points lost %d, outside the band %d; wall pixels in the band %d"
          % (shift, reach, leaked_plain, leaked, board_plain, board_kept, int(lost.sum()), outside, int((band & wall).sum())))
    assert shift > 3 and leaked_plain > 0.5 * shift * (board.any(axis=1).sum())          # the scene shows the leak: most of the strip is red
    assert leaked == 0
    assert board_kept == board_plain == int(board.sum()) > 5000
    assert int(lost.sum()) >= leaked_plain and outside == 0
    assert (occluded_rgb[lost] == 0).all() and np.array_equal(occluded_rgb[~lost], plain_rgb[~lost])
    return leaked_plain, int(lost.sum())


def test_the_model_alone_on_the_scene():
    """No GPU: were a wall point lost outside the band here, the scene or the parameters would be wrong, not the bound."""
    sensor, model, frame = scene()
    dv, cv = views()
    occ = rule_of_thumb(dv, cv, Z_WALL)
    assert occ.splat == 2 and 0.009 < occ.margin < 0.011 < Z_WALL - Z_BOARD
    _points, plain_depth, plain_rgb = lm.cloud([model], frame)
    _points, depth, rgb, _hidden = om.cloud([model], frame, splat=occ.splat, margin=occ.margin)
    judge(frame[0][0], plain_depth[0], plain_rgb[0], depth[0], rgb[0], occ.splat)


@pytest.mark.gpu
def test_board_in_front_of_a_wall(gpu):
    sensor, model, frame = scene()
    dv, cv = views()
    occ = rule_of_thumb(dv, cv, Z_WALL)
    flags = gpu.CWIPC_HIP_RGBD_ATTACH_RGB | gpu.CWIPC_HIP_RGBD_ATTACH_DEPTH

    def images(pc):
        meta = pc.access_metadata()
        assert [meta.name(i) for i in range(2)] == ["rgb.scene", "depth.scene"]
        return (np.frombuffer(bytes(meta.data(0)), dtype=np.uint8).reshape(dv.height, dv.width, 3),
                np.frombuffer(bytes(meta.data(1)), dtype=np.uint16).reshape(dv.height, dv.width))

    with RgbdRig([sensor]) as rig:
        plain = rig.grab(frame, attach_flags=flags)
        occluded = rig.grab(frame, attach_flags=flags, occlusion=occ)
    plain_rgb, plain_depth = images(plain)
    rgb, depth = images(occluded)
    leaked_plain, lost = judge(frame[0][0], plain_depth, plain_rgb, depth, rgb, occ.splat)
    # the same in the clouds: the world is the depth camera's frame, so a point's z says which plane it is on
    def count(points, z, colour=None):
        on = np.abs(points['z'] - np.float32(z)) < 1e-4
        if colour is None:
            return int(on.sum())
        return int((on & (points['r'] == colour[0]) & (points['g'] == colour[1]) & (points['b'] == colour[2])).sum())

    before, after = plain.get_numpy_array(), occluded.get_numpy_array()
    assert count(before, Z_WALL, RED) == leaked_plain > 0 and count(after, Z_WALL, RED) == 0
    assert count(after, Z_BOARD) == count(before, Z_BOARD) == int((frame[0][0] == round(Z_BOARD * 1000)).sum())   # (red but for a rim that rounds onto the wall)
    assert count(after, Z_BOARD, RED) == count(before, Z_BOARD, RED) > 0.99 * count(before, Z_BOARD)
    assert len(before) - len(after) == lost
    # and both are the model's, byte for byte
    assert before.tobytes() == lm.cloud([model], frame)[0].tobytes()
    assert after.tobytes() == om.cloud([model], frame, splat=occ.splat, margin=occ.margin)[0].tobytes()
