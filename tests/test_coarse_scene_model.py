"""The coarse registration scene (tests/coarse_scene.py) on the CPU, with the renderer's numpy model in place of the GPU: the
poses show each camera the markers they are meant to, the stand-in detector finds exactly those, and a corner taken back to 3D
through the model's depth image is within the bound e that tests/test_gpu_multicoarse.py builds on."""
import numpy as np
import pytest

import coarse_scene as cs
import render_model as rm
from cwipc_util_amd.registration.render import default_view, deproject

POINT_SIZE = 5


@pytest.fixture(scope="module")
def rendered():
    """Per camera the model's (rgb, depth, index) of its tile in the identity view."""
    world = cs.board()
    view = default_view()
    return view, [rm.render_model(cs.camera_tile(world, k), view, POINT_SIZE)[:3] for k in range(len(cs.CAMERAS))]


def test_scene_geometry():
    world = cs.board()
    assert len(world) == 801 * 401 and (world['y'] == 0).all()
    for m in (0, 1):
        for c in range(4):
            n = int(((world['r'] == cs.CORNER_COLOURS[m][c][0]) & (world['g'] == cs.CORNER_COLOURS[m][c][1]) & (world['b'] == cs.CORNER_COLOURS[m][c][2])).sum())
            assert 20 <= n <= 40, (m, c, n)         # a disc of 6 mm in a 2 mm lattice
    assert len({col for cols in cs.CORNER_COLOURS.values() for col in cols}) == 8
    view = default_view()
    for k in range(len(cs.CAMERAS)):
        eye, target, _up = cs.CAMERAS[k]
        assert 1.2 <= np.linalg.norm(np.array(eye) - np.array(target)) <= 1.5
        for m in (0, 1):
            assert cs.visibility(view, k, m) == ('in' if m in cs.EXPECTED_VISIBLE[k] else 'out'), (k, m)
    assert cs.EXPECTED_VISIBLE == [{0}, {0, 1}, {1}, set()]


def test_detector_finds_each_marker_where_it_is_visible_and_within_e(rendered):
    view, images = rendered
    detect = cs.make_detector(POINT_SIZE)
    e = cs.corner_bound(view, POINT_SIZE, len(cs.CAMERAS))
    assert 0.010 < e < 0.025
    worst = 0.0
    for k, (rgb, depth, _index) in enumerate(images):
        areas, ids = detect(rgb)
        assert set(ids) == cs.EXPECTED_VISIBLE[k] and len(ids) == len(set(ids)), (k, ids)
        for area, m in zip(areas, ids):
            truth = cs.true_corners_in_camera(k, m)
            assert len(area) == 4
            for c, uv in enumerate(area):
                p = deproject(view, depth, uv)
                assert p is not None
                err = float(np.linalg.norm(np.array(p) - truth[c]))
                worst = max(worst, err)
                assert err <= e, (k, m, c, err, e)
    print("worst corner error %.2f mm, e = %.2f mm" % (worst * 1000, e * 1000))


def test_detector_wants_all_four_corners_and_enough_pixels(rendered):
    _view, images = rendered
    rgb = images[1][0].copy()
    detect = cs.make_detector(POINT_SIZE)
    assert detect(rgb)[1] == [0, 1]
    mask = (rgb == cs.CORNER_COLOURS[1][2]).all(axis=2)
    rows, cols = np.nonzero(mask)
    keep = POINT_SIZE ** 2 - 1
    rgb[rows[keep:], cols[keep:]] = 255          # one corner of marker 1 with too few pixels: the marker is not reported
    assert detect(rgb)[1] == [0]
