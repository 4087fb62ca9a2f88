"""Coarse registration end to end on the GPU (registration/multicoarse.py): the scene of tests/coarse_scene.py, rendered by
cwipc_hip_render, with the stand-in detector in place of cv2.aruco."""
import sys

import numpy as np
import pytest

import coarse_scene as cs
from conftest import make_cloud
from cwipc_util_amd.registration import MultiCameraCoarseAruco, default_view

pytestmark = pytest.mark.gpu

POINT_SIZE = 5


@pytest.fixture(scope="module")
def captures(gpu):
    """The joined tiles of three and of four cameras, as clouds."""
    world = cs.board()
    tiles = [cs.camera_tile(world, k) for k in range(4)]
    return make_cloud(gpu, np.concatenate(tiles[:3])), make_cloud(gpu, np.concatenate(tiles))


def _run(pc):
    algo = MultiCameraCoarseAruco()
    assert algo.point_size == POINT_SIZE and algo.view_for_camera_index(0).extrinsic.tolist() == np.identity(4).tolist()   # default_view()
    algo.set_marker_detector(cs.make_detector(POINT_SIZE))
    algo.set_tiled_pointcloud(pc)
    return algo, algo.run()


def _worst_residual(algo, ncameras):
    worst = 0.0
    for k in range(ncameras):
        T = algo.get_result_transformations()[algo.camera_index_for_tilemask(1 << k)]
        for m in cs.EXPECTED_VISIBLE[k]:
            moved = cs.true_corners_in_camera(k, m) @ T[:3, :3].T + T[:3, 3]
            worst = max(worst, float(np.linalg.norm(moved - np.asarray(cs.MARKERS[m]), axis=1).max()))
    return worst


def test_three_cameras(gpu, captures):
    """Camera A sees marker 0, camera B both markers, camera C only marker 1: C can only be registered through marker 1, whose
    position nobody knows before camera B, registered through marker 0, has seen it.

    The bound.  e (coarse_scene.corner_bound) bounds one deprojected corner: 6 mm of patch radius, 2 (h + 1) pixels at the largest
    corner depth for the rounded centroid, the splat's half width and the half pixel _deproject leaves out, 2 mm of sample spacing;
    17.5 mm here.  A camera's matrix is the least-squares fit of four measured corners m_i = p_i + d_i, |d_i| <= e, onto targets
    t_i.  With exact targets t_i = T p_i the true matrix T leaves residuals |T m_i - t_i| <= e, so the fitted matrix F has
    sum |F m_i - t_i|^2 <= 4 e^2, each residual <= 2 e, and |F p_i - T p_i| <= |F p_i - F m_i| + |F m_i - t_i| <= e + 2 e = 3 e.
    That is rigorous for the corners of the marker a camera was fitted on when that marker's position is exact (cameras A and B,
    marker 0).  For camera B's view of marker 1 and for camera C, whose targets are themselves B's estimate, a worst case would
    add a lever-arm term that no measurement comes near; the check keeps 3 e for every camera and every visible marker.
    Measured with the renderer's numpy model, whose images the GPU's equal byte for byte: worst corner 5.1 mm, worst residual
    4.9 mm."""
    pc, _ = captures
    view = default_view()
    for k in range(3):
        for m in (0, 1):
            assert cs.visibility(view, k, m) == ('in' if m in cs.EXPECTED_VISIBLE[k] else 'out')
    algo, ok = _run(pc)
    assert ok is True
    assert [algo.tilemask_for_camera_index(i) for i in range(3)] == [1, 2, 4]
    assert [set(m) for m in algo.markers] == cs.EXPECTED_VISIBLE[:3]
    # marker 1 was learnt (from camera B, the only registered camera that sees it) and camera C, which never sees marker 0, is registered
    assert sorted(algo.known_marker_positions) == [0, 1]
    assert not np.array_equal(algo.get_result_transformations()[2], np.identity(4))
    e = cs.corner_bound(view, POINT_SIZE)
    # (the learnt corners are camera B's measured corners, each within e of the true ones, moved by B's matrix: 3 e + e)
    assert np.linalg.norm(np.asarray(algo.known_marker_positions[1]) - np.asarray(cs.MARKERS[1]), axis=1).max() <= 4 * e
    worst = _worst_residual(algo, 3)
    print("worst residual %.2f mm, 3 e = %.2f mm" % (worst * 1000, 3 * e * 1000))
    assert worst <= 3 * e
    # the result cloud: every tile, moved by its camera's matrix
    full = algo.get_result_pointcloud_full()
    assert full.count() == pc.count() and gpu.get_tiles_used(full) == [1, 2, 4]


def test_camera_without_marker_stays_unregistered(gpu, captures):
    pc3, pc4 = captures
    algo3, _ = _run(pc3)
    algo, ok = _run(pc4)
    assert ok is False
    got = algo.get_result_transformations()
    assert len(got) == 4 and np.array_equal(got[3], np.identity(4)) and algo._get_unregistered_tiles() == [3]
    assert algo.markers[3] == {}
    for k in range(3):
        assert np.array_equal(got[k], algo3.get_result_transformations()[k])
    assert _worst_residual(algo, 3) <= 3 * cs.corner_bound(default_view(), POINT_SIZE)


def test_no_detector_and_no_cv2(gpu, captures, monkeypatch):
    """Without a detector and without cv2 the call says what is missing instead of finding no markers."""
    monkeypatch.setitem(sys.modules, "cv2", None)          # `import cv2` raises ImportError
    monkeypatch.setitem(sys.modules, "cv2.aruco", None)
    algo = MultiCameraCoarseAruco()
    algo.set_tiled_pointcloud(captures[0])
    algo._prepare()
    with pytest.raises(RuntimeError, match="detector must be set"):
        algo._find_markers(0, 0)
    algo = MultiCameraCoarseAruco()
    algo.set_tiled_pointcloud(captures[0])
    with pytest.raises(RuntimeError, match="set_marker_detector"):
        algo.run()
