"""The host arithmetic of the coarse registration (registration/multicoarse.py, registration/render.py): the rigid fit of a marker's
corners, the depth mean around a pixel, and the run() loop's bookkeeping with hand-made markers.  No GPU."""
import numpy as np
import pytest

from cwipc_util_amd import registration as reg
from cwipc_util_amd.registration.multicoarse import MultiCameraCoarse, MultiCameraCoarseAruco
from cwipc_util_amd.registration.render import mean_depth, look_at


def _rigid(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    rot = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                    [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                    [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    m = np.identity(4)
    m[:3, :3] = rot
    m[:3, 3] = rng.uniform(-2, 2, 3)
    return m


def test_align_marker_recovers_a_rigid_motion():
    rng = np.random.default_rng(1)
    algo = MultiCameraCoarseAruco()
    target = np.array(algo.known_marker_positions[0], dtype=float)
    for _ in range(20):
        m = _rigid(rng)                                        # camera -> world
        inv = np.linalg.inv(m)
        seen = target @ inv[:3, :3].T + inv[:3, 3]             # the corners as the camera sees them
        got = algo._align_marker(0, [tuple(p) for p in target], [tuple(p) for p in seen])
        assert np.abs(got - m).max() <= 1e-12
        assert got[3].tolist() == [0, 0, 0, 1]


def test_align_marker_with_swapped_corners_is_still_a_rotation():
    rng = np.random.default_rng(2)
    algo = MultiCameraCoarse()
    target = np.array([(+0.087, 0, +0.087), (-0.087, 0, +0.087), (-0.087, 0, -0.087), (+0.087, 0, -0.087)])
    for _ in range(20):
        m = _rigid(rng)
        inv = np.linalg.inv(m)
        seen = target @ inv[:3, :3].T + inv[:3, 3]
        seen[[1, 3]] = seen[[3, 1]]                            # the outline now runs the other way round: a mirror image
        got = algo._align_marker(0, target.tolist(), seen.tolist())
        rot = got[:3, :3]
        assert np.linalg.det(rot) == pytest.approx(1.0, abs=1e-12) and np.allclose(rot @ rot.T, np.identity(3), atol=1e-12)
        # the centroids still meet
        assert np.allclose(rot @ seen.mean(axis=0) + got[:3, 3], target.mean(axis=0), atol=1e-12)
    assert algo._align_marker(0, target.tolist(), target[:3].tolist()) is None
    bad = target.copy()
    bad[2, 1] = np.nan
    assert algo._align_marker(0, target.tolist(), bad.tolist()) is None


def test_mean_depth():
    img = np.zeros((20, 30), dtype=np.uint16)
    # the `minimum` rule: nine values are not enough, ten are
    img[9:12, 9:12] = 1000
    assert mean_depth(img, 10, 10) == 0
    img[12, 12] = 1009
    assert mean_depth(img, 10, 10) == (9 * 1000 + 1009) // 10 == 1000
    assert mean_depth(img, 10, 10, minimum=11) == 0
    # zeros are skipped, not averaged in; values outside the window do not count
    img[:] = 0
    img[7:14, 7:14] = 500          # the whole 7x7 window
    img[8, 8] = 0
    img[10, 10] = 0                # the pixel itself may be a hole
    img[6, 10] = 60000
    img[10, 14] = 60000
    assert mean_depth(img, 10, 10) == 500
    assert mean_depth(img, 10, 10, offset=4) == (47 * 500 + 2 * 60000) // 49
    # the image border: only the part of the window inside the image
    img[:] = 0
    img[0:4, 0:4] = 800            # 16 pixels around (0, 0) are inside
    assert mean_depth(img, 0, 0) == 800
    assert mean_depth(img, 0, 0, minimum=17) == 0
    img[16:, 26:] = 700
    assert mean_depth(img, 29, 19) == 700 and mean_depth(img, 40, 19) == 0 and mean_depth(img, -5, -5) == 0
    # x is the column, y the row
    img[:] = 0
    img[2:9, 20:27] = 300
    assert mean_depth(img, 23, 5) == 300 and mean_depth(img, 5, 23) == 0
    # a float image (metres, the renderer's depth): the mean, not its floor
    f = np.zeros((10, 10), dtype=np.float32)
    f[2:6, 2:6] = 1.5
    f[2, 2] = 2.5
    assert mean_depth(f, 4, 4) == pytest.approx((15 * 1.5 + 2.5) / 16)
    assert mean_depth(f, 9, 9) == 0


class _HandMade(MultiCameraCoarse):
    """Markers given by hand per tile number; the cloud is only asked for its tile numbers."""

    def __init__(self, tilenums, markers_by_tile):
        MultiCameraCoarse.__init__(self)
        self._tilenums = tilenums
        self._by_tile = markers_by_tile
        self.original_pointcloud = object()

    def _prepare(self):
        self.per_camera_tilenum = list(self._tilenums)
        self._init_transformations()

    def _find_markers(self, passnum, camindex):
        return self._by_tile[self.per_camera_tilenum[camindex]]


def test_run_hands_markers_from_registered_cameras_to_unregistered_ones():
    """Camera 4 sees only marker 7, camera 2 sees markers 0 and 7, camera 1 only marker 0, camera 8 nothing; the cameras come in the
    order 4, 2, 1, 8, so that camera 4 can only be registered in the second pass, through marker 7 learnt from camera 2."""
    rng = np.random.default_rng(3)
    m0 = np.array([(+0.087, 0, +0.087), (-0.087, 0, +0.087), (-0.087, 0, -0.087), (+0.087, 0, -0.087)])
    m7 = m0 + [0.9, 0, 0.1]
    poses = {t: _rigid(rng) for t in (1, 2, 4, 8)}   # camera -> world

    def seen(t, world):
        inv = np.linalg.inv(poses[t])
        return [tuple(p) for p in world @ inv[:3, :3].T + inv[:3, 3]]

    by_tile = {4: {7: seen(4, m7)}, 2: {0: seen(2, m0), 7: seen(2, m7)}, 1: {0: seen(1, m0), 5: seen(1, m7)[:3]}, 8: {}}
    algo = _HandMade([4, 2, 1, 8], by_tile)
    algo.known_marker_positions = {0: [tuple(p) for p in m0]}
    assert algo.run() is False                              # camera 8 stays unregistered
    got = algo.get_result_transformations()
    for i, t in enumerate((4, 2, 1)):
        assert np.abs(got[i] - poses[t]).max() < 1e-9, t
    assert np.array_equal(got[3], np.identity(4)) and algo._get_unregistered_tiles() == [3]
    assert np.allclose(algo.known_marker_positions[7], m7, atol=1e-9) and 5 not in algo.known_marker_positions
    assert algo.camera_index_for_tilemask(2) == 1 and algo.tilemask_for_camera_index(0) == 4 and algo.camera_count() == 4
    # without camera 8 everything is registered
    algo = _HandMade([4, 2, 1], by_tile)
    algo.known_marker_positions = {0: [tuple(p) for p in m0]}
    assert algo.run() is True
    # a camera's first transformation is kept: a second, different marker position for a registered camera changes nothing
    by_tile2 = {1: {0: seen(1, m0), 7: seen(1, m7)}}
    algo = _HandMade([1], by_tile2)
    algo.known_marker_positions = {0: [tuple(p) for p in m0], 7: [tuple(p) for p in m7 + 0.05]}
    assert algo.run() is True and np.abs(algo.get_result_transformations()[0] - poses[1]).max() < 1e-9


def test_exports_and_detector_plumbing():
    assert reg.MultiCameraCoarse is MultiCameraCoarse and reg.MultiCameraCoarseAruco is MultiCameraCoarseAruco
    assert issubclass(MultiCameraCoarseAruco, MultiCameraCoarse) and issubclass(MultiCameraCoarse, reg.MulticamAlignmentAlgorithm)
    assert MultiCameraCoarse not in reg.ALL_MULTICAMERA_ALGORITHMS and MultiCameraCoarseAruco not in reg.ALL_MULTICAMERA_ALGORITHMS
    algo = MultiCameraCoarseAruco()
    assert algo.verbose is False and sorted(algo.known_marker_positions) == [0]
    assert algo.view_for_camera_index(3).width == 1920
    v = reg.default_view(64, 48, extrinsic=look_at((0, 1, -3), (0, 1, 0), (0, 1, 0)))
    algo.set_view(1, v)
    assert algo.view_for_camera_index(1) is v and algo.view_for_camera_index(0).width == 1920
    algo.set_view(None, v)
    assert algo.view_for_camera_index(0) is v
