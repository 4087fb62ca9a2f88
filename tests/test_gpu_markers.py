"""cwipc_hip_detect_markers, cwipc_hip_render_detect_markers and cwipc_hip_marker_labels on the GPU against the numpy model
(tests/marker_model.py): ids, corners and labels for equality.  The images come from tests/marker_cases.py, whose content
test_marker_model.py checks on the CPU."""
import ctypes
import sys

import numpy as np
import pytest

import coarse_scene as cs
import marker_cases as mc
import marker_model as mm
import marker_scene as ms
from conftest import make_cloud
from cwipc_util_amd.registration import (MarkerDictionary, MultiCameraCoarseAruco, default_view, detect_markers, gpu_marker_detector,
                                         render_pointcloud)

pytestmark = pytest.mark.gpu

WORDS = mm.fixture_words()
DICTIONARY = MarkerDictionary(WORDS)


def check(gpu, img, **params):
    """The GPU's answer equals the model's; returns it as (ids, corners)."""
    want_ids, want_corners = mm.detect(img, WORDS, **params)
    ids, corners, found = gpu.cwipc_hip_detect_markers(img, WORDS, gpu.cwipc_hip_marker_params(**params))
    assert found == len(want_ids)
    assert ids.dtype == np.int32 and corners.dtype == np.float32 and corners.shape == (found, 4, 2)
    assert ids.tolist() == want_ids
    assert np.array_equal(corners, want_corners.astype(np.float32))
    return ids.tolist(), corners


@pytest.mark.parametrize("id", range(8))
def test_axis_aligned(gpu, id):
    ids, corners = check(gpu, mc.axis_aligned(id))
    assert ids == [id] and corners[0].tolist() == [[30, 17], [57, 17], [57, 44], [30, 44]]


def test_half_pixel_samples(gpu):
    """2-pixel cells, a 13-pixel span between the corners: the samples U = 14 and V = 14 fall on exact half pixels."""
    ids, corners = check(gpu, mc.axis_aligned(0, cell=2, left=40, top=20))
    assert ids == [0] and corners[0].tolist() == [[40, 20], [53, 20], [53, 33], [40, 33]]


@pytest.mark.parametrize("rot", [1, 2, 3])
def test_quarter_turns(gpu, rot):
    """The corner order follows the marker: its top-left corner comes first wherever it is in the image."""
    upright = [[30, 17], [57, 17], [57, 44], [30, 44]]
    ids, corners = check(gpu, mc.axis_aligned(0, rot=rot))
    assert ids == [0] and corners[0].tolist() == [upright[(q - rot) % 4] for q in range(4)]


def test_rotated_warped_mirrored(gpu):
    for img, quad in ((mc.rotated30(), mc.square_quad(48.0, 48.0, 49.0, 30.0)), (mc.perspective(), mc.PERSPECTIVE_QUAD)):
        ids, corners = check(gpu, img)
        assert ids == [0] and np.abs(corners[0] - np.array(quad)).max() <= 1.5
    assert check(gpu, mc.axis_aligned(0, mirror=True))[0] == []


def test_mixed_scene(gpu):
    img = mc.mixed_scene()
    ids, corners = check(gpu, img)
    assert ids == mc.MIXED_IDS
    assert corners[1].tolist() == [[230, 8], [271, 8], [271, 49], [230, 49]]   # of the two copies of id 3 the larger
    # the Python layer: the MarkerDetector shape
    areas, got_ids = detect_markers(img, DICTIONARY)
    assert got_ids == ids and areas == corners.astype(np.float64).tolist()
    assert gpu_marker_detector(DICTIONARY)(img) == (areas, got_ids)
    # cap smaller than the number found: the return value is the number found, the first cap are written
    few_ids, few_corners, found = gpu.cwipc_hip_detect_markers(img, WORDS, cap=2)
    assert found == 4 and few_ids.tolist() == ids[:2] and np.array_equal(few_corners, corners[:2])
    none_ids, _none_corners, found = gpu.cwipc_hip_detect_markers(img, WORDS, cap=0)
    assert found == 4 and len(none_ids) == 0
    # a pure function of the image
    again = gpu.cwipc_hip_detect_markers(img, WORDS)
    assert again[0].tobytes() == np.asarray(ids, dtype=np.int32).tobytes() and again[1].tobytes() == corners.tobytes()


@pytest.mark.parametrize("size", mc.TORTURE_SIZES, ids=lambda s: "%dx%d" % (s[1], s[0]))
@pytest.mark.parametrize("pattern", sorted(mc.TORTURE_PATTERNS))
def test_labels(gpu, pattern, size):
    img = mc.TORTURE_PATTERNS[pattern](*size)
    want = mm.label_image(mm.dark_mask(img, **mc.TORTURE_PARAMS))
    got = gpu.cwipc_hip_marker_labels(img, gpu.cwipc_hip_marker_params(**mc.TORTURE_PARAMS))
    assert got.dtype == np.int32 and np.array_equal(got, want)
    check(gpu, img, **mc.TORTURE_PARAMS)   # (none of these is a marker; the later stages see them all the same)


def test_labels_of_a_scene(gpu):
    """The default window on an image with grey levels: the mask's threshold, not only the labelling."""
    rng = np.random.default_rng(3)
    img = mc.mixed_scene()
    img = np.clip(img.astype(np.int64) + rng.integers(-40, 41, img.shape), 0, 255).astype(np.uint8)
    assert np.array_equal(gpu.cwipc_hip_marker_labels(img), mm.label_image(mm.dark_mask(img)))
    check(gpu, img)


def test_error_tolerance(gpu):
    flipped = mc.payload_flipped()
    assert check(gpu, flipped, max_bit_errors=0)[0] == []
    assert check(gpu, flipped, max_bit_errors=1)[0] == [4]
    assert check(gpu, mc.border_whitened(), max_border_errors=1)[0] == []
    assert check(gpu, mc.border_whitened(), max_border_errors=2)[0] == [4]
    assert check(gpu, mc.border_whitened(n=3))[0] == []   # the default lets two pass


def test_argument_checks(gpu):
    dll = gpu.cwipc_util_dll_load()
    img = mc.axis_aligned(0)
    words = np.asarray(WORDS, dtype=np.uint32)
    ids = np.zeros(8, dtype=np.int32)
    corners = np.zeros((8, 4, 2), dtype=np.float32)

    def call(rgb=img.ctypes.data, width=96, height=64, dictionary=words.ctypes.data, n=8, params=None, out_ids=ids.ctypes.data, out=corners.ctypes.data, cap=8):
        rc = dll.cwipc_hip_detect_markers(rgb, width, height, dictionary, n, ctypes.addressof(params) if params is not None else None, out_ids, out, cap)
        return rc, dll.cwipc_hip_last_error().decode('utf8')

    assert call()[0] == 1
    for kw in (dict(rgb=None), dict(dictionary=None), dict(out_ids=None), dict(out=None)):
        rc, text = call(**kw)
        assert rc == -1 and "NULL argument" in text
    assert call(out_ids=None, out=None, cap=0)[0] == 1
    for kw in (dict(width=0), dict(height=0), dict(width=-1), dict(width=8193, height=1), dict(width=1, height=8193), dict(width=8192, height=4096)):
        rc, text = call(**kw)
        assert rc == -1 and "between 1 and 8192" in text and "2^24" in text
    rc, text = call(n=0)
    assert rc == -1 and "nmarkers" in text
    P = gpu.cwipc_hip_marker_params
    for params, name in ((P(window_half=0), "window_half"), (P(window_half=8193), "window_half"), (P(threshold_offset=-1), "threshold_offset"),
                         (P(threshold_offset=256), "threshold_offset"), (P(min_side=1), "min_side"), (P(min_side=8193), "min_side"),
                         (P(max_border_errors=-1), "max_border_errors"), (P(max_border_errors=25), "max_border_errors"),
                         (P(max_bit_errors=-1), "max_bit_errors"), (P(max_bit_errors=26), "max_bit_errors")):
        rc, text = call(params=params)
        assert rc == -1 and name in text
    assert call(params=P())[0] == 1
    with pytest.raises(gpu.CwipcError, match="min_side"):
        gpu.cwipc_hip_detect_markers(img, WORDS, P(min_side=0))
    with pytest.raises(gpu.CwipcError, match="window_half"):
        gpu.cwipc_hip_marker_labels(img, P(window_half=0))
    with pytest.raises(gpu.CwipcError):
        gpu.cwipc_hip_detect_markers(img[:, :, :2], WORDS)
    # an image of one pixel, and a line: nothing to find, no error
    assert gpu.cwipc_hip_detect_markers(np.zeros((1, 1, 3), dtype=np.uint8), WORDS)[2] == 0
    assert gpu.cwipc_hip_detect_markers(mm.white(1, 300), WORDS)[2] == 0


# ---- staying on the device ----
SMALL_VIEW = dict(width=640, height=360)


@pytest.fixture(scope="module")
def scene(gpu):
    """The marker scene's world cloud, camera B's tile (it sees both markers) and the three-camera capture."""
    world = ms.board()
    tiles = [cs.camera_tile(world, k) for k in range(3)]
    return make_cloud(gpu, tiles[1]), make_cloud(gpu, np.concatenate(tiles))


def test_render_and_detect(gpu, scene):
    tile_b, _capture = scene
    view = default_view(**SMALL_VIEW)
    rgb, depth, _index = render_pointcloud(tile_b, view, 5)
    ids, corners = check(gpu, rgb)
    assert ids == [0, 1]
    got_ids, got_corners, got_depth, found = gpu.cwipc_hip_render_detect_markers(tile_b, view.as_struct(), WORDS, 5)
    assert found == 2 and got_ids.tobytes() == np.asarray(ids, dtype=np.int32).tobytes() and got_corners.tobytes() == corners.tobytes()
    want_depth = np.array([[depth[int(v), int(u)] for u, v in marker] for marker in corners], dtype=np.float32)
    assert got_depth.dtype == np.float32 and got_depth.tobytes() == want_depth.tobytes() and (got_depth > 0).all()
    again = gpu.cwipc_hip_render_detect_markers(tile_b, view.as_struct(), WORDS, 5)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again[:3], (got_ids, got_corners, got_depth)))
    # the tile mask and the parameters reach both halves: no tile 1 in this cloud, and a min_side no marker here has
    assert gpu.cwipc_hip_render_detect_markers(tile_b, view.as_struct(), WORDS, 5, tilemask=1)[3] == 0
    assert gpu.cwipc_hip_render_detect_markers(tile_b, view.as_struct(), WORDS, 5, params=gpu.cwipc_hip_marker_params(min_side=200))[3] == 0
    # errors of both calls
    with pytest.raises(gpu.CwipcError, match="point_size"):
        gpu.cwipc_hip_render_detect_markers(tile_b, view.as_struct(), WORDS, 4)
    with pytest.raises(gpu.CwipcError, match="max_bit_errors"):
        gpu.cwipc_hip_render_detect_markers(tile_b, view.as_struct(), WORDS, 5, params=gpu.cwipc_hip_marker_params(max_bit_errors=99))
    # cwipc_hip_render itself is what it was: the same image from the factored driver as the model's (test_gpu_render.py holds the rest)
    assert np.array_equal(rgb, render_pointcloud(tile_b, view, 5)[0])


def test_end_to_end(gpu, scene):
    """MultiCameraCoarseAruco with a dictionary and nothing else: no detector, no cv2.  Camera A sees marker 0, camera B both, camera C
    marker 1 only, so C is registered in the second pass, through the position camera B gave marker 1.

    The bound.  e (marker_scene.corner_bound, derived there from the pixel size at the corners' depth, the splat's half width and the
    sample spacing; 40.3 mm for this scene) bounds one deprojected corner.  For the transformations the argument of
    test_gpu_multicoarse.py holds unchanged: a least-squares fit of four corners each within e of the truth moves the true corners to
    within 3 e of their targets, and a learnt marker's corners are within 4 e.
    Measured with the two numpy models (test_marker_model.py, the images the GPU's equal): worst corner 6.3 mm."""
    _tile_b, capture = scene
    view = default_view()
    for k in range(3):
        for m in (0, 1):
            assert cs.visibility(view, k, m) == ('in' if m in cs.EXPECTED_VISIBLE[k] else 'out')
    algo = MultiCameraCoarseAruco()
    assert algo.marker_detector is None
    algo.set_marker_dictionary(MarkerDictionary.from_file(mm.FIXTURE))
    algo.set_tiled_pointcloud(capture)
    assert algo.run() is True
    assert [set(m) for m in algo.markers] == cs.EXPECTED_VISIBLE[:3]
    e = ms.corner_bound(view, algo.point_size)
    worst_corner = 0.0
    for k in range(3):
        for m, found in algo.markers[k].items():
            assert len(found) == 4
            worst_corner = max(worst_corner, float(np.linalg.norm(np.asarray(found) - cs.true_corners_in_camera(k, m), axis=1).max()))
    assert sorted(algo.known_marker_positions) == [0, 1]
    assert not np.array_equal(algo.get_result_transformations()[2], np.identity(4))
    worst = 0.0
    for k in range(3):
        T = algo.get_result_transformations()[algo.camera_index_for_tilemask(1 << k)]
        for m in cs.EXPECTED_VISIBLE[k]:
            moved = cs.true_corners_in_camera(k, m) @ T[:3, :3].T + T[:3, 3]
            worst = max(worst, float(np.linalg.norm(moved - np.asarray(cs.MARKERS[m]), axis=1).max()))
    print("worst corner %.2f mm, e = %.2f mm; worst residual %.2f mm, 3 e = %.2f mm" % (worst_corner * 1000, e * 1000, worst * 1000, 3 * e * 1000))
    assert worst_corner <= e
    assert np.linalg.norm(np.asarray(algo.known_marker_positions[1]) - np.asarray(cs.MARKERS[1]), axis=1).max() <= 4 * e
    assert worst <= 3 * e
    # the same through the host: an explicit detector comes before the dictionary and sees the same images
    host = MultiCameraCoarseAruco()
    host.set_marker_dictionary(DICTIONARY)
    host.set_marker_detector(gpu_marker_detector(DICTIONARY))
    host.set_tiled_pointcloud(capture)
    assert host.run() is True
    for a, b in zip(host.get_result_transformations(), algo.get_result_transformations()):
        assert np.array_equal(a, b)


def test_nothing_set_names_both_remedies(gpu, scene, monkeypatch):
    monkeypatch.setitem(sys.modules, "cv2", None)
    monkeypatch.setitem(sys.modules, "cv2.aruco", None)
    algo = MultiCameraCoarseAruco()
    algo.set_tiled_pointcloud(scene[1])
    with pytest.raises(RuntimeError, match=r"set_marker_detector\(\).*set_marker_dictionary\(\)"):
        algo.run()
