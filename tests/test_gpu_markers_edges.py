"""The marker detector where test_gpu_markers.py's small images do not reach: images of several trips of the kernels' grid-stride loops,
more rows than row workgroups, 32 chunks of the row scan, more candidates than decode waves, more words than lanes, every tie rule of
steps 5 and 7, the rejections of step 5, the threshold on grey data and the union-find under contention.  Everything is compared with
the numpy model (tests/marker_model.py) for equality, through test_gpu_markers.check; the images come from tests/marker_cases.py,
whose content test_marker_model.py states on the CPU.  DESIGN.md 3.15 names the constants the inputs are sized against."""
import numpy as np
import pytest

import coarse_scene as cs
import marker_cases as mc
import marker_model as mm
import marker_scene as ms
import test_gpu_markers as base
from conftest import make_cloud
from cwipc_util_amd.registration import default_view, render_pointcloud

pytestmark = pytest.mark.gpu

WORDS = mm.fixture_words()


def check(gpu, img, words=None, **params):
    """test_gpu_markers.check, its assertions as they are, against another dictionary (it reads its module's WORDS when it is called).
    The words go to the raw entry point, which takes bits 25-31 as they come."""
    if words is None:
        return base.check(gpu, img, **params)
    saved = base.WORDS
    base.WORDS = list(words)
    try:
        return base.check(gpu, img, **params)
    finally:
        base.WORDS = saved


def check_labels(gpu, img, **params):
    want = mm.label_image(mm.dark_mask(img, **params))
    got = gpu.cwipc_hip_marker_labels(img, gpu.cwipc_hip_marker_params(**params))
    assert got.dtype == np.int32 and np.array_equal(got, want)
    return got


# ---- several trips of the grid-stride loops ----
def test_two_trips_markers(gpu):
    """1024 x 600: rows from 512 on are every loop's second trip.  A marker before, across and past the boundary, and one whose label
    lies before it and whose area lies past it."""
    img = mc.two_trip_scene()
    check_labels(gpu, img)
    ids, corners = check(gpu, img)
    assert ids == mc.TWO_TRIPS_IDS
    assert corners[0].tolist() == [[100, 500], [127, 500], [127, 527], [100, 527]]
    assert corners[1].tolist() == [[300, 540], [327, 540], [327, 567], [300, 567]]
    assert corners[2].tolist() == [[600, 511], [634, 511], [634, 545], [600, 545]]


@pytest.mark.parametrize("pattern", ["block", "comb", "checkerboard", "joined_in_last_row", "noise"])
def test_two_trips_labels(gpu, pattern):
    """(The spiral stays at test_gpu_markers.py's sizes: without path compression its parent chains grow with the arm's length.)"""
    if pattern == "noise":
        img = mc.binary_noise(*mc.TWO_TRIPS, 0.59)
    else:
        img = mc.TORTURE_PATTERNS[pattern](*mc.TWO_TRIPS)
    got = check_labels(gpu, img, **mc.TORTURE_PARAMS)
    assert (got[512:] >= 0).any()
    if pattern in ("block", "comb", "joined_in_last_row"):   # a few large components: the later stages see them too
        check(gpu, img, **mc.TORTURE_PARAMS)


@pytest.fixture(scope="module")
def tile_b(gpu):
    """Camera B's tile of the marker scene: it sees both markers."""
    return make_cloud(gpu, cs.camera_tile(ms.board(), 1))


def test_full_hd_render(gpu, tile_b):
    """1920 x 1080, four trips: the rendered image for equality, and the one-call path against it as test_render_and_detect does at
    640 x 360."""
    view = default_view()
    assert (view.width, view.height) == (1920, 1080)
    rgb, depth, _index = render_pointcloud(tile_b, view, 5)
    ids, corners = check(gpu, rgb)
    assert ids == [0, 1]
    got_ids, got_corners, got_depth, found = gpu.cwipc_hip_render_detect_markers(tile_b, view.as_struct(), WORDS, 5)
    assert found == 2 and got_ids.tobytes() == np.asarray(ids, dtype=np.int32).tobytes() and got_corners.tobytes() == corners.tobytes()
    want_depth = np.array([[depth[int(v), int(u)] for u, v in marker] for marker in corners], dtype=np.float32)
    assert got_depth.dtype == np.float32 and got_depth.tobytes() == want_depth.tobytes() and (got_depth > 0).all()
    assert max(int(v) for marker in corners for _u, v in marker) * 1920 > 2 * 524288   # a corner past the second trip


# ---- more rows than row workgroups, 32 chunks of the row scan; the default window is clipped on all sides ----
def test_tall(gpu):
    img = mc.tall_image()
    check_labels(gpu, img)
    ids, corners = check(gpu, img)
    assert ids == mc.TALL_IDS
    assert corners[0].tolist() == [[3, 5], [16, 5], [16, 18], [3, 18]] and corners[1].tolist() == [[3, 4120], [16, 4120], [16, 4133], [3, 4133]]


def test_wide(gpu):
    img = mc.wide_image()
    check_labels(gpu, img)
    ids, corners = check(gpu, img)
    assert ids == mc.WIDE_IDS
    assert [c[0].tolist() for c in corners] == [[3, 3], [4100, 3], [8175, 3]] and corners[2][2].tolist() == [8188, 16]


# ---- more candidates than decode waves, more words than lanes ----
@pytest.mark.parametrize("nwords", [1100, 64, 65])
def test_grid_of_markers(gpu, nwords):
    img = mc.grid_image()
    words = mc.GRID_WORDS[:nwords]
    ids, corners = check(gpu, img, words)
    want = min(nwords, 1089)
    assert ids == list(range(want))
    assert corners.tolist() == [mc.grid_corners(n, **mc.GRID) for n in range(want)]
    if nwords == 1100:
        assert len(ids) == 1089
        for cap in (1088, 100):   # cap smaller than the number found: that number comes back, the first cap are written
            few_ids, few_corners, found = gpu.cwipc_hip_detect_markers(img, words, cap=cap)
            assert found == 1089 and few_ids.tolist() == ids[:cap] and np.array_equal(few_corners, corners[:cap])


# ---- ties of step 7: to the smallest id, then the smallest k ----
@pytest.mark.parametrize("nwords", mc.TIE_SIZES)
def test_id_and_rotation_ties(gpu, nwords):
    """Beside the model: the id and the first corner written out (marker_cases.TIE_EXPECTED says why)."""
    words = mc.tie_dictionary(nwords)
    for name, payload in mc.TIE_PAYLOADS.items():
        for rot in range(4):
            img = mc.painted_word(payload, rot)
            for errors in (0, 1, 2):
                ids, corners = check(gpu, img, words, max_bit_errors=errors)
                want = mc.tie_expected(name, nwords, rot, errors)
                if want is None:
                    assert ids == [], (name, rot, errors)
                else:
                    assert ids == [want[0]] and corners[0][0].tolist() == want[1], (name, rot, errors)


# ---- step 5: ties to the smallest linear index, and its rejections ----
@pytest.fixture(scope="module")
def thousand():
    return mc.tie_dictionary(1000)


@pytest.mark.parametrize("name", sorted(mc.SHAPES))
def test_shape(gpu, thousand, name):
    img = mc.SHAPES[name]()
    ids, corners = check(gpu, img, thousand, **mc.SHAPE_PARAMS)
    assert len(ids) == 1
    if name in mc.SHAPE_QUADS:
        assert corners[0].tolist() == mc.SHAPE_QUADS[name]
    # the border rule at its edge: the shape's own number of white border cells passes, one fewer does not
    white = mc.white_border_cells(img)
    assert check(gpu, img, thousand, **dict(mc.SHAPE_PARAMS, max_border_errors=white))[0] == ids
    if white > 0:
        assert check(gpu, img, thousand, **dict(mc.SHAPE_PARAMS, max_border_errors=white - 1))[0] == []


@pytest.mark.parametrize("name", sorted(mc.REJECTED_SHAPES))
def test_rejected_shape(gpu, thousand, name):
    assert check(gpu, mc.REJECTED_SHAPES[name][0](), thousand, **mc.SHAPE_PARAMS)[0] == []


def test_shape_sheet(gpu, thousand):
    ids, _corners = check(gpu, mc.shape_sheet(), thousand, **mc.SHAPE_PARAMS)
    assert len(ids) >= 2


def test_each_border_cell_counts(gpu):
    """Each of the 20 border cells that is no corner, white alone: one border error, neither none nor two."""
    for i, j in mc.BORDER_CELLS:
        img = mc.border_cell_whitened(i, j)
        assert check(gpu, img, max_border_errors=0)[0] == [], (i, j)
        assert check(gpu, img, max_border_errors=1)[0] == [4], (i, j)


# ---- the threshold on grey data ----
@pytest.mark.parametrize("size", [(61, 67), (130, 257), (20, 300)], ids=lambda s: "%dx%d" % (s[1], s[0]))
@pytest.mark.parametrize("kind", ["grey", "ramp"])
def test_threshold(gpu, kind, size):
    img = (mc.grey_noise if kind == "grey" else mc.ramp_noise)(*size)
    for window_half in (1, 3, 40, 8192):
        for threshold_offset in (0, 7, 255):
            params = dict(window_half=window_half, threshold_offset=threshold_offset)
            got = check_labels(gpu, img, **params)
            assert (got >= 0).any() == (threshold_offset < 255)
            check(gpu, img, **params, max_border_errors=24, max_bit_errors=25)


# ---- step 8 on areas that waves with several labels add up lane by lane ----
def test_area_rule(gpu):
    ids, corners = check(gpu, mc.area_rule_scene())
    assert ids == [3, 5]
    assert corners[0].tolist() == [[130, 5], [157, 5], [157, 32], [130, 32]]        # equal areas: the smaller label
    assert corners[1].tolist() == [[130, 80], [164, 80], [164, 114], [130, 114]]    # the larger area


# ---- the union-find under contention ----
@pytest.mark.parametrize("size", [(130, 257), mc.TWO_TRIPS], ids=lambda s: "%dx%d" % (s[1], s[0]))
@pytest.mark.parametrize("density", mc.NOISE_DENSITIES)
def test_contention(gpu, density, size):
    """Ragged components: most waves see several labels and their unions collide.  Twice, for identical bytes: the order of the
    candidate list is arbitrary and nothing that goes out may depend on it."""
    img = mc.binary_noise(*size, density)
    loose = dict(max_border_errors=24, max_bit_errors=25)
    labels = check_labels(gpu, img)
    ids, corners = check(gpu, img, **loose)
    again = gpu.cwipc_hip_detect_markers(img, WORDS, gpu.cwipc_hip_marker_params(**loose))
    assert gpu.cwipc_hip_marker_labels(img).tobytes() == labels.tobytes()
    assert again[0].tobytes() == np.asarray(ids, dtype=np.int32).tobytes() and again[1].tobytes() == corners.tobytes()
