"""The marker detector's numpy model (tests/marker_model.py) against plain loops, the dictionary fixture, and the test images the GPU
tests rely on (tests/marker_cases.py, tests/marker_scene.py): no GPU here."""
import math

import numpy as np
import pytest

import coarse_scene as cs
import marker_cases as mc
import marker_model as mm
import marker_scene as ms
import render_model as rm
from cwipc_util_amd.registration import MarkerDictionary, default_view, deproject

WORDS = mm.fixture_words()


# ---- plain loops ----
def dark_loops(rgb, w, offset):
    H, W = rgb.shape[:2]
    y = [[(77 * int(rgb[r, c, 0]) + 150 * int(rgb[r, c, 1]) + 29 * int(rgb[r, c, 2]) + 128) >> 8 for c in range(W)] for r in range(H)]
    dark = np.zeros((H, W), dtype=bool)
    for r in range(H):
        for c in range(W):
            s = n = 0
            for rr in range(max(r - w, 0), min(r + w, H - 1) + 1):
                for cc in range(max(c - w, 0), min(c + w, W - 1) + 1):
                    s += y[rr][cc]
                    n += 1
            dark[r, c] = y[r][c] * n + offset * n < s
    return dark


def labels_loops(dark):
    H, W = dark.shape
    out = np.full((H, W), -1, dtype=np.int32)
    for r in range(H):
        for c in range(W):
            if not dark[r, c] or out[r, c] >= 0:
                continue
            # raster order: the first pixel of a component that is met is its smallest index
            stack = [(r, c)]
            out[r, c] = r * W + c
            while stack:
                pr, pc = stack.pop()
                for qr, qc in ((pr - 1, pc), (pr + 1, pc), (pr, pc - 1), (pr, pc + 1)):
                    if 0 <= qr < H and 0 <= qc < W and dark[qr, qc] and out[qr, qc] < 0:
                        out[qr, qc] = r * W + c
                        stack.append((qr, qc))
    return out


def quad_loops(index, W):
    index = sorted(int(i) for i in index)   # ascending: a strict comparison keeps the smallest index among equals

    def farthest(fx, fy):
        best, arg = -1, None
        for i in index:
            d = (i % W - fx) ** 2 + (i // W - fy) ** 2
            if d > best:
                best, arg = d, i
        return arg
    a = farthest(index[0] % W, index[0] // W)
    c = farthest(a % W, a // W)
    ax, ay, cx, cy = a % W, a // W, c % W, c // W
    kb = kd = None
    for i in index:
        k = (i % W - ax) * (cy - ay) - (i // W - ay) * (cx - ax)
        if kb is None or k > kb[0]:
            kb = (k, i)
        if kd is None or k < kd[0]:
            kd = (k, i)
    if not (kb[0] > 0 > kd[0]):
        return None
    P = [(i % W, i // W) for i in (a, kb[1], c, kd[1])]
    cross = [(P[(q + 1) % 4][0] - P[q][0]) * (P[(q + 2) % 4][1] - P[(q + 1) % 4][1])
             - (P[(q + 1) % 4][1] - P[q][1]) * (P[(q + 2) % 4][0] - P[(q + 1) % 4][0]) for q in range(4)]
    if not (min(cross) > 0 or max(cross) < 0):
        return None
    shoelace = sum(P[q][0] * P[(q + 1) % 4][1] - P[(q + 1) % 4][0] * P[q][1] for q in range(4))
    return P if shoelace > 0 else [P[0], P[3], P[2], P[1]]


def tiny_images():
    rng = np.random.default_rng(7)
    out = [rng.integers(0, 256, (13, 17, 3), dtype=np.uint8), (rng.integers(0, 2, (11, 9, 1), dtype=np.uint8) * 255).repeat(3, axis=2)]
    out.append(mc.axis_aligned(0, cell=2, left=5, top=4, size=(24, 27)))
    return out


@pytest.mark.parametrize("w, offset", [(1, 0), (3, 7), (40, 7)])
def test_mask_and_labels_against_loops(w, offset):
    for img in tiny_images():
        dark = mm.dark_mask(img, w, offset)
        assert np.array_equal(dark, dark_loops(img, w, offset))
        assert np.array_equal(mm.label_image(dark), labels_loops(dark))


def test_quads_against_loops():
    checked = 0
    for img in tiny_images() + [mc.rotated30(), mc.perspective(), mc.mixed_scene()]:
        W = img.shape[1]
        lab = mm.label_image(mm.dark_mask(img, 40, 7)).reshape(-1)
        for root in np.unique(lab[lab >= 0]):
            index = np.nonzero(lab == root)[0]
            assert mm.quad_of_component(index, W) == quad_loops(index, W)
            checked += 1
    assert checked > 20


def test_fixture_id0_and_rotations():
    bits = mm.fixture_bits()
    assert len(bits) == 8
    assert ["".join(str(v) for v in row) for row in bits[0]] == ["10100", "01011", "01100", "10101", "11100"]
    assert WORDS[0] == int("1010001011011001010111100", 2)
    codes = {mm.rotate_code(w, k) for w in WORDS for k in range(4)}
    assert len(codes) == 32
    # rotate_code(., 1) four times is the identity, and twice is the half turn
    for w in WORDS:
        assert mm.rotate_code(mm.rotate_code(w, 1), 1) == mm.rotate_code(w, 2)
        assert mm.rotate_code(mm.rotate_code(w, 2), 2) == w
    # the package's dictionary type reads the same words from the same file
    d = MarkerDictionary.from_file(mm.FIXTURE)
    assert d.words.dtype == np.uint32 and d.words.tolist() == WORDS and len(d) == 8
    assert MarkerDictionary.from_bits(bits).words.tolist() == WORDS
    with pytest.raises(ValueError):
        MarkerDictionary.from_bits(np.zeros((2, 5, 4)))
    with pytest.raises(ValueError):
        MarkerDictionary([1 << 25])


def test_integer_sampling_against_float_homography():
    """Every sample pixel of a skewed quadrilateral is within one pixel of the float64 homography's point (the integer form rounds to
    the nearest pixel: half a pixel, plus the float solve's error)."""
    Q = [(103, 57), (391, 81), (352, 330), (88, 291)]
    src = np.array([(0, 0), (7, 0), (7, 7), (0, 7)], dtype=np.float64)
    A, b = [], []
    for (sx, sy), (dx, dy) in zip(src, Q):
        A.append([sx, sy, 1, 0, 0, 0, -dx * sx, -dx * sy]); b.append(dx)
        A.append([0, 0, 0, sx, sy, 1, -dy * sx, -dy * sy]); b.append(dy)
    h = np.append(np.linalg.solve(np.array(A), np.array(b, dtype=np.float64)), 1.0).reshape(3, 3)
    coef = mm.map_coefficients(Q)
    worst = 0.0
    for V in range(0, 29):
        for U in range(0, 29):
            x, y, w = h @ np.array([U / 4.0, V / 4.0, 1.0])
            px, py = mm.sample_pixel(coef, U, V)
            worst = max(worst, abs(px - x / w), abs(py - y / w))
    assert worst <= 1.0
    assert worst <= 0.5 + 1e-9
    # the square's corners go to the quadrilateral's, exactly
    assert [mm.sample_pixel(coef, U, V) for U, V in ((0, 0), (28, 0), (28, 28), (0, 28))] == Q


def test_half_pixel_rounding():
    """A 13-pixel span: the sample U = 14 falls on x0 + 6.5 exactly and goes up, floor(num/den + 1/2)."""
    coef = mm.map_coefficients([(40, 20), (53, 20), (53, 33), (40, 33)])
    assert mm.sample_pixel(coef, 14, 14) == (47, 27)
    coef = mm.map_coefficients([(-53, -33), (-40, -33), (-40, -20), (-53, -20)])   # negative numerators: floor, not truncation
    assert mm.sample_pixel(coef, 14, 14) == (-46, -26)


# ---- the images the GPU tests use hold what they were built to hold ----
def test_cases_decode_as_built():
    for id in range(8):
        ids, corners = mm.detect(mc.axis_aligned(id), WORDS)
        assert ids == [id] and corners[0].tolist() == [[30, 17], [57, 17], [57, 44], [30, 44]]
    ids, corners = mm.detect(mc.axis_aligned(0, cell=2, left=40, top=20), WORDS)
    assert ids == [0] and corners[0].tolist() == [[40, 20], [53, 20], [53, 33], [40, 33]]
    upright = [[30, 17], [57, 17], [57, 44], [30, 44]]
    for rot in (1, 2, 3):   # numpy.rot90 turns counter-clockwise: the marker's top-left corner goes to the image's bottom-left, ...
        ids, corners = mm.detect(mc.axis_aligned(0, rot=rot), WORDS)
        assert ids == [0] and corners[0].tolist() == [upright[(q - rot) % 4] for q in range(4)]
    assert mm.detect(mc.axis_aligned(0, mirror=True), WORDS)[0] == []
    for img, quad in ((mc.rotated30(), mc.square_quad(48.0, 48.0, 49.0, 30.0)), (mc.perspective(), mc.PERSPECTIVE_QUAD)):
        ids, corners = mm.detect(img, WORDS)
        assert ids == [0] and np.abs(corners[0] - np.array(quad)).max() <= 1.5
    ids, corners = mm.detect(mc.mixed_scene(), WORDS)
    assert ids == mc.MIXED_IDS
    assert corners[1].tolist() == [[230, 8], [271, 8], [271, 49], [230, 49]]   # the larger copy of id 3
    assert mm.detect(mc.payload_flipped(), WORDS)[0] == [] and mm.detect(mc.payload_flipped(), WORDS, max_bit_errors=1)[0] == [4]
    assert mm.detect(mc.border_whitened(), WORDS, max_border_errors=1)[0] == []
    assert mm.detect(mc.border_whitened(), WORDS, max_border_errors=2)[0] == [4]
    assert mm.detect(mc.border_whitened(n=3), WORDS)[0] == []


def test_torture_patterns_are_what_they_say():
    for H, W in mc.TORTURE_SIZES:
        count = {}
        for name, make in mc.TORTURE_PATTERNS.items():
            lab = mm.label_image(mm.dark_mask(make(H, W), **mc.TORTURE_PARAMS))
            count[name] = (int((lab >= 0).sum()), len(np.unique(lab[lab >= 0])))
        assert count['spiral'][1] == 1 and count['spiral'][0] > H * W // 5
        assert count['comb'][1] == 2
        assert count['checkerboard'][0] == count['checkerboard'][1] == (H * W + 1) // 2
        assert count['block'] == ((H - 2) * (W - 2), 1)
        assert count['all_dark'] == (0, 0) and count['all_light'] == (0, 0)
        assert count['joined_in_last_row'][1] == 1


def test_scene_decodes_through_both_models():
    """The chain the end-to-end GPU test relies on, without a GPU: the renderer's model draws each camera's tile of the marker scene,
    the detector's model finds the markers the camera sees, and corner q, taken to 3D through the depth image, is within the
    scene's bound (marker_scene.corner_bound, 40.3 mm) of the scene's corner q.  Measured: 6.3 mm at the worst corner."""
    view = default_view()
    world = ms.board()
    e = ms.corner_bound(view, 5)
    for k in range(3):
        rgb, depth, _index, _covered = rm.render_model(cs.camera_tile(world, k), view, 5)
        ids, corners = mm.detect(rgb, WORDS)
        assert set(ids) == cs.EXPECTED_VISIBLE[k]
        for id, c in zip(ids, corners):
            got = np.array([deproject(view, depth, uv) for uv in c])
            assert np.linalg.norm(got - cs.true_corners_in_camera(k, id), axis=1).max() <= e
    assert ms.corner_bound(view, 5) < 0.087   # (half a marker's side: a bound above it could not tell the corners apart)
    assert math.isfinite(ms.corner_bound(view, 5))
