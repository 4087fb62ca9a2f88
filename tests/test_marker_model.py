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


# ---- the dictionary search: numpy against the loop ----
def test_vectorised_search_equals_the_loop():
    """mm.search_words (xor, popcount, lexicographic minimum) against mm.search_words_loop, on random codes, on every special word of
    the tie dictionaries in its four turns and on codes one and two bits from them, for every dictionary the GPU tests use."""
    rng = np.random.default_rng(21)
    codes = [int(v) for v in rng.integers(0, 1 << 25, 40)] + [0, (1 << 25) - 1]
    for w in mc.TIE_PAYLOADS.values():
        codes += [mm.rotate_code(w, k) for k in range(4)] + [w ^ 1, w ^ (1 << 24), w ^ 0b11, w ^ (0b101 << 11)]
    dictionaries = [WORDS, mc.GRID_WORDS, mc.GRID_WORDS[:64], mc.GRID_WORDS[:65]] + [mc.tie_dictionary(n) for n in mc.TIE_SIZES]
    codes += mc.GRID_WORDS[60:70] + [mm.rotate_code(w, 3) for w in mc.GRID_WORDS[1090:1100]]
    hits = 0
    for words in dictionaries:
        masked = mm.masked_words(words)
        assert masked.dtype == np.uint32 and int(masked.max()) < 1 << 25
        for code in codes:
            for errors in (0, 3, 25):
                want = mm.search_words_loop(code, words, errors)
                assert mm.search_words(code, words, errors) == want
                assert mm.search_words(code, masked, errors) == want
                hits += want is not None
                if errors == 25:
                    assert want is not None   # 25 bits: every code is within reach of some word
    assert hits > len(dictionaries) * len(codes)   # (not everything was a miss)
    # and through the cells: decode_cells is decode_cells_loop
    for img in (mc.axis_aligned(3), mc.payload_flipped(), mc.border_whitened(n=3), mc.shape_L()):
        dark = mm.dark_mask(img)
        for _label, _area, Q, _hit in mm.candidates(img, WORDS, min_side=10):
            if Q is not None:
                black = mm.read_cells(dark, Q)
                for kw in (dict(), dict(max_bit_errors=3), dict(max_border_errors=24, max_bit_errors=25)):
                    assert mm.decode_cells(black, WORDS, **kw) == mm.decode_cells_loop(black, WORDS, **kw)


def test_candidates_and_detect():
    """candidates() says what an image holds; detect() is its step 8."""
    got = mm.candidates(mc.mixed_scene(), WORDS)
    assert [c[0] for c in got] == sorted(c[0] for c in got) and len(got) >= 7
    by_id = {}
    for label, area, Q, hit in got:
        assert Q is None or len(Q) == 4
        if hit is not None:
            by_id.setdefault(hit[0], []).append((area, label))
    assert sorted(by_id) == mc.MIXED_IDS and len(by_id[3]) == 2
    assert sum(1 for c in got if c[2] is not None and c[3] is None) >= 2   # the solid square and the ring read, and are no marker
    ids, corners = mm.detect(mc.mixed_scene(), WORDS)
    big = max(by_id[3])
    assert corners[1].tolist()[0] == [230, 8] and big[1] == 8 * 320 + 230
    # a component that touches the edge, and one below min_side, are no candidates: marker 1 at x = 0 and the 7-pixel marker 4
    labels = {c[0] for c in got}
    assert 150 * 320 + 0 not in labels and 110 * 320 + 130 not in labels


# ---- the grid of markers ----
def test_marker_grid_holds_every_id():
    assert len(set(mc.GRID_WORDS)) == 1100 and all(0 <= w < 1 << 25 for w in mc.GRID_WORDS)
    assert len({mm.rotate_code(w, k) for w in mc.GRID_WORDS for k in range(4)}) == 4400
    img = mc.grid_image()
    assert img.shape == (530, 530, 3)
    ids, corners = mm.detect(img, mc.GRID_WORDS)
    assert ids == list(range(1089)) and len(ids) > 1024   # more candidates than the decode kernel has waves
    for n in (0, 1, 2, 3, 33, 1088):
        assert corners[n].tolist() == mc.grid_corners(n, **mc.GRID)
    assert corners.tolist() == [mc.grid_corners(n, **mc.GRID) for n in range(1089)]
    assert corners[5].tolist() == [[82, 15], [82, 2], [95, 2], [95, 15]]   # one quarter turn: the marker's top-left is at the bottom left
    # against the first 64 and 65 words: exactly those ids
    assert mm.detect(img, mc.GRID_WORDS[:64])[0] == list(range(64))
    assert mm.detect(img, mc.GRID_WORDS[:65])[0] == list(range(65))


# ---- tie dictionaries ----
def test_tie_dictionaries_are_what_they_say():
    """The bit patterns, their symmetries, the duplicate's lanes, the equidistant pairs; and what the model reports for a marker
    painted from each special word, written out."""
    assert mc.QUARTER_BITS == ["11001", "00001", "00100", "10000", "10011"] and mc.QUARTER == 0b1100100001001001000010011
    assert mc.HALF_BITS == ["11000", "00100", "01110", "00100", "00011"] and mc.HALF == 0b1100000100011100010000011
    assert [mm.rotate_code(mc.QUARTER, k) for k in range(4)] == [mc.QUARTER] * 4
    assert mm.rotate_code(mc.HALF, 2) == mc.HALF and mm.rotate_code(mc.HALF, 1) != mc.HALF
    assert mm.rotate_code(mc.HALF, 1) == mm.rotate_code(mc.HALF, 3)
    for n in mc.TIE_SIZES:
        words = mc.tie_dictionary(n)
        assert len(words) == n and words == mc.tie_dictionary(n)
        assert all(words[id] == w for id, w in mc.TIE_PLACES.items() if id < n)
        if n > 1:
            assert any(w >> 25 for w in words)
    words = mc.tie_dictionary(1000)
    masked = mm.masked_words(words).tolist()
    assert [id for id, w in enumerate(masked) if w == WORDS[0]] == [3, 67, 70] and 3 % 64 == 67 % 64 != 70 % 64
    assert [id for id, w in enumerate(masked) if w == mc.QUARTER] == [0, 64] and [id for id, w in enumerate(masked) if w == mc.HALF] == [1, 129]
    assert words[2] >> 25 == 0x7F and words[64] >> 25 and words[70] >> 25 and masked[2] == WORDS[2]
    assert masked[5] == mm.rotate_code(masked[60], 1) and masked[6] == mm.rotate_code(masked[900], 3)
    popcount = lambda v: bin(v).count("1")   # noqa: E731
    assert popcount(WORDS[6] ^ masked[10]) == popcount(WORDS[6] ^ masked[20]) == 1 and 10 % 64 != 20 % 64
    assert [popcount(WORDS[7] ^ masked[id]) for id in (12, 22, 72)] == [2, 2, 2] and len({12 % 64, 22 % 64, 72 % 64}) == 3
    for payload in (WORDS[6], WORDS[7]):   # in no dictionary, in no turn
        assert all(mm.rotate_code(payload, k) not in masked for k in range(4))
    # the equidistant words are the nearest: no other word comes as near in any turn
    near6 = sorted((popcount(mm.rotate_code(WORDS[6], k) ^ w), id) for id, w in enumerate(masked) for k in range(4))[:3]
    assert near6[:2] == [(1, 10), (1, 20)] and near6[2][0] > 2
    near7 = sorted((popcount(mm.rotate_code(WORDS[7], k) ^ w), id) for id, w in enumerate(masked) for k in range(4))[:4]
    assert near7[:3] == [(2, 12), (2, 22), (2, 72)] and near7[3][0] > 2


def test_tie_markers_decode_as_written():
    assert sorted(mc.TIE_EXPECTED) == sorted(mc.TIE_PAYLOADS)
    for n in mc.TIE_SIZES:
        words = mc.tie_dictionary(n)
        for name, payload in mc.TIE_PAYLOADS.items():
            for rot in range(4):
                img = mc.painted_word(payload, rot)
                for errors in (0, 1, 2):
                    ids, corners = mm.detect(img, words, max_bit_errors=errors)
                    want = mc.tie_expected(name, n, rot, errors)
                    if want is None:
                        assert ids == []
                    else:
                        assert ids == [want[0]] and corners[0][0].tolist() == want[1]
                        assert sorted(corners[0].tolist()) == sorted(mc.UPRIGHT)


# ---- shapes ----
def tie_counts_loops(index, W):
    """How many of the component's pixels have the extreme value, for A, C, B and D in turn (plain loops; A and C chosen by quad_loops'
    rule, the smallest index among equals)."""
    index = sorted(int(i) for i in index)

    def farthest(fx, fy):
        best, arg, count = -1, None, 0
        for i in index:
            d = (i % W - fx) ** 2 + (i // W - fy) ** 2
            if d > best:
                best, arg, count = d, i, 1
            elif d == best:
                count += 1
        return arg, count
    a, na = farthest(index[0] % W, index[0] // W)
    c, nc = farthest(a % W, a // W)
    ks = [(i % W - a % W) * (c // W - a // W) - (i // W - a // W) * (c % W - a % W) for i in index]
    return na, nc, ks.count(max(ks)), ks.count(min(ks))


def test_shapes_tie_and_reject_as_stated():
    """Each of A, C, B and D is tied in some shape that still yields a quadrilateral, every accepted shape decodes to some id under
    SHAPE_PARAMS, and every rejected shape is rejected for its stated reason.

    No shape here is rejected as 'not strictly convex', and none can be: with B and D strictly on opposite sides of the line AC the
    cycle A, B, C, D fails to be strictly convex only if A or C lies in the triangle of the other three.  C cannot: seen from A,
    |C| >= |B|, |D| and a proper convex combination of B and D is shorter than the longer of them unless both lie on AC.  A cannot:
    with P0 as the origin of distances, P0.(X - A) >= |X - A|^2 / 2 > 0 for X = B, C, D (none is farther from P0 than A), so no
    combination of B - A, C - A, D - A with non-negative weights is zero.  The non-convex dart is therefore rejected one rule earlier."""
    words = mc.tie_dictionary(1000)
    tied = dict(A=[], C=[], B=[], D=[])
    for name, make in mc.SHAPES.items():
        img = make()
        assert 48 <= img.shape[0] <= 64 and 48 <= img.shape[1] <= 64
        lab = mm.label_image(mm.dark_mask(img)).reshape(-1)
        index = np.nonzero(lab >= 0)[0]
        assert len(np.unique(lab[index])) == 1                     # a single component
        got = mm.candidates(img, words, **mc.SHAPE_PARAMS)
        assert len(got) == 1
        label, area, Q, hit = got[0]
        assert area == len(index) and Q is not None and Q == quad_loops(index, img.shape[1]) and hit is not None
        assert mm.detect(img, words, **mc.SHAPE_PARAMS)[0] == [hit[0]]
        for corner, count in zip("ACBD", tie_counts_loops(index, img.shape[1])):
            if count > 1:
                tied[corner].append(name)
    assert "square_without_last" in tied["A"] and "square_without_first" in tied["C"] and "L" in tied["D"]
    assert all(tied[corner] for corner in "ACBD"), tied
    assert {"square_cut_top_right", "square_cut_bottom_left"} <= set(tied["B"] + tied["D"])
    for name, (make, reason) in mc.REJECTED_SHAPES.items():
        img = make()
        lab = mm.label_image(mm.dark_mask(img)).reshape(-1)
        index = np.nonzero(lab >= 0)[0]
        assert len(np.unique(lab[index])) == 1 and len(index) > 30
        got = mm.candidates(img, words, **mc.SHAPE_PARAMS)
        if reason == 'step 4':
            assert got == []
        else:
            assert len(got) == 1 and got[0][2] is None and got[0][3] is None
            assert mm.quad_verdict(index, img.shape[1]) == (None, reason) and quad_loops(index, img.shape[1]) is None
        assert mm.detect(img, words, **mc.SHAPE_PARAMS)[0] == []
    # the sheet holds them all: as many candidates, the same quadrilaterals moved to their tiles
    sheet = mc.shape_sheet()
    got = mm.candidates(sheet, words, **mc.SHAPE_PARAMS)
    assert sum(1 for c in got if c[2] is not None) == len(mc.SHAPES)
    assert sum(1 for c in got if c[2] is None) == sum(1 for _m, reason in mc.REJECTED_SHAPES.values() if reason != 'step 4')


# ---- noise ----
def test_noise_is_what_it_says():
    for density in mc.NOISE_DENSITIES:
        img = mc.binary_noise(130, 257, density)
        assert set(np.unique(img)) == {0, 255} and (img[:, :, 0] == img[:, :, 1]).all()
        dark = mm.dark_mask(img)
        assert np.array_equal(dark, img[:, :, 0] == 0)             # the mask is the noise
        assert abs(dark.mean() - density) < 0.01
    sizes = {}
    for density in mc.NOISE_DENSITIES:
        lab = mm.label_image(mm.dark_mask(mc.binary_noise(600, 1024, density)))
        sizes[density] = np.bincount(lab[lab >= 0]).max() / (600 * 1024)
    # small clusters below the threshold, one that spans most of the image above it, large ragged ones at it
    assert sizes[0.30] < 0.001 and sizes[0.80] > 0.75 and 0.01 < sizes[0.59] < 0.5, sizes
    grey = mc.grey_noise(130, 257)
    assert grey.dtype == np.uint8 and grey.min() == 0 and grey.max() == 255
    assert abs(np.corrcoef(grey[:, :, 0].reshape(-1), grey[:, :, 1].reshape(-1))[0, 1]) < 0.02
    ramp = mc.ramp_noise(130, 257)
    assert ramp.dtype == np.uint8 and ramp[:8, :8].mean() < 50 and ramp[-8:, -8:].mean() > 200 and ramp.max() <= 254
    for img in (grey, ramp):   # a mask that depends on the window and on the offset, and is empty at offset 255
        masks = [mm.dark_mask(img, w, 7) for w in (1, 3, 40)]
        assert not np.array_equal(masks[0], masks[1]) and not np.array_equal(masks[1], masks[2])
        assert 0.1 < masks[2].mean() < 0.6
        assert mm.dark_mask(img, 40, 0).sum() > masks[2].sum() and not mm.dark_mask(img, 40, 255).any()


# ---- images larger than one trip ----
def test_large_images_hold_what_they_say():
    H, W = mc.TWO_TRIPS
    assert H * W > 524288 and 512 * W == 524288
    got = {hit[0]: (label, area, Q) for label, area, Q, hit in mm.candidates(mc.two_trip_scene(), WORDS) if hit is not None}
    assert sorted(got) == mc.TWO_TRIPS_IDS == mm.detect(mc.two_trip_scene(), WORDS)[0]
    rows = {id: sorted(y for _x, y in Q) for id, (_label, _area, Q) in got.items()}
    assert rows[3][3] < 512                                        # wholly in the first trip
    assert rows[0][0] == 500 and rows[0][3] == 527                 # across the boundary
    assert got[2][0] == 511 * W + 600 and rows[2][3] == 545        # the label's pixel before it, 34 of 35 rows past it
    assert rows[1][0] == 540                                       # wholly past it
    assert rows[5][0] < 512 < rows[5][3]
    tall, wide = mc.tall_image(), mc.wide_image()
    assert tall.shape == (4200, 20, 3) and wide.shape == (20, 8192, 3)
    ids, corners = mm.detect(tall, WORDS)
    assert ids == mc.TALL_IDS and corners[0].tolist() == [[3, 5], [16, 5], [16, 18], [3, 18]] and corners[1][0].tolist() == [3, 4120]
    ids, corners = mm.detect(wide, WORDS)
    assert ids == mc.WIDE_IDS and [c[0].tolist() for c in corners] == [[3, 3], [4100, 3], [8175, 3]]
    assert [c[0][0] // 256 for c in corners.tolist()] == [0, 16, 31] and corners[2][1].tolist() == [8188, 3]
    for name, quad in mc.SHAPE_QUADS.items():
        ids, corners = mm.detect(mc.SHAPES[name](), mc.tie_dictionary(1000), **mc.SHAPE_PARAMS)
        assert len(ids) == 1 and corners[0].tolist() == quad


def test_each_border_cell_counts_once():
    assert len(mc.BORDER_CELLS) == 20
    for i, j in mc.BORDER_CELLS:
        img = mc.border_cell_whitened(i, j)
        (_label, _area, Q, hit), = [c for c in mm.candidates(img, WORDS, max_border_errors=1) if c[2] is not None]
        black = mm.read_cells(mm.dark_mask(img), Q)
        assert mm.code_of_cells(black)[0] == 1 and hit is not None and hit[0] == 4
        assert mm.detect(img, WORDS, max_border_errors=0)[0] == [] and mm.detect(img, WORDS, max_border_errors=1)[0] == [4]
    # a shape whose own border count is neither 0 nor 24: test_shape puts max_border_errors at it and one below
    assert mc.white_border_cells(mc.shape_plus()) == 8 and mc.white_border_cells(mc.shape_L()) == 5 and mc.white_border_cells(mc.shape_disc()) == 0


def test_area_rule_scene():
    img = mc.area_rule_scene()
    got = [c for c in mm.candidates(img, WORDS) if c[3] is not None]
    by_id = {id: sorted((area, label) for label, area, _Q, hit in got if hit[0] == id) for id in (3, 5)}
    assert len(got) == 4 and len(by_id[3]) == len(by_id[5]) == 2
    assert by_id[3][0][0] == by_id[3][1][0] and by_id[3][0][1] == 5 * 256 + 130          # equal areas: the smaller label
    assert by_id[5][1][1] == 80 * 256 + 130 and by_id[5][0][0] < by_id[5][1][0] < 2 * by_id[5][0][0]   # less than twice the smaller
    ids, corners = mm.detect(img, WORDS)
    assert ids == [3, 5] and corners[0][0].tolist() == [130, 5] and corners[1][0].tolist() == [130, 80]
    # the second of each pair shares every one of its rows' 64-pixel spans with the square beside it (the first shares its spans
    # with nothing but its own loose payload cells)
    lab = mm.label_image(mm.dark_mask(img))
    assert all(len(np.unique(lab[r, 0:64][lab[r, 0:64] >= 0])) >= 2 for r in list(range(50, 78)) + list(range(85, 113)))
