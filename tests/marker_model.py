"""numpy model of cwipc_hip_detect_markers' contract (include/cwipc_util_amd/hip_ext.h, csrc/kernels_markers.hip), steps 1 to 8 in the
contract's order and in integers throughout.  Test infrastructure: the GPU tests compare ids, corners and labels with it for equality,
and test_marker_model.py compares it with plain loops on tiny images.

Also here: the drawing helpers the marker tests share (a marker as a 7 x 7 cell matrix, painted axis-aligned or through a homography)."""
import json
import os

import numpy as np
from scipy import ndimage

DEFAULTS = dict(window_half=40, threshold_offset=7, min_side=14, max_border_errors=2, max_bit_errors=0)
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "aruco_5x5_printed.json")


# ---------------------------------------------------------------------------------------------------------------------------------
# dictionary
# ---------------------------------------------------------------------------------------------------------------------------------
def word_of_bits(bits):
    """5 x 5 of 0/1 (1 = white) -> the payload word: bit 24 - (5*row + col)."""
    word = 0
    for r in range(5):
        for c in range(5):
            word |= (int(bits[r][c]) & 1) << (24 - (5 * r + c))
    return word


def bits_of_word(word):
    """word_of_bits' inverse: the 5 x 5 of 0/1 of a payload word (bits 25-31 are not looked at)."""
    return [[(int(word) >> (24 - (5 * r + c))) & 1 for c in range(5)] for r in range(5)]


def fixture_bits():
    with open(FIXTURE) as f:
        return json.load(f)


def fixture_words():
    return [word_of_bits(b) for b in fixture_bits()]


def rotate_code(code, k):
    """The code read with Q_k as the top-left corner, from the code read with Q_0 there."""
    out = 0
    for r in range(5):
        for c in range(5):
            i, j = ((r, c), (c, 4 - r), (4 - r, 4 - c), (4 - c, r))[k]
            out |= ((code >> (24 - (5 * i + j))) & 1) << (24 - (5 * r + c))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# steps 1 to 3
# ---------------------------------------------------------------------------------------------------------------------------------
def grey(rgb):
    v = rgb.astype(np.int64)
    return (77 * v[:, :, 0] + 150 * v[:, :, 1] + 29 * v[:, :, 2] + 128) >> 8


def dark_mask(rgb, window_half=40, threshold_offset=7):
    y = grey(rgb)
    H, W = y.shape
    sat = np.zeros((H + 1, W + 1), dtype=np.int64)
    sat[1:, 1:] = y.cumsum(axis=0).cumsum(axis=1)
    r = np.arange(H)[:, None]
    c = np.arange(W)[None, :]
    r0, r1 = np.maximum(r - window_half, 0), np.minimum(r + window_half, H - 1) + 1
    c0, c1 = np.maximum(c - window_half, 0), np.minimum(c + window_half, W - 1) + 1
    s = sat[r1, c1] - sat[r0, c1] - sat[r1, c0] + sat[r0, c0]
    n = (r1 - r0) * (c1 - c0)
    return y * n + threshold_offset * n < s


def label_image(dark):
    """int32[H, W]: per dark pixel the smallest linear index of its 4-connected component, -1 for a light pixel."""
    lab, count = ndimage.label(dark, structure=[[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    out = np.full(dark.shape, -1, dtype=np.int32)
    if count:
        flat = lab.reshape(-1)
        where = np.nonzero(flat)[0]
        smallest = np.full(count + 1, flat.size, dtype=np.int64)
        np.minimum.at(smallest, flat[where], where)
        out.reshape(-1)[where] = smallest[flat[where]]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# steps 5 to 7, per component
# ---------------------------------------------------------------------------------------------------------------------------------
def _arg_extreme(value, index):
    """The index with the largest value, among equals the smallest index."""
    best = value.max()
    return int(index[value == best].min())


ONE_SIDED = "no pixel on one side of AC"
NOT_CONVEX = "A, B, C, D is not strictly convex"


def quad_verdict(index, W):
    """index: the component's linear indices (any order).  (Q0..Q3 as (x, y) tuples, None), or (None, the reason step 5 rejects the
    component for: ONE_SIDED when k(B) > 0 > k(D) fails, NOT_CONVEX)."""
    index = np.asarray(index, dtype=np.int64)
    x, y = index % W, index // W
    p0 = int(index.min())
    a = _arg_extreme((x - p0 % W) ** 2 + (y - p0 // W) ** 2, index)
    ax, ay = a % W, a // W
    c = _arg_extreme((x - ax) ** 2 + (y - ay) ** 2, index)
    cx, cy = c % W, c // W
    k = (x - ax) * (cy - ay) - (y - ay) * (cx - ax)
    b, d = _arg_extreme(k, index), _arg_extreme(-k, index)
    if not (k.max() > 0 > k.min()):
        return None, ONE_SIDED
    P = [(int(i % W), int(i // W)) for i in (a, b, c, d)]
    cross = []
    shoelace = 0
    for q in range(4):
        (x0, y0), (x1, y1), (x2, y2) = P[q], P[(q + 1) % 4], P[(q + 2) % 4]
        cross.append((x1 - x0) * (y2 - y1) - (y1 - y0) * (x2 - x1))
        shoelace += x0 * y1 - x1 * y0
    if not (all(v > 0 for v in cross) or all(v < 0 for v in cross)):
        return None, NOT_CONVEX
    return (P if shoelace > 0 else [P[0], P[3], P[2], P[1]]), None


def quad_of_component(index, W):
    """Q0..Q3 as (x, y) tuples, or None."""
    return quad_verdict(index, W)[0]


def map_coefficients(Q):
    (x0, y0), (x1, y1), (x2, y2), (x3, y3) = [(int(x), int(y)) for x, y in Q]
    dx1, dx2, sx = x1 - x2, x3 - x2, x0 - x1 + x2 - x3
    dy1, dy2, sy = y1 - y2, y3 - y2, y0 - y1 + y2 - y3
    dn = dx1 * dy2 - dx2 * dy1
    g = sx * dy2 - dx2 * sy
    h = dx1 * sy - sx * dy1
    return ((x1 - x0) * dn + g * x1, (x3 - x0) * dn + h * x3, x0 * dn, (y1 - y0) * dn + g * y1, (y3 - y0) * dn + h * y3, y0 * dn, g, h, dn)


def sample_pixel(coef, U, V):
    """The pixel (x, y) of the sample (U/4, V/4) of the 7 x 7 square, or None when the denominator is 0.  Python ints: exact."""
    ax, bx, cx, ay, by, cy, g, h, dn = coef
    den = g * U + h * V + dn * 28
    nx, ny = ax * U + bx * V + cx * 28, ay * U + by * V + cy * 28
    if den < 0:
        den, nx, ny = -den, -nx, -ny
    if den == 0:
        return None
    return (2 * nx + den) // (2 * den), (2 * ny + den) // (2 * den)


def read_cells(dark, Q):
    """black[7][7] through the map onto Q."""
    H, W = dark.shape
    coef = map_coefficients(Q)
    black = [[False] * 7 for _ in range(7)]
    for i in range(7):
        for j in range(7):
            count = 0
            for b in (1, 2, 3):
                for a in (1, 2, 3):
                    p = sample_pixel(coef, 4 * j + a, 4 * i + b)
                    if p is not None and 0 <= p[0] < W and 0 <= p[1] < H and dark[p[1], p[0]]:
                        count += 1
            black[i][j] = count >= 5
    return black


def code_of_cells(black):
    """(the number of white border cells, the 25 inner cells as a code, white = 1)."""
    border_white = sum(1 for i in range(7) for j in range(7) if (i in (0, 6) or j in (0, 6)) and not black[i][j])
    return border_white, word_of_bits([[0 if black[i + 1][j + 1] else 1 for j in range(5)] for i in range(5)])


def search_words_loop(code, words, max_bit_errors=0):
    """(id, k) of the smallest Hamming distance between the code's four rotations and the words, ties to the smallest id, then the
    smallest k, or None when that distance is above max_bit_errors: one comparison after the other."""
    rot = [rotate_code(code, k) for k in range(4)]
    best = None
    for id, word in enumerate(words):
        for k in range(4):
            cand = (bin(rot[k] ^ (int(word) & 0x1FFFFFF)).count("1"), id, k)
            if best is None or cand < best:
                best = cand
    if best is None or best[0] > max_bit_errors:
        return None
    return best[1], best[2]


_POPCOUNT8 = np.array([bin(v).count("1") for v in range(256)], dtype=np.int64)


def masked_words(words):
    """The dictionary as search_words reads it: uint32[n], bits 25-31 cleared."""
    return (np.asarray([int(w) for w in words], dtype=np.uint64) & 0x1FFFFFF).astype(np.uint32)


def search_words(code, words, max_bit_errors=0):
    """search_words_loop in numpy: xor of every word with the four rotations, a popcount per byte, and the lexicographic minimum
    over (distance, id, k).  words: a sequence of ints, or what masked_words() made of one."""
    if not (isinstance(words, np.ndarray) and words.dtype == np.uint32):
        words = masked_words(words)
    if len(words) == 0:
        return None
    rot = np.array([rotate_code(code, k) for k in range(4)], dtype=np.uint32)
    x = np.ascontiguousarray(words[:, None] ^ rot[None, :])           # [id, k]
    dist = _POPCOUNT8[x.view(np.uint8)].reshape(len(words), 4, 4).sum(axis=2)
    id, k = np.nonzero(dist == dist.min())                            # row-major: ascending id, then ascending k
    if dist[id[0], k[0]] > max_bit_errors:
        return None
    return int(id[0]), int(k[0])


def decode_cells_loop(black, words, max_border_errors=2, max_bit_errors=0):
    """(id, k) or None, the dictionary searched by search_words_loop."""
    border_white, code = code_of_cells(black)
    if border_white > max_border_errors:
        return None
    return search_words_loop(code, words, max_bit_errors)


def decode_cells(black, words, max_border_errors=2, max_bit_errors=0):
    """(id, k) or None."""
    border_white, code = code_of_cells(black)
    if border_white > max_border_errors:
        return None
    return search_words(code, words, max_bit_errors)


# ---------------------------------------------------------------------------------------------------------------------------------
# the whole detector
# ---------------------------------------------------------------------------------------------------------------------------------
def candidates(rgb, words, **params):
    """Steps 1 to 7: per component that passes step 4, in the order of the labels, the tuple (label, area, Q, hit): Q = the
    quadrilateral Q0..Q3 of step 5 as (x, y) tuples, or None when step 5 rejects the component; hit = (id, k) of step 7, or None when
    there is no quadrilateral or step 7 rejects it."""
    p = dict(DEFAULTS)
    p.update(params)
    H, W = rgb.shape[:2]
    words = masked_words(words)
    dark = dark_mask(rgb, p['window_half'], p['threshold_offset'])
    lab = label_image(dark).reshape(-1)
    where = np.nonzero(lab >= 0)[0]
    order = np.argsort(lab[where], kind='stable')
    where = where[order]
    starts = np.nonzero(np.diff(lab[where], prepend=-1))[0]
    out = []
    if len(starts) == 0:
        return out
    # step 4 for all components at once (an image of noise has a hundred thousand): the bounding boxes of the runs of equal labels
    xs, ys = where % W, where // W
    x0, x1 = np.minimum.reduceat(xs, starts), np.maximum.reduceat(xs, starts)
    y0, y1 = np.minimum.reduceat(ys, starts), np.maximum.reduceat(ys, starts)
    passes = (x0 > 0) & (y0 > 0) & (x1 < W - 1) & (y1 < H - 1) & (x1 - x0 + 1 >= p['min_side']) & (y1 - y0 + 1 >= p['min_side'])
    ends = np.append(starts[1:], len(where))
    for s, e in zip(starts[passes].tolist(), ends[passes].tolist()):
        index = where[s:e]
        Q = quad_of_component(index, W)
        hit = None
        if Q is not None:
            hit = decode_cells(read_cells(dark, Q), words, p['max_border_errors'], p['max_bit_errors'])
        out.append((int(lab[index[0]]), len(index), Q, hit))
    return out


def detect(rgb, words, **params):
    """(ids: list of int, corners: int64[n, 4, 2] as (u, v)), sorted by id: step 8 on candidates()."""
    found = {}
    for label, area, Q, hit in candidates(rgb, words, **params):
        if hit is None:
            continue
        id, k = hit
        rank = (-area, label)   # largest area, then smallest label
        if id not in found or rank < found[id][0]:
            found[id] = (rank, [Q[(q + k) % 4] for q in range(4)])
    ids = sorted(found)
    return ids, np.array([found[i][1] for i in ids], dtype=np.int64).reshape(len(ids), 4, 2)


# ---------------------------------------------------------------------------------------------------------------------------------
# drawing
# ---------------------------------------------------------------------------------------------------------------------------------
def cells_of_bits(bits):
    """The marker as a 7 x 7 matrix, 1 = white: the payload inside the black border."""
    cells = np.zeros((7, 7), dtype=np.uint8)
    cells[1:6, 1:6] = np.asarray(bits, dtype=np.uint8)
    return cells


def paint_axis_aligned(img, cells, left, top, cell):
    """The marker's 7 x 7 cells, `cell` pixels each, with their top-left pixel at (left, top); white cells are left as they are."""
    for i in range(7):
        for j in range(7):
            if not cells[i][j]:
                img[top + i * cell: top + (i + 1) * cell, left + j * cell: left + (j + 1) * cell] = 0


def paint_warped(img, cells, quad):
    """The marker through the homography that takes the square (0,0), (7,0), (7,7), (0,7) onto quad (float (x, y) corners): every
    pixel whose centre falls into a black cell is painted black (float64; the model and the GPU both read the finished image)."""
    H, W = img.shape[:2]
    src = np.array([(0, 0), (7, 0), (7, 7), (0, 7)], dtype=np.float64)
    A = []
    for (sx, sy), (dx, dy) in zip(quad, src):   # image -> marker
        A.append([sx, sy, 1, 0, 0, 0, -dx * sx, -dx * sy, -dx])
        A.append([0, 0, 0, sx, sy, 1, -dy * sx, -dy * sy, -dy])
    h = np.linalg.svd(np.array(A, dtype=np.float64))[2][-1].reshape(3, 3)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    w = h[2, 0] * xs + h[2, 1] * ys + h[2, 2]
    u = (h[0, 0] * xs + h[0, 1] * ys + h[0, 2]) / w
    v = (h[1, 0] * xs + h[1, 1] * ys + h[1, 2]) / w
    inside = (u >= 0) & (u < 7) & (v >= 0) & (v < 7)
    ci = np.clip(np.floor(v).astype(np.int64), 0, 6)
    cj = np.clip(np.floor(u).astype(np.int64), 0, 6)
    black = inside & (np.asarray(cells)[ci, cj] == 0)
    img[black] = 0


def white(height, width):
    return np.full((height, width, 3), 255, dtype=np.uint8)
