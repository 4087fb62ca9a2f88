"""The images of the marker detector's tests (test infrastructure), built once and shared: test_marker_model.py checks on the CPU that the
model finds in them what they were built to hold, test_gpu_markers.py that the GPU finds what the model finds."""
import math

import numpy as np

import marker_model as mm

BITS = mm.fixture_bits()


def cells(id):
    return mm.cells_of_bits(BITS[id])


def axis_aligned(id, cell=4, left=30, top=17, size=(64, 96), rot=0, mirror=False):
    """One marker, its cells turned rot quarter turns (counter-clockwise, numpy.rot90) or mirrored left to right."""
    img = mm.white(*size)
    c = cells(id)
    if mirror:
        c = c[:, ::-1]
    mm.paint_axis_aligned(img, np.rot90(c, rot), left, top, cell)
    return img


def square_quad(cx, cy, side, degrees):
    """The corners of a square, top-left first and clockwise on screen, turned by `degrees` (clockwise on screen) about its centre."""
    t = math.radians(degrees)
    out = []
    for x, y in ((-0.5, -0.5), (0.5, -0.5), (0.5, 0.5), (-0.5, 0.5)):
        out.append((cx + side * (x * math.cos(t) - y * math.sin(t)), cy + side * (x * math.sin(t) + y * math.cos(t))))
    return out


def rotated30(id=0):
    img = mm.white(96, 96)
    mm.paint_warped(img, cells(id), square_quad(48.0, 48.0, 49.0, 30.0))
    return img


#: opposite sides 56 and 48.7 pixels long: a ratio of 1.15
PERSPECTIVE_QUAD = [(20.0, 20.0), (76.0, 20.0), (72.35, 70.0), (23.65, 70.0)]


def perspective(id=0):
    img = mm.white(96, 96)
    mm.paint_warped(img, cells(id), PERSPECTIVE_QUAD)
    return img


MIXED_IDS = [2, 3, 5, 7]


def mixed_scene():
    """320 x 200: markers 2 (axis-aligned), 5 (turned 30 degrees) and 7 (in perspective); id 3 twice, 6-pixel and 4-pixel cells; a solid
    black square; a ring with a payload that is in no dictionary (all white but one cell); marker 1 touching the left edge; marker 4
    with 1-pixel cells, below min_side; marker 6 mirrored."""
    img = mm.white(200, 320)
    mm.paint_axis_aligned(img, cells(2), 12, 10, 5)
    mm.paint_warped(img, cells(5), square_quad(100.0, 40.0, 45.0, 30.0))
    mm.paint_warped(img, cells(7), [(150.0, 12.0), (206.0, 16.0), (200.0, 66.0), (152.0, 60.0)])
    mm.paint_axis_aligned(img, cells(3), 230, 8, 6)
    mm.paint_axis_aligned(img, cells(3), 280, 60, 4)
    img[100:130, 20:50] = 0
    ring = np.ones((7, 7), dtype=np.uint8)
    ring[0, :] = ring[6, :] = ring[:, 0] = ring[:, 6] = 0
    ring[3, 3] = 0
    mm.paint_axis_aligned(img, ring, 70, 100, 5)
    mm.paint_axis_aligned(img, cells(1), 0, 150, 5)
    mm.paint_axis_aligned(img, cells(4), 130, 110, 1)
    mm.paint_axis_aligned(img, cells(6)[:, ::-1], 160, 120, 6)
    return img


# ---- labelling: black patterns on white; with a window wider than the image and no offset a black pixel is darker than its window's
# mean as soon as the image has a white pixel, and a white one never is: the mask is the pattern ----
TORTURE_PARAMS = dict(window_half=400, threshold_offset=0)
TORTURE_SIZES = [(64, 64), (97, 201), (130, 257)]


def _from_mask(mask):
    img = mm.white(*mask.shape)
    img[mask] = 0
    return img


def spiral(H, W):
    """A one-pixel line that winds inwards, two pixels between the turns: one component, a long chain of single links."""
    m = np.zeros((H, W), dtype=bool)
    r, c, dr, dc = 1, 1, 0, 1
    m[r, c] = True
    while True:
        for _attempt in range(2):
            nr, nc, ar, ac = r + dr, c + dc, r + 2 * dr, c + 2 * dc
            ahead_taken = 0 <= ar < H and 0 <= ac < W and m[ar, ac]
            if 1 <= nr <= H - 2 and 1 <= nc <= W - 2 and not m[nr, nc] and not ahead_taken:
                break
            dr, dc = dc, -dr   # turn right
        else:
            return _from_mask(m)
        r, c = nr, nc
        m[r, c] = True


def comb(H, W):
    """Teeth one pixel wide, one apart, hanging from a back in row 1; a second comb's teeth rise between them from a back in row H - 2
    without touching."""
    m = np.zeros((H, W), dtype=bool)
    m[1, 1:W - 1] = True
    m[1:H - 4, 1:W - 1:4] = True
    m[H - 2, 1:W - 1] = True
    m[4:H - 1, 3:W - 1:4] = True
    return _from_mask(m)


def checkerboard(H, W):
    m = np.zeros((H, W), dtype=bool)
    m[::2, ::2] = True
    m[1::2, 1::2] = True
    return _from_mask(m)


def block(H, W):
    """Everything but a one-pixel white frame: one component of (H - 2) (W - 2) pixels."""
    m = np.zeros((H, W), dtype=bool)
    m[1:H - 1, 1:W - 1] = True
    return _from_mask(m)


def all_dark(H, W):
    return np.zeros((H, W, 3), dtype=np.uint8)


def all_light(H, W):
    return mm.white(H, W)


def joined_in_last_row(H, W):
    """Two blobs, the left one of smaller indices, that meet only in the image's last row."""
    m = np.zeros((H, W), dtype=bool)
    m[2:H, 3:W // 2 - 1] = True
    m[5:H, W // 2 + 1:W - 2] = True
    m[H - 1, 3:W - 2] = True
    return _from_mask(m)


TORTURE_PATTERNS = dict(spiral=spiral, comb=comb, checkerboard=checkerboard, block=block, all_dark=all_dark, all_light=all_light,
                        joined_in_last_row=joined_in_last_row)


# ---- error tolerance ----
def payload_flipped(id=4):
    """Marker `id`, payload cell (2, 1) inverted."""
    c = cells(id).copy()
    c[3, 2] ^= 1
    img = mm.white(64, 96)
    mm.paint_axis_aligned(img, c, 30, 17, 4)
    return img


def border_whitened(id=4, n=2):
    """Marker `id` with n neighbouring cells of its top border white, from column 2 on: the ring stays in one piece."""
    c = cells(id).copy()
    c[0, 2:2 + n] = 1
    img = mm.white(64, 96)
    mm.paint_axis_aligned(img, c, 30, 17, 4)
    return img
