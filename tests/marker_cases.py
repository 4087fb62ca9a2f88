"""The images of the marker detector's tests (test infrastructure), built once and shared: test_marker_model.py checks on the CPU that the
model finds in them what they were built to hold, test_gpu_markers.py and test_gpu_markers_edges.py that the GPU finds what the model
finds."""
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


# ---- many markers, many words: more candidates than the decode kernel has waves, more words than a wave has lanes ----
def random_words(n, seed):
    """n distinct 25-bit words from a seeded generator."""
    rng = np.random.default_rng(seed)
    words = []
    while len(words) < n:
        w = int(rng.integers(0, 1 << 25))
        if w not in words:
            words.append(w)
    return words


def cells_of_word(word):
    return mm.cells_of_bits(mm.bits_of_word(word))


def marker_grid_image(words, grid, cell, pitch, margin=2):
    """grid x grid markers: marker n of `words` in grid position n (row n // grid, column n % grid), turned n % 4 quarter turns
    (numpy.rot90), axis-aligned with `cell`-pixel cells, its top-left pixel at (margin + column*pitch, margin + row*pitch)."""
    side = margin + grid * pitch
    img = mm.white(side, side)
    for n in range(grid * grid):
        mm.paint_axis_aligned(img, np.rot90(cells_of_word(words[n]), n % 4), margin + (n % grid) * pitch, margin + (n // grid) * pitch, cell)
    return img


def grid_corners(n, grid, cell, pitch, margin=2):
    """The corners marker n of marker_grid_image reports: its own top-left first, wherever the turn put it."""
    left, top, span = margin + (n % grid) * pitch, margin + (n // grid) * pitch, 7 * cell - 1
    upright = [[left, top], [left + span, top], [left + span, top + span], [left, top + span]]
    return [upright[(q - n % 4) % 4] for q in range(4)]


#: the concrete case: 33 x 33 markers of 2-pixel cells at pitch 16 on 530 x 530, the first 1089 of 1100 words
GRID = dict(grid=33, cell=2, pitch=16)
GRID_WORDS = random_words(1100, 11)


def grid_image():
    return marker_grid_image(GRID_WORDS, **GRID)


# ---- tie dictionaries ----
FIX = mm.fixture_words()
#: invariant under a quarter turn                     invariant under a half turn, not under a quarter turn
QUARTER_BITS = ["11001", "00001", "00100", "10000", "10011"]
HALF_BITS = ["11000", "00100", "01110", "00100", "00011"]
QUARTER = mm.word_of_bits([[int(v) for v in row] for row in QUARTER_BITS])
HALF = mm.word_of_bits([[int(v) for v in row] for row in HALF_BITS])
TIE_SIZES = [1, 63, 64, 65, 130, 1000]
#: id -> word; an id at or past the dictionary's size is left out.  Lanes: id % 64.
TIE_PLACES = {
    0: QUARTER,
    1: HALF,
    2: FIX[2] | 0xFE000000,            # bits 25-31 set: not looked at
    3: FIX[0],                         # the duplicate: again at 67 (the same lane) and at 70 (another lane)
    4: FIX[1],
    5: mm.rotate_code(FIX[5], 1),      # a quarter turn of the word at 60
    6: mm.rotate_code(FIX[3], 3),      # three quarter turns of the word at 900
    10: FIX[6] ^ (1 << 24),            # FIX[6] is one bit from 10 and from 20, and in no dictionary
    20: FIX[6] ^ 1,
    12: FIX[7] ^ 0b11,                 # FIX[7] is two bits from 12, 22 and 72 (lanes 12, 22, 8), and in no dictionary
    22: FIX[7] ^ (0b11 << 23),
    60: FIX[5],
    64: QUARTER | 0x80000000,          # lane 0's second word, the only word of a second step when there are 65
    67: FIX[0],
    70: FIX[0] | 0x02000000,
    72: FIX[7] ^ (0b11 << 10),
    129: HALF,
    900: FIX[3],
}
#: what the tie tests paint: name -> payload
TIE_PAYLOADS = dict(quarter=QUARTER, half=HALF, high_bits=FIX[2], duplicate=FIX[0], plain=FIX[1], rotated=FIX[5], rotated_far=FIX[3],
                    one_off=FIX[6], two_off=FIX[7])


def tie_dictionary(n):
    """n words: TIE_PLACES where they fit, seeded random words elsewhere, every seventh of those with random bits above bit 24."""
    rng = np.random.default_rng(1000 + n)
    words = []
    for id in range(n):
        w = int(rng.integers(0, 1 << 25))
        if id % 7 == 0:
            w |= int(rng.integers(1, 128)) << 25
        words.append(TIE_PLACES.get(id, w))
    return words


def painted_word(word, rot=0):
    """axis_aligned() for a payload word instead of a fixture id: 4-pixel cells at (30, 17) on 96 x 64."""
    img = mm.white(64, 96)
    mm.paint_axis_aligned(img, np.rot90(cells_of_word(word), rot), 30, 17, 4)
    return img


#: the corners of a marker painted by mc.painted_word, in the image: top-left, top-right, bottom-right, bottom-left
UPRIGHT = [[30, 17], [57, 17], [57, 44], [30, 44]]
#: name -> (id, the first corner reported for the marker painted with 0, 1, 2, 3 quarter turns (numpy.rot90: counter-clockwise),
#: the least max_bit_errors at which it is found), in every tie dictionary of more than 60 words.
#: duplicate: the smallest of ids 3, 67, 70.  rotated: the word is at id 60 and its quarter turn at id 5; the smaller id wins, and
#: marker 5's top-left corner is the painted marker's top-right.  rotated_far: id 6 holds three quarter turns of the word at 900:
#: its top-left corner is the painted marker's bottom-left.  quarter: all four k tie, k = 0 wins, and Q0 is A, the pixel farthest
#: from the label's pixel (30, 17): the bottom-right corner whatever the turn.  half: k and k + 2 tie, the smaller wins: Q0 = (57, 44)
#: when the marker's top-left corner is at Q0 or Q2 (turns 0 and 2), Q1 = (30, 44) when it is at Q1 or Q3.
TIE_EXPECTED = dict(
    quarter=(0, [[57, 44], [57, 44], [57, 44], [57, 44]], 0),
    half=(1, [[57, 44], [30, 44], [57, 44], [30, 44]], 0),
    high_bits=(2, [[30, 17], [30, 44], [57, 44], [57, 17]], 0),
    duplicate=(3, [[30, 17], [30, 44], [57, 44], [57, 17]], 0),
    plain=(4, [[30, 17], [30, 44], [57, 44], [57, 17]], 0),
    rotated=(5, [[57, 17], [30, 17], [30, 44], [57, 44]], 0),
    rotated_far=(6, [[30, 44], [57, 44], [57, 17], [30, 17]], 0),
    one_off=(10, [[30, 17], [30, 44], [57, 44], [57, 17]], 1),
    two_off=(12, [[30, 17], [30, 44], [57, 44], [57, 17]], 2))


def tie_expected(name, n, rot, max_bit_errors):
    """(id, first corner) or None: TIE_EXPECTED for a dictionary of n words (the one-word dictionary holds QUARTER alone)."""
    id, first, least = TIE_EXPECTED[name]
    if id >= n or max_bit_errors < least:
        return None
    return id, first[rot]


# ---- single dark components for the corner search: ties for A, C, B, D and the rejections of step 5 ----
def _blank(H=56, W=60):
    return np.zeros((H, W), dtype=bool)


def _polygon(m, pts):
    """Every pixel whose centre is inside or on the convex polygon pts ((x, y), clockwise on screen), by integer cross products."""
    ys, xs = np.mgrid[0:m.shape[0], 0:m.shape[1]]
    inside = np.ones(m.shape, dtype=bool)
    for (x0, y0), (x1, y1) in zip(pts, pts[1:] + pts[:1]):
        inside &= (x1 - x0) * (ys - y0) - (y1 - y0) * (xs - x0) >= 0
    m |= inside
    return m


def shape_square_without_last():
    m = _blank()
    m[10:41, 12:43] = True
    m[40, 42] = False
    return _from_mask(m)


def shape_square_without_first():
    m = _blank()
    m[10:41, 12:43] = True
    m[10, 12] = False
    return _from_mask(m)


def _staircase_cut(m, corner):
    """Three pixels of a corner of the square [10, 40] x [12, 42] taken out along the anti-diagonal, leaving a 3-pixel staircase."""
    if corner == 'top_right':
        m[10, 41:43] = False
        m[11, 42] = False
    else:
        m[40, 12:14] = False
        m[39, 12] = False
    return m


def shape_square_cut_top_right():
    m = _blank()
    m[10:41, 12:43] = True
    return _from_mask(_staircase_cut(m, 'top_right'))


def shape_square_cut_bottom_left():
    m = _blank()
    m[10:41, 12:43] = True
    return _from_mask(_staircase_cut(m, 'bottom_left'))


def shape_L():
    m = _blank()
    m[8:44, 10:24] = True
    m[30:44, 10:46] = True
    return _from_mask(m)


def shape_disc():
    m = _blank()
    ys, xs = np.mgrid[0:m.shape[0], 0:m.shape[1]]
    return _from_mask((xs - 30) ** 2 + (ys - 28) ** 2 <= 18 ** 2)


def shape_octagon():
    return _from_mask(_polygon(_blank(), [(22, 10), (38, 10), (48, 20), (48, 36), (38, 46), (22, 46), (12, 36), (12, 20)]))


def shape_diamond_odd():
    """|x - 30| + |y - 28| <= 17: a pixel at each tip."""
    ys, xs = np.mgrid[0:56, 0:60]
    return _from_mask(np.abs(xs - 30) + np.abs(ys - 28) <= 17)


def shape_diamond_even():
    """The centre between four pixels: two pixels at each tip."""
    ys, xs = np.mgrid[0:56, 0:60]
    return _from_mask(np.abs(2 * xs - 59) + np.abs(2 * ys - 55) <= 34)


def shape_plus():
    m = _blank()
    m[8:46, 22:36] = True
    m[20:34, 10:48] = True
    return _from_mask(m)


def shape_parallelogram():
    return _from_mask(_polygon(_blank(), [(20, 12), (50, 12), (40, 42), (10, 42)]))


def shape_rectangle():
    """10 wide, 35 high: below min_side = 14 across, a candidate with min_side = 10."""
    m = _blank()
    m[10:45, 25:35] = True
    return _from_mask(m)


def shape_line_horizontal():
    m = _blank()
    m[20, 10:50] = True
    return _from_mask(m)


def shape_line_vertical():
    m = _blank()
    m[8:48, 30] = True
    return _from_mask(m)


def shape_line_down_right():
    """A one-pixel staircase, 4-connected, from (10, 8) to (45, 43): the pixels (10 + i, 8 + i) lie on the diagonal AC, the steps
    (11 + i, 8 + i) between them all on one side of it."""
    m = _blank()
    for i in range(36):
        m[8 + i, 10 + i] = True
        if i < 35:
            m[8 + i, 11 + i] = True
    return _from_mask(m)


def shape_line_down_left():
    """The same from (49, 8) to (14, 43)."""
    m = _blank()
    for i in range(36):
        m[8 + i, 49 - i] = True
        if i > 0:
            m[8 + i, 50 - i] = True
    return _from_mask(m)


def shape_right_triangle():
    ys, xs = np.mgrid[0:56, 0:60]
    return _from_mask((xs >= 10) & (ys >= 8) & (xs - 10 + ys - 8 <= 36))


def shape_dart():
    """An arrowhead pointing up with a deep notch in its base, a non-convex outline: A and C are the two barbs, and the tip, the notch
    and everything else lie on one side of the line between them."""
    ys, xs = np.mgrid[0:56, 0:60]
    body = (np.abs(xs - 30) * 2 <= ys - 6) & (ys <= 46)
    notch = (np.abs(xs - 30) * 2 <= ys - 26) & (ys <= 46)
    return _from_mask(body & ~notch)


#: shapes that yield a quadrilateral (shape_rectangle with min_side = 10)
SHAPES = dict(square_without_last=shape_square_without_last, square_without_first=shape_square_without_first,
              square_cut_top_right=shape_square_cut_top_right, square_cut_bottom_left=shape_square_cut_bottom_left, L=shape_L, disc=shape_disc,
              octagon=shape_octagon, diamond_odd=shape_diamond_odd, diamond_even=shape_diamond_even, plus=shape_plus,
              parallelogram=shape_parallelogram, rectangle=shape_rectangle)
#: every candidate with a quadrilateral decodes to some id; min_side lets the 10 x 35 rectangle in
SHAPE_PARAMS = dict(max_border_errors=24, max_bit_errors=25, min_side=10)
#: Q0..Q3 of the shapes built for a tie, the tied corner marked: the smallest linear index of the tied pixels.  Solid shapes read
#: as the code 0, which no turn changes, so k = 0 and these are the corners that come out, in this order.
SHAPE_QUADS = dict(
    square_without_last=[[42, 39], [12, 40], [12, 10], [42, 10]],     # A: (42, 39) before (41, 40)
    square_without_first=[[42, 40], [12, 40], [13, 10], [42, 10]],    # C: (13, 10) before (12, 11)
    square_cut_top_right=[[42, 40], [12, 40], [12, 10], [40, 10]],    # D: (40, 10) before (41, 11) and (42, 12)
    square_cut_bottom_left=[[42, 40], [12, 38], [12, 10], [42, 10]],  # B: (12, 38) before (13, 39) and (14, 40)
    L=[[45, 43], [10, 43], [10, 8], [23, 8]])                         # D: (23, 8) before (45, 30)
def white_border_cells(img):
    """How many of the 24 border cells of a one-shape image's only candidate read white (step 7 compares this with max_border_errors)."""
    (_label, _area, Q, _hit), = mm.candidates(img, FIX, **SHAPE_PARAMS)
    return mm.code_of_cells(mm.read_cells(mm.dark_mask(img), Q))[0]


#: shapes that yield none, with the reason: 'step 4' (never a candidate), or what mm.quad_verdict says
REJECTED_SHAPES = dict(line_horizontal=(shape_line_horizontal, 'step 4'), line_vertical=(shape_line_vertical, 'step 4'),
                       line_down_right=(shape_line_down_right, mm.ONE_SIDED), line_down_left=(shape_line_down_left, mm.ONE_SIDED),
                       right_triangle=(shape_right_triangle, mm.ONE_SIDED), dart=(shape_dart, mm.ONE_SIDED))


def shape_sheet():
    """Every shape, accepted and rejected, on one white image, 4 in a row."""
    tiles = [make() for make in SHAPES.values()] + [make() for make, _reason in REJECTED_SHAPES.values()]
    while len(tiles) % 4:
        tiles.append(mm.white(56, 60))
    return np.concatenate([np.concatenate(tiles[r:r + 4], axis=1) for r in range(0, len(tiles), 4)], axis=0)


# ---- noise ----
def binary_noise(H, W, density, seed=5):
    """Independent pixels, black with probability `density`, else white."""
    return _from_mask(np.random.default_rng(seed).random((H, W)) < density)


NOISE_DENSITIES = [0.30, 0.59, 0.80]   # below, at and above the site percolation threshold of the square lattice (0.593)


def grey_noise(H, W, seed=6):
    """The three channels independent and uniform over 0..255."""
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def ramp_noise(H, W, seed=7):
    """Grey noise of amplitude 64 on a smooth ramp from dark (top left) to bright (bottom right), the channels independent."""
    ys, xs = np.mgrid[0:H, 0:W]
    ramp = (190 * (xs * (H - 1) + ys * (W - 1))) // max(2 * (H - 1) * (W - 1), 1)
    return (ramp[:, :, None] + np.random.default_rng(seed).integers(0, 65, (H, W, 3))).astype(np.uint8)


# ---- images larger than one trip of the kernels' loops (DESIGN.md 3.15 names the constants these are sized against) ----
TWO_TRIPS = (600, 1024)   # rows from 512 on lie past the first 524288 pixels
TWO_TRIPS_IDS = [0, 1, 2, 3, 5]


def two_trip_scene():
    """1024 x 600: marker 3 wholly in the first 512 rows; marker 0 across row 512 (rows 500 to 527); marker 2 with its first row, and
    so its label's pixel, in row 511 and the other 34 rows past it; marker 1 wholly past it; marker 5 turned 30 degrees across it."""
    img = mm.white(*TWO_TRIPS)
    mm.paint_axis_aligned(img, cells(3), 40, 100, 6)
    mm.paint_axis_aligned(img, cells(0), 100, 500, 4)
    mm.paint_axis_aligned(img, cells(2), 600, 511, 5)
    mm.paint_axis_aligned(img, cells(1), 300, 540, 4)
    mm.paint_warped(img, cells(5), square_quad(850.0, 512.0, 49.0, 30.0))
    return img


TALL_IDS, WIDE_IDS = [4, 6], [1, 2, 7]


def tall_image():
    """20 columns x 4200 rows, 2-pixel cells: marker 4 near the top, marker 6 below row 4096."""
    img = mm.white(4200, 20)
    mm.paint_axis_aligned(img, cells(4), 3, 5, 2)
    mm.paint_axis_aligned(img, cells(6), 3, 4120, 2)
    return img


def wide_image():
    """8192 columns x 20 rows, 2-pixel cells: markers 1, 2 and 7 in the first, the seventeenth and the last 256-column chunk."""
    img = mm.white(20, 8192)
    mm.paint_axis_aligned(img, cells(1), 3, 3, 2)
    mm.paint_axis_aligned(img, cells(2), 4100, 3, 2)
    mm.paint_axis_aligned(img, cells(7), 8175, 3, 2)
    return img


# ---- the border rule, cell by cell ----
#: the 20 border cells that are no corner cell (a white corner cell would move the component's corner)
BORDER_CELLS = [(i, j) for i in range(7) for j in range(7) if (i in (0, 6)) != (j in (0, 6))]


def border_cell_whitened(i, j, id=4):
    """Marker `id` with the border cell (i, j) white: the ring stays in one piece (its corner cells are black)."""
    c = cells(id).copy()
    c[i, j] = 1
    img = mm.white(64, 96)
    mm.paint_axis_aligned(img, c, 30, 17, 4)
    return img


# ---- step 8 where the areas come from waves that see several labels ----
def area_rule_scene():
    """256 x 120, so that a wave is 64 consecutive pixels of one row.  Id 3 twice with equal areas: at (130, 5), alone in its waves,
    and at (2, 50) with a black square beside it in the same 64 columns; the tie goes to the smaller label, the first.  Id 5 twice:
    5-pixel cells at (130, 80), alone, and 4-pixel cells at (2, 85) beside a square; the larger area stays, the first again.  An
    area that counted the pixels of mixed waves twice would prefer the second of each pair."""
    img = mm.white(120, 256)
    mm.paint_axis_aligned(img, cells(3), 130, 5, 4)
    mm.paint_axis_aligned(img, cells(3), 2, 50, 4)
    img[50:78, 34:62] = 0
    mm.paint_axis_aligned(img, cells(5), 130, 80, 5)
    mm.paint_axis_aligned(img, cells(5), 2, 85, 4)
    img[85:113, 34:62] = 0
    return img
