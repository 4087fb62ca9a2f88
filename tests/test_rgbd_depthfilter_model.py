"""Properties of the depth post-processing's numpy model (tests/rgbd_depthfilter_model.py) that do not come from the model: identities,
the strict comparison, zeros, the order of the passes on lines worked out by hand, and the persistence table written out literally.
The hand-worked cases and the table are what the host program and the GPU tests are held to as well.  CPU only."""
import numpy as np
import pytest

import rgbd_depthfilter_model as dm

# alpha 0.5, delta 10, one iteration; every value below is exact in float64
# forward:  s = 100;  104: |4| < 10, s = 102, d = 102;  108: |6| < 10, s = 105, d = 105                       -> 100 102 105
# backward: s = 105;  102: s = 103.5, d = floor(104.0) = 104;  100: |3.5|, s = 101.75, d = floor(102.25) = 102 -> 102 104 105
# (a backward pass over the ORIGINAL line would start from 108 and give 106 in the middle)
THREE = (np.array([[100, 104, 108]], dtype=np.uint16), np.array([[102, 104, 105]], dtype=np.uint16))
# rows forward:   100 104 -> 100 102;   110 102: |-8| < 10, s = 106 -> 110 106
# rows backward:  s = 102; 100: s = 101 -> 101 102;   s = 106; 110: s = 108 -> 108 106
# columns forward:   101 108: |7|, s = 104.5, d = floor(105.0) = 105 -> 101 105;   102 106: s = 104 -> 102 104
# columns backward:  s = 105; 101: s = 103 -> 103 105;   s = 104; 102: s = 103 -> 103 104
# (columns first would not blend 100 with 110 at all: the difference is exactly delta)
TWO_BY_TWO = (np.array([[100, 104], [110, 102]], dtype=np.uint16), np.array([[103, 103], [105, 104]], dtype=np.uint16))
HAND_ALPHA, HAND_DELTA = 0.5, 10.0

# persists(mode, h): 256 bits per mode as 64 hex digits, h = 0 the leftmost bit
PERSISTS = [
    "0000000000000000000000000000000000000000000000000000000000000000",
    "0000000000000000000000000000000000000000000000000000000000000001",
    "1717171717171717171717171717171717171717171717171717171717171717",
    "177f177f177f177f177f177f177f177f177f177f177f177f177f177f177f177f",
    "177f7fff7fffffff7fffffffffffffff7fffffffffffffffffffffffffffffff",
    "7777777777777777777777777777777777777777777777777777777777777777",
    "7fffffff7fffffff7fffffff7fffffff7fffffff7fffffff7fffffff7fffffff",
    "7fffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffff",
    "ffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffff",
]


def persists_table(mode):
    """bool[256] of the literal table."""
    return np.array([c == "1" for c in format(int(PERSISTS[mode], 16), "0256b")])


def noisy(rng, height, width, zeros=0.1):
    depth = rng.integers(980, 1060, (height, width)).astype(np.uint16)
    depth[rng.random((height, width)) < zeros] = 0
    return depth


def test_alpha_one_is_the_identity():
    rng = np.random.default_rng(1)
    depth = noisy(rng, 23, 31)
    assert np.array_equal(dm.spatial(depth, 3, 1.0, 25.0), depth)
    hist = dm.History(23, 31)
    for _ in range(3):
        frame = noisy(rng, 23, 31)
        assert np.array_equal(hist.temporal(frame, 1.0, 25.0, 0), frame)
    assert (hist.value[frame != 0] == frame[frame != 0]).all()


def test_a_constant_image_is_unchanged():
    for value in (1, 1000, 65535):
        depth = np.full((9, 14), value, dtype=np.uint16)
        assert np.array_equal(dm.spatial(depth, 5, 0.3, 7.0), depth)
        hist = dm.History(9, 14)
        for _ in range(4):
            assert np.array_equal(hist.temporal(depth, 0.3, 7.0, 3), depth)
        assert (hist.value == value).all() and (hist.history == 0x0f).all()


def test_a_step_of_exactly_delta_is_kept_and_one_ulp_more_delta_blends():
    pair = np.array([[1000, 1016]], dtype=np.uint16)
    assert np.array_equal(dm.spatial(pair, 1, 0.5, 16.0), pair)
    assert np.array_equal(dm.spatial(pair.T, 1, 0.5, 16.0), pair.T)
    # forward 1000 1008, backward from 1008: 1004 1008
    assert dm.spatial(pair, 1, 0.5, float(np.nextafter(16.0, np.inf))).tolist() == [[1004, 1008]]
    assert dm.spatial(pair, 1, 0.5, float(np.nextafter(16.0, -np.inf))).tolist() == [[1000, 1016]]
    hist = dm.History(1, 2)
    hist.temporal(np.array([[1000, 1000]], dtype=np.uint16), 0.5, 16.0, 0)
    assert hist.temporal(pair, 0.5, 16.0, 0).tolist() == [[1000, 1016]] and hist.value.tolist() == [[1000.0, 1016.0]]


def test_a_zero_is_never_filled_and_separates_its_neighbours():
    line = np.array([[1000, 1004, 0, 1006, 1002]], dtype=np.uint16)
    got = dm.spatial(line, 1, 0.5, 10.0)
    left, right = dm.spatial(line[:, :2], 1, 0.5, 10.0), dm.spatial(line[:, 3:], 1, 0.5, 10.0)
    assert got[0, 2] == 0 and np.array_equal(got[:, :2], left) and np.array_equal(got[:, 3:], right)
    assert got.tolist() == [[1001, 1002, 0, 1005, 1004]]
    rng = np.random.default_rng(2)
    depth = noisy(rng, 40, 40, 0.2)
    for magnitude in (1, 5):
        out = dm.spatial(depth, magnitude, 0.4, 30.0)
        assert np.array_equal(out == 0, depth == 0) and not np.array_equal(out, depth)


def test_the_backward_pass_sees_the_forward_passs_output():
    line, want = THREE
    assert np.array_equal(dm.spatial(line, 1, HAND_ALPHA, HAND_DELTA), want)
    assert np.array_equal(dm.spatial(line.T, 1, HAND_ALPHA, HAND_DELTA), want.T)          # the same line as a column
    forward = dm.line_pass(line.copy(), HAND_ALPHA, HAND_DELTA, False)
    assert forward.tolist() == [[100, 102, 105]]
    assert dm.line_pass(line.copy(), HAND_ALPHA, HAND_DELTA, True).tolist() == [[103, 106, 108]]   # backward alone: another line


def test_rows_are_filtered_before_columns():
    image, want = TWO_BY_TWO
    assert np.array_equal(dm.spatial(image, 1, HAND_ALPHA, HAND_DELTA), want)
    columns_first = dm.spatial(image.T, 1, HAND_ALPHA, HAND_DELTA).T
    assert not np.array_equal(columns_first, want)


@pytest.mark.parametrize("mode", range(9))
def test_persists_against_the_literal_table(mode):
    table = persists_table(mode)
    assert table.shape == (256,)
    assert np.array_equal(dm.persists(mode, np.arange(256)), table)
    assert [bool(dm.persists(mode, h)) for h in (0, 1, 3, 0x80, 0xff)] == [bool(table[h]) for h in (0, 1, 3, 0x80, 0xff)]


def test_the_literal_table_says_what_the_rules_say():
    counts = [int(persists_table(m).sum()) for m in range(9)]
    # never; one byte; 4 of 8 low patterns; 11 of 16; all but the 9 with at most one bit; 3 of 4; 31 of 32; all but 0; always
    assert counts == [0, 1, 128, 176, 247, 192, 248, 255, 256]
    assert not persists_table(7)[0] and persists_table(8)[0] and persists_table(1)[255] and not persists_table(1)[254]
    assert persists_table(2)[0b011] and not persists_table(2)[0b1100] and persists_table(3)[0b1100] and persists_table(4)[0x81]
    assert persists_table(5)[2] and not persists_table(5)[4] and persists_table(6)[16] and not persists_table(6)[32]


def test_persistence_uses_the_history_from_before_the_grab():
    hist = dm.History(1, 1)
    one, none = np.array([[1000]], dtype=np.uint16), np.array([[0]], dtype=np.uint16)
    hist.temporal(one, 0.4, 20.0, 5)
    assert hist.history[0, 0] == 1
    assert hist.temporal(none, 0.4, 20.0, 5)[0, 0] == 1000 and hist.history[0, 0] == 2      # seen one grab ago
    assert hist.temporal(none, 0.4, 20.0, 5)[0, 0] == 1000 and hist.history[0, 0] == 4      # seen two grabs ago
    assert hist.temporal(none, 0.4, 20.0, 5)[0, 0] == 0 and hist.value[0, 0] == 1000.0      # three: no longer, the value stays
    hist.reset()
    assert hist.temporal(none, 0.4, 20.0, 8)[0, 0] == 0                                     # always -- but there is no value


def test_the_unrounded_running_value_converges():
    hist = dm.History(1, 1)
    outs = [int(hist.temporal(np.array([[d]], dtype=np.uint16), 0.4, 20.0, 0)[0, 0]) for d in [1003] + [1000] * 11]
    # s: 1003, 1001.8, 1001.08, 1000.648, 1000.3888 ...; a rounded s would stall at 1001 (0.4*1000 + 0.6*1001 = 1000.6 -> 1001)
    assert outs[:5] == [1003, 1002, 1001, 1001, 1000] and outs[-1] == 1000
    assert 1000.0 < hist.value[0, 0] < 1000.02
