"""The numpy model of the depth decimation and hole filling (tests/rgbd_decimate_model.py) held to things that do not come from it:
blocks worked out by hand, the literal bit patterns of three derived sensors (computed with exact rational arithmetic, each operation
rounded once), the geometry the derived centre stands for, hole-filled lines written out, and the boundary of the feature: every new
symbol exported, bound and declared.  CPU only."""
import os
import struct

import numpy as np
import pytest

import rgbd_decimate_model as cm
import rgbd_lens_model as lm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["cwipc_hip_rgbd_rig_create_decimated", "cwipc_hip_rgbd_rig_decimation", "cwipc_hip_rgbd_rig_grid_sensor", "cwipc_hip_rgbd_rig_grab_filled"]

#: ((W, H, fx, fy, cx, cy), (k, W', H', the bit patterns of fx' fy' cx' cy'))
SENSORS = [
    ((640, 576, 504.0, 504.5, 320.0, 330.25), (2, 320, 288, (0x406f800000000000, 0x406f880000000000, 0x4063f80000000000, 0x40649c0000000000))),
    ((1280, 720, 607.3, 607.1, 638.7, 367.9), (3, 426, 240, (0x40694ddddddddddd, 0x40694bbbbbbbbbbc, 0x406a922222222223, 0x405e933333333333))),
    ((67, 45, 52.7625, 39.375, 33.5, 25.78125), (8, 8, 5, (0x401a61999999999a, 0x4013b00000000000, 0x400e000000000000, 0x4006480000000000))),
]


def sensor_of(s):
    w, h, fx, fy, cx, cy = s
    return lm.Sensor(w, h, fx, fy, cx, cy, lm.PINHOLE, 0.001, (w + 3, h + 5), 4, (1.0, 2.0, 3.0, 4.0), (0.1,) * 8, np.identity(4) * 2.0, np.identity(4) * 3.0, 7)


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def block(values, k):
    return np.array(values, dtype=np.uint16).reshape(k, k)


# ---- blocks by hand ----

@pytest.mark.parametrize("values,want", [([0, 0, 0, 0], 0), ([5, 0, 0, 0], 5), ([1, 2, 3, 4], 2), ([0, 7, 9, 0], 7), ([4, 3, 2, 1], 2), ([0, 9, 7, 8], 8)])
def test_two_by_two_blocks(values, want):
    assert cm.decimate(block(values, 2), 2).tolist() == [[want]]


def test_three_by_three_blocks():
    assert cm.decimate(block([90, 10, 80, 20, 70, 30, 60, 40, 50], 3), 3).tolist() == [[50]]          # n = 9: the 5th smallest
    assert cm.decimate(block([0, 40, 0, 10, 0, 0, 30, 0, 20], 3), 3).tolist() == [[20]]               # n = 4: the 2nd
    assert cm.decimate(block([0, 0, 0, 0, 0, 0, 0, 0, 65535], 3), 3).tolist() == [[65535]]
    assert cm.decimate(block([3, 0, 0, 0, 0, 0, 0, 0, 1], 3), 3).tolist() == [[1]]                    # n = 2: the lower one


def test_means():
    half = np.zeros((4, 4), dtype=np.uint16)
    half[0, 0], half[3, 3] = 10, 11                                  # 21 / 2 = 10.5 exactly: up
    assert cm.decimate(half, 4).tolist() == [[11]]
    half[1, 2] = 12                                                  # 33 / 3 = 11
    assert cm.decimate(half, 4).tolist() == [[11]]
    half[2, 1] = 12                                                  # 45 / 4 = 11.25
    assert cm.decimate(half, 4).tolist() == [[11]]
    assert cm.decimate(np.full((4, 4), 7, dtype=np.uint16) + (np.arange(16).reshape(4, 4) % 2).astype(np.uint16), 4).tolist() == [[8]]   # 7.5
    assert cm.decimate(np.full((8, 8), 65535, dtype=np.uint16), 8).tolist() == [[65535]]
    assert cm.decimate(np.zeros((8, 8), dtype=np.uint16), 8).tolist() == [[0]]
    for k in range(4, 9):
        one = np.zeros((k, k), dtype=np.uint16)
        one[k - 1, 0] = 4242
        assert cm.decimate(one, k).tolist() == [[4242]]


def test_the_rest_of_a_row_is_not_read():
    line = np.array([[1, 3, 5, 7, 9, 11, 2], [1, 3, 5, 7, 9, 11, 2]], dtype=np.uint16)         # W = 7, k = 2: W' = 3; column 6 would lower the last median
    assert cm.decimate(line, 2).tolist() == [[1, 5, 9]]
    assert cm.decimate(np.vstack([line, np.full((1, 7), 1, dtype=np.uint16)]), 2).tolist() == [[1, 5, 9]]       # nor is row 2 of 3
    wide = np.full((4, 9), 100, dtype=np.uint16)
    wide[:, 8] = 60000                                                                          # k = 4: W' = 2, column 8 would raise a mean
    assert cm.decimate(wide, 4).tolist() == [[100, 100]]
    assert cm.decimate(np.arange(12, dtype=np.uint16).reshape(3, 4), 1).tolist() == np.arange(12).reshape(3, 4).tolist()


# ---- derived intrinsics ----

@pytest.mark.parametrize("s,want", SENSORS)
def test_derived_sensor_bit_patterns(s, want):
    k, width, height, patterns = want
    full = sensor_of(s)
    d = cm.derived_sensor(full, k)
    assert (d.width, d.height) == (width, height)
    assert tuple(bits(x) for x in (d.fx, d.fy, d.cx, d.cy)) == patterns
    # nothing else changes
    assert d._replace(width=0, height=0, fx=0, fy=0, cx=0, cy=0)[6:] == full[6:]
    one = cm.derived_sensor(full, 1)
    assert tuple(bits(x) for x in one[:6]) == tuple(bits(x) for x in full[:6])


@pytest.mark.parametrize("s,want", SENSORS)
def test_a_decimated_pixel_looks_along_the_centre_of_its_block(s, want):
    """(U - cx') / fx' against ((kU + (k - 1) / 2) - cx) / fx, within 4 ulp.  cx' carries the roundings of its subtraction and its
    division, an absolute error of up to an ulp of cx' that U - cx' inherits whatever is left of the difference, so the ulp is that of
    the larger of |U| and |cx'| over fx': next to the optical centre the quotient is small and its own ulp means nothing."""
    _w, _h, fx, _fy, cx, _cy = s
    for k in range(2, 9):
        d = cm.derived_sensor(sensor_of(s), k)
        for U in (0, 1, 7, d.width // 2, d.width - 1):
            got = (np.float64(U) - np.float64(d.cx)) / np.float64(d.fx)
            want_x = ((np.float64(k * U) + np.float64(k - 1) / 2) - np.float64(cx)) / np.float64(fx)
            assert abs(got - want_x) <= 4 * np.spacing(max(abs(U), abs(d.cx)) / abs(d.fx)), (k, U)


# ---- hole filling ----

def test_fill_from_the_left():
    assert cm.holefill(np.array([[0, 0, 3, 0, 0, 5, 0]], dtype=np.uint16), 1).tolist() == [[0, 0, 3, 3, 3, 5, 5]]
    two = np.array([[0, 0, 0], [9, 0, 0], [0, 0, 4]], dtype=np.uint16)                 # a row never takes from another
    assert cm.holefill(two, 1).tolist() == [[0, 0, 0], [9, 9, 9], [0, 0, 4]]


def test_fill_from_around():
    far = np.zeros((1, 5), dtype=np.uint16)
    far[0, 0] = 8
    for mode in (2, 3):
        assert cm.holefill(far, mode).tolist() == [[8, 8, 0, 0, 0]]                    # two pixels away: nothing propagates
    both = np.array([[3, 0, 9]], dtype=np.uint16)
    assert cm.holefill(both, 2).tolist() == [[3, 9, 9]] and cm.holefill(both, 3).tolist() == [[3, 3, 9]]
    ring = np.array([[11, 12, 13], [14, 0, 15], [16, 17, 18]], dtype=np.uint16)
    assert cm.holefill(ring, 2)[1, 1] == 18 and cm.holefill(ring, 3)[1, 1] == 11
    corner = np.array([[0, 0], [0, 6]], dtype=np.uint16)                               # all three holes touch the 6, the diagonal one too
    assert cm.holefill(corner, 2).tolist() == [[6, 6], [6, 6]] == cm.holefill(corner, 3).tolist()
    assert cm.holefill(np.zeros((3, 3), dtype=np.uint16), 2).any() == False


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_a_pixel_with_depth_is_never_changed(mode):
    rng = np.random.default_rng(30 + mode)
    depth = rng.integers(0, 65536, (33, 47)).astype(np.uint16)
    depth[rng.random(depth.shape) < 0.5] = 0
    out = cm.holefill(depth, mode)
    assert np.array_equal(out[depth != 0], depth[depth != 0])
    assert np.array_equal(out, depth) == (mode == 0)
    with pytest.raises(ValueError):
        cm.holefill(depth, 4)


def test_the_composition_runs_the_stages_in_order():
    """Decimation first, the filters on the small grid, the fill last: the temporal state sees the holes, not their filling."""
    import rgbd_depthfilter_model as dm
    from collections import namedtuple
    params = namedtuple("P", "spatial_magnitude spatial_alpha spatial_delta temporal temporal_alpha temporal_delta temporal_persistency")(0, 0.5, 20.0, True, 0.4, 20.0, 0)
    depth = np.zeros((4, 8), dtype=np.uint16)
    depth[:2, :2] = 1000
    hist = [dm.History(2, 4)]
    out = cm.decimated_depth_filter([(depth, None)], hist, 2, params, 1)
    assert out[0][0].tolist() == [[1000, 1000, 1000, 1000], [0, 0, 0, 0]]
    assert hist[0].history.tolist() == [[1, 0, 0, 0], [0, 0, 0, 0]] and hist[0].value[0].tolist() == [1000.0, 0.0, 0.0, 0.0]


# ---- the boundary ----

def test_new_symbols_are_exported_and_declared(cwipc):
    from cwipc_util_amd.util import _SIGNATURES
    dll = cwipc.cwipc_util_dll_load()
    header = open(os.path.join(ROOT, "include", "cwipc_util_amd", "hip_ext.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(dll, name) and name in _SIGNATURES and name in cwipc.util.__all__, name
        assert "%s(" % name in header and "_CWIPC_UTIL_EXPORT" in header[header.index("%s(" % name) - 60: header.index("%s(" % name)], name
    assert "cwipc_hip_rgbd_holefill" in cwipc.util.__all__ and "} cwipc_hip_rgbd_holefill;" in header
    assert "RULE D" in header and header.index("RULE D") < header.index("RULE 0, in front of rule 1")
    import cwipc_util_amd.rgbd as rgbd
    assert "RgbdHoleFill" in rgbd.__all__
    assert rgbd.RgbdHoleFill(2).as_struct().mode == 2 and rgbd.RgbdHoleFill().mode == 1
    import inspect
    assert inspect.signature(rgbd.RgbdRig.__init__).parameters["decimation"].default == 1
    assert inspect.signature(rgbd.RgbdRig.grab).parameters["holefill"].default is None
    source = inspect.signature(rgbd.RgbdRigSource.__init__).parameters
    assert source["decimation"].default == 1 and source["holefill"].default is None
