"""The numpy restatement of RULE C (tests/codec_model.py) held to things that do not come from it: packets worked out by hand, the
properties the rule promises (nesting, the clamp, the error bounds), the packet's sizes, and the library's boundary.  No GPU."""
import struct

import numpy as np
import pytest

import codec_model as cm

# Three points, octree_bits 2, jpeg_quality 95, timestamp 0x0102.  The cube is [0, 1]^3: cells (0,0,0), (1,0,0) and (3,3,3), keys
# 0, 4 (second triple: x) and 63.  Depth 0: children 0 and 7 -> 0x81; depth 1: node 0 has children 0 and 4 -> 0x11, node 7 has child
# 7 -> 0x80.  All tiles are 1: tile_mode 0, tile_value 1.
HAND_POINTS = cm.make_cloud([[1, 1, 1], [0, 0, 0], [0.3, 0, 0]], [[200, 100, 50], [10, 20, 30], [1, 2, 3]], 1)
HAND_PACKET = bytes([
    0x63, 0x77, 0x61, 0x6f,  0x01, 0x00, 0x00, 0x00,                              # "cwao", version 1
    0x02, 0x01, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00,                              # timestamp
    0x03, 0x00, 0x00, 0x00,  0x02, 0x08, 0x00, 0x01,                              # nleaves 3; bits 2, colour bits 8, mode 0, tile 1
    0x00, 0x00, 0x00, 0x00,  0x00, 0x00, 0x00, 0x00,  0x00, 0x00, 0x00, 0x00,    # min
    0x00, 0x00, 0x00, 0x00,                                                      # reserved
    0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0xf0, 0x3f,                              # side 1.0
    0x02, 0x00, 0x00, 0x00,  0x03, 0x00, 0x00, 0x00,                              # nodes
    0x81, 0x11, 0x80, 0x00,                                                      # occupancy, padded
    0x0a, 0x14, 0x1e,  0x01, 0x02, 0x03,  0xc8, 0x64, 0x32,  0x00, 0x00, 0x00,    # colours in key order, padded
])


def test_one_point_at_bits_1():
    packet = cm.encode(cm.make_cloud([[2.0, -3.0, 5.0]], [[9, 8, 7]], 4), 1, 95, 11)
    info = cm.parse(packet)
    assert packet[info["occupancy_offset"]] == 0x01 and info["nodes"] == [1] and info["side"] == 1.0
    pts, ts, cell = cm.decode(packet)
    assert ts == 11 and cell == np.float32(0.5) and len(pts) == 1
    assert (pts['x'][0], pts['y'][0], pts['z'][0]) == (2.25, -2.75, 5.25) and (pts['r'][0], pts['g'][0], pts['b'][0], pts['tile'][0]) == (9, 8, 7, 4)
    # (min + 0.5 of a cell of side 1 / 2: the centre of cell 0)
    assert packet[22] == 0 and packet[23] == 4


def test_opposite_corners_and_all_eight():
    two = cm.encode(cm.make_cloud([[0, 0, 0], [1, 1, 1]]), 1, 95)
    assert two[cm.parse(two)["occupancy_offset"]] == 0x81
    corners = [[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)]
    eight = cm.encode(cm.make_cloud(corners), 1, 95)
    assert eight[cm.parse(eight)["occupancy_offset"]] == 0xFF and cm.parse(eight)["nodes"] == [8]
    # child index: x is the most significant bit of the triple
    x_only = cm.encode(cm.make_cloud([[0, 0, 0], [1, 0, 0]]), 1, 95)
    assert x_only[cm.parse(x_only)["occupancy_offset"]] == 0x11
    z_only = cm.encode(cm.make_cloud([[0, 0, 0], [0, 0, 1]]), 1, 95)
    assert z_only[cm.parse(z_only)["occupancy_offset"]] == 0x03


def test_hand_written_packet():
    assert len(HAND_PACKET) == 72
    assert cm.encode(HAND_POINTS, 2, 95, 0x0102) == HAND_PACKET
    pts, ts, cell = cm.decode(HAND_PACKET)
    assert ts == 0x0102 and cell == np.float32(0.25)
    assert pts['x'].tolist() == [0.125, 0.375, 0.875] and pts['y'].tolist() == [0.125, 0.125, 0.875] and pts['z'].tolist() == [0.125, 0.125, 0.875]
    assert pts['r'].tolist() == [10, 1, 200] and pts['g'].tolist() == [20, 2, 100] and pts['b'].tolist() == [30, 3, 50] and pts['tile'].tolist() == [1, 1, 1]


def test_clamp_puts_the_maximum_into_the_last_cell():
    rng = np.random.default_rng(3)
    for b in (1, 2, 9, 16):
        pts = cm.random_cloud(rng, 200, 7.0, (3.0, -2.0, 0.1))
        P = cm.finite_points(pts)
        mn, side = cm.cube(P)
        q = cm.cells(P, mn, side, b)
        xyz = np.stack([P['x'], P['y'], P['z']], axis=1)
        longest = int(np.argmax(xyz.max(axis=0).astype(np.float64) - mn))
        assert q[np.argmax(xyz[:, longest]), longest] == (1 << b) - 1
        assert q.min() >= 0 and q.max() <= (1 << b) - 1
    cube_corner = cm.make_cloud([[0, 0, 0], [2, 2, 2]])
    mn, side = cm.cube(cube_corner)
    assert cm.cells(cube_corner, mn, side, 5)[1].tolist() == [31, 31, 31]


@pytest.mark.parametrize("scale,offset", [(1e-3, (0, 0, 0)), (1.0, (0.5, -0.25, 3.0)), (1e3, (-200.0, 100.0, 0.0)), (3.0, (1e3, -1e3, 1e-3))])
def test_nesting_and_error_bound(scale, offset):
    rng = np.random.default_rng(int(scale * 1000) % 9973)
    pts = cm.random_cloud(rng, 4000, scale, offset)
    P = cm.finite_points(pts)
    mn, side = cm.cube(P)
    q = {b: cm.cells(P, mn, side, b) for b in range(1, 17)}
    for b in range(2, 17):
        assert np.array_equal(q[b - 1], q[b] >> 1), b
    xyz = np.stack([P['x'], P['y'], P['z']], axis=1)
    for b in (1, 4, 9, 16):
        packet = cm.encode(pts, b, 95)
        dec, _, cell = cm.decode(packet)
        leaf = np.searchsorted(cm.leaf_keys_of(packet), cm.keys(q[b], b))
        got = np.stack([dec['x'], dec['y'], dec['z']], axis=1)[leaf]
        bound = (side / (1 << b)) / 2 + 2 * np.spacing(np.abs(xyz)).astype(np.float64)
        assert (np.abs(got.astype(np.float64) - xyz.astype(np.float64)) <= bound).all(), b


def test_colour_rule_and_its_exact_bound():
    for s in range(5):
        worst = 0
        for m in range(256):
            v = cm.colour_store(m, s)
            assert 0 <= v < (1 << (8 - s))
            worst = max(worst, abs(cm.colour_load(v, s) - m))
        # the low s bits r of m are replaced by (1 << s) >> 1: the error is half - r, r in 0 .. 2^s - 1; 255 is never exceeded
        half = (1 << s) >> 1
        assert worst == max(half, (1 << s) - 1 - half) == (half if s != 1 else 1)
    # a leaf's colour is the rounded mean in integers
    pts = cm.make_cloud([[0, 0, 0]] * 3 + [[1, 1, 1]], [[1, 2, 255], [2, 2, 255], [2, 3, 254], [0, 0, 0]])
    dec, _, _ = cm.decode(cm.encode(pts, 1, 95))
    assert (dec['r'][0], dec['g'][0], dec['b'][0]) == ((5 + 1) // 3, (7 + 1) // 3, (764 + 1) // 3)


@pytest.mark.parametrize("quality,shift", [(100, 0), (91, 0), (90, 0), (89, 1), (76, 1), (75, 1), (74, 2), (51, 2), (50, 2), (49, 3), (26, 3), (25, 3),
                                           (24, 4), (1, 4), (0, 4)])
def test_quality_thresholds(quality, shift):
    assert cm.colour_shift(quality) == shift
    packet = cm.encode(HAND_POINTS, 2, quality)
    assert packet[21] == 8 - shift and len(packet) == 48 + 8 + 4 + cm.pad4((3 * 3 * (8 - shift) + 7) // 8)


def test_tiles():
    pts = cm.make_cloud([[0, 0, 0], [0.01, 0, 0], [1, 1, 1]], None, [1, 2, 3])
    mixed = cm.encode(pts, 1, 95)
    info = cm.parse(mixed)
    assert info["tile_mode"] == 0 and info["tile_value"] == 3          # the OR of the first leaf's tiles is the other leaf's tile
    pts['tile'] = [1, 2, 4]
    mixed = cm.encode(pts, 1, 95)
    info = cm.parse(mixed)
    assert info["tile_mode"] == 1 and info["tile_value"] == 0 and mixed[info["tile_offset"]:] == bytes([3, 4])
    assert cm.decode(mixed)[0]['tile'].tolist() == [3, 4]
    pts['tile'] = 7
    uniform = cm.encode(pts, 1, 95)
    assert cm.parse(uniform)["tile_mode"] == 0 and len(uniform) == len(mixed) - 2 and cm.decode(uniform)[0]['tile'].tolist() == [7, 7]


@pytest.mark.parametrize("bits", [1, 2, 9, 16])
def test_empty_cloud(bits):
    nan = cm.make_cloud([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]])
    for pts in (cm.make_cloud(np.zeros((0, 3))), nan):
        packet = cm.encode(pts, bits, 85, 9)
        assert len(packet) == 48 + 4 * bits
        assert packet[:24] == b"cwao" + struct.pack("<IQIBBBB", 1, 9, 0, bits, 7, 0, 0) and packet[24:40] == bytes(16)
        assert struct.unpack("<d", packet[40:48])[0] == 1.0 and packet[48:] == bytes(4 * bits)
        dec, ts, cell = cm.decode(packet)
        assert len(dec) == 0 and ts == 9 and cell == np.float32(1.0 / (1 << bits))


def test_non_finite_points_are_left_out_and_coincident_points_share_a_cube_of_side_1():
    pts = cm.make_cloud([[1, 2, 3], [np.nan, 2, 3], [1, 2, 3], [1, np.inf, 3]], [[10, 10, 10], [250, 250, 250], [20, 20, 20], [250, 250, 250]], [1, 8, 2, 8])
    dec, _, cell = cm.decode(cm.encode(pts, 3, 95))
    assert len(dec) == 1 and cell == np.float32(0.125) and (dec['r'][0], dec['tile'][0]) == (15, 3)
    assert (dec['x'][0], dec['y'][0], dec['z'][0]) == (1.0625, 2.0625, 3.0625)


def test_library_exports_the_new_symbols(cwipc):
    """The boundary: every new symbol is exported, bound in the wrapper and public; the reference's names are in cwipc_util_amd.codec."""
    from cwipc_util_amd.util import _SIGNATURES
    import cwipc_util_amd.codec as codec
    dll = cwipc.cwipc_util_dll_load()
    names = ["cwipc_hip_new_encoder", "cwipc_hip_encoder_free", "cwipc_hip_encoder_feed", "cwipc_hip_encoder_available",
             "cwipc_hip_encoder_get_encoded_size", "cwipc_hip_encoder_copy_data", "cwipc_hip_encoder_at_gop_boundary", "cwipc_hip_encoder_eof",
             "cwipc_hip_encoder_close", "cwipc_hip_new_encodergroup", "cwipc_hip_encodergroup_addencoder", "cwipc_hip_encodergroup_feed",
             "cwipc_hip_encodergroup_close", "cwipc_hip_encodergroup_free", "cwipc_hip_new_decoder", "cwipc_hip_decoder_feed",
             "cwipc_hip_decoder_available", "cwipc_hip_decoder_get", "cwipc_hip_decoder_eof", "cwipc_hip_decoder_close", "cwipc_hip_decoder_free",
             "cwipc_hip_codec_packet_info"]
    for name in names:
        assert hasattr(dll, name) and name in _SIGNATURES and name in cwipc.util.__all__, name
    assert "cwipc_hip_encoder_params" in cwipc.util.__all__
    assert [f[0] for f in cwipc.cwipc_hip_encoder_params._fields_] == ["do_inter_frame", "gop_size", "exp_factor", "octree_bits", "jpeg_quality",
                                                                       "macroblock_size", "tilenumber", "voxelsize"]
    for name in ("cwipc_encoder_params", "cwipc_new_encoder_params", "cwipc_new_encoder", "cwipc_new_encodergroup", "cwipc_new_decoder",
                 "cwipc_encoder_wrapper", "cwipc_decoder_wrapper", "packet_info"):
        assert name in codec.__all__ and hasattr(codec, name), name
    p = codec.cwipc_new_encoder_params()
    assert (p.do_inter_frame, p.gop_size, p.exp_factor, p.octree_bits, p.jpeg_quality, p.macroblock_size, p.tilenumber, p.voxelsize) == \
        (False, 1, 1.0, 9, 85, 16, 0, 0.0)
    p = codec.cwipc_encoder_params(False, 1, 1.0, 7, 60, 16, 2, 0.5)
    p.octree_bits = 11
    assert (p.octree_bits, p.jpeg_quality, p.tilenumber, p.voxelsize) == (11, 60, 2, 0.5)
    from cwipc_util_amd.net.sink_encoder import cwipc_sink_encoder
    from cwipc_util_amd.net.source_decoder import cwipc_source_decoder, cwipc_activesource_decoder
    assert callable(cwipc_sink_encoder) and callable(cwipc_source_decoder) and callable(cwipc_activesource_decoder)


def test_packet_info_of_the_hand_written_packet(cwipc):
    """Host code of the built library, no GPU: the validator reads the hand-written packet as the model does."""
    import cwipc_util_amd.codec as codec
    info = codec.packet_info(HAND_PACKET)
    want = cm.parse(HAND_PACKET)
    for key in ("timestamp", "nleaves", "octree_bits", "colour_bits", "tile_mode", "tile_value", "side", "nodes", "occupancy_offset", "colour_offset",
                "tile_offset", "total_bytes"):
        assert info[key] == want[key], key
    assert info["min"] == (0.0, 0.0, 0.0)
    with pytest.raises(cwipc.CwipcError, match="magic"):
        codec.packet_info(b"cpcd" + HAND_PACKET[4:])


# ---------------------------------------------------------------------------
# cell boundaries
# ---------------------------------------------------------------------------
# The cubes of the boundary clouds (0.1f is the float32 nearest to 0.1).  A near miss of the cell rule differs from it only for a
# point within an ulp of a cell boundary, and which near miss shows depends on the cube: with min = 0 the subtraction is exact in
# any precision, so [0, 49] shows only the reciprocal and the folded factor (49 is no power of two), [-1.5, 1.5] the float32
# subtraction, [0, 0.1f] the float32 division alone, [0.1f, 1] both float32 steps with a minimum that is no short binary fraction.
BOUNDARY_CUBES = ((0.0, 49.0), (-1.5, 1.5), (0.0, float(np.float32(0.1))), (float(np.float32(0.1)), 1.0))
_boundary_clouds = {}


def boundary_cloud(cube, bits):
    """cm.boundary_cloud of BOUNDARY_CUBES[cube] at `bits`, made once and shared by the CPU, host-program and GPU tests: read only."""
    key = (cube, bits)
    if key not in _boundary_clouds:
        mn, mx = BOUNDARY_CUBES[cube]
        pts = cm.boundary_cloud(mn, mx, bits, np.random.default_rng(7000 + 100 * cube + bits))
        pts.setflags(write=False)
        _boundary_clouds[key] = pts
    return _boundary_clouds[key]


@pytest.mark.parametrize("bits", [1, 4, 9, 16])
@pytest.mark.parametrize("cube", range(len(BOUNDARY_CUBES)))
def test_boundary_clouds_are_what_they_say(cube, bits):
    """The cube is the one asked for, both end cells are hit on every axis, and every inner boundary has a point on each side of it
    (4 and 9 bits, where every boundary is taken)."""
    pts = boundary_cloud(cube, bits)
    mn, side = cm.cube(pts)
    lo, hi = np.float32(BOUNDARY_CUBES[cube][0]), np.float32(BOUNDARY_CUBES[cube][1])
    assert mn.tobytes() == np.array([lo, lo, lo], dtype=np.float32).tobytes() and side == float(np.float64(hi) - np.float64(lo))
    q = cm.cells(pts, mn, side, bits)
    assert q.min(axis=0).tolist() == [0, 0, 0] and q.max(axis=0).tolist() == [(1 << bits) - 1] * 3
    if bits in (4, 9):
        for a in range(3):
            assert len(np.unique(q[:, a])) == 1 << bits
        assert len(pts) == 3 * ((1 << bits) + 1) - 2 + 2      # three per boundary, less the two outside the cube, plus the corners


@pytest.mark.parametrize("variant", cm.CELL_VARIANTS)
@pytest.mark.parametrize("bits", [4, 9, 16])
def test_boundary_clouds_tell_every_near_miss_from_the_rule(bits, variant):
    """A condition on the test inputs, not a measurement: for each near miss of the cell rule at least one of the cubes has 5 or more
    candidate coordinates whose cell it changes (counted on the x axis, which holds every candidate once).  Uniform random points do
    not deliver this: see test_random_clouds_do_not."""
    changed = []
    for cube in range(len(BOUNDARY_CUBES)):
        pts = boundary_cloud(cube, bits)
        mn, side = cm.cube(pts)
        changed.append(int((cm.cells_variant(pts, mn, side, bits, variant)[:, 0] != cm.cells(pts, mn, side, bits)[:, 0]).sum()))
    print(bits, variant, changed)
    assert max(changed) >= 5, changed
    # and each cube earns its place: it is the one, or one of the ones, that shows the variant it was chosen for
    expected = {"recip": (0,), "scale": (0,), "sub32": (1, 3), "div32": (2, 3)}[variant]
    assert all(changed[c] >= (5 if bits > 4 else 3) for c in expected), changed


def test_random_clouds_do_not():
    """Why the boundary clouds exist: over 4096 uniform random points the reciprocal and the folded factor change no cell at any depth."""
    rng = np.random.default_rng(21)
    pts = cm.random_cloud(rng, 4096, 2.0, (1.0, -0.5, 0.25))
    mn, side = cm.cube(pts)
    for bits in (4, 9, 12, 16):
        q = cm.cells(pts, mn, side, bits)
        for variant in ("recip", "scale"):
            assert np.array_equal(cm.cells_variant(pts, mn, side, bits, variant), q), (bits, variant)


@pytest.mark.parametrize("cube", range(len(BOUNDARY_CUBES)))
def test_prefix_property_on_the_boundaries(cube):
    """q(b - 1) == q(b) >> 1 and key(b - 1) == key(b) >> 3, b in 2..16, on every boundary cloud: what lets the encoder group cut a
    coarser packet from a finer sort."""
    for made_for in (1, 4, 9, 16):
        pts = boundary_cloud(cube, made_for)
        mn, side = cm.cube(pts)
        q = {b: cm.cells(pts, mn, side, b) for b in range(1, 17)}
        k = {b: cm.keys(q[b], b) for b in range(1, 17)}
        for b in range(2, 17):
            assert np.array_equal(q[b - 1], q[b] >> 1), (made_for, b)
            assert np.array_equal(k[b - 1], k[b] >> np.uint64(3)), (made_for, b)


# ---------------------------------------------------------------------------
# build_packet
# ---------------------------------------------------------------------------
def test_build_packet_restates_the_hand_written_packet_and_round_trips():
    assert cm.build_packet([0, 4, 63], [[10, 20, 30], [1, 2, 3], [200, 100, 50]], [1, 1, 1], [0, 0, 0], 1.0, 2, 8, 0x0102) == HAND_PACKET
    rng = np.random.default_rng(22)
    for bits, cb, n in ((1, 4, 3), (5, 7, 200), (16, 5, 999)):
        lk = np.unique(rng.integers(0, 1 << (3 * bits), n, dtype=np.uint64))
        stored, tiles = rng.integers(0, 1 << cb, (len(lk), 3)), rng.integers(0, 256, len(lk))
        packet = cm.build_packet(lk, stored, tiles, [-0.0, 1e-42, 3.0], 2.0 ** -60, bits, cb, (1 << 63) + 5)
        info = cm.parse(packet)
        assert info["timestamp"] == (1 << 63) + 5 and info["nleaves"] == len(lk) and info["side"] == 2.0 ** -60
        assert info["min"].tobytes() == np.array([-0.0, 1e-42, 3.0], dtype=np.float32).tobytes()
        assert np.array_equal(cm.leaf_keys_of(packet, info), lk)
        dec = cm.decode(packet)[0]
        s = 8 - cb
        assert np.array_equal(np.stack([dec['r'], dec['g'], dec['b']], axis=1), np.minimum(255, (stored << s) + ((1 << s) >> 1)))
        assert np.array_equal(dec['tile'], tiles.astype(np.uint8))
