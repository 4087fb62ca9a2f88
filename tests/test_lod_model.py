"""RULE L's numpy model (tests/lod_model.py) against RULE C's (tests/codec_model.py): the geometry, the tile fields and the tile plane
of a cut ARE those of the same cloud encoded at the cut's bits; the colours are means of the stored leaf colours.  CPU only."""
import struct

import numpy as np
import pytest

import codec_model as cm
import entropy_model as em
import lod_model as lm


@pytest.fixture(scope="module")
def structured():
    pts = em.structured_cloud(60000)
    return pts, cm.encode(pts, 9, 85, timestamp=4242)


@pytest.mark.parametrize("t", [1, 4, 8, 9])
def test_cut_of_the_structured_cloud_is_the_native_encode_but_for_the_colours(structured, t):
    pts, packet = structured
    cut, native = lm.lod(packet, t), cm.encode(pts, t, 85, timestamp=4242)
    a, b = cm.parse(cut), cm.parse(native)
    assert cut[24:48] == native[24:48]
    assert a["nodes"] == b["nodes"] and a["nleaves"] == b["nleaves"] and a["octree_bits"] == t
    assert cut[a["occupancy_offset"]:a["colour_offset"]] == native[b["occupancy_offset"]:b["colour_offset"]]
    assert (a["tile_mode"], a["tile_value"]) == (b["tile_mode"], b["tile_value"])
    assert cut[a["tile_offset"]:] == native[b["tile_offset"]:]
    assert a["timestamp"] == 4242 and a["colour_bits"] == b["colour_bits"] and len(cut) == len(native)
    if t == 9:
        assert cut == packet
    # hence the points of the cut are the points of the native packet; the colours are close, not equal
    pa, pb = cm.decode(cut)[0], cm.decode(native)[0]
    for f in ("x", "y", "z", "tile"):
        assert pa[f].tobytes() == pb[f].tobytes()
    assert cm.decode(cut)[2] == cm.decode(native)[2]


HAND = lm.hand_packets()


@pytest.mark.parametrize("name", list(HAND))
def test_hand_built_packets(name):
    packet = HAND[name]
    info = cm.parse(packet)
    b = info["octree_bits"]
    assert lm.lod(packet, b) == packet
    for t in lm.targets(b):
        cut = lm.lod(packet, t)
        c = cm.parse(cut)
        assert c["octree_bits"] == t and c["nodes"] == info["nodes"][:t] and c["nleaves"] == info["nodes"][t - 1]
        assert c["colour_bits"] == info["colour_bits"] and c["timestamp"] == info["timestamp"] and cut[24:48] == packet[24:48]
        assert cut[c["occupancy_offset"]:c["occupancy_offset"] + c["occupancy_bytes"]] == packet[info["occupancy_offset"]:info["occupancy_offset"] + c["occupancy_bytes"]]
    for t in (0, b + 1):
        with pytest.raises(ValueError):
            lm.lod(packet, t)


def test_single_leaf_keeps_its_colour_at_every_depth():
    for t in range(1, 8):
        pts = cm.decode(lm.lod(HAND["single leaf"], t))[0]
        assert len(pts) == 1 and (pts["r"][0], pts["g"][0], pts["b"][0], pts["tile"][0]) == (200, 3, 77, 5)


def test_full_block_of_255_rounds_to_255():
    packet = HAND["full block of 255"]
    assert cm.parse(packet)["nleaves"] == 4096
    for t in (1, 2, 4):
        pts = cm.decode(lm.lod(packet, t))[0]
        assert len(pts) == 8 ** (t - 1) and (pts["r"] == 255).all() and (pts["g"] == 255).all() and (pts["b"] == 255).all()


def test_one_leaf_beside_4096():
    packet = HAND["1 beside 4096"]
    full = cm.decode(packet)[0]
    cut = cm.decode(lm.lod(packet, 2))[0]
    assert len(full) == 4097 and len(cut) == 2
    assert (cut["r"][0], cut["g"][0], cut["b"][0], cut["tile"][0]) == (full["r"][0], full["g"][0], full["b"][0], full["tile"][0])
    for ch in "rgb":
        total = int(full[ch][1:].astype(np.int64).sum())
        assert cut[ch][1] == (total + 2048) // 4096
    assert cut["tile"][1] == np.bitwise_or.reduce(full["tile"][1:])


def test_means_are_taken_on_the_stored_values():
    packet = HAND["cb 4, 1001 leaves"]
    info = cm.parse(packet)
    stored = cm.unpack_bits(packet[info["colour_offset"]:info["colour_offset"] + info["colour_bytes"]], 3 * 1001, 4).reshape(-1, 3)
    keys = cm.leaf_keys_of(packet)
    cut = lm.lod(packet, 2)
    c = cm.parse(cut)
    got = cm.unpack_bits(cut[c["colour_offset"]:c["colour_offset"] + c["colour_bytes"]], 3 * c["nleaves"], 4).reshape(-1, 3)
    for j, prefix in enumerate(np.unique(keys >> np.uint64(9))):
        members = stored[(keys >> np.uint64(9)) == prefix]
        assert list(got[j]) == [(int(members[:, ch].sum()) + len(members) // 2) // len(members) for ch in range(3)]


def test_tile_plane_goes_and_stays():
    gone = cm.parse(lm.lod(HAND["plane goes away"], 2))
    assert cm.parse(HAND["plane goes away"])["tile_mode"] == 1 and (gone["tile_mode"], gone["tile_value"]) == (0, 3)
    assert cm.parse(lm.lod(HAND["plane goes away"], 3))["tile_mode"] == 1
    stays = lm.lod(HAND["plane stays"], 2)
    info = cm.parse(stays)
    assert info["tile_mode"] == 1 and set(stays[info["tile_offset"]:]) == {1, 2}
    flat = cm.parse(lm.lod(HAND["tile mode 0"], 2))
    assert (flat["tile_mode"], flat["tile_value"]) == (0, 9)


def test_empty_packet_maps_to_the_empty_packet_of_t_bits():
    empty = cm.encode(np.zeros(0, dtype=cm.POINT_DTYPE), 9, 60, timestamp=99)
    cut = lm.lod(empty, 4)
    want = cm.encode(np.zeros(0, dtype=cm.POINT_DTYPE), 4, 60, timestamp=99)
    assert cut == want and cm.parse(cut)["nleaves"] == 0


def test_cuts_of_cuts_are_not_promised():
    """Means of means: the rule says so, and this cloud shows it."""
    packet = HAND["1 beside 4096"]
    k = np.array([0, 1, 8], dtype=np.uint64)
    p = cm.build_packet(k, [[0, 0, 0], [0, 0, 0], [255, 255, 255]], [1, 1, 1], np.zeros(3, dtype=np.float32), 1.0, 3, 8, 0)
    assert lm.lod(lm.lod(p, 2), 1) != lm.lod(p, 1)
    assert struct.unpack("<I", lm.lod(packet, 1)[16:20])[0] == 2
