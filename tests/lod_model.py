"""RULE L, level-of-detail cuts of octree packets (include/cwipc_util_amd/hip_ext.h), restated in numpy.  Written from the rule's
text, not from csrc/lod_terms.hpp; the tests hold the two, and the decoder's kernels, to each other byte for byte.

lod(P, t) is the "cwao" packet L(P, t); the hand-built packets the tests of all three layers share are made here too."""
import struct

import numpy as np

import codec_model as cm


def lod(packet, t):
    """L(P, t) of a valid "cwao" packet; ValueError for t outside 1 .. octree_bits."""
    info = cm.parse(packet)
    p, b, cb, n = bytes(packet), info["octree_bits"], info["colour_bits"], info["nleaves"]
    t = int(t)
    if not 1 <= t <= b:
        raise ValueError("the target is outside 1 .. octree_bits")
    if t == b:
        return p
    if n == 0:
        return struct.pack("<4sIQIBBBB3fId", cm.MAGIC, 1, info["timestamp"], 0, t, cb, 0, 0, 0.0, 0.0, 0.0, 0, 1.0) + bytes(4 * t)
    keys = cm.leaf_keys_of(p, info)
    stored = cm.unpack_bits(p[info["colour_offset"]:info["colour_offset"] + info["colour_bytes"]], 3 * n, cb).reshape(n, 3)
    if info["tile_mode"] == 1:
        tiles = np.frombuffer(p, dtype=np.uint8, count=n, offset=info["tile_offset"])
    else:
        tiles = np.full(n, info["tile_value"], dtype=np.uint8)
    # one leaf per distinct prefix of t triples; its members are a contiguous run of P's leaves
    prefix = keys >> np.uint64(3 * (b - t))
    new_keys, first, count = np.unique(prefix, return_index=True, return_counts=True)
    assert (np.diff(first) == count[:-1]).all() and first[0] == 0
    new_stored = np.zeros((len(new_keys), 3), dtype=np.int64)
    new_tiles = np.zeros(len(new_keys), dtype=np.uint8)
    for j, (a, c) in enumerate(zip(first.tolist(), count.tolist())):
        for ch in range(3):
            total = sum(int(v) for v in stored[a:a + c, ch])          # Python integers: exact for any run
            new_stored[j, ch] = (total + c // 2) // c
        new_tiles[j] = np.bitwise_or.reduce(tiles[a:a + c])
    # the header's minimum travels as the bits it has
    mn = np.frombuffer(p, dtype="<f4", count=3, offset=24)
    return cm.build_packet(new_keys, new_stored, new_tiles, mn, info["side"], t, cb, info["timestamp"])


def keys_of_cells(q, bits):
    return cm.keys(np.asarray(q, dtype=np.int64).reshape(-1, 3), bits)


def block_keys(origin, edge, bits):
    """The keys of the edge^3 cells from `origin` on, ascending."""
    r = np.arange(edge)
    q = np.stack(np.meshgrid(r, r, r, indexing="ij"), axis=-1).reshape(-1, 3) + np.asarray(origin)
    return np.sort(keys_of_cells(q, bits))


def hand_packets():
    """{name: "cwao" packet}: the hand-built trees of RULE L's tests."""
    rng = np.random.default_rng(77)
    mn, side = np.array([-1.0, 0.5, 2.0], dtype=np.float32), 3.0
    out = {}
    out["single leaf"] = cm.build_packet([0o1234567], [[200, 3, 77]], [5], mn, side, 7, 8, 11)
    # one node of depth 1 holding a full 16^3 block of leaves, all 255: the rounding and no overflow (4096 x 255 a channel)
    full = block_keys((0, 0, 0), 16, 5)
    out["full block of 255"] = cm.build_packet(full, np.full((len(full), 3), 255), np.full(len(full), 1), mn, side, 5, 8, 12)
    # a node with one leaf beside a node with 4096
    lone = keys_of_cells([[3, 2, 1]], 6)
    crowd = block_keys((32, 32, 32), 16, 6)
    k = np.concatenate([lone, crowd])
    out["1 beside 4096"] = cm.build_packet(k, rng.integers(0, 256, (len(k), 3)), rng.choice([1, 2, 4], len(k)), mn, side, 6, 8, 13)
    # every colour width, a leaf count that is no multiple of 32
    for cb, n in ((4, 1001), (5, 77), (7, 333), (8, 4099)):
        k = np.sort(rng.choice(1 << 15, n, replace=False).astype(np.uint64))
        out["cb %d, %d leaves" % (cb, n)] = cm.build_packet(k, rng.integers(0, 1 << cb, (n, 3)), rng.choice([1, 2, 4, 8], n), mn, side, 5, cb, 14)
    # tiles 1 and 2 mixed so that every new leaf of depth 2 ORs to 3: the plane goes away (mode 0, value 3)
    k = np.sort(np.concatenate([(np.uint64(p) << np.uint64(6)) | np.array([1, 40], dtype=np.uint64) for p in (0, 9, 10, 63)]))
    out["plane goes away"] = cm.build_packet(k, rng.integers(0, 64, (len(k), 3)), np.tile([1, 2], len(k) // 2), mn, side, 4, 6, 15)
    # a plane that stays
    k = np.sort(rng.choice(1 << 12, 700, replace=False).astype(np.uint64))
    tiles = np.where(k < np.uint64(1 << 11), 1, 2)
    out["plane stays"] = cm.build_packet(k, rng.integers(0, 256, (700, 3)), tiles, mn, side, 4, 8, 16)
    # tile_mode 0 in
    out["tile mode 0"] = cm.build_packet(k, rng.integers(0, 128, (700, 3)), np.full(700, 9), mn, side, 4, 7, 17, tile_mode=0)
    return out


def targets(bits):
    """The cuts the tests take of a packet of `bits`: 1, one in the middle, bits - 1, bits."""
    return sorted({1, max(1, bits // 2), max(1, bits - 1), bits})
