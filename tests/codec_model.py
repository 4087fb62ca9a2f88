"""RULE C of the octree codec (include/cwipc_util_amd/hip_ext.h) restated in numpy: encode, decode, validity.  Written from the
rule's text, not from csrc/codec_terms.hpp; the tests hold the two to each other byte for byte.  The input filters (tilenumber,
voxelsize) are the library's own calls and not part of this model: encode() takes the cloud after them.

A cloud is a structured array of the library's point dtype (x, y, z float32; r, g, b, tile uint8)."""
import struct

import numpy as np

POINT_DTYPE = np.dtype([('x', '<f4'), ('y', '<f4'), ('z', '<f4'), ('r', 'u1'), ('g', 'u1'), ('b', 'u1'), ('tile', 'u1')])
MAGIC = b"cwao"
HEADER = 48


class Invalid(ValueError):
    pass


def colour_shift(jpeg_quality):
    q = int(jpeg_quality)
    return 0 if q >= 90 else 1 if q >= 75 else 2 if q >= 50 else 3 if q >= 25 else 4


def colour_store(m, s):
    return int(m) >> s


def colour_load(v, s):
    return min(255, (int(v) << s) + ((1 << s) >> 1))


def finite_points(pts):
    keep = np.isfinite(pts['x']) & np.isfinite(pts['y']) & np.isfinite(pts['z'])
    return pts[keep]


def cube(P):
    """(min as float32[3], side as float64) of the points P (all finite, at least one)."""
    xyz = np.stack([P['x'], P['y'], P['z']], axis=1).astype(np.float32)
    mn = xyz.min(axis=0) + np.float32(0.0)          # a zero minimum is +0
    mx = xyz.max(axis=0)
    side = float((mx.astype(np.float64) - mn.astype(np.float64)).max())
    return mn.astype(np.float32), (side if side != 0.0 else 1.0)


def cells(P, mn, side, bits):
    """q[n, 3] as int64."""
    xyz = np.stack([P['x'], P['y'], P['z']], axis=1).astype(np.float64)
    u = (xyz - mn.astype(np.float64)) / np.float64(side)
    return np.minimum((1 << bits) - 1, np.floor(u * np.float64(1 << bits)).astype(np.int64))


def keys(q, bits):
    """The 3 bits-bit key per row of q, as Python-int-safe uint64."""
    k = np.zeros(len(q), dtype=np.uint64)
    for level in range(bits):                         # most significant triple first
        shift = bits - 1 - level
        triple = (((q[:, 0] >> shift) & 1) << 2) | (((q[:, 1] >> shift) & 1) << 1) | ((q[:, 2] >> shift) & 1)
        k = (k << np.uint64(3)) | triple.astype(np.uint64)
    return k


def pad4(n):
    return (n + 3) & ~3


def pack_bits(values, width):
    """values of `width` bits each, LSB first into bytes."""
    values = np.asarray(values, dtype=np.int64).reshape(-1)
    bits = ((values[:, None] >> np.arange(width)) & 1).astype(np.uint8).reshape(-1)
    return np.packbits(bits, bitorder="little").tobytes()


def unpack_bits(data, count, width):
    bits = np.unpackbits(np.frombuffer(data, dtype=np.uint8), bitorder="little")[:count * width].reshape(count, width).astype(np.int64)
    return (bits << np.arange(width)).sum(axis=1)


def encode(pts, octree_bits, jpeg_quality, timestamp=0):
    """The packet of the cloud `pts` (already tile-filtered and downsampled)."""
    b = int(octree_bits)
    assert 1 <= b <= 16 and 0 <= jpeg_quality <= 100
    s = colour_shift(jpeg_quality)
    P = finite_points(np.asarray(pts, dtype=POINT_DTYPE))
    if len(P) == 0:
        return struct.pack("<4sIQIBBBB3fId", MAGIC, 1, timestamp, 0, b, 8 - s, 0, 0, 0.0, 0.0, 0.0, 0, 1.0) + bytes(4 * b)
    mn, side = cube(P)
    k = keys(cells(P, mn, side, b), b)
    leaf_keys, inverse = np.unique(k, return_inverse=True)
    n = len(leaf_keys)
    count = np.bincount(inverse, minlength=n).astype(np.int64)
    stored = []
    for ch in ('r', 'g', 'b'):
        total = np.bincount(inverse, weights=P[ch].astype(np.float64), minlength=n).astype(np.int64)
        stored.append(((total + count // 2) // count) >> s)
    tiles = np.zeros(n, dtype=np.uint8)
    np.bitwise_or.at(tiles, inverse, P['tile'])
    return build_packet(leaf_keys, np.stack(stored, axis=1), tiles, mn, side, b, 8 - s, timestamp)


def build_packet(leaf_keys, stored_colours, tiles, mn, side, bits, colour_bits, timestamp, tile_mode=None):
    """The packet of a tree given by its leaves: `leaf_keys` ascending and distinct (at least one), `stored_colours` [n, 3] as the
    packet stores them (below 2^colour_bits), `tiles` [n].  `mn` goes into the header as the float32 bits it has (a -0.0 stays one).
    tile_mode None: the encoder's choice (0 when every leaf has the same tile); 0: the tiles must be equal; 1: a tile plane, whatever
    it holds.  Trees that no cloud produces are made this way, for the decoder."""
    b, cb = int(bits), int(colour_bits)
    leaf_keys = np.asarray(leaf_keys, dtype=np.uint64).reshape(-1)
    n = len(leaf_keys)
    stored = np.asarray(stored_colours, dtype=np.int64).reshape(n, 3)
    tiles = np.asarray(tiles, dtype=np.uint8).reshape(n)
    mn = np.asarray(mn, dtype=np.float32).reshape(3)
    assert 1 <= b <= 16 and 4 <= cb <= 8 and n >= 1 and (n == 1 or (leaf_keys[1:] > leaf_keys[:-1]).all())
    assert int(leaf_keys[-1]) < (1 << (3 * b)) and stored.min() >= 0 and stored.max() < (1 << cb)
    # nodes[L] and the occupancy bytes, depth by depth
    nodes, occupancy = [], bytearray()
    for depth in range(b):
        child_prefixes = np.unique(leaf_keys >> np.uint64(3 * (b - 1 - depth)))
        nodes.append(len(child_prefixes))
        parents, where = np.unique(child_prefixes >> np.uint64(3), return_inverse=True)
        byte = np.zeros(len(parents), dtype=np.uint8)
        np.bitwise_or.at(byte, where, (np.uint8(1) << (child_prefixes & np.uint64(7)).astype(np.uint8)))
        occupancy += byte.tobytes()
    assert len(occupancy) == 1 + sum(nodes[:-1]) and nodes[-1] == n
    occupancy += bytes(pad4(len(occupancy)) - len(occupancy))
    colours = pack_bits(stored.reshape(-1), cb)
    colours += bytes(pad4(len(colours)) - len(colours))
    uniform = bool((tiles == tiles[0]).all())
    if tile_mode is None:
        tile_mode = 0 if uniform else 1
    assert tile_mode == 1 or (tile_mode == 0 and uniform)
    header = struct.pack("<4sIQIBBBB", MAGIC, 1, timestamp, n, b, cb, tile_mode, 0 if tile_mode else int(tiles[0])) + mn.astype('<f4').tobytes() + \
        struct.pack("<Id", 0, side)
    return header + struct.pack("<%dI" % b, *nodes) + bytes(occupancy) + colours + (tiles.tobytes() if tile_mode else b"")


def parse(packet):
    """The validity test; returns the header as a dict with the offsets of the parts, raises Invalid with the reason."""
    p = bytes(packet)
    if len(p) < HEADER:
        raise Invalid("truncated header")
    magic, version, ts, n, b, cb, mode, tile_value, mnx, mny, mnz, zero, side = struct.unpack("<4sIQIBBBB3fId", p[:HEADER])
    if magic != MAGIC:
        raise Invalid("magic")
    if version != 1:
        raise Invalid("version")
    if not 1 <= b <= 16 or not 4 <= cb <= 8 or mode > 1 or zero != 0 or (mode == 1 and tile_value != 0):
        raise Invalid("range")
    if not all(np.isfinite([mnx, mny, mnz, side])) or not side > 0:
        raise Invalid("cube")
    if len(p) < HEADER + 4 * b:
        raise Invalid("truncated node counts")
    nodes = list(struct.unpack("<%dI" % b, p[HEADER:HEADER + 4 * b]))
    if nodes[-1] != n:
        raise Invalid("leaf count")
    if n == 0:
        if any(nodes) or mode or tile_value or p[24:36] != bytes(12) or side != 1.0:
            raise Invalid("empty cloud")
        occ_bytes = 0
    else:
        if not 1 <= nodes[0] <= 8 or any(nodes[i + 1] > 8 * nodes[i] or nodes[i + 1] < nodes[i] for i in range(b - 1)):
            raise Invalid("node counts")
        occ_bytes = 1 + sum(nodes[:-1])
    occ_at = HEADER + 4 * b
    col_at = occ_at + pad4(occ_bytes)
    col_bytes = (n * 3 * cb + 7) // 8
    tile_at = col_at + pad4(col_bytes)
    total = tile_at + (n if mode == 1 else 0)
    if len(p) != total:
        raise Invalid("length")
    at = occ_at
    for depth in range(b if n else 0):
        cnt = 1 if depth == 0 else nodes[depth - 1]
        level = np.frombuffer(p, dtype=np.uint8, count=cnt, offset=at)
        if (level == 0).any():
            raise Invalid("occupancy byte 0")
        if int(np.unpackbits(level).sum()) != nodes[depth]:
            raise Invalid("popcount")
        at += cnt
    if any(p[occ_at + occ_bytes:col_at]) or any(p[col_at + col_bytes:tile_at]):
        raise Invalid("padding")
    if (n * 3 * cb) % 8 and p[col_at + col_bytes - 1] >> ((n * 3 * cb) % 8):
        raise Invalid("padding")
    return dict(timestamp=ts, nleaves=n, octree_bits=b, colour_bits=cb, tile_mode=mode, tile_value=tile_value,
                min=np.array([mnx, mny, mnz], dtype=np.float32), side=side, nodes=nodes, occupancy_offset=occ_at, occupancy_bytes=occ_bytes,
                colour_offset=col_at, colour_bytes=col_bytes, tile_offset=tile_at, total_bytes=total)


def leaf_keys_of(packet, info=None):
    """The leaves' keys, in order, from the occupancy bytes."""
    info = info or parse(packet)
    p, b = bytes(packet), info["octree_bits"]
    prefixes = np.zeros(1, dtype=np.uint64)
    at = info["occupancy_offset"]
    for depth in range(b if info["nleaves"] else 0):
        level = np.frombuffer(p, dtype=np.uint8, count=len(prefixes), offset=at)
        at += len(prefixes)
        bits = np.unpackbits(level.reshape(-1, 1), axis=1, bitorder="little")      # [node, child]
        node, child = np.nonzero(bits)
        prefixes = (prefixes[node] << np.uint64(3)) | child.astype(np.uint64)
    return prefixes if info["nleaves"] else np.zeros(0, dtype=np.uint64)


def decode(packet):
    """(points, timestamp, cellsize as float32)."""
    info = parse(packet)
    p, b, n, cb = bytes(packet), info["octree_bits"], info["nleaves"], info["colour_bits"]
    s = 8 - cb
    cell = np.float64(info["side"]) / np.float64(1 << b)
    out = np.zeros(n, dtype=POINT_DTYPE)
    if n:
        lk = leaf_keys_of(p, info)
        q = np.zeros((n, 3), dtype=np.int64)
        for level in range(b):
            triple = ((lk >> np.uint64(3 * (b - 1 - level))) & np.uint64(7)).astype(np.int64)
            for a in range(3):
                q[:, a] = (q[:, a] << 1) | ((triple >> (2 - a)) & 1)
        mn = info["min"].astype(np.float64)
        with np.errstate(over="ignore"):             # a side above float32's range: the rule's (float) gives infinity, and so does this
            xyz = (mn + (q.astype(np.float64) + 0.5) * cell).astype(np.float32)
        out['x'], out['y'], out['z'] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
        vals = unpack_bits(p[info["colour_offset"]:info["colour_offset"] + info["colour_bytes"]], 3 * n, cb).reshape(n, 3)
        dec = np.minimum(255, (vals << s) + ((1 << s) >> 1)).astype(np.uint8)
        out['r'], out['g'], out['b'] = dec[:, 0], dec[:, 1], dec[:, 2]
        if info["tile_mode"] == 1:
            out['tile'] = np.frombuffer(p, dtype=np.uint8, count=n, offset=info["tile_offset"])
        else:
            out['tile'] = info["tile_value"]
    with np.errstate(over="ignore", under="ignore"):
        return out, info["timestamp"], np.float32(cell)


def make_cloud(xyz, rgb=None, tile=None):
    xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    pts = np.zeros(len(xyz), dtype=POINT_DTYPE)
    pts['x'], pts['y'], pts['z'] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    if rgb is not None:
        rgb = np.asarray(rgb, dtype=np.uint8).reshape(-1, 3)
        pts['r'], pts['g'], pts['b'] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    if tile is not None:
        pts['tile'] = tile
    return pts


def random_cloud(rng, n, scale=1.0, offset=(0.0, 0.0, 0.0), tiles=(1, 2, 4)):
    pts = make_cloud(rng.uniform(-1.0, 1.0, (n, 3)) * scale + np.asarray(offset), rng.integers(0, 256, (n, 3)))
    pts['tile'] = rng.choice(np.asarray(tiles, dtype=np.uint8), n)
    return pts


# ---------------------------------------------------------------------------
# test material: clouds aimed at the cell boundaries, and the near misses of the cell rule they must tell from it
# ---------------------------------------------------------------------------
def boundary_cloud(mn, mx, bits, rng):
    """A cloud whose cube is [mn, mx]^3 (mn < mx, both float32) and whose coordinates lie on the cell boundaries of `bits` bits, as
    closely as float32 allows: for every boundary k in 0 .. 2^bits (4096 of the inner ones, drawn by rng, plus both ends when there
    are more than 8192) the float32 nearest to mn + k side / 2^bits, worked out in extended precision, and its two float32
    neighbours, those inside [mn, mx].  Every axis gets all candidates, each in an order of its own; colours and tiles are random;
    the last two points are the corners that pin the cube."""
    mn, mx = np.float32(mn), np.float32(mx)
    assert mn < mx
    total = 1 << int(bits)
    if total > 8192:
        k = np.concatenate([[0, total], 1 + rng.choice(total - 1, 4096, replace=False)])
    else:
        k = np.arange(total + 1)
    k = np.sort(k).astype(np.longdouble)
    side = np.longdouble(mx) - np.longdouble(mn)
    centre = (np.longdouble(mn) + k * side / np.longdouble(total)).astype(np.float32)
    cand = np.unique(np.concatenate([np.nextafter(centre, np.float32(-np.inf)), centre, np.nextafter(centre, np.float32(np.inf))]))
    cand = cand[(cand >= mn) & (cand <= mx)]
    xyz = np.stack([cand[rng.permutation(len(cand))] for _ in range(3)], axis=1)
    xyz = np.concatenate([xyz, [[mn, mn, mn], [mx, mx, mx]]]).astype(np.float32)
    pts = make_cloud(xyz, rng.integers(0, 256, (len(xyz), 3)))
    pts['tile'] = rng.choice(np.array([1, 2, 4], dtype=np.uint8), len(xyz))
    return pts


CELL_VARIANTS = ("recip", "scale", "sub32", "div32")


def cells_variant(P, mn, side, bits, name):
    """cells() as a kernel might compute it by mistake.  recip: (p - min) * (1 / side); scale: (p - min) * (2^b / side), one factor;
    sub32: the subtraction in float32; div32: the subtraction and the division in float32.  None of them is the rule: the tests'
    inputs must be able to tell each of them from it."""
    xyz32 = np.stack([P['x'], P['y'], P['z']], axis=1).astype(np.float32)
    mn32, side, two_b = np.asarray(mn, dtype=np.float32), np.float64(side), np.float64(1 << bits)
    d = xyz32.astype(np.float64) - mn32.astype(np.float64)
    if name == "recip":
        f = (d * (np.float64(1.0) / side)) * two_b
    elif name == "scale":
        f = d * (two_b / side)
    elif name == "sub32":
        f = ((xyz32 - mn32).astype(np.float64) / side) * two_b
    elif name == "div32":
        f = ((xyz32 - mn32) / np.float32(side)).astype(np.float64) * two_b
    else:
        raise ValueError(name)
    return np.minimum((1 << bits) - 1, np.floor(f).astype(np.int64))
