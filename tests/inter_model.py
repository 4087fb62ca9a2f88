"""RULE P of the octree codec (include/cwipc_util_amd/hip_ext.h) restated in numpy: key and delta packets ("cwap"), the cube of a
GOP, the sequence rules.  Written from the rule's text, not from csrc/inter_terms.hpp; the tests hold the two, and the kernels, to
each other byte for byte.  RULE C and RULE E come from codec_model and entropy_model, which this module only imports."""
import struct

import numpy as np

import codec_model as cm
import entropy_model as em

MAGIC = b"cwap"
PREFIX = 32
KEY, DELTA = 0, 1


class Invalid(ValueError):
    pass


def inter_on(do_inter_frame, gop_size, exp_factor):
    return bool(do_inter_frame) and 2 <= gop_size <= 65535 and bool(np.isfinite(exp_factor)) and 1.0 <= exp_factor <= 16.0


# ---------------------------------------------------------------------------
# the cube
# ---------------------------------------------------------------------------
def expand_cube(mn, side, exp_factor):
    """(min', side') of a key frame from RULE C's cube."""
    side = np.float64(side)
    grown = side * np.float64(np.float32(exp_factor))
    margin = (grown - side) * np.float64(0.5)
    mn2 = (np.asarray(mn, dtype=np.float32).astype(np.float64) - margin).astype(np.float32) + np.float32(0.0)
    return mn2.astype(np.float32), float(grown)


def extremes(P):
    xyz = np.stack([P['x'], P['y'], P['z']], axis=1).astype(np.float32)
    return xyz.min(axis=0), xyz.max(axis=0)


def contained(lo, hi, mn, side):
    lo, hi, mn = (np.asarray(v, dtype=np.float32) for v in (lo, hi, mn))
    if not (lo >= mn).all():
        return False
    u = (hi.astype(np.float64) - mn.astype(np.float64)) / np.float64(side)
    return bool((u <= 1.0).all())


def encode_in_cube(pts, mn, side, octree_bits, jpeg_quality, timestamp=0):
    """RULE C's packet of the cloud (at least one finite point, contained) quantised in the cube (mn, side)."""
    b, s = int(octree_bits), cm.colour_shift(jpeg_quality)
    P = cm.finite_points(np.asarray(pts, dtype=cm.POINT_DTYPE))
    k = cm.keys(cm.cells(P, np.asarray(mn, dtype=np.float32), side, b), b)
    leaf_keys, inverse = np.unique(k, return_inverse=True)
    n = len(leaf_keys)
    count = np.bincount(inverse, minlength=n).astype(np.int64)
    stored = []
    for ch in ('r', 'g', 'b'):
        total = np.bincount(inverse, weights=P[ch].astype(np.float64), minlength=n).astype(np.int64)
        stored.append(((total + count // 2) // count) >> s)
    tiles = np.zeros(n, dtype=np.uint8)
    np.bitwise_or.at(tiles, inverse, P['tile'])
    return cm.build_packet(leaf_keys, np.stack(stored, axis=1), tiles, mn, side, b, 8 - s, timestamp)


# ---------------------------------------------------------------------------
# leaves of a cwao packet
# ---------------------------------------------------------------------------
def leaves_of(packet):
    """(info, keys, stored colours [n, 3], tiles [n]) of a valid cwao packet; the tiles are the tile value without a plane."""
    p = bytes(packet)
    info = cm.parse(p)
    n, cb = info["nleaves"], info["colour_bits"]
    keys = cm.leaf_keys_of(p, info)
    col = cm.unpack_bits(p[info["colour_offset"]:info["colour_offset"] + info["colour_bytes"]], 3 * n, cb).reshape(n, 3)
    if info["tile_mode"] == 1:
        tiles = np.frombuffer(p, dtype=np.uint8, count=n, offset=info["tile_offset"]).copy()
    else:
        tiles = np.full(n, info["tile_value"], dtype=np.uint8)
    return info, keys, col, tiles


def tree_of(keys, b):
    """(nodes[b], occupancy bytes per depth) of the tree with the leaves `keys` (ascending, distinct, at least one)."""
    keys = np.asarray(keys, dtype=np.uint64)
    nodes, levels = [], []
    for depth in range(b):
        child = np.unique(keys >> np.uint64(3 * (b - 1 - depth)))
        nodes.append(len(child))
        parents, where = np.unique(child >> np.uint64(3), return_inverse=True)
        byte = np.zeros(len(parents), dtype=np.uint8)
        np.bitwise_or.at(byte, where, (np.uint8(1) << (child & np.uint64(7)).astype(np.uint8)))
        levels.append(byte)
    return nodes, levels


def predictor(rkeys, pkeys):
    """(pred[j], found[j]) for every key of pkeys in the ascending rkeys."""
    ub = np.searchsorted(rkeys, pkeys, side="right")
    pred = np.maximum(0, ub - 1)
    found = (ub > 0) & (rkeys[pred] == pkeys)
    return pred, found


# ---------------------------------------------------------------------------
# packets
# ---------------------------------------------------------------------------
def prefix(kind, gop_index=0, ref_timestamp=0, ref_nleaves=0):
    return MAGIC + struct.pack("<IIIQII", 1, kind, gop_index, ref_timestamp, ref_nleaves, 0)


def key_packet(embedded):
    return prefix(KEY) + bytes(embedded)


def _payload(kind, values, cb):
    """(mode, payload) by RULE E's mode rule, without its colour prediction.  kind: "bytes" (raw as it is) or "bits" (raw at cb bits)."""
    values = np.asarray(values, dtype=np.int64)
    raw = em.raw_payload("colour" if kind == "bits" else "tile", values, cb)
    if len(values) >= em.BLOCK:
        f = em.normalise(np.bincount(values, minlength=256))
        blocks = [em.block_bytes(st, w) for st, w in em.encode_blocks(values, f)]
        coded = f.astype("<u2").tobytes() + struct.pack("<%dI" % len(blocks), *[len(x) for x in blocks]) + b"".join(blocks)
        if len(coded) < len(raw):
            return 1, coded
    return 0, raw


def delta_streams(R, P, overlap=False):
    """(header info of P, nadded, nodesA, [(kind, values)]) of the delta of the cwao packet P against the cwao packet R.
    overlap: not the rule -- the first kept leaf is listed among the added ones instead (test material: the counts still add up)."""
    ri, rk, rc, rt = leaves_of(R)
    pi, pk, pc, pt = leaves_of(P)
    assert ri["nleaves"] > 0 and pi["nleaves"] > 0
    assert (ri["octree_bits"], ri["colour_bits"], ri["side"]) == (pi["octree_bits"], pi["colour_bits"], pi["side"])
    assert ri["min"].tobytes() == pi["min"].tobytes()
    b, cb, nr = pi["octree_bits"], pi["colour_bits"], ri["nleaves"]
    pred, found = predictor(rk, pk)
    if overlap:
        found = found.copy()
        found[np.nonzero(found)[0][0]] = False
    keepbits = np.zeros(8 * ((nr + 7) // 8), dtype=np.uint8)
    keepbits[pred[found]] = 1
    streams = [("bytes", np.packbits(keepbits, bitorder="little").astype(np.int64))]
    added = pk[~found]
    nodes = [0] * b
    if len(added):
        nodes, levels = tree_of(added, b)
        streams += [("bytes", lv.astype(np.int64)) for lv in levels]
    for ch in range(3):
        streams.append(("bits", (pc[:, ch] - rc[pred, ch]) & ((1 << cb) - 1)))
    if pi["tile_mode"] == 1:
        streams.append(("bytes", (pt ^ rt[pred]).astype(np.int64)))
    return pi, len(added), nodes, streams


def diff(P, R, gop_index=1, overlap=False):
    """The delta packet of the cwao packet P against the cwao packet R."""
    P, R = bytes(P), bytes(R)
    ri = cm.parse(R)
    pi, nadded, nodes, streams = delta_streams(R, P, overlap)
    made = [_payload(kind, values, pi["colour_bits"]) for kind, values in streams]
    out = prefix(DELTA, gop_index, ri["timestamp"], ri["nleaves"]) + P[8:48] + struct.pack("<I", nadded) + struct.pack("<%dI" % pi["octree_bits"], *nodes)
    out += struct.pack("<I", len(made)) + b"".join(struct.pack("<II", mode, len(payload)) for mode, payload in made)
    return out + b"".join(payload for _, payload in made)


def parse(packet, reference=None):
    """The container test of a cwap packet.  reference: None, or the cwao packet a decoder holds (b"" for none held)."""
    p = bytes(packet)
    if len(p) < PREFIX:
        raise Invalid("truncated prefix")
    if p[:4] != MAGIC:
        raise Invalid("magic")
    version, kind, gop_index, ref_ts, ref_n, zero = struct.unpack("<IIIQII", p[4:PREFIX])
    if version != 1 or kind > 1 or zero != 0:
        raise Invalid("prefix")
    out = dict(kind=kind, gop_index=gop_index, ref_timestamp=ref_ts, ref_nleaves=ref_n)
    if kind == KEY:
        if gop_index or ref_ts or ref_n:
            raise Invalid("key packet names a reference")
        q = p[PREFIX:]
        try:
            out["embedded"] = em.parse(q) if q[:4] == em.MAGIC else cm.parse(q)
        except (cm.Invalid, em.Invalid) as e:
            raise Invalid(str(e))
        out["entropy"] = q[:4] == em.MAGIC
        return out
    if not 1 <= gop_index <= 65534 or ref_n == 0:
        raise Invalid("delta prefix")
    if len(p) < PREFIX + 40 + 4:
        raise Invalid("truncated header")
    ts, n, b, cb, mode, tile_value, mnx, mny, mnz, zero, side = struct.unpack("<QIBBBB3fId", p[PREFIX:PREFIX + 40])
    if not 1 <= b <= 16 or not 4 <= cb <= 8 or mode > 1 or zero != 0 or (mode == 1 and tile_value != 0):
        raise Invalid("range")
    if not all(np.isfinite([mnx, mny, mnz, side])) or not side > 0:
        raise Invalid("cube")
    if n == 0:
        raise Invalid("empty delta")
    nadded = struct.unpack("<I", p[PREFIX + 40:PREFIX + 44])[0]
    if nadded > n or n - nadded > ref_n:
        raise Invalid("added leaves")
    at = PREFIX + 44
    if len(p) < at + 4 * b:
        raise Invalid("truncated node counts")
    nodes = list(struct.unpack("<%dI" % b, p[at:at + 4 * b]))
    if nadded == 0:
        if any(nodes):
            raise Invalid("node counts without added leaves")
    elif nodes[-1] != nadded or not 1 <= nodes[0] <= 8 or any(nodes[i + 1] > 8 * nodes[i] or nodes[i + 1] < nodes[i] for i in range(b - 1)):
        raise Invalid("node counts")
    at += 4 * b
    kinds = [("keep", 0, (ref_n + 7) // 8)]
    if nadded:
        kinds += [("occupancy", d, 1 if d == 0 else nodes[d - 1]) for d in range(b)]
    kinds += [("colour", ch, n) for ch in range(3)]
    if mode == 1:
        kinds.append(("tile", 0, n))
    if len(p) < at + 4:
        raise Invalid("truncated stream count")
    if struct.unpack("<I", p[at:at + 4])[0] != len(kinds):
        raise Invalid("stream count")
    directory = at + 4
    at = directory + 8 * len(kinds)
    if len(p) < at:
        raise Invalid("truncated directory")
    streams = []
    for i, (kind_, which, count) in enumerate(kinds):
        smode, size = struct.unpack("<II", p[directory + 8 * i:directory + 8 * i + 8])
        used = (count * cb + 7) // 8 if kind_ == "colour" else count
        nblocks = (count + em.BLOCK - 1) // em.BLOCK
        if smode > 1:
            raise Invalid("mode")
        if smode == 0 and size != cm.pad4(used):
            raise Invalid("raw payload size")
        if smode == 1 and (count < em.BLOCK or size % 4 or size < 512 + nblocks * 260 or size >= cm.pad4(used)):
            raise Invalid("coded payload size")
        streams.append(dict(kind=kind_, which=which, symbols=count, mode=smode, offset=at, bytes=size, nblocks=nblocks, used=used))
        at += size
    if len(p) != at:
        raise Invalid("length")
    for s in streams:
        q = p[s["offset"]:s["offset"] + s["bytes"]]
        if s["mode"] == 0:
            if any(q[s["used"]:]):
                raise Invalid("padding")
            if s["kind"] == "colour" and (s["symbols"] * cb) % 8 and q[s["used"] - 1] >> ((s["symbols"] * cb) % 8):
                raise Invalid("padding")
            if s["kind"] == "occupancy":
                _occupancy_rules(np.frombuffer(q, dtype=np.uint8, count=s["symbols"]), nodes[s["which"]])
            continue
        f = np.frombuffer(q, dtype="<u2", count=256).astype(np.int64)
        if f.sum() != em.M:
            raise Invalid("frequencies do not sum to 4096")
        if s["kind"] == "occupancy" and f[0]:
            raise Invalid("occupancy byte 0 has a frequency")
        if s["kind"] == "colour" and f[1 << cb:].any():
            raise Invalid("colour value above its bits")
        sizes = np.frombuffer(q, dtype="<u4", count=s["nblocks"], offset=512).astype(np.int64)
        if (sizes % 4).any() or (sizes < 256).any() or (sizes > 256 + 2 * em.BLOCK).any() or sizes.sum() != s["bytes"] - 512 - 4 * s["nblocks"]:
            raise Invalid("block sizes")
        s["f"], s["block_bytes"] = f, sizes
        s["block_offsets"] = s["offset"] + 512 + 4 * s["nblocks"] + np.concatenate([[0], np.cumsum(sizes)[:-1]])
    out.update(timestamp=ts, nleaves=n, octree_bits=b, colour_bits=cb, tile_mode=mode, tile_value=tile_value,
               min=np.array([mnx, mny, mnz], dtype=np.float32), side=side, nadded=nadded, nodes_added=nodes, streams=streams,
               directory_offset=directory - 4)
    if reference is not None:
        if not reference:
            raise Invalid("no reference is held")
        ri = cm.parse(reference)
        if ri["nleaves"] == 0 or (ri["timestamp"], ri["nleaves"]) != (ref_ts, ref_n):
            raise Invalid("wrong reference")
        if (ri["octree_bits"], ri["colour_bits"]) != (b, cb) or ri["min"].tobytes() != out["min"].tobytes() or struct.pack("<d", ri["side"]) != struct.pack("<d", side):
            raise Invalid("wrong reference cube")
    return out


def _occupancy_rules(level, children):
    if (level == 0).any():
        raise Invalid("occupancy byte 0")
    if int(np.unpackbits(level).sum()) != children:
        raise Invalid("popcount")


def _stream_values(p, s, cb):
    q = p[s["offset"]:s["offset"] + s["bytes"]]
    if s["mode"] == 0:
        return cm.unpack_bits(q, s["symbols"], cb) if s["kind"] == "colour" else np.frombuffer(q, dtype=np.uint8, count=s["symbols"]).astype(np.int64)
    blocks = [(np.frombuffer(p, dtype="<u4", count=em.LANES, offset=int(at)), np.frombuffer(p, dtype="<u2", count=(int(size) - 256) // 2, offset=int(at) + 256))
              for at, size in zip(s["block_offsets"], s["block_bytes"])]
    counts = [min(em.BLOCK, s["symbols"] - em.BLOCK * k) for k in range(s["nblocks"])]
    values, intact = em.decode_blocks(blocks, counts, s["f"])
    if not intact.all():
        raise Invalid("block not intact")
    return values


def apply(D, R):
    """The cwao packet the cwap packet D stands for after the cwao packet R; a key packet's embedded packet verbatim."""
    p = bytes(D)
    if parse(p)["kind"] == KEY:
        return p[PREFIX:]
    info = parse(p, bytes(R) if R is not None else b"")
    ri, rk, rc, rt = leaves_of(R)
    b, cb, n, nr, nadded = info["octree_bits"], info["colour_bits"], info["nleaves"], ri["nleaves"], info["nadded"]
    values = [_stream_values(p, s, cb) for s in info["streams"]]
    for s, v in zip(info["streams"], values):
        if s["kind"] == "occupancy" and s["mode"] == 1:
            _occupancy_rules(v.astype(np.uint8), info["nodes_added"][s["which"]])
    keepbits = np.unpackbits(values[0].astype(np.uint8), bitorder="little")
    if keepbits[nr:].any():
        raise Invalid("keep padding bits")
    if int(keepbits.sum()) + nadded != n:
        raise Invalid("kept and added leaves differ from the leaf count")
    added = np.zeros(1 if nadded else 0, dtype=np.uint64)
    for depth in range(b if nadded else 0):
        bits = np.unpackbits(values[1 + depth].astype(np.uint8).reshape(-1, 1), axis=1, bitorder="little")
        node, child = np.nonzero(bits)
        added = (added[node] << np.uint64(3)) | child.astype(np.uint64)
    if np.isin(added, rk).any():
        raise Invalid("an added leaf is a leaf of the reference")
    pk = np.sort(np.concatenate([rk[keepbits[:nr].astype(bool)], added]))
    pred, _ = predictor(rk, pk)
    first = 1 + (b if nadded else 0)
    stored = np.stack([(rc[pred, ch] + values[first + ch]) & ((1 << cb) - 1) for ch in range(3)], axis=1)
    if info["tile_mode"] == 1:
        tiles = (rt[pred] ^ values[first + 3].astype(np.uint8)).astype(np.uint8)
    else:
        tiles = np.full(n, info["tile_value"], dtype=np.uint8)
    return cm.build_packet(pk, stored, tiles, info["min"], info["side"], b, cb, info["timestamp"], tile_mode=info["tile_mode"])


# ---------------------------------------------------------------------------
# the sequence
# ---------------------------------------------------------------------------
class Encoder:
    """An inter-mode encoder as the rule states it: feed(cloud, timestamp) returns the cwap packet."""

    def __init__(self, gop_size, exp_factor, octree_bits=9, jpeg_quality=85, entropy=False):
        assert inter_on(True, gop_size, exp_factor)
        self.gop, self.exp, self.bits, self.quality, self.entropy = gop_size, np.float32(exp_factor), octree_bits, jpeg_quality, entropy
        self.g, self.reference, self.cube = 0, None, None
        self.kinds = []

    def at_gop_boundary(self):
        return self.g == 0 or self.reference is None

    def feed(self, pts, timestamp=0):
        P = cm.finite_points(np.asarray(pts, dtype=cm.POINT_DTYPE))
        empty = len(P) == 0
        key = self.g == 0 or self.reference is None or empty or not contained(*extremes(P), *self.cube)
        if key:
            self.g = 0
            if empty:
                packet = cm.encode(P, self.bits, self.quality, timestamp)
                self.reference = None
            else:
                self.cube = expand_cube(*cm.cube(P), self.exp)
                packet = encode_in_cube(P, *self.cube, self.bits, self.quality, timestamp)
                self.reference = packet
            out = key_packet(em.pack(packet) if self.entropy else packet)
        else:
            packet = encode_in_cube(P, *self.cube, self.bits, self.quality, timestamp)
            out = diff(packet, self.reference, self.g)
            self.reference = packet
        self.kinds.append(KEY if key else DELTA)
        self.intra = packet            # the same frame coded on its own in the same cube
        self.g = (self.g + 1) % self.gop
        return out


class Decoder:
    """feed(packet) returns the cwao packet it stands for; a cwap packet leaves a reference, other packets leave it alone."""

    def __init__(self):
        self.reference = None

    def feed(self, packet):
        p = bytes(packet)
        if p[:4] != MAGIC:
            return em.unpack(p) if p[:4] == em.MAGIC else p
        info = parse(p)
        if info["kind"] == KEY:
            q = p[PREFIX:]
            out = em.unpack(q) if info["entropy"] else q
        else:
            out = apply(p, self.reference)
        self.reference = out if cm.parse(out)["nleaves"] else None
        return out


# ---------------------------------------------------------------------------
# test material
# ---------------------------------------------------------------------------
def damages(packet, reference):
    """(what, bytes) for damages of a delta packet that the CONTAINER test must refuse (with `reference` held)."""
    p = bytes(packet)
    info = parse(p, reference)
    b = info["octree_bits"]
    counts = PREFIX + 40
    directory = info["directory_offset"]
    streams = info["streams"]
    out = []

    def put(what, at, data):
        out.append((what, p[:at] + data + p[at + len(data):]))

    edges = {0, 4, 31, PREFIX, PREFIX + 39, counts, counts + 4, directory, directory + 4, directory + 4 + 8 * len(streams), len(p) - 1}
    for s in streams:
        edges |= {s["offset"], s["offset"] + s["bytes"] - 1}
    for at in sorted(edges):
        if 0 <= at < len(p):
            out.append((f"truncated at {at}", p[:at]))
    out.append(("one byte appended", p + b"\x00"))
    out.append(("four bytes appended", p + bytes(4)))
    put("magic of the plain packet", 0, cm.MAGIC)
    put("magic", 0, b"cwaP")
    put("version", 4, struct.pack("<I", 2))
    put("kind 2", 8, struct.pack("<I", 2))
    put("kind key", 8, struct.pack("<I", 0))
    put("gop_index 0", 12, struct.pack("<I", 0))
    put("gop_index 65535", 12, struct.pack("<I", 65535))
    put("ref_timestamp + 1", 16, struct.pack("<Q", info["ref_timestamp"] + 1))
    put("ref_nleaves + 8", 24, struct.pack("<I", info["ref_nleaves"] + 8))
    put("ref_nleaves 0", 24, struct.pack("<I", 0))
    put("prefix reserved word", 28, struct.pack("<I", 1))
    put("nleaves 0", PREFIX + 8, struct.pack("<I", 0))
    put("nleaves + 64", PREFIX + 8, struct.pack("<I", info["nleaves"] + 64))
    put("octree_bits 0", PREFIX + 12, b"\x00")
    put("octree_bits + 1", PREFIX + 12, bytes([b + 1]))
    put("octree_bits 17", PREFIX + 12, b"\x11")
    put("colour bits 9", PREFIX + 13, b"\x09")
    put("colour bits other", PREFIX + 13, bytes([4 if info["colour_bits"] != 4 else 5]))
    put("tile mode 2", PREFIX + 14, b"\x02")
    put("tile mode flipped", PREFIX + 14, bytes([1 - info["tile_mode"], 0]))
    if info["tile_mode"] == 1:
        put("tile value with a plane", PREFIX + 15, b"\x01")
    put("min x nan", PREFIX + 16, struct.pack("<f", np.nan))
    put("min y moved", PREFIX + 20, struct.pack("<f", float(info["min"][1]) + 1.0))
    put("reserved word", PREFIX + 28, b"\x01")
    put("side 0", PREFIX + 32, struct.pack("<d", 0.0))
    put("side doubled", PREFIX + 32, struct.pack("<d", 2 * info["side"]))
    put("nadded + 1", counts, struct.pack("<I", info["nadded"] + 1))
    put("nadded above nleaves", counts, struct.pack("<I", info["nleaves"] + 1))
    if info["nadded"]:
        put("nadded 0", counts, struct.pack("<I", 0))
        put("nodesA[0] 0", counts + 4, struct.pack("<I", 0))
        put("nodesA[0] 9", counts + 4, struct.pack("<I", 9))
        put("nodesA last + 1", counts + 4 * b, struct.pack("<I", info["nodes_added"][-1] + 1))
    else:
        put("nodesA without added leaves", counts + 4, struct.pack("<I", 1))
    for delta in (1, -1):
        put(f"S {delta:+d}", directory, struct.pack("<I", len(streams) + delta))
    for i, s in enumerate(streams):
        entry = directory + 4 + 8 * i
        put(f"stream {i} mode 2", entry, struct.pack("<I", 2))
        put(f"stream {i} mode flipped", entry, struct.pack("<I", 1 - s["mode"]))
        for delta in (4, -4, 1):
            if s["bytes"] + delta >= 0:
                put(f"stream {i} payload_bytes {delta:+d}", entry + 4, struct.pack("<I", s["bytes"] + delta))
        at = s["offset"]
        if s["mode"] == 0:
            for pad in range(at + s["used"], at + s["bytes"]):
                put(f"stream {i} pad byte", pad, b"\x01")
            if s["kind"] == "colour" and (s["symbols"] * info["colour_bits"]) % 8:
                put(f"stream {i} pad bits", at + s["used"] - 1, bytes([p[at + s["used"] - 1] | 0x80]))
            if s["kind"] == "occupancy":
                put(f"stream {i} raw occupancy byte 0", at, b"\x00")
                put(f"stream {i} raw occupancy bit flipped", at, bytes([p[at] ^ 1 if p[at] != 1 else 3]))
            continue
        f = s["f"]
        top = int(np.argmax(f))
        for delta in (1, -1):
            put(f"stream {i} sum f {delta:+d}", at + 2 * top, struct.pack("<H", int(f[top]) + delta))
        k = s["nblocks"] - 1
        size_at, size = at + 512 + 4 * k, int(s["block_bytes"][k])
        for what, value in (("odd", size + 1), ("off by two", size + 2), ("too small", 252), ("too large", 256 + 2 * em.BLOCK + 4), ("+4", size + 4)):
            put(f"stream {i} block_bytes {what}", size_at, struct.pack("<I", value))
    return out


def payload_damages(packet, reference):
    """(what, bytes) for damages that the container test ACCEPTS and applying the delta must refuse: coded blocks, keep's padding
    bits and count, an added leaf that the reference has."""
    p = bytes(packet)
    info = parse(p, reference)
    out = []
    for i, s in enumerate(info["streams"]):
        if s["mode"] != 1:
            continue
        k = s["nblocks"] - 1
        at, size = int(s["block_offsets"][k]), int(s["block_bytes"][k])
        out.append((f"stream {i} state below 2^16", p[:at + 8] + struct.pack("<I", 0xffff) + p[at + 12:]))
        out.append((f"stream {i} state 0xffffffff", p[:at + 4 * 63] + struct.pack("<I", 0xffffffff) + p[at + 4 * 64:]))
        if size > 256 + 4:
            w = at + 256
            out.append((f"stream {i} word flipped", p[:w] + bytes([p[w] ^ 0x5a, p[w + 1] ^ 0xa5]) + p[w + 2:]))
    more = p[:PREFIX + 8] + struct.pack("<I", info["nleaves"] + 1) + p[PREFIX + 12:]
    try:
        parse(more, reference)                               # one leaf more than kept and added: where the sizes hide it from the container test
        out.append(("nleaves + 1", more))
    except Invalid:
        pass
    keep = info["streams"][0]
    if keep["mode"] == 0:
        nr, at = info["ref_nleaves"], keep["offset"]
        if nr % 8:
            last = at + keep["symbols"] - 1
            out.append(("keep padding bit", p[:last] + bytes([p[last] | 0x80]) + p[last + 1:]))
        out.append(("keep bit flipped", p[:at] + bytes([p[at] ^ 1]) + p[at + 1:]))
    return out
