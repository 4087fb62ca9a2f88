"""RULE T of the octree codec (include/cwipc_util_amd/hip_ext.h) restated in numpy: transform colour coding, the packet form "cwat".
Written from the rule's text, not from csrc/transform_terms.hpp; the tests hold the two, and the kernels, to each other byte for byte.
The parents of a depth are transformed side by side (one numpy row per parent, its eight child places and seven butterfly places as
columns); the depths are a Python loop.  The streams' coding is RULE E's (entropy_model)."""
import math
import struct

import numpy as np

import codec_model as cm
import entropy_model as em

MAGIC = b"cwat"
FIXED = 20          # u16 Q16, i16 dc[3], u32 nescapes[3]


class Invalid(ValueError):
    pass


def q16_of(jpeg_quality):
    q = max(1, int(jpeg_quality))
    sc = 5000 // q if q < 50 else 200 - 2 * q
    return min(1024, 16 + (12 * sc) // 10)


def channel_q16(q16, ch):
    return q16 if ch == 0 or q16 == 16 else min(1024, 2 * q16)


def isqrt(v):
    """The exact floor of the square root of a Python int."""
    return math.isqrt(int(v))


def floor_div(n, d):
    """floor(n / d) towards minus infinity, d > 0 (Python's and numpy's // on integers)."""
    return n // d


def step_of(q16c, w1, w2):
    t = (int(q16c) * int(q16c) * (int(w1) + int(w2))) // (int(w1) * int(w2))
    return max(1, (isqrt(t) + 8) >> 4)


def _steps(q16c, w1, w2):
    """step_of for arrays (every w above 0): t is below 2^22, so the float root is off by one at the most and is corrected in integers."""
    t = (np.int64(q16c) * np.int64(q16c) * (w1 + w2)) // (w1 * w2)
    r = np.floor(np.sqrt(t.astype(np.float64))).astype(np.int64)
    r = np.where(r * r > t, r - 1, r)
    r = np.where((r + 1) * (r + 1) <= t, r + 1, r)
    return np.maximum(1, (r + 8) >> 4)


def to_ycocg(rgb):
    rgb = np.asarray(rgb, dtype=np.int64).reshape(-1, 3)
    r, g, b = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    co = r - b
    t = b + (co >> 1)
    cg = g - t
    y = t + (cg >> 1)
    return np.stack([y, co, cg], axis=1)


def to_rgb(v):
    v = np.asarray(v, dtype=np.int64).reshape(-1, 3)
    y, co, cg = v[:, 0], v[:, 1], v[:, 2]
    t = y - (cg >> 1)
    g = cg + t
    b = t - (co >> 1)
    r = b + co
    return np.clip(np.stack([r, g, b], axis=1), 0, 255)


def zigzag(c):
    c = np.asarray(c, dtype=np.int64)
    return np.where(c >= 0, 2 * c, -2 * c - 1)


def unzigzag(zz):
    zz = np.asarray(zz, dtype=np.int64)
    return np.where(zz & 1, -((zz + 1) >> 1), zz >> 1)


def quantise(d, step):
    return np.sign(d) * ((np.abs(d) + step // 2) // step)


# ---------------------------------------------------------------------------
# the tree
# ---------------------------------------------------------------------------
def levels_of(packet, info):
    """Per depth 0 .. b - 1 the occupancy bits of its parents as a bool array [parents, 8]."""
    p, at, out = bytes(packet), info["occupancy_offset"], []
    for depth in range(info["octree_bits"]):
        count = 1 if depth == 0 else info["nodes"][depth - 1]
        level = np.frombuffer(p, dtype=np.uint8, count=count, offset=at)
        at += count
        out.append(np.unpackbits(level.reshape(-1, 1), axis=1, bitorder="little").astype(bool))
    return out


def _places(w):
    """w [P, 8] -> (w1, w2) [P, 7]: the x butterfly, the two y butterflies (low half first), the four z butterflies."""
    z1, z2 = w[:, 0::2], w[:, 1::2]
    wz = z1 + z2
    y1, y2 = wz[:, 0::2], wz[:, 1::2]
    wy = y1 + y2
    return np.concatenate([wy[:, :1], y1, z1], axis=1), np.concatenate([wy[:, 1:], y2, z2], axis=1)


def _weights(levels, nleaves):
    """Per depth the weights of its parents' child places [P, 8] (0: no child), bottom-up."""
    out, below = [None] * len(levels), np.ones(nleaves, dtype=np.int64)
    for depth in range(len(levels) - 1, -1, -1):
        w = np.zeros(levels[depth].shape, dtype=np.int64)
        w[levels[depth]] = below           # row-major: the parents ascending, their children ascending
        out[depth] = w
        below = w.sum(axis=1)
    return out


def _lift(d, w1, w2):
    W = w1 + w2
    return floor_div(w2 * d + (W >> 1), np.maximum(W, 1))


def _merge(a, w1, b, w2):
    """[..., 3] values with [...] weights -> the merged values and the coefficients (0 where there is no butterfly)."""
    both = ((w1 > 0) & (w2 > 0))[..., None]
    d = np.where(both, b - a, 0)
    l = np.where(both, a + _lift(d, w1[..., None], w2[..., None]), np.where((w1 > 0)[..., None], a, b))
    return l, d


def forward(levels, ycocg, q16):
    """The leaves' values [n, 3] -> (zz [n - 1, 3] in the decoder's order, dc [3])."""
    n = len(ycocg)
    weights = _weights(levels, n)
    below = np.asarray(ycocg, dtype=np.int64)
    per_depth = [None] * len(levels)
    for depth in range(len(levels) - 1, -1, -1):
        bits, w = levels[depth], weights[depth]
        v = np.zeros(bits.shape + (3,), dtype=np.int64)
        v[bits] = below
        w1, w2 = _places(w)
        z, dz = _merge(v[:, 0::2], w[:, 0::2], v[:, 1::2], w[:, 1::2])
        wz = w[:, 0::2] + w[:, 1::2]
        y, dy = _merge(z[:, 0::2], wz[:, 0::2], z[:, 1::2], wz[:, 1::2])
        wy = wz[:, 0::2] + wz[:, 1::2]
        x, dx = _merge(y[:, 0], wy[:, 0], y[:, 1], wy[:, 1])
        d = np.concatenate([dx[:, None], dy, dz], axis=1)                  # [P, 7, 3]
        has = (w1 > 0) & (w2 > 0)
        coef = np.zeros((int(has.sum()), 3), dtype=np.int64)
        for ch in range(3):
            steps = _steps(channel_q16(q16, ch), w1[has], w2[has])
            coef[:, ch] = zigzag(quantise(d[..., ch][has], steps))
        per_depth[depth] = coef
        below = x
    zz = np.concatenate(per_depth) if per_depth else np.zeros((0, 3), dtype=np.int64)
    assert len(zz) == n - 1
    return zz, below[0]


def inverse(levels, zz, dc, q16, nleaves):
    """-> the leaves' reconstructed values [n, 3], unclamped."""
    weights = _weights(levels, nleaves)
    zz = np.asarray(zz, dtype=np.int64).reshape(-1, 3)
    value = np.asarray(dc, dtype=np.int64).reshape(1, 3)
    at = 0
    for depth in range(len(levels)):
        bits, w = levels[depth], weights[depth]
        w1, w2 = _places(w)
        has = (w1 > 0) & (w2 > 0)
        count = int(has.sum())
        d = np.zeros(has.shape + (3,), dtype=np.int64)
        for ch in range(3):
            steps = _steps(channel_q16(q16, ch), w1[has], w2[has])
            plane = np.zeros(has.shape, dtype=np.int64)
            plane[has] = unzigzag(zz[at:at + count, ch]) * steps
            d[..., ch] = plane
        at += count

        def split(l, k):
            both = has[:, k][..., None]
            a = np.where(both, l - _lift(d[:, k], w1[:, k][..., None], w2[:, k][..., None]), l)
            return a, np.where(both, a + d[:, k], l)
        y0, y1 = split(value, 0)
        z0, z1 = split(y0, 1)
        z2, z3 = split(y1, 2)
        v = np.zeros(bits.shape + (3,), dtype=np.int64)
        for k, z in enumerate((z0, z1, z2, z3)):
            v[:, 2 * k], v[:, 2 * k + 1] = split(z, 3 + k)
        value = v[bits]
    assert at == len(zz)
    return value


# ---------------------------------------------------------------------------
# packets
# ---------------------------------------------------------------------------
def streams_of(info, nescapes):
    """[(kind, which, symbols)] in the rule's order."""
    if info["nleaves"] == 0:
        return []
    b, n = info["octree_bits"], info["nleaves"]
    out = [("occupancy", d, 1 if d == 0 else info["nodes"][d - 1]) for d in range(b)]
    for ch in range(3):
        out += [("token", ch, n - 1), ("escape", ch, nescapes[ch])]
    if info["tile_mode"] == 1:
        out.append(("tile", 0, n))
    return out


def coefficients(packet, jpeg_quality):
    """(zz [n - 1, 3], dc) of a valid 8-bit cwao packet with leaves."""
    p = bytes(packet)
    info = cm.parse(p)
    n = info["nleaves"]
    rgb = np.frombuffer(p, dtype=np.uint8, count=3 * n, offset=info["colour_offset"]).reshape(n, 3)
    return forward(levels_of(p, info), to_ycocg(rgb), q16_of(jpeg_quality))


def pack(packet, jpeg_quality):
    """A valid cwao packet with 8 colour bits -> cwat."""
    p = bytes(packet)
    info = cm.parse(p)
    if info["colour_bits"] != 8:
        raise Invalid("colour bits")
    b, n, q16 = info["octree_bits"], info["nleaves"], q16_of(jpeg_quality)
    head = 48 + 4 * b
    if n == 0:
        return MAGIC + struct.pack("<I", 1) + p[8:head] + struct.pack("<H3h3II", q16, 0, 0, 0, 0, 0, 0, 0)
    zz, dc = coefficients(p, jpeg_quality)
    nescapes = [int((zz[:, ch] >= 255).sum()) for ch in range(3)]
    plain = dict(zip([(k, w) for k, w, _ in em.streams_of(info)], em.stream_values(p, info)))
    directory, payloads = [], []
    for kind, which, count in streams_of(info, nescapes):
        if kind == "escape":
            data = (zz[:, which][zz[:, which] >= 255] - 255).astype("<u2").tobytes()
            payload, mode = data + bytes(cm.pad4(len(data)) - len(data)), 0
        else:
            values = np.minimum(zz[:, which], 255) if kind == "token" else plain[(kind, which)]
            payload, mode = em.raw_payload(kind, values, 8), 0
            if count >= em.BLOCK:
                coded = em.coded_payload(kind, values, 8)
                if len(coded) < len(payload):
                    payload, mode = coded, 1
        directory.append(struct.pack("<II", mode, len(payload)))
        payloads.append(payload)
    fixed = struct.pack("<H3h3I", q16, int(dc[0]), int(dc[1]), int(dc[2]), *nescapes)
    return MAGIC + struct.pack("<I", 1) + p[8:head] + fixed + struct.pack("<I", len(payloads)) + b"".join(directory) + b"".join(payloads)


def parse(packet):
    """The container test (what the host checks before the device sees anything).  Returns the cwao header's fields plus q16, dc,
    nescapes and `streams`: dicts kind, which, symbols, mode, offset, bytes, and for a coded one f, block_offsets, block_bytes."""
    p = bytes(packet)
    if len(p) < 48:
        raise Invalid("truncated header")
    if p[:4] != MAGIC:
        raise Invalid("magic")
    try:
        b = p[20]
        if not 1 <= b <= 16 or len(p) < 48 + 4 * b:
            raise cm.Invalid("bits or truncated node counts")
        info = em._header(p, b, struct.unpack("<I", p[16:20])[0])
    except cm.Invalid as e:
        raise Invalid(str(e))
    if info["colour_bits"] != 8:
        raise Invalid("colour bits")
    head = 48 + 4 * b
    if len(p) < head + FIXED + 4:
        raise Invalid("truncated transform header")
    q16, dc0, dc1, dc2, e0, e1, e2 = struct.unpack("<H3h3I", p[head:head + FIXED])
    n = info["nleaves"]
    if not 16 <= q16 <= 1024:
        raise Invalid("Q16")
    if n == 0 and any((dc0, dc1, dc2, e0, e1, e2)):
        raise Invalid("dc or escapes of an empty cloud")
    if n and max(e0, e1, e2) > n - 1:
        raise Invalid("more escapes than coefficients")
    info.update(q16=q16, dc=[dc0, dc1, dc2], nescapes=[e0, e1, e2])
    streams = streams_of(info, info["nescapes"])
    at = head + FIXED
    if struct.unpack("<I", p[at:at + 4])[0] != len(streams):
        raise Invalid("stream count")
    entries = at + 4
    at = entries + 8 * len(streams)
    if len(p) < at:
        raise Invalid("truncated directory")
    out = []
    for i, (kind, which, count) in enumerate(streams):
        mode, size = struct.unpack("<II", p[entries + 8 * i:entries + 8 * i + 8])
        used = 2 * count if kind == "escape" else count
        nblocks = 0 if kind == "escape" else (count + em.BLOCK - 1) // em.BLOCK
        if mode > 1 or (kind == "escape" and mode):
            raise Invalid("mode")
        if mode == 0 and size != cm.pad4(used):
            raise Invalid("raw payload size")
        if mode == 1 and (count < em.BLOCK or size % 4 or size < 512 + nblocks * (4 + 256) or size >= cm.pad4(used)):
            raise Invalid("coded payload size")
        out.append(dict(kind=kind, which=which, symbols=count, mode=mode, offset=at, bytes=size, nblocks=nblocks, used=used))
        at += size
    if len(p) != at:
        raise Invalid("length")
    for s in out:
        q = p[s["offset"]:s["offset"] + s["bytes"]]
        if s["mode"] == 0:
            if any(q[s["used"]:]):
                raise Invalid("padding")
            if s["kind"] == "occupancy":
                try:
                    em._occupancy_rules(np.frombuffer(q, dtype=np.uint8, count=s["symbols"]), info["nodes"][s["which"]])
                except em.Invalid as e:
                    raise Invalid(str(e))
            continue
        f = np.frombuffer(q, dtype="<u2", count=256).astype(np.int64)
        if f.sum() != em.M:
            raise Invalid("frequencies do not sum to 4096")
        if s["kind"] == "occupancy" and f[0]:
            raise Invalid("occupancy byte 0 has a frequency")
        sizes = np.frombuffer(q, dtype="<u4", count=s["nblocks"], offset=512).astype(np.int64)
        if (sizes % 4).any() or (sizes < 256).any() or (sizes > 256 + 2 * em.BLOCK).any() or sizes.sum() != s["bytes"] - 512 - 4 * s["nblocks"]:
            raise Invalid("block sizes")
        s["f"], s["block_bytes"] = f, sizes
        s["block_offsets"] = s["offset"] + 512 + 4 * s["nblocks"] + np.concatenate([[0], np.cumsum(sizes)[:-1]])
    info["streams"] = out
    return info


def _stream_values(p, s, info):
    if s["mode"] == 0:
        return np.frombuffer(p, dtype="<u2" if s["kind"] == "escape" else np.uint8, count=s["symbols"], offset=s["offset"]).astype(np.int64)
    blocks = []
    for at, size in zip(s["block_offsets"], s["block_bytes"]):
        blocks.append((np.frombuffer(p, dtype="<u4", count=em.LANES, offset=int(at)), np.frombuffer(p, dtype="<u2", count=(int(size) - 256) // 2, offset=int(at) + 256)))
    counts = [min(em.BLOCK, s["symbols"] - em.BLOCK * k) for k in range(s["nblocks"])]
    values, intact = em.decode_blocks(blocks, counts, s["f"])
    if not intact.all():
        raise Invalid("block not intact")
    if s["kind"] == "occupancy":
        try:
            em._occupancy_rules(values.astype(np.uint8), info["nodes"][s["which"]])
        except em.Invalid as e:
            raise Invalid(str(e))
    return values


def unpack(packet):
    """cwat -> the cwao packet it stands for; Invalid for a packet that is refused."""
    p = bytes(packet)
    info = parse(p)
    n, b = info["nleaves"], info["octree_bits"]
    head = cm.MAGIC + struct.pack("<I", 1) + p[8:48 + 4 * b]
    if n == 0:
        return head
    occupancy, tiles, zz = bytearray(), b"", np.zeros((n - 1, 3), dtype=np.int64)
    for s in info["streams"]:
        values = _stream_values(p, s, info)
        if s["kind"] == "occupancy":
            occupancy += values.astype(np.uint8).tobytes()
        elif s["kind"] == "tile":
            tiles = values.astype(np.uint8).tobytes()
        elif s["kind"] == "token":
            zz[:, s["which"]] = values
        else:
            where = zz[:, s["which"]] == 255
            if int(where.sum()) != s["symbols"]:
                raise Invalid("tokens equal to 255 differ from the escape count")
            zz[where, s["which"]] += values
    occupancy += bytes(cm.pad4(len(occupancy)) - len(occupancy))
    shell = head + bytes(occupancy) + bytes(cm.pad4(3 * n)) + tiles
    rgb = to_rgb(inverse(levels_of(shell, cm.parse(shell)), zz, info["dc"], info["q16"], n))
    col = rgb.astype(np.uint8).tobytes()
    return head + bytes(occupancy) + col + bytes(cm.pad4(len(col)) - len(col)) + tiles


def colour_payload_bytes(packet):
    """The bytes a cwat packet spends on colour: the token and escape payloads and their directory entries."""
    return sum(s["bytes"] + 8 for s in parse(packet)["streams"] if s["kind"] in ("token", "escape"))


# ---------------------------------------------------------------------------
# test material
# ---------------------------------------------------------------------------
def sphere_cloud(n=400000, sigma=3.0, seed=20261020):
    """Points on a unit sphere with a smooth colour field plus Gaussian noise of `sigma` per channel: the cloud of the rate-distortion
    comparison."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    rgb = np.stack([128 + 100 * np.sin(5 * x) * np.cos(3 * y), 128 + 90 * np.sin(4 * y + 1), 128 + 80 * np.cos(6 * z)], axis=1)
    rgb = np.clip(np.rint(rgb + rng.normal(scale=sigma, size=rgb.shape)), 0, 255).astype(np.uint8)
    pts = cm.make_cloud(d, rgb)
    pts['tile'] = 1
    return pts


def leaves_packet(keys, rgb, bits, tiles=None, timestamp=0):
    """A cwao packet with 8 colour bits from leaf keys (ascending) and their colours."""
    keys = np.asarray(keys, dtype=np.uint64)
    tiles = np.ones(len(keys), dtype=np.uint8) if tiles is None else tiles
    return cm.build_packet(keys, rgb, tiles, np.zeros(3, dtype=np.float32), 1.0, bits, 8, timestamp)
