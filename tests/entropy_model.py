"""RULE E of the octree codec (include/cwipc_util_amd/hip_ext.h) restated in numpy: the entropy-coded form "cwae" of a "cwao" packet.
Written from the rule's text, not from csrc/entropy_terms.hpp; the tests hold the two, and the kernels, to each other byte for byte.
The blocks of a stream are coded side by side (one numpy row per block), the 64 lanes of a block side by side too; the rounds are a
Python loop."""
import struct

import numpy as np

import codec_model as cm

MAGIC = b"cwae"
BLOCK = 4096
LANES = 64
M = 4096
LOW = 1 << 16
ROUNDS = BLOCK // LANES


class Invalid(ValueError):
    pass


def normalise(counts):
    """f[256] from the 256 counts of a stream."""
    c = [int(v) for v in counts]
    assert len(c) == 256 and sum(c) > 0
    total = sum(c)
    f = [0 if v == 0 else max(1, (v * M) // total) for v in c]
    d = M - sum(f)
    if d > 0:
        f[c.index(max(c))] += d
    while d < 0:
        top = f.index(max(f))
        assert f[top] > 1
        f[top] -= 1
        d += 1
    assert sum(f) == M
    return np.array(f, dtype=np.int64)


def cumulate(f):
    return np.concatenate([[0], np.cumsum(f)[:-1]]).astype(np.int64)


def _grid(symbols):
    """symbols -> [nblocks, ROUNDS, LANES] (zero filled) and the mask of the places that hold one."""
    n = len(symbols)
    nblocks = (n + BLOCK - 1) // BLOCK
    grid = np.zeros(nblocks * BLOCK, dtype=np.int64)
    grid[:n] = symbols
    live = np.zeros(nblocks * BLOCK, dtype=bool)
    live[:n] = True
    return grid.reshape(nblocks, ROUNDS, LANES), live.reshape(nblocks, ROUNDS, LANES)


def encode_blocks(symbols, f):
    """[(states[64], words)] per block of 4096 symbols: the encoder of the rule, all blocks at once."""
    f = np.asarray(f, dtype=np.int64)
    cum = cumulate(f)
    grid, live = _grid(np.asarray(symbols, dtype=np.int64))
    nblocks = grid.shape[0]
    x = np.full((nblocks, LANES), LOW, dtype=np.int64)
    emitted = np.zeros((nblocks, ROUNDS, LANES), dtype=bool)
    word = np.zeros((nblocks, ROUNDS, LANES), dtype=np.int64)
    for r in range(ROUNDS - 1, -1, -1):            # the lanes of a round do not touch each other's state: their order only orders the words
        s, on = grid[:, r, :], live[:, r, :]
        fs = np.where(on, f[s], 1)
        emit = on & (x >= (fs << 20))
        word[:, r, :] = np.where(emit, x & 0xffff, 0)
        emitted[:, r, :] = emit
        x = np.where(emit, x >> 16, x)
        x = np.where(on, (x // fs) * M + (x % fs) + cum[s], x)
    # emission runs from the last round to the first, lanes descending: reversed, that is rounds ascending, lanes ascending
    return [(x[b].copy(), word[b][emitted[b]]) for b in range(nblocks)]


def decode_blocks(blocks, counts, f):
    """blocks: [(states[64], word slots)] with counts[b] symbols each -> (symbols, intact[b]).  The decoder of the rule."""
    f = np.asarray(f, dtype=np.int64)
    cum = cumulate(f)
    nblocks = len(blocks)
    x = np.array([np.asarray(st, dtype=np.int64) for st, _ in blocks]).reshape(nblocks, LANES)
    nwords = np.array([len(w) for _, w in blocks], dtype=np.int64)
    slots = np.zeros((nblocks, BLOCK + LANES + 1), dtype=np.int64)
    for b, (_, w) in enumerate(blocks):
        slots[b, :len(w)] = w
    counts = np.asarray(counts, dtype=np.int64)
    bad = (x < LOW).any(axis=1)
    cursor = np.zeros(nblocks, dtype=np.int64)
    out = np.zeros((nblocks, ROUNDS, LANES), dtype=np.int64)
    lane = np.arange(LANES)
    for r in range(ROUNDS):
        on = (LANES * r + lane)[None, :] < counts[:, None]
        slot = x & (M - 1)
        s = np.searchsorted(cum, slot.reshape(-1), side="right").reshape(slot.shape) - 1      # the last s with cum[s] <= slot: f[s] > 0
        out[:, r, :] = np.where(on, s, 0)
        x = np.where(on, f[s] * (x >> 12) + slot - cum[s], x)
        need = on & (x < LOW)
        rank = np.cumsum(need, axis=1) - need
        at = cursor[:, None] + rank
        bad |= (need & (at >= nwords[:, None])).any(axis=1)
        got = np.where(at < nwords[:, None], np.take_along_axis(slots, np.minimum(at, BLOCK + LANES), axis=1), 0)
        x = np.where(need, ((x << 16) | got) & 0xffffffff, x)
        cursor += need.sum(axis=1)
    bad |= (x != LOW).any(axis=1)
    at_end = (cursor == nwords) | ((cursor + 1 == nwords) & (np.take_along_axis(slots, np.minimum(cursor, BLOCK + LANES)[:, None], axis=1)[:, 0] == 0))
    bad |= ~at_end
    symbols = np.concatenate([out[b].reshape(-1)[:counts[b]] for b in range(nblocks)]) if nblocks else np.zeros(0, dtype=np.int64)
    return symbols, ~bad


def block_bytes(states, words):
    data = np.asarray(states, dtype="<u4").tobytes() + np.asarray(words, dtype="<u2").tobytes()
    return data + bytes(cm.pad4(len(data)) - len(data))


def streams_of(info):
    """[(kind, which, symbols)] in the rule's order."""
    if info["nleaves"] == 0:
        return []
    b, n = info["octree_bits"], info["nleaves"]
    out = [("occupancy", d, 1 if d == 0 else info["nodes"][d - 1]) for d in range(b)]
    out += [("colour", ch, n) for ch in range(3)]
    if info["tile_mode"] == 1:
        out.append(("tile", 0, n))
    return out


def stream_values(packet, info):
    """The plain values of every stream of a cwao packet."""
    p, n, cb = bytes(packet), info["nleaves"], info["colour_bits"]
    out, at = [], info["occupancy_offset"]
    colours = cm.unpack_bits(p[info["colour_offset"]:info["colour_offset"] + info["colour_bytes"]], 3 * n, cb).reshape(n, 3) if n else None
    for kind, which, count in streams_of(info):
        if kind == "occupancy":
            out.append(np.frombuffer(p, dtype=np.uint8, count=count, offset=at).astype(np.int64))
            at += count
        elif kind == "colour":
            out.append(colours[:, which].astype(np.int64))
        else:
            out.append(np.frombuffer(p, dtype=np.uint8, count=n, offset=info["tile_offset"]).astype(np.int64))
    return out


def predict(values, cb):
    """Colour symbols: the difference to the value before, mod 2^cb; the first of each block of 4096 as it is."""
    v = np.asarray(values, dtype=np.int64)
    sym = v.copy()
    sym[1:] = (v[1:] - v[:-1]) & ((1 << cb) - 1)
    sym[::BLOCK] = v[::BLOCK]
    return sym


def unpredict(symbols, cb):
    out = np.zeros(len(symbols), dtype=np.int64)
    for start in range(0, len(symbols), BLOCK):
        out[start:start + BLOCK] = np.cumsum(symbols[start:start + BLOCK]) & ((1 << cb) - 1)
    return out


def raw_payload(kind, values, cb):
    data = cm.pack_bits(values, cb) if kind == "colour" else np.asarray(values, dtype=np.uint8).tobytes()
    return data + bytes(cm.pad4(len(data)) - len(data))


def coded_payload(kind, values, cb):
    symbols = predict(values, cb) if kind == "colour" else np.asarray(values, dtype=np.int64)
    f = normalise(np.bincount(symbols, minlength=256))
    blocks = [block_bytes(st, w) for st, w in encode_blocks(symbols, f)]
    return f.astype("<u2").tobytes() + struct.pack("<%dI" % len(blocks), *[len(b) for b in blocks]) + b"".join(blocks)


def pack(packet):
    """cwao -> cwae."""
    p = bytes(packet)
    info = cm.parse(p)
    head = 48 + 4 * info["octree_bits"]
    directory, payloads = [], []
    for (kind, which, count), values in zip(streams_of(info), stream_values(p, info)):
        payload, mode = raw_payload(kind, values, info["colour_bits"]), 0
        if count >= BLOCK:
            coded = coded_payload(kind, values, info["colour_bits"])
            if len(coded) < len(payload):
                payload, mode = coded, 1
        directory.append(struct.pack("<II", mode, len(payload)))
        payloads.append(payload)
    return MAGIC + struct.pack("<I", 1) + p[8:head] + struct.pack("<I", len(payloads)) + b"".join(directory) + b"".join(payloads)


def parse(packet):
    """The container test (what the host checks before the device sees anything).  Returns the cwao header's fields plus
    `streams`: a list of dicts kind, which, symbols, mode, offset, bytes, and for a coded one f, block_offsets, block_bytes."""
    p = bytes(packet)
    if len(p) < 48:
        raise Invalid("truncated header")
    if p[:4] != MAGIC:
        raise Invalid("magic")
    try:
        b = p[20]
        if not 1 <= b <= 16 or len(p) < 48 + 4 * b:
            raise cm.Invalid("bits or truncated node counts")
        # RULE C's own header test, on a cwao packet with this header and a body that the header's counts size (its content is not looked at)
        n = struct.unpack("<I", p[16:20])[0]
        info = _header(p, b, n)
    except cm.Invalid as e:
        raise Invalid(str(e))
    head = 48 + 4 * b
    if len(p) < head + 4:
        raise Invalid("truncated stream count")
    streams = streams_of(info)
    if struct.unpack("<I", p[head:head + 4])[0] != len(streams):
        raise Invalid("stream count")
    at = head + 4 + 8 * len(streams)
    if len(p) < at:
        raise Invalid("truncated directory")
    out = []
    for i, (kind, which, count) in enumerate(streams):
        mode, size = struct.unpack("<II", p[head + 4 + 8 * i:head + 12 + 8 * i])
        raw = cm.pad4((count * info["colour_bits"] + 7) // 8 if kind == "colour" else count)
        nblocks = (count + BLOCK - 1) // BLOCK
        if mode > 1:
            raise Invalid("mode")
        if mode == 0 and size != raw:
            raise Invalid("raw payload size")
        if mode == 1 and (count < BLOCK or size % 4 or size < 512 + nblocks * (4 + 256) or size >= raw):
            raise Invalid("coded payload size")
        out.append(dict(kind=kind, which=which, symbols=count, mode=mode, offset=at, bytes=size, nblocks=nblocks))
        at += size
    if len(p) != at:
        raise Invalid("length")
    for s in out:
        q = p[s["offset"]:s["offset"] + s["bytes"]]
        if s["mode"] == 0:
            used = (s["symbols"] * info["colour_bits"] + 7) // 8 if s["kind"] == "colour" else s["symbols"]
            if any(q[used:]):
                raise Invalid("padding")
            if s["kind"] == "colour" and (s["symbols"] * info["colour_bits"]) % 8 and q[used - 1] >> ((s["symbols"] * info["colour_bits"]) % 8):
                raise Invalid("padding")
            if s["kind"] == "occupancy":
                _occupancy_rules(np.frombuffer(q, dtype=np.uint8, count=s["symbols"]), info["nodes"][s["which"]])
            continue
        f = np.frombuffer(q, dtype="<u2", count=256).astype(np.int64)
        if f.sum() != M:
            raise Invalid("frequencies do not sum to 4096")
        if s["kind"] == "occupancy" and f[0]:
            raise Invalid("occupancy byte 0 has a frequency")
        if s["kind"] == "colour" and f[1 << info["colour_bits"]:].any():
            raise Invalid("colour value above its bits")
        sizes = np.frombuffer(q, dtype="<u4", count=s["nblocks"], offset=512).astype(np.int64)
        if (sizes % 4).any() or (sizes < 256).any() or (sizes > 256 + 2 * BLOCK).any() or sizes.sum() != s["bytes"] - 512 - 4 * s["nblocks"]:
            raise Invalid("block sizes")
        s["f"], s["block_bytes"] = f, sizes
        s["block_offsets"] = s["offset"] + 512 + 4 * s["nblocks"] + np.concatenate([[0], np.cumsum(sizes)[:-1]])
    info["streams"] = out
    return info


def _header(p, b, n):
    """The cwao header's fields by RULE C's rules, through codec_model.parse on a packet made to fit the header."""
    nodes = list(struct.unpack("<%dI" % b, p[48:48 + 4 * b]))
    cb, mode = p[21], p[22]
    if not 4 <= cb <= 8 or mode > 1:
        raise cm.Invalid("range")
    if nodes[-1] != n:
        raise cm.Invalid("leaf count")
    if n and (not 1 <= nodes[0] <= 8 or any(nodes[i + 1] > 8 * nodes[i] or nodes[i + 1] < nodes[i] for i in range(b - 1))):
        raise cm.Invalid("node counts")
    if n > (1 << 26):
        raise cm.Invalid("too large for the model")
    # a body that passes RULE C's body test for these node counts: depth d's bytes hold nodes[d] bits, none 0
    body = bytearray()
    for d in range(b if n else 0):
        parents, children = (1 if d == 0 else nodes[d - 1]), nodes[d]
        extra = children - parents
        level = np.ones(parents, dtype=np.int64)
        level[:extra // 7] += 7
        if extra % 7:
            level[extra // 7] += extra % 7
        body += ((1 << level) - 1).astype(np.uint8).tobytes()
    body += bytes(cm.pad4(len(body)) - len(body))
    body += bytes(cm.pad4((n * 3 * cb + 7) // 8)) + (bytes(n) if mode == 1 else b"")
    return cm.parse(cm.MAGIC + p[4:48 + 4 * b] + bytes(body))


def _occupancy_rules(level, children):
    if (level == 0).any():
        raise Invalid("occupancy byte 0")
    if int(np.unpackbits(level).sum()) != children:
        raise Invalid("popcount")


def unpack(packet):
    """cwae -> the cwao packet it stands for; Invalid for a packet that the container test, a block's integrity or the occupancy
    rules refuse."""
    p = bytes(packet)
    info = parse(p)
    n, cb, b = info["nleaves"], info["colour_bits"], info["octree_bits"]
    occupancy, colours, tiles = bytearray(), [None] * 3, b""
    for s in info["streams"]:
        q = p[s["offset"]:s["offset"] + s["bytes"]]
        if s["mode"] == 0:
            values = cm.unpack_bits(q, s["symbols"], cb) if s["kind"] == "colour" else np.frombuffer(q, dtype=np.uint8, count=s["symbols"]).astype(np.int64)
        else:
            blocks = []
            for at, size in zip(s["block_offsets"], s["block_bytes"]):
                blocks.append((np.frombuffer(p, dtype="<u4", count=LANES, offset=int(at)), np.frombuffer(p, dtype="<u2", count=(int(size) - 256) // 2, offset=int(at) + 256)))
            counts = [min(BLOCK, s["symbols"] - BLOCK * k) for k in range(s["nblocks"])]
            values, intact = decode_blocks(blocks, counts, s["f"])
            if not intact.all():
                raise Invalid("block not intact")
            if s["kind"] == "colour":
                values = unpredict(values, cb)
            elif s["kind"] == "occupancy":
                _occupancy_rules(values.astype(np.uint8), info["nodes"][s["which"]])
        if s["kind"] == "occupancy":
            occupancy += values.astype(np.uint8).tobytes()
        elif s["kind"] == "colour":
            colours[s["which"]] = values
        else:
            tiles = values.astype(np.uint8).tobytes()
    head = cm.MAGIC + struct.pack("<I", 1) + p[8:48 + 4 * b]
    if n == 0:
        return head
    occupancy += bytes(cm.pad4(len(occupancy)) - len(occupancy))
    col = cm.pack_bits(np.stack(colours, axis=1).reshape(-1), cb)
    col += bytes(cm.pad4(len(col)) - len(col))
    return head + bytes(occupancy) + col + tiles


def directory(packet):
    """[(mode, payload bytes)] per stream."""
    return [(s["mode"], s["bytes"]) for s in parse(packet)["streams"]]


# ---------------------------------------------------------------------------
# test material
# ---------------------------------------------------------------------------
def structured_cloud(n=60000, tiles=(1, 2), seed=0):
    """A sphere's surface with a smooth colour, two tiles by hemisphere: what a camera rig gives, in the small."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rgb = np.clip(128 + 100 * np.stack([d[:, 0], d[:, 1], np.sin(3 * d[:, 2])], axis=1), 0, 255).astype(np.uint8)
    pts = cm.make_cloud(d, rgb)
    pts['tile'] = np.where(d[:, 0] < 0, tiles[0], tiles[-1]).astype(np.uint8)
    return pts


def damages(packet):
    """(what, bytes) for each damage of a cwae packet that the CONTAINER test must refuse."""
    p = bytes(packet)
    info = parse(p)
    b = info["octree_bits"]
    head = 48 + 4 * b
    streams = info["streams"]
    out = []
    edges = {0, 4, 8, 20, 48, head, head + 4, head + 4 + 8 * len(streams), len(p) - 1}
    for s in streams:
        edges |= {s["offset"], s["offset"] + s["bytes"] - 1}
        if s["mode"] == 1:
            edges |= {s["offset"] + 512, s["offset"] + 512 + 4 * s["nblocks"], int(s["block_offsets"][-1]) + 256}
    for at in sorted(edges):
        if 0 <= at < len(p):
            out.append((f"truncated at {at}", p[:at]))
    out.append(("one byte appended", p + b"\x00"))
    out.append(("four bytes appended", p + bytes(4)))
    out.append(("magic of the plain packet", cm.MAGIC + p[4:]))
    out.append(("magic", b"cwaE" + p[4:]))
    out.append(("version", p[:4] + struct.pack("<I", 2) + p[8:]))
    out.append(("octree_bits 0", p[:20] + b"\x00" + p[21:]))
    out.append(("colour bits 9", p[:21] + b"\x09" + p[22:]))
    out.append(("reserved word", p[:36] + b"\x01" + p[37:]))
    out.append(("side 0", p[:40] + struct.pack("<d", 0.0) + p[48:]))
    out.append(("nleaves + 1", p[:16] + struct.pack("<I", info["nleaves"] + 1) + p[20:]))
    nstreams = len(streams)
    for delta in (1, -1):
        if nstreams + delta >= 0:
            out.append((f"S {delta:+d}", p[:head] + struct.pack("<I", nstreams + delta) + p[head + 4:]))
    if info["nleaves"]:
        out.append(("tile mode flipped", p[:22] + bytes([1 - info["tile_mode"], 0]) + p[24:]))
    for i, s in enumerate(streams):
        entry = head + 4 + 8 * i
        out.append((f"stream {i} mode 2", p[:entry] + struct.pack("<I", 2) + p[entry + 4:]))
        out.append((f"stream {i} mode flipped", p[:entry] + struct.pack("<I", 1 - s["mode"]) + p[entry + 4:]))
        for delta in (4, -4, 1):
            if s["bytes"] + delta >= 0:
                out.append((f"stream {i} payload_bytes {delta:+d}", p[:entry + 4] + struct.pack("<I", s["bytes"] + delta) + p[entry + 8:]))
        at = s["offset"]
        if s["mode"] == 0:
            used = (s["symbols"] * info["colour_bits"] + 7) // 8 if s["kind"] == "colour" else s["symbols"]
            for pad in range(at + used, at + s["bytes"]):
                out.append((f"stream {i} pad byte", p[:pad] + b"\x01" + p[pad + 1:]))
            if s["kind"] == "colour" and (s["symbols"] * info["colour_bits"]) % 8:
                last = at + used - 1
                out.append((f"stream {i} pad bits", p[:last] + bytes([p[last] | 0x80]) + p[last + 1:]))
            if s["kind"] == "occupancy":
                out.append((f"stream {i} raw occupancy byte 0", p[:at] + b"\x00" + p[at + 1:]))
                out.append((f"stream {i} raw occupancy bit flipped", p[:at] + bytes([p[at] ^ 1 if p[at] != 1 else 3]) + p[at + 1:]))
            continue
        f = s["f"]
        top = int(np.argmax(f))
        for delta in (1, -1):
            out.append((f"stream {i} sum f {delta:+d}", p[:at + 2 * top] + struct.pack("<H", int(f[top]) + delta) + p[at + 2 * top + 2:]))
        k = s["nblocks"] - 1
        size_at, size = at + 512 + 4 * k, int(s["block_bytes"][k])
        for what, value in (("odd", size + 1), ("off by two", size + 2), ("too small", 252), ("too large", 256 + 2 * BLOCK + 4), ("+4", size + 4)):
            out.append((f"stream {i} block_bytes {what}", p[:size_at] + struct.pack("<I", value) + p[size_at + 4:]))
    return out


def payload_damages(packet, limit_per_stream=None):
    """(what, bytes) for damages inside coded payloads that the container test ACCEPTS: the block decoder (or, for occupancy, the two
    occupancy rules) must refuse each.  One block per coded stream, the last one."""
    p = bytes(packet)
    info = parse(p)
    out = []
    for i, s in enumerate(info["streams"]):
        if s["mode"] != 1:
            continue
        k = s["nblocks"] - 1
        at, size = int(s["block_offsets"][k]), int(s["block_bytes"][k])
        out.append((f"stream {i} state below 2^16", p[:at + 8] + struct.pack("<I", 0xffff) + p[at + 12:]))
        out.append((f"stream {i} state 0", p[:at] + struct.pack("<I", 0) + p[at + 4:]))
        out.append((f"stream {i} state 0xffffffff", p[:at + 4 * 63] + struct.pack("<I", 0xffffffff) + p[at + 4 * 64:]))
        if size > 256 + 4:
            for w in (at + 256, at + 256 + (size - 256) // 4 * 2, at + size - 4):
                out.append((f"stream {i} word at {w - at} flipped", p[:w] + bytes([p[w] ^ 0x5a, p[w + 1] ^ 0xa5]) + p[w + 2:]))
            # two words (one block-size step) removed from the end of the block, sizes adjusted
            entry = 48 + 4 * info["octree_bits"] + 4 + 8 * i
            size_at = s["offset"] + 512 + 4 * k
            cut = p[:at + size - 4] + p[at + size:]
            cut = cut[:size_at] + struct.pack("<I", size - 4) + cut[size_at + 4:]
            cut = cut[:entry + 4] + struct.pack("<I", s["bytes"] - 4) + cut[entry + 8:]
            out.append((f"stream {i} words removed", cut))
        # two frequencies that differ swapped among the symbols a stream of this kind may use: the sum stays
        f = s["f"]
        used = np.nonzero(f)[0]
        if len(used) >= 2 and f[used].min() != f[used].max():
            a, c = int(used[np.argmax(f[used])]), int(used[np.argmin(f[used])])
            g = f.copy()
            g[a], g[c] = f[c], f[a]
            out.append((f"stream {i} f permuted", p[:s["offset"]] + g.astype("<u2").tobytes() + p[s["offset"] + 512:]))
    return out
