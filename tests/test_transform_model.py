"""RULE T (include/cwipc_util_amd/hip_ext.h), transform colour coding, in its numpy restatement (tests/transform_model.py): packets
worked by hand, the properties the rule promises, and the test material (packets, container damages, payload damages) that
test_transform_host.py runs through the header compiled for the host and test_gpu_colour_transform.py through the kernels.  CPU only."""
import struct

import numpy as np
import pytest

import codec_model as cm
import entropy_model as em
import transform_model as tm


def grey(values):
    return [(v, v, v) for v in values]


def colours_of(packet):
    info = cm.parse(packet)
    return np.frombuffer(bytes(packet), dtype=np.uint8, count=3 * info["nleaves"], offset=info["colour_offset"]).reshape(-1, 3)


def tokens_of(packet):
    """(zz [n - 1, 3] rebuilt from tokens and escapes, info) of a cwat packet whose token streams are raw."""
    info = tm.parse(packet)
    zz = np.zeros((info["nleaves"] - 1, 3), dtype=np.int64)
    for s in info["streams"]:
        if s["kind"] in ("token", "escape"):
            values = tm._stream_values(bytes(packet), s, info)
            if s["kind"] == "token":
                zz[:, s["which"]] = values
            else:
                zz[zz[:, s["which"]] == 255, s["which"]] += values
    return zz, info


# ---------------------------------------------------------------------------
# hand-worked packets
# ---------------------------------------------------------------------------
def hand_packets():
    """name -> the cwao packet."""
    chain = (0o1234567012345670 >> 3) << 3            # sixteen triples; the last one is replaced
    return {
        "one leaf": tm.leaves_packet([5], [(10, 200, 30)], 3),
        "two siblings": tm.leaves_packet([2, 3], [(100, 100, 100), (110, 100, 90)], 1),
        "all eight children": tm.leaves_packet(np.arange(8), grey([0, 10, 20, 40, 80, 100, 140, 200]), 1),
        "chain of sixteen": tm.leaves_packet([chain | 1, chain | 6], grey([50, 90]), 16),
        "weights 1 and 7": tm.leaves_packet([3] + list(range(32, 39)), grey([80] + [160] * 7), 2),
    }


def test_one_leaf_has_no_coefficients():
    P = hand_packets()["one leaf"]
    T = tm.pack(P, 100)
    info = tm.parse(T)
    # Co = 10 - 30 = -20; t = 30 - 10 = 20; Cg = 180; Y = 20 + 90
    assert info["dc"] == [110, -20, 180] and info["nescapes"] == [0, 0, 0] and info["q16"] == 16
    assert [(s["kind"], s["symbols"], s["mode"], s["bytes"]) for s in info["streams"][3:]] == [("token", 0, 0, 0), ("escape", 0, 0, 0)] * 3
    assert len(T) == 48 + 12 + 20 + 4 + 8 * 9 + 3 * 4 and tm.unpack(T) == P
    assert tm.unpack(tm.pack(P, 0)) == P              # nothing to quantise


def test_two_sibling_leaves():
    P = hand_packets()["two siblings"]
    # both leaves have Y = 100 and Cg = 0; Co is 0 and 20: d = 20, l = 0 + floor((20 + 1) / 2)
    zz, info = tokens_of(tm.pack(P, 100))
    assert info["dc"] == [100, 10, 0] and zz.tolist() == [[0, 40, 0]]
    assert tm.unpack(tm.pack(P, 100)) == P
    # quality 25: Q16 = 256, the chroma scale 512: t = 512 * 512 * 2 = 524288, isqrt 724, step (724 + 8) >> 4 = 45; c = (20 + 22) / 45 = 0
    assert tm.q16_of(25) == 256 and tm.step_of(512, 1, 1) == 45 and tm.step_of(256, 1, 1) == 23
    zz, info = tokens_of(tm.pack(P, 25))
    assert zz.tolist() == [[0, 0, 0]] and info["dc"] == [100, 10, 0]
    assert colours_of(tm.unpack(tm.pack(P, 25))).tolist() == [[105, 100, 95]] * 2       # both leaves get Y 100, Co 10, Cg 0


def test_parent_with_all_eight_children():
    P = hand_packets()["all eight children"]
    zz, info = tokens_of(tm.pack(P, 100))
    # z: d = 10, 20, 20, 60 and l = 5, 30, 90, 170; y: d = 25, 80 and l = 5 + floor(52 / 4) = 18, 90 + floor(162 / 4) = 130;
    # x: d = 112, l = 18 + floor((4 * 112 + 4) / 8) = 74.  Order: x, y low, y high, z ascending; zz = 2 d
    assert info["dc"] == [74, 0, 0]
    assert zz[:, 0].tolist() == [224, 50, 160, 20, 40, 40, 120] and not zz[:, 1:].any()
    assert tm.unpack(tm.pack(P, 100)) == P


def test_chain_of_single_children_has_one_butterfly():
    P = hand_packets()["chain of sixteen"]
    assert cm.parse(P)["nodes"] == [1] * 15 + [2]
    zz, info = tokens_of(tm.pack(P, 100))
    # children 1 and 6 of the last parent meet only in the x butterfly: d = 40, l = 50 + floor(41 / 2)
    assert zz.tolist() == [[80, 0, 0]] and info["dc"] == [70, 0, 0]
    assert tm.unpack(tm.pack(P, 100)) == P


def test_halves_of_weights_one_and_seven():
    P = hand_packets()["weights 1 and 7"]
    zz, info = tokens_of(tm.pack(P, 100))
    # the root's x butterfly: a = 80 (w 1), b = 160 (w 7): d = 80, l = 80 + floor((7 * 80 + 4) / 8) = 150; it is the first coefficient
    assert info["dc"] == [150, 0, 0] and zz[:, 0].tolist() == [160] + [0] * 6
    # quality 50: Q16 136; t = 136 * 136 * 8 / 7 = 21138, isqrt 145, step (145 + 8) >> 4 = 9; c = (80 + 4) / 9 = 9, d^ = 81;
    # a^ = 150 - floor((7 * 81 + 4) / 8) = 79, b^ = 160
    assert tm.step_of(136, 1, 7) == 9
    assert colours_of(tm.unpack(tm.pack(P, 50))).tolist() == [list(c) for c in grey([79] + [160] * 7)]


# ---------------------------------------------------------------------------
# properties
# ---------------------------------------------------------------------------
_random = {}


def random_packets():
    """name -> a cwao packet with 8 colour bits and random colours: 20 of them, 1 to 9000 leaves, 1 to 16 bits, tiles equal and mixed."""
    if _random:
        return _random
    rng = np.random.default_rng(2026)
    for i in range(20):
        bits = int(rng.integers(1, 17))
        n = int(min(rng.choice([1, 2, 3, 9, 70, 500, 4097, 9000]), 1 << (3 * bits)))
        keys = np.sort(rng.choice(min(1 << (3 * bits), 1 << 30), n, replace=False).astype(np.uint64)) << np.uint64(max(0, 3 * bits - 30))
        tiles = rng.choice(np.array([1, 2, 4], dtype=np.uint8), n) if i % 2 else np.full(n, 3, dtype=np.uint8)
        _random[f"random {i}: {n} leaves, {bits} bits"] = tm.leaves_packet(keys, rng.integers(0, 256, (n, 3)), bits, tiles, timestamp=1000 + i)
    return _random


QUALITIES = (100, 85, 50, 24, 0)


def test_quality_100_is_exact_for_random_colours():
    for name, P in random_packets().items():
        assert tm.unpack(tm.pack(P, 100)) == P, name


def test_lossy_packets_unpack_to_valid_packets_with_the_same_tree():
    for i, (name, P) in enumerate(random_packets().items()):
        T = tm.pack(P, QUALITIES[1 + i % 4])
        U = tm.unpack(T)
        info = cm.parse(U)
        assert U[:info["colour_offset"]] == P[:info["colour_offset"]] and U[info["tile_offset"]:] == P[info["tile_offset"]:], name


def test_every_quality_gives_a_scale_in_range():
    assert all(16 <= tm.q16_of(q) <= 1024 for q in range(101))
    assert {q: tm.q16_of(q) for q in (100, 85, 50, 49, 25, 24, 1, 0)} == {100: 16, 85: 52, 50: 136, 49: 138, 25: 256, 24: 265, 1: 1024, 0: 1024}
    assert all(tm.q16_of(q) >= tm.q16_of(q + 1) for q in range(100))
    assert [tm.channel_q16(q, 1) for q in (16, 17, 512, 513, 1024)] == [16, 34, 1024, 1024, 1024] and tm.channel_q16(700, 0) == 700


def test_isqrt_is_the_exact_floor():
    for k in [1, 2, 3, 255, 256, 65535, 65536, (1 << 31) - 1, 1 << 31, 3037000499]:      # 3037000499^2 < 2^63 < 3037000500^2
        for v in (k * k - 1, k * k, k * k + 1):
            r = tm.isqrt(v)
            assert r * r <= v < (r + 1) * (r + 1)
    assert tm.isqrt(0) == 0 and tm.isqrt((1 << 63) - 1) == 3037000499


def test_steps_of_arrays_equal_the_scalar_rule():
    rng = np.random.default_rng(5)
    w1, w2 = rng.integers(1, 1 << 20, 3000), rng.integers(1, 1 << 20, 3000)
    w1[:100], w2[:100] = 1, rng.integers(1, 9, 100)
    for q in (16, 52, 136, 272, 1024):
        assert tm._steps(q, w1, w2).tolist() == [tm.step_of(q, a, b) for a, b in zip(w1, w2)]
    assert tm.step_of(1024, 1, 1) == 91 and tm.step_of(16, 1, 1) == 1 and tm.step_of(16, 1 << 31, 1 << 31) == 1


def test_floor_division_rounds_negative_numerators_down():
    assert [tm.floor_div(n, 2) for n in (-4, -3, -2, -1, 0, 1)] == [-2, -2, -1, -1, 0, 0]
    assert tm.floor_div(-7, 8) == -1 and tm.floor_div(-9, 8) == -2
    d = np.array([-81, -80, -1, 0, 1, 81], dtype=np.int64)
    assert tm._lift(d, np.int64(1), np.int64(7)).tolist() == [(7 * int(v) + 4) // 8 for v in d] == [-71, -70, -1, 0, 1, 71]
    # a butterfly with a negative d comes back exactly at step 1
    P = tm.leaves_packet([0, 1], grey([200, 3]), 1)
    assert tokens_of(tm.pack(P, 100))[0].tolist() == [[2 * 197 - 1, 0, 0]] and tm.unpack(tm.pack(P, 100)) == P


def test_clamping_comes_after_the_inverse_colour_transform():
    P = tm.leaves_packet([0, 1], [(255, 0, 255), (0, 255, 0)], 1)
    T = tm.pack(P, 0)
    zz, info = tokens_of(T)
    # Y = 127 for both, Cg = -255 and 255: d = 510, step 91, c = 6, d^ = 546; l = 0; a^ = -273, b^ = 273: G = -9 and 264 before the clamp
    assert info["q16"] == 1024 and zz.tolist() == [[0, 0, 12]] and info["dc"] == [127, 0, 0]
    v = tm.inverse(tm.levels_of(P, cm.parse(P)), zz, info["dc"], 1024, 2)
    assert v.tolist() == [[127, 0, -273], [127, 0, 273]]
    assert colours_of(tm.unpack(T)).tolist() == [[255, 0, 255], [0, 255, 0]]


def test_random_colours_at_quality_100_escape():
    P = max(random_packets().values(), key=len)
    zz, dc = tm.coefficients(P, 100)
    assert (zz >= 255).any() and zz.max() <= 2 * 510
    info = tm.parse(tm.pack(P, 100))
    for ch in range(3):
        token = [s for s in info["streams"] if s["kind"] == "token" and s["which"] == ch][0]
        tokens = tm._stream_values(tm.pack(P, 100), token, info)
        assert info["nescapes"][ch] == int((tokens == 255).sum()) == int((zz[:, ch] >= 255).sum()) > 0


def test_smooth_colours_cost_less_at_lower_quality():
    P = smooth_packet()
    sizes = [tm.colour_payload_bytes(tm.pack(P, q)) for q in QUALITIES]
    assert sizes == sorted(sizes, reverse=True) and sizes[-1] < sizes[0] / 3


_smooth = []


def smooth_packet():
    """20 000 points of the structured sphere at 8 bits, two tiles: several blocks per token stream, coded streams."""
    if not _smooth:
        _smooth.append(cm.encode(em.structured_cloud(20000, seed=1), 8, 100, 77))
    return _smooth[0]


# ---------------------------------------------------------------------------
# damages
# ---------------------------------------------------------------------------
def damage_packets():
    """The three packets whose damages are tried: raw streams only; coded streams, tiles, escapes; one leaf."""
    rnd = random_packets()
    mixed = [P for name, P in rnd.items() if cm.parse(P)["nleaves"] >= 4097 and cm.parse(P)["tile_mode"] == 1][0]
    return {"all eight children": tm.pack(hand_packets()["all eight children"], 100), "random with tiles": tm.pack(mixed, 100), "smooth": tm.pack(smooth_packet(), 50)}


def damages(packet):
    """(what, bytes) for each single-field damage of a cwat packet that the CONTAINER test must refuse."""
    p = bytes(packet)
    info = tm.parse(p)
    b, n = info["octree_bits"], info["nleaves"]
    head = 48 + 4 * b
    fixed, entries = head, head + tm.FIXED + 4
    streams = info["streams"]
    out = []
    edges = {0, 4, 8, 20, 48, head, head + 2, head + 8, head + tm.FIXED, entries, entries + 8 * len(streams), len(p) - 1}
    for s in streams:
        edges |= {s["offset"], s["offset"] + s["bytes"] - 1}
    for at in sorted(edges):
        if 0 <= at < len(p):
            out.append((f"truncated at {at}", p[:at]))
    out.append(("one byte appended", p + b"\x00"))
    out.append(("four bytes appended", p + bytes(4)))
    out.append(("magic of the entropy-coded packet", em.MAGIC + p[4:]))
    out.append(("magic", b"cwaT" + p[4:]))
    out.append(("version", p[:4] + struct.pack("<I", 2) + p[8:]))
    out.append(("octree_bits 0", p[:20] + b"\x00" + p[21:]))
    out.append(("colour bits 7", p[:21] + b"\x07" + p[22:]))
    out.append(("colour bits 9", p[:21] + b"\x09" + p[22:]))
    out.append(("reserved word", p[:36] + b"\x01" + p[37:]))
    out.append(("nleaves + 1", p[:16] + struct.pack("<I", n + 1) + p[20:]))
    for q in (0, 15, 1025, 65535):
        out.append((f"Q16 {q}", p[:fixed] + struct.pack("<H", q) + p[fixed + 2:]))
    for ch in range(3):
        at = fixed + 8 + 4 * ch
        out.append((f"nescapes[{ch}] == nleaves", p[:at] + struct.pack("<I", n) + p[at + 4:]))
        out.append((f"nescapes[{ch}] + 2", p[:at] + struct.pack("<I", info["nescapes"][ch] + 2) + p[at + 4:]))
        if info["nescapes"][ch] >= 2:
            out.append((f"nescapes[{ch}] - 2", p[:at] + struct.pack("<I", info["nescapes"][ch] - 2) + p[at + 4:]))
    for delta in (1, -1):
        out.append((f"S {delta:+d}", p[:entries - 4] + struct.pack("<I", len(streams) + delta) + p[entries:]))
    out.append(("tile mode flipped", p[:22] + bytes([1 - info["tile_mode"], 0]) + p[24:]))
    for i, s in enumerate(streams):
        entry = entries + 8 * i
        out.append((f"stream {i} mode 2", p[:entry] + struct.pack("<I", 2) + p[entry + 4:]))
        out.append((f"stream {i} mode flipped", p[:entry] + struct.pack("<I", 1 - s["mode"]) + p[entry + 4:]))
        for delta in (4, -4, 1):
            if s["bytes"] + delta >= 0:
                out.append((f"stream {i} payload_bytes {delta:+d}", p[:entry + 4] + struct.pack("<I", s["bytes"] + delta) + p[entry + 8:]))
        at = s["offset"]
        if s["mode"] == 0:
            for pad in range(at + s["used"], at + s["bytes"]):
                out.append((f"stream {i} pad byte", p[:pad] + b"\x01" + p[pad + 1:]))
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
        for what, value in (("odd", size + 1), ("off by two", size + 2), ("too small", 252), ("too large", 256 + 2 * em.BLOCK + 4), ("+4", size + 4)):
            out.append((f"stream {i} block_bytes {what}", p[:size_at] + struct.pack("<I", value) + p[size_at + 4:]))
    return out


def payload_damages(packet):
    """(what, bytes) for damages that the container test ACCEPTS: unpack must answer each with a packet or a reason, in bounds."""
    p = bytes(packet)
    info = tm.parse(p)
    head = 48 + 4 * info["octree_bits"]
    out = []
    for lo, hi in ((-32768, 32767), (32767, -32768)):
        out.append((f"dc {lo} {hi} {lo}", p[:head + 2] + struct.pack("<3h", lo, hi, lo) + p[head + 8:]))
    for s in info["streams"]:
        at, i = s["offset"], (s["kind"], s["which"])
        if s["kind"] == "token" and s["mode"] == 0 and s["symbols"]:
            q = bytearray(p[at:at + s["symbols"]])
            flipped = bytes(v ^ 0x55 for v in q)
            out.append((f"{i} tokens flipped", p[:at] + flipped + p[at + s["symbols"]:]))
            q[0] = 255 if q[0] != 255 else 0
            out.append((f"{i} one token to or from 255", p[:at] + bytes(q) + p[at + s["symbols"]:]))
            out.append((f"{i} every token 254", p[:at] + bytes([254]) * s["symbols"] + p[at + s["symbols"]:]))
        if s["kind"] == "escape" and s["symbols"]:
            out.append((f"{i} escapes 65535", p[:at] + b"\xff" * (2 * s["symbols"]) + p[at + 2 * s["symbols"]:]))
        if s["mode"] == 1:
            f = s["f"]
            used = np.nonzero(f)[0]
            if len(used) >= 2 and f[used].min() != f[used].max():
                a, c = int(used[np.argmax(f[used])]), int(used[np.argmin(f[used])])
                g = f.copy()
                g[a], g[c] = f[c], f[a]
                out.append((f"{i} f swapped", p[:at] + g.astype("<u2").tobytes() + p[at + 512:]))
            k = int(s["block_offsets"][-1])
            out.append((f"{i} state below 2^16", p[:k + 8] + struct.pack("<I", 0xffff) + p[k + 12:]))
            if s["kind"] == "token":
                # every symbol the most frequent one: a valid table whose blocks no longer fit
                g = np.zeros(256, dtype=np.int64)
                g[255] = 4096
                out.append((f"{i} every frequency on 255", p[:at] + g.astype("<u2").tobytes() + p[at + 512:]))
    return out


@pytest.mark.parametrize("name", list(damage_packets()))
def test_the_container_test_refuses_every_single_field_damage(name):
    T = damage_packets()[name]
    tm.parse(T)
    cases = damages(T)
    assert len(cases) > 60
    for what, data in cases:
        with pytest.raises(tm.Invalid):
            tm.parse(data)
            pytest.fail(what)


def model_answer(data):
    """("packet", bytes) or ("refused", reason) of unpack."""
    try:
        return "packet", tm.unpack(data)
    except tm.Invalid as e:
        return "refused", str(e)


@pytest.mark.parametrize("name", list(damage_packets()))
def test_payload_damages_pass_the_container_test_and_get_an_answer(name):
    T = damage_packets()[name]
    cases = payload_damages(T)
    assert len(cases) >= 5
    kinds = set()
    for what, data in cases:
        tm.parse(data)
        kind, answer = model_answer(data)
        kinds.add(kind)
        if kind == "packet":
            cm.parse(answer)                      # a valid packet: the colours are clamped, whatever the coefficients
    assert "packet" in kinds
    if name != "all eight children":
        assert "refused" in kinds


def escape_count_off_by_one():
    """(a packet with one escape in Y, the same with nescapes[0] == 2): the escape stream's padded size is 4 for both, so the container
    test passes and only the count of the tokens equal to 255 tells."""
    T = tm.pack(tm.leaves_packet([0, 1, 2], grey([0, 200, 100]), 1), 100)            # the z butterfly of (0, 1): d = 200, zz = 400
    info = tm.parse(T)
    assert info["nescapes"] == [1, 0, 0]
    at = 48 + 4 + 8
    return T, T[:at] + struct.pack("<I", 2) + T[at + 4:]


def test_escape_count_off_by_one_is_refused_by_the_token_count():
    good, more = escape_count_off_by_one()
    tm.unpack(good)
    tm.parse(more)
    with pytest.raises(tm.Invalid, match="escape count"):
        tm.unpack(more)
