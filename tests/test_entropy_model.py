"""RULE E (the entropy-coded packet form "cwae": include/cwipc_util_amd/hip_ext.h) in its numpy restatement (tests/entropy_model.py):
the round trip, the size bound, the mode decisions and the frequency rule on their edge cases, and a block worked out by hand.  CPU
only, the model alone; test_entropy_host.py holds csrc/entropy_terms.hpp to the same cases and test_gpu_entropy.py the kernels."""
import struct

import numpy as np
import pytest

import codec_model as cm
import entropy_model as em

BLOCK_SIZES = (1, 63, 64, 65, 4095, 4096, 4097, 8193)


def skewed(rng, m, alphabet=256):
    """m symbols, geometrically distributed over `alphabet` values: compressible, and every state path is taken."""
    return np.minimum(rng.geometric(0.3, m) - 1, alphabet - 1).astype(np.int64)


def round_trip_stream(symbols, f=None):
    f = em.normalise(np.bincount(symbols, minlength=256)) if f is None else f
    blocks = em.encode_blocks(symbols, f)
    counts = [min(em.BLOCK, len(symbols) - em.BLOCK * k) for k in range(len(blocks))]
    slots = []
    for states, words in blocks:
        data = em.block_bytes(states, words)
        assert len(data) % 4 == 0 and 256 <= len(data) <= 256 + 2 * em.BLOCK and len(words) <= em.BLOCK
        assert (states >= em.LOW).all() and (states < (1 << 32)).all()
        slots.append((np.frombuffer(data, dtype="<u4", count=64), np.frombuffer(data, dtype="<u2", offset=256)))
    got, intact = em.decode_blocks(slots, counts, f)
    assert intact.all() and np.array_equal(got, symbols)
    return blocks


@pytest.mark.parametrize("m", BLOCK_SIZES)
def test_blocks_of_every_size_round_trip(m):
    rng = np.random.default_rng(m)
    blocks = round_trip_stream(skewed(rng, m))
    assert len(blocks) == (m + 4095) // 4096
    if m < 64:
        assert (blocks[0][0][m:] == em.LOW).all()          # a lane that never had a symbol keeps 2^16


def test_one_distinct_symbol_emits_no_word():
    symbols = np.full(5000, 37, dtype=np.int64)
    f = em.normalise(np.bincount(symbols, minlength=256))
    assert f[37] == 4096 and f.sum() == 4096
    for states, words in round_trip_stream(symbols, f):
        assert len(words) == 0 and (states == em.LOW).all()
    assert len(em.coded_payload("tile", symbols, 8)) == 512 + 4 * 2 + 256 * 2


def test_all_256_symbols():
    rng = np.random.default_rng(2)
    symbols = np.concatenate([np.arange(256), skewed(rng, 9000)])
    rng.shuffle(symbols)
    f = em.normalise(np.bincount(symbols, minlength=256))
    assert (f > 0).all()
    round_trip_stream(symbols, f)


def test_normalise_takes_from_the_largest_when_the_floors_exceed():
    counts = np.ones(256, dtype=np.int64)
    counts[100] += 10 ** 6
    f = em.normalise(counts)
    assert f[100] == 3841 and (np.delete(f, 100) == 1).all() and f.sum() == 4096
    # decrements move to the next largest once the first is no longer alone at the top; the lowest symbol goes first on ties
    counts = np.ones(256, dtype=np.int64)
    counts[[7, 200]] = 4000
    f = em.normalise(counts)
    assert f.sum() == 4096 and (np.delete(f, [7, 200]) == 1).all() and f[7] == 1921 and f[200] == 1921
    counts[3] = 2
    f = em.normalise(counts)
    assert f.sum() == 4096 and f[3] == 1 and abs(int(f[7]) - int(f[200])) <= 1 and f[7] <= f[200]


def test_normalise_gives_the_remainder_to_the_largest_count_lowest_symbol_on_ties():
    counts = np.zeros(256, dtype=np.int64)
    counts[[5, 9, 11]] = 1
    f = em.normalise(counts)                        # 1365 each, 1 left over
    assert f[5] == 1366 and f[9] == 1365 and f[11] == 1365
    counts[[5, 9, 11]] = (3, 7, 7)
    f = em.normalise(counts)                        # floors 722, 1686, 1686: 2 left over for symbol 9
    assert f.tolist()[5] == 722 and f[9] == 1688 and f[11] == 1686
    rng = np.random.default_rng(3)
    for _ in range(50):
        counts = rng.integers(0, 4, 256) * rng.integers(0, 1000, 256)
        if counts.sum():
            f = em.normalise(counts)
            assert f.sum() == 4096 and ((f > 0) == (counts > 0)).all()


# The block worked out by hand.  65 symbols, f[7] = 4095 (cum 0), f[9] = 1 (cum 4095); all are 7 but symbols 0 and 64, which are 9 and
# both belong to lane 0 (rounds 0 and 1).
#   Encoder, round 1: lane 0 takes 9: 65536 < 1 << 20, no word; x = 65536 * 4096 + 0 + 4095 = 0x10000fff.
#   Encoder, round 0: lanes 63 .. 1 take 7: x = (65536 / 4095) * 4096 + 65536 % 4095 + 0 = 16 * 4096 + 16 = 0x10010.
#                     lane 0 takes 9: 0x10000fff >= 1 << 20: the word 0x0fff goes out, x = 0x1000; then x = 0x1000 * 4096 + 4095 = 0x01000fff.
#   Decoder, round 0: lane 0: slot 0xfff is symbol 9, x = 1 * 0x1000 + 0 = 0x1000 < 2^16, takes the word: 0x10000fff.
#                     lane l > 0: slot 0x010 is symbol 7, x = 4095 * 16 + 16 = 2^16.
#   Decoder, round 1: lane 0: slot 0xfff is symbol 9, x = 1 * 0x10000 + 0 = 2^16.  One word, one padding word: 260 bytes.
HAND_SYMBOLS = np.array([9] + [7] * 63 + [9], dtype=np.int64)
HAND_F = np.zeros(256, dtype=np.int64)
HAND_F[7], HAND_F[9] = 4095, 1
HAND_BLOCK = struct.pack("<I", 0x01000fff) + struct.pack("<I", 0x00010010) * 63 + struct.pack("<HH", 0x0fff, 0)


def test_hand_worked_block():
    assert len(HAND_BLOCK) == 260
    (states, words), = em.encode_blocks(HAND_SYMBOLS, HAND_F)
    assert em.block_bytes(states, words) == HAND_BLOCK
    slots = [(np.frombuffer(HAND_BLOCK, dtype="<u4", count=64), np.frombuffer(HAND_BLOCK, dtype="<u2", offset=256))]
    got, intact = em.decode_blocks(slots, [65], HAND_F)
    assert intact.all() and np.array_equal(got, HAND_SYMBOLS)
    for at, value in ((0, 0x01000ffe), (256, 0x0ffe), (258, 1), (4, 0xffff)):          # a state, the word, the padding word, a state below 2^16
        bad = bytearray(HAND_BLOCK)
        bad[at:at + 2] = struct.pack("<H", value & 0xffff)
        if at < 256:
            bad[at:at + 4] = struct.pack("<I", value)
        slots = [(np.frombuffer(bytes(bad), dtype="<u4", count=64), np.frombuffer(bytes(bad), dtype="<u2", offset=256))]
        assert not em.decode_blocks(slots, [65], HAND_F)[1].any(), at
    short = [(np.frombuffer(HAND_BLOCK, dtype="<u4", count=64), np.zeros(0, dtype="<u2"))]      # the word is missing: a read past the block
    assert not em.decode_blocks(short, [65], HAND_F)[1].any()


# ---------------------------------------------------------------------------
# whole packets
# ---------------------------------------------------------------------------
def smooth_packet(n, bits=6, cb=7, tile_mode=1, rng=None):
    """A tree of n leaves with slowly varying colours and long tile runs: every stream of n symbols is compressible."""
    rng = rng or np.random.default_rng(n)
    lk = np.sort(rng.choice(1 << (3 * bits), n, replace=False)).astype(np.uint64)
    t = np.arange(n)
    colours = np.stack([(t // 40) % (1 << cb), (t // 25 + 3) % (1 << cb), (t // 60 + 9) % (1 << cb)], axis=1)
    tiles = np.where((t // 500) % 2 == 0, 1, 2).astype(np.uint8) if tile_mode == 1 else np.full(n, 3, dtype=np.uint8)
    return cm.build_packet(lk, colours, tiles, (0.5, -1.0, 4.0), 2.0, bits, cb, 99, tile_mode)


_packets = {}


def model_packets():
    """name -> cwao packet: the cases of the issue, shared (read only) with the host-program and GPU tests."""
    if _packets:
        return _packets
    rng = np.random.default_rng(700)
    _packets["empty"] = cm.encode(cm.random_cloud(rng, 0), 9, 85, 5)
    _packets["one leaf, 1 bit"] = cm.encode(cm.random_cloud(rng, 1), 1, 85, 6)
    _packets["one leaf, 16 bits"] = cm.encode(cm.random_cloud(rng, 1), 16, 95, 7)
    _packets["random 700"] = cm.encode(cm.random_cloud(rng, 700), 5, 85, 8)
    _packets["random 5003"] = cm.encode(cm.random_cloud(rng, 5003), 9, 60, 9)
    _packets["random 9000, 16 bits"] = cm.encode(cm.random_cloud(rng, 9000), 16, 10, 10)
    _packets["4095 smooth leaves"] = smooth_packet(4095)
    _packets["4096 smooth leaves"] = smooth_packet(4096)
    _packets["4097 smooth leaves, no tile plane"] = smooth_packet(4097, tile_mode=0)
    _packets["8193 smooth leaves, 4 colour bits"] = smooth_packet(8193, bits=7, cb=4)
    _packets["9000 smooth leaves, 8 colour bits"] = smooth_packet(9000, bits=8, cb=8)
    structured = em.structured_cloud()
    _packets["structured, 9 bits"] = cm.encode(structured, 9, 85, 11)
    _packets["structured, 7 bits"] = cm.encode(structured, 7, 85, 12)
    noisy = structured.copy()
    noisy['r'], noisy['g'], noisy['b'] = rng.integers(0, 256, (3, len(noisy)))
    _packets["structured, random colours"] = cm.encode(noisy, 9, 95, 13)
    return _packets


_packed = {}


def packed(name):
    if name not in _packed:
        _packed[name] = em.pack(model_packets()[name])
    return _packed[name]


@pytest.mark.parametrize("name", list(model_packets()))
def test_round_trip_and_size_bound(name):
    p = model_packets()[name]
    e = packed(name)
    assert e[:4] == b"cwae" and e[8:48 + 4 * p[20]] == p[8:48 + 4 * p[20]]
    assert em.unpack(e) == p
    info = em.parse(e)
    S = len(info["streams"])
    assert S == (0 if info["nleaves"] == 0 else info["octree_bits"] + 3 + info["tile_mode"])
    assert len(e) <= len(p) + 4 + 11 * S
    for s in info["streams"]:
        assert s["mode"] == 0 or s["symbols"] >= 4096


def test_empty_cloud_has_no_streams():
    e = packed("empty")
    assert len(e) == 48 + 36 + 4 and e[-4:] == bytes(4)


def test_threshold_between_4095_and_4096_symbols():
    below, at = em.parse(packed("4095 smooth leaves")), em.parse(packed("4096 smooth leaves"))
    assert all(s["mode"] == 0 for s in below["streams"])
    assert [s["mode"] for s in at["streams"] if s["kind"] != "occupancy"] == [1, 1, 1, 1]
    assert len(packed("4096 smooth leaves")) < len(model_packets()["4096 smooth leaves"]) < len(packed("4095 smooth leaves"))


def test_uniformly_random_bytes_come_out_raw():
    rng = np.random.default_rng(8)
    values = rng.integers(0, 256, 20000)
    assert len(em.coded_payload("tile", values, 8)) > len(em.raw_payload("tile", values, 8))
    n = 6000
    lk = np.sort(rng.choice(1 << 18, n, replace=False)).astype(np.uint64)
    p = cm.build_packet(lk, rng.integers(0, 256, (n, 3)), rng.integers(0, 256, n).astype(np.uint8), (0, 0, 0), 1.0, 6, 8, 1, 1)
    e = em.pack(p)
    assert [s["mode"] for s in em.parse(e)["streams"] if s["kind"] != "occupancy"] == [0, 0, 0, 0]
    assert em.unpack(e) == p and len(e) <= len(p) + 4 + 11 * 10


def test_the_structured_cloud_is_what_the_gpu_tests_need():
    """A condition on the inputs, not on the code: coded occupancy, colour and tile streams, and a smaller packet."""
    for name in ("structured, 9 bits", "structured, 7 bits"):
        info = em.parse(packed(name))
        kinds = {(s["kind"], s["mode"]) for s in info["streams"]}
        assert ("colour", 1) in kinds and ("tile", 1) in kinds and ("colour", 0) not in kinds, name
        assert len(packed(name)) < len(model_packets()[name])
    assert ("occupancy", 1) in {(s["kind"], s["mode"]) for s in em.parse(packed("structured, 9 bits"))["streams"]}
    noisy = em.parse(packed("structured, random colours"))
    assert [s["mode"] for s in noisy["streams"] if s["kind"] == "colour"] == [0, 0, 0]


def test_damaged_containers_are_refused():
    count = 0
    for name in ("empty", "random 700", "4096 smooth leaves", "8193 smooth leaves, 4 colour bits", "structured, 7 bits"):
        for what, data in em.damages(packed(name)):
            with pytest.raises(em.Invalid):
                em.parse(data)
            count += 1
    assert count > 200


def test_damaged_payloads_pass_the_container_test_and_fail_the_blocks():
    count = 0
    for name in ("4096 smooth leaves", "8193 smooth leaves, 4 colour bits", "structured, 9 bits"):
        for what, data in em.payload_damages(packed(name)):
            em.parse(data)
            with pytest.raises(em.Invalid):
                em.unpack(data)
            count += 1
    assert count > 40
