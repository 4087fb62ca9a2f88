"""The octree codec's arithmetic and packet validator (csrc/codec_terms.hpp) compiled for the host as a stand-alone program
(tests/abi/codec_packet_host.cpp, its own main) with -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all, and held
to the numpy model (tests/codec_model.py) as RAW BITS: cells and keys of random points, the colour rule for every (m, s), the decoded
positions, and the validator on every valid model packet and on each of them after each of a list of damages: every damaged packet must
be refused with a message while the sanitizers stay silent (a validator that reads past a truncated packet aborts the program).  The
same damaged packets then go through packet_info of the built library, unsanitised, in Python.  CPU only; the kernels include the same
header.

Random points essentially never lie within an ulp of a cell boundary, which is the only place where a codec_cell with a reciprocal, a
folded factor or a float32 step differs from the rule: the cells are therefore also held to the model on the boundary clouds of
test_codec_model.py and on clouds at the edges of float32 (edge_clouds), and the validator and the decoded positions on valid packets
that no encoder makes (hand_built_packets).  The GPU tests (test_gpu_codec_edges.py) feed the same inputs to the kernels."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import codec_model as cm
from test_codec_model import BOUNDARY_CUBES, HAND_PACKET, boundary_cloud

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler: codec_terms.hpp cannot be checked"
    d = tmp_path_factory.mktemp("codec_packet")
    exe = str(d / "codec_packet_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "cwipc_util_amd", "csrc"), os.path.join(ROOT, "tests", "abi", "codec_packet_host.cpp"), "-o", exe], check=True)

    def run(mode, data, dtype):
        inp, out = str(d / "in.bin"), str(d / "out.bin")
        if isinstance(data, (bytes, bytearray)):
            with open(inp, "wb") as f:
                f.write(data)
        else:
            np.ascontiguousarray(data, dtype=np.float64).tofile(inp)
        proc = subprocess.run([exe, mode, inp, out], capture_output=True, text=True, timeout=300)
        assert proc.returncode == 0 and not proc.stderr, proc.stderr      # a sanitizer report ends the program with a message
        return np.fromfile(out, dtype=dtype)

    return run


def cloud_for_cells(rng, n):
    """Mixed signs, magnitudes 1e-3 .. 1e3, some points on the faces of the cube and some coincident."""
    scale = float(rng.choice([1e-3, 1.0, 37.0, 1e3]))
    pts = cm.random_cloud(rng, n, scale, rng.uniform(-2, 2, 3) * scale)
    xyz = np.stack([pts['x'], pts['y'], pts['z']], axis=1)
    lo, hi = xyz.min(axis=0), xyz.max(axis=0)
    for i in range(0, 60, 3):
        a = (i // 3) % 3
        xyz[i, a] = hi[a]
        xyz[i + 1, a] = lo[a]
        xyz[i + 2] = xyz[i + 1]
    pts['x'], pts['y'], pts['z'] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    return pts


@pytest.mark.parametrize("bits", [1, 2, 9, 16])
def test_cells_and_keys_equal_the_model(host, bits):
    rng = np.random.default_rng(100 + bits)
    pts = cloud_for_cells(rng, 6000)
    xyz = np.stack([pts['x'], pts['y'], pts['z']], axis=1).astype(np.float64)
    got = host("cells", np.concatenate([[bits, len(pts)], xyz.reshape(-1)]), np.uint64)
    mn, side = cm.cube(pts)
    assert got[:3].astype(np.uint32).tobytes() == mn.tobytes() and got[3:4].tobytes() == np.float64(side).tobytes()
    q = cm.cells(pts, mn, side, bits)
    rows = got[4:].reshape(-1, 4)
    assert np.array_equal(rows[:, :3].astype(np.int64), q)
    assert rows[:, 3].tobytes() == cm.keys(q, bits).tobytes()
    assert q.max() == (1 << bits) - 1 and q.min() == 0


def test_negative_zero_minimum_becomes_positive_zero(host):
    xyz = np.array([[-0.0, 0.0, 1.0], [0.0, -0.0, 2.0], [0.5, 0.25, 1.5]])
    got = host("cells", np.concatenate([[4, 3], xyz.reshape(-1)]), np.uint64)
    assert got[0] == 0 and got[1] == 0
    mn, _ = cm.cube(cm.make_cloud(xyz))
    assert mn.tobytes() == got[:3].astype(np.uint32).tobytes()


def test_colour_rule_for_every_value_and_shift(host):
    got = host("colour", [0.0], np.uint8)
    table = got[:5 * 256 * 2].reshape(5, 256, 2)
    for s in range(5):
        for m in range(256):
            assert table[s, m, 0] == cm.colour_store(m, s) and table[s, m, 1] == cm.colour_load(cm.colour_store(m, s), s), (s, m)
    assert got[5 * 256 * 2:].tolist() == [cm.colour_shift(q) for q in range(101)]


def test_leaf_means_are_rounded_in_integers(host):
    rng = np.random.default_rng(7)
    count = np.concatenate([[1, 1, 2, 2, 3, 3000, 3000, 2 ** 24, 2 ** 32 - 1], rng.integers(1, 5000, 500)]).astype(np.int64)
    total = np.concatenate([[0, 255, 255, 1, 382, 3000 * 255, 1499, 255 * 2 ** 24, 255 * (2 ** 32 - 1)], rng.integers(0, 256, 500) * count[9:] // 2]).astype(np.int64)
    got = host("mean", np.stack([total, count], axis=1).reshape(-1), np.uint32)
    assert got.tolist() == [(int(t) + int(c) // 2) // int(c) for t, c in zip(total, count)]


@pytest.mark.parametrize("bits", [1, 2, 9, 16])
def test_decoded_positions_equal_the_model(host, bits):
    rng = np.random.default_rng(200 + bits)
    pts = cloud_for_cells(rng, 3000)
    packet = cm.encode(pts, bits, 95)
    info = cm.parse(packet)
    lk = cm.leaf_keys_of(packet, info)
    record = np.concatenate([[bits, info["side"]], info["min"].astype(np.float64), [len(lk)], lk.astype(np.float64)])
    got = host("decode", record, np.uint32)
    dec, _, cell = cm.decode(packet)
    want = np.stack([dec['x'], dec['y'], dec['z']], axis=1)
    assert got[:-1].tobytes() == want.tobytes() and got[-1:].tobytes() == np.float32(cell).tobytes()


# ---------------------------------------------------------------------------
# the validator
# ---------------------------------------------------------------------------
def valid_packets():
    rng = np.random.default_rng(300)
    packets = [HAND_PACKET]
    for n, bits, quality in ((0, 1, 85), (0, 16, 10), (1, 1, 95), (1, 16, 85), (2, 2, 60), (65, 3, 30), (257, 9, 10), (700, 5, 85), (5003, 9, 85), (300, 16, 95)):
        pts = cm.random_cloud(rng, n, 2.0, (0.5, -1.0, 4.0))
        packets.append(cm.encode(pts, bits, quality, 1000 + n))
        pts['tile'] = 5
        packets.append(cm.encode(pts, bits, quality, 2000 + n))
    return packets


def damages(packet):
    """(what, bytes) for each damage the validator must refuse."""
    info = cm.parse(packet)
    b, n = info["octree_bits"], info["nleaves"]
    out = []
    boundaries = sorted({0, 4, 8, 16, 20, 21, 22, 23, 24, 36, 40, 48, 48 + 4 * b, info["colour_offset"], info["tile_offset"], len(packet)})
    for at in boundaries:
        if at < len(packet):
            out.append((f"truncated at {at}", packet[:at]))
    out.append(("truncated by one byte", packet[:-1]))
    out.append(("one byte appended", packet + b"\x00"))
    out.append(("magic", b"cwaO" + packet[4:]))
    out.append(("magic of the uncompressed packet", b"cpcd" + packet[4:]))
    out.append(("version", packet[:4] + struct.pack("<I", 2) + packet[8:]))
    for bad_bits in (0, 17):
        out.append((f"octree_bits {bad_bits}", packet[:20] + bytes([bad_bits]) + packet[21:]))
    for bad_cb in (3, 9):
        out.append((f"colour bits {bad_cb}", packet[:21] + bytes([bad_cb]) + packet[22:]))
    out.append(("tile mode 2", packet[:22] + b"\x02" + packet[23:]))
    out.append(("reserved word", packet[:36] + b"\x01" + packet[37:]))
    out.append(("side 0", packet[:40] + struct.pack("<d", 0.0) + packet[48:]))
    out.append(("side NaN", packet[:40] + struct.pack("<d", float("nan")) + packet[48:]))
    out.append(("min inf", packet[:24] + struct.pack("<f", float("inf")) + packet[28:]))
    for depth in range(b):
        at = 48 + 4 * depth
        value = struct.unpack("<I", packet[at:at + 4])[0]
        for delta in (1, -1):
            if value + delta >= 0:
                out.append((f"nodes[{depth}] {delta:+d}", packet[:at] + struct.pack("<I", value + delta) + packet[at + 4:]))
    for delta in (1, -1):
        if n + delta >= 0:
            out.append((f"nleaves {delta:+d}", packet[:16] + struct.pack("<I", n + delta) + packet[20:]))
    if n:
        occ = info["occupancy_offset"]
        for at in sorted({occ, occ + info["occupancy_bytes"] // 2, occ + info["occupancy_bytes"] - 1}):
            out.append((f"occupancy byte {at - occ} set to 0", packet[:at] + b"\x00" + packet[at + 1:]))
            for bit in (0, 7):
                flipped = packet[at] ^ (1 << bit)
                out.append((f"occupancy byte {at - occ} bit {bit} flipped", packet[:at] + bytes([flipped]) + packet[at + 1:]))
        for at in range(occ + info["occupancy_bytes"], info["colour_offset"]):
            out.append((f"occupancy pad byte {at}", packet[:at] + b"\x01" + packet[at + 1:]))
        for at in range(info["colour_offset"] + info["colour_bytes"], info["tile_offset"]):
            out.append((f"colour pad byte {at}", packet[:at] + b"\x80" + packet[at + 1:]))
        if (n * 3 * info["colour_bits"]) % 8:
            at = info["colour_offset"] + info["colour_bytes"] - 1
            out.append(("colour pad bits", packet[:at] + bytes([packet[at] | 0x80]) + packet[at + 1:]))
        if info["tile_mode"] == 0:
            out.append(("tile mode 1 without a plane", packet[:22] + b"\x01\x00" + packet[24:]))
        else:
            out.append(("tile mode 0 with a plane", packet[:22] + b"\x00" + packet[23:]))
            out.append(("tile value with a plane", packet[:23] + b"\x05" + packet[24:]))
    else:
        out.append(("tile value of an empty cloud", packet[:23] + b"\x01" + packet[24:]))
        out.append(("cube of an empty cloud", packet[:24] + struct.pack("<f", 1.0) + packet[28:]))
    return out


@pytest.fixture(scope="module")
def cases():
    good = valid_packets()
    bad = [(what, data) for packet in good for what, data in damages(packet)]
    for what, data in bad:                      # the model refuses every one of them too
        with pytest.raises(cm.Invalid):
            cm.parse(data)
    return good, bad


def test_validator_accepts_every_model_packet_and_refuses_every_damage(host, cases):
    good, bad = cases
    assert len(bad) > 40 * len(good) // 2
    stream = b"".join(struct.pack("<I", len(p)) + p for p in good + [data for _, data in bad])
    got = host("validate", stream, np.uint8).tobytes()
    at = 0
    for packet in good:
        assert got[at] == 1 and got[at + 1] == 0, "a valid packet was refused: " + got[at + 2:at + 2 + got[at + 1]].decode()
        nleaves, total = struct.unpack("<QQ", got[at + 2:at + 18])
        assert nleaves == cm.parse(packet)["nleaves"] and total == len(packet)
        at += 18
    for what, _ in bad:
        assert got[at] == 0, what
        assert got[at + 1] > 0, what + ": refused without a message"
        at += 2 + got[at + 1]
    assert at == len(got)


def test_packet_info_of_the_built_library(cwipc, cases):
    """The same packets through the library's exported validator, unsanitised; no GPU is touched."""
    import cwipc_util_amd.codec as codec
    good, bad = cases
    for packet in good:
        info, want = codec.packet_info(packet), cm.parse(packet)
        for key in ("timestamp", "nleaves", "octree_bits", "colour_bits", "tile_mode", "tile_value", "side", "nodes", "occupancy_offset", "colour_offset",
                    "tile_offset", "total_bytes"):
            assert info[key] == want[key], key
        assert np.array(info["min"], dtype=np.float32).tobytes() == want["min"].tobytes()
    for what, data in bad:
        with pytest.raises(cwipc.CwipcError) as err:
            codec.packet_info(data)
        assert len(str(err.value)) > 0, what


# ---------------------------------------------------------------------------
# cell boundaries and value edges
# ---------------------------------------------------------------------------
EDGE_BITS = (1, 9, 16)
_edge_clouds = {}


def edge_clouds():
    """name -> a cloud of about 500 finite points at an edge of float32: shared, read only, by this file and the GPU tests."""
    if _edge_clouds:
        return _edge_clouds
    rng = np.random.default_rng(400)
    n = 500

    def cloud(xyz):
        pts = cm.make_cloud(xyz, rng.integers(0, 256, (len(xyz), 3)))
        pts['tile'] = rng.choice(np.array([1, 2, 4], dtype=np.uint8), len(pts))
        return pts

    # denormals: k * 2^-149 for integers k < 4096, as bit patterns (no arithmetic that a flush to zero could spoil)
    k = rng.integers(0, 4096, (n, 3))
    k[0], k[1] = 0, 4095
    _edge_clouds["denormal"] = cloud(k.astype(np.uint32).view(np.float32))
    # nearly all of float32's range: the side (6.8e38) is beyond it
    xyz = rng.uniform(-3e38, 3e38, (n, 3)).astype(np.float32)
    for a in range(3):
        xyz[2 * a, a], xyz[2 * a + 1, a] = 3.4e38, -3.4e38
    _edge_clouds["huge"] = cloud(xyz)
    # ordinary and 1e-40-scale points, the minimum of every axis being the -0.0 of one point: the header holds +0
    xyz = rng.uniform(0.0, 1.0, (n, 3)).astype(np.float32)
    xyz[:200] = (rng.uniform(0.0, 9.0, (200, 3)) * 1e-40).astype(np.float32)
    xyz[:200][xyz[:200] == 0] = np.float32(1e-40)
    xyz[250] = -0.0
    _edge_clouds["negative zero minimum"] = cloud(xyz)
    # a line and a plane
    xyz = rng.uniform(-2.0, 3.0, (n, 3)).astype(np.float32)
    xyz[:, 0], xyz[:, 2] = 0.75, -1.25
    _edge_clouds["line"] = cloud(xyz)
    xyz = rng.uniform(-2.0, 3.0, (n, 3)).astype(np.float32)
    xyz[:, 1] = 0.1
    _edge_clouds["plane"] = cloud(xyz)
    # extent 2^-10 at 4096, where float32 has a spacing of 2^-11 (x, y) and of 2^-12 just below it (z)
    xyz = (4096.0 + rng.uniform(0.0, 2.0 ** -10, (n, 3))).astype(np.float32)
    xyz[:, 2] = (4096.0 - rng.uniform(0.0, 2.0 ** -10, n)).astype(np.float32)
    xyz[0], xyz[1] = (4096.0, 4096.0, 4096.0 - 2.0 ** -10), (4096.0 + 2.0 ** -10, 4096.0 + 2.0 ** -10, 4096.0)
    _edge_clouds["tiny extent far out"] = cloud(xyz)
    for pts in _edge_clouds.values():
        assert np.isfinite(np.stack([pts['x'], pts['y'], pts['z']])).all()
        pts.setflags(write=False)
    return _edge_clouds


def test_edge_clouds_are_what_they_say():
    clouds = edge_clouds()
    d = clouds["denormal"]
    assert cm.cube(d)[1] == 4095 * 2.0 ** -149 and 0 < d['x'].max() < np.finfo(np.float32).tiny
    assert cm.decode(cm.encode(d, 16, 85))[2].tobytes() == np.float32(0.0).tobytes()          # the cellsize, as float32, is exactly 0
    assert cm.cube(clouds["huge"])[1] > float(np.finfo(np.float32).max)
    z = clouds["negative zero minimum"]
    for axis in "xyz":
        assert z[axis].min() == 0 and np.signbit(z[axis][250]) and (z[axis][np.arange(len(z)) != 250] > 0).all()
    assert cm.cube(z)[0].tobytes() == bytes(12) and cm.encode(z, 9, 85)[24:36] == bytes(12)
    assert len(np.unique(clouds["tiny extent far out"]['x'])) == 3 and cm.cube(clouds["tiny extent far out"])[1] == 2.0 ** -10
    for pts in clouds.values():
        with np.errstate(over="raise", invalid="raise", divide="raise"):      # (underflow is what denormals are)
            for bits in EDGE_BITS:
                dec = cm.decode(cm.encode(pts, bits, 85))[0]
                assert np.isfinite(np.stack([dec['x'], dec['y'], dec['z']])).all()


def host_cells_equal_model(host, pts, bits):
    xyz = np.stack([pts['x'], pts['y'], pts['z']], axis=1).astype(np.float64)
    got = host("cells", np.concatenate([[bits, len(pts)], xyz.reshape(-1)]), np.uint64)
    mn, side = cm.cube(pts)
    assert got[:3].astype(np.uint32).tobytes() == mn.tobytes() and got[3:4].tobytes() == np.float64(side).tobytes()
    q = cm.cells(pts, mn, side, bits)
    rows = got[4:].reshape(-1, 4)
    assert np.array_equal(rows[:, :3].astype(np.int64), q)
    assert rows[:, 3].tobytes() == cm.keys(q, bits).tobytes()
    return q


@pytest.mark.parametrize("made_for", [1, 4, 9, 16])
@pytest.mark.parametrize("cube", range(len(BOUNDARY_CUBES)))
def test_cells_on_the_cell_boundaries(host, cube, made_for):
    """Points within a float32 ulp of every cell boundary: where codec_cell with a reciprocal, a folded factor or a float32 step would
    differ from the rule (test_codec_model.py holds the clouds to that).  At the depth the cloud was made for and at its neighbours."""
    pts = boundary_cloud(cube, made_for)
    for bits in sorted({made_for, max(1, made_for - 1), min(16, made_for + 1)}):
        q = host_cells_equal_model(host, pts, bits)
        assert q.min() == 0 and q.max() == (1 << bits) - 1


@pytest.mark.parametrize("bits", EDGE_BITS)
def test_cells_at_the_edges_of_float32(host, bits):
    for name, pts in edge_clouds().items():
        host_cells_equal_model(host, pts, bits)


# ---------------------------------------------------------------------------
# valid packets that no encoder makes
# ---------------------------------------------------------------------------
BIG_TIMESTAMP = (1 << 63) + 5
_hand_built = []


def hand_built_packets():
    """[(name, packet)]: trees and headers that are valid by the rule and come out of no encoder, made with cm.build_packet.  Shared,
    read only, with the GPU tests, which feed them to the decoder."""
    if _hand_built:
        return _hand_built
    rng = np.random.default_rng(500)

    def packet(name, lk, bits, cb=8, tiles=None, mn=(0.5, -1.0, 4.0), side=2.0, timestamp=77, tile_mode=None):
        lk = np.asarray(lk, dtype=np.uint64)
        tiles = rng.choice(np.array([1, 2, 4, 8], dtype=np.uint8), len(lk)) if tiles is None else tiles
        _hand_built.append((name, cm.build_packet(lk, rng.integers(0, 1 << cb, (len(lk), 3)), tiles, mn, side, bits, cb, timestamp, tile_mode)))

    def some_keys(n, bits):
        return np.sort(rng.choice(1 << (3 * bits), n, replace=False)).astype(np.uint64)

    packet("full tree at 5 bits", np.arange(1 << 15), 5)
    chain = int(rng.integers(0, 1 << 45))
    packet("a chain at 16 bits ending in 8 children", (chain << 3) + np.arange(8), 16)
    corners = np.array([[0, 0, 0], [0, 0, 65535], [0, 65535, 0], [65535, 0, 0], [65535, 65535, 65535], [65535, 65534, 65535]])
    packet("q = 65535 on each axis", np.sort(cm.keys(corners, 16)), 16)
    for cb in (4, 5, 6, 7, 8):
        for n in (1, 2, 3, 11):
            packet(f"{cb} colour bits, {n} leaves", some_keys(n, 3), 3, cb=cb)
    packet("tile_mode 0, tile_value 255", some_keys(40, 4), 4, tiles=np.full(40, 255, dtype=np.uint8), tile_mode=0)
    tiles = rng.integers(0, 3, 300).astype(np.uint8)
    tiles[:5] = 0
    packet("a tile plane with zeros", some_keys(300, 6), 6, tiles=tiles, tile_mode=1)
    packet("a tile plane of zeros only", some_keys(7, 2), 2, tiles=np.zeros(7, dtype=np.uint8), tile_mode=1)
    packet("min -0.0", some_keys(100, 7), 7, mn=(-0.0, -0.0, 1.0))
    packet("min with a denormal", some_keys(100, 7), 7, mn=(1e-42, -3e-45, 1.0), side=1e-38)
    for side in (2.0 ** -60, 1.0, 1e30):
        packet(f"side {side!r}", some_keys(257, 9), 9, side=side)
    packet("timestamp 2^63 + 5", some_keys(50, 5), 5, timestamp=BIG_TIMESTAMP)
    # A side above float32's range.  The rule's decoding ends in (float) of a float64 beyond float32's range, which IEEE 754 rounds to
    # infinity, as numpy's cast does: model and rule agree on the bytes (children 0 and 7 of the root: 2.5e38 and +inf; cellsize +inf).
    packet("side 1e39", [0, 7], 1, mn=(0.0, 0.0, 0.0), side=1e39)
    for _, p in _hand_built:
        cm.parse(p)
    return _hand_built


def test_hand_built_packets_are_what_they_say():
    by_name = dict(hand_built_packets())
    full = cm.parse(by_name["full tree at 5 bits"])
    assert full["nodes"] == [8, 64, 512, 4096, 32768]
    assert by_name["full tree at 5 bits"][full["occupancy_offset"]:full["occupancy_offset"] + full["occupancy_bytes"]] == b"\xff" * 4681
    assert cm.parse(by_name["a chain at 16 bits ending in 8 children"])["nodes"] == [1] * 15 + [8]
    assert struct.unpack("<Q", by_name["timestamp 2^63 + 5"][8:16])[0] == BIG_TIMESTAMP
    assert by_name["min -0.0"][24:36] == struct.pack("<3f", -0.0, -0.0, 1.0) and by_name["min -0.0"][27] == 0x80
    info = cm.parse(by_name["tile_mode 0, tile_value 255"])
    assert (info["tile_mode"], info["tile_value"]) == (0, 255)
    ends = {(cm.parse(p)["nleaves"] * 3 * cm.parse(p)["colour_bits"]) % 32 for name, p in by_name.items() if "colour bits" in name}
    assert any(e % 8 for e in ends) and {8, 16, 24} <= ends             # the colour plane ends inside a byte, and at each byte inside a word
    dec, _, cell = cm.decode(by_name["side 1e39"])
    assert dec['x'].tolist() == [np.float32(2.5e38), np.inf] and np.isinf(cell)
    dec = cm.decode(by_name["q = 65535 on each axis"])[0]
    assert dec['x'].max() == np.float32(0.5 + 65535.5 * 2.0 / 65536)


@pytest.fixture(scope="module")
def hand_cases():
    good = [p for _, p in hand_built_packets()]
    bad = [(name + ": " + what, data) for name, packet in hand_built_packets() for what, data in damages(packet)]
    for what, data in bad:
        with pytest.raises(cm.Invalid):
            cm.parse(data)
    return good, bad


def test_validator_accepts_every_hand_built_packet_and_refuses_its_damages(host, hand_cases):
    good, bad = hand_cases
    stream = b"".join(struct.pack("<I", len(p)) + p for p in good + [data for _, data in bad])
    got = host("validate", stream, np.uint8).tobytes()
    at = 0
    for (name, packet) in hand_built_packets():
        assert got[at] == 1 and got[at + 1] == 0, name + " was refused: " + got[at + 2:at + 2 + got[at + 1]].decode()
        nleaves, total = struct.unpack("<QQ", got[at + 2:at + 18])
        assert nleaves == cm.parse(packet)["nleaves"] and total == len(packet), name
        at += 18
    for what, _ in bad:
        assert got[at] == 0, what
        assert got[at + 1] > 0, what + ": refused without a message"
        at += 2 + got[at + 1]
    assert at == len(got)


def test_decoded_positions_of_hand_built_packets_equal_the_model(host):
    for name, packet in hand_built_packets():
        info = cm.parse(packet)
        lk = cm.leaf_keys_of(packet, info)
        record = np.concatenate([[info["octree_bits"], info["side"]], info["min"].astype(np.float64), [len(lk)], lk.astype(np.float64)])
        got = host("decode", record, np.uint32)
        dec, _, cell = cm.decode(packet)
        want = np.stack([dec['x'], dec['y'], dec['z']], axis=1)
        assert got[:-1].tobytes() == want.tobytes() and got[-1:].tobytes() == np.float32(cell).tobytes(), name


def test_packet_info_of_hand_built_packets(cwipc, hand_cases):
    import cwipc_util_amd.codec as codec
    good, bad = hand_cases
    for packet in good:
        info, want = codec.packet_info(packet), cm.parse(packet)
        for key in ("timestamp", "nleaves", "octree_bits", "colour_bits", "tile_mode", "tile_value", "side", "nodes", "occupancy_offset", "colour_offset",
                    "tile_offset", "total_bytes"):
            assert info[key] == want[key], key
        assert np.array(info["min"], dtype=np.float32).tobytes() == want["min"].tobytes()
    for what, data in bad:
        with pytest.raises(cwipc.CwipcError) as err:
            codec.packet_info(data)
        assert len(str(err.value)) > 0, what
