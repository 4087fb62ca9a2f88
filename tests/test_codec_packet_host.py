"""The octree codec's arithmetic and packet validator (csrc/codec_terms.hpp) compiled for the host as a stand-alone program
(tests/abi/codec_packet_host.cpp, its own main) with -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all, and held
to the numpy model (tests/codec_model.py) as RAW BITS: cells and keys of random points, the colour rule for every (m, s), the decoded
positions, and the validator on every valid model packet and on each of them after each of a list of damages: every damaged packet must
be refused with a message while the sanitizers stay silent (a validator that reads past a truncated packet aborts the program).  The
same damaged packets then go through packet_info of the built library, unsanitised, in Python.  CPU only; the kernels include the same
header."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import codec_model as cm
from test_codec_model import HAND_PACKET

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
