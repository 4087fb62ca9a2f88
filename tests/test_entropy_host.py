"""RULE E's host code (csrc/entropy_terms.hpp: normalisation, block coder, container validator, pack and unpack of whole packets)
compiled as a stand-alone program (tests/abi/entropy_host.cpp, its own main) with -fsanitize=address,undefined
-fno-sanitize-recover=all and held to the numpy model (tests/entropy_model.py) as raw bytes.  The validator must refuse every damaged
container, and the block decoder every damaged payload that the validator lets through, with a message and with the sanitizers silent:
the per-symbol steps, the slot search and the bounded word read are the functions the kernels call, so this is the evidence that they
stay inside their buffers for any bytes.  The same packets then go through the built library's host entries in Python, unsanitised.
CPU only."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import codec_model as cm
import entropy_model as em
from test_entropy_model import BLOCK_SIZES, HAND_BLOCK, HAND_F, HAND_SYMBOLS, model_packets, packed, skewed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler: entropy_terms.hpp cannot be checked"
    d = tmp_path_factory.mktemp("entropy_host")
    exe = str(d / "entropy_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "cwipc_util_amd", "csrc"), os.path.join(ROOT, "tests", "abi", "entropy_host.cpp"), "-o", exe], check=True)

    def run(mode, data):
        inp, out = str(d / "in.bin"), str(d / "out.bin")
        with open(inp, "wb") as f:
            f.write(data)
        proc = subprocess.run([exe, mode, inp, out], capture_output=True, text=True, timeout=300)
        assert proc.returncode == 0 and not proc.stderr, proc.stderr      # a sanitizer report ends the program with a message
        with open(out, "rb") as f:
            return f.read()

    return run


def framed(packets):
    return b"".join(struct.pack("<I", len(p)) + bytes(p) for p in packets)


def results(got, count):
    """[(True, packet) | (False, message)] of a pack or unpack run."""
    out, at = [], 0
    for _ in range(count):
        if got[at] == 1:
            n = struct.unpack("<I", got[at + 1:at + 5])[0]
            out.append((True, got[at + 5:at + 5 + n]))
            at += 5 + n
        else:
            out.append((False, got[at + 2:at + 2 + got[at + 1]].decode()))
            at += 2 + got[at + 1]
    assert at == len(got)
    return out


def test_normalise_equals_the_model(host):
    rng = np.random.default_rng(1)
    sets = []
    big = np.ones(256, dtype=np.int64)
    big[100] += 10 ** 6
    sets.append(big)
    ties = np.ones(256, dtype=np.int64)
    ties[[7, 200]] = 4000
    sets.append(ties)
    few = np.zeros(256, dtype=np.int64)
    few[[5, 9, 11]] = 1
    sets.append(few)
    one = np.zeros(256, dtype=np.int64)
    one[255] = 2 ** 32 - 1
    sets.append(one)
    sets.append(np.full(256, 2 ** 24, dtype=np.int64))
    for _ in range(60):
        sets.append(rng.integers(0, 4, 256) * rng.integers(0, 100000, 256) + (rng.integers(0, 256) == np.arange(256)))
    got = np.frombuffer(host("normalise", b"".join(s.astype("<u4").tobytes() for s in sets)), dtype="<u2").reshape(-1, 256)
    for s, f in zip(sets, got):
        assert np.array_equal(f, em.normalise(s))
    assert got[0][100] == 3841


@pytest.mark.parametrize("m", [s for s in BLOCK_SIZES if s <= 4096] + [2, 129, 1000])
def test_blocks_equal_the_model(host, m):
    rng = np.random.default_rng(10 + m)
    records, wants = b"", []
    for alphabet in (2, 16, 256):
        symbols = skewed(rng, m, alphabet)
        f = em.normalise(np.bincount(symbols, minlength=256))
        (states, words), = em.encode_blocks(symbols, f)
        wants.append((symbols, f, em.block_bytes(states, words)))
        records += struct.pack("<I", m) + f.astype("<u2").tobytes() + symbols.astype(np.uint8).tobytes()
    got, at = host("encode", records), 0
    for symbols, f, block in wants:
        n = struct.unpack("<I", got[at:at + 4])[0]
        assert got[at + 4:at + 4 + n] == block
        at += 4 + n
    assert at == len(got)
    records = b"".join(struct.pack("<I", m) + f.astype("<u2").tobytes() + struct.pack("<I", len(block)) + block for _, f, block in wants)
    got, at = host("decode", records), 0
    for symbols, _, _ in wants:
        assert got[at] == 1 and got[at + 1:at + 1 + m] == symbols.astype(np.uint8).tobytes()
        at += 1 + m


def test_hand_worked_block(host):
    table = HAND_F.astype("<u2").tobytes()
    got = host("encode", struct.pack("<I", 65) + table + HAND_SYMBOLS.astype(np.uint8).tobytes())
    assert got == struct.pack("<I", 260) + HAND_BLOCK
    got = host("decode", struct.pack("<I", 65) + table + struct.pack("<I", 260) + HAND_BLOCK)
    assert got == b"\x01" + HAND_SYMBOLS.astype(np.uint8).tobytes()
    # the word missing, the padding word set, a state below 2^16, a state of 0xffffffff, a table that gives every slot to one symbol
    bad = [HAND_BLOCK[:256], HAND_BLOCK[:258] + b"\x01\x00", HAND_BLOCK[:8] + struct.pack("<I", 0xffff) + HAND_BLOCK[12:],
           HAND_BLOCK[:252] + struct.pack("<I", 0xffffffff) + HAND_BLOCK[256:]]
    records = b"".join(struct.pack("<I", 65) + table + struct.pack("<I", len(b)) + b for b in bad)
    other = np.zeros(256, dtype="<u2")
    other[255] = 4096
    records += struct.pack("<I", 65) + other.tobytes() + struct.pack("<I", 260) + HAND_BLOCK
    got = host("decode", records)
    assert [got[66 * i] for i in range(5)] == [0] * 5


def test_random_bytes_as_blocks_stay_in_bounds(host):
    """Any bytes, any table (even one whose sum is not 4096, which the container test would have refused): the decoder reports and the
    sanitizers stay silent."""
    rng = np.random.default_rng(5)
    records = b""
    for i in range(200):
        m = int(rng.integers(1, 4097))
        size = 256 + 4 * int(rng.integers(0, 2049))
        table = rng.integers(0, 65536 if i % 2 else 64, 256).astype("<u2")
        records += struct.pack("<I", m) + table.tobytes() + struct.pack("<I", size) + rng.integers(0, 256, size).astype(np.uint8).tobytes()
    got = host("decode", records)
    assert len(got) > 200


NAMES = list(model_packets())


def test_pack_and_unpack_equal_the_model(host):
    plain = [model_packets()[n] for n in NAMES]
    coded = [packed(n) for n in NAMES]
    for name, want, (ok, got) in zip(NAMES, coded, results(host("pack", framed(plain)), len(plain))):
        assert ok and got == want, name
    for name, want, (ok, got) in zip(NAMES, plain, results(host("unpack", framed(coded)), len(coded))):
        assert ok and got == want, name
    # a packet of the wrong form is refused by both
    assert not results(host("pack", framed(coded[:3])), 3)[1][0] and not results(host("unpack", framed(plain[:3])), 3)[1][0]


@pytest.fixture(scope="module")
def container_cases():
    bad = [(name + ": " + what, data) for name in NAMES for what, data in em.damages(packed(name))]
    for what, data in bad:
        with pytest.raises(em.Invalid):
            em.parse(data)
    return bad


@pytest.fixture(scope="module")
def payload_cases():
    bad = [(name + ": " + what, data) for name in NAMES for what, data in em.payload_damages(packed(name))]
    for what, data in bad:
        em.parse(data)
        with pytest.raises(em.Invalid):
            em.unpack(data)
    return bad


def test_validator_accepts_every_model_packet_and_refuses_every_damage(host, container_cases):
    good = [packed(n) for n in NAMES]
    assert len(container_cases) > 40 * len(good)
    got, at = host("validate", framed(good + [data for _, data in container_cases])), 0
    for name, packet in zip(NAMES, good):
        assert got[at] == 1, name + " was refused: " + got[at + 2:at + 2 + got[at + 1]].decode()
        S = struct.unpack("<I", got[at + 1:at + 5])[0]
        entries = struct.unpack("<%dI" % (2 * S), got[at + 5:at + 5 + 8 * S])
        assert list(zip(entries[0::2], entries[1::2])) == em.directory(packet), name
        at += 5 + 8 * S
    for what, _ in container_cases:
        assert got[at] == 0, what
        assert got[at + 1] > 0, what + ": refused without a message"
        at += 2 + got[at + 1]
    assert at == len(got)
    # and unpack refuses them too, before it decodes anything
    assert not any(ok for ok, _ in results(host("unpack", framed([data for _, data in container_cases])), len(container_cases)))


def test_damaged_payloads_pass_the_validator_and_are_refused_by_the_decoder(host, payload_cases):
    assert len(payload_cases) > 100
    data = [d for _, d in payload_cases]
    got, at = host("validate", framed(data)), 0
    for what, _ in payload_cases:
        assert got[at] == 1, what
        at += 5 + 8 * struct.unpack("<I", got[at + 1:at + 5])[0]
    reasons = set()
    for (what, _), (ok, message) in zip(payload_cases, results(host("unpack", framed(data)), len(data))):
        assert not ok, what
        assert message in ("entropy-coded block is not intact", "occupancy byte is 0", "occupancy bits differ from the node count"), what
        reasons.add(message)
    assert "entropy-coded block is not intact" in reasons


def test_host_entries_of_the_built_library(cwipc, container_cases, payload_cases):
    """The same packets through the library's exported host entries, unsanitised; no GPU is touched."""
    import cwipc_util_amd.codec as codec
    for name in NAMES:
        plain, coded = model_packets()[name], packed(name)
        assert bytes(codec.entropy_pack(plain)) == coded, name
        assert bytes(codec.entropy_unpack(coded)) == plain, name
        info = codec.entropy_info(coded)
        assert info["streams"] == em.directory(coded) and info["total_bytes"] == len(coded), name
        assert info["nleaves"] == cm.parse(plain)["nleaves"]
    for what, data in container_cases:
        for call in (codec.entropy_info, codec.entropy_unpack):
            with pytest.raises(cwipc.CwipcError) as err:
                call(data)
            assert len(str(err.value)) > 0, what
    for what, data in payload_cases:
        codec.entropy_info(data)
        with pytest.raises(cwipc.CwipcError) as err:
            codec.entropy_unpack(data)
        assert len(str(err.value)) > 0, what
    with pytest.raises(cwipc.CwipcError):
        codec.entropy_pack(packed("random 700"))
