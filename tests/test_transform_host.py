"""RULE T's host code (csrc/transform_terms.hpp: the arithmetic the kernels call, the container validator, pack and unpack of whole
packets) compiled as a stand-alone program (tests/abi/transform_host.cpp, its own main) with -fsanitize=address,undefined
-fno-sanitize-recover=all and held to the numpy model (tests/transform_model.py) as raw bytes.  The validator must refuse every
single-field damage of three packets, and unpack every payload damage that the validator lets through, with a message or a result
and with the sanitizers silent.  The trees of tests/tree_cases.py (chosen leaf keys; hostile but valid packets) are packed and
unpacked here before any kernel sees them.  The same packets then go through the built library's host entries in Python, unsanitised.  CPU only."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import transform_model as tm
from test_transform_model import (QUALITIES, damage_packets, damages, escape_count_off_by_one, hand_packets, model_answer, payload_damages, random_packets,
                                  smooth_packet)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler: transform_terms.hpp cannot be checked"
    d = tmp_path_factory.mktemp("transform_host")
    exe = str(d / "transform_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "cwipc_util_amd", "csrc"), os.path.join(ROOT, "tests", "abi", "transform_host.cpp"), "-o", exe], check=True)

    def run(mode, data):
        inp, out = str(d / "in.bin"), str(d / "out.bin")
        with open(inp, "wb") as f:
            f.write(data)
        proc = subprocess.run([exe, mode, inp, out], capture_output=True, text=True, timeout=300)
        assert proc.returncode == 0 and not proc.stderr, proc.stderr      # a sanitizer report ends the program with a message
        with open(out, "rb") as f:
            return f.read()

    return run


def framed(*packets):
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


_cases = []


def cases():
    """[(name, cwao packet, quality)]: the hand-worked packets at every quality, the 20 random ones at one each and at 100, the smooth one."""
    if not _cases:
        for name, P in hand_packets().items():
            _cases.extend((name, P, q) for q in QUALITIES)
        for i, (name, P) in enumerate(random_packets().items()):
            _cases.append((name, P, 100))
            _cases.append((name, P, QUALITIES[1 + i % 4]))
        _cases.extend(("smooth", smooth_packet(), q) for q in QUALITIES)
    return _cases


_models = {}


def model(name, P, q):
    if (name, q) not in _models:
        _models[(name, q)] = tm.pack(P, q)
    return _models[(name, q)]


def test_pack_and_unpack_equal_the_model(host):
    records = b"".join(struct.pack("<I", q) + framed(P) for _, P, q in cases())
    packed = results(host("pack", records), len(cases()))
    for (name, P, q), (ok, got) in zip(cases(), packed):
        assert ok and got == model(name, P, q), (name, q)
    unpacked = results(host("unpack", framed(*[model(*c) for c in cases()])), len(cases()))
    for (name, P, q), (ok, got) in zip(cases(), unpacked):
        assert ok and got == tm.unpack(model(name, P, q)), (name, q)
        if q == 100:
            assert got == P, name


def test_pack_refuses_what_is_no_eight_bit_packet(host):
    import codec_model as cm
    import entropy_model as em
    low = cm.encode(em.structured_cloud(500, seed=2), 6, 60, 5)          # 6 colour bits
    good = hand_packets()["two siblings"]
    records = struct.pack("<I", 50) + framed(low) + struct.pack("<I", 101) + framed(good) + struct.pack("<I", 50) + framed(good[:-1])
    got = results(host("pack", records), 3)
    assert [ok for ok, _ in got] == [False] * 3 and "8 colour bits" in got[0][1] and "jpeg_quality" in got[1][1]


def test_the_terms_equal_the_rule(host):
    import math
    records, want = b"", []
    for k in [1, 2, 3, 255, 256, 65535, 65536, (1 << 31) - 1, 1 << 31, 3037000499]:
        for v in (k * k - 1, k * k, k * k + 1):
            records += struct.pack("<BQqQ", 0, v, 0, 0)
            want.append(math.isqrt(v))
    for v in (0, (1 << 63) - 1, (1 << 64) - 1):
        records += struct.pack("<BQqQ", 0, v, 0, 0)
        want.append(math.isqrt(v))
    for n in (-9, -8, -7, -4, -3, -2, -1, 0, 1, 7, 8, -(1 << 62), (1 << 62) + 1):
        for d in (1, 2, 8, (1 << 32)):
            records += struct.pack("<BQqQ", 1, 0, n, d)
            want.append((n // d) & ((1 << 64) - 1))
    for q in range(101):
        records += struct.pack("<BQqQ", 2, 0, q, 0)
        want.append(tm.q16_of(q))
    rng = np.random.default_rng(11)
    for q16 in (16, 32, 52, 136, 272, 1024):
        for w1, w2 in [(1, 1), (1, 7), (7, 1), (1 << 31, 1 << 31), (1, (1 << 32) - 1)] + [tuple(int(v) for v in rng.integers(1, 1 << 24, 2)) for _ in range(40)]:
            records += struct.pack("<BQqQ", 3, q16, w1, w2)
            want.append(tm.step_of(q16, w1, w2))
    got = host("terms", records)
    assert list(struct.unpack("<%dQ" % len(want), got)) == want


@pytest.mark.parametrize("name", list(damage_packets()))
def test_the_validator_refuses_every_single_field_damage(host, name):
    T = damage_packets()[name]
    cases_ = damages(T)
    got = host("validate", framed(T, *[data for _, data in cases_]))
    assert got[0] == 1                                     # the packet itself passes, and its fields are the model's
    info = tm.parse(T)
    n = len(info["streams"])
    fields = struct.unpack("<I3i3II%dI" % (2 * n), got[1:1 + 4 * (8 + 2 * n)])
    assert fields[0] == info["q16"] and list(fields[1:4]) == info["dc"] and list(fields[4:7]) == info["nescapes"] and fields[7] == n
    assert list(fields[8:]) == [v for s in info["streams"] for v in (s["mode"], s["bytes"])]
    at = 1 + 4 * (8 + 2 * n)
    for what, _ in cases_:
        assert got[at] == 0, what
        assert got[at + 1] > 0
        at += 2 + got[at + 1]
    assert at == len(got)


@pytest.mark.parametrize("name", list(damage_packets()))
def test_unpack_answers_every_payload_damage_in_bounds(host, name):
    cases_ = payload_damages(damage_packets()[name])
    got = results(host("unpack", framed(*[data for _, data in cases_])), len(cases_))
    for (what, data), (ok, answer) in zip(cases_, got):
        kind, want = model_answer(data)
        assert ok == (kind == "packet"), (what, answer, want)
        if ok:
            assert answer == want, what
        else:
            assert answer, what


def test_escape_count_off_by_one(host):
    good, more = escape_count_off_by_one()
    (ok_good, _), (ok_more, reason) = results(host("unpack", framed(good, more)), 2)
    assert ok_good and not ok_more and "escape count" in reason


# ---------------------------------------------------------------------------
# the built library's host entries (no GPU is touched)
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def codec():
    import cwipc_util_amd.codec as codec
    return codec


def test_library_entries_equal_the_model(codec):
    for name, P, q in cases():
        T = bytes(codec.transform_pack(P, q))
        assert T == model(name, P, q), (name, q)
        assert bytes(codec.transform_unpack(T)) == tm.unpack(T), (name, q)
        info, want = codec.transform_info(T), tm.parse(T)
        assert (info["q16"], info["dc"], info["nescapes"]) == (want["q16"], want["dc"], want["nescapes"])
        assert info["streams"] == [(s["mode"], s["bytes"]) for s in want["streams"]]
        assert info["kinds"] == [(s["kind"], s["which"], s["symbols"]) for s in want["streams"]]
        assert info["total_bytes"] == len(T) and info["colour_bytes"] == tm.colour_payload_bytes(T) and info["colour_bits"] == 8


def test_library_entries_refuse_the_damages(codec):
    from cwipc_util_amd.util import CwipcError
    for name, T in damage_packets().items():
        for what, data in damages(T):
            with pytest.raises(CwipcError, match="cwipc_hip_codec_transform_info"):
                codec.transform_info(data)
            with pytest.raises(CwipcError):
                codec.transform_unpack(data)
        for what, data in payload_damages(T):
            codec.transform_info(data)
            kind, want = model_answer(data)
            if kind == "packet":
                assert bytes(codec.transform_unpack(data)) == want, (name, what)
            else:
                with pytest.raises(CwipcError, match="cwipc_hip_codec_transform_unpack"):
                    codec.transform_unpack(data)


# ---------------------------------------------------------------------------
# the trees of tests/tree_cases.py: chosen leaf keys, and the hostile packets before any kernel sees them
# ---------------------------------------------------------------------------
def tree_models():
    """[(name, quality, P, tm.pack(P, quality))] of every transform run of the table, made once."""
    import tree_cases
    if not _tree_models:
        _tree_models.extend((name, q, tree_cases.cases()[name].packet, tm.pack(tree_cases.cases()[name].packet, q)) for name, q in tree_cases.transform_runs())
    return _tree_models


_tree_models = []


def test_every_tree_case_packs_and_unpacks_as_the_model(host):
    runs = tree_models()
    packed = results(host("pack", b"".join(struct.pack("<I", q) + framed(P) for _, q, P, _ in runs)), len(runs))
    for (name, q, _, T), (ok, got) in zip(runs, packed):
        assert ok and got == T, (name, q)
    unpacked = results(host("unpack", framed(*[T for _, _, _, T in runs])), len(runs))
    for (name, q, P, T), (ok, got) in zip(runs, unpacked):
        assert ok and got == tm.unpack(T), (name, q)
        if q == 100:
            assert got == P, name


def test_hostile_packets_are_answered_in_bounds(host):
    import tree_cases
    packets = tree_cases.hostile()
    got = results(host("unpack", framed(*packets.values())), len(packets))
    for (name, T), (ok, answer) in zip(packets.items(), got):
        assert ok and answer == tm.unpack(T), name
    assert host("validate", framed(*packets.values()))[0] == 1


def test_library_entries_equal_the_model_on_the_tree_cases(codec):
    import tree_cases
    for name, q, P, T in tree_models():
        assert bytes(codec.transform_pack(P, q)) == T, (name, q)
        assert bytes(codec.transform_unpack(T)) == tm.unpack(T), (name, q)
    for name, T in tree_cases.hostile().items():
        assert bytes(codec.transform_unpack(T)) == tm.unpack(T), name
        assert codec.transform_info(T)["nescapes"] == [tm.parse(T)["nleaves"] - 1] * 3
