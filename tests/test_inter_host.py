"""RULE P's host code (csrc/inter_terms.hpp: the cube, the sequence, the container validator, pack and unpack of whole packets)
compiled as a stand-alone program (tests/abi/inter_host.cpp, its own main) with -fsanitize=address,undefined
-fno-sanitize-recover=all and held to the numpy model (tests/inter_model.py) as raw bytes.  The validator must refuse every damaged
container, and unpack every damaged payload that the validator lets through, with a message and with the sanitizers silent: the
predictor's search and the stream decoders are the functions the kernels call.  The same packets then go through the built
library's host entries in Python, unsanitised.  CPU only."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import codec_model as cm
import entropy_model as em
import inter_cases
import inter_model as im
from test_inter_model import container_cases, delta, hand_delta, hand_pair, pairs, payload_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(pairs())


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler: inter_terms.hpp cannot be checked"
    d = tmp_path_factory.mktemp("inter_host")
    exe = str(d / "inter_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "cwipc_util_amd", "csrc"), os.path.join(ROOT, "tests", "abi", "inter_host.cpp"), "-o", exe], check=True)

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


def gop_index(name):
    return im.parse(delta(name))["gop_index"]


def test_pack_and_unpack_equal_the_model(host):
    records = b"".join(struct.pack("<I", gop_index(n)) + framed(*pairs()[n]) for n in NAMES)
    for name, (ok, got) in zip(NAMES, results(host("pack", records), len(NAMES))):
        assert ok and got == delta(name), name
    records = b"".join(framed(pairs()[n][0], delta(n)) for n in NAMES)
    for name, (ok, got) in zip(NAMES, results(host("unpack", records), len(NAMES))):
        assert ok and got == pairs()[name][1], name


def test_pack_and_unpack_equal_the_model_on_chosen_leaf_sets(host):
    """Every delta of the streams of tests/inter_cases.py (leaf counts at the wave, the workgroup and the keep byte, 65 793 leaves,
    1 to 16 bits, key 0 and the last key, every colour depth): the pairs the kernels are held to in test_gpu_inter_edges.py."""
    pairs_, want = [], []
    for name, case in inter_cases.cases().items():
        packets, intra, kinds = case.model()
        indices = case.gop_indices()
        for i in range(1, len(packets)):
            if kinds[i] == "d":
                pairs_.append((indices[i], intra[i - 1], intra[i]))
                want.append((f"{name}, frame {i}", packets[i]))
    assert len(pairs_) > 250
    got = results(host("pack", b"".join(struct.pack("<I", g) + framed(R, P) for g, R, P in pairs_)), len(pairs_))
    for (what, D), (ok, packet) in zip(want, got):
        assert ok and packet == D, what
    got = results(host("unpack", b"".join(framed(R, D) for (_, R, _), (_, D) in zip(pairs_, want))), len(pairs_))
    for (what, _), (_, _, P), (ok, packet) in zip(want, pairs_, got):
        assert ok and packet == P, what


def test_hand_worked_delta(host):
    for case in (0, 1):
        R, P = hand_pair(case)
        (ok, got), = results(host("pack", struct.pack("<I", 2) + framed(R, P)), 1)
        assert ok and got == hand_delta(case)
        (ok, got), = results(host("unpack", framed(R, hand_delta(case))), 1)
        assert ok and got == P


def test_key_packets_and_wrong_inputs(host):
    R, P = pairs()["random"]
    empty = cm.encode(np.zeros(0, dtype=cm.POINT_DTYPE), 5, 85, 3)
    keys = [im.key_packet(R), im.key_packet(em.pack(R)), im.key_packet(empty)]
    for want, (ok, got) in zip((R, em.pack(R), empty), results(host("unpack", b"".join(framed(b"", k) for k in keys)), 3)):
        assert ok and got == want
    other = pairs()["nR 9"][0]
    bad = [(1, R, empty), (1, empty, P), (1, other, P), (0, R, P), (65535, R, P), (1, em.pack(R), P), (1, R, delta("random"))]
    got = results(host("pack", b"".join(struct.pack("<I", g) + framed(r, p) for g, r, p in bad)), len(bad))
    assert not any(ok for ok, _ in got) and all(message for _, message in got)
    bad = [im.key_packet(R[:-1]), im.prefix(im.KEY, 1) + R, im.key_packet(delta("random")), R, b"cwap", b""]
    got = results(host("unpack", b"".join(framed(R, d) for d in bad)), len(bad))
    assert not any(ok for ok, _ in got)


def test_validator_accepts_every_model_packet_and_refuses_every_damage(host):
    cases = container_cases()
    records = b"".join(framed(pairs()[n][0], delta(n)) for n in NAMES) + b"".join(framed(b"", delta(n)) for n in NAMES)
    records += b"".join(framed(R, data) for _, R, data in cases if R)
    got, at = host("validate", records), 0
    for name in NAMES + NAMES:
        assert got[at] == 1, name + " was refused: " + got[at + 2:at + 2 + got[at + 1]].decode()
        kind, nadded, S = struct.unpack("<III", got[at + 1:at + 13])
        entries = struct.unpack("<%dI" % (2 * S), got[at + 13:at + 13 + 8 * S])
        info = im.parse(delta(name))
        assert (kind, nadded) == (1, info["nadded"]) and list(zip(entries[0::2], entries[1::2])) == [(s["mode"], s["bytes"]) for s in info["streams"]], name
        at += 13 + 8 * S
    held = [what for what, R, _ in cases if R]
    for what in held:
        assert got[at] == 0, what
        assert got[at + 1] > 0, what + ": refused without a message"
        at += 2 + got[at + 1]
    # and unpack refuses them too, the one without a reference included
    data = b"".join(framed(R, d) for _, R, d in cases)
    assert not any(ok for ok, _ in results(host("unpack", data), len(cases)))


def test_damaged_payloads_pass_the_validator_and_are_refused_by_unpack(host):
    cases = payload_cases()
    got, at = host("validate", b"".join(framed(R, d) for _, R, d in cases)), 0
    for what, _, _ in cases:
        assert got[at] == 1, what
        at += 13 + 8 * struct.unpack("<I", got[at + 9:at + 13])[0]
    reasons = set()
    for (what, _, _), (ok, message) in zip(cases, results(host("unpack", b"".join(framed(R, d) for _, R, d in cases)), len(cases))):
        assert not ok, what
        reasons.add(message)
    assert reasons == {"entropy-coded block is not intact", "padding bits of the kept leaves are not 0", "kept and added leaves differ from the leaf count",
                       "an added leaf is a leaf of the reference"}


def test_random_bytes_as_payloads_stay_in_bounds(host):
    """The directory of a model packet kept, everything behind it random: whatever unpack answers, the sanitizers stay silent."""
    rng = np.random.default_rng(6)
    records = b""
    for name in ("random", "nleaves 4097", "cb 4, coded", "nR 32769"):
        R, _ = pairs()[name]
        D = delta(name)
        start = im.parse(D)["streams"][0]["offset"]
        for _ in range(6):
            records += framed(R, D[:start] + rng.integers(0, 256, len(D) - start).astype(np.uint8).tobytes())
    assert len(host("unpack", records)) > 24


def test_cube_and_sequence_equal_the_model(host):
    rng = np.random.default_rng(8)
    records, wants = b"", []
    for i in range(300):
        mn = (rng.normal(size=3) * 10.0 ** rng.integers(-3, 4)).astype(np.float32)
        if i % 7 == 0:
            mn[i % 3] = -0.0
        side = float(np.float32(abs(rng.normal()) * 10.0 ** rng.integers(-3, 4)).astype(np.float64)) or 1.0
        f = np.float32([1.0, 1.25, 1.1, 2.0, 16.0, 1.0000001][i % 6])
        mn2, side2 = im.expand_cube(mn, side, f)
        # extremes at the edges of the grown cube, a float32 step inside or outside
        lo = mn2.copy()
        hi = (mn2.astype(np.float64) + side2).astype(np.float32)
        step = i % 4
        if step == 1:
            lo[i % 3] = np.nextafter(lo[i % 3], np.float32(-np.inf))
        if step == 2:
            hi[i % 3] = np.nextafter(hi[i % 3], np.float32(np.inf))
        if step == 3:
            hi[i % 3] = np.nextafter(hi[i % 3], np.float32(-np.inf))
        records += mn.tobytes() + struct.pack("<df", side, f) + lo.tobytes() + hi.tobytes()
        wants.append(mn2.tobytes() + struct.pack("<d", side2) + bytes([im.contained(lo, hi, mn2, side2)]))
    assert host("cube", records) == b"".join(wants)
    assert {w[-1] for w in wants} == {0, 1}
    for gop in (2, 3, 8):
        frames = rng.choice([2, 2, 2, 2, 0, 3, 1], 60)
        enc_g, have, want = 0, False, b""
        for f in frames:
            empty, inside = bool(f & 1), bool(f & 2)
            want += bytes([enc_g == 0 or not have])
            key = enc_g == 0 or not have or empty or not inside
            if key:
                enc_g = 0
            want += bytes([0 if key else 1]) + struct.pack("<I", enc_g)
            have = not empty
            enc_g = (enc_g + 1) % gop
        assert host("sequence", struct.pack("<I", gop) + bytes(frames.astype(np.uint8))) == want


def test_host_entries_of_the_built_library(cwipc):
    """The same packets through the library's exported host entries, unsanitised; no GPU is touched."""
    import cwipc_util_amd.codec as codec
    for name in NAMES:
        R, P = pairs()[name]
        D = delta(name)
        assert bytes(codec.inter_pack(R, P, gop_index(name))) == D, name
        assert bytes(codec.inter_unpack(R, D)) == P, name
        info, want = codec.inter_info(D), im.parse(D)
        assert info["kind"] == "delta" and info["streams"] == [(s["mode"], s["bytes"]) for s in want["streams"]] and info["total_bytes"] == len(D), name
        assert (info["nadded"], info["nodes_added"], info["nleaves"], info["ref_nleaves"]) == (want["nadded"], want["nodes_added"], want["nleaves"], want["ref_nleaves"])
        assert [k[0] for k in info["kinds"]] == [s["kind"] for s in want["streams"]], name
    R, P = pairs()["random"]
    for embedded in (R, em.pack(R)):
        K = im.key_packet(embedded)
        assert bytes(codec.inter_unpack(None, K)) == embedded and codec.inter_info(K)["kind"] == "key"
        assert codec.inter_info(K)["nleaves"] == cm.parse(R)["nleaves"] and codec.inter_info(K)["entropy"] == (embedded != R)
    for what, ref, data in container_cases():
        with pytest.raises(cwipc.CwipcError) as err:
            codec.inter_unpack(ref or None, data)
        assert len(str(err.value)) > 0, what
    for what, ref, data in payload_cases():
        codec.inter_info(data)
        with pytest.raises(cwipc.CwipcError) as err:
            codec.inter_unpack(ref, data)
        assert len(str(err.value)) > 0, what
    with pytest.raises(cwipc.CwipcError):
        codec.inter_pack(R, delta("random"), 1)
