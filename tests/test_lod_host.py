"""RULE L's host code (csrc/lod_terms.hpp: the packet function of "cwao" and "cwae" packets) compiled as a stand-alone program
(tests/abi/lod_host.cpp, its own main) with -fsanitize=address,undefined -fno-sanitize-recover=all and held to the numpy model
(tests/lod_model.py) as raw bytes.  Every damaged packet must be refused with a message and with the sanitizers silent; the trees of
tests/tree_cases.py (runs of chosen lengths and places, exact halves of the mean) are cut here as the model cuts them.  The same
packets then go through the built library's host entry in Python, unsanitised.  CPU only."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import codec_model as cm
import entropy_model as em
import inter_model as im
import lod_model as lm
import transform_model as tm
from test_codec_packet_host import damages as plain_damages

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler: lod_terms.hpp cannot be checked"
    d = tmp_path_factory.mktemp("lod_host")
    exe = str(d / "lod_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "cwipc_util_amd", "csrc"), os.path.join(ROOT, "tests", "abi", "lod_host.cpp"), "-o", exe], check=True)

    def run(records):
        """[(bits, packet)] -> [(True, cut) | (False, message)]"""
        inp, outp = str(d / "in.bin"), str(d / "out.bin")
        with open(inp, "wb") as f:
            f.write(b"".join(struct.pack("<II", bits & 0xffffffff, len(p)) + bytes(p) for bits, p in records))
        proc = subprocess.run([exe, "lod", inp, outp], capture_output=True, text=True, timeout=300)
        assert proc.returncode == 0 and not proc.stderr, proc.stderr      # a sanitizer report ends the program with a message
        with open(outp, "rb") as f:
            got = f.read()
        out, at = [], 0
        for _ in records:
            if got[at] == 1:
                n = struct.unpack("<I", got[at + 1:at + 5])[0]
                out.append((True, got[at + 5:at + 5 + n]))
                at += 5 + n
            else:
                out.append((False, got[at + 2:at + 2 + got[at + 1]].decode()))
                at += 2 + got[at + 1]
        assert at == len(got)
        return out

    return run


@pytest.fixture(scope="module")
def packets():
    """{name: "cwao" packet}: the hand-built packets, the structured cloud at 9 bits, an empty cloud."""
    out = dict(lm.hand_packets())
    out["structured, 9 bits"] = cm.encode(em.structured_cloud(60000), 9, 85, timestamp=4242)
    out["empty, 9 bits"] = cm.encode(np.zeros(0, dtype=cm.POINT_DTYPE), 9, 60, timestamp=99)
    return out


def wanted(packets):
    """[(name, t, packet, the model's cut)]"""
    out = []
    for name, p in packets.items():
        for t in lm.targets(cm.parse(p)["octree_bits"]):
            out.append((name, t, p, lm.lod(p, t)))
    return out


def test_cuts_equal_the_model(host, packets):
    want = wanted(packets)
    for (name, t, _, cut), (ok, got) in zip(want, host([(t, p) for _, t, p, _ in want])):
        assert ok and got == cut, (name, t, got if not ok else "bytes differ")


def test_cuts_of_entropy_coded_packets_equal_the_model(host, packets):
    want = wanted(packets)
    for (name, t, _, cut), (ok, got) in zip(want, host([(t, em.pack(p)) for _, t, p, _ in want])):
        assert ok and got == em.pack(cut), (name, t, got if not ok else "bytes differ")


def test_targets_outside_the_packet_are_refused(host, packets):
    records = []
    for p in packets.values():
        b = cm.parse(p)["octree_bits"]
        records += [(0, p), (-1, p), (b + 1, p), (17, p), (0, em.pack(p)), (b + 1, em.pack(p))]
    for ok, message in host(records):
        assert not ok and "octree bits of the cut" in message


def test_other_forms_are_refused_with_the_function_to_compose_with(host, packets):
    p = packets["cb 8, 4099 leaves"]
    key = im.key_packet(p)
    assert im.parse(key)["kind"] == im.KEY
    (ok1, m1), (ok2, m2) = host([(2, tm.pack(p, 80)), (2, key)])
    assert not ok1 and "cwipc_hip_codec_transform_unpack" in m1
    assert not ok2 and "cwipc_hip_codec_inter_unpack" in m2


@pytest.fixture(scope="module")
def damaged(packets):
    names = ["single leaf", "cb 5, 77 leaves", "plane goes away", "tile mode 0", "cb 8, 4099 leaves", "empty, 9 bits"]
    bad = [(name + ": " + what, data) for name in names for what, data in plain_damages(packets[name])]
    for what, data in bad:
        with pytest.raises(cm.Invalid):
            cm.parse(data)
    coded = [(name + " (cwae): " + what, data) for name in names for what, data in em.damages(em.pack(packets[name]))]
    for what, data in coded:
        with pytest.raises(em.Invalid):
            em.parse(data)
    return bad + coded


def test_damaged_packets_are_refused_with_a_message(host, damaged):
    assert len(damaged) > 300
    for (what, _), (ok, message) in zip(damaged, host([(1, data) for _, data in damaged])):
        assert not ok and len(message) > 0, what


def test_host_entry_of_the_built_library(cwipc, packets, damaged):
    """The same packets through the library's exported host entry, unsanitised; no GPU is touched."""
    import cwipc_util_amd.codec as codec
    for name, t, p, cut in wanted(packets):
        assert bytes(codec.lod(p, t)) == cut, (name, t)
        assert bytes(codec.lod(em.pack(p), t)) == em.pack(cut), (name, t)
    p = packets["plane stays"]
    for bad_bits in (0, -1, 5, 17):
        with pytest.raises(cwipc.CwipcError, match="octree bits of the cut"):
            codec.lod(p, bad_bits)
    with pytest.raises(cwipc.CwipcError, match="cwipc_hip_codec_transform_unpack"):
        codec.lod(tm.pack(packets["cb 8, 4099 leaves"], 80), 2)
    for what, data in damaged:
        with pytest.raises(cwipc.CwipcError) as err:
            codec.lod(data, 1)
        assert len(str(err.value)) > 0, what


# ---------------------------------------------------------------------------
# the trees of tests/tree_cases.py: runs of chosen lengths and places, exact halves, every colour width
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tree_cuts():
    """[(name, t, P, em.pack(P), the model's cut)] of every cut of the table that lies inside its packet."""
    import tree_cases
    coded = {}
    out = []
    for name, t in tree_cases.lod_runs():
        case = tree_cases.cases()[name]
        if t <= case.octree_bits:
            if name not in coded:
                coded[name] = em.pack(case.packet)
            out.append((name, t, case.packet, coded[name], lm.lod(case.packet, t)))
    return out


def test_every_tree_case_is_cut_as_the_model_cuts_it(host, tree_cuts):
    assert len(tree_cuts) > 60
    for (name, t, _, _, cut), (ok, got) in zip(tree_cuts, host([(t, P) for _, t, P, _, _ in tree_cuts])):
        assert ok and got == cut, (name, t, got if not ok else "bytes differ")
    for (name, t, _, _, cut), (ok, got) in zip(tree_cuts, host([(t, E) for _, t, _, E, _ in tree_cuts])):
        assert ok and got == em.pack(cut), (name, t, got if not ok else "bytes differ")


def test_host_entry_of_the_built_library_on_the_tree_cases(cwipc, tree_cuts):
    import cwipc_util_amd.codec as codec
    for name, t, P, E, cut in tree_cuts:
        assert bytes(codec.lod(P, t)) == cut, (name, t)
        assert bytes(codec.lod(E, t)) == em.pack(cut), (name, t)
