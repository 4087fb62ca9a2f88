"""RULE P (include/cwipc_util_amd/hip_ext.h) through its numpy restatement (tests/inter_model.py): a delta worked out by hand,
apply(diff(P, R), R) == P over the shapes that take another path, the cube of a GOP at its float32 edges, the sequence rules as a
scripted state machine, and what a delta saves on clouds like a camera rig's.  CPU only; the host code and the kernels are held to
this model byte for byte in test_inter_host.py and test_gpu_inter.py, which take their cases from here."""
import functools
import struct

import numpy as np
import pytest

import codec_model as cm
import entropy_model as em
import inter_model as im


# ---------------------------------------------------------------------------
# material
# ---------------------------------------------------------------------------
def tree_packet(seed, keys, b, cb=8, tile="plane", timestamp=0, mn=(-1.0, 0.0, 0.5), side=2.5):
    """A cwao packet with the leaves `keys` and random stored colours.  tile: "plane" (random tiles 1, 2, 4) or a value for all leaves."""
    rng = np.random.default_rng(seed)
    keys = np.unique(np.asarray(keys, dtype=np.uint64))
    n = len(keys)
    stored = rng.integers(0, 1 << cb, (n, 3))
    if tile == "plane":
        tiles, mode = rng.choice(np.array([1, 2, 4], dtype=np.uint8), n), 1
    else:
        tiles, mode = np.full(n, tile, dtype=np.uint8), 0
    return cm.build_packet(keys, stored, tiles, np.asarray(mn, dtype=np.float32), side, b, cb, timestamp, tile_mode=mode)


def draw(seed, n, b):
    return np.random.default_rng(seed).choice(1 << (3 * b), n, replace=False).astype(np.uint64)


@functools.lru_cache(maxsize=None)
def pairs():
    """{name: (R, P)}: cwao packets in one cube."""
    out = {}
    a, c = draw(1, 300, 5), draw(2, 280, 5)
    both = np.concatenate([a[:150], c[:120]])
    out["random"] = (tree_packet(10, a, 5, timestamp=7), tree_packet(11, both, 5, timestamp=8))
    out["random, deep and sparse"] = (tree_packet(12, draw(3, 50, 10), 10), tree_packet(13, np.concatenate([draw(3, 50, 10)[:20], draw(4, 45, 10)]), 10))
    out["P == R"] = (tree_packet(14, a, 5, timestamp=1), tree_packet(14, a, 5, timestamp=2))
    out["P inside R"] = (tree_packet(15, a, 5), tree_packet(16, a[::3], 5))
    out["R inside P"] = (tree_packet(17, a[::3], 5), tree_packet(18, a, 5))
    out["disjoint"] = (tree_packet(19, a[a % 2 == 0], 5), tree_packet(20, a[a % 2 == 1], 5))
    out["one leaf each, the same"] = (tree_packet(21, [77], 3), tree_packet(22, [77], 3))
    out["one leaf each, P before R"] = (tree_packet(21, [77], 3), tree_packet(22, [5], 3))
    out["one leaf each, P behind R"] = (tree_packet(21, [77], 3), tree_packet(22, [500], 3))
    out["b = 1"] = (tree_packet(23, [0, 3, 7], 1), tree_packet(24, [1, 3, 6, 7], 1))
    for nr in (7, 8, 9):
        k = draw(30 + nr, 40, 4)
        out[f"nR {nr}"] = (tree_packet(31, k[:nr], 4), tree_packet(32, k[3:20], 4))
    k = draw(40, 36000, 6)
    out["nR 32769"] = (tree_packet(41, k[:32769], 6, tile=3), tree_packet(42, k[30000:36000], 6, tile=3))
    k = draw(50, 6000, 5)
    for n in (4095, 4096, 4097):
        out[f"nleaves {n}"] = (tree_packet(51, k[:5000], 5, cb=6), tree_packet(52, k[1000:1000 + n], 5, cb=6))
    for rt, pt in ((1, 1), (1, "plane"), ("plane", 2), ("plane", "plane")):
        out[f"tiles R {rt} P {pt}"] = (tree_packet(61, a, 5, tile=rt), tree_packet(62, both, 5, tile=pt))
    k = draw(70, 9000, 5)
    for cb in (4, 8):
        out[f"cb {cb}, coded"] = (tree_packet(71, k[:8000], 5, cb=cb), tree_packet(72, k[500:9000], 5, cb=cb))
    # the colours of the kept leaves unchanged: what a still scene gives
    R = tree_packet(81, k[:8000], 5, cb=7)
    out["still"] = (R, R[:8] + struct.pack("<Q", 99) + R[16:])
    return out


@functools.lru_cache(maxsize=None)
def delta(name):
    R, P = pairs()[name]
    return im.diff(P, R, 1 + len(name) % 5)


# ---------------------------------------------------------------------------
# a delta worked out by hand
# ---------------------------------------------------------------------------
HAND_R_KEYS, HAND_P_KEYS = [3, 10, 17, 40, 63], [3, 9, 12, 40, 41, 50]
HAND_R_COL = np.array([[10, 1, 200], [20, 2, 201], [30, 3, 202], [40, 4, 203], [50, 5, 204]])
HAND_P_COL = np.array([[10, 1, 0], [5, 1, 0], [25, 1, 0], [41, 1, 0], [40, 1, 0], [255, 1, 0]])
HAND_MN = np.array([0.0, 1.0, 2.0], dtype=np.float32)


def hand_pair(case):
    """case 0: R without a tile plane (tile 1), P with one; case 1: R with a plane, P without (tile 2)."""
    rt, pt = ([1] * 5, [1, 2, 1, 2, 1, 2]) if case == 0 else ([1, 2, 4, 8, 16], [2] * 6)
    R = cm.build_packet(HAND_R_KEYS, HAND_R_COL, rt, HAND_MN, 4.0, 2, 8, 1000)
    P = cm.build_packet(HAND_P_KEYS, HAND_P_COL, pt, HAND_MN, 4.0, 2, 8, 1033)
    return R, P


def hand_delta(case):
    """Keys 3 and 40 stay (R's leaves 0 and 3): keep = 0b01001.  A = 9, 12, 41, 50: the root has the children 1, 5, 6; node 1 the
    children 1 and 4, node 5 the child 1, node 6 the child 2.  Predictors: 3 -> 0; 9 -> 0 (R's 3 is the last key <= 9); 12 -> 1;
    40, 41, 50 -> 3."""
    R, P = hand_pair(case)
    S = 7 if case == 0 else 6
    out = b"cwap" + struct.pack("<IIIQII", 1, 1, 2, 1000, 5, 0) + P[8:48] + struct.pack("<I", 4) + struct.pack("<II", 3, 4)
    out += struct.pack("<I", S) + struct.pack("<II", 0, 4) * 3 + struct.pack("<II", 0, 8) * (S - 3)
    out += bytes([0x09, 0, 0, 0]) + bytes([0x62, 0, 0, 0]) + bytes([0x12, 0x02, 0x04, 0])
    out += bytes([0, 251, 5, 1, 0, 215, 0, 0])          # r: 10-10, 5-10, 25-20, 41-40, 40-40, 255-40
    out += bytes([0, 0, 255, 253, 253, 253, 0, 0])      # g: 1-1, 1-1, 1-2, 1-4 three times
    out += bytes([56, 56, 55, 53, 53, 53, 0, 0])        # b: 0-200, 0-200, 0-201, 0-203 three times
    if case == 0:
        out += bytes([0, 3, 0, 3, 0, 3, 0, 0])          # tile: P's 1, 2, 1, 2, 1, 2 against R's 1 throughout
    return out


@pytest.mark.parametrize("case", [0, 1])
def test_hand_worked_delta(case):
    R, P = hand_pair(case)
    assert cm.parse(P)["tile_mode"] == 1 - case and cm.parse(R)["tile_mode"] == case
    assert im.diff(P, R, 2) == hand_delta(case)
    assert im.apply(hand_delta(case), R) == P


# ---------------------------------------------------------------------------
# apply(diff(P, R), R) == P
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(pairs()))
def test_round_trip(name):
    R, P = pairs()[name]
    D = delta(name)
    info = im.parse(D, R)
    ri, pi = cm.parse(R), cm.parse(P)
    assert (info["kind"], info["ref_timestamp"], info["ref_nleaves"]) == (im.DELTA, ri["timestamp"], ri["nleaves"])
    assert D[im.PREFIX:im.PREFIX + 40] == P[8:48]
    assert len(info["streams"]) == 1 + (pi["octree_bits"] if info["nadded"] else 0) + 3 + pi["tile_mode"]
    assert im.apply(D, R) == P


def test_the_paths_the_cases_are_there_for():
    modes = lambda name: [s["mode"] for s in im.parse(delta(name))["streams"]]
    assert modes("nR 32769")[0] == 1                         # keep reaches 4096 bytes and is coded
    assert im.parse(delta("nR 32769"))["streams"][0]["symbols"] == 4097
    assert all(m == 0 for m in modes("nleaves 4095"))
    assert modes("nleaves 4096")[-1] == 1 and modes("nleaves 4097")[-1] == 1      # the tile stream: three values, coded from 4096 symbols on
    assert im.parse(delta("P == R"))["nadded"] == 0 and im.parse(delta("P inside R"))["nadded"] == 0
    assert im.parse(delta("disjoint"))["nadded"] == cm.parse(pairs()["disjoint"][1])["nleaves"]
    still = im.parse(delta("still"))
    assert [s["mode"] for s in still["streams"][-3:]] == [1, 1, 1] and all(s["bytes"] == 512 + 2 * 4 + 2 * 256 for s in still["streams"][-3:])


def test_key_packets():
    R, _ = pairs()["random"]
    for embedded in (R, em.pack(R), cm.encode(np.zeros(0, dtype=cm.POINT_DTYPE), 5, 85, 3)):
        K = im.key_packet(embedded)
        assert im.parse(K)["kind"] == im.KEY and im.apply(K, None) == embedded
    with pytest.raises(im.Invalid):
        im.parse(im.key_packet(R[:-1]))
    with pytest.raises(im.Invalid):
        im.parse(im.prefix(im.KEY, 1) + R)


@functools.lru_cache(maxsize=None)
def container_cases():
    """[(what, R, damaged D)]: the container test with R held must refuse each."""
    out = []
    for name in ("random", "P == R", "nR 9", "nleaves 4097", "tiles R plane P 2", "cb 4, coded", "nR 32769"):
        R, _ = pairs()[name]
        out += [(name + ": " + what, R, data) for what, data in im.damages(delta(name), R)]
    R, P = pairs()["random"]
    other = tree_packet(10, draw(1, 300, 5), 5, timestamp=7, side=2.0)
    out.append(("reference with another side", other, delta("random")))
    out.append(("reference with other bits", tree_packet(10, draw(1, 300, 5), 5, cb=7, timestamp=7), delta("random")))
    out.append(("reference is the frame itself", P, delta("random")))
    out.append(("no reference", b"", delta("random")))
    return out


@functools.lru_cache(maxsize=None)
def payload_cases():
    """[(what, R, damaged D)]: the container test accepts each, applying it must refuse each."""
    out = []
    for name in ("random", "nR 9", "nleaves 4097", "cb 4, coded", "nR 32769", "still"):
        R, P = pairs()[name]
        out += [(name + ": " + what, R, data) for what, data in im.payload_damages(delta(name), R)]
        if name != "still":
            out.append((name + ": an added leaf is a leaf of the reference", R, im.diff(P, R, 1, overlap=True)))
    return out


def test_damaged_containers_are_refused():
    cases = container_cases()
    assert len(cases) > 400
    for what, R, data in cases:
        with pytest.raises(im.Invalid):
            im.parse(data, R)
            pytest.fail(what)


def test_damaged_payloads_pass_the_container_test_and_are_refused():
    cases = payload_cases()
    assert len(cases) >= 25
    for what, R, data in cases:
        im.parse(data, R)
        with pytest.raises((im.Invalid, em.Invalid)):
            im.apply(data, R)
            pytest.fail(what)


# ---------------------------------------------------------------------------
# the cube
# ---------------------------------------------------------------------------
def test_exp_factor_1_gives_rule_c_cube():
    rng = np.random.default_rng(3)
    for pts in (cm.random_cloud(rng, 500, 3.0, (10.0, -4.0, 0.5)), cm.make_cloud([[1.5, -2.0, 3.0]]), cm.make_cloud([[-0.0, 0.0, 5.0], [1.0, 2.0, 6.0]])):
        mn, side = cm.cube(pts)
        mn2, side2 = im.expand_cube(mn, side, 1.0)
        assert mn2.tobytes() == mn.tobytes() and side2 == side
        assert im.encode_in_cube(pts, mn2, side2, 6, 85, 5) == cm.encode(pts, 6, 85, 5)
        assert im.contained(*im.extremes(pts), mn2, side2)
    assert cm.cube(cm.make_cloud([[1.5, -2.0, 3.0]]))[1] == 1.0


def test_cube_edges():
    mn, side = np.array([1.0, -3.0, 0.25], dtype=np.float32), 2.0
    mn2, side2 = im.expand_cube(mn, side, 1.25)
    assert side2 == 2.5 and mn2.tolist() == [0.75, -3.25, 0.0]
    inside = np.array([0.75, -3.25, 0.0], dtype=np.float32)
    top = (mn2.astype(np.float64) + side2).astype(np.float32)          # exact here: the last float32 inside
    assert im.contained(inside, top, mn2, side2)
    for a in range(3):
        lo = inside.copy()
        lo[a] = np.nextafter(lo[a], np.float32(-np.inf))
        assert not im.contained(lo, top, mn2, side2)
        hi = top.copy()
        hi[a] = np.nextafter(hi[a], np.float32(np.inf))
        assert not im.contained(inside, hi, mn2, side2)
    # a point at the top edge takes the clamp, as RULE C's own maximum does
    pts = cm.make_cloud([inside, top])
    q = cm.cells(pts, mn2, side2, 9)
    assert q.min() == 0 and q.max() == 511
    # a -0.0 minimum: the cube's origin is +0 whatever the margin
    assert np.signbit(im.expand_cube(np.array([-0.0, -0.0, -0.0], dtype=np.float32), 1.0, 1.0)[0]).sum() == 0
    z = im.expand_cube(np.array([0.125, 0.0, 0.0], dtype=np.float32), 1.0, 1.25)[0]
    assert z[0] == 0.0 and not np.signbit(z[0])
    # the margin is rounded as the rule says: float64 throughout, the origin to float32 last
    mn3, side3 = im.expand_cube(np.array([0.1, 0.2, 0.3], dtype=np.float32), 0.7, 1.1)
    grown = np.float64(0.7) * np.float64(np.float32(1.1))
    assert side3 == grown and mn3[0] == np.float32(np.float64(np.float32(0.1)) - (grown - np.float64(0.7)) * 0.5)
    assert not im.inter_on(True, 1, 1.25) and not im.inter_on(False, 8, 1.25) and not im.inter_on(True, 8, 0.99)
    assert not im.inter_on(True, 8, np.nan) and not im.inter_on(True, 65536, 1.0) and im.inter_on(True, 65535, 16.0) and im.inter_on(True, 2, 1.0)


# ---------------------------------------------------------------------------
# the sequence
# ---------------------------------------------------------------------------
def small_cloud(seed, n=400, shift=0.0):
    pts = cm.random_cloud(np.random.default_rng(seed), n, 1.0)
    pts['x'] += np.float32(shift)
    return pts


EMPTY = np.zeros(0, dtype=cm.POINT_DTYPE)


def script(gop, frames):
    """frames: "." a frame inside the cube, "e" an empty one, "o" one that leaves the cube -> the kinds, the gop indices, the
    boundary flags before each frame, the packets and the decoded packets."""
    enc, dec = im.Encoder(gop, 1.25, 6, 85), im.Decoder()
    kinds, index, boundary, packets = "", [], [], []
    for i, f in enumerate(frames):
        boundary.append(enc.at_gop_boundary())
        pts = EMPTY if f == "e" else small_cloud(i, shift=10.0 * frames[:i + 1].count("o") + 0.001 * i)   # (an "o" moves the scene for good)
        packet = enc.feed(pts, 100 + i)
        info = im.parse(packet)
        kinds += "K" if info["kind"] == im.KEY else "d"
        index.append(info["gop_index"])
        packets.append(packet)
        assert dec.feed(packet) == enc.intra
    return kinds, index, boundary, packets


def test_sequence_rules():
    assert script(2, "......")[:2] == ("KdKdKd", [0, 1, 0, 1, 0, 1])
    assert script(3, ".......")[:2] == ("KddKddK", [0, 1, 2, 0, 1, 2, 0])
    kinds, index, boundary, _ = script(8, "." * 10)
    assert kinds == "KdddddddKd" and index == [0, 1, 2, 3, 4, 5, 6, 7, 0, 1]
    assert boundary == [True] + [False] * 7 + [True, False]
    # an empty frame mid-GOP: a key that leaves no reference, so the next frame is a key too and starts the GOP anew
    kinds, index, boundary, _ = script(4, "..e...")
    assert kinds == "KdKKdd" and index == [0, 1, 0, 0, 1, 2]
    assert boundary == [True, False, False, True, False, False]
    # a frame that leaves the cube: a key forced inside the GOP sets g to 0 first
    kinds, index, boundary, _ = script(4, "..o....")
    assert kinds == "KdKdddK" and index == [0, 1, 0, 1, 2, 3, 0]
    assert boundary == [True, False, False, False, False, False, True]


def test_a_delta_chain_does_not_drift():
    enc, dec = im.Encoder(8, 1.25, 5, 60, entropy=True), im.Decoder()
    rng = np.random.default_rng(9)
    pts = small_cloud(1, 3000)
    for i in range(6):
        pts = pts.copy()
        move = rng.random(len(pts)) < 0.2
        pts['x'][move] += np.float32(0.01)
        pts['r'][move] = rng.integers(0, 256, int(move.sum()))
        packet = enc.feed(pts, i)
        assert dec.feed(packet) == enc.intra == im.encode_in_cube(pts, *enc.cube, 5, 60, i)
    assert enc.kinds == [im.KEY] + [im.DELTA] * 5


# ---------------------------------------------------------------------------
# what a delta saves
# ---------------------------------------------------------------------------
def test_size_conditions():
    pts = em.structured_cloud(40000, seed=4)
    enc = im.Encoder(8, 1.25, 7, 85)
    enc.feed(pts, 0)
    still = enc.feed(pts, 1)
    assert im.parse(still)["kind"] == im.DELTA
    ratio = len(still) / len(em.pack(enc.intra))
    print("static frame: delta / cwae =", ratio)
    assert ratio < 1 / 3
    moved = pts.copy()
    cap = moved['x'] > 0.8                                   # a tenth of a sphere's surface
    assert 0.08 < cap.mean() < 0.12
    moved['x'][cap] += np.float32(0.02)
    part = enc.feed(moved, 2)
    assert im.parse(part)["kind"] == im.DELTA
    ratio = len(part) / len(em.pack(enc.intra))
    print("a tenth displaced: delta / cwae =", ratio)
    assert len(part) < len(em.pack(enc.intra))
