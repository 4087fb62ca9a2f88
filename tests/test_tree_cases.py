"""The cases of tests/tree_cases.py against the numpy models alone (RULE T: transform_model, RULE L: lod_model).  CPU only.

Three things.  Every case's cloud encodes to the case's packet (the GPU tests feed the cloud to the encoder and expect the model's
bytes of that packet).  Every case reaches the path it is named for: its pins are worked out again here from tm.parse,
tm.coefficients, the model's weights and the keys.  And the smallest cases are held to values worked by hand: the exact-half means
of RULE L and the butterfly of weights 1 and 2 of RULE T.

The groups: leaf, coefficient and inner-node counts at the workgroup, the escape block and the coded-stream threshold; scans past one
round of 256 block counts (the first-child scan and the escape scan, each alone and both); depth widths of 255, 256 and 257 nodes
(the shared launch against launches of their own), trees of 1, 2, 3 and 16 bits; butterflies of large equal, very unequal and 1-and-2
weights; the largest coefficients, the token/escape border, extreme dc, channels and whole blocks of escapes; every quality's branch;
tiles uniform and mixed; hostile but valid packets; runs of chosen lengths at chosen lanes, runs of one, one run of 70 000; exact
halves of the mean; a tile bit that one leaf carries; every colour width with the last leaf across two colour words."""
import numpy as np
import pytest

import codec_model as cm
import entropy_model as em
import lod_model as lm
import transform_model as tm
from tree_cases import (BIG, BIG_RUN, BORDER, COUNTS, LANES, RUN_STARTS, SMALL, TIMESTAMP, WAVE, cases, hostile, lod_runs, run_lengths, transform_runs)

NAMES = list(cases())

_packed = {}


def packed(name, q):
    if (name, q) not in _packed:
        _packed[(name, q)] = tm.pack(cases()[name].packet, q)
    return _packed[(name, q)]


@pytest.mark.parametrize("name", NAMES)
def test_the_cloud_encodes_to_the_packet(name):
    case = cases()[name]
    assert cm.encode(case.cloud, case.octree_bits, case.quality, TIMESTAMP) == case.packet
    assert len(case.cloud) == len(case.keys) and (case.qualities or case.cuts)
    assert case.colour_bits == 8 or not case.qualities


# ---------------------------------------------------------------------------
# the pins
# ---------------------------------------------------------------------------
def blocks(n):
    return (n + LANES - 1) // LANES


def zz_of(name, q):
    return tm.coefficients(cases()[name].packet, q)[0]


def butterflies_of(case):
    """Every (w1, w2) of the tree's butterflies."""
    info = cm.parse(case.packet)
    out = set()
    for w in tm._weights(tm.levels_of(case.packet, info), info["nleaves"]):
        w1, w2 = tm._places(w)
        has = (w1 > 0) & (w2 > 0)
        out |= set(zip(w1[has].tolist(), w2[has].tolist()))
    return out


def check(name, case, pin, want):
    info = cm.parse(case.packet)
    n, b, nodes = info["nleaves"], info["octree_bits"], info["nodes"]
    inner = 1 + sum(nodes[:-1])
    if pin == "nleaves":
        assert n == want
    elif pin == "ncoef":
        assert n - 1 == want
    elif pin == "inner":
        assert inner == want
    elif pin == "first_blocks":
        assert blocks(inner) == want
    elif pin == "first_rounds":
        assert blocks(blocks(inner)) == want
    elif pin == "escape_rounds":
        assert blocks(blocks(n - 1)) == want
    elif pin == "just_past_inner":
        assert want < inner <= want + 16 and n - 1 <= 65536           # a leaf adds 15 inner nodes at the most
    elif pin == "coded_tokens":
        streams = tm.parse(packed(name, 100))["streams"]
        tokens = [s for s in streams if s["kind"] == "token"]
        assert all(s["nblocks"] > 1 for s in tokens) and {s["mode"] for s in tokens} == {0, 1}          # several blocks; raw and coded
    elif pin == "widths_from_3":
        assert nodes[3:] == want and nodes[2] < want[0]
    elif pin == "widths":
        assert nodes == want
    elif pin == "own_launches":                                       # the depths whose parents do not fit one workgroup
        assert sum(1 for L in range(1, b) if nodes[L - 1] > LANES) == want
    elif pin == "butterflies":
        assert set(want) <= butterflies_of(case)
    elif pin == "nescapes":
        for q, e in want.items():
            assert tm.parse(packed(name, q))["nescapes"] == e
    elif pin == "max_zz":
        for q, top in want.items():
            assert int(zz_of(name, q).max()) == top
    elif pin == "dc":
        for q, dc in want.items():
            assert tm.parse(packed(name, q))["dc"] == dc
    elif pin == "exact":
        assert tm.unpack(packed(name, 100)) == case.packet
    elif pin == "escape_blocks":                                      # the escapes of Y in each block of 256 coefficients
        for q, per_block in want.items():
            is_escape = zz_of(name, q)[:, 0] >= 255
            assert [int(is_escape[k:k + LANES].sum()) for k in range(0, len(is_escape), LANES)] == per_block
    elif pin == "zz_has":
        for q, values in want.items():
            assert set(values) <= set(zz_of(name, q)[:, 0].tolist())
    elif pin == "tile_mode":
        assert info["tile_mode"] == want
        for q in case.qualities:
            assert ("tile" in [s["kind"] for s in tm.parse(packed(name, q))["streams"]]) == bool(want)
    elif pin == "placed":                                             # every length at every place
        t, lengths = want
        starts, got = run_lengths(case.keys, b, t)
        have = set(zip(got.tolist(), (starts % LANES).tolist()))
        assert {(n_, s) for n_ in lengths for s in RUN_STARTS} <= have
        # and so: runs that start at a wave's first lane, end at its last, lie in one wave, cross waves, cross workgroups
        ends = (starts + got - 1)
        assert ((starts % WAVE == 0) & (ends % WAVE == WAVE - 1) & (got == WAVE)).any() and ((got == 1) & (starts % LANES == 0)).any()
        assert ((got == 65) & (starts // WAVE + 1 == ends // WAVE)).any() and ((got == 257) & (starts // LANES + 1 == ends // LANES)).any()
    elif pin == "run_set":
        t, lengths = want
        assert sorted(set(run_lengths(case.keys, b, t)[1].tolist())) == lengths
    elif pin == "run_list":
        t, lengths = want
        assert run_lengths(case.keys, b, t)[1].tolist() == lengths
    elif pin == "last_leaf_straddles":
        bit = 3 * case.colour_bits * (n - 1)
        assert bit // 32 + 1 == (3 * case.colour_bits * n - 1) // 32 == (info["colour_bytes"] + 3) // 4 - 1
    elif pin == "halves":
        starts, got = run_lengths(case.keys, b, case.cuts[0])
        kinds = set()
        for a, c in zip(starts.tolist(), got.tolist()):
            for ch in range(3):
                total = int(case.stored[a:a + c, ch].sum())
                kinds.add(("even" if c % 2 == 0 else "odd", "half" if 2 * (total % c) == c else "below" if total % c == c // 2 - 1 and c > 2 else "other"))
        assert {("even", "half"), ("even", "below"), ("odd", "other")} <= kinds
        assert any(not case.stored[a:a + c].any() for a, c in zip(starts, got)) and any((case.stored[a:a + c] == 255).all() for a, c in zip(starts, got))
    elif pin == "tile_bits":
        t, tiles = want
        cut = cm.parse(lm.lod(case.packet, t))
        assert np.frombuffer(lm.lod(case.packet, t), dtype=np.uint8, count=cut["nleaves"], offset=cut["tile_offset"]).tolist() == tiles
        assert [int(v) for v in np.bincount(case.tiles, minlength=256)[[0x81, 0x41, 0x21]]] == [1, 1, 1]       # one leaf each
    else:
        pytest.fail("a pin that nothing checks: " + pin)


@pytest.mark.parametrize("name", NAMES)
def test_every_case_reaches_the_path_it_is_named_for(name):
    case = cases()[name]
    for pin, want in case.pins.items():
        check(name, case, pin, want)


def test_the_table_holds_every_group():
    """A case that leaves the table takes its path with it: the names the GPU files and the issue's list rely on."""
    names = set(NAMES)
    assert {f"counts: {n} leaves" for n in COUNTS} <= names and COUNTS == (1, 2, 3, 9, 256, 257, 258, 513, 4096, 4097)
    assert {"counts: 256 inner nodes", "counts: 257 inner nodes", BIG, BIG_RUN, "two scan rounds: coefficients alone", "two scan rounds: inner nodes alone"} <= names
    assert {f"depths: {m} chains" for m in (255, 256, 257)} <= names
    for group, least in (("depths", 9), ("weights", 3), ("values", 9), ("quality", 1), ("tiles", 2), ("runs", 11), ("means", 1), ("tile or", 1)):
        assert sum(1 for name in names if name.startswith(group + ":")) >= least, group
    assert cases()["quality: 5000 smooth leaves"].qualities == (0, 1, 49, 50, 99, 100)
    assert {cases()[name].colour_bits for name in names} == {4, 5, 7, 8}
    assert len(transform_runs()) > 60 and len(lod_runs()) > 60 and len(SMALL) > 40
    # stream modes, escapes present and absent, tile planes kept and dropped, over the whole table
    seen = set()
    for name, q in transform_runs():
        if cases()[name].keys.size > 10000 and name != BIG:
            continue
        info = tm.parse(packed(name, q))
        seen |= {(s["kind"], s["mode"]) for s in info["streams"]} | {("escapes", any(info["nescapes"]))}
    assert {("token", 0), ("token", 1), ("occupancy", 0), ("occupancy", 1), ("tile", 0), ("tile", 1), ("escape", 0), ("escapes", True), ("escapes", False)} <= seen
    # the cuts: 1, b - 1, b, b + 1 of some case, and 16 bits cut to 15 and to 1
    cuts = {(cases()[name].octree_bits, t) for name, t in lod_runs()}
    assert {(16, 15), (16, 1), (16, 16), (5, 6), (5, 5), (5, 4), (5, 1)} <= cuts


def test_every_quality_takes_its_branch():
    assert [tm.q16_of(q) for q in (0, 1, 49, 50, 99, 100)] == [1024, 1024, 138, 136, 18, 16]
    name = "quality: 5000 smooth leaves"
    sizes = [len(packed(name, q)) for q in (0, 1, 49, 50, 99, 100)]
    assert sizes[0] == sizes[1] < sizes[2] <= sizes[3] < sizes[4] < sizes[5]
    assert packed(name, 49) != packed(name, 50) and packed(name, 0)[:-1] == packed(name, 1)[:-1]
    assert tm.unpack(packed(name, 100)) == cases()[name].packet and tm.unpack(packed(name, 99)) != cases()[name].packet


# ---------------------------------------------------------------------------
# hostile packets
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(hostile()))
def test_hostile_packets_pass_the_container_test_and_unpack_to_clamped_colours(name):
    T = hostile()[name]
    info = tm.parse(T)
    n = info["nleaves"]
    assert info["q16"] == 1024 and info["nescapes"] == [n - 1] * 3 and abs(info["dc"][0]) == 255
    for s in info["streams"]:
        if s["kind"] == "token":
            assert T[s["offset"]:s["offset"] + s["symbols"]] == b"\xff" * (n - 1)
        if s["kind"] == "escape":
            assert T[s["offset"]:s["offset"] + 2 * s["symbols"]] == b"\xff" * (2 * n - 2)
    U = tm.unpack(T)
    got = cm.parse(U)
    colours = np.frombuffer(U, dtype=np.uint8, count=3 * n, offset=got["colour_offset"])
    assert set(colours.tolist()) <= {0, 255}
    cm.decode(U)


# ---------------------------------------------------------------------------
# worked by hand
# ---------------------------------------------------------------------------
def grey_zz(T):
    """Y's zigzag values of a packet with raw token streams and no escapes."""
    info = tm.parse(T)
    s = [s for s in info["streams"] if s["kind"] == "token" and s["which"] == 0][0]
    return list(T[s["offset"]:s["offset"] + s["symbols"]])


def test_the_butterfly_of_weights_one_and_two_by_hand():
    """Leaves 0 (grey 10), 8 and 9 (110, 150) and 63 (200) at 2 bits.  Node 1 of depth 1: the z butterfly of two leaves, d = 40,
    l = 110 + floor((40 + 1) / 2) = 130, weight 2.  The root: the z butterfly of its children 0 and 1, weights 1 and 2: d = 120,
    l = 10 + floor((2 * 120 + 1) / 3) = 90, weight 3; the x butterfly of that and child 7, weights 3 and 1: d = 110,
    l = 90 + floor((110 + 2) / 4) = 118.  Order: the root's x, the root's z, node 1's z.
    Quality 0, Q16 1024.  Steps: weights 3, 1: t = 1024^2 * 4 / 3 = 1398101, root 1182, (1182 + 8) >> 4 = 74; weights 1, 2:
    t = 1572864, root 1254, step 78; two leaves: 91.  c = (110 + 37) / 74 = 1, (120 + 39) / 78 = 2, (40 + 45) / 91 = 0.  (With the
    two-leaf step 91 in place of 78 the second would be (120 + 45) / 91 = 1.)
    Back: x: d = 74, a = 118 - floor((74 + 2) / 4) = 99, b = 173; z: d = 156, a = 99 - floor((2 * 156 + 1) / 3) = -5, b = 151;
    node 1: d = 0, both 151.  The colours are grey 0 (clamped), 151, 151, 173."""
    case = cases()["weights: 1 and 2"]
    assert case.keys.tolist() == [0, 8, 9, 63] and case.stored[:, 0].tolist() == [10, 110, 150, 200]
    assert (tm.step_of(1024, 3, 1), tm.step_of(1024, 1, 2), tm.step_of(1024, 1, 1)) == (74, 78, 91)
    exact, coarse = tm.pack(case.packet, 100), tm.pack(case.packet, 0)
    assert grey_zz(exact) == [220, 240, 80] and tm.parse(exact)["dc"] == [118, 0, 0] and tm.unpack(exact) == case.packet
    assert grey_zz(coarse) == [2, 4, 0] and tm.parse(coarse)["dc"] == [118, 0, 0]
    U = tm.unpack(coarse)
    assert np.frombuffer(U, dtype=np.uint8, count=12, offset=cm.parse(U)["colour_offset"]).reshape(4, 3).tolist() == [[0] * 3, [151] * 3, [151] * 3, [173] * 3]


def test_the_border_between_token_and_escape_by_hand():
    """Pairs of grey sibling leaves at quality 100: d = b - a, zigzag 2 d or -2 d - 1; 255 and above escape with zigzag - 255."""
    name = "values: zigzag 254, 255, 256"
    zz = zz_of(name, 100)[:, 0]
    assert zz[len(BORDER) - 1:].tolist() == [254, 255, 256, 253, 254, 255, 256, 254]
    T = packed(name, 100)
    info = tm.parse(T)
    assert info["nescapes"] == [4, 0, 0]
    token, escape = [s for s in info["streams"] if s["which"] == 0 and s["kind"] in ("token", "escape")]
    assert list(T[token["offset"]:token["offset"] + token["symbols"]])[len(BORDER) - 1:] == [254, 255, 255, 253, 254, 255, 255, 254]
    assert np.frombuffer(T, dtype="<u2", count=4, offset=escape["offset"]).tolist() == [0, 1, 0, 1]


def test_exact_half_means_by_hand():
    """Five leaves at 2 bits cut to 1: the run 0 .. 3 and the all-ones leaf.  Red 10, 10, 11, 11: 42 / 4 = 10.5, up to 11 ((42 + 2) / 4).
    Green 10, 10, 10, 11: 41 / 4 = 10.25: 10 ((41 + 2) / 4 = 10).  Blue 0, 0, 0, 255: 63.75: 64.  The tiles 1, 2, 4, 0x80 OR to 0x87."""
    zero = np.zeros(3, dtype=np.float32)
    P = cm.build_packet([0, 1, 2, 3, 63], [[10, 10, 0], [10, 10, 0], [11, 10, 0], [11, 11, 255], [7, 8, 9]], [1, 2, 4, 0x80, 1], zero, 1.0, 2, 8, 5)
    assert lm.lod(P, 1) == cm.build_packet([0, 7], [[11, 10, 64], [7, 8, 9]], [0x87, 1], zero, 1.0, 1, 8, 5)
    # two leaves: 10 and 11 give 11, 10 and 10 give 10, 254 and 255 give 255; three leaves 1, 1, 2: 4 / 3 -> (4 + 1) / 3 = 1
    P = cm.build_packet([0, 1, 8, 9, 10, 63], [[10, 10, 254], [11, 10, 255], [1, 0, 0], [1, 0, 0], [2, 1, 0], [0, 0, 0]], [1] * 6, zero, 1.0, 2, 8, 5)
    assert lm.lod(P, 1) == cm.build_packet([0, 1, 7], [[11, 10, 255], [1, 0, 0], [0, 0, 0]], [1] * 3, zero, 1.0, 1, 8, 5)
    # the case of the table: every run's mean is its base value, or one more where at least half of its leaves have one more
    case = cases()["means: halves"]
    cut = lm.lod(case.packet, 3)
    starts, got = run_lengths(case.keys, 6, 3)
    means = np.frombuffer(cut, dtype=np.uint8, count=3 * len(got), offset=cm.parse(cut)["colour_offset"]).reshape(-1, 3)
    for j, (a, c) in enumerate(zip(starts.tolist(), got.tolist())):
        low, more = case.stored[a:a + c].min(axis=0), (case.stored[a:a + c] != case.stored[a:a + c].min(axis=0)).sum(axis=0)
        assert means[j].tolist() == [int(low[ch]) + (1 if 2 * int(more[ch]) >= c else 0) for ch in range(3)], j


def test_cuts_of_the_entropy_and_transform_forms_stand_for_the_same_packet():
    case = cases()["runs: the full 16^3 block cut to waves"]
    assert em.unpack(em.pack(case.packet)) == case.packet == tm.unpack(tm.pack(case.packet, 100))
    cut = cm.parse(lm.lod(case.packet, 3))
    assert cut["nleaves"] == 65 and cut["octree_bits"] == 3
