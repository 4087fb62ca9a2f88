"""What the model alone must give for the streams of tests/inter_cases.py before the GPU is asked anything (CPU only): every lattice
frame's intra packet is the packet it was made from, every delta is im.diff of the two intra packets and im.apply gives the frame
back, and each case reaches the path it is there for -- its key / delta pattern, leaf counts, added counts, the workgroup counts past
one scan round, the point count past the bounds grid's cap, both stream modes of every stream kind, every padding residue of the keep
and the per-leaf streams, both values of R's last keep bit.  The groups:

  counts             nR, nP and the added count over 1, 7, 8, 9, 63 .. 65, 255 .. 257, 511 .. 513, each group one stream of 26 deltas
  two scan rounds    65 793 against 65 793 leaves with 65 537 added; 65 537 leaves with every third dropped; both with entropy too
  positions          P before R, P behind R, alternating cells, a run of 600 added keys, key 0 and the last key kept, added, dropped
  depth              bits 1 and 2 over shaped and drawn subsets, bits 11 to 16 sparse, bits 16 with 512 keys under one depth-13 node
  colour, tiles      colour bits 4 to 8 with residuals that wrap both ways; uniform and plane tiles in every order
  no decoder output  crowded leaves, non-finite points, 140 000 points, points on and a float32 step off the cube's faces"""
import numpy as np
import pytest

import codec_model as cm
import inter_model as im
from inter_cases import BIG, COUNTS, CROWDED, MID, MN, QUEUED, SIDE, TINY, WIDE, anchor, cases

NAMES = list(cases())


def deltas(name):
    """[(frame index, delta packet, its parsed form, R, P)] of a case's stream."""
    packets, intra, kinds = cases()[name].model()
    return [(i, packets[i], im.parse(packets[i]), intra[i - 1], intra[i]) for i in range(1, len(packets)) if kinds[i] == "d"]


def test_the_anchor_gives_the_cube():
    mn, side = im.expand_cube(*cm.cube(anchor()), 2.0)
    assert mn.tolist() == list(MN) and side == SIDE
    assert len(NAMES) == 35 and all(n in cases() for n in CROWDED + QUEUED + (BIG, TINY, MID))


@pytest.mark.parametrize("name", NAMES)
def test_model_over_the_stream(name):
    case = cases()[name]
    packets, intra, kinds = case.model()
    assert kinds == case.kinds and len(packets) == 1 + len(case.frames) and len(case.frames) == len(case.lattice) == len(case.pins)
    for i, X in enumerate(case.lattice):
        if X is not None:
            assert intra[i + 1] == X, i + 1
    indices = case.gop_indices()
    for i, D, info, R, P in deltas(name):
        assert D == im.diff(P, R, indices[i]), i
        assert im.apply(D, R) == P, i
        assert info["gop_index"] == indices[i] and info["ref_timestamp"] == cm.parse(R)["timestamp"]
    for i, k in enumerate(kinds):
        if k == "K":
            assert im.parse(packets[i])["entropy"] == case.entropy and im.Decoder().feed(packets[i]) == intra[i]
    assert case.boundaries()[0] and len(case.boundaries()) == len(packets) + 1


@pytest.mark.parametrize("name", NAMES)
def test_the_case_reaches_its_path(name):
    case = cases()[name]
    packets, intra, kinds = case.model()
    checked = 0
    for i, pins in enumerate(case.pins, start=1):
        P = cm.parse(intra[i])
        info = im.parse(packets[i]) if kinds[i] == "d" else None
        for what, want in pins.items():
            checked += 1
            if what == "nleaves":
                assert P["nleaves"] == want, i
            elif what == "points":
                assert len(case.frames[i - 1]) == want
            elif what == "nR":
                assert info["ref_nleaves"] == want, i
            elif what == "nadded":
                assert info["nadded"] == want, i
            elif what == "nodes_added":
                assert info["nodes_added"] == want, i
            elif what == "tile_mode":
                assert P["tile_mode"] == want and len(info["streams"]) == 1 + (case.octree_bits if info["nadded"] else 0) + 3 + want, i
            elif what == "last_kept":
                keep = info["streams"][0]
                assert keep["mode"] == 0 and bool(packets[i][keep["offset"] + (info["ref_nleaves"] - 1) // 8] >> ((info["ref_nleaves"] - 1) % 8) & 1) == want, i
            elif what == "last_depth":
                s = info["streams"][case.octree_bits]
                assert (s["kind"], s["which"], s["mode"]) == ("occupancy", case.octree_bits - 1, 0) and packets[i][s["offset"]:s["offset"] + s["used"]] == want
            elif what == "holds":
                keys = cm.leaf_keys_of(intra[i])
                assert (int(keys[0]) == 0, int(keys[-1]) == (1 << (3 * case.octree_bits)) - 1) == want, i
            elif what == "cells":
                axis = "xyz".index(name[5])
                q = cm.cells(case.frames[i - 1], np.asarray(MN, dtype=np.float32), SIDE, case.octree_bits)[:, axis]
                assert (q.min(), q.max()) == want and info is not None
            else:
                pytest.fail(what)
    assert checked >= len(case.pins)


def test_counts_cover_the_list():
    for name, what in (("counts: nR", "ref_nleaves"), ("counts: nP", "nleaves"), ("counts: added", "nadded")):
        seen = [info[what] for i, _, info, _, _ in deltas(name) if i % 2 == 0]
        assert seen == list(COUNTS), name
        assert all(k == "d" for k in cases()[name].model()[2][1:]) and len(cases()[name].frames) == 26
    kept = {(nr % 8 == 0, cases()["counts: nR"].pins[i - 1]["last_kept"]) for i, _, info, _, _ in deltas("counts: nR") if i % 2 == 0 for nr in [info["ref_nleaves"]]}
    assert kept == {(True, True), (True, False), (False, True), (False, False)}
    assert all(info["nleaves"] - info["nadded"] == 10 for i, _, info, _, _ in deltas("counts: added") if i % 2 == 0)
    sizes = {cm.parse(p)["nleaves"] for p in cases()["counts: nR"].model()[1]}
    assert len(sizes) > 20                                    # the reference's buffers change size from frame to frame


def test_two_scan_rounds():
    blocks = lambda n: (n + 255) // 256
    for tail in ("", ", entropy"):
        (_, _, first, _, _), (_, _, info, _, _) = deltas("two scan rounds: added" + tail)
        assert (info["ref_nleaves"], info["nleaves"], info["nadded"]) == (65793, 65793, 65537)
        assert blocks(info["nleaves"]) > 256 and blocks(info["nadded"]) > 256 and blocks(info["ref_nleaves"]) > 256
        assert blocks(first["nadded"]) > 256
        info = deltas("two scan rounds: dropped" + tail)[1][2]
        assert (info["ref_nleaves"], info["nleaves"], info["nadded"]) == (65537, 65537 - 21845, 0) and blocks(info["ref_nleaves"]) > 256
        assert im.parse(cases()["two scan rounds: added" + tail].model()[0][0])["entropy"] == bool(tail)
    assert cases()["two scan rounds: added"].colour_bits == 5 and cases()["two scan rounds: added"].octree_bits == 7


def test_the_wide_frames_pass_the_bounds_grids_cap():
    case = cases()["wide frame"]
    assert all(len(f) == WIDE for f in case.frames) and WIDE > 512 * 256
    f = case.frames
    assert np.isnan(f[1]['x'][-1]) and f[1]['y'][-1] == np.float32(1e9) and np.isfinite(f[1]['x'][:-1]).all()
    assert f[2]['x'][-1] == 3.5 and f[2]['x'][:-1].max() < 3.0 and case.kinds == "KddKdK"
    assert f[4]['x'][131071] == -4.0 and np.delete(f[4]['x'], 131071).min() > -1.0 and -4.0 < cm.parse(case.model()[1][3])["min"][0] < -3.0
    leaves = [cm.parse(p)["nleaves"] for p in case.model()[1]]
    assert min(leaves[1:3]) > 20000 and max(leaves) <= 32768 and min(leaves[3:]) > 500    # several points in most leaves, fifty and more in the keys' own cubes


def test_every_stream_mode_padding_residue_and_colour_depth_occurs():
    modes, keep_residue, leaf_residue, bits, cbs = set(), set(), set(), set(), set()
    for name in NAMES:
        case = cases()[name]
        for _, _, info, _, _ in deltas(name):
            modes |= {(s["kind"], s["mode"]) for s in info["streams"]}
            keep_residue.add((info["ref_nleaves"] + 7) // 8 % 4)
            leaf_residue.add(info["nleaves"] % 4)
            bits.add(info["octree_bits"])
            cbs.add(info["colour_bits"])
    assert modes == {(k, m) for k in ("keep", "occupancy", "colour", "tile") for m in (0, 1)}
    assert keep_residue == leaf_residue == {0, 1, 2, 3}
    assert bits >= {1, 2, 11, 12, 13, 14, 15, 16} and cbs == {4, 5, 6, 7, 8}


def test_non_finite_points_and_faces():
    case = cases()["non-finite points"]
    packets, intra, kinds = case.model()
    assert kinds == "KddddKKd" and cm.parse(intra[5])["nleaves"] == 0 and case.boundaries() == [True, False, False, False, False, False, True, False, False]
    for f, where in zip(case.frames[:3], ("first", "last", "scattered")):
        bad = ~(np.isfinite(f['x']) & np.isfinite(f['y']) & np.isfinite(f['z']))
        assert bad.sum() == 30 and {"first": bad[:30].all(), "last": bad[-30:].all(), "scattered": bad[0] and bad[-1] and not bad[1] and not bad[-2]}[where]
        worst = np.stack([f['x'], f['y'], f['z']], axis=1)[bad]
        assert np.isnan(worst).any() and np.isposinf(worst).any() and np.isneginf(worst).any() and (worst == np.float32(1e9)).any() and (worst == np.float32(-1e30)).any()
    assert not np.isfinite(case.frames[3]['x'][:600] + case.frames[3]['y'][:600] + case.frames[3]['z'][:600]).any() and len(case.frames[3]) == 650
    assert not np.isfinite(case.frames[4]['x'] + case.frames[4]['y'] + case.frames[4]['z']).any()
    for axis in "xyz":
        for second in ("past", "below"):
            case = cases()[f"face {axis}: {second}"]
            assert case.model()[2] == "KdKd"
            other = case.frames[1][axis]
            assert (other.max() == np.nextafter(np.float32(3.0), np.float32(4.0))) == (second == "past")
            assert (other.min() == np.nextafter(np.float32(-1.0), np.float32(-2.0))) == (second == "below")
