"""Transform colour coding on the GPU (RULE T in include/cwipc_util_amd/hip_ext.h; csrc/kernels_transform.hip) against its numpy
restatement (tests/transform_model.py).  Bytes only: an encoder with colour_transform=True must deliver
transform_model.pack(codec_model.encode(cloud, bits, 100), quality), a decoder fed that packet the cloud it hands out for
transform_model.unpack of it.  The damaged packets are ones the sanitised host program has answered in bounds
(test_transform_host.py): the container test refuses them before anything is launched, the others are refused by the check inside feed."""
import gc
import struct

import numpy as np
import pytest

import codec_model as cm
import entropy_model as em
import transform_model as tm
from conftest import make_cloud
from test_transform_model import damage_packets, damages, escape_count_off_by_one

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def codec(gpu):
    import cwipc_util_amd.codec as codec
    return codec


@pytest.fixture(scope="module", autouse=True)
def clouds_before(gpu):
    gc.collect()
    return gpu.cwipc_dangling_allocations(False)


def lattice(n, bits, rng):
    """A cloud of exactly n leaves at `bits` bits, one point a leaf: k / (2^bits - 1) lies in cell k; the two corners pin the cube."""
    top = (1 << bits) - 1
    if n == 1:
        return np.array([[0.25, 0.5, 0.75]])
    cells = rng.choice((top + 1) ** 3 - 2, n - 2, replace=False) + 1
    q = np.stack([cells // ((top + 1) ** 2), (cells // (top + 1)) % (top + 1), cells % (top + 1)], axis=1)
    q = np.concatenate([[[0, 0, 0]], q, [[top, top, top]]])
    return q[rng.permutation(n)] / float(top)


def smooth_colours(xyz):
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    return np.clip(np.stack([128 + 100 * np.sin(5 * x) * np.cos(3 * y), 128 + 90 * np.sin(4 * y + 1), 128 + 80 * np.cos(6 * z)], axis=1), 0, 255).astype(np.uint8)


_clouds = {}


def clouds():
    """name -> (points, octree_bits, jpeg_quality): shared, read only."""
    if _clouds:
        return _clouds
    rng = np.random.default_rng(77)

    def add(name, xyz, bits, quality, colours="smooth", tiles="equal"):
        xyz = np.asarray(xyz, dtype=np.float64)
        rgb = smooth_colours(xyz) if colours == "smooth" else rng.integers(0, 256, (len(xyz), 3)) if colours == "random" else np.full((len(xyz), 3), (90, 160, 30))
        pts = cm.make_cloud(xyz, rgb)
        pts['tile'] = 5 if tiles == "equal" else rng.choice(np.array([1, 2, 4], dtype=np.uint8), len(xyz))
        pts.setflags(write=False)
        _clouds[name] = (pts, bits, quality)

    add("1 leaf", lattice(1, 9, rng), 9, 85)
    add("2 leaves at 1 bit", lattice(2, 1, rng), 1, 100, "random")
    add("9 leaves at 2 bits", lattice(9, 2, rng), 2, 50, "random", "mixed")
    add("4096 leaves: 4095 tokens", lattice(4096, 9, rng), 9, 100)
    add("4097 leaves: 4096 tokens", lattice(4097, 9, rng), 9, 85, "smooth", "mixed")
    add("4098 leaves, random colours", lattice(4098, 9, rng), 9, 100, "random")
    sphere = rng.normal(size=(20000, 3))
    sphere /= np.linalg.norm(sphere, axis=1, keepdims=True)
    for quality in (100, 85, 50, 24, 0):
        add(f"sphere at quality {quality}", sphere, 9, quality, "smooth", "mixed")
    add("sphere, random colours", sphere, 9, 100, "random")
    add("sphere, constant colour", sphere, 9, 50, "constant", "mixed")
    add("random points at 16 bits", rng.uniform(-1, 1, (3000, 3)), 16, 24, "random", "mixed")
    many = em.structured_cloud(60000)
    add("many points a leaf", np.stack([many['x'], many['y'], many['z']], axis=1), 7, 85, "smooth", "mixed")
    add("empty", np.zeros((0, 3)), 9, 60)
    return _clouds


_pairs = {}


def pair(name):
    """(the cwao packet with 8 colour bits, its transform-coded form at the cloud's quality), both from the models."""
    if name not in _pairs:
        pts, bits, quality = clouds()[name]
        plain = cm.encode(pts, bits, 100, 1234)
        _pairs[name] = (plain, tm.pack(plain, quality))
    return _pairs[name]


def encode(codec, cwipc, pts, bits, quality, timestamp=1234, **kw):
    enc = codec.cwipc_new_encoder(octree_bits=bits, jpeg_quality=quality, **kw)
    enc.feed(make_cloud(cwipc, pts, 0.0, timestamp))
    assert enc.available(True)
    data = bytes(enc.get_bytes())
    assert not enc.available(False)
    enc.free()
    return data


def decode(codec, packet):
    dec = codec.cwipc_new_decoder()
    dec.feed(packet)
    assert dec.available(True)
    pc = dec.get()
    assert pc is not None and not dec.available(False)
    dec.free()
    return pc


# ---------------------------------------------------------------------------
# encoder and decoder against the model
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(clouds()))
def test_encoder_delivers_the_model_packet(codec, gpu, name):
    pts, bits, quality = clouds()[name]
    plain, coded = pair(name)
    got = encode(codec, gpu, pts, bits, quality, colour_transform=True)
    assert got[:4] == b"cwat" and len(got) == len(coded)
    assert got == coded
    assert encode(codec, gpu, pts, bits, quality) == cm.encode(pts, bits, quality, 1234)        # off, the default: today's bytes


@pytest.mark.parametrize("name", list(clouds()))
def test_decoder_hands_out_the_unpacked_packets_cloud(codec, gpu, name):
    plain, coded = pair(name)
    unpacked = tm.unpack(coded)
    want, ts, cell = cm.decode(unpacked)
    got = decode(codec, coded)
    assert got.count() == len(want) and got.timestamp() == ts
    assert np.float32(got.cellsize()).tobytes() == np.float32(cell).tobytes()
    assert got.get_numpy_array().tobytes() == want.tobytes()
    if clouds()[name][2] == 100:
        assert unpacked == plain
        assert got.get_numpy_array().tobytes() == decode(codec, plain).get_numpy_array().tobytes()


def test_the_inputs_reach_every_path():
    """Raw and coded token streams, escapes present and absent, a token stream of 4095, 4096 and of several blocks, all tokens 0, packets
    with and without a tile plane, depths run in the shared launch and depths with a launch of their own."""
    seen = set()
    for name in clouds():
        if name == "empty":
            continue
        info = tm.parse(pair(name)[1])
        for s in info["streams"]:
            seen.add((s["kind"], s["mode"]))
            if s["kind"] == "token":
                seen.add(("tokens", min(s["symbols"], 4097)))
                if s["mode"] == 1 and s["nblocks"] > 1:
                    seen.add("several blocks")
        seen.add(("escapes", any(info["nescapes"])))
        seen.add(("deep launches", any(c > 256 for c in info["nodes"][:-1])))
    assert {("token", 0), ("token", 1), ("escape", 0), ("occupancy", 0), ("occupancy", 1), ("tile", 0), ("tile", 1), ("tokens", 0), ("tokens", 1), ("tokens", 4095),
            ("tokens", 4096), ("tokens", 4097), "several blocks", ("escapes", True), ("escapes", False), ("deep launches", True), ("deep launches", False)} <= seen
    constant = tm.parse(pair("sphere, constant colour")[1])
    assert constant["nescapes"] == [0, 0, 0] and tm.coefficients(pair("sphere, constant colour")[0], 50)[0].max() == 0
    assert min(tm.parse(pair("sphere, random colours")[1])["nescapes"]) > 100


def test_input_order_does_not_change_the_bytes(codec, gpu):
    pts, bits, quality = clouds()["sphere at quality 50"]
    shuffled = pts[np.random.default_rng(3).permutation(len(pts))]
    enc = codec.cwipc_new_encoder(octree_bits=bits, jpeg_quality=quality, colour_transform=True)
    enc.feed(make_cloud(gpu, pts))
    enc.feed(make_cloud(gpu, shuffled))
    got = []
    for _ in range(2):
        assert enc.available(True)
        assert enc.get_encoded_size() == len(pair("sphere at quality 50")[1])
        got.append(bytes(enc.get_bytes()))
    assert got[0] == got[1] == pair("sphere at quality 50")[1]
    enc.free()


def test_group_of_plain_entropy_and_transform_encoders(codec, gpu):
    pts = clouds()["sphere at quality 85"][0]
    group = codec.cwipc_new_encodergroup()
    plain = group.addencoder(octree_bits=9, jpeg_quality=60)
    entropy = group.addencoder(octree_bits=8, jpeg_quality=85, entropy=True)
    transform = group.addencoder(octree_bits=9, jpeg_quality=85, colour_transform=True)
    with gpu.cwipc_hip_profile() as prof:
        group.feed(make_cloud(gpu, pts, 0.0, 1234))
        for enc in (plain, entropy, transform):
            assert enc.available(True)
    assert prof.kernels["codec_keys"][1] == 1 and prof.kernels["transform_assemble"][1] == 1       # one sort for the three
    assert bytes(plain.get_bytes()) == cm.encode(pts, 9, 60, 1234) == encode(codec, gpu, pts, 9, 60)
    assert bytes(entropy.get_bytes()) == em.pack(cm.encode(pts, 8, 85, 1234)) == encode(codec, gpu, pts, 8, 85, entropy=True)
    assert bytes(transform.get_bytes()) == pair("sphere at quality 85")[1] == encode(codec, gpu, pts, 9, 85, colour_transform=True)
    group.free()


def test_set_colour_transform_after_a_feed_is_refused(codec, gpu):
    pts, bits, quality = clouds()["9 leaves at 2 bits"]
    enc = codec.cwipc_new_encoder(octree_bits=bits, jpeg_quality=quality)
    enc.set_colour_transform(True)
    enc.set_colour_transform(False)
    enc.set_colour_transform(True)
    enc.feed(make_cloud(gpu, pts))
    with pytest.raises(gpu.CwipcError, match="cwipc_hip_encoder_set_colour_transform"):
        enc.set_colour_transform(False)
    dll = gpu.util.cwipc_util_dll_load()
    assert dll.cwipc_hip_encoder_set_colour_transform(enc._handle(), 0) == -1
    assert enc.available(True) and bytes(enc.get_bytes()) == pair("9 leaves at 2 bits")[1]
    enc.free()


def test_an_inter_mode_encoder_refuses_it_with_a_reason(codec, gpu):
    enc = codec.cwipc_new_encoder(octree_bits=7, jpeg_quality=60, do_inter_frame=True, gop_size=4, exp_factor=1.25)
    with pytest.raises(gpu.CwipcError, match="inter mode.*RULE P"):
        enc.set_colour_transform(True)
    with pytest.raises(gpu.CwipcError, match="inter mode"):
        codec.cwipc_new_encoder(octree_bits=7, jpeg_quality=60, do_inter_frame=True, gop_size=4, exp_factor=1.25, colour_transform=True)
    pts = clouds()["9 leaves at 2 bits"][0]
    enc.feed(make_cloud(gpu, pts))                       # the encoder is as it was: an inter-mode encoder
    assert enc.available(True) and bytes(enc.get_bytes())[:4] == b"cwap"
    enc.free()


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------
def test_damaged_containers_launch_nothing(codec, gpu):
    dll = gpu.util.cwipc_util_dll_load()
    dec = codec.cwipc_new_decoder()
    dll.cwipc_hip_synchronize()
    pool = dll.cwipc_hip_pool_bytes()
    with gpu.cwipc_hip_profile() as prof:
        for name, T in damage_packets().items():
            for what, data in damages(T)[::3]:
                with pytest.raises(gpu.CwipcError) as err:
                    dec.feed(data)
                assert "cwipc_hip_decoder_feed" in str(err.value), what
                assert not dec.available(False)
    assert prof.kernels == {} and dll.cwipc_hip_pool_bytes() == pool
    dec.free()


def replace_stream(packet, index, payload, mode):
    """The cwat packet with stream `index` given another payload and mode; the directory follows."""
    p = bytes(packet)
    info = tm.parse(p)
    s = info["streams"][index]
    entry = 48 + 4 * info["octree_bits"] + tm.FIXED + 4 + 8 * index
    return p[:entry] + struct.pack("<II", mode, len(payload)) + p[entry + 8:s["offset"]] + payload + p[s["offset"] + s["bytes"]:]


def device_side_refusals():
    """(what, packet, the reason's words): four packets that pass the container test and are refused by the checks on the device."""
    good = pair("sphere at quality 50")[1]
    info = tm.parse(good)
    out = []
    token = [s for s in info["streams"] if s["kind"] == "token" and s["mode"] == 1][0]
    at = int(token["block_offsets"][-1])
    out.append(("a broken block", good[:at + 8] + struct.pack("<I", 0xffff) + good[at + 12:], "not intact"))
    _, more = escape_count_off_by_one()
    out.append(("an escape count off by one", more, "escape count"))
    coded = [(i, s) for i, s in enumerate(info["streams"]) if s["kind"] == "occupancy" and s["mode"] == 1]
    assert len(coded) >= 2
    for (i, s), change in zip(coded[-2:], ("one bit more", "one bit less")):
        values = tm._stream_values(good, s, info).astype(np.int64)
        if change == "one bit more":
            k = int(np.nonzero(values != 255)[0][0])
            values[k] |= 1 << int(np.nonzero(((values[k] >> np.arange(8)) & 1) == 0)[0][0])
        else:
            k = int(np.nonzero((values & (values - 1)) != 0)[0][0])          # two bits or more: no byte becomes 0
            values[k] &= values[k] - 1
        payload = em.coded_payload("occupancy", values, 8)
        assert len(payload) < cm.pad4(len(values))
        out.append((f"coded occupancy of depth {s['which']}, {change}", replace_stream(good, i, payload, 1), "occupancy bits differ"))
    return good, out


def test_device_side_refusals_launch_nothing_further(codec, gpu):
    good, cases = device_side_refusals()
    assert len(cases) == 4
    dec = codec.cwipc_new_decoder()
    with gpu.cwipc_hip_profile() as prof:
        for what, data, reason in cases:
            tm.parse(data)                               # the container test lets it through
            with pytest.raises(tm.Invalid):
                tm.unpack(data)
            with pytest.raises(gpu.CwipcError) as err:
                dec.feed(data)
            assert "cwipc_hip_decoder_feed" in str(err.value) and reason in str(err.value), (what, str(err.value))
            assert not dec.available(False)
    assert "entropy_check" in prof.kernels and "transform_escape_scan" in prof.kernels
    assert not {"transform_inverse_top", "transform_rgb", "codec_points", "codec_expand"} & set(prof.kernels)
    dec.feed(good)                                       # the decoder is usable
    assert dec.available(True)
    assert dec.get().get_numpy_array().tobytes() == cm.decode(tm.unpack(good))[0].tobytes()
    dec.free()


# ---------------------------------------------------------------------------
# rate against distortion
# ---------------------------------------------------------------------------
RD_QUALITY = 24


def test_transform_costs_less_and_loses_no_more_at_the_coarse_end(codec, gpu):
    """The sphere of transform_model.sphere_cloud (400 k points, 9 bits, noise sigma 3) at quality 24: the colour payload of the "cwat"
    packet is strictly smaller than that of the "cwae" packet of the same cloud at the same quality, and the symmetric Y-PSNR is not
    lower.  The numpy models alone give 0.296 against 0.529 bytes a leaf, and 39.38 against 38.57 dB of Y-PSNR against the leaves' means, on
    this cloud at this quality (no other quality was tried)."""
    from cwipc_util_amd import quality
    pts = tm.sphere_cloud()
    pc = make_cloud(gpu, pts)
    packets = {}
    for form, kw in (("cwae", dict(entropy=True)), ("cwat", dict(colour_transform=True))):
        enc = codec.cwipc_new_encoder(octree_bits=9, jpeg_quality=RD_QUALITY, **kw)
        enc.feed(pc)
        assert enc.available(True)
        packets[form] = bytes(enc.get_bytes())
        enc.free()
    entropy_info, transform_info = codec.entropy_info(packets["cwae"]), codec.transform_info(packets["cwat"])
    nleaves = transform_info["nleaves"]
    assert nleaves == entropy_info["nleaves"] > 300000
    entropy_colour = sum(size + 8 for (mode, size), (kind, _, _) in zip(entropy_info["streams"], entropy_info["kinds"]) if kind == "colour")
    psnr = {}
    psnr["cwae"] = quality.codec_distortion(pc, entropy=True, octree_bits=9, jpeg_quality=RD_QUALITY, plane=False)[0].psnr_y
    psnr["cwat"] = quality.codec_distortion(pc, colour_transform=True, octree_bits=9, jpeg_quality=RD_QUALITY, plane=False)[0].psnr_y
    print(f"quality {RD_QUALITY}: cwae {entropy_colour / nleaves:.3f} B/leaf, Y {psnr['cwae']:.2f} dB; cwat {transform_info['colour_bytes'] / nleaves:.3f} B/leaf, "
          f"Y {psnr['cwat']:.2f} dB")
    assert transform_info["colour_bytes"] < entropy_colour
    assert psnr["cwat"] >= psnr["cwae"]


def test_nothing_is_left_behind(codec, gpu, clouds_before):
    """Last in the file: every cloud the tests above made has been freed with its wrapper."""
    gc.collect()
    assert gpu.cwipc_dangling_allocations(False) == clouds_before
