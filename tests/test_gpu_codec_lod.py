"""Level-of-detail decoding on the GPU (RULE L in include/cwipc_util_amd/hip_ext.h; csrc/kernels_lod.hip) against its numpy
restatement (tests/lod_model.py): a decoder with set_max_octree_bits(t) hands out, for a packet that stands for the "cwao" packet P,
exactly the cloud cm.decode(lm.lod(P, t)) -- points, colours, tiles, count, timestamp, cellsize, compared as bytes.  No tolerance
anywhere."""
import gc

import numpy as np
import pytest

import codec_model as cm
import entropy_model as em
import lod_model as lm
from conftest import make_cloud

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def codec(gpu):
    import cwipc_util_amd.codec as codec
    return codec


@pytest.fixture(scope="module", autouse=True)
def clouds_before(gpu):
    gc.collect()
    return gpu.cwipc_dangling_allocations(False)


_cuts = {}


def model_cloud(plain, t):
    """cm.decode(L(P, min(t, b))), computed once per (packet, t) and left unchanged."""
    plain = bytes(plain)
    b = cm.parse(plain)["octree_bits"]
    key = (plain, min(t, b))
    if key not in _cuts:
        _cuts[key] = cm.decode(lm.lod(plain, min(t, b)))
    return _cuts[key]


def same_cloud(pc, want):
    points, ts, cell = want
    assert pc is not None and pc.count() == len(points) and pc.timestamp() == ts
    assert np.float32(pc.cellsize()).tobytes() == np.float32(cell).tobytes()
    got = pc.get_numpy_array()
    for f in ("x", "y", "z", "r", "g", "b", "tile"):
        assert got[f].tobytes() == points[f].tobytes(), f
    assert got.tobytes() == points.tobytes()


def fed(dec, packet):
    dec.feed(packet)
    assert dec.available(True)
    pc = dec.get()
    assert pc is not None and not dec.available(False)
    return pc


def targets_for(b):
    """1, one in the middle, b - 1, b, b + 1."""
    return [t for t in sorted({1, max(1, b // 2), max(1, b - 1), b, b + 1}) if t <= 16]


HAND = lm.hand_packets()


@pytest.mark.parametrize("name", list(HAND))
def test_hand_built_packets_in_both_plain_forms(codec, gpu, name):
    plain = HAND[name]
    coded = bytes(codec.entropy_pack(plain))
    assert coded == em.pack(plain)
    dec = codec.cwipc_new_decoder()
    for t in targets_for(cm.parse(plain)["octree_bits"]):
        dec.set_max_octree_bits(t)
        same_cloud(fed(dec, plain), model_cloud(plain, t))
        same_cloud(fed(dec, coded), model_cloud(plain, t))
    dec.free()


@pytest.fixture(scope="module")
def structured():
    return em.structured_cloud(60000)


def encode(codec, gpu, pts, bits, quality, timestamp=4242, **kw):
    enc = codec.cwipc_new_encoder(octree_bits=bits, jpeg_quality=quality, **kw)
    enc.feed(make_cloud(gpu, pts, 0.0, timestamp))
    assert enc.available(True)
    data = bytes(enc.get_bytes())
    enc.free()
    return data


FORMS = {
    "cwao": (dict(), 85),
    "cwae": (dict(entropy=True), 85),
    "cwat, quality 24": (dict(colour_transform=True), 24),
    "cwat, quality 100": (dict(colour_transform=True), 100),
}


@pytest.mark.parametrize("form", list(FORMS))
def test_structured_cloud_through_the_real_encoder(codec, gpu, structured, form):
    kw, quality = FORMS[form]
    packet = encode(codec, gpu, structured, 9, quality, **kw)
    assert packet[:4] == form[:4].encode()
    plain = packet if form == "cwao" else bytes(codec.entropy_unpack(packet)) if form == "cwae" else bytes(codec.transform_unpack(packet))
    assert cm.parse(plain)["octree_bits"] == 9 and cm.parse(plain)["nleaves"] > 30000
    dec = codec.cwipc_new_decoder()
    for t in targets_for(9):
        dec.set_max_octree_bits(t)
        same_cloud(fed(dec, packet), model_cloud(plain, t))
    dec.free()


def test_geometry_of_a_cut_is_that_of_the_native_packet(codec, gpu, structured):
    full = encode(codec, gpu, structured, 9, 85)
    for t in (1, 4, 8):
        native = fed(codec.cwipc_new_decoder(), encode(codec, gpu, structured, t, 85))
        cut = fed(codec.cwipc_new_decoder(max_octree_bits=t), full)
        a, b = native.get_numpy_array(), cut.get_numpy_array()
        assert native.count() == cut.count() and np.float32(native.cellsize()).tobytes() == np.float32(cut.cellsize()).tobytes()
        for f in ("x", "y", "z", "tile"):
            assert a[f].tobytes() == b[f].tobytes(), (t, f)


@pytest.mark.parametrize("entropy", [False, True])
def test_key_and_two_deltas_keep_the_full_reference(codec, gpu, structured, entropy):
    frames = []
    for i in range(3):          # a part of the surface moves and changes colour from frame to frame: leaves leave, come and change
        f = structured.copy()
        cap = f['x'] > 0.7
        f['x'][cap] -= np.float32(0.004 * i)
        f['g'][cap] = np.minimum(255, f['g'][cap].astype(np.int64) + 9 * i).astype(np.uint8)
        frames.append(f)
    enc = codec.cwipc_new_encoder(octree_bits=9, jpeg_quality=85, do_inter_frame=True, gop_size=4, exp_factor=1.25, entropy=entropy)
    packets = []
    for i, f in enumerate(frames):
        enc.feed(make_cloud(gpu, f, 0.0, 100 + i))
        assert enc.available(True)
        packets.append(bytes(enc.get_bytes()))
    enc.free()
    assert [codec.inter_info_kind(p) for p in packets] == ["key", "delta", "delta"]
    plain, before = [], None
    for p in packets:
        before = bytes(codec.inter_unpack(before, p))
        if before[:4] == b"cwae":
            before = bytes(codec.entropy_unpack(before))
        plain.append(before)
    assert codec.inter_info(packets[2])["nadded"] > 0
    for t in targets_for(9):
        full, cut = codec.cwipc_new_decoder(), codec.cwipc_new_decoder(max_octree_bits=t)
        for i, (p, q) in enumerate(zip(packets, plain)):
            whole = fed(full, p)
            assert whole.get_numpy_array().tobytes() == cm.decode(q)[0].tobytes()
            same_cloud(fed(cut, p), model_cloud(q, t))       # (the second delta is accepted: the reference is the full frame)
        full.free()
        cut.free()


def test_setter_misuse_and_changes_between_feeds(codec, gpu):
    plain = HAND["cb 7, 333 leaves"]
    dec, untouched = codec.cwipc_new_decoder(), codec.cwipc_new_decoder()
    for bad in (-1, 17):
        with pytest.raises(gpu.CwipcError, match="cwipc_hip_decoder_set_max_octree_bits"):
            dec.set_max_octree_bits(bad)
    same_cloud(fed(dec, plain), cm.decode(plain))            # a refused setting changes nothing
    # a change applies to the next feed only: a cloud fed before it, and not yet taken, stays what it was
    dec.set_max_octree_bits(2)
    dec.feed(plain)
    dec.set_max_octree_bits(3)
    dec.feed(plain)
    dec.set_max_octree_bits(None)
    dec.feed(plain)
    for want in (model_cloud(plain, 2), model_cloud(plain, 3), cm.decode(plain)):
        assert dec.available(True)
        same_cloud(dec.get(), want)
    # a decoder that never calls the setter gives today's bytes, and so does one whose limit is not below the packet's bits
    for limit in (5, 6, 16):
        dec.set_max_octree_bits(limit)
        assert fed(dec, plain).get_numpy_array().tobytes() == fed(untouched, plain).get_numpy_array().tobytes() == cm.decode(plain)[0].tobytes()
    # an empty cloud's packet: the cut's cellsize
    empty = cm.encode(np.zeros(0, dtype=cm.POINT_DTYPE), 9, 60, timestamp=99)
    dec.set_max_octree_bits(4)
    same_cloud(fed(dec, empty), model_cloud(empty, 4))
    dec.free()
    untouched.free()


def test_a_refused_packet_is_refused_as_before(codec, gpu):
    plain = HAND["plane stays"]
    dec = codec.cwipc_new_decoder(max_octree_bits=2)
    for bad in (plain[:-1], plain + b"\x00", plain[:60] + bytes([0]) + plain[61:]):
        with pytest.raises(gpu.CwipcError):
            dec.feed(bad)
        assert not dec.available(False)
    same_cloud(fed(dec, plain), model_cloud(plain, 2))
    dec.free()


def test_source_decoder_and_quality_pass_the_limit_on(codec, gpu, structured):
    from cwipc_util_amd import quality
    from cwipc_util_amd.net.source_decoder import cwipc_source_decoder
    packet = encode(codec, gpu, structured[:5000], 7, 85)
    src = cwipc_source_decoder([packet], max_octree_bits=3)
    assert src.available(True)
    same_cloud(src.get(), model_cloud(packet, 3))
    src.free()
    pc = make_cloud(gpu, structured[:5000], 0.0, 1)
    whole, nbytes = quality.codec_distortion(pc, octree_bits=7, jpeg_quality=85)
    cut, cut_bytes = quality.codec_distortion(pc, octree_bits=7, jpeg_quality=85, decode_bits=4)
    native, native_bytes = quality.codec_distortion(pc, octree_bits=4, jpeg_quality=85)
    assert nbytes == cut_bytes > native_bytes
    assert cut.psnr_d1 == native.psnr_d1 < whole.psnr_d1      # the geometry of the cut is the native packet's


def test_nothing_is_left_behind(codec, gpu, clouds_before):
    """Last in the file: every cloud the tests above made has been freed with its wrapper."""
    gc.collect()
    assert gpu.cwipc_dangling_allocations(False) == clouds_before
