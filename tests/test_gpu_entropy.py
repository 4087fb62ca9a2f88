"""The entropy-coded packet form on the GPU (RULE E in include/cwipc_util_amd/hip_ext.h; csrc/kernels_entropy.hip) against its numpy
restatement (tests/entropy_model.py).  Bytes only: an encoder with entropy=True must deliver entropy_model.pack(codec_model.encode(...)),
a decoder fed that packet the cloud it hands out for the plain packet.  The damaged packets are the ones test_entropy_host.py has
already run through the sanitised host program: the container test refuses them before anything is launched, the payload damages are
refused by the check inside feed."""
import gc

import numpy as np
import pytest

import codec_model as cm
import entropy_model as em
from conftest import make_cloud
from test_entropy_model import model_packets, packed

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def codec(gpu):
    import cwipc_util_amd.codec as codec
    return codec


@pytest.fixture(scope="module", autouse=True)
def clouds_before(gpu):
    gc.collect()
    return gpu.cwipc_dangling_allocations(False)


_clouds = {}


def clouds():
    """name -> (points, octree_bits, jpeg_quality): shared, read only."""
    if _clouds:
        return _clouds
    rng = np.random.default_rng(900)
    structured = em.structured_cloud()
    _clouds["structured, 9 bits"] = (structured, 9, 85)
    _clouds["structured, 7 bits"] = (structured, 7, 85)
    for n in (1, 65, 700, 5003):
        _clouds[f"random {n}"] = (cm.random_cloud(rng, n, 2.0, (1.0, -0.5, 0.25)), 9, 85)
    _clouds["131073 points at 16 bits"] = (cm.random_cloud(rng, 131073, 1.0), 16, 85)
    small = em.structured_cloud(20000, seed=1)
    for quality in (95, 80, 60, 30, 10):
        _clouds[f"quality {quality}"] = (small, 8, quality)
    uniform = small.copy()
    uniform['tile'] = 4
    _clouds["uniform tiles"] = (uniform, 8, 85)
    _clouds["empty"] = (cm.random_cloud(rng, 0), 9, 85)
    for pts, _, _ in _clouds.values():
        pts.setflags(write=False)
    return _clouds


_pairs = {}


def pair(name):
    """(the plain packet, its entropy-coded form), both from the models."""
    if name not in _pairs:
        pts, bits, quality = clouds()[name]
        plain = cm.encode(pts, bits, quality, 1234)
        _pairs[name] = (plain, em.pack(plain))
    return _pairs[name]


def encode(codec, cwipc, pts, bits, quality, timestamp=1234, **kw):
    enc = codec.cwipc_new_encoder(octree_bits=bits, jpeg_quality=quality, **kw)
    enc.feed(make_cloud(cwipc, pts, 0.0, timestamp))
    assert enc.available(True)
    data = bytes(enc.get_bytes())
    assert not enc.available(False)
    return data


def decode(codec, packet):
    dec = codec.cwipc_new_decoder()
    dec.feed(packet)
    assert dec.available(True)
    pc = dec.get()
    assert pc is not None and not dec.available(False)
    return pc


# ---------------------------------------------------------------------------
# encoder
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(clouds()))
def test_encoder_delivers_the_model_packet(codec, gpu, name):
    pts, bits, quality = clouds()[name]
    plain, coded = pair(name)
    got = encode(codec, gpu, pts, bits, quality, entropy=True)
    assert got[:4] == b"cwae" and len(got) == len(coded)
    assert got == coded
    assert bytes(codec.entropy_unpack(got)) == plain
    assert encode(codec, gpu, pts, bits, quality) == plain                   # entropy off, the default: today's bytes
    assert encode(codec, gpu, pts, bits, quality, entropy=False) == plain


def test_the_inputs_reach_every_path():
    """Coded and raw streams of every kind, several blocks per stream, a last block that is not full, a packet without tile plane."""
    seen = set()
    for name in clouds():
        for s in em.parse(pair(name)[1])["streams"]:
            seen.add((s["kind"], s["mode"]))
            if s["mode"] == 1 and s["nblocks"] > 1 and s["symbols"] % 4096:
                seen.add("partial last block")
    assert {("occupancy", 0), ("occupancy", 1), ("colour", 0), ("colour", 1), ("tile", 0), ("tile", 1), "partial last block"} <= seen
    assert cm.parse(pair("uniform tiles")[0])["tile_mode"] == 0 and len(em.parse(pair("uniform tiles")[1])["streams"]) == 8 + 3
    assert len(pair("structured, 9 bits")[1]) < 0.6 * len(pair("structured, 9 bits")[0])
    assert [s["mode"] for s in em.parse(pair("131073 points at 16 bits")[1])["streams"] if s["kind"] == "colour"] == [0, 0, 0]


def lattice_cloud(tiles, rng):
    """One point per cell of a 32 x 32 x 16 lattice at 5 bits (k / 31 lies in cell k), the first len(tiles) cells taken: the tile
    plane holds exactly `tiles`, in some order, so its 256 counts are the test's to choose."""
    g = np.arange(32) / 31.0
    xyz = np.stack(np.meshgrid(g, g, g[:16], indexing="ij"), axis=-1).reshape(-1, 3)
    xyz[-1] = (1.0, 1.0, 1.0)                    # (pins the cube's side to 1 when cells are left out)
    keep = np.concatenate([rng.permutation(len(xyz) - 1)[:len(tiles) - 1], [len(xyz) - 1]])
    return cm.make_cloud(xyz[keep], rng.integers(0, 256, (len(tiles), 3)), np.asarray(tiles, dtype=np.uint8))


@pytest.mark.parametrize("case", ["one large count, every symbol once", "two equal large counts, every symbol once", "three equal counts"])
def test_frequencies_on_the_paths_of_the_rule(codec, gpu, case):
    """The kernel normalises on a wave, the host and the model serially: the tile plane's counts are chosen to take d < 0 with one
    symbol on top (191 decrements), d < 0 with two symbols tied on top, and d > 0 with three tied counts."""
    rng = np.random.default_rng(len(case))
    if case.startswith("one"):
        tiles = np.concatenate([np.full(16384 - 255, 100), np.delete(np.arange(256), 100)])
    elif case.startswith("two"):
        tiles = np.concatenate([np.full(8065, 7), np.full(8065, 200), np.delete(np.arange(256), [7, 200])])
    else:
        tiles = np.repeat([5, 9, 11], 5461)
    pts = lattice_cloud(rng.permutation(tiles), rng)
    plain = cm.encode(pts, 5, 85, 1234)
    info = cm.parse(plain)
    assert info["nleaves"] == len(tiles) and info["tile_mode"] == 1
    coded = em.pack(plain)
    stream = em.parse(coded)["streams"][-1]
    assert stream["kind"] == "tile" and stream["mode"] == 1
    counts = np.bincount(tiles, minlength=256)
    floors = np.where(counts > 0, np.maximum(1, counts * 4096 // counts.sum()), 0)
    assert (4096 - floors.sum() < -100) if case[1] == "n" or case[1] == "w" else (4096 - floors.sum() == 1)
    assert np.array_equal(stream["f"], em.normalise(counts))
    assert encode(codec, gpu, pts, 5, 85, entropy=True) == coded
    assert decode(codec, coded).get_numpy_array().tobytes() == cm.decode(plain)[0].tobytes()


def test_input_order_does_not_change_the_bytes(codec, gpu):
    pts, bits, quality = clouds()["structured, 7 bits"]
    shuffled = pts[np.random.default_rng(3).permutation(len(pts))]
    enc = codec.cwipc_new_encoder(octree_bits=bits, jpeg_quality=quality, entropy=True)
    enc.feed(make_cloud(gpu, pts))
    enc.feed(make_cloud(gpu, shuffled))
    enc.feed(make_cloud(gpu, pts))
    got = []
    for _ in range(3):
        assert enc.available(True)
        assert enc.get_encoded_size() == len(pair("structured, 7 bits")[1])
        got.append(bytes(enc.get_bytes()))
    assert got[0] == got[1] == got[2] == pair("structured, 7 bits")[1]
    assert not enc.available(False)


def test_polling_settles_the_size(codec, gpu):
    pts, bits, quality = clouds()["structured, 9 bits"]
    enc = codec.cwipc_new_encoder(octree_bits=bits, jpeg_quality=quality)
    enc.set_entropy(True)
    enc.feed(make_cloud(gpu, pts))
    for _ in range(2000000):
        if enc.available(False):
            break
    assert enc.available(False)
    assert bytes(enc.get_bytes()) == pair("structured, 9 bits")[1]


def test_set_entropy_after_a_feed_is_refused(codec, gpu):
    pts, bits, quality = clouds()["random 700"]
    enc = codec.cwipc_new_encoder(octree_bits=bits, jpeg_quality=quality)
    enc.set_entropy(True)
    enc.set_entropy(False)
    enc.feed(make_cloud(gpu, pts))
    with pytest.raises(gpu.CwipcError, match="cwipc_hip_encoder_set_entropy"):
        enc.set_entropy(True)
    assert enc.available(True) and bytes(enc.get_bytes()) == pair("random 700")[0]
    group = codec.cwipc_new_encodergroup()
    member = group.addencoder(octree_bits=bits, jpeg_quality=quality)
    member.set_entropy(True)
    group.feed(make_cloud(gpu, pts))
    with pytest.raises(gpu.CwipcError, match="cwipc_hip_encoder_set_entropy"):
        member.set_entropy(False)
    assert member.available(True) and bytes(member.get_bytes()) == pair("random 700")[1]
    group.free()


def test_group_of_entropy_and_plain_encoders_shares_one_sort(codec, gpu):
    pts = clouds()["structured, 9 bits"][0]
    settings = [(9, 85, True), (9, 85, False), (7, 60, True), (7, 60, False), (5, 10, True)]
    group = codec.cwipc_new_encodergroup()
    encoders = [group.addencoder(octree_bits=bits, jpeg_quality=quality, entropy=entropy) for bits, quality, entropy in settings]
    with gpu.cwipc_hip_profile() as prof:
        for frame in range(2):
            group.feed(make_cloud(gpu, pts, 0.0, 70 + frame))
        for enc in encoders:
            assert enc.available(True)
    assert prof.kernels["codec_keys"][1] == 2 and prof.kernels["entropy_plan"][1] == 6       # one sort per frame; three entropy stages per frame
    for frame in range(2):
        for enc, (bits, quality, entropy) in zip(encoders, settings):
            plain = cm.encode(pts, bits, quality, 70 + frame)
            assert enc.available(True)
            got = bytes(enc.get_bytes())
            assert got == (em.pack(plain) if entropy else plain), (frame, bits, quality, entropy)
            if frame == 0:
                assert got == encode(codec, gpu, pts, bits, quality, 70, entropy=entropy)
    group.free()


# ---------------------------------------------------------------------------
# decoder
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(clouds()))
def test_decoder_hands_out_the_plain_packets_cloud(codec, gpu, name):
    plain, coded = pair(name)
    a, b = decode(codec, plain), decode(codec, coded)
    want, ts, cell = cm.decode(plain)
    assert b.count() == len(want) and b.timestamp() == a.timestamp() == ts
    assert np.float32(b.cellsize()).tobytes() == np.float32(cell).tobytes()
    assert b.get_numpy_array().tobytes() == a.get_numpy_array().tobytes() == want.tobytes()


def test_model_packets_of_every_shape_decode(codec, gpu):
    """The packets of test_entropy_model.py: 4095, 4096, 4097 and 8193 leaves, 4 and 8 colour bits, one leaf, 1 and 16 bits."""
    for name, plain in model_packets().items():
        pc = decode(codec, packed(name))
        assert pc.get_numpy_array().tobytes() == cm.decode(plain)[0].tobytes(), name
        assert pc.timestamp() == cm.parse(plain)["timestamp"]


def test_mixed_packets_come_out_first_in_first_out(codec, gpu):
    order = [("structured, 7 bits", 1), ("random 5003", 0), ("quality 60", 1), ("empty", 1), ("quality 60", 0), ("structured, 9 bits", 1)]
    dec = codec.cwipc_new_decoder()
    for name, form in order:
        dec.feed(pair(name)[form])
    for name, _ in order:
        assert dec.available(True)
        assert dec.get().get_numpy_array().tobytes() == cm.decode(pair(name)[0])[0].tobytes(), name
    assert not dec.available(False) and dec.get() is None
    dec.free()


def test_damaged_containers_launch_nothing(codec, gpu):
    """Only packets that the host-side container test refuses are fed: the profiling counters, which see every launch of the library,
    stay empty, and the memory pool does not grow."""
    dll = gpu.util.cwipc_util_dll_load()
    dec = codec.cwipc_new_decoder()
    good = pair("structured, 7 bits")[1]
    dll.cwipc_hip_synchronize()
    pool = dll.cwipc_hip_pool_bytes()
    with gpu.cwipc_hip_profile() as prof:
        for name in ("random 700", "structured, 7 bits", "empty"):
            for what, data in em.damages(pair(name)[1]):
                with pytest.raises(gpu.CwipcError) as err:
                    dec.feed(data)
                assert "cwipc_hip_decoder_feed" in str(err.value), what
                assert not dec.available(False)
    assert prof.kernels == {} and dll.cwipc_hip_pool_bytes() == pool
    with gpu.cwipc_hip_profile() as prof:      # the counters do see a packet that is decoded
        dec.feed(good)
        assert dec.available(True)
    assert {"entropy_block_decode", "entropy_repack", "entropy_check", "codec_points", "codec_expand"} <= set(prof.kernels)
    assert dec.get().count() == cm.parse(pair("structured, 7 bits")[0])["nleaves"]
    dec.free()


def test_damaged_payloads_are_refused_at_feed(codec, gpu):
    """Eight of the payload damages that the sanitised host program has decoded in bounds (test_entropy_host.py, on this very packet):
    the container test lets them through, the check inside feed refuses them, and none of the octree decoder's kernels runs."""
    good = packed("structured, 9 bits")
    cases = em.payload_damages(good)
    picked = cases[:4] + cases[-4:]
    assert len({what.split()[1] for what, _ in picked}) == 2 and len(picked) == 8         # two streams
    dec = codec.cwipc_new_decoder()
    with gpu.cwipc_hip_profile() as prof:
        for what, data in picked:
            with pytest.raises(gpu.CwipcError) as err:
                dec.feed(data)
            assert "cwipc_hip_decoder_feed" in str(err.value), what
            assert any(reason in str(err.value) for reason in ("not intact", "occupancy")), what
            assert not dec.available(False)
    assert "entropy_check" in prof.kernels and "codec_points" not in prof.kernels and "codec_expand" not in prof.kernels
    dec.feed(good)
    assert dec.available(True)
    assert dec.get().get_numpy_array().tobytes() == cm.decode(model_packets()["structured, 9 bits"])[0].tobytes()
    dec.free()


# ---------------------------------------------------------------------------
# pipeline
# ---------------------------------------------------------------------------
def test_pipeline_sink_encoder_with_entropy_to_source_decoder_to_synchronizer(codec, gpu):
    from cwipc_util_amd.capture import TileSource, capture_tile
    from cwipc_util_amd.net import cwipc_source_synchronizer
    from cwipc_util_amd.net.sink_encoder import cwipc_sink_encoder
    from cwipc_util_amd.net.source_decoder import cwipc_source_decoder
    tiles = [capture_tile(6000, t, 2) for t in range(2)]
    host_tiles = [t.get_numpy_array() for t in tiles]
    sources = [TileSource(t, 2, first_timestamp=100, timestamp_step=33) for t in tiles]
    streams = []
    sink = cwipc_sink_encoder(streams, nodrop=True)
    sink.set_encoder_params([dict(cameraMask=1), dict(cameraMask=2)], octree_bits=8, jpeg_quality=60, entropy=True)
    for _ in range(2):
        sink.feed(gpu.cwipc_join(sources[0].get(), sources[1].get()))
    assert len(streams) == 2 and [len(s) for s in streams] == [2, 2]
    plain = [[cm.encode(host_tiles[i], 8, 60, 100 + 33 * f) for f in range(2)] for i in range(2)]
    for i, stream in enumerate(streams):
        assert [bytes(p) for p in stream] == [em.pack(p) for p in plain[i]]
    decoders = [cwipc_source_decoder(stream) for stream in streams]
    sync = cwipc_source_synchronizer(None, decoders)
    for f in range(2):
        fused = sync.core.poll()
        assert fused is not None and fused.timestamp() == 100 + 33 * f
        assert fused.get_numpy_array().tobytes() == np.concatenate([cm.decode(plain[0][f])[0], cm.decode(plain[1][f])[0]]).tobytes()
    assert sync.core.poll() is None and all(d.eof() for d in decoders)
    sink.free()
    for d in decoders:
        d.free()


def test_nothing_is_left_behind(codec, gpu, clouds_before):
    """Last in the file: every cloud the tests above made has been freed with its wrapper."""
    gc.collect()
    assert gpu.cwipc_dangling_allocations(False) == clouds_before
