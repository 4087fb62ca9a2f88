"""The octree codec on the GPU (cwipc_util_amd.codec; RULE C in include/cwipc_util_amd/hip_ext.h) against its numpy restatement
(tests/codec_model.py).  There is no tolerance anywhere: packets are compared as bytes, decoded clouds as the bytes of their points
plus timestamp plus cellsize.  The input filters (tilenumber, voxelsize) are the library's own cwipc_tilefilter and cwipc_downsample:
the model is given what they return."""
import gc

import numpy as np
import pytest

import codec_model as cm
from conftest import make_cloud
from test_codec_model import HAND_PACKET, HAND_POINTS
from test_codec_packet_host import damages

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def codec(gpu):
    import cwipc_util_amd.codec as codec
    return codec


@pytest.fixture(scope="module", autouse=True)
def clouds_before(gpu):
    """What other test files of the same run still hold when this one starts."""
    gc.collect()
    return gpu.cwipc_dangling_allocations(False)


def encode(codec, cwipc, pts, bits, quality, timestamp=1234, **kw):
    enc = codec.cwipc_new_encoder(octree_bits=bits, jpeg_quality=quality, **kw)
    enc.feed(make_cloud(cwipc, pts, 0.0, timestamp))
    assert enc.available(True)
    assert enc.at_gop_boundary() and not enc.eof()
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


def check_decodes_to_model(codec, packet):
    pc = decode(codec, packet)
    want, ts, cell = cm.decode(packet)
    assert pc.count() == len(want) and pc.timestamp() == ts
    assert np.float32(pc.cellsize()).tobytes() == np.float32(cell).tobytes()
    assert pc.get_numpy_array().tobytes() == want.tobytes()
    return pc


def check(codec, cwipc, pts, bits, quality, timestamp=1234):
    """Encoder == model, decoder == model, on one cloud."""
    packet = encode(codec, cwipc, pts, bits, quality, timestamp)
    assert packet == cm.encode(pts, bits, quality, timestamp)
    check_decodes_to_model(codec, packet)
    return packet


def repeated_positions(rng, k, m):
    """k random positions, each m times (one leaf of exactly m points each, whatever the cube), with random colours and tiles."""
    pts = np.repeat(cm.random_cloud(rng, k, 1.5, (0.2, 0.1, -0.3)), m)
    pts['r'], pts['g'], pts['b'] = rng.integers(0, 256, (3, len(pts)))
    pts['tile'] = rng.choice(np.array([1, 2, 4, 8], dtype=np.uint8), len(pts))
    return pts


# ---------------------------------------------------------------------------
# sizes and distributions
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [1, 2, 9, 16])
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 255, 256, 257, 5003])
def test_sizes(codec, gpu, n, bits):
    rng = np.random.default_rng(1000 * bits + n)
    check(codec, gpu, cm.random_cloud(rng, n, 2.0, (1.0, -0.5, 0.25)), bits, 85)


def test_hand_written_packet(codec, gpu):
    assert encode(codec, gpu, HAND_POINTS, 2, 95, 0x0102) == HAND_PACKET
    check_decodes_to_model(codec, HAND_PACKET)


@pytest.mark.parametrize("bits", [1, 9, 16])
def test_all_points_in_one_cell(codec, gpu, bits):
    """3000 points in one leaf, across waves and workgroups: the sums must come out whole.  The two corner points pin the cube."""
    rng = np.random.default_rng(5)
    pts = cm.random_cloud(rng, 3002, 1e-7, (0.3, 0.3, 0.3))
    pts['x'][:3000], pts['y'][:3000], pts['z'][:3000] = 0.3, 0.3, 0.3
    pts['x'][3000], pts['y'][3000], pts['z'][3000] = 0, 0, 0
    pts['x'][3001], pts['y'][3001], pts['z'][3001] = 1, 1, 1
    pts = pts[rng.permutation(len(pts))]
    packet = check(codec, gpu, pts, bits, 95)
    assert cm.parse(packet)["nleaves"] == (2 if bits == 1 else 3)
    same = pts.copy()
    same['r'] = 255                      # 3002 x 255: the mean is 255, not a wrapped sum
    check(codec, gpu, same, bits, 95)


def test_coincident_points_have_a_cube_of_side_1(codec, gpu):
    pts = np.repeat(cm.make_cloud([[0.25, -4.0, 9.5]]), 300)
    pts['r'], pts['tile'] = np.arange(300) % 256, 2
    packet = check(codec, gpu, pts, 9, 95)
    info = cm.parse(packet)
    assert info["nleaves"] == 1 and info["side"] == 1.0


def test_every_point_in_a_cell_of_its_own(codec, gpu):
    rng = np.random.default_rng(6)
    g = np.arange(16) / 15.0
    xyz = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    pts = cm.make_cloud(xyz, rng.integers(0, 256, (4096, 3)), 1)[rng.permutation(4096)]
    packet = check(codec, gpu, pts, 4, 85)
    info = cm.parse(packet)
    assert info["nleaves"] == 4096 and info["nodes"] == [8, 64, 512, 4096]
    assert packet[info["occupancy_offset"]:info["occupancy_offset"] + info["occupancy_bytes"]] == b"\xff" * 585


@pytest.mark.parametrize("per_leaf", [64, 256, 61, 257])
def test_leaf_boundaries_on_and_off_wave_and_workgroup_boundaries(codec, gpu, per_leaf):
    rng = np.random.default_rng(per_leaf)
    pts = repeated_positions(rng, 24, per_leaf)
    shuffled = pts[rng.permutation(len(pts))]
    for bits in (2, 16):
        packet = check(codec, gpu, shuffled, bits, 95)
        if bits == 16:
            assert cm.parse(packet)["nleaves"] == 24


def test_points_on_the_max_faces_and_negative_coordinates(codec, gpu):
    rng = np.random.default_rng(8)
    pts = cm.random_cloud(rng, 3000, 5.0, (-20.0, -7.0, -0.001))
    for a, axis in enumerate("xyz"):
        pts[axis][a * 100:(a + 1) * 100] = pts[axis].max()
        pts[axis][300 + a * 100:300 + (a + 1) * 100] = pts[axis].min()
    assert (pts['x'] < 0).all() and (pts['y'] < 0).all()
    for bits in (1, 2, 9, 16):
        check(codec, gpu, pts, bits, 85)


def test_non_finite_points_are_left_out(codec, gpu):
    rng = np.random.default_rng(9)
    pts = cm.random_cloud(rng, 2000, 1.0)
    bad = rng.permutation(2000)[:300]
    pts['x'][bad[:100]] = np.nan
    pts['y'][bad[100:200]] = np.inf
    pts['z'][bad[200:]] = -np.inf
    pts['r'][bad], pts['tile'][bad] = 255, 128
    packet = check(codec, gpu, pts, 9, 95)
    assert packet == encode(codec, gpu, np.delete(pts, bad), 9, 95)
    only_bad = pts[bad]
    assert len(check(codec, gpu, only_bad, 9, 95)) == 48 + 36


@pytest.mark.parametrize("quality", [100, 90, 89, 75, 74, 50, 49, 25, 24, 0])
def test_every_quality_class(codec, gpu, quality):
    rng = np.random.default_rng(10)
    pts = cm.random_cloud(rng, 1501, 1.0)      # 1501 leaves x 3 channels x 4..8 bits: the colour plane ends inside a byte for some
    packet = check(codec, gpu, pts, 12, quality)
    assert packet[21] == 8 - cm.colour_shift(quality)


def test_tiles_mixed_and_uniform(codec, gpu):
    rng = np.random.default_rng(11)
    pts = cm.random_cloud(rng, 4000, 1.0, tiles=(1, 2, 4))
    mixed = check(codec, gpu, pts, 5, 85)
    assert cm.parse(mixed)["tile_mode"] == 1
    pts['tile'] = 4
    uniform = check(codec, gpu, pts, 5, 85)
    assert cm.parse(uniform)["tile_mode"] == 0 and uniform[23] == 4
    # every leaf holds both tiles: the ORs are all 3, which is uniform again
    both = np.concatenate([pts, pts])
    both['tile'][:4000], both['tile'][4000:] = 1, 2
    packet = check(codec, gpu, both, 5, 85)
    assert cm.parse(packet)["tile_mode"] == 0 and packet[23] == 3


@pytest.mark.parametrize("tilenumber", [0, 2, 3])
def test_tilenumber_is_the_tile_filter(codec, gpu, tilenumber):
    rng = np.random.default_rng(12)
    pts = cm.random_cloud(rng, 5000, 1.0, tiles=(1, 2, 3))
    packet = encode(codec, gpu, pts, 9, 85, tilenumber=tilenumber)
    kept = gpu.cwipc_tilefilter(make_cloud(gpu, pts), tilenumber).get_numpy_array()
    assert len(kept) == (len(pts) if tilenumber == 0 else int((pts['tile'] == tilenumber).sum()))
    assert packet == cm.encode(kept, 9, 85, 1234)
    check_decodes_to_model(codec, packet)
    assert len(encode(codec, gpu, pts, 9, 85, tilenumber=64)) == 48 + 36       # a tile that does not occur: an empty packet


def test_voxelsize_is_the_downsample_filter(codec, gpu):
    rng = np.random.default_rng(13)
    pts = cm.random_cloud(rng, 20000, 1.0)
    packet = encode(codec, gpu, pts, 9, 85, voxelsize=0.05)
    ds = gpu.cwipc_downsample(make_cloud(gpu, pts), 0.05)
    assert 0 < ds.count() < len(pts)
    assert packet == cm.encode(ds.get_numpy_array(), 9, 85, 1234)
    lone = codec.cwipc_new_encoder(octree_bits=9, jpeg_quality=85)
    lone.feed(ds)
    assert lone.available(True) and bytes(lone.get_bytes()) == packet
    check_decodes_to_model(codec, packet)


@pytest.mark.parametrize("bits", [9, 12])
def test_synthetic_100k(codec, gpu, synth, bits):
    pts, _ = synth(100000)
    packet = check(codec, gpu, pts, bits, 85)
    info = cm.parse(packet)
    assert 1000 < info["nleaves"] <= 100000
    # the decoder scans a depth's popcounts per workgroup of 256 nodes: several workgroups at 9 bits, and at 12 more than the 256 that
    # the scanning workgroup takes in one round (the cloud has 89330 nodes at depth 8 and more below)
    assert info["nodes"][-1] == info["nleaves"] and max(info["nodes"][:-1]) > (65536 if bits == 12 else 256 * 64), info["nodes"]


def test_order_independence_and_repeat(codec, gpu):
    rng = np.random.default_rng(14)
    pts = np.concatenate([cm.random_cloud(rng, 9000, 1.0), repeated_positions(rng, 5, 700)])
    enc = codec.cwipc_new_encoder(octree_bits=7, jpeg_quality=60)
    pc = make_cloud(gpu, pts)
    enc.feed(pc)
    enc.feed(pc)
    enc.feed(make_cloud(gpu, pts[np.random.default_rng(99).permutation(len(pts))]))
    packets = []
    for _ in range(3):
        assert enc.available(True)
        packets.append(bytes(enc.get_bytes()))
    assert packets[0] == packets[1] == packets[2] == cm.encode(pts, 7, 60, 1234)
    check_decodes_to_model(codec, packets[0])


# ---------------------------------------------------------------------------
# decoder
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [6, 9])
def test_reencoding_a_decoded_cloud_keeps_the_tree(codec, gpu, bits):
    """A decoded cloud's points are cell centres.  Its own cube starts half a cell further in and is one cell shorter (every axis has a
    point in cell 0, the longest axis one in cell 2^b - 1), so a centre of cell q lands at u = q / (2^b - 1) and
    floor(u 2^b) = floor(q + q / (2^b - 1)) = q for q < 2^b - 1, and the clamp gives q for the last.  The float32 rounding of the centres
    moves them by 2^-24 |p| / cell cells, against a margin of 1 / (2^b - 1) cells: with |p| <= 2 side and b <= 9 that is 6e-5 against
    2e-3.  Hence the same leaves and the same occupancy bytes, for these bits."""
    rng = np.random.default_rng(15 + bits)
    pts = cm.random_cloud(rng, 6000, 1.0, (0.5, 0.0, -0.5))
    first = encode(codec, gpu, pts, bits, 85)
    pc = decode(codec, first)
    enc = codec.cwipc_new_encoder(octree_bits=bits, jpeg_quality=85)
    enc.feed(pc)
    assert enc.available(True)
    second = bytes(enc.get_bytes())
    a, b = cm.parse(first), cm.parse(second)
    assert a["nleaves"] == b["nleaves"] and a["nodes"] == b["nodes"]
    assert first[a["occupancy_offset"]:a["colour_offset"]] == second[b["occupancy_offset"]:b["colour_offset"]]
    assert second == cm.encode(cm.decode(first)[0], bits, 85, 1234)


def test_decoded_clouds_are_ordinary_device_clouds(codec, gpu):
    rng = np.random.default_rng(16)
    a = decode(codec, encode(codec, gpu, cm.random_cloud(rng, 5000, 1.0), 9, 85, 40))
    b = decode(codec, encode(codec, gpu, cm.random_cloud(rng, 3000, 1.0, (3.0, 0, 0)), 8, 85, 50))
    assert gpu.util.cwipc_util_dll_load().cwipc_hip_is_device_resident(a.as_cwipc_p()) == 1
    host_a, host_b = make_cloud(gpu, a.get_numpy_array(), a.cellsize(), 40), make_cloud(gpu, b.get_numpy_array(), b.cellsize(), 50)
    joined = gpu.cwipc_join(a, b)
    assert joined.get_numpy_array().tobytes() == gpu.cwipc_join(host_a, host_b).get_numpy_array().tobytes()
    assert joined.count() == a.count() + b.count() and joined.timestamp() == 40
    ds, want = gpu.cwipc_downsample(a, 0.05), gpu.cwipc_downsample(host_a, 0.05)
    assert 0 < ds.count() < a.count() and ds.get_numpy_array().tobytes() == want.get_numpy_array().tobytes() and ds.cellsize() == want.cellsize()


# ---------------------------------------------------------------------------
# group
# ---------------------------------------------------------------------------
def test_group_delivers_what_each_encoder_delivers_alone(codec, gpu):
    rng = np.random.default_rng(17)
    frames = [cm.random_cloud(rng, 8000 + 100 * i, 1.0, (0.1 * i, 0, 0), tiles=(1, 2)) for i in range(3)]
    settings = [(tile, bits, quality) for tile in (1, 2) for bits in (6, 9, 12) for quality in (60, 95)]
    group = codec.cwipc_new_encodergroup()
    encoders = [group.addencoder(params=codec.cwipc_encoder_params(False, 1, 1.0, bits, quality, 16, tile, 0)) for tile, bits, quality in settings]
    for i, pts in enumerate(frames):                 # three frames in a row, then the results: first in, first out, per encoder
        group.feed(make_cloud(gpu, pts, 0.0, 500 + i))
    for i, pts in enumerate(frames):
        for enc, (tile, bits, quality) in zip(encoders, settings):
            assert enc.available(True)
            got = bytes(enc.get_bytes())
            assert got == encode(codec, gpu, pts, bits, quality, 500 + i, tilenumber=tile), (i, tile, bits, quality)
            assert got == cm.encode(pts[pts['tile'] == tile], bits, quality, 500 + i)
            if i == 0:
                check_decodes_to_model(codec, got)
    assert not any(enc.available(False) for enc in encoders)
    group.close()
    assert all(enc.eof() for enc in encoders)
    group.free()


# ---------------------------------------------------------------------------
# life cycle
# ---------------------------------------------------------------------------
def test_life_cycle(codec, gpu):
    rng = np.random.default_rng(18)
    enc = codec.cwipc_new_encoder(octree_bits=5, jpeg_quality=85)
    dec = codec.cwipc_new_decoder()
    assert not enc.available(False) and not dec.available(False) and dec.get() is None
    first, second = cm.random_cloud(rng, 700, 1.0), cm.random_cloud(rng, 900, 2.0)
    enc.feed(make_cloud(gpu, first, 0.0, 1))
    enc.feed(make_cloud(gpu, second, 0.0, 2))
    packets = []
    for _ in range(2):
        assert enc.available(True)
        packets.append(bytes(enc.get_bytes()))
    assert packets == [cm.encode(first, 5, 85, 1), cm.encode(second, 5, 85, 2)]
    dec.feed(packets[0])
    dec.feed(packets[1])
    for packet in packets:
        assert dec.available(True)
        pc = dec.get()
        assert pc.timestamp() == cm.parse(packet)["timestamp"] and pc.get_numpy_array().tobytes() == cm.decode(packet)[0].tobytes()
    enc.close()
    dec.close()
    assert enc.eof() and dec.eof()
    with pytest.raises(gpu.CwipcError):
        enc.feed(make_cloud(gpu, first))
    enc.free()
    dec.free()


@pytest.mark.parametrize("kw,message", [(dict(do_inter_frame=True), "do_inter_frame"), (dict(gop_size=2), "gop_size"), (dict(exp_factor=2.0), "exp_factor"),
                                        (dict(octree_bits=0), "octree_bits"), (dict(octree_bits=17), "octree_bits"), (dict(jpeg_quality=-1), "jpeg_quality"),
                                        (dict(jpeg_quality=101), "jpeg_quality")])
def test_refused_parameters(codec, gpu, kw, message):
    with pytest.raises(gpu.CwipcError, match=message):
        codec.cwipc_new_encoder(**kw)
    group = codec.cwipc_new_encodergroup()
    with pytest.raises(gpu.CwipcError, match=message):
        group.addencoder(**kw)
    group.free()
    codec.cwipc_new_encoder(macroblock_size=4).free()        # accepted and ignored


def test_malformed_packets_launch_nothing(codec, gpu):
    """Only packets that the host-side validator refuses are fed: the profiling counters, which see every launch of the library, stay
    empty, and the memory pool does not grow."""
    rng = np.random.default_rng(19)
    good = encode(codec, gpu, cm.random_cloud(rng, 3000, 1.0), 6, 60)
    dll = gpu.util.cwipc_util_dll_load()
    dec = codec.cwipc_new_decoder()
    dll.cwipc_hip_synchronize()
    pool = dll.cwipc_hip_pool_bytes()
    with gpu.cwipc_hip_profile() as prof:
        for packet in (good, HAND_PACKET):
            for what, data in damages(packet):
                with pytest.raises(gpu.CwipcError) as err:
                    dec.feed(data)
                assert "cwipc_hip_decoder_feed" in str(err.value), what
                assert not dec.available(False)
    assert prof.kernels == {} and dll.cwipc_hip_pool_bytes() == pool
    with gpu.cwipc_hip_profile() as prof:      # the counters do see a packet that is decoded
        dec.feed(good)
        assert dec.available(True)
    assert "codec_points" in prof.kernels and "codec_expand" in prof.kernels
    assert dec.get().count() == cm.parse(good)["nleaves"]


# ---------------------------------------------------------------------------
# pipeline
# ---------------------------------------------------------------------------
def test_pipeline_sink_encoder_to_source_decoder_to_synchronizer(codec, gpu):
    """Two TileSource tiles -> cwipc_sink_encoder -> one packet list per stream -> two cwipc_source_decoder -> cwipc_source_synchronizer:
    the cloud is the join of the two decoded tiles, timestamp the smaller one, for three frames."""
    from cwipc_util_amd.capture import TileSource, capture_tile
    from cwipc_util_amd.net import cwipc_source_synchronizer
    from cwipc_util_amd.net.sink_encoder import cwipc_sink_encoder
    from cwipc_util_amd.net.source_decoder import cwipc_source_decoder
    tiles = [capture_tile(6000, t, 2) for t in range(2)]
    host_tiles = [t.get_numpy_array() for t in tiles]
    sources = [TileSource(t, 3, first_timestamp=100, timestamp_step=33) for t in tiles]
    streams = []
    sink = cwipc_sink_encoder(streams, nodrop=True)
    sink.set_encoder_params([dict(cameraMask=1), dict(cameraMask=2)], octree_bits=8, jpeg_quality=60)
    for _ in range(3):
        sink.feed(gpu.cwipc_join(sources[0].get(), sources[1].get()))
    assert len(streams) == 2 and [len(s) for s in streams] == [3, 3]
    for i, stream in enumerate(streams):
        assert stream == [cm.encode(host_tiles[i], 8, 60, 100 + 33 * f) for f in range(3)]
    expected = [[cm.decode(p)[0] for p in stream] for stream in streams]
    cellsizes = [[cm.decode(p)[2] for p in stream] for stream in streams]
    decoders = [cwipc_source_decoder(stream) for stream in streams]
    sync = cwipc_source_synchronizer(None, decoders)
    for f in range(3):
        fused = sync.core.poll()
        assert fused is not None and fused.timestamp() == 100 + 33 * f
        assert fused.get_numpy_array().tobytes() == np.concatenate([expected[0][f], expected[1][f]]).tobytes()
        assert np.float32(fused.cellsize()) == min(cellsizes[0][f], cellsizes[1][f])
    assert sync.core.poll() is None and all(d.eof() for d in decoders)
    sink.free()
    for d in decoders:
        d.free()


def test_nothing_is_left_behind(codec, gpu, clouds_before):
    """Last in the file: every cloud the tests above made has been freed with its wrapper (alone, this file starts from 0)."""
    gc.collect()
    assert gpu.cwipc_dangling_allocations(False) == clouds_before
