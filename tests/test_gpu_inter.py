"""Inter-frame coding on the GPU (RULE P in include/cwipc_util_amd/hip_ext.h; csrc/kernels_inter.hip) against its numpy restatement
(tests/inter_model.py).  Bytes only: an inter-mode encoder must deliver the model encoder's packets over whole sequences, a decoder
fed them the clouds a plain decoder hands out for the packets they stand for.  The damaged deltas are ones test_inter_host.py has
already run through the sanitised host program: the container test refuses them before anything is launched, the payload damages are
refused by the check inside feed, with none of the point-making kernels launched and the reference left as it was."""
import gc
import threading

import numpy as np
import pytest

import codec_model as cm
import entropy_model as em
import inter_model as im
from conftest import make_cloud
from test_inter_model import container_cases, delta, pairs, payload_cases

pytestmark = pytest.mark.gpu

EMPTY = np.zeros(0, dtype=cm.POINT_DTYPE)


@pytest.fixture(scope="module")
def codec(gpu):
    import cwipc_util_amd.codec as codec
    return codec


@pytest.fixture(scope="module", autouse=True)
def clouds_before(gpu):
    gc.collect()
    return gpu.cwipc_dangling_allocations(False)


# ---------------------------------------------------------------------------
# sequences
# ---------------------------------------------------------------------------
def sphere(n, seed, tiles=(1, 2)):
    return em.structured_cloud(n, tiles=tiles, seed=seed)


def sequences():
    """name -> (frames, gop_size, exp_factor, octree_bits, jpeg_quality, entropy); 5 to 9 frames of 3 000 to 60 000 points."""
    out = {}
    rng = np.random.default_rng(77)
    base = sphere(30000, 1)
    out["static"] = ([base] * 6, 4, 1.25, 7, 85, False)
    frames = []
    for i in range(7):                                       # a tenth of the surface moves a little further each frame, and changes colour
        f = base.copy()
        cap = f['x'] > 0.8
        f['x'][cap] += np.float32(0.01 * i)
        f['g'][cap] = np.minimum(255, f['g'][cap].astype(np.int64) + 7 * i).astype(np.uint8)
        frames.append(f)
    out["part moved"] = (frames, 8, 1.25, 8, 85, True)
    frames = []
    for i in range(5):                                       # every point jitters: most leaves at 10 bits are new in every frame
        f = sphere(60000, 2).copy()
        for a in 'xyz':
            f[a] += rng.normal(0, 0.001, len(f)).astype(np.float32)
        frames.append(f)
    out["noise"] = (frames, 3, 1.5, 10, 60, True)
    frames = []
    for i in range(9):                                       # the cloud grows until it leaves the cube: a key inside the GOP
        f = sphere(8000, 3).copy()
        for a in 'xyz':
            f[a] *= np.float32(1.0 + 0.06 * i)
        frames.append(f)
    out["growing past the cube"] = (frames, 8, 1.25, 6, 30, False)
    small = cm.random_cloud(rng, 3000, 1.0)
    out["an empty frame"] = ([small, small[:2000], EMPTY, small, small[500:], small], 4, 1.1, 4, 85, False)
    uniform = sphere(20000, 4).copy()
    uniform['tile'] = 4
    mixed = sphere(20000, 4)
    out["tiles uniform, then mixed"] = ([uniform, uniform, mixed, mixed, uniform, mixed[:15000]], 8, 2.0, 7, 10, True)
    out["exp_factor 1, gop 2"] = ([small, small[:2500], small[100:], small, small[::2]], 2, 1.0, 9, 95, False)
    for frames, *_ in out.values():
        for f in frames:
            f.setflags(write=False)
    return out


_model = {}


def model(name):
    """(packets, the cwao packets they stand for, kinds) of the model encoder over a sequence."""
    if name not in _model:
        frames, gop, exp, bits, quality, entropy = sequences()[name]
        enc = im.Encoder(gop, exp, bits, quality, entropy)
        packets, plain = [], []
        for i, f in enumerate(frames):
            packets.append(enc.feed(f, 1000 + 33 * i))
            plain.append(enc.intra)
        _model[name] = (packets, plain, list(enc.kinds))
    return _model[name]


def new_encoder(codec, name, **kw):
    _, gop, exp, bits, quality, entropy = sequences()[name]
    return codec.cwipc_new_encoder(do_inter_frame=True, gop_size=gop, exp_factor=exp, octree_bits=bits, jpeg_quality=quality, entropy=entropy, **kw)


def run_encoder(codec, gpu, name, frames=None, boundaries=None):
    enc = new_encoder(codec, name)
    got = []
    for i, f in enumerate(frames if frames is not None else sequences()[name][0]):
        if boundaries is not None:
            boundaries.append(enc.at_gop_boundary())
        enc.feed(make_cloud(gpu, f, 0.0, 1000 + 33 * i))
        assert enc.available(True)
        got.append(bytes(enc.get_bytes()))
        assert not enc.available(False)
    if boundaries is not None:
        boundaries.append(enc.at_gop_boundary())
    enc.free()
    return got


NAMES = list(sequences())


def test_the_sequences_reach_every_path():
    kinds = {name: "".join("Kd"[k] for k in model(name)[2]) for name in NAMES}
    assert kinds["static"] == "KdddKd" and kinds["part moved"] == "Kdddddd" and kinds["noise"] == "KddKd"
    assert kinds["growing past the cube"].count("K") == 2 and kinds["growing past the cube"][:3] == "Kdd" and "dK" in kinds["growing past the cube"][:8]
    assert kinds["an empty frame"] == "KdKKdd" and kinds["exp_factor 1, gop 2"][0] == "K"
    seen = set()
    for name in NAMES:
        for p in model(name)[0]:
            info = im.parse(p)
            if info["kind"] == im.DELTA:
                seen |= {(s["kind"], s["mode"]) for s in info["streams"]}
                seen.add("nothing added" if info["nadded"] == 0 else "added")
    assert {("keep", 0), ("keep", 1), ("occupancy", 0), ("occupancy", 1), ("colour", 0), ("colour", 1), ("tile", 0), ("tile", 1), "nothing added", "added"} <= seen


@pytest.mark.parametrize("name", NAMES)
def test_encoder_delivers_the_model_packets(codec, gpu, name):
    packets, plain, kinds = model(name)
    boundaries = []
    got = run_encoder(codec, gpu, name, boundaries=boundaries)
    for i, (g, want) in enumerate(zip(got, packets)):
        assert g[:4] == b"cwap" and len(g) == len(want), (i, len(g), len(want))
        assert g == want, i
    # the key / delta pattern and at_gop_boundary(): true iff the next frame is a key whatever it holds
    gop = sequences()[name][1]
    g, have, want = 0, False, []
    for k, p in zip(kinds, plain):
        want.append(g == 0 or not have)
        g = 0 if k == im.KEY else g
        have = cm.parse(p)["nleaves"] > 0
        g = (g + 1) % gop
    want.append(g == 0 or not have)
    assert boundaries == want


def test_shuffled_points_give_the_same_bytes(codec, gpu):
    rng = np.random.default_rng(5)
    for name in ("part moved", "tiles uniform, then mixed"):
        frames = [f[rng.permutation(len(f))] for f in sequences()[name][0]]
        assert run_encoder(codec, gpu, name, frames) == model(name)[0]


def test_exp_factor_1_key_embeds_the_plain_encoders_packet(codec, gpu):
    name = "exp_factor 1, gop 2"
    frames, _, _, bits, quality, _ = sequences()[name]
    got = run_encoder(codec, gpu, name)
    plain = codec.cwipc_new_encoder(octree_bits=bits, jpeg_quality=quality)
    for i, (g, f) in enumerate(zip(got, frames)):
        if im.parse(g)["kind"] == im.KEY:
            plain.feed(make_cloud(gpu, f, 0.0, 1000 + 33 * i))
            assert g[im.PREFIX:] == bytes(plain.get_bytes()) == cm.encode(f, bits, quality, 1000 + 33 * i)
    plain.free()


def test_entropy_on_and_off(codec, gpu):
    """The same sequence both ways: the key packets embed the cwae or the cwao form, the delta packets are the same bytes."""
    name = "part moved"
    frames, gop, exp, bits, quality, _ = sequences()[name]
    enc = codec.cwipc_new_encoder(do_inter_frame=True, gop_size=gop, exp_factor=exp, octree_bits=bits, jpeg_quality=quality)
    packets, plain, _ = model(name)
    for i, f in enumerate(frames[:3]):
        enc.feed(make_cloud(gpu, f, 0.0, 1000 + 33 * i))
        got = bytes(enc.get_bytes())
        assert got == (im.key_packet(plain[0]) if i == 0 else packets[i])
    with pytest.raises(gpu.CwipcError):
        enc.set_entropy(True)
    enc.free()


def test_parameters(codec, gpu):
    for kw in (dict(do_inter_frame=True, gop_size=1, exp_factor=1.25), dict(do_inter_frame=True, gop_size=65536), dict(do_inter_frame=True, gop_size=4, exp_factor=0.5),
               dict(do_inter_frame=True, gop_size=4, exp_factor=17.0), dict(do_inter_frame=True, gop_size=4, exp_factor=float("nan")), dict(do_inter_frame=True)):
        with pytest.raises(gpu.CwipcError, match="do_inter_frame"):
            codec.cwipc_new_encoder(**kw)
    with pytest.raises(gpu.CwipcError, match="gop_size"):
        codec.cwipc_new_encoder(gop_size=4, exp_factor=1.25)
    group = codec.cwipc_new_encodergroup()
    with pytest.raises(gpu.CwipcError, match="do_inter_frame"):
        group.addencoder(do_inter_frame=True, gop_size=4, exp_factor=1.25)
    group.free()
    enc = codec.cwipc_new_encoder(do_inter_frame=True, gop_size=65535, exp_factor=16.0)
    assert enc.at_gop_boundary()
    enc.free()
    assert codec.cwipc_new_encoder().at_gop_boundary()


# ---------------------------------------------------------------------------
# decoder
# ---------------------------------------------------------------------------
def decoded(pc):
    return pc.get_numpy_array().tobytes()


@pytest.mark.parametrize("name", NAMES)
def test_decoder_hands_out_the_clouds_of_the_packets_they_stand_for(codec, gpu, name):
    packets, plain, _ = model(name)
    dec, ref = codec.cwipc_new_decoder(), codec.cwipc_new_decoder()
    for i, (p, q) in enumerate(zip(packets, plain)):
        dec.feed(p)
        ref.feed(q)
        assert dec.available(True) and ref.available(True)
        a, b = dec.get(), ref.get()
        want, ts, cell = cm.decode(q)
        assert a.timestamp() == b.timestamp() == ts and a.count() == len(want), i
        assert np.float32(a.cellsize()).tobytes() == np.float32(cell).tobytes()
        assert decoded(a) == decoded(b) == want.tobytes(), i
    dec.free()
    ref.free()


def test_model_pairs_of_every_shape_decode(codec, gpu):
    """The pairs of test_inter_model.py (7, 8, 9 and 32769 reference leaves, 4095 to 4097 leaves, one leaf, all tile combinations, 4 and
    8 colour bits): the key packet of R, then the delta."""
    dec = codec.cwipc_new_decoder()
    for name, (R, P) in pairs().items():
        dec.feed(im.key_packet(R))
        dec.feed(delta(name))
        assert dec.available(True)
        assert decoded(dec.get()) == cm.decode(R)[0].tobytes(), name
        assert dec.available(True)
        pc = dec.get()
        assert decoded(pc) == cm.decode(P)[0].tobytes() and pc.timestamp() == cm.parse(P)["timestamp"], name
    dec.free()


def test_a_dropped_delta_is_refused_until_the_next_key(codec, gpu):
    packets, plain, kinds = model("static")                  # K d d d K d
    dec = codec.cwipc_new_decoder()
    with pytest.raises(gpu.CwipcError, match="no reference"):
        dec.feed(packets[1])
    dec.feed(packets[0])
    for p in packets[2:4]:                                   # packets[1] never arrives
        with pytest.raises(gpu.CwipcError, match="reference held is not the one"):
            dec.feed(p)
    dec.feed(packets[1])                                     # the reference is still frame 0: the dropped packet, late, is taken
    dec.feed(packets[4])
    dec.feed(packets[5])
    for i in (0, 1, 4, 5):
        assert dec.available(True)
        assert decoded(dec.get()) == cm.decode(plain[i])[0].tobytes(), i
    assert not dec.available(False)
    dec.free()


def test_plain_packets_between_deltas_leave_the_reference_alone(codec, gpu):
    packets, plain, _ = model("part moved")
    other = cm.encode(cm.random_cloud(np.random.default_rng(3), 3000, 1.0), 6, 85, 5)
    dec = codec.cwipc_new_decoder()
    with gpu.cwipc_hip_profile() as prof:
        dec.feed(other)
        dec.feed(em.pack(other))
        assert dec.available(True)
    assert not any(name.startswith("inter_") for name in prof.kernels)      # nothing is kept of a plain packet
    assert decoded(dec.get()) == decoded(dec.get())
    for i in range(4):
        dec.feed(packets[i])
        dec.feed(other if i % 2 else em.pack(other))
    for i in range(4):
        assert dec.available(True)
        assert decoded(dec.get()) == cm.decode(plain[i])[0].tobytes(), i
        assert decoded(dec.get()) == cm.decode(other)[0].tobytes()
    dec.free()


def test_damaged_containers_launch_nothing(codec, gpu):
    """Only deltas that the host-side container test refuses are fed, with their reference held: the profiling counters, which see
    every launch of the library, stay empty, and the memory pool does not grow."""
    dll = gpu.util.cwipc_util_dll_load()
    dec = codec.cwipc_new_decoder()
    by_reference = {}
    for what, R, data in container_cases():
        if R:
            by_reference.setdefault(R, []).append((what, data))
    refused = 0
    for R, cases in by_reference.items():
        dec.feed(im.key_packet(R))
        assert dec.available(True)
        dec.get()
        dll.cwipc_hip_synchronize()
        pool = dll.cwipc_hip_pool_bytes()
        with gpu.cwipc_hip_profile() as prof:
            for what, data in cases:
                with pytest.raises(gpu.CwipcError) as err:
                    dec.feed(data)
                assert "cwipc_hip_decoder_feed" in str(err.value), what
                assert not dec.available(False)
                refused += 1
        assert prof.kernels == {} and dll.cwipc_hip_pool_bytes() == pool
    assert refused > 400
    dec.free()


def test_damaged_payloads_are_refused_at_feed_and_the_reference_stays(codec, gpu):
    """The payload damages that the sanitised host program has applied in bounds (test_inter_host.py, on these very packets): the
    container test lets them through, the check inside feed refuses them, none of the point-making kernels runs, and the delta itself
    is still taken afterwards."""
    dec = codec.cwipc_new_decoder()
    reasons = set()
    for name in ("random", "nleaves 4097", "cb 4, coded", "nR 32769", "still"):
        R, P = pairs()[name]
        cases = [(what, data) for what, ref, data in payload_cases() if ref is R and what.startswith(name + ":")]
        assert cases
        dec.feed(im.key_packet(R))
        assert dec.available(True)
        dec.get()
        with gpu.cwipc_hip_profile() as prof:
            for what, data in cases:
                with pytest.raises(gpu.CwipcError) as err:
                    dec.feed(data)
                assert "cwipc_hip_decoder_feed" in str(err.value), what
                reasons |= {r for r in ("not intact", "padding bits", "leaf count", "leaf of the reference") if r in str(err.value)}
                assert not dec.available(False)
        assert "inter_status" in prof.kernels and not {"inter_merge", "inter_rebuild", "codec_points"} & set(prof.kernels), name
        dec.feed(delta(name))
        assert dec.available(True)
        assert decoded(dec.get()) == cm.decode(P)[0].tobytes(), name
    assert reasons == {"not intact", "padding bits", "leaf count", "leaf of the reference"}
    dec.free()


# ---------------------------------------------------------------------------
# threads, host functions
# ---------------------------------------------------------------------------
def test_encoder_and_decoder_fed_from_two_threads_in_turn(codec, gpu):
    name = "part moved"
    frames = sequences()[name][0]
    packets, plain, _ = model(name)
    enc, dec = new_encoder(codec, name), codec.cwipc_new_decoder()
    got, clouds, errors = [], [], []
    turn = [threading.Semaphore(1), threading.Semaphore(0)]

    def worker(me):
        try:
            gpu.cwipc_hip_set_device(0)
            for i in range(me, len(frames), 2):
                turn[me].acquire()
                enc.feed(make_cloud(gpu, frames[i], 0.0, 1000 + 33 * i))
                packet = bytes(enc.get_bytes())
                dec.feed(packet)
                assert dec.available(True)
                got.append(packet)
                clouds.append(decoded(dec.get()))
                turn[1 - me].release()
        except Exception as e:                               # noqa: BLE001 (handed to the main thread)
            errors.append(e)
            turn[1 - me].release()

    threads = [threading.Thread(target=worker, args=(me,)) for me in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert got == packets
    assert clouds == [cm.decode(q)[0].tobytes() for q in plain]
    enc.free()
    dec.free()


def test_host_functions_against_encoder_output(codec, gpu):
    name = "tiles uniform, then mixed"
    got = run_encoder(codec, gpu, name)
    _, plain, kinds = model(name)
    held = None
    for i, (g, q, k) in enumerate(zip(got, plain, kinds)):
        info = codec.inter_info(g)
        assert info["kind"] == ("key" if k == im.KEY else "delta") and info["total_bytes"] == len(g) and info["timestamp"] == 1000 + 33 * i
        out = bytes(codec.inter_unpack(held, g))
        if k == im.KEY:
            out = bytes(codec.entropy_unpack(out))
        else:
            assert bytes(codec.inter_pack(held, q, info["gop_index"])) == g
            assert info["ref_timestamp"] == 1000 + 33 * (i - 1) and info["nleaves"] == cm.parse(q)["nleaves"]
        assert out == q, i
        held = out


# ---------------------------------------------------------------------------
# pipeline
# ---------------------------------------------------------------------------
def test_sequence_rate(codec, gpu):
    from cwipc_util_amd import quality
    for name in ("static", "part moved"):
        frames, gop, exp, bits, q, entropy = sequences()[name]
        packets, plain, kinds = model(name)
        rows = quality.sequence_rate([make_cloud(gpu, f, 0.0, 1000 + 33 * i) for i, f in enumerate(frames)], entropy=entropy, do_inter_frame=True, gop_size=gop,
                                     exp_factor=exp, octree_bits=bits, jpeg_quality=q)
        assert [r["kind"] for r in rows] == ["key" if k == im.KEY else "delta" for k in kinds]
        assert [r["bytes"] for r in rows] == [len(p) for p in packets]
        assert [r["intra_bytes"] for r in rows] == [len(em.pack(p)) if entropy else len(p) for p in plain]
        assert all(r["bytes"] < r["intra_bytes"] for r in rows if r["kind"] == "delta")


def test_quality_script_with_gop(codec, gpu):
    from cwipc_util_amd.scripts import cwipc_codec_quality as script
    args = script.build_parser().parse_args(["--synthetic", "20000", "--gop", "3", "--octree_bits", "7", "--frames", "5", "--entropy"])
    table = script.CodecQualityTable(args)
    table.load_input(None, args.synthetic)
    table.run()
    kinds = [r["kind"] for r in table.rows]                 # (the source turns: a frame may leave the cube and force a key)
    assert len(kinds) == 5 and kinds[0] == "key" and "delta" in kinds and "kkk" not in "".join(k[0] for k in kinds)
    lines = table.table().splitlines()
    assert lines[0].split() == list(script.GOP_COLUMNS) and len(lines) == 6 and [line.split()[1] for line in lines[1:]] == kinds


def test_pipeline_sink_encoder_with_gop_to_source_decoder(codec, gpu, capsys):
    """Two tiles, inter-frame coded by lone encoders, into lists and back through source decoders; then a stream that has lost a delta:
    the deltas behind the gap are logged and skipped, the next key packet recovers."""
    from cwipc_util_amd.capture import TileSource, capture_tile
    from cwipc_util_amd.net.sink_encoder import cwipc_sink_encoder
    from cwipc_util_amd.net.source_decoder import cwipc_source_decoder
    tiles = [capture_tile(6000, t, 2) for t in range(2)]
    host_tiles = [t.get_numpy_array() for t in tiles]
    sources = [TileSource(t, 5, first_timestamp=100, timestamp_step=33) for t in tiles]
    streams = []
    sink = cwipc_sink_encoder(streams, nodrop=True)
    sink.set_encoder_params([dict(cameraMask=1), dict(cameraMask=2)], octree_bits=8, jpeg_quality=60, entropy=True, gop_size=3)
    for _ in range(5):
        sink.feed(gpu.cwipc_join(sources[0].get(), sources[1].get()))
    assert [len(s) for s in streams] == [5, 5]
    want, plain = [], []
    for i in range(2):
        enc = im.Encoder(3, 1.25, 8, 60, entropy=True)
        want.append([])
        plain.append([])
        for f in range(5):
            want[i].append(enc.feed(host_tiles[i], 100 + 33 * f))
            plain[i].append(enc.intra)
        assert enc.kinds == [im.KEY, im.DELTA, im.DELTA, im.KEY, im.DELTA]
    assert [[bytes(p) for p in s] for s in streams] == want
    source = cwipc_source_decoder(list(streams[0]))
    for f in range(5):
        pc = source.get()
        assert pc is not None and pc.timestamp() == 100 + 33 * f and decoded(pc) == cm.decode(plain[0][f])[0].tobytes()
    assert source.eof() and source.skipped == 0
    source.free()
    capsys.readouterr()
    lossy = cwipc_source_decoder([p for f, p in enumerate(streams[1]) if f != 1])      # K . d K d
    got = []
    while not lossy.eof():
        pc = lossy.get()
        if pc is not None:
            got.append(pc.timestamp())
    assert got == [100, 100 + 33 * 3, 100 + 33 * 4] and lossy.skipped == 1
    assert "delta packet skipped" in capsys.readouterr().out
    lossy.free()
    sink.free()


def test_nothing_is_left_behind(codec, gpu, clouds_before):
    """Last in the file: every cloud the tests above made has been freed with its wrapper."""
    gc.collect()
    assert gpu.cwipc_dangling_allocations(False) == clouds_before
