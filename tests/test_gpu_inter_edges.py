"""Inter-frame coding on the GPU (RULE P; csrc/kernels_inter.hip) over the streams of tests/inter_cases.py: CHOSEN leaf sets, leaf
counts at the wave, the workgroup and the keep byte, scans past one round, the bounds grid past its cap, trees of 1 to 16 bits, every
colour depth, crowded leaves, non-finite points, points on the cube's faces -- each through the encoder, the decoder and the host
functions, all held to the numpy model's bytes (test_inter_cases.py has held the model to the cases).  Then what a stream of calls
adds: another point order, several frames queued before the first packet is taken, two streams fed in turn on one thread, a case
given again after large ones have used the pool's blocks.  Bytes only; there is no tolerance in this file."""
import gc

import numpy as np
import pytest

import codec_model as cm
import inter_model as im
from conftest import make_cloud
from inter_cases import BIG, CROWDED, EXP_FACTOR, MID, QUEUED, TINY, cases, timestamp

pytestmark = pytest.mark.gpu

NAMES = list(cases())
_ran = {"encoder": [], "decoder": [], "host": []}
_encoded = {}


@pytest.fixture(scope="module")
def codec(gpu):
    import cwipc_util_amd.codec as codec
    return codec


@pytest.fixture(scope="module", autouse=True)
def clouds_before(gpu):
    gc.collect()
    return gpu.cwipc_dangling_allocations(False)


def new_encoder(codec, case):
    return codec.cwipc_new_encoder(do_inter_frame=True, gop_size=case.gop_size, exp_factor=EXP_FACTOR, octree_bits=case.octree_bits, jpeg_quality=case.jpeg_quality,
                                   entropy=case.entropy)


def run_encoder(codec, gpu, case, stream=None, boundaries=None):
    """The packets of an encoder over the stream, each taken right after its feed."""
    enc = new_encoder(codec, case)
    got = []
    for i, f in enumerate(case.stream() if stream is None else stream):
        if boundaries is not None:
            boundaries.append(enc.at_gop_boundary())
        enc.feed(make_cloud(gpu, f, 0.0, timestamp(i)))
        assert enc.available(True)
        got.append(bytes(enc.get_bytes()))
        assert not enc.available(False)
    if boundaries is not None:
        boundaries.append(enc.at_gop_boundary())
    enc.free()
    return got


def same_packets(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g[:4] == b"cwap" and len(g) == len(w), (i, len(g), len(w))
        assert g == w, i


def encoded(codec, gpu, name):
    """The encoder's packets of a case, made once."""
    if name not in _encoded:
        _encoded[name] = run_encoder(codec, gpu, cases()[name])
    return _encoded[name]


def decoded(pc):
    return pc.get_numpy_array().tobytes()


def same_cloud(pc, packet, what):
    want, ts, cell = cm.decode(packet)
    assert pc.timestamp() == ts and pc.count() == len(want), what
    assert np.float32(pc.cellsize()).tobytes() == np.float32(cell).tobytes(), what
    assert decoded(pc) == want.tobytes(), what


# ---------------------------------------------------------------------------
# every case: encoder, decoder, host functions
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_encoder_delivers_the_model_packets(codec, gpu, name):
    _ran["encoder"].append(name)
    case = cases()[name]
    boundaries = []
    got = run_encoder(codec, gpu, case, boundaries=boundaries)
    same_packets(got, case.model()[0])
    assert boundaries == case.boundaries()
    _encoded[name] = got


@pytest.mark.parametrize("name", NAMES)
def test_decoder_hands_out_the_clouds_of_the_intra_packets(codec, gpu, name):
    _ran["decoder"].append(name)
    packets, intra, _ = cases()[name].model()
    dec, plain = codec.cwipc_new_decoder(), codec.cwipc_new_decoder()
    for i, (p, q) in enumerate(zip(packets, intra)):
        dec.feed(p)
        plain.feed(q)
        assert dec.available(True) and plain.available(True)
        a, b = dec.get(), plain.get()
        same_cloud(a, q, i)
        same_cloud(b, q, i)
        assert not dec.available(False)
    dec.free()
    plain.free()


@pytest.mark.parametrize("name", NAMES)
def test_host_functions_against_the_encoders_deltas(codec, gpu, name):
    _ran["host"].append(name)
    case = cases()[name]
    _, intra, kinds = case.model()
    got, indices = encoded(codec, gpu, name), case.gop_indices()
    for i in range(1, len(got)):
        info = codec.inter_info(got[i])
        assert info["kind"] == ("key" if kinds[i] == "K" else "delta") and info["total_bytes"] == len(got[i]) and info["timestamp"] == timestamp(i), i
        if kinds[i] == "K":
            continue
        R, P, want = intra[i - 1], intra[i], im.parse(got[i])
        assert bytes(codec.inter_pack(R, P, indices[i])) == got[i], i
        assert bytes(codec.inter_unpack(R, got[i])) == P, i
        assert (info["nadded"], info["nleaves"], info["ref_timestamp"], info["gop_index"]) == (want["nadded"], want["nleaves"], timestamp(i - 1), indices[i]), i
        assert (info["ref_nleaves"], info["nodes_added"]) == (want["ref_nleaves"], want["nodes_added"]), i
        assert info["streams"] == [(s["mode"], s["bytes"]) for s in want["streams"]], i


def test_every_case_of_the_table_ran():
    assert _ran["encoder"] == _ran["decoder"] == _ran["host"] == list(cases())


# ---------------------------------------------------------------------------
# a stream of calls
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", CROWDED)
def test_another_point_order_gives_the_same_bytes(codec, gpu, name):
    case = cases()[name]
    rng = np.random.default_rng(5)
    stream = [f[rng.permutation(len(f))] for f in case.stream()]
    same_packets(run_encoder(codec, gpu, case, stream), case.model()[0])


@pytest.mark.parametrize("name", QUEUED)
def test_frames_queued_before_the_first_packet_is_taken(codec, gpu, name):
    case = cases()[name]
    packets, intra, _ = case.model()
    enc = new_encoder(codec, case)
    for i, f in enumerate(case.stream()):
        enc.feed(make_cloud(gpu, f, 0.0, timestamp(i)))
    got = []
    for _ in packets:
        assert enc.available(True)
        got.append(bytes(enc.get_bytes()))
    assert not enc.available(False)
    enc.free()
    same_packets(got, packets)
    assert got == encoded(codec, gpu, name)
    dec = codec.cwipc_new_decoder()
    for p in packets:
        dec.feed(p)
    for i, q in enumerate(intra):
        assert dec.available(True)
        same_cloud(dec.get(), q, i)
    assert not dec.available(False)
    dec.free()


@pytest.mark.parametrize("order", [(BIG, TINY), (TINY, BIG)])
def test_two_streams_in_turn_on_one_thread(codec, gpu, order):
    """Two encoders and two decoders that differ in bits, colour depth and leaf counts (65 793 leaves against a few dozen), each
    frame of the one between two frames of the other: both feeds are made before either packet is taken."""
    these = [cases()[name] for name in order]
    encs, decs = [new_encoder(codec, c) for c in these], [codec.cwipc_new_decoder() for _ in these]
    streams, models = [c.stream() for c in these], [c.model() for c in these]
    got, clouds = [[], []], [[], []]
    for i in range(max(len(s) for s in streams)):
        live = [k for k in range(2) if i < len(streams[k])]
        for k in live:
            encs[k].feed(make_cloud(gpu, streams[k][i], 0.0, timestamp(i)))
        for k in live:
            assert encs[k].available(True)
            got[k].append(bytes(encs[k].get_bytes()))
        for k in live:
            decs[k].feed(got[k][i])
        for k in live:
            assert decs[k].available(True)
            clouds[k].append(decoded(decs[k].get()))
    for k in range(2):
        same_packets(got[k], models[k][0])
        assert clouds[k] == [cm.decode(q)[0].tobytes() for q in models[k][1]], order[k]
        assert not encs[k].available(False) and not decs[k].available(False)
        encs[k].free()
        decs[k].free()


def test_a_case_given_again_after_the_large_ones(codec, gpu):
    """The 65 793-leaf and the 140 000-point streams have been through this process by now (and go through once more here): the
    pool's blocks have held other frames.  A mid-sized case gives its bytes again, and a second pass takes no more memory than the first."""
    dll = gpu.util.cwipc_util_dll_load()
    for name in (BIG, "wide frame"):
        same_packets(run_encoder(codec, gpu, cases()[name]), cases()[name].model()[0])
    case = cases()[MID]
    pool = []
    for _ in range(2):
        same_packets(run_encoder(codec, gpu, case), case.model()[0])
        dll.cwipc_hip_synchronize()
        pool.append(dll.cwipc_hip_pool_bytes())
    assert pool[0] == pool[1]


def test_nothing_is_left_behind(codec, gpu, clouds_before):
    """Last in the file: every cloud the tests above made has been freed with its wrapper."""
    gc.collect()
    assert gpu.cwipc_dangling_allocations(False) == clouds_before
