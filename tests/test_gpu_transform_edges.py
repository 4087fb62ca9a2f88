"""Transform colour coding on the GPU (RULE T; csrc/kernels_transform.hip) over the trees of tests/tree_cases.py: CHOSEN leaf keys,
leaf, coefficient and inner-node counts at the workgroup and the coded-stream threshold, scans past one round (the first-child scan
and the escape scan, each alone and both), depths of 255, 256 and 257 nodes, trees of 1 to 16 bits, butterflies of large equal, very
unequal and 1-and-2 weights, the largest coefficients, the token/escape border, whole blocks of escapes, every quality's branch,
uniform and mixed tiles -- each through the encoder, the decoder and the host functions, all held to the numpy model's bytes
(test_tree_cases.py has held the model to the cases).  Hostile but valid packets, which the model and the sanitised host program
(test_transform_host.py) answer in bounds, go to the decoder alone.  Then what a stream of calls adds: another point order, frames
queued before the first packet is taken, a transform encoder and a level-of-detail decoder in turn on one thread, every small case again
after the large ones have used the pool's blocks.  Bytes only; there is no tolerance in this file."""
import gc

import numpy as np
import pytest

import codec_model as cm
import lod_model as lm
import transform_model as tm
from conftest import make_cloud
from tree_cases import BIG, SMALL, TIMESTAMP, cases, hostile, transform_runs

pytestmark = pytest.mark.gpu

RUNS = transform_runs()
IDS = [f"{name}, quality {q}" for name, q in RUNS]
_ran = {"encoder": [], "decoder": [], "host": []}
_models = {}


@pytest.fixture(scope="module")
def codec(gpu):
    import cwipc_util_amd.codec as codec
    return codec


@pytest.fixture(scope="module", autouse=True)
def clouds_before(gpu):
    gc.collect()
    return gpu.cwipc_dangling_allocations(False)


def model(name, q):
    """(T, the cloud of its unpacked packet): tm.pack and cm.decode(tm.unpack) of the case at quality q, made once and left unchanged."""
    if (name, q) not in _models:
        T = tm.pack(cases()[name].packet, q)
        _models[(name, q)] = (T, tm.unpack(T))
    return _models[(name, q)]


def encode(codec, gpu, case, q, pts=None):
    enc = codec.cwipc_new_encoder(octree_bits=case.octree_bits, jpeg_quality=q, colour_transform=True)
    enc.feed(make_cloud(gpu, case.cloud if pts is None else pts, 0.0, TIMESTAMP))
    assert enc.available(True)
    data = bytes(enc.get_bytes())
    assert not enc.available(False)
    enc.free()
    return data


def same_cloud(pc, packet, what=None):
    want, ts, cell = cm.decode(packet)
    assert pc is not None and pc.count() == len(want) and pc.timestamp() == ts, what
    assert np.float32(pc.cellsize()).tobytes() == np.float32(cell).tobytes(), what
    assert pc.get_numpy_array().tobytes() == want.tobytes(), what


def fed(dec, packet):
    dec.feed(packet)
    assert dec.available(True)
    pc = dec.get()
    assert pc is not None and not dec.available(False)
    return pc


# ---------------------------------------------------------------------------
# every case at every quality of its own: encoder, decoder, host functions
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,q", RUNS, ids=IDS)
def test_encoder_delivers_the_model_packet(codec, gpu, name, q):
    _ran["encoder"].append((name, q))
    T = model(name, q)[0]
    got = encode(codec, gpu, cases()[name], q)
    assert got[:4] == b"cwat" and len(got) == len(T)
    assert got == T


@pytest.mark.parametrize("name,q", RUNS, ids=IDS)
def test_decoder_hands_out_the_unpacked_packets_cloud(codec, gpu, name, q):
    _ran["decoder"].append((name, q))
    T, unpacked = model(name, q)
    dec = codec.cwipc_new_decoder()
    same_cloud(fed(dec, T), unpacked)
    dec.free()
    if q == 100:
        assert unpacked == cases()[name].packet


@pytest.mark.parametrize("name,q", RUNS, ids=IDS)
def test_host_functions_agree_with_the_model(codec, gpu, name, q):
    _ran["host"].append((name, q))
    T, unpacked = model(name, q)
    assert bytes(codec.transform_pack(cases()[name].packet, q)) == T
    assert bytes(codec.transform_unpack(T)) == unpacked
    info, want = codec.transform_info(T), tm.parse(T)
    assert (info["q16"], info["dc"], info["nescapes"], info["nleaves"]) == (want["q16"], want["dc"], want["nescapes"], want["nleaves"])
    assert info["streams"] == [(s["mode"], s["bytes"]) for s in want["streams"]]
    assert info["kinds"] == [(s["kind"], s["which"], s["symbols"]) for s in want["streams"]]
    assert info["total_bytes"] == len(T) and info["colour_bytes"] == tm.colour_payload_bytes(T)


def test_every_run_of_the_table_ran():
    assert _ran["encoder"] == _ran["decoder"] == _ran["host"] == transform_runs()


# ---------------------------------------------------------------------------
# hostile but valid packets: the decoder alone
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(hostile()))
def test_hostile_packets_decode_to_the_models_clamped_cloud(codec, gpu, name):
    T = hostile()[name]
    tm.parse(T)                                          # the container test lets it through
    unpacked = tm.unpack(T)                              # and the model answers it
    assert bytes(codec.transform_unpack(T)) == unpacked
    dec = codec.cwipc_new_decoder()
    same_cloud(fed(dec, T), unpacked)
    good = model("counts: 9 leaves", 100)
    same_cloud(fed(dec, good[0]), good[1])               # the decoder is as usable as before
    dec.free()


# ---------------------------------------------------------------------------
# a stream of calls
# ---------------------------------------------------------------------------
SHUFFLED = ("counts: 4097 leaves", "depths: 257 chains", "weights: 1 against 4096", "values: a block of 256 escapes, then none", BIG)


@pytest.mark.parametrize("name", SHUFFLED)
def test_another_point_order_gives_the_same_bytes(codec, gpu, name):
    case = cases()[name]
    q = case.qualities[-1]
    pts = case.cloud[np.random.default_rng(5).permutation(len(case.cloud))]
    assert encode(codec, gpu, case, q, pts) == model(name, q)[0]


QUEUED = ("counts: 4097 leaves", "counts: 3 leaves", "counts: 257 leaves")          # all of 9 bits: coded and raw streams, one and many blocks


def test_three_frames_queued_before_the_first_packet_is_taken(codec, gpu):
    """Three trees that differ in leaf count and stream modes through one encoder, then their packets through one decoder."""
    enc = codec.cwipc_new_encoder(octree_bits=9, jpeg_quality=100, colour_transform=True)
    for name in QUEUED:
        enc.feed(make_cloud(gpu, cases()[name].cloud, 0.0, TIMESTAMP))
    got = []
    for _ in QUEUED:
        assert enc.available(True)
        got.append(bytes(enc.get_bytes()))
    assert not enc.available(False)
    enc.free()
    assert got == [model(name, 100)[0] for name in QUEUED]
    dec = codec.cwipc_new_decoder()
    for name in QUEUED:
        dec.feed(model(name, 100)[0])
    for name in QUEUED:
        assert dec.available(True)
        same_cloud(dec.get(), model(name, 100)[1], name)
    assert not dec.available(False)
    dec.free()


def test_a_transform_encoder_and_a_lod_decoder_in_turn(codec, gpu):
    """On one thread: each packet of the encoder goes to a decoder that hands out 3 bits at the most, while the next cloud is already
    fed; the decoder's clouds are the cuts of the unpacked packets."""
    names = ["tiles: mixed", "tiles: uniform", "counts: 4097 leaves", "quality: 5000 smooth leaves"]           # all of 9 bits
    enc = codec.cwipc_new_encoder(octree_bits=9, jpeg_quality=50, colour_transform=True)
    dec = codec.cwipc_new_decoder(max_octree_bits=3)
    enc.feed(make_cloud(gpu, cases()[names[0]].cloud, 0.0, TIMESTAMP))
    for i, name in enumerate(names):
        if i + 1 < len(names):
            enc.feed(make_cloud(gpu, cases()[names[i + 1]].cloud, 0.0, TIMESTAMP))
        assert enc.available(True)
        T = bytes(enc.get_bytes())
        want = tm.pack(cases()[name].packet, 50)
        assert T == want
        same_cloud(fed(dec, T), lm.lod(tm.unpack(want), 3), name)
    enc.free()
    dec.free()


def test_every_small_case_again_after_the_large_ones(codec, gpu):
    """The 70 000-leaf trees have been through this process by now (and the largest goes through once more here): the pool's blocks
    have held their sums, escapes, zigzag values and scan words.  Every small case gives its bytes and its cloud again, and a second
    pass takes no more memory than the first."""
    dll = gpu.util.cwipc_util_dll_load()
    assert encode(codec, gpu, cases()[BIG], 100) == model(BIG, 100)[0]
    dec = codec.cwipc_new_decoder()
    same_cloud(fed(dec, model(BIG, 100)[0]), model(BIG, 100)[1])
    pool = []
    for _ in range(2):
        for name in SMALL:
            case = cases()[name]
            if not case.qualities:
                continue
            q = case.qualities[-1]
            T, unpacked = model(name, q)
            assert encode(codec, gpu, case, q) == T, name
            same_cloud(fed(dec, T), unpacked, name)
        dll.cwipc_hip_synchronize()
        pool.append(dll.cwipc_hip_pool_bytes())
    dec.free()
    assert pool[0] == pool[1]


def test_nothing_is_left_behind(codec, gpu, clouds_before):
    """Last in the file: every cloud the tests above made has been freed with its wrapper."""
    gc.collect()
    assert gpu.cwipc_dangling_allocations(False) == clouds_before
