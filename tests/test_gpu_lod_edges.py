"""Level-of-detail decoding on the GPU (RULE L; csrc/kernels_lod.hip) over the trees of tests/tree_cases.py: runs of CHOSEN lengths
(1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 4096, one of 70 000) that start at a workgroup's first lane, at a wave's first and last
lane and in mid-wave, runs of one only, exact halves of the mean, a tile bit that a single leaf in another wave carries, every colour
width with the last leaf across two colour words, trees whose first-child scan runs past one round, cuts to 1, b - 1, b and b + 1.
A decoder with set_max_octree_bits(t) must hand out cm.decode(lm.lod(P, t)) for P as "cwao", as "cwae", as "cwat" (the packed 8-bit
path with the transform's first children) and inside a "cwap" key packet (the runs come from the leaves' keys); codec.lod must give
the model's packet.  Key and delta chains of tests/inter_cases.py, the ones past 65 536 leaves among them, are decoded with a limit to
their end.  Bytes only; there is no tolerance in this file (test_tree_cases.py has held the model to the cases)."""
import gc

import numpy as np
import pytest

import codec_model as cm
import entropy_model as em
import inter_cases
import inter_model as im
import lod_model as lm
import transform_model as tm
from tree_cases import BIG, BIG_RUN, SMALL, cases, lod_runs

pytestmark = pytest.mark.gpu

RUNS = lod_runs()
IDS = [f"{name}, cut to {t}" for name, t in RUNS]
FORMS = ("cwao", "cwae", "cwat", "cwap key")
_ran = {"decoder": [], "host": []}
_cuts, _forms = {}, {}


@pytest.fixture(scope="module")
def codec(gpu):
    import cwipc_util_amd.codec as codec
    return codec


@pytest.fixture(scope="module", autouse=True)
def clouds_before(gpu):
    gc.collect()
    return gpu.cwipc_dangling_allocations(False)


def cut_of(plain, t):
    """(L(P, min(t, b)), its cloud), computed once per (packet, t) and left unchanged."""
    plain = bytes(plain)
    t = min(t, cm.parse(plain)["octree_bits"])
    if (plain, t) not in _cuts:
        L = lm.lod(plain, t)
        _cuts[(plain, t)] = (L, cm.decode(L))
    return _cuts[(plain, t)]


def forms_of(name):
    """{form: the packet that stands for the case's P}"""
    if name not in _forms:
        case = cases()[name]
        P = case.packet
        out = {"cwao": P, "cwae": em.pack(P), "cwap key": im.key_packet(P)}
        if case.colour_bits == 8:
            out["cwat"] = tm.pack(P, 100)
        _forms[name] = out
    return _forms[name]


def same_cloud(pc, want, what=None):
    points, ts, cell = want
    assert pc is not None and pc.count() == len(points) and pc.timestamp() == ts, what
    assert np.float32(pc.cellsize()).tobytes() == np.float32(cell).tobytes(), what
    got = pc.get_numpy_array()
    for f in ("x", "y", "z", "r", "g", "b", "tile"):
        assert got[f].tobytes() == points[f].tobytes(), (what, f)
    assert got.tobytes() == points.tobytes(), what


def fed(dec, packet):
    dec.feed(packet)
    assert dec.available(True)
    pc = dec.get()
    assert pc is not None and not dec.available(False)
    return pc


# ---------------------------------------------------------------------------
# every case at every cut of its own
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,t", RUNS, ids=IDS)
def test_decoder_hands_out_the_cut_of_every_form(codec, gpu, name, t):
    _ran["decoder"].append((name, t))
    want = cut_of(cases()[name].packet, t)[1]
    for form, packet in forms_of(name).items():
        dec = codec.cwipc_new_decoder(max_octree_bits=t)         # (a key packet leaves a reference behind: a decoder a form)
        same_cloud(fed(dec, packet), want, form)
        dec.free()


@pytest.mark.parametrize("name,t", RUNS, ids=IDS)
def test_host_function_gives_the_models_packet(codec, gpu, name, t):
    _ran["host"].append((name, t))
    case = cases()[name]
    if t > case.octree_bits:
        with pytest.raises(gpu.CwipcError, match="octree bits of the cut"):
            codec.lod(case.packet, t)
        return
    L = cut_of(case.packet, t)[0]
    assert bytes(codec.lod(case.packet, t)) == L
    assert bytes(codec.lod(forms_of(name)["cwae"], t)) == em.pack(L)


def test_every_cut_of_the_table_ran():
    assert _ran["decoder"] == _ran["host"] == lod_runs()
    assert all(set(forms_of(name)) == set(FORMS) - ({"cwat"} if cases()[name].colour_bits != 8 else set()) for name, _ in RUNS)


# ---------------------------------------------------------------------------
# key and delta chains
# ---------------------------------------------------------------------------
def chains():
    """The streams of inter_cases that have a frame past 65 536 leaves, and three small ones."""
    return [name for name in inter_cases.cases() if name.startswith("two scan rounds")] + [inter_cases.TINY, inter_cases.MID, "tiles"]


@pytest.mark.parametrize("limit", ["1", "b - 1"])
@pytest.mark.parametrize("name", chains())
def test_chains_decoded_with_a_limit_validate_to_their_end(codec, gpu, name, limit):
    case = inter_cases.cases()[name]
    packets, intra, kinds = case.model()
    t = 1 if limit == "1" else case.octree_bits - 1
    if name.startswith("two scan rounds"):
        assert max(cm.parse(q)["nleaves"] for q in intra) > 65536
    dec = codec.cwipc_new_decoder(max_octree_bits=t)
    for i, (p, q) in enumerate(zip(packets, intra)):
        same_cloud(fed(dec, p), cut_of(q, t)[1], i)               # (a delta after a cut frame is accepted: the reference is the full frame)
    assert "d" in kinds and i == len(packets) - 1
    dec.free()


# ---------------------------------------------------------------------------
# a stream of calls
# ---------------------------------------------------------------------------
def test_cuts_queued_and_the_limit_changed_between_feeds(codec, gpu):
    name = "runs: b - t = 3, ascending"
    P, b = cases()[name].packet, cases()[name].octree_bits
    dec = codec.cwipc_new_decoder()
    order = [(3, "cwao"), (1, "cwat"), (None, "cwae"), (b - 1, "cwae"), (3, "cwat")]
    for t, form in order:
        dec.set_max_octree_bits(t)
        dec.feed(forms_of(name)[form])
    for t, form in order:
        assert dec.available(True)
        same_cloud(dec.get(), cut_of(P, b if t is None else t)[1], (t, form))
    assert not dec.available(False)
    dec.free()


def test_every_small_case_again_after_the_large_ones(codec, gpu):
    """The 70 000-leaf trees have been through this process by now (and go through once more here): the pool's blocks have held their
    sums, starts and scan words.  Every small case gives its clouds again through one decoder a form, and a second pass takes no more
    memory than the first."""
    dll = gpu.util.cwipc_util_dll_load()
    decs = {form: codec.cwipc_new_decoder() for form in FORMS}
    for name in (BIG, BIG_RUN):
        for t in cases()[name].cuts[:2]:
            for form, packet in forms_of(name).items():
                decs[form].set_max_octree_bits(t)
                same_cloud(fed(decs[form], packet), cut_of(cases()[name].packet, t)[1], (name, t, form))
    pool = []
    for _ in range(2):
        for name in SMALL:
            case = cases()[name]
            for t in case.cuts[:1]:
                for form, packet in forms_of(name).items():
                    decs[form].set_max_octree_bits(t)
                    same_cloud(fed(decs[form], packet), cut_of(case.packet, t)[1], (name, t, form))
        dll.cwipc_hip_synchronize()
        pool.append(dll.cwipc_hip_pool_bytes())
    for dec in decs.values():
        dec.free()
    assert pool[0] == pool[1]


def test_nothing_is_left_behind(codec, gpu, clouds_before):
    """Last in the file: every cloud the tests above made has been freed with its wrapper."""
    gc.collect()
    assert gpu.cwipc_dangling_allocations(False) == clouds_before
