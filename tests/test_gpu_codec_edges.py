"""The octree codec on the GPU where a uniform random cloud does not reach: points within a float32 ulp of every cell boundary, the
edges of float32, more points than one pass of the bounds kernel covers, valid packets that no encoder makes, groups whose members come
and go, and results collected on another thread than the one that fed.  The discipline is test_gpu_codec.py's, whose helpers are used:
encoder == model and decoder == model (tests/codec_model.py) as bytes, no tolerance anywhere.  The inputs are made once and shared
with the CPU tests (test_codec_model.py: the boundary clouds; test_codec_packet_host.py: the edge clouds, the hand-built packets), which
hold the same inputs to the host build of codec_terms.hpp and show that they tell the rule from its near misses.  Every packet fed to
the decoder here is valid by the model's parse()."""
import gc
import threading
import time

import numpy as np
import pytest

import codec_model as cm
from conftest import make_cloud
from test_codec_model import BOUNDARY_CUBES, boundary_cloud
from test_codec_packet_host import BIG_TIMESTAMP, EDGE_BITS, edge_clouds, hand_built_packets
from test_gpu_codec import check, check_decodes_to_model, encode

pytestmark = pytest.mark.gpu

LINE = 131072          # 512 workgroups of 256 points: what one pass of codec_bounds_kernel covers


@pytest.fixture(scope="module")
def codec(gpu):
    import cwipc_util_amd.codec as codec
    return codec


@pytest.fixture(scope="module", autouse=True)
def clouds_before(gpu):
    """What other test files of the same run still hold when this one starts."""
    gc.collect()
    return gpu.cwipc_dangling_allocations(False)


# ---------------------------------------------------------------------------
# cell boundaries
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [1, 4, 9, 16])
@pytest.mark.parametrize("cube", range(len(BOUNDARY_CUBES)))
def test_cell_boundaries(codec, gpu, cube, bits):
    packet = check(codec, gpu, boundary_cloud(cube, bits), bits, 85)
    info = cm.parse(packet)
    lo, hi = BOUNDARY_CUBES[cube]
    assert info["min"].tolist() == [np.float32(lo)] * 3 and info["side"] == float(np.float64(np.float32(hi)) - np.float64(np.float32(lo)))


@pytest.mark.parametrize("cube", range(len(BOUNDARY_CUBES)))
def test_cell_boundaries_in_a_group(codec, gpu, cube):
    """One sort at 16 bits yields the packets of 1, 5 and 16 bits: q(b - 1) == q(b) >> 1 at the boundaries, on the device."""
    depths = (1, 5, 16)
    frames = [boundary_cloud(cube, made_for) for made_for in (1, 4, 9, 16)]
    group = codec.cwipc_new_encodergroup()
    encoders = [group.addencoder(octree_bits=bits, jpeg_quality=85) for bits in depths]
    for i, pts in enumerate(frames):
        group.feed(make_cloud(gpu, pts, 0.0, 900 + i))
    for i, pts in enumerate(frames):
        for enc, bits in zip(encoders, depths):
            assert enc.available(True)
            got = bytes(enc.get_bytes())
            assert got == cm.encode(pts, bits, 85, 900 + i), (i, bits)
            assert got == encode(codec, gpu, pts, bits, 85, 900 + i), (i, bits)
    assert not any(enc.available(False) for enc in encoders)
    group.free()


# ---------------------------------------------------------------------------
# the edges of float32
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bits", EDGE_BITS)
@pytest.mark.parametrize("name", list(edge_clouds()))
def test_value_edges(codec, gpu, name, bits):
    pts = edge_clouds()[name]
    packet = check(codec, gpu, pts, bits, 85)
    info = cm.parse(packet)
    if name == "negative zero minimum":
        assert packet[24:36] == bytes(12)                                   # +0, not the -0.0 that is the minimum
    if name == "denormal":
        assert info["side"] == 4095 * 2.0 ** -149                            # nothing was flushed to zero on the way
        pc = check_decodes_to_model(codec, packet)
        assert (pc.cellsize() == 0.0) == (bits == 16)                        # side / 2^16 is below half the smallest float32
        assert pc.get_numpy_array()['x'].max() > 0
    if name == "huge":
        assert info["side"] == 2 * float(np.float32(3.4e38))


def non_finite_cloud(rng, n, first):
    """2000 points of which 300 have a non-finite coordinate: scattered, or the first 300 in input order."""
    pts = cm.random_cloud(rng, n, 1.0)
    bad = np.arange(300) if first else rng.permutation(n)[:300]
    pts['x'][bad[:100]] = np.nan
    pts['y'][bad[100:200]] = np.inf
    pts['z'][bad[200:]] = -np.inf
    pts['r'][bad], pts['tile'][bad] = 255, 128
    return pts, bad


@pytest.mark.parametrize("first", [False, True])
@pytest.mark.parametrize("bits", [1, 16])
def test_non_finite_points_at_both_ends_of_the_key_range(codec, gpu, bits, first):
    """The key of a point that is left out is 1 << 3 b: 8 at 1 bit, 2^48 at 16."""
    pts, bad = non_finite_cloud(np.random.default_rng(30 + bits), 2000, first)
    packet = check(codec, gpu, pts, bits, 95)
    assert packet == encode(codec, gpu, np.delete(pts, bad), bits, 95)
    assert not (cm.decode(packet)[0]['tile'] & 128).any()                  # (the tile of the points that are left out)
    assert len(check(codec, gpu, pts[bad], bits, 95)) == 48 + 4 * bits


# ---------------------------------------------------------------------------
# more points than one pass of the bounds kernel covers
# ---------------------------------------------------------------------------
def past_the_line(n):
    """n points uniform in the cube [-1, 1]^3 whose six extreme coordinates (+-1 exactly) lie at indices 0, 255, LINE - 1, LINE, n - 1
    and in the middle (others in the middle where these coincide or do not exist), with non-finite points on both sides of LINE
    where there is a second side."""
    rng = np.random.default_rng(n)
    pts = cm.random_cloud(rng, n, 1.0, tiles=(1, 2, 4))
    for axis in "xyz":
        np.clip(pts[axis], -0.999, 0.999, out=pts[axis])
    places = []
    for i in (0, 255, LINE - 1, LINE, n - 1, 70001, 65536, 99999):
        if i < n and i not in places:
            places.append(i)
    places = places[:6]
    for j, i in enumerate(places):
        pts["xyz"[j // 2]][i] = -1.0 if j % 2 == 0 else 1.0
    bad = sorted({i for i in (LINE - 73, LINE - 3, LINE - 2, LINE + 1, LINE + 2, LINE + 200, n - 2) if i < n and i not in places})
    pts['x'][bad[0::3]], pts['y'][bad[1::3]], pts['z'][bad[2::3]] = np.nan, np.inf, -np.inf
    pts['r'][bad], pts['tile'][bad] = 255, 128
    return pts, places, bad


@pytest.mark.parametrize("bits", [2, 16])
@pytest.mark.parametrize("n", [LINE, LINE + 1, LINE + 257])
def test_past_the_bounds_grid(codec, gpu, n, bits):
    """The smallest sizes at which the stride of codec_bounds_kernel takes a second step (none, one and two workgroups take it): an
    extreme or a non-finite point that only the second step sees must count.  The same cloud rotated by LINE positions, which swaps
    what lies on either side, gives the same packet."""
    pts, places, bad = past_the_line(n)
    assert len(places) == 6 and len(bad) >= 3 and (n == LINE or max(places) >= LINE) and (n <= LINE + 1 or max(bad) > LINE)
    packet = check(codec, gpu, pts, bits, 85)
    info = cm.parse(packet)
    assert info["min"].tolist() == [-1.0, -1.0, -1.0] and info["side"] == 2.0
    assert packet == encode(codec, gpu, np.roll(pts, LINE), bits, 85)
    if bits == 16:
        # the decoder's scan of a depth's popcounts runs past 256 workgroups of nodes: a second round of the scanning workgroup
        assert max(info["nodes"][:-1]) > 65536, info["nodes"]
        assert info["nleaves"] > n - len(bad) - 1000


# ---------------------------------------------------------------------------
# valid packets that no encoder makes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", [name for name, _ in hand_built_packets()])
def test_hand_built_packets(codec, gpu, name):
    packet = dict(hand_built_packets())[name]
    info = cm.parse(packet)
    pc = check_decodes_to_model(codec, packet)
    assert pc.count() == info["nleaves"]
    if name == "timestamp 2^63 + 5":
        assert pc.timestamp() == BIG_TIMESTAMP             # the wrapper carries all 64 bits
    if name == "side 1e39":
        assert np.isinf(pc.cellsize()) and np.isinf(pc.get_numpy_array()['x']).tolist() == [False, True]
    if name == "tile_mode 0, tile_value 255":
        assert (pc.get_numpy_array()['tile'] == 255).all()


# ---------------------------------------------------------------------------
# groups whose members come and go
# ---------------------------------------------------------------------------
def test_group_classes_closed_members_and_late_comers(codec, gpu):
    """Two voxelsizes x two tiles: four classes, one of them with two members of equal parameters; a fifth class whose tile does not
    occur; one member closed after the first feed; one added after it.  Every packet is what an encoder alone delivers and what the
    model makes of the library's own filter output."""
    rng = np.random.default_rng(40)
    frames = [cm.random_cloud(rng, 20000 + 500 * i, 1.0, (0.1 * i, 0, 0), tiles=(1, 2)) for i in range(3)]
    group = codec.cwipc_new_encodergroup()
    settings = [(1, 0.0, 9, 85), (1, 0.0, 9, 85), (2, 0.0, 6, 60), (1, 0.05, 12, 95), (2, 0.05, 9, 85), (64, 0.0, 7, 85)]

    def add(setting):
        tile, voxelsize, bits, quality = setting
        return group.addencoder(params=codec.cwipc_encoder_params(False, 1, 1.0, bits, quality, 16, tile, voxelsize))

    def expected(setting, frame):
        tile, voxelsize, bits, quality = setting
        pc = gpu.cwipc_tilefilter(make_cloud(gpu, frames[frame], 0.0, 700 + frame), tile)
        if voxelsize > 0:
            pc = gpu.cwipc_downsample(pc, voxelsize)
        kept = pc.get_numpy_array() if pc.count() else np.zeros(0, dtype=cm.POINT_DTYPE)
        want = cm.encode(kept, bits, quality, 700 + frame)
        assert want == encode(codec, gpu, frames[frame], bits, quality, 700 + frame, tilenumber=tile, voxelsize=voxelsize), (setting, frame)
        return want, len(kept)

    def take(enc):
        assert enc.available(True)
        return bytes(enc.get_bytes())

    encoders = [add(s) for s in settings]
    group.feed(make_cloud(gpu, frames[0], 0.0, 700))
    closed = 1                                              # one of the two equal members: its class goes on with the other
    encoders[closed].close()
    assert not encoders[closed].eof()                       # its packet of the first feed is still queued
    late_setting = (2, 0.0, 11, 85)
    late = add(late_setting)
    for frame in (1, 2):
        group.feed(make_cloud(gpu, frames[frame], 0.0, 700 + frame))
    for i, (enc, setting) in enumerate(zip(encoders, settings)):
        for frame in range(3):
            if i == closed and frame > 0:
                break
            want, kept = expected(setting, frame)
            got = take(enc)
            assert got == want, (setting, frame)
            if setting[0] == 64:
                assert kept == 0 and len(got) == 48 + 4 * setting[2]
            else:
                assert 0 < kept and (kept < int((frames[frame]['tile'] == setting[0]).sum())) == (setting[1] > 0)
            if frame == 0:
                check_decodes_to_model(codec, got)
        assert not enc.available(False) and enc.eof() == (i == closed)
    assert [take(late) for _ in range(2)] == [expected(late_setting, frame)[0] for frame in (1, 2)]
    assert not late.available(False)
    group.close()
    assert all(enc.eof() for enc in encoders + [late])
    group.free()


# ---------------------------------------------------------------------------
# the queue
# ---------------------------------------------------------------------------
def test_polling_sees_the_packet_arrive(codec, gpu):
    rng = np.random.default_rng(50)
    pts = cm.random_cloud(rng, 50000, 1.0)
    enc = codec.cwipc_new_encoder(octree_bits=10, jpeg_quality=85)
    enc.feed(make_cloud(gpu, pts, 0.0, 5))
    deadline = time.monotonic() + 10.0
    while not enc.available(False):
        if time.monotonic() > deadline:
            pytest.fail("available(False) did not become true within 10 s of the feed")
    assert bytes(enc.get_bytes()) == cm.encode(pts, 10, 85, 5)
    assert not enc.available(False)
    packet = cm.encode(pts, 10, 85, 5)
    dec = codec.cwipc_new_decoder()
    dec.feed(packet)
    deadline = time.monotonic() + 10.0
    while not dec.available(False):
        if time.monotonic() > deadline:
            pytest.fail("the decoder's available(False) did not become true within 10 s of the feed")
    assert dec.get().get_numpy_array().tobytes() == cm.decode(packet)[0].tobytes()


def test_results_can_be_taken_without_asking_first(codec, gpu):
    """get_encoded_size() and get_bytes() wait for the oldest packet themselves."""
    rng = np.random.default_rng(51)
    clouds = [cm.random_cloud(rng, 30000 + i, 1.0, tiles=(1, 2, 4) if i else (4,)) for i in range(2)]
    enc = codec.cwipc_new_encoder(octree_bits=11, jpeg_quality=60)
    assert enc.get_encoded_size() == 0
    for i, pts in enumerate(clouds):
        enc.feed(make_cloud(gpu, pts, 0.0, i))
    want = [cm.encode(pts, 11, 60, i) for i, pts in enumerate(clouds)]
    assert cm.parse(want[0])["tile_mode"] == 0 and cm.parse(want[1])["tile_mode"] == 1      # the size depends on what the device found
    assert enc.get_encoded_size() == len(want[0])
    assert bytes(enc.get_bytes()) == want[0]
    assert bytes(enc.get_bytes()) == want[1]
    assert enc.get_encoded_size() == 0 and not enc.available(False)


def in_thread(*jobs):
    """Runs each job in a thread of its own, all at once, and joins them; what a job raised is raised here."""
    failures = []
    barrier = threading.Barrier(len(jobs))

    def run(job):
        try:
            barrier.wait(timeout=10)
            job()
        except BaseException as e:   # noqa: B036 -- handed to the main thread
            failures.append(e)

    threads = [threading.Thread(target=run, args=(job,)) for job in jobs]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if failures:
        raise failures[0]


def test_fed_on_one_thread_collected_on_another(codec, gpu):
    """feed leaves its work in flight on the calling thread's stream; that thread has ended when the results are asked for."""
    rng = np.random.default_rng(52)
    clouds = [cm.random_cloud(rng, 40000 + 1000 * i, 1.0 + i) for i in range(3)]
    enc = codec.cwipc_new_encoder(octree_bits=12, jpeg_quality=85)
    in_thread(lambda: [enc.feed(make_cloud(gpu, pts, 0.0, 60 + i)) for i, pts in enumerate(clouds)])
    packets = []
    for _ in clouds:
        assert enc.available(True)
        packets.append(bytes(enc.get_bytes()))
    assert packets == [cm.encode(pts, 12, 85, 60 + i) for i, pts in enumerate(clouds)]
    assert not enc.available(False)
    dec = codec.cwipc_new_decoder()
    in_thread(lambda: [dec.feed(p) for p in packets])
    for p in packets:
        assert dec.available(True)
        pc = dec.get()
        want, ts, cell = cm.decode(p)
        assert pc.timestamp() == ts and np.float32(pc.cellsize()).tobytes() == cell.tobytes()
        assert pc.get_numpy_array().tobytes() == want.tobytes()
    assert not dec.available(False) and dec.get() is None


def test_two_threads_feed_two_encoders_at_once(codec, gpu):
    rng = np.random.default_rng(53)
    clouds = [[cm.random_cloud(rng, 20000 + 3000 * i + 500 * t, 1.0, (t, 0, 0)) for i in range(3)] for t in range(2)]
    settings = [(9, 85), (13, 60)]
    encoders = [codec.cwipc_new_encoder(octree_bits=bits, jpeg_quality=quality) for bits, quality in settings]

    def feeder(t):
        return lambda: [encoders[t].feed(make_cloud(gpu, pts, 0.0, 100 * t + i)) for i, pts in enumerate(clouds[t])]

    in_thread(feeder(0), feeder(1))
    for t, (bits, quality) in enumerate(settings):
        for i, pts in enumerate(clouds[t]):                 # each encoder's packets in its own feed order
            assert encoders[t].available(True)
            assert bytes(encoders[t].get_bytes()) == cm.encode(pts, bits, quality, 100 * t + i), (t, i)
        assert not encoders[t].available(False)


def test_nothing_is_left_behind(codec, gpu, clouds_before):
    """Last in the file: every cloud the tests above made, on whichever thread, has been freed with its wrapper."""
    gc.collect()
    assert gpu.cwipc_dangling_allocations(False) == clouds_before
