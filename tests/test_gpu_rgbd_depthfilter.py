"""The raw entry's depth post-processing (cwipc_hip_rgbd_rig_grab_filtered) on the GPU, byte for byte against the numpy model
(tests/rgbd_depthfilter_model.py in front of rgbd_lens_model / rgbd_occlusion_model): a NULL or all-off filter against the two existing
entries, the spatial filter on image shapes where a line kernel goes wrong, the hand-worked lines of the model test, alpha == 1, the
temporal filter through every history byte and every persistence mode, its arithmetic, the state's life, everything else of the raw
entry at once, the errors.  No tolerance anywhere: clouds, attached images and the state (doubles as bit patterns) are compared for
equality."""
import gc
import math

import numpy as np
import pytest

import rgbd_depthfilter_model as dm
import rgbd_lens_model as lm
import rgbd_model as rm
import rgbd_occlusion_model as om
from test_gpu_rgbd import FILTERS, assert_cloud, to_filter
from test_gpu_rgbd_occlusion import attached, cloud_bytes, frame_structs, pinhole_pair
from test_gpu_rgbd_raw import raw_images, raw_pair
from test_rgbd_depthfilter_model import HAND_ALPHA, HAND_DELTA, THREE, TWO_BY_TWO, persists_table
from cwipc_util_amd.rgbd import RgbdDepthFilter, RgbdOcclusion, RgbdPrep, RgbdRig, RgbdRigSource

pytestmark = pytest.mark.gpu

OFF = RgbdDepthFilter(0, 0.5, 20.0, False, 0.4, 20.0, 0)


def identity_pair(width, height, tile, serial):
    """A sensor without lenses whose colour side is its depth side: every pixel with depth keeps it, so the attached depth image is
    the filtered one."""
    intr = (0.9 * width, 1.1 * width, 0.48 * width, 0.53 * height)
    return pinhole_pair(width, height, width, height, intr, intr, tile=tile, serial=serial)


def banded(rng, width, height, delta, zeros=0.1, base=1000):
    """Depth in a band four delta wide -- neighbours blend about as often as not -- with about `zeros` of the pixels 0, in runs along
    rows and down columns; the first and the last pixel are holes, so some lines start and some end with one."""
    depth = (base + rng.integers(0, int(4 * delta) + 1, (height, width))).astype(np.uint16)
    if zeros > 0:
        flat = depth.reshape(-1)
        while (flat == 0).sum() < zeros * flat.size:
            start = int(rng.integers(0, flat.size))
            flat[start:start + int(rng.integers(1, 6))] = 0
        for _ in range(1 + width * height // 400):
            u, v = int(rng.integers(0, width)), int(rng.integers(0, height))
            depth[v:v + int(rng.integers(1, 5)), u] = 0
        depth[0, 0] = depth[-1, -1] = 0
    return depth


def colour_for(rng, sensor):
    return rng.integers(0, 256, (sensor.colour_height, sensor.colour_width, sensor.bpp)).astype(np.uint8)


def histories(sensors):
    return [dm.History(s.height, s.width) for s in sensors]


def assert_history(rig, hists):
    for i, hist in enumerate(hists):
        value, history = rig.history(i)
        assert value.dtype == np.float64 and history.dtype == np.uint8 and value.shape == hist.value.shape == history.shape
        assert np.array_equal(value.view(np.uint64), np.ascontiguousarray(hist.value).view(np.uint64))
        assert np.array_equal(history, hist.history)


def check(gpu, rig, sensors, models, frame, df, hists, occ=None, flt=rm.Filter(), ex=0, ey=0, tables=None, grab_frame=None):
    """One filtered grab with both images attached: cloud, depth images and registered images are the model's, and so is the state
    afterwards.  Returns (the model's result, the filtered frame)."""
    filtered = dm.depth_filter(frame, hists, df)
    if occ is None:
        want = lm.cloud(models, filtered, flt, ex, ey, tables)
    else:
        want = om.cloud(models, filtered, flt, ex, ey, tables, occ.splat, occ.margin)
    pc = rig.grab(frame if grab_frame is None else grab_frame, to_filter(flt), RgbdPrep(ex, ey), 4711, 0.5,
                  gpu.CWIPC_HIP_RGBD_ATTACH_RGB | gpu.CWIPC_HIP_RGBD_ATTACH_DEPTH, occ, df)
    got = attached(pc, sensors)
    for (rgb, depth), want_depth, want_rgb in zip(got, want[1], want[2]):
        assert np.array_equal(depth, want_depth)
        assert np.array_equal(rgb, want_rgb)
    assert_cloud(pc, want[0], 4711, 0.5)
    assert_history(rig, hists)
    return want, filtered


# ---- 1: off is the existing entries ----

@pytest.fixture(scope="module")
def raw(gpu):
    """test_gpu_rgbd_raw.py's two raw sensors (depth 67 x 45, colour 101 x 77, rational lenses, R, G, B and B, G, R, A), their model
    twins and ray tables, and three frames whose depth lies in a band, so that the filters have something to blend."""
    rng = np.random.default_rng(303)
    pairs = [raw_pair(67, 45, 101, 77, 2, "raw3", 3, rng), raw_pair(67, 45, 101, 77, 4, "raw4", 4, rng)]
    frames = []
    for n in range(3):
        frames.append([(banded(rng, 67, 45, 20.0, 0.08, 1500 + 10 * n), raw_images(67, 45, 101, 77, bpp, rng)[1]) for bpp in (3, 4)])
    sensors, models = [p[0] for p in pairs], [p[1] for p in pairs]
    tables = [lm.ray_table(m.width, m.height, m.fx, m.fy, m.cx, m.cy, m.coeffs) for m in models]
    with RgbdRig(sensors) as rig:
        yield sensors, models, tables, frames, rig


@pytest.mark.parametrize("occluded", [False, True])
def test_off_is_the_existing_entries(gpu, raw, occluded):
    sensors, _models, _tables, frames, _rig = raw
    flags = gpu.CWIPC_HIP_RGBD_ATTACH_RGB | gpu.CWIPC_HIP_RGBD_ATTACH_DEPTH
    occ = RgbdOcclusion(1, 0.02) if occluded else None
    flt, prep = to_filter(FILTERS["depth"]), RgbdPrep(1, 2)
    with RgbdRig(sensors) as rig:
        want = rig.grab(frames[0], flt, prep, 99, 0.125, flags, occ)
        assert want.count() > 0
        structs = frame_structs(gpu, frames[0])
        null = gpu.cwipc_hip_rgbd_rig_grab_filtered(rig._handle(), structs, None, prep.as_struct(), occ.as_struct() if occ else None, flt.as_struct(), 99, 0.125, flags)
        off = rig.grab(frames[0], flt, prep, 99, 0.125, flags, occ, OFF)
        for got in (null, off):
            assert cloud_bytes(got) == cloud_bytes(want) and got.timestamp() == 99 and got.cellsize() == 0.125
            assert gpu.get_tiles_used(got) == gpu.get_tiles_used(want)
            for (rgb, depth), (want_rgb, want_depth) in zip(attached(got, sensors), attached(want, sensors)):
                assert np.array_equal(rgb, want_rgb) and np.array_equal(depth, want_depth)
        assert_history(rig, histories(sensors))     # zeros: there is no state


# ---- 2: the spatial filter on shapes where a line kernel goes wrong ----

SHAPES = [(1, 1), (1, 7), (7, 1), (63, 5), (64, 64), (65, 66), (129, 3), (200, 130)]      # width x height


@pytest.fixture(scope="module")
def shapes(gpu):
    pairs = [identity_pair(w, h, k + 1, "s%dx%d" % (w, h)) for k, (w, h) in enumerate(SHAPES)]
    sensors, models = [p[0] for p in pairs], [p[1] for p in pairs]
    with RgbdRig(sensors) as rig:
        yield sensors, models, rig


@pytest.mark.parametrize("magnitude,empty,full", [(1, 1, 4), (2, 2, 5), (5, 6, 3)])
def test_spatial_on_shapes_where_a_line_kernel_goes_wrong(gpu, shapes, magnitude, empty, full):
    """Lines that end inside, at and just past 32 and 64 pixels, cameras of one line, more lines than one workgroup holds (200 x 130),
    neighbouring cameras whose lines must not run into each other.  Camera `empty` is all zero, camera `full` has no hole."""
    sensors, models, rig = shapes
    rng = np.random.default_rng(400 + magnitude)
    delta = 12.0
    frame = []
    for k, s in enumerate(sensors):
        depth = np.zeros((s.height, s.width), dtype=np.uint16) if k == empty else banded(rng, s.width, s.height, delta, 0.0 if k == full else 0.1)
        frame.append((depth, colour_for(rng, s)))
    df = RgbdDepthFilter(magnitude, 0.45, delta, False)
    want, filtered = check(gpu, rig, sensors, models, frame, df, histories(sensors))
    for k, ((depth, _c), (out, _c2)) in enumerate(zip(frame, filtered)):
        assert np.array_equal(out == 0, depth == 0)
        if k != empty and depth.shape[1] >= 63:
            # both branches of the comparison occur: two values of a band four delta wide are within delta 7 times in 16
            both = (depth[:, 1:] != 0) & (depth[:, :-1] != 0)
            near = np.abs(depth[:, 1:].astype(np.int64) - depth[:, :-1].astype(np.int64)) < delta
            assert 0.25 < near[both].mean() < 0.65 and not np.array_equal(out, depth)
    assert not filtered[empty][0].any() and filtered[full][0].all()
    assert len(want[0]) == sum(int((d != 0).sum()) for d, _c in frame)


def test_spatial_on_lines_longer_than_one_chunk(gpu):
    """A line of more than 1020 pixels goes through the kernel's LDS tile in chunks, the running value carried over: rows of 1021 and
    2045 pixels (two and three chunks), columns of 1030, holes included."""
    rng = np.random.default_rng(410)
    pairs = [identity_pair(w, h, k + 1, "long%d" % k) for k, (w, h) in enumerate([(1021, 2), (2, 1030), (2045, 1)])]
    sensors, models = [p[0] for p in pairs], [p[1] for p in pairs]
    frame = [(banded(rng, s.width, s.height, 12.0, 0.03), colour_for(rng, s)) for s in sensors]
    frame[0][0][:, 1015:1021] = 1020 + np.arange(6, dtype=np.uint16)            # no hole where the first chunk ends
    frame[2][0][0, 1015:1025] = 1020 + np.arange(10, dtype=np.uint16)
    with RgbdRig(sensors) as rig:
        for magnitude in (1, 2):
            _want, filtered = check(gpu, rig, sensors, models, frame, RgbdDepthFilter(magnitude, 0.45, 12.0, False), histories(sensors))
            assert (filtered[0][0][:, 1019:1021] != frame[0][0][:, 1019:1021]).any()


# ---- 3: order and strictness on the device ----

def test_hand_worked_lines_on_the_device(gpu):
    rng = np.random.default_rng(420)
    pairs = [identity_pair(3, 1, 1, "three"), identity_pair(2, 2, 2, "two"), identity_pair(2, 1, 3, "pair"), identity_pair(1, 3, 4, "column")]
    sensors, models = [p[0] for p in pairs], [p[1] for p in pairs]
    pair = np.array([[1000, 1016]], dtype=np.uint16)
    frame = [(d, colour_for(rng, s)) for d, s in zip((THREE[0], TWO_BY_TWO[0], pair, np.ascontiguousarray(THREE[0].T)), sensors)]
    flags = gpu.CWIPC_HIP_RGBD_ATTACH_DEPTH | gpu.CWIPC_HIP_RGBD_ATTACH_RGB
    with RgbdRig(sensors) as rig:
        def depths(df):
            check(gpu, rig, sensors, models, frame, df, histories(sensors))
            return [d for _rgb, d in attached(rig.grab(frame, attach_flags=flags, depthfilter=df), sensors)]

        got = depths(RgbdDepthFilter(1, HAND_ALPHA, HAND_DELTA, False))
        assert np.array_equal(got[0], THREE[1]) and np.array_equal(got[1], TWO_BY_TWO[1]) and np.array_equal(got[3], THREE[1].T)
        assert np.array_equal(depths(RgbdDepthFilter(1, 0.5, 16.0, False))[2], pair)                              # exactly delta: kept
        assert depths(RgbdDepthFilter(1, 0.5, float(np.nextafter(16.0, np.inf)), False))[2].tolist() == [[1004, 1008]]


# ---- 4: alpha == 1 ----

def test_alpha_one_is_the_all_off_result(gpu, raw):
    sensors, _models, _tables, frames, _rig = raw
    flags = gpu.CWIPC_HIP_RGBD_ATTACH_RGB | gpu.CWIPC_HIP_RGBD_ATTACH_DEPTH
    for df in (RgbdDepthFilter(2, 1.0, 20.0, False), RgbdDepthFilter(0, 0.5, 20.0, True, 1.0, 20.0, 0), RgbdDepthFilter(5, 1.0, 20.0, True, 1.0, 20.0, 0)):
        with RgbdRig(sensors) as rig, RgbdRig(sensors) as plain:
            for frame in frames:
                got, want = rig.grab(frame, None, RgbdPrep(1, 1), 5, 0.0, flags, None, df), plain.grab(frame, None, RgbdPrep(1, 1), 5, 0.0, flags)
                assert want.count() > 0 and cloud_bytes(got) == cloud_bytes(want)
                for (rgb, depth), (want_rgb, want_depth) in zip(attached(got, sensors), attached(want, sensors)):
                    assert np.array_equal(rgb, want_rgb) and np.array_equal(depth, want_depth)


# ---- 5: every history byte, every mode ----

@pytest.mark.parametrize("mode", range(9))
def test_temporal_all_histories_all_modes(gpu, mode):
    """Pixel i of the 16 x 16 camera has depth in frame f of 0 .. 7 iff bit 7 - f of i is set, so before frame 8 its history byte is
    i.  Frame 8 is empty: depth comes out exactly where persists(mode, i) holds and the pixel has a value.  The 5 x 3 camera beside
    it checks the per-camera offsets of the state."""
    rng = np.random.default_rng(500 + mode)
    alpha, delta = 0.4, 20.0
    pairs = [identity_pair(16, 16, 1, "bytes"), identity_pair(5, 3, 2, "beside")]
    sensors, models = [p[0] for p in pairs], [p[1] for p in pairs]
    df = RgbdDepthFilter(0, 0.5, 20.0, True, alpha, delta, mode)
    index = np.arange(256).reshape(16, 16)
    hists = histories(sensors)
    with RgbdRig(sensors) as rig:
        for f in range(10):
            if f < 8:
                last = 1000 + rng.integers(-9, 10, (16, 16))          # any two of these, and any blend of them, are within delta
                first = np.where((index >> (7 - f)) & 1, last, 0).astype(np.uint16)
                second = banded(rng, 5, 3, delta, 0.3)
            elif f == 8:
                first, second = np.zeros((16, 16), dtype=np.uint16), np.zeros((3, 5), dtype=np.uint16)
            else:
                first, second = banded(rng, 16, 16, delta, 0.0), banded(rng, 5, 3, delta, 0.0)
            if f == 8:
                assert np.array_equal(hists[0].history, index.astype(np.uint8))
                running = hists[0].value.copy()
            frame = [(first, colour_for(rng, sensors[0])), (second, colour_for(rng, sensors[1]))]
            _want, filtered = check(gpu, rig, sensors, models, frame, df, hists)
            if f == 8:
                expect = persists_table(mode).reshape(16, 16) & (index != 0)
                out = filtered[0][0]
                assert np.array_equal(out != 0, expect)
                assert np.array_equal(out[expect], np.floor(running[expect] + 0.5).astype(np.uint16))
                assert (hists[0].history == ((index << 1) & 0xff)).all() and np.array_equal(hists[0].value, running)
        assert (hists[0].history & 1).all() and (hists[1].history & 1).all()


# ---- 6: the temporal arithmetic ----

def test_temporal_arithmetic(gpu):
    pairs = [identity_pair(2, 1, 1, "jump"), identity_pair(1, 1, 2, "settle")]
    sensors, models = [p[0] for p in pairs], [p[1] for p in pairs]
    rng = np.random.default_rng(600)
    colours = [colour_for(rng, s) for s in sensors]
    jumps = [[1000, 1000], [1020, 980]] + [[1020, 980]] * 10
    settle = [1003] + [1000] * 11
    for delta, second in ((20.0, [1020, 980]), (float(np.nextafter(20.0, np.inf)), [1008, 992])):
        hists = histories(sensors)
        with RgbdRig(sensors) as rig:
            outs = []
            for jump, value in zip(jumps, settle):
                frame = [(np.array([jump], dtype=np.uint16), colours[0]), (np.array([[value]], dtype=np.uint16), colours[1])]
                _want, filtered = check(gpu, rig, sensors, models, frame, RgbdDepthFilter(0, 0.5, 20.0, True, 0.4, delta, 0), hists)
                outs.append((filtered[0][0][0].tolist(), int(filtered[1][0][0, 0])))
            assert outs[1][0] == second                                   # exactly delta: taken over; one ulp less: blended
            # the unrounded s goes 1003, 1001.8, 1001.08, 1000.648, 1000.3888, ...; a rounded one would stall at 1001
            assert [o[1] for o in outs[:5]] == [1003, 1002, 1001, 1001, 1000] and outs[-1][1] == 1000
            value, _history = rig.history(1)
            assert 1000.0 < value[0, 0] < 1000.02


# ---- 7: the state's life ----

def test_state_handling(gpu, raw):
    sensors, models, tables, frames, _rig = raw
    df = RgbdDepthFilter(1, 0.5, 20.0, True, 0.4, 20.0, 3)
    flags = gpu.CWIPC_HIP_RGBD_ATTACH_RGB | gpu.CWIPC_HIP_RGBD_ATTACH_DEPTH
    with RgbdRig(sensors) as rig, RgbdRig(sensors) as other:
        hists, other_hists = histories(sensors), histories(sensors)
        first = check(gpu, rig, sensors, models, frames[0], df, hists, tables=tables)[0]
        # a grab without the temporal stage, a plain grab and a refused grab in the middle: the state stays
        rig.grab(frames[2], depthfilter=RgbdDepthFilter(2, 0.5, 20.0, False))
        rig.grab(frames[2])
        with pytest.raises(gpu.CwipcError, match="temporal_persistency"):
            rig.grab(frames[2], depthfilter=RgbdDepthFilter(1, 0.5, 20.0, True, 0.4, 20.0, 9))
        assert_history(rig, hists)
        # two rigs fed alternately do not mix
        check(gpu, other, sensors, models, frames[2], df, other_hists, tables=tables)
        second = check(gpu, rig, sensors, models, frames[1], df, hists, tables=tables)[0]
        check(gpu, other, sensors, models, frames[0], df, other_hists, tables=tables)
        check(gpu, rig, sensors, models, frames[2], df, hists, tables=tables)
        assert first[0].tobytes() != second[0].tobytes() and hists[0].value.tobytes() != other_hists[0].value.tobytes()
        # reset: the next grab is a fresh rig's first
        rig.reset_history()
        assert_history(rig, histories(sensors))
        again = rig.grab(frames[0], None, None, 4711, 0.5, flags, None, df)
        assert cloud_bytes(again) == first[0].tobytes()
        for (rgb, depth), want_depth, want_rgb in zip(attached(again, sensors), first[1], first[2]):
            assert np.array_equal(depth, want_depth) and np.array_equal(rgb, want_rgb)
        # ... and the one after it is that rig's second, which is not what a first grab of the same frame gives
        hists = histories(sensors)
        dm.depth_filter(frames[0], hists, df)
        after = check(gpu, rig, sensors, models, frames[1], df, hists, tables=tables)[0]
        alone = lm.cloud(models, dm.depth_filter(frames[1], histories(sensors), df), rm.Filter(), 0, 0, tables)
        assert after[0].tobytes() != alone[0].tobytes()
    # free(), then a new rig: empty
    with RgbdRig(sensors) as fresh:
        assert_history(fresh, histories(sensors))
        check(gpu, fresh, sensors, models, frames[0], df, histories(sensors), tables=tables)


# ---- 8: with everything else ----

@pytest.mark.parametrize("name", list(FILTERS))
def test_with_erosion_occlusion_lenses_bgra_filters_and_page_locked_images(gpu, raw, name):
    sensors, models, tables, frames, rig = raw
    keep = []

    def pin(a):
        block = gpu.cwipc_hip_pinned_points((a.nbytes + 15) // 16)
        keep.append(block)
        out = block.view(np.uint8)[:a.nbytes].view(a.dtype).reshape(a.shape)
        out[...] = a
        return out

    df = RgbdDepthFilter(2, 0.5, 20.0, True, 0.4, 20.0, 3)
    rig.reset_history()
    hists = histories(sensors)
    for n, frame in enumerate(frames):
        pinned = [(pin(d), pin(c)) for d, c in frame] if n != 1 else None
        want, filtered = check(gpu, rig, sensors, models, frame, df, hists, RgbdOcclusion(1, 0.02), FILTERS[name], 1, 2, tables, grab_frame=pinned)
        assert all(not np.array_equal(f[0], g[0]) for f, g in zip(filtered, frame))
        if pinned is not None:
            assert all(np.array_equal(p[0], g[0]) for p, g in zip(pinned, frame))      # the caller's images are not written
        assert len(want[0]) > 0 or name != "off"
    assert all(int(((f[0] != 0) & (g[0] == 0)).sum()) > 0 for f, g in zip(filtered, frames[2]))      # persisted pixels, in the last frame


def test_rig_source_with_a_depth_filter(gpu, raw):
    sensors, models, tables, frames, _rig = raw
    df = RgbdDepthFilter()
    assert (df.spatial_magnitude, df.spatial_alpha, df.spatial_delta, df.temporal, df.temporal_alpha, df.temporal_delta, df.temporal_persistency) == \
        (2, 0.5, 20.0, True, 0.4, 20.0, 3)
    struct = RgbdDepthFilter(1, 0.25, 3.5, False, 0.75, 4.5, 7).as_struct()
    assert isinstance(struct, gpu.cwipc_hip_rgbd_depthfilter)
    assert (struct.spatial_magnitude, struct.spatial_alpha, struct.spatial_delta, struct.temporal, struct.temporal_alpha, struct.temporal_delta,
            struct.temporal_persistency) == (1, 0.25, 3.5, 0, 0.75, 4.5, 7)
    src = RgbdRigSource(sensors, list(frames), None, RgbdPrep(1, 1), 0.25, 12, depthfilter=df)
    src.request_metadata("rgb")
    src.request_metadata("depth")
    hists = histories(sensors)
    for n, frame in enumerate(frames):
        want = lm.cloud(models, dm.depth_filter(frame, hists, df), rm.Filter(), 1, 1, tables)
        pc = src.get()
        assert_cloud(pc, want[0], 12 + n, 0.25)
        for (rgb, depth), want_depth, want_rgb in zip(attached(pc, sensors), want[1], want[2]):
            assert np.array_equal(depth, want_depth) and np.array_equal(rgb, want_rgb)
    assert_history(src.rig, hists)
    assert src.get() is None
    src.free()
    plain = RgbdRigSource(sensors, [frames[0]])
    assert plain.depthfilter is None
    plain.free()


# ---- 9: errors ----

def test_bad_depth_filters_are_errors_and_leave_nothing(gpu, raw):
    sensors, _models, _tables, frames, rig = raw
    rig.reset_history()
    rig.grab(frames[0], depthfilter=RgbdDepthFilter())       # (the state exists from here on)
    value, history = rig.history(0)
    gc.collect()
    before = gpu.cwipc_dangling_allocations(False)
    bad = [(RgbdDepthFilter(-1), "spatial_magnitude must be between 0 and 5"), (RgbdDepthFilter(6), "spatial_magnitude must be between 0 and 5"),
           (RgbdDepthFilter(temporal_persistency=-1), "temporal_persistency must be between 0 and 8"),
           (RgbdDepthFilter(temporal_persistency=9), "temporal_persistency must be between 0 and 8"),
           (RgbdDepthFilter(0, temporal=False, temporal_persistency=9), "temporal_persistency must be between 0 and 8")]
    for alpha in (0.0, -0.5, float(np.nextafter(1.0, np.inf)), math.nan, math.inf):
        bad += [(RgbdDepthFilter(spatial_alpha=alpha), "spatial_alpha must be"), (RgbdDepthFilter(temporal_alpha=alpha), "temporal_alpha must be")]
    for delta in (0.0, -1.0, math.nan, math.inf):
        bad += [(RgbdDepthFilter(spatial_delta=delta), "spatial_delta must be"), (RgbdDepthFilter(temporal_delta=delta), "temporal_delta must be")]
    for df, text in bad:
        with pytest.raises(gpu.CwipcError, match=text):
            rig.grab(frames[1], depthfilter=df)
        assert gpu.cwipc_dangling_allocations(False) == before
    # everything the two existing entries refuse, through the new one
    with pytest.raises(gpu.CwipcError, match="between 0 and 32"):
        rig.grab(frames[1], None, RgbdPrep(33, 0), depthfilter=RgbdDepthFilter())
    with pytest.raises(gpu.CwipcError, match="splat must be between 0 and 8"):
        rig.grab(frames[1], occlusion=RgbdOcclusion(9, 0.02), depthfilter=RgbdDepthFilter())
    with pytest.raises(gpu.CwipcError, match="margin must be finite"):
        rig.grab(frames[1], occlusion=RgbdOcclusion(1, -1.0), depthfilter=RgbdDepthFilter())
    good = frame_structs(gpu, frames[1])
    with pytest.raises(gpu.CwipcError, match="NULL argument"):
        gpu.cwipc_hip_rgbd_rig_grab_filtered(rig._handle(), [gpu.cwipc_hip_rgbd_frame(None, good[0].colour), good[1]], RgbdDepthFilter().as_struct())
    with pytest.raises(gpu.CwipcError, match="NULL argument"):
        gpu.cwipc_hip_rgbd_rig_grab_filtered(None, good, RgbdDepthFilter().as_struct())
    with pytest.raises(gpu.CwipcError, match="NULL argument"):
        gpu.cwipc_hip_rgbd_rig_grab_filtered(rig._handle(), [], RgbdDepthFilter().as_struct())
    gc.collect()
    assert gpu.cwipc_dangling_allocations(False) == before
    # none of them touched the state
    after = rig.history(0)
    assert np.array_equal(after[0].view(np.uint64), value.view(np.uint64)) and np.array_equal(after[1], history) and history.any()
    with pytest.raises(IndexError):
        rig.history(2)
    with pytest.raises(gpu.CwipcError):
        gpu.cwipc_hip_rgbd_rig_history(rig._handle(), 2, 67, 45)
    # the parameters of a stage that is off are not judged
    assert rig.grab(frames[1], depthfilter=RgbdDepthFilter(0, 7.0, -1.0, True, 0.4, 20.0, 3)).count() > 0
    assert rig.grab(frames[1], depthfilter=RgbdDepthFilter(2, 0.5, 20.0, False, math.nan, 0.0, 8)).count() > 0
    assert rig.grab(frames[1], depthfilter=RgbdDepthFilter(0, 7.0, math.nan, False, -3.0, math.inf, 0)).count() > 0
