"""The raw entry's depth decimation (cwipc_hip_rgbd_rig_create_decimated) and hole filling (cwipc_hip_rgbd_rig_grab_filled) on the GPU,
byte for byte: decimation 1 against cwipc_hip_rgbd_rig_create; a decimated rig fed full frames against a plain rig made from the numpy
model's derived sensors and fed the model's decimated frames (tests/rgbd_decimate_model.py), through every grab entry, with the
temporal state compared after each grab; image shapes where the decimation kernel goes wrong; the three fill modes against the model on
rows that begin with holes, have none, and have their only depth in column 0 at the widths where the scan's chunks end; the Python
source; one rig whose device block has every kind of part at odd sizes, with every stage on; the refusals.  No tolerance anywhere: clouds, attached images, ray tables and the state (doubles as bit patterns) are compared
for equality."""
import gc
import struct

import numpy as np
import pytest

import rgbd_decimate_model as cm
import rgbd_lens_model as lm
from test_gpu_rgbd import FILTERS, assert_cloud, to_filter
from test_gpu_rgbd_depthfilter import assert_history, banded, colour_for, histories, identity_pair
from test_gpu_rgbd_occlusion import attached, cloud_bytes, frame_structs, pinhole_pair
from test_gpu_rgbd_raw import raw_images, raw_pair
from cwipc_util_amd.rgbd import RgbdDepthFilter, RgbdHoleFill, RgbdOcclusion, RgbdPrep, RgbdRig, RgbdRigSource, RgbdSensor

pytestmark = pytest.mark.gpu

DF = RgbdDepthFilter(2, 0.5, 20.0, True, 0.4, 20.0, 3)


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def fields(sensor_struct):
    """Every field of a cwipc_hip_rgbd_sensor but the serial: numbers as bit patterns."""
    out = []
    for name, _type in sensor_struct._fields_:
        value = getattr(sensor_struct, name)
        if name != "serial":
            out.append(tuple(bits(x) for x in value) if hasattr(value, "__len__") else (bits(value) if isinstance(value, float) else value))
    return out


def sensor_from_model(m, serial):
    """The RgbdSensor of an lm.Sensor: how a derived sensor of the model becomes a plain rig's."""
    return RgbdSensor(m.width, m.height, m.fx, m.fy, m.cx, m.cy, m.colour_size[0], m.colour_size[1], *m.colour_intr, m.coeffs, m.colour_coeffs,
                      m.depth_to_colour, m.depth_scale, m.trafo, m.tile, serial, m.bpp)


def flags_of(gpu):
    return gpu.CWIPC_HIP_RGBD_ATTACH_RGB | gpu.CWIPC_HIP_RGBD_ATTACH_DEPTH


def assert_same(gpu, got, want, grid):
    """Two clouds grabbed with both images attached are the same: points, timestamp, cell size, tiles, images and their descriptions."""
    assert cloud_bytes(got) == cloud_bytes(want) and got.timestamp() == want.timestamp() and got.cellsize() == want.cellsize()
    assert gpu.get_tiles_used(got) == gpu.get_tiles_used(want)
    for (rgb, depth), (want_rgb, want_depth) in zip(attached(got, grid), attached(want, grid)):
        assert np.array_equal(rgb, want_rgb) and np.array_equal(depth, want_depth)
    meta, want_meta = got.access_metadata(), want.access_metadata()
    for i, s in enumerate(grid):
        for j, bpp in ((2 * i, 3), (2 * i + 1, 2)):
            assert meta.description(j) == want_meta.description(j) == "width=%d,height=%d,bpp=%d" % (s.width, s.height, bpp)


def assert_same_history(rig, plain, n):
    for i in range(n):
        (value, history), (want_value, want_history) = rig.history(i), plain.history(i)
        assert value.shape == want_value.shape and np.array_equal(value.view(np.uint64), want_value.view(np.uint64)) and np.array_equal(history, want_history)


def kernels_of(gpu, call):
    with gpu.cwipc_hip_profile() as prof:
        rv = call()
    return rv, prof.kernels


@pytest.fixture(scope="module")
def raw(gpu):
    """Two raw sensors with rational lenses (depth 131 x 93, colour 101 x 77, R, G, B and B, G, R, A), their model twins, and three
    frames whose depth lies in a band -- the filters blend, medians and means differ -- with holes in runs and one large hole that no
    decimation closes."""
    rng = np.random.default_rng(808)
    pairs = [raw_pair(131, 93, 101, 77, 2, "dec3", 3, rng), raw_pair(131, 93, 101, 77, 4, "dec4", 4, rng)]
    frames = []
    for n in range(3):
        frame = []
        for bpp in (3, 4):
            depth = banded(rng, 131, 93, 20.0, 0.15, 1500 + 10 * n)
            depth[10 + n:44, 20:60 - n] = 0
            frame.append((depth, raw_images(131, 93, 101, 77, bpp, rng)[1]))
        frames.append(frame)
    return [p[0] for p in pairs], [p[1] for p in pairs], frames


# ---- 1: decimation 1 is cwipc_hip_rgbd_rig_create ----

def test_decimation_one_is_rig_create(gpu, raw):
    sensors, _models, frames = raw
    through = RgbdRig.__new__(RgbdRig)          # an RgbdRig over a handle of the new entry (RgbdRig(sensors, 1) itself takes the old one)
    through.sensors, through.decimation, through.grid_sensors = list(sensors), 1, list(sensors)
    through._rig = gpu.cwipc_hip_rgbd_rig_create_decimated([s.as_struct() for s in sensors], 1)
    flags = flags_of(gpu)
    with through as rig, RgbdRig(sensors) as plain:
        assert gpu.cwipc_hip_rgbd_rig_decimation(rig._handle()) == 1 == gpu.cwipc_hip_rgbd_rig_decimation(plain._handle()) == plain.decimation
        assert gpu.cwipc_hip_rgbd_rig_decimation(None) == 0
        for i, s in enumerate(sensors):
            for handle in (rig._handle(), plain._handle()):
                g = gpu.cwipc_hip_rgbd_rig_grid_sensor(handle, i)
                assert fields(g) == fields(s.as_struct()) and g.serial is None
            assert rig.ray_table(i).tobytes() == plain.ray_table(i).tobytes()
            assert rig.map2d3d(i, 17, 23, 1234) == plain.map2d3d(i, 17, 23, 1234) and rig.map2d3d(i, 131, 0, 5) is None
            assert plain.grid_sensors[i] == s
        flt, prep, occ = to_filter(FILTERS["depth"]), RgbdPrep(1, 2), RgbdOcclusion(1, 0.02)
        for kw in (dict(), dict(occlusion=occ), dict(depthfilter=DF), dict(depthfilter=DF, occlusion=occ)):
            for frame in frames[:2]:
                got, kernels = kernels_of(gpu, lambda: rig.grab(frame, flt, prep, 99, 0.125, flags, **kw))
                want, want_kernels = kernels_of(gpu, lambda: plain.grab(frame, flt, prep, 99, 0.125, flags, **kw))
                assert want.count() > 0
                assert_same(gpu, got, want, sensors)
                assert {name: n for name, (_ms, n) in kernels.items()} == {name: n for name, (_ms, n) in want_kernels.items()}
                assert "rgbd_decimate" not in kernels
            assert_same_history(rig, plain, len(sensors))


# ---- 2: the equivalence that carries the feature ----

@pytest.mark.parametrize("k", range(2, 9))
def test_a_decimated_rig_is_a_plain_rig_on_the_models_grid(gpu, raw, k):
    sensors, models, frames = raw
    derived = [cm.derived_sensor(m, k) for m in models]
    small_sensors = [sensor_from_model(d, s.serial) for d, s in zip(derived, sensors)]
    small_frames = [[(cm.decimate(depth, k), colour) for depth, colour in frame] for frame in frames]
    assert all((d == 0).any() and (d != 0).any() and d.shape == (93 // k, 131 // k) for frame in small_frames for d, _c in frame)
    tables = [lm.ray_table(m.width, m.height, m.fx, m.fy, m.cx, m.cy, m.coeffs) for m in derived]
    flags = flags_of(gpu)
    with RgbdRig(sensors, k) as rig, RgbdRig(small_sensors) as plain:
        assert rig.decimation == k == gpu.cwipc_hip_rgbd_rig_decimation(rig._handle())
        for i, (g, d, s) in enumerate(zip(rig.grid_sensors, derived, sensors)):
            assert (g.width, g.height) == (d.width, d.height) == (131 // k, 93 // k)
            assert [bits(x) for x in (g.fx, g.fy, g.cx, g.cy)] == [bits(x) for x in (d.fx, d.fy, d.cx, d.cy)]
            assert g == small_sensors[i]                                               # lenses, colour side, matrices, tile: unchanged
            raw_struct = gpu.cwipc_hip_rgbd_rig_grid_sensor(rig._handle(), i)
            assert fields(raw_struct) == fields(small_sensors[i].as_struct()) and raw_struct.serial is None
            table = rig.ray_table(i)
            assert table.shape == (d.height, d.width, 2) and table.tobytes() == plain.ray_table(i).tobytes()
            assert np.array_equal(table.view(np.uint64), tables[i].view(np.uint64))
            for u, v in ((0, 0), (d.width - 1, d.height - 1), (d.width // 2, d.height // 3)):
                assert rig.map2d3d(i, u, v, 1777) == plain.map2d3d(i, u, v, 1777) and rig.map2d3d(i, u, v, 1777) is not None
                assert rig.mapcolordepth(i, u, v) == (u, v)
            # the full-size grid's far pixels are not pixels of this rig
            assert rig.map2d3d(i, d.width, 0, 1777) is None and rig.map2d3d(i, 0, d.height, 1777) is None
            assert rig.mapcolordepth(i, d.width, 0) is None and rig.mapcolordepth(i, 130, 92) is None
        flt, prep, occ = to_filter(FILTERS["all"]), RgbdPrep(2, 2), RgbdOcclusion(1, 0.02)
        for kw in (dict(), dict(occlusion=occ), dict(filter=to_filter(FILTERS["depth"])), dict(filter=flt, prep=prep), dict(filter=flt, prep=prep, occlusion=occ)):
            got, kernels = kernels_of(gpu, lambda: rig.grab(frames[0], timestamp=7, cellsize=0.25, attach_flags=flags, **kw))
            want = plain.grab(small_frames[0], timestamp=7, cellsize=0.25, attach_flags=flags, **kw)
            assert_same(gpu, got, want, rig.grid_sensors)
            assert kernels["rgbd_decimate"][1] == 1 and not any(name.startswith("rgbd_holefill") for name in kernels)
            if "prep" not in kw:
                assert want.count() > 0
        assert_cloud(rig.grab(frames[0]), cm.cloud(models, frames[0], k, tables=tables)[1][0], 0, 0.0)
        # three consecutive filtered grabs, the state after each; against the plain rig and against the model
        hists = histories(derived)
        for n in range(3):
            kw = dict(filter=to_filter(FILTERS["depth"]), prep=RgbdPrep(1, 1), occlusion=occ if n == 1 else None, depthfilter=DF)
            got = rig.grab(frames[n], timestamp=n, cellsize=0.5, attach_flags=flags, **kw)
            want = plain.grab(small_frames[n], timestamp=n, cellsize=0.5, attach_flags=flags, **kw)
            assert_same(gpu, got, want, rig.grid_sensors)
            assert_same_history(rig, plain, len(sensors))
            model = cm.cloud(models, frames[n], k, hists, DF, 0, FILTERS["depth"], 1, 1, (1, 0.02) if n == 1 else None, tables)[1]
            assert_cloud(got, model[0], n, 0.5)
            assert len(model[0]) > 0
            assert_history(rig, hists)
        assert any(h.history.any() for h in hists) and any((h.history == 0).any() for h in hists)


# ---- 3: shapes where the decimation kernel can go wrong ----

@pytest.mark.parametrize("k", range(2, 9))
def test_decimation_on_shapes_where_the_kernel_goes_wrong(gpu, k):
    """All in one rig: results of one pixel, one row and one column; result widths of 63, 64, 65 and 129 (the erosion's words, and
    more than one tile of the kernel across); widths and heights that are no multiple of k, whose rest must not be read; a camera
    with no depth at all, one without a hole, and one whose every block has exactly one value, in every position of a block."""
    rng = np.random.default_rng(900 + k)
    shapes = [(k, k), (5 * k + k - 1, k), (k, 7 * k + 1), (63 * k + k - 1, 3 * k + 1), (64 * k, 2 * k), (65 * k + 1, 5 * k + k - 1), (129 * k, 3 * k),
              (9 * k + 1, 4 * k), (20 * k, 3 * k), (k * k + 1, k * k + k - 1)]
    empty, full, single = 7, 8, 9
    pairs = [identity_pair(w, h, i + 1, "d%d" % i) for i, (w, h) in enumerate(shapes)]
    sensors, models = [p[0] for p in pairs], [p[1] for p in pairs]
    frame = []
    for i, s in enumerate(sensors):
        if i == empty:
            depth = np.zeros((s.height, s.width), dtype=np.uint16)
        elif i == single:
            depth = np.zeros((s.height, s.width), dtype=np.uint16)
            for b in range(k * k):                                      # block (b % k, b // k) has its one value at position b of the block
                depth[(b // k) * k + b // k, (b % k) * k + b % k] = 1 + 1000 * b
            depth[:, k * k] = 60000                                     # the rest of the rows and the rest of the columns: never read
            depth[k * k:, :] = 60000
        else:
            depth = banded(rng, s.width, s.height, 20.0, 0.0 if i == full else 0.3, int(rng.choice([1, 1000, 65535 - 80])))
            if i != full:
                depth[rng.random(depth.shape) < 0.4] = 0
        frame.append((depth, colour_for(rng, s)))
    with RgbdRig(sensors, k) as rig:
        pc = rig.grab(frame, None, None, 11, 0.0, flags_of(gpu))
        derived, want = cm.cloud(models, frame, k)
        got = attached(pc, rig.grid_sensors)
        for i, ((rgb, depth), (full_depth, _c)) in enumerate(zip(got, frame)):
            small = cm.decimate(full_depth, k)
            assert depth.shape == small.shape == (shapes[i][1] // k, shapes[i][0] // k) and np.array_equal(depth, small), i
            assert np.array_equal(depth, want[1][i]) and np.array_equal(rgb, want[2][i])
        assert_cloud(pc, want[0], 11, 0.0)
        assert not got[empty][1].any() and got[full][1].all()
        diagonal = got[single][1]                                       # (none of the 60000s, which a mean or a median would show)
        assert diagonal.shape == (k, k) and diagonal.reshape(-1).tolist() == [1 + 1000 * b for b in range(k * k)]
        # with the erosion on the decimated grid's words
        eroded = rig.grab(frame, None, RgbdPrep(1, 1), 12, 0.0, flags_of(gpu))
        want = cm.cloud(models, frame, k, ex=1, ey=1)[1]
        assert_cloud(eroded, want[0], 12, 0.0)
        for (rgb, depth), want_depth in zip(attached(eroded, rig.grid_sensors), want[1]):
            assert np.array_equal(depth, want_depth)


# ---- 4: hole filling ----

FILL_SHAPES = [(1, 1), (1, 7), (7, 1), (63, 5), (64, 64), (65, 66), (513, 3), (1025, 2), (2049, 2), (511, 2), (512, 2)]      # width x height


@pytest.fixture(scope="module")
def fill_rig(gpu):
    """Every camera: about half holes, in runs.  Row 0 of the wide ones (511 .. 2049) has its ONLY depth in column 0, so whatever the
    scan's chunks are the value must be carried through all of them; the last row of 63 x 5, 65 x 66 and 513 x 3 has no depth at all;
    64 x 64 begins every row with holes, has a hole with all eight neighbours present, and holes in its corners."""
    rng = np.random.default_rng(950)
    pairs = [identity_pair(w, h, i + 1, "f%d" % i) for i, (w, h) in enumerate(FILL_SHAPES)]
    sensors, models = [p[0] for p in pairs], [p[1] for p in pairs]
    frame = []
    for (w, h), s in zip(FILL_SHAPES, sensors):
        depth = banded(rng, w, h, 20.0, 0.5, int(rng.choice([1, 1000, 65535 - 80]))) if w * h > 1 else np.array([[0]], dtype=np.uint16)
        if w >= 511:
            depth[0, :] = 0
            depth[0, 0] = 4000 + w
        if (w, h) in ((63, 5), (65, 66), (513, 3)):
            depth[-1, :] = 0
        if (w, h) == (64, 64):
            depth[:, :3] = 0
            depth[9:12, 29:32] = np.array([[11, 12, 13], [14, 0, 15], [16, 17, 18]], dtype=np.uint16) + 2000
            depth[10, 30] = 0
            depth[0, 0] = depth[0, -1] = depth[-1, 0] = depth[-1, -1] = 0
            depth[1, 1], depth[0, -2], depth[-2, 0], depth[-2, -2] = 3001, 3002, 3003, 3004
        frame.append((depth, colour_for(rng, s)))
    with RgbdRig(sensors) as rig:
        yield sensors, models, frame, rig


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_hole_filling_equals_the_model(gpu, fill_rig, mode):
    sensors, models, frame, rig = fill_rig
    (pc, kernels) = kernels_of(gpu, lambda: rig.grab(frame, None, None, 21, 0.0, flags_of(gpu), holefill=RgbdHoleFill(mode)))
    _derived, want = cm.cloud(models, frame, 1, mode=mode)
    got = attached(pc, sensors)
    for i, ((rgb, depth), (source, _c)) in enumerate(zip(got, frame)):
        filled = cm.holefill(source, mode)
        assert np.array_equal(depth, filled), FILL_SHAPES[i]
        assert np.array_equal(depth[source != 0], source[source != 0])                     # a pixel with depth is never changed
        assert np.array_equal(depth, want[1][i]) and np.array_equal(rgb, want[2][i])
    assert_cloud(pc, want[0], 21, 0.0)
    by_shape = {shape: depth for shape, (_rgb, depth) in zip(FILL_SHAPES, got)}
    for w in (511, 512, 513, 1025, 2049):
        row = by_shape[(w, 2 if w != 513 else 3)][0]
        if mode == 1:
            assert (row == 4000 + w).all()                                                  # carried through every chunk
    assert not by_shape[(63, 5)][-1].any() or mode != 1                                     # a row without depth stays so from the left
    square = by_shape[(64, 64)]
    assert square[10, 30] == {1: 2014, 2: 2018, 3: 2011}[mode]
    if mode == 1:
        assert not square[2:-2, :3].any() and kernels["rgbd_holefill_left"][1] == 1 and "rgbd_holefill_around" not in kernels
    else:
        assert (square[0, 0], square[0, -1], square[-1, 0], square[-1, -1]) != (0, 0, 0, 0) and square[0, 0] == 3001
        assert kernels["rgbd_holefill_around"][1] == 2 and "rgbd_holefill_left" not in kernels
    assert by_shape[(1, 1)].tolist() == [[0]]
    assert "rgbd_decimate" not in kernels


def test_no_hole_filling_is_grab_filtered(gpu, raw):
    sensors, _models, frames = raw
    flags = flags_of(gpu)
    flt, prep, occ = to_filter(FILTERS["depth"]).as_struct(), RgbdPrep(1, 2).as_struct(), RgbdOcclusion(1, 0.02).as_struct()
    with RgbdRig(sensors) as rig, RgbdRig(sensors) as plain:
        for n, df in enumerate((None, DF.as_struct(), DF.as_struct())):
            structs = frame_structs(gpu, frames[n])
            want, want_kernels = kernels_of(gpu, lambda: gpu.cwipc_hip_rgbd_rig_grab_filtered(plain._handle(), structs, df, prep, occ, flt, 5, 0.5, flags))
            for holefill in (None, gpu.cwipc_hip_rgbd_holefill(0)):
                if holefill is not None and df is not None:
                    continue            # (a second temporal grab of the frame would move the state on)
                got, kernels = kernels_of(gpu, lambda: gpu.cwipc_hip_rgbd_rig_grab_filled(rig._handle(), structs, holefill, df, prep, occ, flt, 5, 0.5, flags))
                assert want.count() > 0
                assert_same(gpu, got, want, sensors)
                assert {name: c for name, (_ms, c) in kernels.items()} == {name: c for name, (_ms, c) in want_kernels.items()}
                assert not any(name.startswith("rgbd_holefill") or name == "rgbd_decimate" for name in kernels)
            assert_same_history(rig, plain, len(sensors))
        off = rig.grab(frames[0], None, None, 5, 0.5, flags, holefill=RgbdHoleFill(0))
        assert_same(gpu, off, plain.grab(frames[0], None, None, 5, 0.5, flags), sensors)


@pytest.mark.parametrize("mode", [1, 2])
def test_hole_filling_leaves_the_temporal_state_alone(gpu, raw, mode):
    sensors, models, frames = raw
    tables = [lm.ray_table(m.width, m.height, m.fx, m.fy, m.cx, m.cy, m.coeffs) for m in models]
    hists = histories(models)
    with RgbdRig(sensors) as rig, RgbdRig(sensors) as plain:
        for n, frame in enumerate(frames):
            got = rig.grab(frame, None, RgbdPrep(1, 1), n, 0.0, flags_of(gpu), None, DF, RgbdHoleFill(mode))
            without = plain.grab(frame, None, RgbdPrep(1, 1), n, 0.0, flags_of(gpu), None, DF)
            assert_same_history(rig, plain, len(sensors))
            want = cm.cloud(models, frame, 1, hists, DF, mode, ex=1, ey=1, tables=tables)[1]
            assert_history(rig, hists)
            assert_cloud(got, want[0], n, 0.0)
            for (rgb, depth), want_depth, want_rgb in zip(attached(got, sensors), want[1], want[2]):
                assert np.array_equal(depth, want_depth) and np.array_equal(rgb, want_rgb)
            assert got.count() > without.count()


# ---- 5: the Python source ----

def test_rig_source_decimated_and_filled(gpu, raw):
    sensors, models, frames = raw
    k = 2
    derived = [cm.derived_sensor(m, k) for m in models]
    tables = [lm.ray_table(m.width, m.height, m.fx, m.fy, m.cx, m.cy, m.coeffs) for m in derived]
    src = RgbdRigSource(sensors, list(frames), None, RgbdPrep(1, 1), 0.25, 12, depthfilter=DF, decimation=k, holefill=RgbdHoleFill(1))
    assert src.rig.decimation == 2 and src.holefill == RgbdHoleFill(1) and [(g.width, g.height) for g in src.rig.grid_sensors] == [(65, 46)] * 2
    src.request_metadata("rgb")
    src.request_metadata("depth")
    hists = histories(derived)
    for n, frame in enumerate(frames):
        want = cm.cloud(models, frame, k, hists, DF, 1, ex=1, ey=1, tables=tables)[1]
        pc = src.get()
        assert_cloud(pc, want[0], 12 + n, 0.25)
        for (rgb, depth), want_depth, want_rgb in zip(attached(pc, src.rig.grid_sensors), want[1], want[2]):
            assert depth.shape == (46, 65) and np.array_equal(depth, want_depth) and np.array_equal(rgb, want_rgb)
        assert pc.access_metadata().description(1) == "width=65,height=46,bpp=2"
    assert_history(src.rig, hists)
    # the auxiliary operations work on the decimated grid: every point of camera 0 of the last cloud is map2d3d of its pixel
    depth = want[1][0]
    vs, us = np.nonzero(depth)
    points = pc.get_numpy_array()
    points = points[points['tile'] == sensors[0].tile]
    assert len(points) == len(us) > 500
    for j in range(0, len(us), 97):
        out = bytearray(12)
        assert src.auxiliary_operation("map2d3d", struct.pack("ffff", float(sensors[0].tile), float(us[j]), float(vs[j]), float(depth[vs[j], us[j]])), out)
        assert bytes(out) == np.array([points['x'][j], points['y'][j], points['z'][j]], dtype=np.float32).tobytes()
    out = bytearray(8)
    assert src.auxiliary_operation("mapcolordepth", struct.pack("iii", sensors[0].tile, 64, 45), out) and struct.unpack("ii", out) == (64, 45)
    assert not src.auxiliary_operation("mapcolordepth", struct.pack("iii", sensors[0].tile, 65, 45), out)
    assert not src.auxiliary_operation("map2d3d", struct.pack("ffff", float(sensors[0].tile), 100.0, 50.0, 1500.0), bytearray(12))
    assert src.get_tileinfo_dict(1)["cameraMask"] == sensors[0].tile and src.maxtile() == 3
    assert src.get() is None
    src.free()
    plain = RgbdRigSource(sensors, [frames[0]])
    assert plain.rig.decimation == 1 and plain.holefill is None
    plain.free()


# ---- 6: every kind of part of the rig's device block at once ----

def test_every_part_of_the_rigs_block_with_every_stage_on(gpu):
    """One decimated rig whose device block has every kind of part at odd sizes -- a ray table (camera 0's rational lens) and none
    (camera 1's pinhole), depth planes of 33 x 22 and 65 x 4 pixels, colour images of 33 x 21 R, G, B and 64 x 48 B, G, R, A bytes,
    registered images, full-size planes of 67 x 45 and 130 x 9 -- and two consecutive grabs from ordinary memory with every stage on,
    so that every part, the z-buffer, the state (read by the second grab) and the fill plane are written and read: cloud, attached
    images and history against the models."""
    rng = np.random.default_rng(1717)
    intr, cintr = (117.0, 143.0, 62.4, 4.77), (57.6, 70.4, 30.7, 24.0)
    pairs = [raw_pair(67, 45, 33, 21, 2, "odd", 3, rng), pinhole_pair(130, 9, 64, 48, intr, cintr, tile=4, serial="flat", bpp=4)]
    sensors, models = [p[0] for p in pairs], [p[1] for p in pairs]
    df, fill, prep, occ = RgbdDepthFilter(1, 0.5, 20.0, True, 0.4, 20.0, 3), RgbdHoleFill(2), RgbdPrep(1, 1), RgbdOcclusion(1, 0.02)
    derived = [cm.derived_sensor(m, 2) for m in models]
    tables = [lm.ray_table(m.width, m.height, m.fx, m.fy, m.cx, m.cy, m.coeffs) for m in derived]
    hists = histories(derived)
    with RgbdRig(sensors, 2) as rig:
        assert [(g.width, g.height) for g in rig.grid_sensors] == [(33, 22), (65, 4)]
        for n in range(2):
            frame = [(banded(rng, s.width, s.height, 20.0, 0.3, 1500 + 10 * n), colour_for(rng, s)) for s in sensors]
            pc, kernels = kernels_of(gpu, lambda: rig.grab(frame, to_filter(FILTERS["depth"]), prep, 30 + n, 0.25, flags_of(gpu), occ, df, fill))
            want = cm.cloud(models, frame, 2, hists, df, 2, FILTERS["depth"], 1, 1, (1, 0.02), tables)[1]
            assert_cloud(pc, want[0], 30 + n, 0.25)
            assert len(want[0]) > 0 and {m.tile for m in models} == set(np.unique(want[0]['tile']).tolist())   # (both cameras give points)
            for (rgb, depth), want_depth, want_rgb in zip(attached(pc, rig.grid_sensors), want[1], want[2]):
                assert np.array_equal(depth, want_depth) and np.array_equal(rgb, want_rgb)
            assert_history(rig, hists)
            for name in ("rgbd_decimate", "rgbd_temporal", "rgbd_zsplat", "rgbd_register_occluded"):
                assert kernels[name][1] == 1, name
            assert kernels["rgbd_holefill_around"][1] == 2 and "rgbd_register" not in kernels
        assert all((h.history == 3).any() for h in hists)                         # (depth in both grabs: the second one read the first one's state)


# ---- 7: refusals ----

def test_refusals_leave_nothing_behind(gpu, raw):
    sensors, _models, frames = raw
    dll = gpu.util.cwipc_util_dll_load()
    structs = [s.as_struct() for s in sensors]
    narrow = RgbdSensor(5, 9, 5.0, 5.0, 2.0, 4.0, 8, 8, 5.0, 5.0, 4.0, 4.0, serial="narrow")
    low = RgbdSensor(9, 5, 5.0, 5.0, 4.0, 2.0, 8, 8, 5.0, 5.0, 4.0, 4.0, serial="low")
    bad_bpp = RgbdSensor(9, 9, 5.0, 5.0, 4.0, 4.0, 8, 8, 5.0, 5.0, 4.0, 4.0, serial="bpp", bpp=5)
    no_focal = RgbdSensor(9, 9, 0.0, 5.0, 4.0, 4.0, 8, 8, 5.0, 5.0, 4.0, 4.0, serial="focal")
    with RgbdRig(sensors, 2) as rig:
        rig.grab(frames[0], depthfilter=DF, holefill=RgbdHoleFill(2))        # (the state and the scratch plane exist from here on)
        RgbdRig([narrow, low], 5).free()                                       # 5 is the size: grids of one pixel
        before_history = [rig.history(i) for i in range(len(sensors))]
        gc.collect()
        dll.cwipc_hip_synchronize()
        pool, dangling = dll.cwipc_hip_pool_bytes(), gpu.cwipc_dangling_allocations(False)
        with gpu.cwipc_hip_profile() as prof:
            for k in (0, -1, 9, 64):
                with pytest.raises(gpu.CwipcError, match="cwipc_hip_rgbd_rig_create_decimated.*decimation must be between 1 and 8"):
                    gpu.cwipc_hip_rgbd_rig_create_decimated(structs, k)
                with pytest.raises(gpu.CwipcError, match="decimation must be between 1 and 8"):
                    RgbdRig(sensors, k)
            for sensor, k in ((narrow, 6), (low, 6), (narrow, 8), (low, 8)):
                with pytest.raises(gpu.CwipcError, match="camera 1: width and height must be at least the decimation"):
                    RgbdRig([sensors[0], sensor], k)
            # everything rig_create refuses
            with pytest.raises(gpu.CwipcError, match="camera 0: colour_bpp must be 3"):
                RgbdRig([bad_bpp], 2)
            with pytest.raises(gpu.CwipcError, match="camera 0: fx and fy must not be zero"):
                RgbdRig([no_focal], 3)
            with pytest.raises(gpu.CwipcError, match="ncam must be at least 1"):
                gpu.cwipc_hip_rgbd_rig_create_decimated([], 2)
            with pytest.raises(gpu.CwipcError):
                gpu.cwipc_hip_rgbd_rig_grid_sensor(rig._handle(), 2)
            with pytest.raises(gpu.CwipcError):
                gpu.cwipc_hip_rgbd_rig_grid_sensor(None, 0)
            # a hole-fill mode outside 0 .. 3, with everything else in order
            for mode in (-1, 4, 99):
                with pytest.raises(gpu.CwipcError, match="cwipc_hip_rgbd_rig_grab_filled.*holefill: mode must be between 0 and 3"):
                    rig.grab(frames[1], depthfilter=DF, holefill=RgbdHoleFill(mode))
            # everything grab_filtered refuses, through the new entry
            with pytest.raises(gpu.CwipcError, match="temporal_persistency must be between 0 and 8"):
                rig.grab(frames[1], depthfilter=RgbdDepthFilter(temporal_persistency=9), holefill=RgbdHoleFill(1))
            with pytest.raises(gpu.CwipcError, match="between 0 and 32"):
                rig.grab(frames[1], None, RgbdPrep(33, 0), holefill=RgbdHoleFill(1))
            with pytest.raises(gpu.CwipcError, match="NULL argument"):
                gpu.cwipc_hip_rgbd_rig_grab_filled(None, frame_structs(gpu, frames[1]), gpu.cwipc_hip_rgbd_holefill(1))
            # a frame of the decimated size is not this rig's frame
            small = [(np.ascontiguousarray(d[:46, :65]), c) for d, c in frames[1]]
            with pytest.raises(ValueError, match="depth must be a contiguous uint16"):
                rig.grab(small)
            gc.collect()
        assert prof.kernels == {}
        assert dll.cwipc_hip_pool_bytes() == pool and gpu.cwipc_dangling_allocations(False) == dangling
        for (value, history), (was_value, was_history) in zip([rig.history(i) for i in range(len(sensors))], before_history):
            assert np.array_equal(value.view(np.uint64), was_value.view(np.uint64)) and np.array_equal(history, was_history) and history.any()
        # ... and the rig still works
        assert rig.grab(frames[1], depthfilter=DF, holefill=RgbdHoleFill(3)).count() > 0
