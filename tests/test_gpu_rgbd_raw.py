"""The RGB-D source's raw entry (cwipc_hip_rgbd_rig_grab) on the GPU: a degenerate rig against cwipc_hip_from_rgbd byte for byte, the
erosion against the model on word seams and image borders, raw sensor pairs with rational lenses against the numpy model
(tests/rgbd_lens_model.py) byte for byte, an analytic scene that needs no model, the attached images, the mappings and the errors."""
import ctypes
import gc
import struct

import numpy as np
import pytest

import rgbd_lens_model as lm
import rgbd_model as rm
from test_gpu_rgbd import FILTERS, assert_cloud, camera_pair, images, to_filter
from cwipc_util_amd.rgbd import RgbdPrep, RgbdRig, RgbdRigSource, RgbdSensor, from_rgbd

pytestmark = pytest.mark.gpu

DEPTH_LENS = (4.9, 3.1, 1e-4, -5e-5, 0.16, 5.2, 4.8, 0.85)                                  # of a 640 x 576 image, f 504, centre 320, 330
COLOUR_LENS = (0.4569, -2.7217, 4.7e-4, -1.6e-4, 1.5964, 0.3335, -2.5460, 1.5223)           # of a 1280 x 720 image, f 607, centre 638, 367
SIDEWAYS = np.identity(4)
SIDEWAYS[0, 3] = -0.032


def degenerate(cam):
    """The raw sensor that an aligned RgbdCamera is: no lens, the colour side equal to the depth side, no offset between them."""
    return RgbdSensor(cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy, cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy,
                      depth_scale=cam.depth_scale, trafo=cam.trafo, tile=cam.tile, serial=cam.serial, bpp=cam.bpp)


def raw_pair(width, height, cwidth, cheight, tile, serial, bpp, rng, d2c=SIDEWAYS, trafo=None):
    """The same raw sensor for the library and for the model: the rational depth and colour lenses scaled to the image sizes."""
    fx, fy, cx, cy = 504.0 * width / 640, 504.0 * height / 576, 320.0 * width / 640, 330.0 * height / 576
    cfx, cfy, ccx, ccy = 607.0 * cwidth / 1280, 607.0 * cheight / 720, 638.0 * cwidth / 1280, 367.0 * cheight / 720
    m = rm.random_rigid(rng, 1.0) if trafo is None else trafo
    return (RgbdSensor(width, height, fx, fy, cx, cy, cwidth, cheight, cfx, cfy, ccx, ccy, DEPTH_LENS, COLOUR_LENS, d2c, 0.001, m, tile, serial, bpp),
            lm.Sensor(width, height, fx, fy, cx, cy, DEPTH_LENS, 0.001, (cwidth, cheight), bpp, (cfx, cfy, ccx, ccy), COLOUR_LENS, d2c, m, tile))


def raw_images(width, height, cwidth, cheight, bpp, rng, zeros=0.02):
    depth = rng.integers(300, 4000, (height, width)).astype(np.uint16)
    depth[rng.random((height, width)) < zeros] = 0
    return depth, rng.integers(0, 256, (cheight, cwidth, bpp)).astype(np.uint8)


def cloud_bytes(pc):
    return pc.get_numpy_array().tobytes()


# ---- 4: a degenerate rig is the aligned path ----

@pytest.fixture(scope="module")
def three(gpu):
    """test_gpu_rgbd.py's three cameras and frame, and the rig of their degenerate sensors."""
    rng = np.random.default_rng(101)
    pairs = [camera_pair(1, 1, 1, "one", 3, rng), camera_pair(67, 45, 2, "s67", 3, rng), camera_pair(64, 48, 4, "s64", 4, rng)]
    frame = [images(1, 1, 3, rng, zeros=0.0), images(67, 45, 3, rng), images(64, 48, 4, rng)]
    cams = [p[0] for p in pairs]
    with RgbdRig([degenerate(c) for c in cams]) as rig:
        yield cams, frame, rig


@pytest.mark.parametrize("name", list(FILTERS))
def test_degenerate_rig_equals_the_aligned_path(gpu, three, name):
    cams, frame, rig = three
    flt = to_filter(FILTERS[name])
    want = from_rgbd(cams, frame, flt, 424242, 0.005)
    got = rig.grab(frame, flt, None, 424242, 0.005)
    assert want.count() > 0 and got.count() == want.count()
    assert cloud_bytes(got) == cloud_bytes(want)
    assert got.timestamp() == want.timestamp() and got.cellsize() == want.cellsize()
    assert gpu.get_tiles_used(got) == gpu.get_tiles_used(want)
    assert cloud_bytes(rig.grab(frame, flt, RgbdPrep(0, 0), 424242, 0.005)) == cloud_bytes(want)


# ---- 5: erosion ----

EROSION_SHAPES = [(1, 1), (5, 3), (67, 45), (130, 70)]


@pytest.fixture(scope="module")
def erosion_rig(gpu):
    """Four degenerate sensors of the erosion shapes (every depth pixel keeps its colour: the attached depth image is the eroded
    one), and a frame: random holes, and in the 130 x 70 image holes on the word seams and on the image's borders."""
    rng = np.random.default_rng(55)
    cams = [camera_pair(w, h, 1 << k, "e%d" % k, 3 + (k & 1), rng)[0] for k, (w, h) in enumerate(EROSION_SHAPES)]
    frame = []
    for k, (w, h) in enumerate(EROSION_SHAPES):
        depth, colour = images(w, h, 3 + (k & 1), rng, zeros=0.004 if w > 5 else 0.0)
        frame.append((depth, colour))
    seams = frame[3][0]
    seams[:] = rng.integers(300, 4000, seams.shape)
    for n, u in enumerate((63, 64, 65, 127, 128, 129)):
        seams[5 + 10 * n, u] = 0
    seams[0, 20] = seams[0, 64] = seams[69, 100] = seams[69, 129] = seams[30, 0] = 0
    with RgbdRig([degenerate(c) for c in cams]) as rig:
        yield cams, frame, rig


def eroded_images(gpu, cams, pc):
    meta = pc.access_metadata()
    assert [meta.name(i) for i in range(meta.count())] == ["depth." + c.serial for c in cams]
    return [np.frombuffer(bytes(meta.data(i)), dtype=np.uint16).reshape(c.height, c.width) for i, c in enumerate(cams)]


def check_erosion(gpu, cams, frame, rig, ex, ey):
    pc = rig.grab(frame, None, RgbdPrep(ex, ey), attach_flags=gpu.CWIPC_HIP_RGBD_ATTACH_DEPTH)
    want = [lm.erode(depth, ex, ey) for depth, _colour in frame]
    got = eroded_images(gpu, cams, pc)
    for k in range(len(cams)):
        assert np.array_equal(got[k], want[k]), (k, ex, ey)
    # ... and the cloud is the aligned path's on the eroded images
    assert cloud_bytes(pc) == cloud_bytes(from_rgbd(cams, [(w, colour) for w, (_d, colour) in zip(want, frame)]))
    return want


@pytest.mark.parametrize("ex,ey", [(0, 3), (3, 0), (1, 1), (32, 32), (7, 0), (7, 1)])
def test_erosion_equals_the_model(gpu, erosion_rig, ex, ey):
    cams, frame, rig = erosion_rig
    want = check_erosion(gpu, cams, frame, rig, ex, ey)
    if (ex, ey) == (1, 1):
        assert 0 < np.count_nonzero(want[3]) < np.count_nonzero(frame[3][0])      # (it erodes, and not everything)
        assert want[3][1, 20] == 0 and want[3][1, 64] == 0 and want[3][68, 129] == 0 and want[3][30, 1] == 0
    if ex == 7:
        assert np.array_equal(want[1], frame[1][0])                               # 5 x 3 without a hole: the borders do not erode


def test_erosion_all_valid_all_zero_and_an_empty_middle(gpu, erosion_rig):
    cams, frame, rig = erosion_rig
    rng = np.random.default_rng(56)
    full = [(rng.integers(1, 65536, d.shape).astype(np.uint16), c) for d, c in frame]
    for ex, ey in ((1, 1), (32, 32)):
        want = check_erosion(gpu, cams, full, rig, ex, ey)
        assert all(np.array_equal(w, d) for w, (d, _c) in zip(want, full))
    empty = [(np.zeros_like(d), c) for d, c in frame]
    pc = rig.grab(empty, None, RgbdPrep(2, 2), attach_flags=gpu.CWIPC_HIP_RGBD_ATTACH_DEPTH)
    assert pc.count() == 0 and not any(img.any() for img in eroded_images(gpu, cams, pc))
    middle = [full[0], full[1], empty[2], full[3]]
    for ex, ey in ((1, 1), (3, 0)):
        check_erosion(gpu, cams, middle, rig, ex, ey)
    pc = rig.grab(middle, None, RgbdPrep(1, 1))
    assert gpu.get_tiles_used(pc) == [1, 2, 8] and pc.count() == 1 + 15 + 130 * 70


def test_erosion_out_of_range_is_an_error(gpu, erosion_rig):
    cams, frame, rig = erosion_rig
    gc.collect()
    before = gpu.cwipc_dangling_allocations(False)
    for prep in (RgbdPrep(33, 0), RgbdPrep(0, -1), RgbdPrep(-1, 33)):
        with pytest.raises(gpu.CwipcError, match="between 0 and 32"):
            rig.grab(frame, None, prep)
    assert gpu.cwipc_dangling_allocations(False) == before
    assert rig.grab(frame, None, RgbdPrep(32, 0)).count() >= 0


# ---- 6: raw sensor pairs against the model ----

@pytest.fixture(scope="module")
def raw(gpu):
    """Two raw sensors, depth 67 x 45 and colour 101 x 77, R, G, B and B, G, R, A; their model twins with the model's own ray
    tables; two frames; the rig."""
    rng = np.random.default_rng(202)
    pairs = [raw_pair(67, 45, 101, 77, 2, "raw3", 3, rng), raw_pair(67, 45, 101, 77, 4, "raw4", 4, rng)]
    frames = [[raw_images(67, 45, 101, 77, bpp, rng) for bpp in (3, 4)] for _ in range(2)]
    sensors, models = [p[0] for p in pairs], [p[1] for p in pairs]
    tables = [lm.ray_table(m.width, m.height, m.fx, m.fy, m.cx, m.cy, m.coeffs) for m in models]
    with RgbdRig(sensors) as rig:
        yield sensors, models, tables, frames, rig


def test_ray_table_is_the_models(gpu, raw):
    sensors, models, tables, _frames, rig = raw
    for i in range(2):
        got = rig.ray_table(i)
        assert got.shape == (45, 67, 2) and not np.isnan(got).any()
        assert np.array_equal(got.view(np.uint64), tables[i].view(np.uint64))
    with pytest.raises(IndexError):
        rig.ray_table(2)


@pytest.mark.parametrize("name", list(FILTERS))
def test_raw_rig_against_the_model(gpu, raw, name):
    sensors, models, tables, frames, rig = raw
    flt = FILTERS[name]
    want, _depths, _colours = lm.cloud(models, frames[0], flt, 1, 2, tables)
    everything = lm.cloud(models, frames[0], rm.Filter(), 1, 2, tables)[0]
    assert 500 < len(everything) < int(sum((d != 0).sum() for d, _c in frames[0]))     # erosion and registration drop some, keep many
    if name != "off":
        assert 0 < len(want) < len(everything)
    assert_cloud(rig.grab(frames[0], to_filter(flt), RgbdPrep(1, 2), 31337, 0.01), want, 31337, 0.01)


def test_two_frames_through_one_rig_and_nothing_dangles(gpu, raw):
    """cwipc_dangling_allocations counts every live cloud of the process, other test modules' fixtures included, so "0 after the
    frees" is taken against the count before the first grab: the two clouds show in it while they live and nothing of theirs stays."""
    sensors, models, tables, frames, rig = raw
    gc.collect()
    before = gpu.cwipc_dangling_allocations(False)
    clouds = [rig.grab(frame, None, RgbdPrep(1, 2), 5 + i) for i, frame in enumerate(frames)]
    wants = [lm.cloud(models, frame, rm.Filter(), 1, 2, tables)[0] for frame in frames]
    assert wants[0].tobytes() != wants[1].tobytes()
    for i in range(2):
        assert_cloud(clouds[i], wants[i], 5 + i, 0.0)
    assert gpu.cwipc_dangling_allocations(False) - before == 2
    for pc in clouds:
        pc.free(force=True)
    del clouds
    assert gpu.cwipc_dangling_allocations(False) - before == 0


def test_raw_rig_page_locked_images(gpu, raw):
    sensors, models, tables, frames, rig = raw
    keep = []

    def pin(a):
        block = gpu.cwipc_hip_pinned_points((a.nbytes + 15) // 16)
        keep.append(block)
        out = block.view(np.uint8)[:a.nbytes].view(a.dtype).reshape(a.shape)
        out[...] = a
        return out

    frame = [(pin(d), pin(c)) for d, c in frames[1]]
    want = lm.cloud(models, frames[1], FILTERS["all"], 1, 2, tables)[0]
    assert_cloud(rig.grab(frame, to_filter(FILTERS["all"]), RgbdPrep(1, 2), 9, 0.0), want, 9, 0.0)


def test_every_point_behind_the_colour_camera(gpu, raw):
    """depth_to_colour turned half round about y: Pz < 0 everywhere, no pixel has a colour, the cloud is empty and is a cloud."""
    sensors, models, _tables, frames, _rig = raw
    about = np.diag([-1.0, 1.0, -1.0, 1.0])
    turned = [RgbdSensor(**{**s.__dict__, "depth_to_colour": about}) for s in sensors]
    assert len(lm.cloud([m._replace(depth_to_colour=about) for m in models], frames[0])[0]) == 0
    with RgbdRig(turned) as rig:
        pc = rig.grab(frames[0], None, None, 77, 0.25, gpu.CWIPC_HIP_RGBD_ATTACH_DEPTH | gpu.CWIPC_HIP_RGBD_ATTACH_RGB)
        assert pc.count() == 0 and len(pc.get_numpy_array()) == 0 and pc.timestamp() == 77 and pc.cellsize() == 0.25
        assert gpu.get_tiles_used(pc) == []
        meta = pc.access_metadata()
        assert meta.count() == 4 and not any(any(bytes(meta.data(i))) for i in range(4))


def test_vga_raw_camera_on_the_three_launch_flow(gpu):
    """640 x 480 = 307 200 depth pixels: more than the 256 k up to which the count kernel's last workgroup scans.  Colour 701 x 523."""
    rng = np.random.default_rng(8)
    sensor, model = raw_pair(640, 480, 701, 523, 8, "vga", 3, rng)
    frame = [raw_images(640, 480, 701, 523, 3, rng, zeros=0.001)]
    want = lm.cloud([model], frame, rm.Filter(), 1, 1)[0]
    assert 640 * 480 > 262144 and len(want) > 200000
    with RgbdRig([sensor]) as rig:
        assert_cloud(rig.grab(frame, None, RgbdPrep(1, 1), 5, 0.0), want, 5, 0.0)
        flt = FILTERS["all"]
        assert_cloud(rig.grab(frame, to_filter(flt), RgbdPrep(1, 1), 6, 0.0), lm.cloud([model], frame, flt, 1, 1)[0], 6, 0.0)


# ---- 7: an analytic scene ----

def test_analytic_plane_with_a_baseline(gpu):
    """Pinhole sensors, the colour camera b to the side, a plane of constant depth z, a colour image whose pixel (uc, vc) says
    (uc, vc).  Depth pixel (u, v) is seen by the colour camera at fxc ((u - cx)/fx + b/z) + cxc (and alike in v, without b): the
    colour a point carries must name a pixel within 0.5 + 1e-6 of that -- nearest-pixel rounding, and slack for the order of the
    float64 evaluation -- and a pixel is in the cloud if that position is inside the colour image, absent if it is outside."""
    w, h, fx, fy, cx, cy = 67, 45, 60.0, 58.0, 33.2, 22.4
    wc, hc, fxc, fyc, cxc, cyc = 300, 200, 310.0, 305.0, 149.3, 101.7
    b, d, scale = 0.05, 1250, 0.001
    z = d * scale
    d2c = np.identity(4)
    d2c[0, 3] = b
    vc_grid, uc_grid = np.meshgrid(np.arange(hc), np.arange(wc), indexing='ij')
    colour = np.stack([uc_grid & 255, vc_grid & 255, (uc_grid >> 8) | ((vc_grid >> 8) << 4)], axis=-1).astype(np.uint8)
    depth = np.full((h, w), d, dtype=np.uint16)
    sensor = RgbdSensor(w, h, fx, fy, cx, cy, wc, hc, fxc, fyc, cxc, cyc, depth_to_colour=d2c, depth_scale=scale, tile=1, serial="plane")
    with RgbdRig([sensor]) as rig:
        got = rig.grab([(depth, colour)]).get_numpy_array()
    # which pixel each point came from, from its own coordinates (the world is the camera's frame)
    u = np.rint(got['x'].astype(np.float64) / got['z'] * fx + cx).astype(np.int64)
    v = np.rint(got['y'].astype(np.float64) / got['z'] * fy + cy).astype(np.int64)
    assert (np.abs(got['z'] - np.float32(z)) < 1e-6).all()
    assert np.array_equal(np.lexsort((u, v)), np.arange(len(got)))             # row-major order, no pixel twice
    assert len(set(zip(u.tolist(), v.tolist()))) == len(got)
    au = fxc * ((u - cx) / fx + b / z) + cxc
    av = fyc * ((v - cy) / fy) + cyc
    uc = got['r'].astype(np.int64) | ((got['b'].astype(np.int64) & 15) << 8)
    vc = got['g'].astype(np.int64) | ((got['b'].astype(np.int64) >> 4) << 8)
    err = max(np.abs(uc - au).max(), np.abs(vc - av).max())
    print("worst colour coordinate error %.6f px" % err)
    assert err <= 0.5 + 1e-6
    # presence
    vv, uu = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    pu = fxc * ((uu - cx) / fx + b / z) + cxc
    pv = fyc * ((vv - cy) / fy) + cyc
    present = np.zeros((h, w), dtype=bool)
    present[v, u] = True
    outside = (pu < -0.5 - 1e-6) | (pu > wc - 0.5 + 1e-6) | (pv < -0.5 - 1e-6) | (pv > hc - 0.5 + 1e-6)
    inside = (pu > -0.5 + 1e-6) & (pu < wc - 0.5 - 1e-6) & (pv > -0.5 + 1e-6) & (pv < hc - 0.5 - 1e-6)
    assert outside.any() and inside.any()
    assert not present[outside].any() and present[inside].all()


# ---- 8: metadata, mappings, errors ----

def test_attached_images_and_mappings(gpu, raw):
    sensors, models, tables, frames, _rig = raw
    want, depths, colours = lm.cloud(models, frames[0], rm.Filter(), 1, 2, tables)
    src = RgbdRigSource(sensors, [frames[0], frames[0]], None, RgbdPrep(1, 2))
    pc = src.get()
    assert pc.access_metadata().count() == 0 and pc.get_numpy_array().tobytes() == want.tobytes()
    src.request_metadata("rgb")
    src.request_metadata("depth")
    pc = src.get()
    meta = pc.access_metadata()
    assert [meta.name(i) for i in range(meta.count())] == ["rgb.raw3", "depth.raw3", "rgb.raw4", "depth.raw4"]
    assert [meta.description(i) for i in range(meta.count())] == ["width=67,height=45,bpp=3", "width=67,height=45,bpp=2"] * 2
    assert meta.get_image_description(2) == {"width": 67, "height": 45, "bpp": 3, "image_format": "RGB8"}
    for i in range(2):
        assert bytes(meta.data(2 * i)) == colours[i].tobytes() and bytes(meta.data(2 * i + 1)) == depths[i].tobytes()
        assert (colours[i][depths[i] == 0] == 0).all()                            # black where there is no point
        eroded = lm.erode(frames[0][i][0], 1, 2)
        assert ((depths[i] == eroded) | (depths[i] == 0)).all() and 0 < np.count_nonzero(depths[i]) < np.count_nonzero(eroded)
    by_serial = meta.get_all_images("raw4")
    assert np.array_equal(by_serial["depth."], depths[1]) and np.array_equal(by_serial["rgb."], colours[1][:, :, ::-1])
    assert src.serial_dict() == {2: "raw3", 4: "raw4"} and src.maxtile() == 3
    # map2d3d reproduces the cloud's points bit for bit, through the rig and through the source
    got = pc.get_numpy_array()
    first = got[got['tile'] == 2]
    vs, us = np.nonzero(depths[0])
    assert len(first) == len(us) > 300
    cloud_bits = np.stack([first['x'], first['y'], first['z']], axis=1).view(np.uint32)
    direct = np.float32([src.rig.map2d3d(0, int(u), int(v), int(depths[0][v, u])) for u, v in zip(us, vs)])
    assert np.array_equal(direct.view(np.uint32), cloud_bits)
    out = bytearray(12)
    for i in (0, len(us) // 2, len(us) - 1):
        assert src.auxiliary_operation("map2d3d", struct.pack("ffff", 2.0, float(us[i]), float(vs[i]), float(depths[0][vs[i], us[i]])), out) is True
        assert np.array_equal(np.float32(struct.unpack("fff", out)).view(np.uint32), cloud_bits[i])
    assert src.auxiliary_operation("map2d3d", struct.pack("ffff", 2.0, 3.0, 3.0, 0.0), out) is False            # no depth
    assert src.auxiliary_operation("map2d3d", struct.pack("ffff", 2.0, 67.0, 3.0, 900.0), out) is False         # outside
    assert src.auxiliary_operation("map2d3d", struct.pack("ffff", 3.0, 3.0, 3.0, 900.0), out) is False          # no such tile
    pixel = bytearray(8)
    for u, v in ((0, 0), (66, 44), (30, 7)):
        assert src.auxiliary_operation("mapcolordepth", struct.pack("iii", 4, u, v), pixel) is True and struct.unpack("ii", pixel) == (u, v)
    for u, v in ((67, 0), (0, 45), (-1, 3), (3, -1), (100, 76)):
        assert src.auxiliary_operation("mapcolordepth", struct.pack("iii", 4, u, v), pixel) is False
    assert src.auxiliary_operation("mapcolordepth", struct.pack("iii", 3, 0, 0), pixel) is False
    assert src.auxiliary_operation("nosuchop", b"", bytearray(0)) is False
    assert src.get() is None and src.eof()
    src.free()


def test_a_pixel_without_a_ray_gives_no_point(gpu):
    """The folded lens (k1 = -1.5): its table has NaN entries; those pixels are cleared in the attached depth image, map2d3d says
    false for them, and the cloud is the model's."""
    rng = np.random.default_rng(12)
    k = (-1.5, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
    sensor = RgbdSensor(67, 45, 31.0, 31.0, 33.0, 22.0, 67, 45, 31.0, 31.0, 33.0, 22.0, coeffs=k, tile=1, serial="fold")
    model = lm.Sensor(67, 45, 31.0, 31.0, 33.0, 22.0, k, 0.001, (67, 45), 3, (31.0, 31.0, 33.0, 22.0), lm.PINHOLE, np.identity(4), np.identity(4), 1)
    frame = [raw_images(67, 45, 67, 45, 3, rng, zeros=0.0)]
    with RgbdRig([sensor]) as rig:
        table = rig.ray_table(0)
        nan = np.isnan(table[..., 0])
        assert nan.any() and not nan.all()
        want, depths, _colours = lm.cloud([model], frame)
        pc = rig.grab(frame, attach_flags=gpu.CWIPC_HIP_RGBD_ATTACH_DEPTH)
        assert_cloud(pc, want, 0, 0.0)
        assert bytes(pc.access_metadata().data(0)) == depths[0].tobytes() and not depths[0][nan].any()
        v, u = (int(c[0]) for c in np.nonzero(nan))
        assert rig.map2d3d(0, u, v, 900) is None


def test_create_and_grab_errors_leave_nothing_behind(gpu, raw):
    sensors, _models, _tables, frames, rig = raw
    gc.collect()
    before = gpu.cwipc_dangling_allocations(False)

    def broken(**changes):
        s = sensors[0].as_struct()
        for name, value in changes.items():
            setattr(s, name, value)
        return s

    def with_entry(name, index, value):
        s = sensors[0].as_struct()
        getattr(s, name)[index] = value
        return s

    cases = [([], "ncam must be at least 1"), ([broken(width=0)], "at least 1"), ([broken(height=-3)], "at least 1"), ([broken(colour_width=0)], "at least 1"),
             ([broken(colour_height=0)], "at least 1"), ([broken(colour_bpp=2)], "colour_bpp must be 3"), ([broken(colour_bpp=5)], "colour_bpp must be 3"),
             ([broken(fx=float('nan'))], "must be finite"), ([broken(colour_cy=float('inf'))], "must be finite"),
             ([broken(depth_scale=float('-inf'))], "must be finite"), ([with_entry("coeffs", 3, float('nan'))], "must be finite"),
             ([with_entry("colour_coeffs", 7, float('inf'))], "must be finite"), ([with_entry("depth_to_colour", 5, float('nan'))], "must be finite"),
             ([with_entry("trafo", 11, float('inf'))], "must be finite"), ([broken(fy=0.0)], "must not be zero"), ([broken(colour_fx=0.0)], "must not be zero"),
             ([broken(width=65536, height=32768)], "more than 2\\^31 - 1 pixels"), ([broken(colour_width=65536, colour_height=32768)], "more than 2\\^31 - 1 pixels"),
             ([sensors[0].as_struct(), broken(colour_bpp=7)], "camera 1: colour_bpp must be 3")]
    for structs, text in cases:
        with pytest.raises(gpu.CwipcError, match=text):
            gpu.cwipc_hip_rgbd_rig_create(structs)
    # a depth_to_colour that is no rigid matrix is accepted: it is not judged
    sheared = with_entry("depth_to_colour", 1, 0.3)
    sheared.depth_to_colour[0] = 1.7
    handle = gpu.cwipc_hip_rgbd_rig_create([sheared])
    assert handle
    gpu.cwipc_hip_rgbd_rig_free(handle)
    dll = gpu.cwipc_util_dll_load()
    err = ctypes.c_char_p()
    assert not dll.cwipc_hip_rgbd_rig_create(None, 1, ctypes.byref(err)) and b"NULL argument" in err.value
    assert not dll.cwipc_hip_rgbd_rig_create(None, 1, None) and b"NULL argument" in dll.cwipc_hip_last_error()
    dll.cwipc_hip_rgbd_rig_free(None)
    # grab
    good = [gpu.cwipc_hip_rgbd_frame(d.ctypes.data, c.ctypes.data) for d, c in frames[0]]
    for bad in ([gpu.cwipc_hip_rgbd_frame(None, good[0].colour), good[1]], [good[0], gpu.cwipc_hip_rgbd_frame(good[1].depth, None)]):
        with pytest.raises(gpu.CwipcError, match="NULL argument"):
            gpu.cwipc_hip_rgbd_rig_grab(rig._handle(), bad)
    with pytest.raises(gpu.CwipcError, match="NULL argument"):
        gpu.cwipc_hip_rgbd_rig_grab(rig._handle(), [])
    with pytest.raises(gpu.CwipcError, match="NULL argument"):
        gpu.cwipc_hip_rgbd_rig_grab(None, good)
    assert not dll.cwipc_hip_rgbd_rig_grab(None, None, None, None, 0, 0.0, 0, None) and b"NULL argument" in dll.cwipc_hip_last_error()
    no_serial = gpu.cwipc_hip_rgbd_rig_create([broken(serial=None)])
    try:
        with pytest.raises(gpu.CwipcError, match="NULL argument"):
            gpu.cwipc_hip_rgbd_rig_grab(no_serial, good[:1], attach_flags=gpu.CWIPC_HIP_RGBD_ATTACH_DEPTH)
        assert gpu.cwipc_hip_rgbd_rig_grab(no_serial, good[:1]).count() > 0
    finally:
        gpu.cwipc_hip_rgbd_rig_free(no_serial)
    assert dll.cwipc_hip_rgbd_rig_map2d3d(None, 0, 1, 1, 900, (ctypes.c_float * 3)()) == 0
    assert rig.map2d3d(2, 1, 1, 900) is None and rig.map2d3d(-1, 1, 1, 900) is None and rig.mapcolordepth(2, 1, 1) is None
    assert not dll.cwipc_hip_rgbd_rig_ray_table(None, 0) and not dll.cwipc_hip_rgbd_rig_ray_table(rig._handle(), 2)
    with pytest.raises(ValueError):
        rig.grab(frames[0][:1])
    with pytest.raises(ValueError):
        rig.grab([(frames[0][0][0], frames[0][0][1][:50]), frames[0][1]])
    gc.collect()
    assert gpu.cwipc_dangling_allocations(False) == before
    # ... and the rig still works afterwards
    assert rig.grab(frames[0]).count() > 0
