"""The raw entry's occlusion test (cwipc_hip_rgbd_rig_grab_occluded) on the GPU, byte for byte against the numpy model
(tests/rgbd_occlusion_model.py): the NULL occlusion against cwipc_hip_rgbd_rig_grab, the window rule an identity rig collapses to
against a brute-force scan written here, a finer colour grid that leaks at splat 0 and does not at splat 1, hundreds of candidates on
one cell in two arrival orders, squares clipped at every border, cameras that must not mix, a z-buffer that must be reset, lenses,
BGRA, erosion, filters, page-locked images and the three-launch flow, the attached images, the errors and the Python surface."""
import gc
import math

import numpy as np
import pytest

import rgbd_lens_model as lm
import rgbd_model as rm
import rgbd_occlusion_model as om
from test_gpu_rgbd import FILTERS, assert_cloud, to_filter
from test_gpu_rgbd_raw import raw_images, raw_pair
from cwipc_util_amd.rgbd import RgbdOcclusion, RgbdPrep, RgbdRig, RgbdRigSource, RgbdSensor

pytestmark = pytest.mark.gpu


def cloud_bytes(pc):
    return pc.get_numpy_array().tobytes()


def frame_structs(gpu, frame):
    return [gpu.cwipc_hip_rgbd_frame(d.ctypes.data, c.ctypes.data) for d, c in frame]


def pinhole_pair(width, height, cwidth, cheight, intr, cintr, d2c=None, tile=1, serial="cam", bpp=3):
    """A sensor without lenses for the library and for the model, the world being the depth camera's frame."""
    d2c = np.identity(4) if d2c is None else d2c
    return (RgbdSensor(width, height, *intr, cwidth, cheight, *cintr, depth_to_colour=d2c, tile=tile, serial=serial, bpp=bpp),
            lm.Sensor(width, height, *intr, lm.PINHOLE, 0.001, (cwidth, cheight), bpp, cintr, lm.PINHOLE, d2c, np.identity(4), tile))


def attached(pc, sensors):
    """[(registered rgb, depth)] per camera of a cloud grabbed with both attach flags."""
    meta = pc.access_metadata()
    assert meta.count() == 2 * len(sensors)
    out = []
    for i, s in enumerate(sensors):
        assert meta.name(2 * i) == "rgb." + s.serial and meta.name(2 * i + 1) == "depth." + s.serial
        out.append((np.frombuffer(bytes(meta.data(2 * i)), dtype=np.uint8).reshape(s.height, s.width, 3),
                    np.frombuffer(bytes(meta.data(2 * i + 1)), dtype=np.uint16).reshape(s.height, s.width)))
    return out


def check_against_model(gpu, rig, sensors, models, frame, occ, flt=rm.Filter(), ex=0, ey=0, tables=None, grab_frame=None):
    """One occluded grab with both images attached: cloud, depth images and registered images are the model's.  Returns the model's."""
    want = om.cloud(models, frame, flt, ex, ey, tables, occ.splat, occ.margin)
    pc = rig.grab(frame if grab_frame is None else grab_frame, to_filter(flt), RgbdPrep(ex, ey), 4711, 0.5,
                  gpu.CWIPC_HIP_RGBD_ATTACH_RGB | gpu.CWIPC_HIP_RGBD_ATTACH_DEPTH, occ)
    assert_cloud(pc, want[0], 4711, 0.5)
    for (rgb, depth), want_depth, want_rgb in zip(attached(pc, sensors), want[1], want[2]):
        assert np.array_equal(depth, want_depth) and np.array_equal(rgb, want_rgb)
    return want


# ---- 1: no occlusion through the new entry ----

@pytest.fixture(scope="module")
def raw(gpu):
    """test_gpu_rgbd_raw.py's two raw sensors (depth 67 x 45, colour 101 x 77, rational lenses, R, G, B and B, G, R, A), their model
    twins and ray tables, two frames, the rig."""
    rng = np.random.default_rng(202)
    pairs = [raw_pair(67, 45, 101, 77, 2, "raw3", 3, rng), raw_pair(67, 45, 101, 77, 4, "raw4", 4, rng)]
    frames = [[raw_images(67, 45, 101, 77, bpp, rng) for bpp in (3, 4)] for _ in range(2)]
    sensors, models = [p[0] for p in pairs], [p[1] for p in pairs]
    tables = [lm.ray_table(m.width, m.height, m.fx, m.fy, m.cx, m.cy, m.coeffs) for m in models]
    with RgbdRig(sensors) as rig:
        yield sensors, models, tables, frames, rig


@pytest.mark.parametrize("name", list(FILTERS))
def test_null_occlusion_is_rig_grab(gpu, raw, name):
    sensors, _models, _tables, frames, rig = raw
    flt = to_filter(FILTERS[name]).as_struct()
    prep = RgbdPrep(1, 2).as_struct()
    flags = gpu.CWIPC_HIP_RGBD_ATTACH_RGB | gpu.CWIPC_HIP_RGBD_ATTACH_DEPTH
    structs = frame_structs(gpu, frames[0])
    want = gpu.cwipc_hip_rgbd_rig_grab(rig._handle(), structs, prep, flt, 99, 0.125, flags)
    got = gpu.cwipc_hip_rgbd_rig_grab_occluded(rig._handle(), structs, prep, None, flt, 99, 0.125, flags)
    assert want.count() > 0 and cloud_bytes(got) == cloud_bytes(want)
    assert got.timestamp() == 99 and got.cellsize() == 0.125 and gpu.get_tiles_used(got) == gpu.get_tiles_used(want)
    for (rgb, depth), (want_rgb, want_depth) in zip(attached(got, sensors), attached(want, sensors)):
        assert np.array_equal(rgb, want_rgb) and np.array_equal(depth, want_depth)


def test_null_occlusion_one_pixel(gpu):
    sensor, model = pinhole_pair(1, 1, 1, 1, (1.0, 1.0, 0.0, 0.0), (1.0, 1.0, 0.0, 0.0), serial="one")
    frame = [(np.array([[1234]], dtype=np.uint16), np.array([[[9, 8, 7]]], dtype=np.uint8))]
    with RgbdRig([sensor]) as rig:
        structs = frame_structs(gpu, frame)
        want = gpu.cwipc_hip_rgbd_rig_grab(rig._handle(), structs)
        got = gpu.cwipc_hip_rgbd_rig_grab_occluded(rig._handle(), structs)
        assert want.count() == 1 and cloud_bytes(got) == cloud_bytes(want) == lm.cloud([model], frame)[0].tobytes()
        # ... and with the test on, a single pixel hides nothing
        check_against_model(gpu, rig, [sensor], [model], frame, RgbdOcclusion(8, 0.0))
        assert rig.grab(frame, occlusion=RgbdOcclusion(0, 0.0)).count() == 1


# ---- 2: the window rule on an identity rig ----

WINDOW_SHAPES = [(5, 3), (67, 45), (130, 70)]
LEVELS = np.array([0, 1000, 1010, 1500, 1510, 2500], dtype=np.uint16)
WINDOW_LEVELS = np.array([0, 1, 1000, 1010, 1500, 2500], dtype=np.uint16)


@pytest.fixture(scope="module")
def identity_rigs(gpu):
    """Per shape: a sensor without lenses, the colour side equal to the depth side, identity depth_to_colour -- every pixel with depth
    is a candidate at its own colour pixel with Pz = z -- and a depth image of a few levels, so many depths tie.  One level is a
    single depth unit, z = 0.001: from 1.000 the margin that reaches it is 0.999, nearly all of z, and only then does one ulp of the
    margin show in z - margin."""
    rng = np.random.default_rng(77)
    out = {}
    for w, h in WINDOW_SHAPES:
        intr = (0.9 * w, 1.1 * w, 0.48 * w, 0.53 * h)
        sensor, model = pinhole_pair(w, h, w, h, intr, intr, serial="id%d" % w)
        depth = WINDOW_LEVELS[rng.choice(len(WINDOW_LEVELS), (h, w), p=[0.04, 0.02, 0.4, 0.2, 0.2, 0.14])]
        colour = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
        out[(w, h)] = (sensor, model, [(depth, colour)], RgbdRig([sensor]))
    yield out
    for entry in out.values():
        entry[3].free()


def window_scan(depth, s, margin):
    """The rule an identity rig collapses to, offset by offset: dropped iff the minimum of z over the pixels with depth of the
    (2s + 1)^2 window, inside the image, is < z - margin."""
    h, w = depth.shape
    z = depth.astype(np.float64) * np.float64(0.001)
    padded = np.full((h + 2 * s, w + 2 * s), np.inf)             # +inf outside the image and where there is no depth
    padded[s:s + h, s:s + w] = np.where(depth != 0, z, np.inf)
    zmin = np.full((h, w), np.inf)
    for dv in range(-s, s + 1):
        for du in range(-s, s + 1):
            zmin = np.minimum(zmin, padded[s + dv:s + dv + h, s + du:s + du + w])
    return (depth != 0) & (zmin < z - np.float64(margin))


@pytest.mark.parametrize("s", [0, 1, 3, 8])
@pytest.mark.parametrize("shape", WINDOW_SHAPES)
def test_window_rule_on_an_identity_rig(gpu, identity_rigs, shape, s):
    sensor, model, frame, rig = identity_rigs[shape]
    depth = frame[0][0]
    exact = float(np.float64(1000) * np.float64(0.001) - np.float64(1) * np.float64(0.001))      # a difference of two z values present
    dropped = []
    for margin in (float(np.nextafter(exact, -np.inf)), exact, float(np.nextafter(exact, np.inf))):
        want = check_against_model(gpu, rig, [sensor], [model], frame, RgbdOcclusion(s, margin))
        drop = window_scan(depth, s, margin)
        assert np.array_equal(want[3][0], drop)                                      # the model is the window rule here ...
        pc = rig.grab(frame, attach_flags=gpu.CWIPC_HIP_RGBD_ATTACH_DEPTH, occlusion=RgbdOcclusion(s, margin))
        got_depth = attached_depth(pc, sensor)
        assert np.array_equal(got_depth, np.where(drop, 0, depth))                   # ... and so is the library, without the model
        assert pc.count() == int(((depth != 0) & ~drop).sum())
        dropped.append(int(drop.sum()))
    assert dropped[0] >= dropped[1] >= dropped[2]
    if s == 0:
        assert dropped == [0, 0, 0]                                                  # a pixel alone on its colour pixel hides nothing
    elif shape != (5, 3):
        assert dropped[0] > dropped[2] > 0                                           # 0.001 under 1.000: dropped below the margin, kept above it


def attached_depth(pc, sensor):
    meta = pc.access_metadata()
    assert meta.count() == 1 and meta.name(0) == "depth." + sensor.serial
    return np.frombuffer(bytes(meta.data(0)), dtype=np.uint16).reshape(sensor.height, sensor.width)


# ---- 3: a finer colour grid ----

def strip_scene():
    """64 x 48 depth, 128 x 96 colour (twice as fine), the colour sensor 50 mm along x.  A far plane at 2 m, green; in front of it at
    0.8 m a strip over depth columns 28 .. 35, red.  The colour image is what the colour sensor sees: red between the strip's edges
    (half a depth pixel beyond its outermost samples) projected into it, green elsewhere."""
    w, h, wc, hc = 64, 48, 128, 96
    intr, cintr = (60.0, 60.0, 31.5, 23.5), (120.0, 120.0, 63.5, 47.5)
    d2c = np.identity(4)
    d2c[0, 3] = -0.05
    sensor, model = pinhole_pair(w, h, wc, hc, intr, cintr, d2c, serial="strip")
    depth = np.full((h, w), 2000, dtype=np.uint16)
    depth[:, 28:36] = 800
    left = cintr[0] * (((27.5 - intr[2]) / intr[0] * 0.8 - 0.05) / 0.8) + cintr[2]
    right = cintr[0] * (((35.5 - intr[2]) / intr[0] * 0.8 - 0.05) / 0.8) + cintr[2]
    colour = np.zeros((hc, wc, 3), dtype=np.uint8)
    colour[..., 1] = 255
    cols = np.arange(wc)
    colour[:, (cols >= left) & (cols <= right)] = (255, 0, 0)
    return sensor, model, [(depth, colour)]


def test_finer_colour_grid_leaks_at_splat_0_and_not_at_1(gpu):
    sensor, model, frame = strip_scene()
    strip_pixels = int((frame[0][0] == 800).sum())

    def leaked(points):
        wall = points[np.abs(points['z'] - np.float32(2.0)) < 1e-3]
        return int(((wall['r'] == 255) & (wall['g'] == 0)).sum())

    def strip_kept(points):
        return int((np.abs(points['z'] - np.float32(0.8)) < 1e-3).sum())

    plain = lm.cloud([model], frame)[0]
    gaps = om.cloud([model], frame, splat=0, margin=0.02)[0]
    closed = om.cloud([model], frame, splat=1, margin=0.02)[0]
    # the scene shows the leak, in the model alone
    assert leaked(plain) > 100 and 0 < leaked(gaps) <= leaked(plain) and leaked(closed) == 0
    assert strip_kept(plain) == strip_kept(gaps) == strip_kept(closed) == strip_pixels
    with RgbdRig([sensor]) as rig:
        assert_cloud(rig.grab(frame), plain, 0, 0.0)
        check_against_model(gpu, rig, [sensor], [model], frame, RgbdOcclusion(0, 0.02))
        check_against_model(gpu, rig, [sensor], [model], frame, RgbdOcclusion(1, 0.02))
        got = rig.grab(frame, occlusion=RgbdOcclusion(1, 0.02)).get_numpy_array()
        assert leaked(got) == 0 and strip_kept(got) == strip_pixels
        assert leaked(rig.grab(frame, occlusion=RgbdOcclusion(0, 0.02)).get_numpy_array()) == leaked(gaps)


# ---- 4: contention and ties ----

def test_hundreds_of_candidates_on_one_cell_in_two_orders(gpu):
    """67 x 45 depth pixels into a 3 x 2 colour image: about 500 candidates per cell, depths of five levels.  Then the same camera with
    its rows reversed (fy and cy mirrored, the depth image flipped): the same rays, the candidates arriving in another order."""
    rng = np.random.default_rng(91)
    w, h = 67, 45
    fx, fy, cx, cy = 60.0, 58.0, 33.25, 22.5
    cintr = (3.0 / w * fx, 2.0 / h * fy, 1.0, 0.5)
    depth = LEVELS[rng.choice(len(LEVELS), (h, w), p=[0.04, 0.02, 0.3, 0.3, 0.24, 0.1])]
    colour = rng.integers(0, 256, (2, 3, 3)).astype(np.uint8)
    sensor, model = pinhole_pair(w, h, 3, 2, (fx, fy, cx, cy), cintr, serial="few")
    mirrored, mirrored_model = pinhole_pair(w, h, 3, 2, (fx, -fy, cx, (h - 1) - cy), cintr, serial="few")
    flipped = np.ascontiguousarray(depth[::-1])
    with RgbdRig([sensor]) as rig, RgbdRig([mirrored]) as mirrored_rig:
        for occ in (RgbdOcclusion(0, 0.0), RgbdOcclusion(0, 0.0105), RgbdOcclusion(1, 0.0)):
            want = check_against_model(gpu, rig, [sensor], [model], [(depth, colour)], occ)
            other = check_against_model(gpu, mirrored_rig, [mirrored], [mirrored_model], [(flipped, colour)], occ)
            assert 0 < int(want[3][0].sum()) < int((depth != 0).sum())
            assert np.array_equal(other[1][0][::-1], want[1][0]) and np.array_equal(other[2][0][::-1], want[2][0])
            fields = list(want[0].dtype.names)
            assert np.array_equal(np.sort(other[0], order=fields), np.sort(want[0], order=fields))
    # the candidates do share few cells
    _xc, _yc, _z, cand, uc, vc, _pz = om.projection(model, depth)
    assert np.bincount((vc * 3 + uc)[cand], minlength=6).min() > 300


# ---- 5: clipping ----

@pytest.mark.parametrize("splat", [1, 8])
def test_squares_clipped_at_every_border(gpu, splat):
    """A 5 x 3 colour image at half the depth image's resolution with common origin: depth pixel (u, v) lands at (u / 2, v / 2) exactly,
    odd ones on x.5 boundaries (which go up); (0, 0), (8, 0), (0, 4) and (8, 4) are the four corners, column 9 and row 5 fall outside."""
    rng = np.random.default_rng(17)
    sensor, model = pinhole_pair(10, 6, 5, 3, (2.0, 2.0, 0.0, 0.0), (1.0, 1.0, 0.0, 0.0), serial="clip")
    depth = rng.integers(900, 1100, (6, 10)).astype(np.uint16)
    colour = rng.integers(0, 256, (3, 5, 3)).astype(np.uint8)
    _xc, _yc, _z, cand, uc, vc, _pz = om.projection(model, depth)
    assert not cand[:, 9].any() and not cand[5, :].any() and cand[:5, :9].all()
    assert [(int(uc[v, u]), int(vc[v, u])) for v, u in ((0, 0), (0, 8), (4, 0), (4, 8), (1, 1), (3, 7))] == [(0, 0), (4, 0), (0, 2), (4, 2), (1, 1), (4, 2)]
    with RgbdRig([sensor]) as rig:
        for margin in (0.0, 0.05):
            want = check_against_model(gpu, rig, [sensor], [model], [(depth, colour)], RgbdOcclusion(splat, margin))
            assert 0 < len(want[0]) < int(cand.sum())
        if splat == 8:   # every square covers the image: only the nearest depth's pixels stay
            assert (check_against_model(gpu, rig, [sensor], [model], [(depth, colour)], RgbdOcclusion(8, 0.0))[1][0][:5, :9] ==
                    np.where(depth[:5, :9] == depth[:5, :9].min(), depth[:5, :9], 0)).all()


# ---- 6: cameras do not mix ----

def test_cameras_do_not_mix(gpu):
    """Three cameras of one make: a scene, nothing, and the same scene 1.5 m farther.  Were the z-buffers shared, the first would hide
    the third."""
    rng = np.random.default_rng(5)
    d2c = np.identity(4)
    d2c[0, 3] = -0.04
    intr, cintr = (60.0, 58.0, 33.2, 22.4), (95.0, 93.0, 50.1, 38.3)
    pairs = [pinhole_pair(67, 45, 101, 77, intr, cintr, d2c, 1 << k, "mix%d" % k) for k in range(3)]
    sensors, models = [p[0] for p in pairs], [p[1] for p in pairs]
    near = LEVELS[rng.choice(len(LEVELS), (45, 67), p=[0.04, 0.3, 0.2, 0.2, 0.16, 0.1])]
    far = np.where(near != 0, near + 1500, 0).astype(np.uint16)
    colours = [rng.integers(0, 256, (77, 101, 3)).astype(np.uint8) for _ in range(3)]
    frame = [(near, colours[0]), (np.zeros_like(near), colours[1]), (far, colours[2])]
    occ = RgbdOcclusion(1, 0.004)
    with RgbdRig(sensors) as rig:
        want = check_against_model(gpu, rig, sensors, models, frame, occ)
        got = rig.grab(frame, occlusion=occ).get_numpy_array()
    assert 0 < int(want[3][0].sum()) and 0 < int(want[3][2].sum()) and not want[3][1].any()
    for k in (0, 2):
        with RgbdRig([sensors[k]]) as single:
            alone = single.grab([frame[k]], occlusion=occ).get_numpy_array()
        assert len(alone) > 500 and got[got['tile'] == 1 << k].tobytes() == alone.tobytes()
    assert not (got['tile'] == 2).any()


# ---- 7: two frames through one rig ----

def test_the_zbuffer_is_reset_between_frames(gpu, raw):
    sensors, models, tables, frames, rig = raw
    occ = RgbdOcclusion(1, 0.02)
    first = frames[0]
    farther = [(np.where(d != 0, d.astype(np.uint32) + 4000, 0).astype(np.uint16), c) for d, c in first]   # everywhere behind the first
    check_against_model(gpu, rig, sensors, models, first, occ, tables=tables)
    want = check_against_model(gpu, rig, sensors, models, farther, occ, tables=tables)
    assert len(want[0]) > 500
    with RgbdRig(sensors) as fresh:
        assert cloud_bytes(fresh.grab(farther, occlusion=occ)) == cloud_bytes(rig.grab(farther, occlusion=occ)) == want[0].tobytes()
    # a plain grab on the rig that has a z-buffer by now
    assert_cloud(rig.grab(first, None, RgbdPrep(1, 2), 3, 0.0), lm.cloud(models, first, rm.Filter(), 1, 2, tables)[0], 3, 0.0)


# ---- 8: other inputs ----

@pytest.mark.parametrize("name", ["off", "all"])
def test_lenses_bgra_erosion_filters(gpu, raw, name):
    sensors, models, tables, frames, rig = raw
    for occ in (RgbdOcclusion(), RgbdOcclusion(0, 0.0), RgbdOcclusion(2, 0.3)):
        want = check_against_model(gpu, rig, sensors, models, frames[1], occ, FILTERS[name], 2, 2, tables)
        hidden = sum(int(h.sum()) for h in want[3])
        plain = lm.cloud(models, frames[1], rm.Filter(), 2, 2, tables)[0]
        assert 0 < hidden < len(plain) and len(want[0]) > 50                        # the test drops some and keeps some, on both cameras
        assert all(h.any() for h in want[3])


def test_page_locked_images(gpu, raw):
    sensors, models, tables, frames, rig = raw
    keep = []

    def pin(a):
        block = gpu.cwipc_hip_pinned_points((a.nbytes + 15) // 16)
        keep.append(block)
        out = block.view(np.uint8)[:a.nbytes].view(a.dtype).reshape(a.shape)
        out[...] = a
        return out

    pinned = [(pin(d), pin(c)) for d, c in frames[0]]
    check_against_model(gpu, rig, sensors, models, frames[0], RgbdOcclusion(1, 0.05), FILTERS["all"], 1, 2, tables, grab_frame=pinned)


def test_vga_on_the_three_launch_flow(gpu):
    """640 x 480 = 307 200 depth pixels: more than the 256 k up to which the count kernel's last workgroup scans.  Colour 701 x 523,
    lenses on both sensors; the depth smooth enough for most of it to stay."""
    rng = np.random.default_rng(8)
    sensor, model = raw_pair(640, 480, 701, 523, 8, "vga", 3, rng)
    v, u = np.meshgrid(np.arange(480), np.arange(640), indexing='ij')
    depth = (1500 + 300 * np.sin(u / 40.0) * np.cos(v / 35.0) + 700 * ((u // 80 + v // 60) % 2)).astype(np.uint16)
    depth[rng.random(depth.shape) < 0.001] = 0
    frame = [(depth, rng.integers(0, 256, (523, 701, 3)).astype(np.uint8))]
    with RgbdRig([sensor]) as rig:
        want = check_against_model(gpu, rig, [sensor], [model], frame, RgbdOcclusion(1, 0.03), rm.Filter(), 1, 1)
    assert 640 * 480 > 262144 and len(want[0]) > 200000 and int(want[3][0].sum()) > 1000


# ---- 9: attached images and mappings ----

def test_attached_images_show_the_occluded_pixels(gpu, raw):
    sensors, models, tables, frames, rig = raw
    occ = RgbdOcclusion(1, 0.02)
    plain = lm.cloud(models, frames[0], rm.Filter(), 1, 2, tables)
    want = om.cloud(models, frames[0], rm.Filter(), 1, 2, tables, occ.splat, occ.margin)
    before = [rig.map2d3d(0, u, v, 900) for u, v in ((0, 0), (30, 7), (66, 44))] + [rig.mapcolordepth(1, 30, 7), rig.mapcolordepth(1, 67, 0)]
    src = RgbdRigSource(sensors, [frames[0]], None, RgbdPrep(1, 2), occlusion=occ)
    src.request_metadata("rgb")
    src.request_metadata("depth")
    pc = src.get()
    meta = pc.access_metadata()
    assert [meta.name(i) for i in range(meta.count())] == ["rgb.raw3", "depth.raw3", "rgb.raw4", "depth.raw4"]
    assert [meta.description(i) for i in range(meta.count())] == ["width=67,height=45,bpp=3", "width=67,height=45,bpp=2"] * 2
    for i, (rgb, depth) in enumerate(attached(pc, sensors)):
        hidden = want[3][i]
        assert hidden.any() and (plain[1][i][hidden] != 0).all()                     # they had depth and a colour without the test
        assert np.array_equal(depth, np.where(hidden, 0, plain[1][i])) and np.array_equal(depth, want[1][i])
        assert np.array_equal(rgb, np.where(hidden[..., None], 0, plain[2][i])) and np.array_equal(rgb, want[2][i])
    assert pc.get_numpy_array().tobytes() == want[0].tobytes()
    # the mappings do not know about occlusion: as before, and the cloud's points bit for bit
    after = [src.rig.map2d3d(0, u, v, 900) for u, v in ((0, 0), (30, 7), (66, 44))] + [src.rig.mapcolordepth(1, 30, 7), src.rig.mapcolordepth(1, 67, 0)]
    assert after == before and before[3] == (30, 7) and before[4] is None
    got = pc.get_numpy_array()
    first = got[got['tile'] == 2]
    vs, us = np.nonzero(want[1][0])
    direct = np.float32([src.rig.map2d3d(0, int(u), int(v), int(want[1][0][v, u])) for u, v in zip(us, vs)])
    assert np.array_equal(direct.view(np.uint32), np.stack([first['x'], first['y'], first['z']], axis=1).view(np.uint32))
    src.free()


# ---- 10: errors ----

def test_bad_occlusion_is_an_error_and_leaves_nothing(gpu, raw):
    sensors, _models, _tables, frames, rig = raw
    gc.collect()
    before = gpu.cwipc_dangling_allocations(False)
    for occ, text in ((RgbdOcclusion(-1, 0.02), "splat must be between 0 and 8"), (RgbdOcclusion(9, 0.02), "splat must be between 0 and 8"),
                      (RgbdOcclusion(1, -0.01), "margin must be finite"), (RgbdOcclusion(1, math.nan), "margin must be finite"),
                      (RgbdOcclusion(1, math.inf), "margin must be finite")):
        with pytest.raises(gpu.CwipcError, match=text):
            rig.grab(frames[0], occlusion=occ)
        assert gpu.cwipc_dangling_allocations(False) == before
    # rig_grab's own errors, through the new entry
    with pytest.raises(gpu.CwipcError, match="between 0 and 32"):
        rig.grab(frames[0], None, RgbdPrep(33, 0), occlusion=RgbdOcclusion())
    good = frame_structs(gpu, frames[0])
    with pytest.raises(gpu.CwipcError, match="NULL argument"):
        gpu.cwipc_hip_rgbd_rig_grab_occluded(rig._handle(), [gpu.cwipc_hip_rgbd_frame(None, good[0].colour), good[1]], None, RgbdOcclusion().as_struct())
    with pytest.raises(gpu.CwipcError, match="NULL argument"):
        gpu.cwipc_hip_rgbd_rig_grab_occluded(None, good, None, RgbdOcclusion().as_struct())
    gc.collect()
    assert gpu.cwipc_dangling_allocations(False) == before
    assert rig.grab(frames[0], occlusion=RgbdOcclusion(8, 0.0)).count() > 0 and rig.grab(frames[0], occlusion=RgbdOcclusion(0, 1e9)).count() > 0


# ---- 11: the Python surface ----

def test_python_surface_gives_the_c_entrys_cloud(gpu, raw):
    sensors, _models, _tables, frames, rig = raw
    occ = RgbdOcclusion(2, 0.01)
    assert (RgbdOcclusion().splat, RgbdOcclusion().margin) == (1, 0.02)
    struct = occ.as_struct()
    assert isinstance(struct, gpu.cwipc_hip_rgbd_occlusion) and (struct.splat, struct.margin) == (2, 0.01)
    flt = to_filter(FILTERS["depth"])
    want = gpu.cwipc_hip_rgbd_rig_grab_occluded(rig._handle(), frame_structs(gpu, frames[0]), RgbdPrep(1, 1).as_struct(), struct, flt.as_struct(), 12, 0.25)
    assert want.count() > 0 and cloud_bytes(want) != cloud_bytes(rig.grab(frames[0], flt, RgbdPrep(1, 1), 12, 0.25))
    assert cloud_bytes(rig.grab(frames[0], flt, RgbdPrep(1, 1), 12, 0.25, occlusion=occ)) == cloud_bytes(want)
    src = RgbdRigSource(sensors, [frames[0], frames[0]], flt, RgbdPrep(1, 1), 0.25, 12, occlusion=occ)
    pc = src.get()
    assert cloud_bytes(pc) == cloud_bytes(want) and pc.timestamp() == 12 and pc.cellsize() == 0.25
    assert src.get().timestamp() == 13
    src.free()
    plain = RgbdRigSource(sensors, [frames[0]], flt, RgbdPrep(1, 1), 0.25, 12)
    assert plain.occlusion is None and cloud_bytes(plain.get()) == cloud_bytes(rig.grab(frames[0], flt, RgbdPrep(1, 1), 12, 0.25))
    plain.free()
