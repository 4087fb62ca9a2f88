"""cwipc_hip_from_rgbd on the GPU against the numpy model (tests/rgbd_model.py): the cloud byte for byte -- order, coordinates,
colours, tiles -- with its timestamp, cellsize and count; the tiles it knows, the attached images, the two mappings and the errors."""
import ctypes
import struct

import numpy as np
import pytest

import rgbd_model as rm
from test_gpu_exact_filters import round_up, spacing
from cwipc_util_amd.rgbd import RgbdCamera, RgbdFilter, RgbdRig, RgbdSensor, RgbdSource, from_rgbd

pytestmark = pytest.mark.gpu

FILTERS = {
    "off": rm.Filter(),
    "depth": rm.Filter(threshold_near=1.0, threshold_far=3.0),
    "height": rm.Filter(height_min=-0.6, height_max=1.1),
    "radius": rm.Filter(radius=2.5),
    "green": rm.Filter(greenscreen=True),
    "all": rm.Filter(1.0, 3.0, -0.6, 1.1, 2.5, True),
}


def camera_pair(width, height, tile, serial, bpp, rng, scale=0.001, trafo=None):
    """The same camera for the library and for the model"""
    fx, fy, cx, cy = rng.uniform(0.7, 1.3) * width, rng.uniform(0.7, 1.3) * width, rng.uniform(0.4, 0.6) * width, rng.uniform(0.4, 0.6) * height
    m = rm.random_rigid(rng, 1.0) if trafo is None else trafo
    return RgbdCamera(width, height, fx, fy, cx, cy, scale, m, tile, serial, bpp), rm.Camera(fx, fy, cx, cy, scale, m, tile, bpp)


def images(width, height, bpp, rng, zeros=0.3):
    depth = rng.integers(300, 4000, (height, width)).astype(np.uint16)
    depth[rng.random((height, width)) < zeros] = 0
    return depth, rng.integers(0, 256, (height, width, bpp)).astype(np.uint8)


def to_filter(flt):
    return RgbdFilter(*flt)


def assert_cloud(pc, want, timestamp, cellsize):
    got = pc.get_numpy_array()
    assert pc.count() == len(want) == len(got)
    assert got.tobytes() == want.tobytes()
    assert pc.timestamp() == timestamp and pc.cellsize() == np.float32(cellsize)


@pytest.fixture(scope="module")
def three(gpu):
    """Cameras of 1 x 1, 67 x 45 RGB8 and 64 x 48 BGRA, each with its own matrix and tile, and one frame of them: depth with about
    30 % zeros (the single pixel has depth)."""
    rng = np.random.default_rng(101)
    pairs = [camera_pair(1, 1, 1, "one", 3, rng), camera_pair(67, 45, 2, "s67", 3, rng), camera_pair(64, 48, 4, "s64", 4, rng)]
    frame = [images(1, 1, 3, rng, zeros=0.0), images(67, 45, 3, rng), images(64, 48, 4, rng)]
    return [p[0] for p in pairs], [p[1] for p in pairs], frame


@pytest.mark.parametrize("name", list(FILTERS))
def test_three_cameras_against_the_model(gpu, three, name):
    cams, model_cams, frame = three
    flt = FILTERS[name]
    want = rm.cloud(model_cams, frame, flt)
    if name != "off":
        assert 0 < len(want) < len(rm.cloud(model_cams, frame))   # (the filter drops some points and keeps some)
    assert_cloud(from_rgbd(cams, frame, to_filter(flt), 987654321012, 0.005), want, 987654321012, 0.005)


@pytest.mark.parametrize("name", ["off", "all"])
def test_vga_camera_crosses_the_flow_boundary(gpu, name):
    """640 x 480 = 307 200 pixels, nearly all valid: more than the 256 k up to which the count kernel's last workgroup scans."""
    rng = np.random.default_rng(7)
    cam, model_cam = camera_pair(640, 480, 8, "vga", 3, rng)
    frame = [images(640, 480, 3, rng, zeros=0.01)]
    want = rm.cloud([model_cam], frame, FILTERS[name])
    assert len(want) > (262144 if name == "off" else 1000)
    assert_cloud(from_rgbd([cam], frame, to_filter(FILTERS[name]), 5, 0.0), want, 5, 0.0)


def test_megapixel_camera_fills_one_scan_round(gpu):
    """1024 x 1024 pixels are 1024 workgroups of 1024 pixels: exactly one round of the 1024-lane scan of their counts."""
    rng = np.random.default_rng(11)
    cam, model_cam = camera_pair(1024, 1024, 3, "mp", 3, rng)
    frame = [images(1024, 1024, 3, rng, zeros=0.01)]
    want = rm.cloud([model_cam], frame)
    assert len(want) > 1000000
    assert_cloud(from_rgbd([cam], frame, to_filter(FILTERS["off"]), 6, 0.0), want, 6, 0.0)


@pytest.mark.parametrize("depth", ["random", "sparse"])
def test_one_workgroup_past_a_scan_round(gpu, depth):
    """1025 x 1024 pixels are 1025 workgroups: the scan's second round holds a single count, and what the first round carries over is
    its offset.  sparse: depth only in workgroups 0, 1023 and 1024 (a hundred pixels each) and at the last pixel, so a wrong carry
    shows as points at wrong places, not only as a wrong total."""
    rng = np.random.default_rng(12)
    width, height = 1025, 1024
    cam, model_cam = camera_pair(width, height, 5, "mp1", 3, rng)
    frame = [images(width, height, 3, rng, zeros=0.01)]
    if depth == "sparse":
        flat = np.zeros(width * height, dtype=np.uint16)
        for group in (0, 1023, 1024):
            flat[group * 1024 + rng.choice(1024, 100, replace=False)] = rng.integers(300, 4000, 100)
        flat[-1] = 1234
        frame = [(flat.reshape(height, width), frame[0][1])]
    want = rm.cloud([model_cam], frame)
    assert 300 <= len(want) <= 301 if depth == "sparse" else len(want) > 1000000
    assert_cloud(from_rgbd([cam], frame, to_filter(FILTERS["off"]), 7, 0.0), want, 7, 0.0)


def test_middle_camera_without_depth(gpu, three):
    cams, model_cams, frame = three
    rng = np.random.default_rng(3)
    extra, model_extra = camera_pair(33, 21, 16, "mid", 4, rng)
    empty = (np.zeros((21, 33), dtype=np.uint16), images(33, 21, 4, rng)[1])
    cams3, model3, frame3 = [cams[1], extra, cams[2]], [model_cams[1], model_extra, model_cams[2]], [frame[1], empty, frame[2]]
    pc = from_rgbd(cams3, frame3, None, 1, 0.0)
    assert_cloud(pc, rm.cloud(model3, frame3), 1, 0.0)
    assert gpu.get_tiles_used(pc) == [2, 4]


def test_nothing_survives(gpu, three):
    """Filters that drop everything: count 0, and the cloud is a cloud."""
    cams, model_cams, frame = three
    flt = rm.Filter(threshold_near=100.0, threshold_far=200.0)
    assert len(rm.cloud(model_cams, frame, flt)) == 0
    pc = from_rgbd(cams, frame, to_filter(flt), 77, 0.25)
    assert pc.count() == 0 and len(pc.get_numpy_array()) == 0 and pc.timestamp() == 77 and pc.cellsize() == 0.25
    assert gpu.get_tiles_used(pc) == [] and gpu.cwipc_tilefilter(pc, 2).count() == 0
    other = from_rgbd(cams, frame)
    assert gpu.cwipc_join(pc, other).count() == other.count()


@pytest.fixture(scope="module")
def square(gpu):
    """One 64 x 64 camera (4096 pixels) for the library and the model; the one-sensor pinhole rig that it is (depth and colour both
    64 x 64, identity depth_to_colour); a colour image; the points of a second cloud for a join."""
    rng = np.random.default_rng(202)
    cam, model_cam = camera_pair(64, 64, 2, "sq", 3, rng)
    sensor = RgbdSensor(64, 64, cam.fx, cam.fy, cam.cx, cam.cy, 64, 64, cam.fx, cam.fy, cam.cx, cam.cy, depth_scale=cam.depth_scale, trafo=cam.trafo,
                        tile=cam.tile, serial=cam.serial, bpp=cam.bpp)
    colour = images(64, 64, 3, rng)[1]
    second = rm.cloud([model_cam], [images(64, 64, 3, rng, zeros=0.9)])
    assert 100 < len(second) < 4096
    with RgbdRig([sensor]) as rig:
        yield cam, model_cam, rig, colour, second


@pytest.mark.parametrize("entry", ["from_rgbd", "rig_grab"])
@pytest.mark.parametrize("kept", [0, 1, 255, 256, 257, 4095, 4096])
def test_result_size_exits(gpu, square, kept, entry):
    """Exactly `kept` of the 4096 pixels have depth, no filter.  kept * 16 >= 4096 (256 and up): the result stays in the planes that
    had room for every pixel, with their spacing, and only the count shrinks; below that (0, 1, 255) it is copied to planes of its
    own size.  Either way the cloud is the model's, and so is its join with a second cloud, in both orders: a shrunk cloud is a
    cloud.  Through cwipc_hip_from_rgbd and through cwipc_hip_rgbd_rig_grab."""
    cam, model_cam, rig, colour, second = square
    rng = np.random.default_rng(300 + kept)
    depth = np.zeros(4096, dtype=np.uint16)
    depth[rng.permutation(4096)[:kept]] = rng.integers(300, 4000, kept)
    frame = [(depth.reshape(64, 64), colour)]
    want = rm.cloud([model_cam], frame)
    assert len(want) == kept
    pc = from_rgbd([cam], frame, None, 31, 0.5) if entry == "from_rgbd" else rig.grab(frame, None, None, 31, 0.5)
    assert_cloud(pc, want, 31, 0.5)
    assert spacing(gpu, pc) == (round_up(4096) if kept * 16 >= 4096 else round_up(kept)), (kept, spacing(gpu, pc))
    other = gpu.cwipc_from_numpy_array(second, 30)
    other._set_cellsize(0.25)
    assert_cloud(gpu.cwipc_join(pc, other), np.concatenate([want, second]), 30, 0.25)
    assert_cloud(gpu.cwipc_join(other, pc), np.concatenate([second, want]), 30, 0.25)
    assert_cloud(pc, want, 31, 0.5)   # (and the cloud is as it was)


@pytest.mark.parametrize("pinned", [False, True])
def test_every_pixel_kept_pageable_and_pinned(gpu, pinned):
    """No zero depth, no filter: every pixel is a point.  The images in ordinary memory and in cwipc_hip_host_alloc memory."""
    rng = np.random.default_rng(11)
    cam_a, model_a = camera_pair(67, 45, 1, "a", 3, rng, scale=1.0 / 1024)
    cam_b, model_b = camera_pair(40, 30, 2, "b", 4, rng)
    frame = [images(67, 45, 3, rng, zeros=0.0), images(40, 30, 4, rng, zeros=0.0)]
    keep = []
    if pinned:
        def pin(a):
            raw = gpu.cwipc_hip_pinned_points((a.nbytes + 15) // 16)
            keep.append(raw)
            out = raw.view(np.uint8)[:a.nbytes].view(a.dtype).reshape(a.shape)
            out[...] = a
            return out
        frame = [(pin(d), pin(c)) for d, c in frame]
    want = rm.cloud([model_a, model_b], frame)
    assert len(want) == 67 * 45 + 40 * 30
    assert_cloud(from_rgbd([cam_a, cam_b], frame, None, 9, 0.0), want, 9, 0.0)


def test_tiles(gpu, three):
    cams, _model_cams, frame = three
    pc = from_rgbd(cams, frame)
    assert gpu.get_tiles_used(pc) == [1, 2, 4]
    assert gpu.cwipc_tilefilter(pc, 8).count() == 0 and gpu.cwipc_tilefilter(pc, 3).count() == 0
    got = gpu.cwipc_tilefilter(pc, 4).get_numpy_array()
    assert len(got) == int((frame[2][0] != 0).sum()) and (got['tile'] == 4).all()


def test_metadata_images(gpu, three):
    """The expectations written out: a colour image comes out B, G, R whatever its format (R, G, B bytes reversed; the first three of
    B, G, R, A bytes), a depth image as it went in."""
    cams, _model_cams, frame = three
    src = RgbdSource(cams, [frame, frame, frame])
    pc = src.get()                                     # (the metadata live as long as their cloud: keep it)
    assert pc.access_metadata().count() == 0           # no flags: no metadata
    src.request_metadata("depth")
    pc = src.get()
    meta = pc.access_metadata()
    assert [meta.name(i) for i in range(meta.count())] == ["depth.one", "depth.s67", "depth.s64"]
    src.request_metadata("rgb")
    assert src.is_metadata_requested("rgb") and not src.is_metadata_requested("skeleton")
    pc = src.get()
    meta = pc.access_metadata()
    assert [meta.name(i) for i in range(meta.count())] == ["rgb.one", "depth.one", "rgb.s67", "depth.s67", "rgb.s64", "depth.s64"]
    assert [meta.description(i) for i in range(meta.count())] == ["width=1,height=1,bpp=3", "width=1,height=1,bpp=2", "width=67,height=45,bpp=3",
                                                                  "width=67,height=45,bpp=2", "width=64,height=48,bpp=4", "width=64,height=48,bpp=2"]
    assert meta.get_image_description(2) == {"width": 67, "height": 45, "bpp": 3, "image_format": "RGB8"}
    assert meta.data(3) == frame[1][0].tobytes() and meta.data(4) == frame[2][1].tobytes()
    by_serial = meta.get_all_images("s67")
    assert sorted(by_serial) == ["depth.", "rgb."]
    assert by_serial["depth."].dtype == np.uint16 and np.array_equal(by_serial["depth."], frame[1][0])
    assert by_serial["rgb."].shape == (45, 67, 3) and np.array_equal(by_serial["rgb."], frame[1][1][:, :, ::-1])
    # bpp=4 reads as "RGBA" in the reference's get_image_description, which its get_image does not know: it raises, and so does this
    assert meta.get_image_description(4) == {"width": 64, "height": 48, "bpp": 4, "image_format": "RGBA"}
    with pytest.raises(gpu.CwipcError, match="Unknown auxiliary data image format: 'RGBA'"):
        meta.get_image(4)
    with pytest.raises(gpu.CwipcError, match="Unknown auxiliary data image format"):
        meta.get_all_images("rgb.")
    assert src.get() is None and src.eof()
    # the two RGB8 cameras alone: every colour image by serial number
    src = RgbdSource(cams[:2], iter([frame[:2]]))
    src.request_metadata("rgb")
    src.request_metadata("depth")
    pc = src.get()
    colour = pc.access_metadata().get_all_images("rgb.")
    assert sorted(colour) == ["one", "s67"]
    assert np.array_equal(colour["s67"], frame[1][1][:, :, ::-1]) and np.array_equal(colour["one"], frame[0][1][:, :, ::-1])


def test_bgra_image_by_format_number(gpu):
    """format=3 is the reference's BGRA: get_image hands out the first three of every four bytes.  (An item made through the parser
    alone: a description is all get_image_description looks at.)"""
    meta = gpu.cwipc_metadata.__new__(gpu.cwipc_metadata)
    assert meta._parse_aux_description("width=2,height=1,format=3,name=x") == {"width": 2, "height": 1, "format": 3, "name": "x"}
    pixels = np.arange(8, dtype=np.uint8)
    meta.description = lambda idx: "width=2,height=1,format=3"
    meta.data = lambda idx: bytearray(pixels.tobytes())
    assert meta.get_image_description(0) == {"width": 2, "height": 1, "format": 3, "bpp": 4, "image_format": "BGRA"}
    assert meta.get_image(0).tolist() == [[[0, 1, 2], [4, 5, 6]]]
    meta.description = lambda idx: "width=2,height=2,format=4"
    assert meta.get_image(0).tolist() == [[0x0100, 0x0302], [0x0504, 0x0706]]
    meta.description = lambda idx: "width=2,height=1,format=YUYV"
    with pytest.raises(gpu.CwipcError, match="'YUYV'"):
        meta.get_image(0)


def test_map2d3d_is_the_cloud_bit_for_bit(gpu, three):
    """For every kept pixel of the 67 x 45 camera map2d3d(u, v, depth[v, u]) is that point's three floats, through the C call and
    through RgbdSource.auxiliary_operation."""
    cams, _model_cams, frame = three
    cam, (depth, colour) = cams[1], frame[1]
    got = from_rgbd([cam], [(depth, colour)]).get_numpy_array()
    vs, us = np.nonzero(depth)
    assert len(got) == len(us) > 1500
    cloud_bits = np.stack([got['x'], got['y'], got['z']], axis=1).view(np.uint32)
    cstruct = cam.as_struct()
    direct = np.float32([gpu.cwipc_hip_rgbd_map2d3d(cstruct, int(u), int(v), int(depth[v, u])) for u, v in zip(us, vs)])
    assert np.array_equal(direct.view(np.uint32), cloud_bits)
    src = RgbdSource(cams, [])
    through = np.zeros((len(us), 3), dtype=np.float32)
    for i, (u, v) in enumerate(zip(us, vs)):
        out = bytearray(12)
        assert src.auxiliary_operation("map2d3d", struct.pack("ffff", 2.0, float(u), float(v), float(depth[v, u])), out) is True
        through[i] = struct.unpack("fff", out)
    assert np.array_equal(through.view(np.uint32), cloud_bits)


def test_mappings_say_false(gpu, three):
    cams, _model_cams, _frame = three
    src = RgbdSource(cams, [])
    out = bytearray(8)
    assert src.auxiliary_operation("mapcolordepth", struct.pack("iii", 2, 66, 44), out) is True and struct.unpack("ii", out) == (66, 44)
    assert src.auxiliary_operation("mapcolordepth", struct.pack("iii", 2, 0, 0), out) is True and struct.unpack("ii", out) == (0, 0)
    for u, v in ((67, 0), (0, 45), (-1, 3), (3, -1)):
        assert src.auxiliary_operation("mapcolordepth", struct.pack("iii", 2, u, v), out) is False
    assert src.auxiliary_operation("mapcolordepth", struct.pack("iii", 3, 0, 0), out) is False          # no camera has tile 3
    assert src.auxiliary_operation("map2d3d", struct.pack("ffff", 3.0, 1.0, 1.0, 900.0), bytearray(12)) is False
    assert src.auxiliary_operation("map2d3d", struct.pack("ffff", 2.0, 1.0, 1.0, 0.0), bytearray(12)) is False   # no depth
    assert src.auxiliary_operation("nosuchop", b"", bytearray(0)) is False
    cstruct = cams[1].as_struct()
    assert gpu.cwipc_hip_rgbd_mapcolordepth(cstruct, 67, 0) is None and gpu.cwipc_hip_rgbd_mapcolordepth(cstruct, 66, 44) == (66, 44)
    assert src.serial_dict() == {1: "one", 2: "s67", 4: "s64"} and src.maxtile() == 4
    assert src.get_tileinfo_dict(0)["cameraMask"] == 7 and src.get_tileinfo_dict(2)["cameraMask"] == 2 and src.get_tileinfo_dict(2)["ncamera"] == 1


def test_errors_leave_nothing_behind(gpu, three):
    cams, _model_cams, frame = three
    good = cams[1].as_struct(*frame[1])
    before = gpu.cwipc_dangling_allocations(False)

    def broken(**changes):
        s = cams[1].as_struct(*frame[1])
        for name, value in changes.items():
            setattr(s, name, value)
        return s

    cases = [([broken(depth=None)], "NULL argument"), ([broken(colour=None)], "NULL argument"), ([], "ncam must be at least 1"),
             ([broken(width=0)], "width and height must be at least 1"), ([broken(height=-3)], "width and height must be at least 1"),
             ([broken(bpp=2)], "bpp must be 3"), ([broken(bpp=5)], "bpp must be 3"), ([broken(fx=float('nan'))], "must be finite"),
             ([broken(cy=float('inf'))], "must be finite"), ([broken(depth_scale=float('-inf'))], "must be finite"), ([broken(fy=0.0)], "must not be zero"),
             ([good, broken(bpp=7)], "camera 1: bpp must be 3")]
    for structs, text in cases:
        with pytest.raises(gpu.CwipcError, match=text):
            gpu.cwipc_hip_from_rgbd(structs)
    bad_matrix = broken()
    bad_matrix.trafo[7] = float('nan')
    with pytest.raises(gpu.CwipcError, match="must be finite"):
        gpu.cwipc_hip_from_rgbd([bad_matrix])
    no_serial = broken(serial=None)
    with pytest.raises(gpu.CwipcError, match="NULL argument"):
        gpu.cwipc_hip_from_rgbd([no_serial], attach_flags=gpu.CWIPC_HIP_RGBD_ATTACH_DEPTH)
    # the C call itself: NULL cameras, and a NULL errorMessage is fine
    dll = gpu.cwipc_util_dll_load()
    err = ctypes.c_char_p()
    assert not dll.cwipc_hip_from_rgbd(None, 1, None, 0, 0.0, 0, ctypes.byref(err)) and b"NULL argument" in err.value
    assert not dll.cwipc_hip_from_rgbd(None, 1, None, 0, 0.0, 0, None) and b"NULL argument" in dll.cwipc_hip_last_error()
    assert gpu.cwipc_dangling_allocations(False) == before
    # ... and the good camera still works afterwards
    assert gpu.cwipc_hip_from_rgbd([good]).count() == int((frame[1][0] != 0).sum())
