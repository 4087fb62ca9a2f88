"""cwipc_hip_render on the GPU against its numpy model (tests/render_model.py): byte-equal colour, depth and index images and the same
number of covered pixels, over cloud sizes around the workgroup size, images from one pixel to full HD, splats larger than the image,
every edge of the contract, thousands of points in one pixel, tile masks, threads and the error returns."""
import ctypes
import functools
import math
import threading

import numpy as np
import pytest

import render_model as rm
from conftest import make_cloud
from cwipc_util_amd.registration.render import PinholeView, default_view, look_at, render_pointcloud
from cwipc_util_amd.util import cwipc_point_numpy_dtype

pytestmark = pytest.mark.gpu

UP = (0, 1, 0)
BG = (7, 130, 255)


def _raw(gpu, pc, view, point_size=5, tilemask=0, background=BG, want_index=True):
    """The C call itself: (return value, rgb, depth, index)."""
    s = view.as_struct() if isinstance(view, PinholeView) else view
    h, w = max(int(s.height), 1), max(int(s.width), 1)
    rgb = np.full((h, w, 3), 99, dtype=np.uint8)
    depth = np.full((h, w), -1, dtype=np.float32)
    index = np.full((h, w), -7, dtype=np.int32) if want_index else None
    bg = (ctypes.c_uint8 * 3)(*background)
    rc = gpu.cwipc_util_dll_load().cwipc_hip_render(pc.as_cwipc_p(), ctypes.addressof(s), point_size, tilemask, ctypes.addressof(bg), rgb.ctypes.data,
                                                   depth.ctypes.data, index.ctypes.data if want_index else None)
    return rc, rgb, depth, index


def _check(gpu, pts, view, point_size=5, tilemask=0, background=BG):
    """Render and compare with the model; returns the model's images and count."""
    rc, rgb, depth, index = _raw(gpu, make_cloud(gpu, pts), view, point_size, tilemask, background)
    m_rgb, m_depth, m_index, m_covered = rm.render_model(pts, view, point_size, tilemask, background)
    assert rc == m_covered, (rc, m_covered)
    assert np.array_equal(index, m_index), "index: %d pixels differ" % int((index != m_index).sum())
    assert np.array_equal(depth.view(np.uint32), m_depth.view(np.uint32))
    assert rgb.tobytes() == m_rgb.tobytes()
    return m_rgb, m_depth, m_index, m_covered


def _pts(n):
    return np.zeros(n, dtype=cwipc_point_numpy_dtype)


def _scaled_view(width, height, extrinsic):
    f = (height / 2.0) / math.tan(math.radians(30.0))
    return PinholeView(width, height, f, f, (width - 1) / 2.0, (height - 1) / 2.0, extrinsic)


@functools.lru_cache(maxsize=None)
def _random_cloud(n, in_camera_space):
    """Random points in front of the camera, some outside the image; half of them on a lattice, so that depths and pixels coincide."""
    rng = np.random.default_rng(1000 + n + (7 if in_camera_space else 0))
    p = np.empty((n, 3))
    if in_camera_space:     # the identity view: x right, y down, z forward
        p[:, 0], p[:, 1], p[:, 2] = rng.uniform(-3, 3, n), rng.uniform(-1.5, 1.5, n), rng.uniform(2, 4.5, n)
    else:                   # the world in front of look_at((0, 1, -3), (0, 1, 0), up)
        p[:, 0], p[:, 1], p[:, 2] = rng.uniform(-2, 2, n), rng.uniform(-0.5, 2.5, n), rng.uniform(-1, 1.5, n)
    lattice = rng.random(n) < 0.5
    p[lattice] = np.round(p[lattice] * 32) / 32
    pts = _pts(n)
    pts['x'], pts['y'], pts['z'] = p[:, 0], p[:, 1], p[:, 2]
    pts['r'], pts['g'], pts['b'] = rng.integers(0, 256, (3, n))
    pts['tile'] = rng.choice([1, 2, 4], n)
    return pts


SIZES = [0, 1, 63, 64, 65, 1023, 1025, 200001]
SHAPES = [(1, 1, 1), (1, 1, 5), (7, 5, 1), (7, 5, 3), (7, 5, 15), (64, 64, 1), (64, 64, 5), (640, 480, 5)]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("width, height, point_size", SHAPES)
def test_sizes(gpu, n, width, height, point_size):
    view = _scaled_view(width, height, look_at((0, 1, -3), (0, 1, 0), UP))
    covered = _check(gpu, _random_cloud(n, False), view, point_size)[3]
    if n >= 1023:
        assert covered > 0


@pytest.mark.parametrize("n", SIZES)
def test_sizes_default_view(gpu, n):
    covered = _check(gpu, _random_cloud(n, True), default_view(), 5)[3]
    if n >= 63:
        assert covered > 25


# ---- edges: a 16 x 16 image, fx = fy = 8, cx = cy = 8 and z = 1: x = k / 8 gives u = k + 8 exactly ----
def _edge_view(**kw):
    return PinholeView(16, 16, 8.0, 8.0, 8.0, 8.0, **kw)


def _at(uv_list, z=1.0):
    """Points whose (u, v) in _edge_view are the given values, at depth z (one value or one per point): exactly, for multiples of 1/8
    and depths that are powers of two."""
    pts = _pts(len(uv_list))
    uv = np.asarray(uv_list, dtype=np.float64).reshape(-1, 2)
    zs = np.broadcast_to(np.asarray(z, dtype=np.float64), (len(pts),))
    pts['x'], pts['y'], pts['z'] = (uv[:, 0] - 8.0) / 8.0 * zs, (uv[:, 1] - 8.0) / 8.0 * zs, zs
    pts['r'] = np.arange(len(pts)) + 1
    pts['g'] = 200
    pts['tile'] = 1
    return pts


@pytest.mark.parametrize("point_size", [1, 3, 5])
def test_edge_integer_and_fractional_pixels(gpu, point_size):
    h = (point_size - 1) // 2
    # u or v exactly an integer, among them the image's first and last pixel and the first one outside
    pts = _at([(0, 0), (15, 15), (16, 3), (3, 16), (5, 7), (5.875, 7.875), (6, 8), (0, 15.875), (-0.125, 4)])
    _, _, index, _ = _check(gpu, pts, _edge_view(), point_size)
    assert index[0, 0] == 0 and index[15, 15] == 1 and index[7, 5] == 4
    assert (index == 2).any() == (h >= 1)          # u = 16 is outside; its splat reaches in from h = 1 on
    # u in (-1, 0): floor gives -1, a conversion that truncates would give 0
    pts = _at([(-0.5, 4), (4, -0.5), (-0.875, -0.125)])
    _, _, index, covered = _check(gpu, pts, _edge_view(), point_size)
    if h == 0:
        assert covered == 0
    else:
        assert index[4, 0] == 0 and index[0, 4] == 1 and index[0, 0] == 2 and (index[:, h:] != 0).all()   # columns -1-h .. -1+h


@pytest.mark.parametrize("point_size", [1, 3, 5, 15])
def test_edge_centres_off_every_side(gpu, point_size):
    h = (point_size - 1) // 2
    uv = []
    for k in (h, h + 1, h + 2):
        uv += [(-k, 8), (15 + k, 8), (8, -k), (8, 15 + k), (-k, -k), (15 + k, 15 + k)]
    # (each point of a group at a depth of its own, the later the nearer: no point hides behind a tie with an earlier one)
    _, _, index, _ = _check(gpu, _at(uv, [4, 2, 1, 0.5, 0.25, 0.125] * 3), _edge_view(), point_size)
    seen = set(index[index >= 0].tolist())
    assert seen == set(range(6))                   # off by h: one row or column of the splat is inside; off by more: nothing is


def test_edge_near_and_far(gpu):
    up = np.nextafter(np.float32(0.5), np.float32(1)), np.nextafter(np.float32(4), np.float32(0))
    # at near, just above it, behind the camera, at far, just below it, beyond it, in between: one pixel each in row 1
    zs = np.array([0.5, up[0], -1.0, 4.0, up[1], 5.0, 1.0], dtype=np.float32)
    pts = _at([(2 * k + 1.5, 1.5) for k in range(7)], zs)
    view = _edge_view(near=0.5, far=4.0)
    _, depth, index, covered = _check(gpu, pts, view, 1)
    assert sorted(index[index >= 0].tolist()) == [1, 4, 6] and covered == 3
    assert depth[index == 1][0] == up[0] and depth[index == 4][0] == up[1]
    # no far plane: everything in front of near
    _, _, index, _ = _check(gpu, pts, _edge_view(near=0.5), 1)
    assert sorted(index[index >= 0].tolist()) == [1, 3, 4, 5, 6]


@pytest.mark.parametrize("point_size", [1, 5])
def test_edge_not_finite_and_huge(gpu, point_size):
    good = _at([(8, 8)])
    bad = _pts(0)
    for f in ('x', 'y', 'z'):
        for v in (np.nan, np.inf, -np.inf):
            p = _at([(8, 8)], z=0.5)               # (in front of the good point if it were drawn)
            p[f] = v
            bad = np.concatenate([bad, p])
    pts = np.concatenate([bad, good])
    _, _, index, covered = _check(gpu, pts, _edge_view(), point_size)
    assert covered == point_size ** 2 and set(index[index >= 0].tolist()) == {9}
    # coordinates of 1e30: u and v far beyond any integer type, or a quotient of two huge numbers that lands in the image
    huge = _pts(6)
    huge['z'] = 1.0
    huge['x'][0], huge['y'][1], huge['x'][2], huge['y'][3] = 1e30, 1e30, -1e30, -1e30
    huge['x'][4], huge['z'][4] = 2.0 ** 99, 2.0 ** 100                       # u = 12
    huge['x'][5], huge['y'][5], huge['z'][5] = 1e30, -1e30, 1e-30            # u = +1e60 * 8, v alike
    huge['b'] = 50
    pts = np.concatenate([huge, good])
    _, depth, index, _ = _check(gpu, pts, _edge_view(), point_size)
    assert set(index[index >= 0].tolist()) == {4, 6} and depth[8, 12] == np.float32(2.0 ** 100)
    # ... and through a matrix that makes camera coordinates overflow
    _check(gpu, pts, _edge_view(extrinsic=np.diag([1e300, 1e300, 1.0, 1.0])), point_size)
    _check(gpu, pts, _edge_view(extrinsic=np.diag([1.0, 1.0, 1e300, 1.0])), point_size)


def test_edge_every_point_excluded(gpu):
    pts = _random_cloud(1025, True).copy()
    pts['z'] = -pts['z']
    rgb, depth, index, covered = _check(gpu, pts, _edge_view(), 5)
    assert covered == 0 and (index == -1).all() and (depth == 0).all() and (rgb.reshape(-1, 3) == BG).all()


# ---- contention and ties ----
@pytest.mark.parametrize("point_size", [1, 5])
def test_many_points_in_one_pixel(gpu, point_size):
    n = 100000
    rng = np.random.default_rng(9)
    base = _at([(8.5, 8.5)] * n)
    base['r'], base['g'], base['b'] = rng.integers(0, 256, (3, n))
    # distinct depths in a random order: the nearest wins
    pts = base.copy()
    pts['z'] = rng.permutation(n).astype(np.float32) / n + 1.0
    pts['x'] = pts['y'] = 0.0625 * pts['z']
    _, depth, index, covered = _check(gpu, pts, _edge_view(), point_size)
    assert covered == point_size ** 2 and index[8, 8] == int(np.argmin(pts['z'])) and depth[8, 8] == 1.0
    # ... also when it is the cloud's last point
    order = np.argsort(-pts['z'], kind='stable')
    _, _, index, _ = _check(gpu, pts[order], _edge_view(), point_size)
    assert index[8, 8] == n - 1
    # one depth: index 0 wins
    _, _, index, _ = _check(gpu, base, _edge_view(), point_size)
    assert (index[index >= 0] == 0).all()
    # the tie is among the cloud's last points only: the first of them wins
    pts = base.copy()
    pts['z'][:n - 100] = 2.0
    pts['x'] = pts['y'] = 0.0625 * pts['z']
    _, _, index, _ = _check(gpu, pts, _edge_view(), point_size)
    assert (index[index >= 0] == n - 100).all()


def test_tile_masks(gpu):
    pts = _random_cloud(1025, True).copy()
    pts['tile'] = np.array([1, 2, 4, 3], dtype=np.uint8)[np.arange(len(pts)) % 4]
    view = PinholeView(64, 64, 20.0, 20.0, 31.5, 31.5)
    for mask, tiles in ((0, {1, 2, 3, 4}), (1, {1, 3}), (2, {2, 3}), (6, {2, 3, 4}), (128, set())):
        _, _, index, covered = _check(gpu, pts, view, 3, mask)
        # index is a position in the unfiltered cloud
        assert set(pts['tile'][index[index >= 0]].tolist()) == tiles, mask
        assert (covered == 0) == (mask == 128)


# ---- calls ----
def test_repeatable_threads_wrapper_and_no_index(gpu):
    pts = _random_cloud(200001, False)
    pc = make_cloud(gpu, pts)
    view = _scaled_view(640, 480, look_at((0, 1, -3), (0, 1, 0), UP))
    first = _raw(gpu, pc, view)
    second = _raw(gpu, pc, view)
    assert first[0] == second[0] > 0
    for a, b in zip(first[1:], second[1:]):
        assert a.tobytes() == b.tobytes()
    box = []
    t = threading.Thread(target=lambda: box.append(_raw(gpu, pc, view)))
    t.start()
    t.join()
    assert box and box[0][0] == first[0] and all(a.tobytes() == b.tobytes() for a, b in zip(first[1:], box[0][1:]))
    # index = NULL
    rc, rgb, depth, index = _raw(gpu, pc, view, want_index=False)
    assert index is None and rc == first[0] and rgb.tobytes() == first[1].tobytes() and depth.tobytes() == first[2].tobytes()
    # the Python wrappers: open3d's point size and background by default
    w_rgb, w_depth, w_index = render_pointcloud(pc, view)
    white = _raw(gpu, pc, view, 5, 0, (255, 255, 255))
    assert w_rgb.tobytes() == white[1].tobytes() and w_depth.tobytes() == first[2].tobytes() and w_index.tobytes() == first[3].tobytes()
    assert w_rgb.shape == (480, 640, 3) and w_depth.shape == w_index.shape == (480, 640)
    assert gpu.cwipc_hip_render(pc, view.as_struct(), want_index=False)[2] is None


def test_errors(gpu):
    pts = _random_cloud(1025, True)
    pc = make_cloud(gpu, pts)
    dll = gpu.cwipc_util_dll_load()
    good = _edge_view()
    want = _raw(gpu, pc, good)

    def refused(view=good, point_size=5, call=None):
        if call is None:
            rc = _raw(gpu, pc, view, point_size)[0]
        else:
            rc = call()
        msg = dll.cwipc_hip_last_error().decode()
        assert rc == -1 and msg.startswith("cwipc_hip_render: ") and len(msg) > 20, (rc, msg)
        again = _raw(gpu, pc, good)        # a later valid call is not disturbed
        assert again[0] == want[0] and all(a.tobytes() == b.tobytes() for a, b in zip(want[1:], again[1:]))
        return msg

    s = good.as_struct()
    bg = (ctypes.c_uint8 * 3)(1, 2, 3)
    rgb, depth = np.zeros((16, 16, 3), np.uint8), np.zeros((16, 16), np.float32)
    args = [pc.as_cwipc_p(), ctypes.addressof(s), 5, 0, ctypes.addressof(bg), rgb.ctypes.data, depth.ctypes.data, None]
    for k in (0, 1, 4, 5, 6):
        a = list(args)
        a[k] = None
        assert "NULL" in refused(call=lambda: dll.cwipc_hip_render(*a))
    for w, h in ((0, 16), (16, 0), (-1, 16), (16, -3), (4097, 4096), (1 << 16, 1 << 16)):
        v = _edge_view()
        v.width, v.height = w, h
        assert "width" in refused(call=lambda v=v: _raw_small(gpu, pc, v))
    for ps in (0, 2, 4, 16, 17, -1, -5):
        assert "point_size" in refused(point_size=ps)
    for near, far in ((0.0, math.inf), (-1.0, 2.0), (math.nan, 2.0), (1.0, 1.0), (2.0, 1.0), (1.0, math.nan), (math.inf, math.inf)):
        assert "near" in refused(_edge_view(near=near, far=far))
    for f in ('fx', 'fy', 'cx', 'cy'):
        for bad in (math.nan, math.inf, -math.inf):
            v = _edge_view()
            setattr(v, f, bad)
            assert "finite" in refused(v)
    for at in ((0, 0), (1, 3), (2, 2), (3, 1), (3, 3)):
        for bad in (math.nan, math.inf):
            e = np.identity(4)
            e[at] = bad
            assert "finite" in refused(_edge_view(extrinsic=e))
    with pytest.raises(gpu.CwipcError, match="point_size"):
        gpu.cwipc_hip_render(pc, good.as_struct(), point_size=4)
    # the largest image that is accepted has 2^24 pixels
    big = PinholeView(4096, 4096, 2000.0, 2000.0, 2047.5, 2047.5)
    rc, _, depth, index = _raw(gpu, pc, big, 1)
    assert rc > 0 and rc == int((index >= 0).sum()) == int((depth > 0).sum())
    gpu.cwipc_util_dll_load().cwipc_hip_pool_trim()   # (the key and image buffers of that call: 300 MB the rest of the suite has no use for)


def _raw_small(gpu, pc, view):
    """A call with an image size the library must refuse, with arrays of one pixel."""
    s = view.as_struct()
    bg = (ctypes.c_uint8 * 3)(1, 2, 3)
    rgb, depth, index = np.zeros(3, np.uint8), np.zeros(1, np.float32), np.zeros(1, np.int32)
    return gpu.cwipc_util_dll_load().cwipc_hip_render(pc.as_cwipc_p(), ctypes.addressof(s), 5, 0, ctypes.addressof(bg), rgb.ctypes.data, depth.ctypes.data,
                                                    index.ctypes.data)
