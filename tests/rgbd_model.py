"""The numpy statement of the RGB-D source (test infrastructure): what cwipc_hip_from_rgbd must give, written from its contract
(include/cwipc_util_amd/hip_ext.h) and from the reference's capturer header (include/cwipc_util/internal/capturers.hpp:208-275), not from
the code under test.  Float64 elementwise operations in the stated order -- numpy rounds each on its own -- no `@`, and np.trunc for the
hue's C integer division.

    z  = (double)d * depth_scale;  xc = ((double)u - cx) * z / fx;  yc = ((double)v - cy) * z / fy
    X  = ((m00*xc + m01*yc) + m02*z) + m03, Y and Z alike;  the point is float32(X, Y, Z)
    filters, in order: depth range (z), height (float32 world y), radius (float32 world x, z), green screen (integer hue)."""
from collections import namedtuple

import numpy as np

POINT_DTYPE = [('x', '<f4'), ('y', '<f4'), ('z', '<f4'), ('r', 'u1'), ('g', 'u1'), ('b', 'u1'), ('tile', 'u1')]

#: the filters' settings; the defaults are "off" (far <= near, height_min == height_max, radius <= 0, greenscreen false)
Filter = namedtuple("Filter", "threshold_near threshold_far height_min height_max radius greenscreen", defaults=(0.0, 0.0, 0.0, 0.0, 0.0, False))
#: one camera: intrinsics, metres per depth unit, camera -> world matrix (4 x 4), tile, colour format (3: R, G, B; 4: B, G, R, A)
Camera = namedtuple("Camera", "fx fy cx cy depth_scale trafo tile bpp", defaults=(1, 3))


def points(cam, u, v, d):
    """float32 x, y, z of pixels (u, v) with depths d (arrays of one shape), and z along the camera's axis in float64."""
    m = np.asarray(cam.trafo, dtype=np.float64)
    z = d.astype(np.float64) * np.float64(cam.depth_scale)
    xc = (u.astype(np.float64) - np.float64(cam.cx)) * z / np.float64(cam.fx)
    yc = (v.astype(np.float64) - np.float64(cam.cy)) * z / np.float64(cam.fy)
    world = [(((m[row, 0] * xc + m[row, 1] * yc) + m[row, 2] * z) + m[row, 3]).astype(np.float32) for row in range(3)]
    return world[0], world[1], world[2], z


def trunc_div(a, b):
    """C's integer division: towards zero."""
    return np.trunc(a.astype(np.float64) / b.astype(np.float64)).astype(np.int64)


def hue(r, g, b, floor=False):
    """The reference's rgbToHsv, the h field: unsigned char fields, int arithmetic, the result stored into an unsigned char.  floor=True:
    with Python's floor division instead -- what the hue must NOT be."""
    r, g, b = (np.asarray(c).astype(np.int64) for c in (r, g, b))
    mn, mx = np.minimum(np.minimum(r, g), b), np.maximum(np.maximum(r, g), b)
    delta = mx - mn
    safe_mx, safe_delta = np.where(mx == 0, 1, mx), np.where(delta == 0, 1, delta)
    div = (lambda a, b_: a // b_) if floor else trunc_div
    s = trunc_div(255 * delta, safe_mx) & 255
    h = np.where(mx == r, 0 + div(43 * (g - b), safe_delta), np.where(mx == g, 85 + div(43 * (b - r), safe_delta), 171 + div(43 * (r - g), safe_delta))) & 255
    h = np.where((mx == 0) | (s == 0), 0, h)
    return h, np.where(mx == 0, 0, s), mx


def in_hue_window(r, g, b):
    h, _s, _v = hue(r, g, b)
    return (h >= 60) & (h <= 130)


def is_not_green_full(r, g, b):
    """The reference's isNotGreen, all of it: (what it returns, the r and b it leaves behind -- as integers, before they are stored
    back into an unsigned char, which is undefined in C++ where they pass 255)."""
    r, g, b = (np.asarray(c).astype(np.int64) for c in (r, g, b))
    h, s, v = hue(r, g, b)
    window = (h >= 60) & (h <= 130)
    reduce = window & (s >= 0.15) & (v >= 0.15)
    rb = r * b
    strong = (rb != 0) & (trunc_div(g * g, np.where(rb == 0, 1, rb)) > 1.5)
    factor = np.where(strong, 1.4, 1.2)
    new_r = np.where(reduce, np.trunc(r * factor).astype(np.int64), r)
    new_b = np.where(reduce, np.trunc(b * factor).astype(np.int64), b)
    return np.where(window, ~((s >= 0.4) & (v >= 0.3)), True), new_r, new_b


def split_colour(cam, colour):
    """r, g, b planes of a colour image of the camera's format."""
    if cam.bpp == 3:
        return colour[..., 0], colour[..., 1], colour[..., 2]
    return colour[..., 2], colour[..., 1], colour[..., 0]


def keep_mask(cam, flt, u, v, d, r, g, b):
    """Which pixels give a point, and their points."""
    x, y, z, zc = points(cam, u, v, d)
    keep = d != 0
    if not flt.threshold_far <= flt.threshold_near:
        keep &= ~((zc < flt.threshold_near) | (zc > flt.threshold_far))
    if not flt.height_min == flt.height_max:
        y64 = y.astype(np.float64)
        keep &= ~((y64 < flt.height_min) | (y64 > flt.height_max))
    if not np.float32(flt.radius) <= 0:
        d2 = (x.astype(np.float64) * x.astype(np.float64) + z.astype(np.float64) * z.astype(np.float64)).astype(np.float32)
        keep &= d2 < np.float32(flt.radius) * np.float32(flt.radius)
    if flt.greenscreen:
        keep &= ~in_hue_window(r, g, b)
    return keep, x, y, z


def camera_cloud(cam, flt, depth, colour):
    """One camera's points: the kept pixels in row-major order."""
    height, width = depth.shape
    v, u = np.meshgrid(np.arange(height), np.arange(width), indexing='ij')
    r, g, b = split_colour(cam, colour)
    keep, x, y, z = keep_mask(cam, flt, u, v, depth, r, g, b)
    out = np.zeros(int(keep.sum()), dtype=POINT_DTYPE)
    out['x'], out['y'], out['z'] = x[keep], y[keep], z[keep]
    out['r'], out['g'], out['b'] = r[keep], g[keep], b[keep]
    out['tile'] = cam.tile
    return out


def cloud(cameras, frame, flt=Filter()):
    """The whole frame's points: the cameras in order."""
    return np.concatenate([camera_cloud(cam, flt, depth, colour) for cam, (depth, colour) in zip(cameras, frame)])


def random_rigid(rng, spread=2.0):
    """A rotation (QR of a Gaussian matrix, made proper) and a translation as a 4 x 4 matrix."""
    q, _r = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    m = np.identity(4)
    m[:3, :3], m[:3, 3] = q, rng.uniform(-spread, spread, 3)
    return m
