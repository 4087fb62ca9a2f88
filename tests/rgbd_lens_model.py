"""The numpy statement of the RGB-D source's raw entry (test infrastructure): what cwipc_hip_rgbd_rig_grab must give, written from its
contract (include/cwipc_util_amd/hip_ext.h), not from the code under test.  Float64 elementwise operations in the stated
order -- numpy rounds each on its own -- and no `@`.  The world point and the four filters are tests/rgbd_model.py's.

    distort(x, y):  xx = x*x; yy = y*y; r2 = xx + yy
                    num = 1 + r2*(k1 + r2*(k2 + r2*k3)); den = 1 + r2*(k4 + r2*(k5 + r2*k6)); rad = num / den
                    a1 = (2*x)*y; a2 = r2 + 2*xx; a3 = r2 + 2*yy
                    x' = (x*rad + p1*a1) + p2*a2;  y' = (y*rad + p1*a3) + p2*a1
    ray(u, v):      Newton's method on distort(x, y) = ((u - cx)/fx, (v - cy)/fy) from that point, at most 20 steps, accepted when both
                    residuals are below 1e-12 and the Jacobian's determinant is positive there; else (NaN, NaN)
    point:          z = d*depth_scale; xc = xn*z; yc = yn*z (all depth coefficients zero: rgbd_model's xc, yc); then rgbd_model's world
    colour pixel:   P = depth_to_colour . (xc, yc, z), each row ((m0*xc + m1*yc) + m2*z) + m3; none if Pz <= 0 or not finite;
                    (x', y') = distort(Px/Pz, Py/Pz); uc = floor((fxc*x' + cxc) + 0.5), vc alike; none outside [0, Wc) x [0, Hc)
    erosion:        a row pass, then a column pass, each over the pixels inside the image"""
from collections import namedtuple

import numpy as np

import rgbd_model as rm

PINHOLE = (0.0,) * 8
NEWTON_STEPS = 20
NEWTON_EPS = 1e-12

#: one raw camera.  coeffs: k1 k2 p1 p2 k3 k4 k5 k6.  The colour side: colour_size (Wc, Hc), bpp, colour_intr (fx, fy, cx, cy),
#: colour_coeffs, depth_to_colour (4 x 4).  trafo: camera -> world (4 x 4)
Sensor = namedtuple("Sensor", "width height fx fy cx cy coeffs depth_scale colour_size bpp colour_intr colour_coeffs depth_to_colour trafo tile")


def _radial(k, x, y):
    k1, k2, _p1, _p2, k3, k4, k5, k6 = (np.float64(c) for c in k)
    xx, yy = x * x, y * y
    r2 = xx + yy
    num = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
    den = 1.0 + r2 * (k4 + r2 * (k5 + r2 * k6))
    return xx, yy, r2, num, den, num / den


def _distort_with(k, radial, x, y):
    p1, p2 = np.float64(k[2]), np.float64(k[3])
    xx, yy, r2, _num, _den, rad = radial
    a1 = (2.0 * x) * y
    a2 = r2 + 2.0 * xx
    a3 = r2 + 2.0 * yy
    return (x * rad + p1 * a1) + p2 * a2, (y * rad + p1 * a3) + p2 * a1


def distort(k, x, y):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    with np.errstate(all='ignore'):
        return _distort_with(k, _radial(k, x, y), x, y)


def _jacobian(k, radial, x, y):
    k1, k2, p1, p2, k3, k4, k5, k6 = (np.float64(c) for c in k)
    xx, yy, r2, num, den, rad = radial
    dn = k1 + r2 * (2.0 * k2 + r2 * (3.0 * k3))
    dd = k4 + r2 * (2.0 * k5 + r2 * (3.0 * k6))
    g = (dn * den - num * dd) / (den * den)
    j00 = ((rad + (2.0 * xx) * g) + (2.0 * p1) * y) + (6.0 * p2) * x
    j01 = (((2.0 * x) * y) * g + (2.0 * p1) * x) + (2.0 * p2) * y
    j11 = ((rad + (2.0 * yy) * g) + (6.0 * p1) * y) + (2.0 * p2) * x
    return j00, j01, j01, j11, j00 * j11 - j01 * j01


def jacobian_det(k, x, y):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    with np.errstate(all='ignore'):
        return _jacobian(k, _radial(k, x, y), x, y)[4]


def undistort(k, xd, yd):
    """The rays of distorted normalised coordinates (arrays of one shape): (x, y), NaN where there is none."""
    xd, yd = np.asarray(xd, dtype=np.float64), np.asarray(yd, dtype=np.float64)
    if all(c == 0.0 for c in k):
        return xd.copy(), yd.copy()
    x, y = xd.copy(), yd.copy()
    out_x, out_y = np.full(xd.shape, np.nan), np.full(xd.shape, np.nan)
    done = np.zeros(xd.shape, dtype=bool)
    with np.errstate(all='ignore'):
        for step in range(NEWTON_STEPS + 1):
            radial = _radial(k, x, y)
            ax, ay = _distort_with(k, radial, x, y)
            ex, ey = ax - xd, ay - yd
            j00, j01, j10, j11, det = _jacobian(k, radial, x, y)
            small = ~done & (np.abs(ex) < NEWTON_EPS) & (np.abs(ey) < NEWTON_EPS)
            accept = small & (det > 0.0)
            out_x[accept], out_y[accept] = x[accept], y[accept]
            done |= small
            if step == NEWTON_STEPS or done.all():
                break
            x = np.where(done, x, x - (j11 * ex - j01 * ey) / det)
            y = np.where(done, y, y - (j00 * ey - j10 * ex) / det)
    return out_x, out_y


def ray_table(width, height, fx, fy, cx, cy, k):
    """float64[height, width, 2]"""
    v, u = np.meshgrid(np.arange(height), np.arange(width), indexing='ij')
    xd = (u.astype(np.float64) - np.float64(cx)) / np.float64(fx)
    yd = (v.astype(np.float64) - np.float64(cy)) / np.float64(fy)
    return np.stack(undistort(k, xd, yd), axis=-1)


def colour_pixel(intr, k, m, size, xc, yc, z):
    """(has a colour pixel, uc, vc) of points in depth-camera coordinates; uc, vc are 0 where there is none."""
    m = np.asarray(m, dtype=np.float64)
    fx, fy, cx, cy = (np.float64(c) for c in intr)
    with np.errstate(all='ignore'):
        px, py, pz = [((m[row, 0] * xc + m[row, 1] * yc) + m[row, 2] * z) + m[row, 3] for row in range(3)]
        front = (pz > 0.0) & np.isfinite(pz)
        ax, ay = distort(k, px / pz, py / pz)
        uc = np.floor((fx * ax + cx) + 0.5)
        vc = np.floor((fy * ay + cy) + 0.5)
        ok = front & (uc >= 0.0) & (uc < float(size[0])) & (vc >= 0.0) & (vc < float(size[1]))
    return ok, np.where(ok, uc, 0.0).astype(np.int64), np.where(ok, vc, 0.0).astype(np.int64)


def erode(depth, ex, ey):
    """The separable statement: a row pass over the validity mask, then a column pass; pixels outside the image do not erode."""
    valid = depth != 0
    height, width = valid.shape
    rows = valid.copy()
    for s in range(1, min(ex, width - 1) + 1):
        rows[:, :-s] &= valid[:, s:]
        rows[:, s:] &= valid[:, :-s]
    out = rows.copy()
    for s in range(1, min(ey, height - 1) + 1):
        out[:-s, :] &= rows[s:, :]
        out[s:, :] &= rows[:-s, :]
    return np.where(out, depth, 0).astype(depth.dtype)


def erode_brute(depth, ex, ey):
    """The definition, pixel by pixel."""
    height, width = depth.shape
    out = depth.copy()
    for v in range(height):
        for u in range(width):
            window = depth[max(v - ey, 0): v + ey + 1, max(u - ex, 0): u + ex + 1]
            if (window == 0).any():
                out[v, u] = 0
    return out


def sensor_frame(s, flt, depth, colour, ex=0, ey=0, table=None):
    """One camera: (its points, the depth image the cloud is made from, the registered RGB8 image)."""
    eroded = erode(depth, ex, ey)
    v, u = np.meshgrid(np.arange(s.height), np.arange(s.width), indexing='ij')
    cam = rm.Camera(s.fx, s.fy, s.cx, s.cy, s.depth_scale, s.trafo, s.tile, 3)
    z = eroded.astype(np.float64) * np.float64(s.depth_scale)
    with np.errstate(all='ignore'):
        if all(c == 0.0 for c in s.coeffs):
            xc = (u.astype(np.float64) - np.float64(s.cx)) * z / np.float64(s.fx)
            yc = (v.astype(np.float64) - np.float64(s.cy)) * z / np.float64(s.fy)
        else:
            if table is None:
                table = ray_table(s.width, s.height, s.fx, s.fy, s.cx, s.cy, s.coeffs)
            xc, yc = table[..., 0] * z, table[..., 1] * z
        ok, uc, vc = colour_pixel(s.colour_intr, s.colour_coeffs, s.depth_to_colour, s.colour_size, xc, yc, z)
        has = (eroded != 0) & ok
        used = np.where(has, eroded, 0).astype(np.uint16)
        planes = rm.split_colour(rm.Camera(0, 0, 0, 0, 0, None, 0, s.bpp), colour)
        registered = np.zeros((s.height, s.width, 3), dtype=np.uint8)
        for c in range(3):
            registered[..., c] = np.where(has, planes[c][vc, uc], 0)
        m = np.asarray(s.trafo, dtype=np.float64)
        x, y, zw = [(((m[row, 0] * xc + m[row, 1] * yc) + m[row, 2] * z) + m[row, 3]).astype(np.float32) for row in range(3)]
    keep = has.copy()
    r, g, b = registered[..., 0], registered[..., 1], registered[..., 2]
    if not flt.threshold_far <= flt.threshold_near:
        keep &= ~((z < flt.threshold_near) | (z > flt.threshold_far))
    if not flt.height_min == flt.height_max:
        y64 = y.astype(np.float64)
        keep &= ~((y64 < flt.height_min) | (y64 > flt.height_max))
    if not np.float32(flt.radius) <= 0:
        d2 = (x.astype(np.float64) * x.astype(np.float64) + zw.astype(np.float64) * zw.astype(np.float64)).astype(np.float32)
        keep &= d2 < np.float32(flt.radius) * np.float32(flt.radius)
    if flt.greenscreen:
        keep &= ~rm.in_hue_window(r, g, b)
    out = np.zeros(int(keep.sum()), dtype=rm.POINT_DTYPE)
    out['x'], out['y'], out['z'] = x[keep], y[keep], zw[keep]
    out['r'], out['g'], out['b'] = r[keep], g[keep], b[keep]
    out['tile'] = cam.tile
    return out, used, registered


def cloud(sensors, frame, flt=rm.Filter(), ex=0, ey=0, tables=None):
    """The whole frame: (points, [depth images used], [registered images]), the cameras in order."""
    parts = [sensor_frame(s, flt, depth, colour, ex, ey, None if tables is None else tables[i]) for i, (s, (depth, colour)) in enumerate(zip(sensors, frame))]
    return np.concatenate([p[0] for p in parts]), [p[1] for p in parts], [p[2] for p in parts]
