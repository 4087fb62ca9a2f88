"""The numpy statement of the raw entry's occlusion test (test infrastructure): what cwipc_hip_rgbd_rig_grab_occluded must give, written
from its contract (include/cwipc_util_amd/hip_ext.h rules 3a and 3b), not from the code under test.  Everything up to the
colour pixel is tests/rgbd_lens_model.py's; float64 elementwise operations in the stated order.

    candidate:   a depth pixel with depth after erosion and a colour pixel (uc, vc) -- so a ray, and Pz finite and > 0
    Zmin(a, b):  per camera, the minimum of Pz(q) over the candidates q with |uc(q) - a| <= splat and |vc(q) - b| <= splat; a
                 candidate writes the cells of its square that lie inside the colour image (+inf where nobody writes)
    occluded:    Zmin(uc(p), vc(p)) < Pz(p) - margin; such a pixel is a pixel without a colour: no point, depth 0, colour black
    then the four filters and the compaction, as without occlusion"""
import numpy as np

import rgbd_lens_model as lm
import rgbd_model as rm


def projection(s, eroded, table=None):
    """Of one camera's eroded depth image: (xc, yc, z, candidate mask, uc, vc, Pz), arrays of the depth image's shape."""
    v, u = np.meshgrid(np.arange(s.height), np.arange(s.width), indexing='ij')
    z = eroded.astype(np.float64) * np.float64(s.depth_scale)
    with np.errstate(all='ignore'):
        if all(c == 0.0 for c in s.coeffs):
            xc = (u.astype(np.float64) - np.float64(s.cx)) * z / np.float64(s.fx)
            yc = (v.astype(np.float64) - np.float64(s.cy)) * z / np.float64(s.fy)
        else:
            if table is None:
                table = lm.ray_table(s.width, s.height, s.fx, s.fy, s.cx, s.cy, s.coeffs)
            xc, yc = table[..., 0] * z, table[..., 1] * z
        ok, uc, vc = lm.colour_pixel(s.colour_intr, s.colour_coeffs, s.depth_to_colour, s.colour_size, xc, yc, z)
        m = np.asarray(s.depth_to_colour, dtype=np.float64)
        pz = ((m[2, 0] * xc + m[2, 1] * yc) + m[2, 2] * z) + m[2, 3]
    return xc, yc, z, (eroded != 0) & ok, uc, vc, pz


def zbuffer(size, cand, uc, vc, pz, splat):
    """float64[Hc, Wc]: Zmin, +inf where no candidate's square reaches."""
    wc, hc = size
    zmin = np.full((hc, wc), np.inf)
    a, b, depth = uc[cand], vc[cand], pz[cand]
    for dv in range(-splat, splat + 1):
        for du in range(-splat, splat + 1):
            col, row = a + du, b + dv
            inside = (col >= 0) & (col < wc) & (row >= 0) & (row < hc)
            np.minimum.at(zmin, (row[inside], col[inside]), depth[inside])
    return zmin


def occluded(zmin, cand, uc, vc, pz, margin):
    """The candidates that something nearer hides from the colour camera."""
    with np.errstate(all='ignore'):
        return cand & (zmin[vc, uc] < pz - np.float64(margin))


def sensor_frame(s, flt, depth, colour, ex=0, ey=0, table=None, splat=1, margin=0.02):
    """One camera: (its points, the depth image the cloud is made from, the registered RGB8 image, the occluded mask)."""
    eroded = lm.erode(depth, ex, ey)
    xc, yc, z, cand, uc, vc, pz = projection(s, eroded, table)
    hidden = occluded(zbuffer(s.colour_size, cand, uc, vc, pz, splat), cand, uc, vc, pz, margin)
    has = cand & ~hidden
    used = np.where(has, eroded, 0).astype(np.uint16)
    planes = rm.split_colour(rm.Camera(0, 0, 0, 0, 0, None, 0, s.bpp), colour)
    registered = np.zeros((s.height, s.width, 3), dtype=np.uint8)
    for c in range(3):
        registered[..., c] = np.where(has, planes[c][vc, uc], 0)
    m = np.asarray(s.trafo, dtype=np.float64)
    with np.errstate(all='ignore'):
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
    out['tile'] = s.tile
    return out, used, registered, hidden


def cloud(sensors, frame, flt=rm.Filter(), ex=0, ey=0, tables=None, splat=1, margin=0.02):
    """The whole frame: (points, [depth images used], [registered images], [occluded masks]), the cameras in order."""
    parts = [sensor_frame(s, flt, depth, colour, ex, ey, None if tables is None else tables[i], splat, margin)
             for i, (s, (depth, colour)) in enumerate(zip(sensors, frame))]
    return np.concatenate([p[0] for p in parts]), [p[1] for p in parts], [p[2] for p in parts], [p[3] for p in parts]
