"""The numpy statement of the raw entry's depth decimation and hole filling (test infrastructure): what a decimated rig
(cwipc_hip_rgbd_rig_create_decimated) makes of a full-size depth image before anything else, and what cwipc_hip_rgbd_rig_grab_filled
makes of the depth images between the temporal filter and the erosion, written from the contract (include/cwipc_util_amd/hip_ext.h
RULE D and rule 0c), not from the code under test.  float64 elementwise operations in the stated order;
q(x) = (uint16) floor(x + 0.5).

    RULE D:  W' = W div k;  H' = H div k;  fx' = fx / k;  fy' = fy / k;  cx' = (cx - (k - 1) * 0.5) / k;  cy' alike
             pixel (U, V), n the number of non-zero values among its k * k source pixels:  n == 0: 0
             k = 2, 3: the lower median, sorted ascending a[(n - 1) div 2];   k = 4 .. 8: q(sum / n) over the non-zero values
    rule 0c: mode 1: a hole takes the nearest value with depth to its left in its row, none: 0
             mode 2 / 3: a hole takes the largest / smallest non-zero value among its up to eight neighbours of the INPUT, none: 0
             a pixel with depth is never changed"""
import numpy as np

import rgbd_depthfilter_model as dm
import rgbd_lens_model as lm
import rgbd_model as rm
import rgbd_occlusion_model as om


def derived_sensor(s, k):
    """lm.Sensor s on the grid decimated by k: size and depth intrinsics change, nothing else does."""
    k64 = np.float64(k)
    fx, fy = np.float64(s.fx) / k64, np.float64(s.fy) / k64
    shift = np.float64(k - 1) * np.float64(0.5)
    cx, cy = (np.float64(s.cx) - shift) / k64, (np.float64(s.cy) - shift) / k64
    return s._replace(width=s.width // k, height=s.height // k, fx=float(fx), fy=float(fy), cx=float(cx), cy=float(cy))


def decimate(depth, k):
    """uint16[H, W] -> uint16[H div k, W div k]"""
    depth = np.asarray(depth, dtype=np.uint16)
    if k == 1:
        return depth.copy()
    h, w = depth.shape[0] // k, depth.shape[1] // k
    blocks = depth[:h * k, :w * k].reshape(h, k, w, k).transpose(0, 2, 1, 3).reshape(h, w, k * k).astype(np.int64)
    n = (blocks != 0).sum(axis=2)
    if k <= 3:
        ordered = np.sort(np.where(blocks != 0, blocks, 1 << 16), axis=2)          # the holes behind every depth
        at = np.maximum(n - 1, 0) // 2
        value = np.take_along_axis(ordered, at[..., None], axis=2)[..., 0]
    else:
        total = blocks.sum(axis=2)
        with np.errstate(all='ignore'):
            value = np.floor(total.astype(np.float64) / np.maximum(n, 1).astype(np.float64) + np.float64(0.5)).astype(np.int64)
    return np.where(n > 0, value, 0).astype(np.uint16)


def holefill(depth, mode):
    """Rule 0c on uint16[H, W]; mode 0: a copy."""
    depth = np.asarray(depth, dtype=np.uint16)
    if mode == 0:
        return depth.copy()
    h, w = depth.shape
    if mode == 1:
        # the column of the nearest pixel with depth at or left of each pixel, -1: none
        cols = np.where(depth != 0, np.arange(w)[None, :], -1)
        last = np.maximum.accumulate(cols, axis=1)
        taken = np.take_along_axis(depth, np.maximum(last, 0), axis=1)
        return np.where(last >= 0, taken, 0).astype(np.uint16)
    if mode not in (2, 3):
        raise ValueError("hole-fill mode %r" % (mode,))
    empty = 0 if mode == 2 else 1 << 16
    padded = np.full((h + 2, w + 2), empty, dtype=np.int64)
    padded[1:-1, 1:-1] = np.where(depth != 0, depth.astype(np.int64), empty)
    best = np.full((h, w), empty, dtype=np.int64)
    for dv in range(3):
        for du in range(3):
            if (dv, du) != (1, 1):
                shifted = padded[dv:dv + h, du:du + w]
                best = np.maximum(best, shifted) if mode == 2 else np.minimum(best, shifted)
    best = np.where(best == empty, 0, best)
    return np.where(depth != 0, depth, best).astype(np.uint16)


def decimated_depth_filter(frames, histories, k, depthfilter=None, mode=0):
    """One full-size frame -- per camera its (depth, colour) -- through RULE D, rules 0a / 0b (rgbd_depthfilter_model, the histories on
    the decimated grid) and rule 0c: the frame rules 1-4 run on, with the derived sensors."""
    small = [(decimate(depth, k), colour) for depth, colour in frames]
    filtered = dm.depth_filter(small, histories, depthfilter)
    return [(holefill(depth, mode), colour) for depth, colour in filtered]


def cloud(models, frame, k, histories=None, depthfilter=None, mode=0, flt=rm.Filter(), ex=0, ey=0, occlusion=None, tables=None):
    """(the derived sensors, (points, [depth images used], [registered images])) of a full-size frame on a rig decimated by k.
    occlusion: None or (splat, margin).  tables: the derived sensors' ray tables, where they have been computed already."""
    derived = [derived_sensor(m, k) for m in models]
    grid = decimated_depth_filter(frame, histories, k, depthfilter, mode)
    if occlusion is None:
        return derived, lm.cloud(derived, grid, flt, ex, ey, tables)
    return derived, om.cloud(derived, grid, flt, ex, ey, tables, occlusion[0], occlusion[1])
