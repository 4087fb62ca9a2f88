"""The numpy statement of the library's seeded random filters (include/cwipc_util_amd/hip_ext.h, csrc/counter_rng.hpp): the draws, the
noise filter's arithmetic (reference python/cwipc/filters/noise.py:31-50), the soft camera assignment (python/cwipc/filters/
simulatecams.py:44-70) and the composition the analysis-test creator runs.  Test infrastructure: the GPU results and the host
program's are compared with these for equality.  No reference module is imported and no code of it is run.
"""
import ctypes
import ctypes.util
import fractions
import math

import numpy as np

import exact_model
from floor_model import GOLDEN, MASK64, splitmix64

TAG_NOISE = 0x6e6f697365
TAG_CAMS = 0x63616d73


def base(seed, tag):
    return int(splitmix64(np.uint64((int(seed) + tag) & MASK64)))


def draw(b, k):
    """draw(b, k) = mix(b + (k + 1) * GOLDEN) on uint64 (wrapping) for an array (or one) k"""
    k = np.asarray(k, dtype=np.uint64)
    with np.errstate(over='ignore'):
        return splitmix64(np.uint64(b) + (k + np.uint64(1)) * np.uint64(GOLDEN))


def u01(x):
    """(double)(x >> 11) * 2^-53: exact (53 bits), in [0, 1)"""
    return (np.asarray(x, dtype=np.uint64) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def noise_draws(seed, n):
    """(n, 4) doubles: point i's u_0 .. u_3 = u01(draw(base(seed, noise), 4 i + j))"""
    return u01(draw(base(seed, TAG_NOISE), np.arange(4 * n, dtype=np.uint64))).reshape(n, 4)


def noise_vectors(u, distance):
    """n_c of the header, one numpy operation per rounding: (n, 3) float64"""
    u = np.asarray(u, dtype=np.float64).reshape(-1, 4)
    with np.errstate(all='ignore'):
        v = -1.0 + 2.0 * u[:, :3]
        s = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
        scale = np.sqrt(s) / u[:, 3]
        return (v / scale[:, None]) * np.float64(distance)


def noise_vectors_reference_expression(u, distance):
    """The reference's own expression (noise.py:46-50) on the same v and unif: uniform(-1, 1) is -1 + 2 u in numpy's generator"""
    u = np.asarray(u, dtype=np.float64).reshape(-1, 4)
    with np.errstate(all='ignore'):
        rnd_vec = -1.0 + 2.0 * u[:, :3]
        unif = u[:, 3]
        scale_f = np.expand_dims(np.linalg.norm(rnd_vec, axis=1) / unif, axis=1)
        rnd_vec = rnd_vec / scale_f
        return rnd_vec * distance


def add_noise(xyz, nvec):
    """`float32 += float64` (noise.py:35): evaluated in f64, rounded once to float32"""
    with np.errstate(all='ignore'):
        return (np.asarray(xyz, dtype=np.float32).astype(np.float64) + nvec).astype(np.float32)


def noise(pts, distance, seed):
    """cwipc_hip_noise on a structured point array"""
    out = pts.copy()
    if len(pts):
        xyz = add_noise(np.stack([pts['x'], pts['y'], pts['z']], axis=1), noise_vectors(noise_draws(seed, len(pts)), distance))
        out['x'], out['y'], out['z'] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    return out


def camera_vectors(ncam):
    cams = np.zeros((ncam, 3), dtype=float)
    for c in range(ncam):
        cams[c, 0], cams[c, 2] = np.cos(2 * np.pi * c / ncam), np.sin(2 * np.pi * c / ncam)
    return cams


def _fma_function():
    """fma(a, b, c) = a * b + c rounded once: Python's (3.13), the C library's, or exact rational arithmetic"""
    if hasattr(math, "fma"):
        return math.fma
    try:
        libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        libm.fma.argtypes, libm.fma.restype = [ctypes.c_double] * 3, ctypes.c_double
        return libm.fma
    except (OSError, AttributeError):
        return lambda a, b, c: float(fractions.Fraction(a) * fractions.Fraction(b) + fractions.Fraction(c))


_fma = _fma_function()


def camera_dots(x, z, centroid, cams):
    """(n, ncam) float64: position minus centroid in float32, then fl(vx * cx) and one fused multiply-add for vz * cz (numpy.dot)"""
    vx = (np.asarray(x, dtype=np.float32) - np.float32(centroid[0])).astype(np.float32).astype(np.float64)
    vz = (np.asarray(z, dtype=np.float32) - np.float32(centroid[2])).astype(np.float32).astype(np.float64)
    dots = np.zeros((len(vx), len(cams)))
    for c, (cx, _, cz) in enumerate(cams):
        prod = vx * cx
        dots[:, c] = [_fma(float(a), float(cz), float(p)) for a, p in zip(vz, prod)]
    return dots


def cams_draws(seed, n):
    return u01(draw(base(seed, TAG_CAMS), np.arange(n, dtype=np.uint64)))


def soft_cameras(dots, skew, u):
    """(camera, chance, w0, w1) per point: the top two of the reversed stable ascending sort, the weights and the chance"""
    order = np.argsort(dots, axis=1, kind="stable")[:, ::-1]
    first, second = order[:, 0], order[:, 1]
    rows = np.arange(len(dots))
    d0, d1 = dots[rows, first], dots[rows, second]
    with np.errstate(all='ignore'):
        w0, w1 = (d0, d1) if skew == 1.0 else (np.power(d0, np.float64(skew)), np.power(d1, np.float64(skew)))
        chance = -w0 + (w1 + w0) * u
    return np.where(chance < 0, first, second), chance, w0, w1


def soft_tiles(pts, centroid, ncam, skew, seed):
    """(tile bytes, mask of the points whose choice hangs on the last bits of pow)"""
    dots = camera_dots(pts['x'], pts['z'], centroid, camera_vectors(ncam))
    cam, chance, w0, w1 = soft_cameras(dots, skew, cams_draws(seed, len(pts)))
    with np.errstate(all='ignore'):
        fragile = (np.abs(chance) > 0) & (np.abs(chance) <= 1e-12 * (np.abs(w0) + np.abs(w1)))
    return ((1 << cam) & 0xff).astype(np.uint8), fragile if skew != 1.0 else np.zeros(len(pts), dtype=bool)


def transform(pts, m):
    """cwipc_transform (reference python/cwipc/registration/util.py:295-309): R @ p + t in float64, stored as float32"""
    m = np.asarray(m, dtype=np.float64)
    xyz = np.stack([pts['x'], pts['y'], pts['z']], axis=1)
    moved = (m[:3, :3] @ xyz.transpose()).transpose() + m[:3, 3].transpose()
    out = pts.copy()
    out['x'], out['y'], out['z'] = moved[:, 0].astype(np.float32), moved[:, 1].astype(np.float32), moved[:, 2].astype(np.float32)
    return out


def tie_inputs():
    """The inputs of tests/test_gpu_exact_filters.py's camera tests, made again: every point on the centroid; points on the bisectors of four
    cameras (|x| == |z| around the centroid); random finite points."""
    rng = np.random.default_rng(4)
    on = exact_model.edge_cloud(rng, 300, special=0.0)
    on['x'], on['z'] = np.float32(0.3), np.float32(-1.7)
    t = np.concatenate([2.0 ** np.arange(-20, 4), rng.random(76) * 3]).astype(np.float32)
    bis = exact_model.empty(4 * len(t))
    bis['x'] = np.concatenate([t, -t, -t, t])
    bis['z'] = np.concatenate([t, t, -t, -t])
    bis['y'] = rng.random(len(bis))
    bis['tile'] = 200
    rnd = exact_model.edge_cloud(rng, 600, special=0.1, finite=True)
    return {"on the centroid": (on, (np.float32(0.3), 0.0, np.float32(-1.7))), "bisectors": (bis, (0.0, 0.0, 0.0)),
            "random": (rnd, (np.float32(0.1), 0.0, np.float32(-0.2)))}


def ks_distance_from_uniform(values):
    """sup |F_n(x) - x| of a sample against the uniform distribution on [0, 1]"""
    v = np.sort(np.asarray(values, dtype=np.float64))
    n = len(v)
    i = np.arange(1, n + 1)
    return float(max((i / n - v).max(), (v - (i - 1) / n).max()))
