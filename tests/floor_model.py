"""What the reference's floor and tile helpers compute (python/cwipc/registration/util.py:146-229), restated in numpy on the
structured point array (fields x, y, z, r, g, b, tile) instead of the reference's (n, 7) float32 matrix -- the matrix holds the
same float32 coordinates and the bytes as floats, so selecting rows of one selects the same points of the other.  Test
infrastructure: the GPU results are compared with these for equality.  The reference module itself is not imported (it needs
open3d) and no code of it is run.

Line references are to python/cwipc/registration/util.py unless stated otherwise.
"""
import numpy as np

POINT_DTYPE = [('x', '<f4'), ('y', '<f4'), ('z', '<f4'), ('r', 'u1'), ('g', 'u1'), ('b', 'u1'), ('tile', 'u1')]
MASK64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


def empty(n):
    return np.zeros(n, dtype=POINT_DTYPE)


def is_floor(pts, level):
    """:149, :160, :206, :221 -- `pc_np[:,1] < level`: numpy's comparison of the float32 column with the scalar as it is handed
    in (a Python float is rounded to float32 first, an np.float64 is not); NaN < level is False."""
    with np.errstate(invalid='ignore'):
        return pts['y'] < level


def threshold(value):
    """The double d for which `(double)y < d` is numpy's `y < value` for every float32 y: the comparison happens in
    result_type(float32, value)."""
    return float(np.result_type(np.float32, value).type(value))


def norm3(x, y, z):
    """numpy.linalg.norm(m[:, 0:3], axis=1) of float32 rows (:224): sqrt(add.reduce(m * m, axis=1)) -- the squares and the two
    additions in index order, each rounded to float32, then the correctly rounded float32 root."""
    x, y, z = (np.asarray(v, dtype=np.float32) for v in (x, y, z))
    with np.errstate(over='ignore', invalid='ignore'):
        return np.sqrt((x * x + y * y) + z * z)


def floor_filter(pts, level=0.1, keep=False):
    """:146-155"""
    f = is_floor(pts, level)
    return pts[f] if keep else pts[~f]


def limit_floor_to_radius(pts, radius, level=0.1):
    """:218-229 -- the floor points whose norm (all three coordinates, :224) is below the radius, then the other points"""
    f = is_floor(pts, level)
    floor, rest = pts[f], pts[~f]
    with np.errstate(invalid='ignore'):
        near = norm3(floor['x'], floor['y'], floor['z']) < radius
    return np.concatenate((floor[near], rest))


def splitmix64(z):
    """One splitmix64 output step on uint64 values (wrapping arithmetic)."""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over='ignore'):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def shuffle_keys(seed, n):
    i = np.arange(1, n + 1, dtype=np.uint64)
    with np.errstate(over='ignore'):
        return splitmix64(np.uint64(seed & MASK64) + i * np.uint64(GOLDEN))


def permutation_from_keys(keys):
    """The stable ascending argsort: of equal keys the lower index first."""
    return np.argsort(np.asarray(keys, dtype=np.uint64), kind='stable')


def randomize_floor(pts, level=0.1, seed=0):
    """:157-168 with the library's permutation in place of numpy.random.shuffle: floor point j takes the tile of floor point perm[j]"""
    f = is_floor(pts, level)
    floor, rest = pts[f].copy(), pts[~f]
    perm = permutation_from_keys(shuffle_keys(seed, len(floor)))
    floor['tile'] = floor['tile'][perm]
    return np.concatenate((floor, rest))


def xz_distances(pts):
    """:209-212 -- y set to 0, then the norm of the rows: sqrt((x*x + 0) + z*z) in float32"""
    return norm3(pts['x'], np.zeros(len(pts), dtype=np.float32), pts['z'])


def percentile99_neighbours(n):
    """The indices numpy.percentile(d, 99) interpolates between for n float32 values and the weight of the upper one: for
    float32 data numpy divides 99 by float32(100) and computes the virtual index (n - 1) * q in float32 (numpy
    lib/_function_base_impl.py, percentile / _quantile / _get_gamma, method 'linear')."""
    virtual = np.float32(n - 1) * np.float32(0.99)
    lo = int(np.floor(virtual))
    return lo, min(lo + 1, n - 1), np.float32(virtual - np.float32(lo))


def percentile99(values):
    """numpy.percentile(values, 99) of float32 values, spelled out: a + (b - a) * g, or b - (b - a) * (1 - g) where g >= 0.5
    (numpy's _lerp), all in float32.  nan for no values (a departure the library states: the reference raises IndexError)."""
    s = np.sort(np.asarray(values, dtype=np.float32))
    if len(s) == 0:
        return np.float32(np.nan)
    lo, hi, g = percentile99_neighbours(len(s))
    a, b = s[lo], s[hi]
    with np.errstate(invalid='ignore', over='ignore'):
        diff = np.float32(b - a)
        if g >= 0.5:
            return np.float32(b - diff * np.float32(np.float32(1) - g))
        return np.float32(a + diff * g)


def radius_stats(pts, level=0.1):
    """What the selection kernel returns: per class (floor, not floor) the count and the two order statistics"""
    f = is_floor(pts, level)
    counts, stats = [], []
    for cls in (pts[f], pts[~f]):
        d = np.sort(xz_distances(cls))
        counts.append(len(d))
        if len(d):
            lo, hi, _ = percentile99_neighbours(len(d))
            stats += [d[lo], d[hi]]
        else:
            stats += [np.float32(np.nan), np.float32(np.nan)]
    return np.array(counts, dtype=np.uint64), np.array(stats, dtype=np.float32)


def compute_radius(pts, level=0.1):
    """:202-216 -- (overall, not floor, floor); an empty class gives nan and leaves the overall radius to the other"""
    f = is_floor(pts, level)
    floor_max = percentile99(xz_distances(pts[f]))
    nonfloor_max = percentile99(xz_distances(pts[~f]))
    if not f.any():
        overall = nonfloor_max
    elif f.all():
        overall = floor_max
    else:
        overall = max(floor_max, nonfloor_max)
    return overall, nonfloor_max, floor_max


def tile_counts(pts, nonfloor_only=False, level=0.1):
    if nonfloor_only:
        pts = pts[~is_floor(pts, level)]
    return np.bincount(pts['tile'], minlength=256).astype(np.uint64)


def occupancy_from_counts(counts):
    """:193-200 -- the tiles that occur, ascending (get_tiles_used), with their counts, stably sorted by count, descending"""
    rv = [(t, int(counts[t])) for t in range(256) if counts[t]]
    rv.sort(key=lambda tp: tp[1], reverse=True)
    return rv


def bounds(pts):
    """min x, y, z, max x, y, z with NaN skipped per coordinate (+inf / -inf where there is nothing)"""
    out = np.array([np.inf] * 3 + [-np.inf] * 3, dtype=np.float32)
    for a, f in enumerate('xyz'):
        v = pts[f][~np.isnan(pts[f])]
        if len(v):
            out[a], out[3 + a] = v.min(), v.max()
    return out


class AnalyzeLoop:
    """The per-point loop of the reference's analyze filter (python/cwipc/filters/analyze.py:10-41)."""

    def __init__(self):
        self.count = 0
        self.min_x = self.min_y = self.min_z = 999999
        self.max_x = self.max_y = self.max_z = -999999
        self.sum_avg_x = self.sum_avg_y = self.sum_avg_z = 0

    def filter(self, pts):
        self.count += 1
        lo = {f: 999999 for f in 'xyz'}
        hi = {f: -999999 for f in 'xyz'}
        for p in pts:
            for f in 'xyz':
                v = float(p[f])
                if v < lo[f]: lo[f] = v
                if v > hi[f]: hi[f] = v
        for f in 'xyz':
            if lo[f] < getattr(self, 'min_' + f): setattr(self, 'min_' + f, lo[f])
            if hi[f] > getattr(self, 'max_' + f): setattr(self, 'max_' + f, hi[f])
            setattr(self, 'sum_avg_' + f, getattr(self, 'sum_avg_' + f) + (lo[f] + hi[f]) / 2)

    def state(self):
        return tuple(getattr(self, a + f) for f in 'xyz' for a in ('min_', 'max_', 'sum_avg_'))
