"""numpy and scipy model of RULE N (include/cwipc_util_amd/hip_ext.h): fixed-radius neighbour counts, the radius outlier filter and
first-order moving-least-squares smoothing, written from the rule's text.

Candidates come from scipy.spatial.cKDTree.query_pairs at a slightly larger radius (the tree's own arithmetic decides nothing); the
rule's float64 d2 < r2 and the tile test cut them.  The smoothing's ten sums are int64 (np.add.at: exact), the normal comes from
numpy.linalg.eigh -- NOT the Jacobi solver of csrc/smallest_eigvec.hpp, so a smoothed coordinate may differ from the library's by one
float32 step where the f64 results straddle a rounding boundary (tests/test_smooth_host.py has the argument).  brute_force_* are the
O(n^2) restatements, with Python integers, that the model is checked against (tests/test_neigh_model.py)."""
import numpy as np
from scipy.spatial import cKDTree

MAX_CNT = 262144
GAP_MIN = 1e-2     # relative eigengap (w1 - w0) / w2 below which the two solvers' normals are not compared


def _xyz(xyz):
    return np.asarray(xyz, dtype=np.float32).reshape(-1, 3)


def xyz_of(pts):
    return np.stack([pts["x"], pts["y"], pts["z"]], axis=1)


def _offsets(a, b):
    """d = (double)b - (double)a and d2 = (dx*dx + dy*dy) + dz*dz, every operation rounded on its own; a, b: float32 (m, 3)"""
    d = b.astype(np.float64) - a.astype(np.float64)
    return d, (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def pairs_within(xyz, radius, tiles=None):
    """The unordered pairs (i, j), i != j, with j in N(i): int64 (m, 2), each pair once; and the finite points' indices."""
    xyz = _xyz(xyz)
    with np.errstate(over="ignore", under="ignore"):
        r2 = np.float64(radius) * np.float64(radius)
    finite = np.flatnonzero(np.isfinite(xyz).all(axis=1))
    none = np.zeros((0, 2), dtype=np.int64)
    if len(finite) == 0 or not r2 > 0:
        return none, finite[:0]
    pts = xyz[finite]
    reach = float(radius) * (1.0 + 1e-6) + 1e-30
    if not np.isfinite(reach):
        reach = np.finfo(np.float64).max
    with np.errstate(over="ignore", invalid="ignore"):
        pairs = cKDTree(pts.astype(np.float64)).query_pairs(reach, output_type="ndarray").astype(np.int64).reshape(-1, 2)
        if len(pairs):
            pairs = pairs[_offsets(pts[pairs[:, 0]], pts[pairs[:, 1]])[1] < r2]
    pairs = finite[pairs]
    if tiles is not None and len(pairs):
        tiles = np.asarray(tiles)
        pairs = pairs[tiles[pairs[:, 0]] == tiles[pairs[:, 1]]]
    return pairs, finite


def directed_pairs(xyz, radius, tiles=None):
    """All (i, j) with j in N(i), i itself included when r2 > 0: int64 (m, 2), sorted by i then j."""
    pairs, finite = pairs_within(xyz, radius, tiles)
    own = np.stack([finite, finite], axis=1)
    both = np.concatenate([pairs, pairs[:, ::-1], own])
    return both[np.lexsort((both[:, 1], both[:, 0]))]


def counts(xyz, radius, tiles=None):
    """count[i] = |N(i)| - 1 for a finite point, 0 for a non-finite one; uint32"""
    xyz = _xyz(xyz)
    pairs, _ = pairs_within(xyz, radius, tiles)
    return np.bincount(pairs.ravel(), minlength=len(xyz)).astype(np.uint32)


def keep_mask(xyz, cnt, min_neighbours=1):
    """the radius outlier filter's keep mask from the counts"""
    return np.isfinite(_xyz(xyz)).all(axis=1) & (cnt.astype(np.int64) >= int(min_neighbours))


def radius_outlier_filter(points, radius, min_neighbours=1, same_tile=False):
    """points: the structured cwipc point array; -> the kept points, in input order"""
    xyz = xyz_of(points)
    return points[keep_mask(xyz, counts(xyz, radius, points["tile"] if same_tile else None), min_neighbours)]


def moves(cnt, min_neighbours):
    """the move decision of a finite point with cnt = |N(i)|"""
    return cnt - 1 >= max(2, int(min_neighbours)) and cnt <= MAX_CNT


def sums(xyz, radius, tiles=None):
    """(W (n,), S1 (n, 3), S2 (n, 6: xx xy xz yy yz zz), cnt (n,)) int64, by RULE N's Smoothing"""
    xyz = _xyz(xyz)
    n = len(xyz)
    r2 = np.float64(radius) * np.float64(radius)
    s = np.float64(65536.0) / np.float64(radius)
    pairs = directed_pairs(xyz, radius, tiles)
    i = pairs[:, 0]
    d, d2 = _offsets(xyz[i], xyz[pairs[:, 1]])
    o = np.rint(d * s).astype(np.int64)
    t = 1.0 - d2 / r2
    w = np.rint(4096.0 * (t * t)).astype(np.int64)
    W, S1, S2 = np.zeros(n, np.int64), np.zeros((n, 3), np.int64), np.zeros((n, 6), np.int64)
    np.add.at(W, i, w)
    np.add.at(S1, i, w[:, None] * o)
    for k, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        np.add.at(S2[:, k], i, w * o[:, a] * o[:, b])
    return W, S1, S2, np.bincount(i, minlength=n).astype(np.int64)


def _matrices(W, S1, S2):
    Wf, S1f, S2f = W.astype(np.float64), S1.astype(np.float64), S2.astype(np.float64)
    M = np.zeros((len(W), 3, 3))
    for k, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        M[:, a, b] = M[:, b, a] = Wf * S2f[:, k] - S1f[:, a] * S1f[:, b]
    return M


def displace(xyz, radius, W, S1, S2, moved):
    """The moved points' new coordinates from the sums, the normal by eigh -> (out float32 (n, 3), gap (n,): the relative eigengap
    (w1 - w0) / w2 of a moved point's matrix, inf for the others)"""
    xyz = _xyz(xyz)
    out, gap = xyz.copy(), np.full(len(xyz), np.inf)
    m = np.flatnonzero(moved)
    if len(m) == 0:
        return out, gap
    s = np.float64(65536.0) / np.float64(radius)
    ev, vec = np.linalg.eigh(_matrices(W[m], S1[m], S2[m]))
    nrm = vec[:, :, 0]
    with np.errstate(invalid="ignore", divide="ignore"):
        g = (ev[:, 1] - ev[:, 0]) / ev[:, 2]
    gap[m] = np.where(np.isfinite(g), g, 0.0)
    c = S1[m].astype(np.float64) / W[m].astype(np.float64)[:, None]
    h = (nrm[:, 0] * c[:, 0] + nrm[:, 1] * c[:, 1]) + nrm[:, 2] * c[:, 2]
    out[m] = (xyz[m].astype(np.float64) + (nrm * h[:, None]) / s).astype(np.float32)
    return out, gap


def smooth_xyz(xyz, radius, min_neighbours=2, tiles=None):
    """-> (out float32 (n, 3), moved bool (n,), gap (n,), cnt int64 (n,))"""
    xyz = _xyz(xyz)
    W, S1, S2, cnt = sums(xyz, radius, tiles)
    moved = np.isfinite(xyz).all(axis=1) & (cnt - 1 >= max(2, int(min_neighbours))) & (cnt <= MAX_CNT)
    out, gap = displace(xyz, radius, W, S1, S2, moved)
    return out, moved, gap, cnt


def smooth(points, radius, min_neighbours=2, same_tile=False):
    """points: the structured cwipc point array -> (the smoothed points, moved, gap)"""
    out, moved, gap, _ = smooth_xyz(xyz_of(points), radius, min_neighbours, points["tile"] if same_tile else None)
    res = points.copy()
    for a, name in enumerate("xyz"):
        res[name][moved] = out[moved, a]
    return res, moved, gap


def ulp_steps(a, b):
    """how many float32 values lie between a and b (0: equal, 1: adjacent); -0.0 and +0.0 count as one value"""
    def key(v):
        u = np.ascontiguousarray(v, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(u < 0, -(u & 0x7FFFFFFF), u)
    return np.abs(key(a) - key(b))


# ---------------------------------------------------------------------------
# the smoothing tests' inputs (tests/test_smooth_host.py on the host twin, tests/test_gpu_neigh.py on the device)
# ---------------------------------------------------------------------------
POINT_DTYPE = [('x', '<f4'), ('y', '<f4'), ('z', '<f4'), ('r', 'u1'), ('g', 'u1'), ('b', 'u1'), ('tile', 'u1')]


def as_points(xyz, tile=1, seed=0):
    """the structured cwipc point array of xyz with random colours"""
    xyz = _xyz(xyz)
    pts = np.zeros(len(xyz), dtype=POINT_DTYPE)
    if len(xyz):
        pts["x"], pts["y"], pts["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
        rng = np.random.default_rng(seed)
        pts["r"], pts["g"], pts["b"] = rng.integers(0, 256, (3, len(xyz)), dtype=np.uint8)
        pts["tile"] = tile
    return pts


PLANE_NORMAL = np.array([0.36, 0.48, 0.8])          # unit length
PLANE_ORIGIN = np.array([0.1, -0.2, 1.5])


def noisy_plane():
    """64 x 64 points, 0.005 apart, on the plane through PLANE_ORIGIN with PLANE_NORMAL, each moved along the normal by N(0, 0.0015)
    and in the plane by up to a fifth of a step; shuffled.  r = 0.016: about 31 neighbours."""
    rng = np.random.default_rng(64)
    e1 = np.cross(PLANE_NORMAL, [0.0, 0.0, 1.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(PLANE_NORMAL, e1)
    u, v = np.meshgrid(np.arange(64), np.arange(64), indexing="ij")
    uv = np.stack([u.ravel(), v.ravel()], axis=1) + rng.uniform(-0.2, 0.2, (4096, 2))
    xyz = PLANE_ORIGIN + 0.005 * (uv[:, :1] * e1 + uv[:, 1:] * e2) + rng.normal(0, 0.0015, (4096, 1)) * PLANE_NORMAL
    return as_points(xyz[rng.permutation(4096)], tile=rng.choice(np.uint8([1, 2, 4, 8]), 4096), seed=1), 0.016


def plane_rms(xyz):
    """rms distance of the points to the true plane of noisy_plane, in float64"""
    d = (np.asarray(xyz, dtype=np.float64) - PLANE_ORIGIN) @ PLANE_NORMAL
    return float(np.sqrt(np.mean(d * d)))


def noisy_sphere():
    """6000 points on the sphere of radius 0.48 around (0, 1, 0), each moved along its radius by N(0, 0.003).  r = 0.06: about 23
    neighbours."""
    rng = np.random.default_rng(6000)
    d = rng.normal(size=(6000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    xyz = np.array([0.0, 1.0, 0.0]) + d * (0.48 + rng.normal(0, 0.003, (6000, 1)))
    return as_points(xyz, tile=rng.choice(np.uint8([1, 2]), 6000), seed=2), 0.06


def gaussian_blob():
    """4000 points of N(0, 0.05) around (-1, 0.5, 2): no surface at all, neighbourhoods from one point to a few hundred.  r = 0.03."""
    rng = np.random.default_rng(4000)
    return as_points(np.array([-1.0, 0.5, 2.0]) + rng.normal(0, 0.05, (4000, 3)), tile=7, seed=3), 0.03


# name: (constructor, the cap on the share of moved points whose eigengap is below GAP_MIN -- measured with this model alone: 0, 0 and
# 0.5 % -- ; tests/test_neigh_model.py re-checks it)
SMOOTH_INPUTS = {"noisy plane": (noisy_plane, 0.01), "noisy sphere": (noisy_sphere, 0.01), "gaussian blob": (gaussian_blob, 0.05)}


def check_against_model(name, pts, got, radius, min_neighbours=2, same_tile=False, cap=None):
    """What every smoothed cloud `got` of `pts` must satisfy, with the eigh model as the yardstick: for every point, no exclusions --
    colours and tiles unchanged, an unmoved point's bytes unchanged, a moved point less than radius from where it was; where the
    eigengap is at least GAP_MIN each coordinate equal or adjacent to the model's float32; the share of moved points left out of
    that comparison at most `cap`.  Returns (moved, compared, the number of coordinates that are adjacent rather than equal)."""
    want, moved, gap = smooth(pts, radius, min_neighbours, same_tile)
    assert got.dtype == pts.dtype and len(got) == len(pts), name
    for f in ("r", "g", "b", "tile"):
        assert np.array_equal(got[f], pts[f]), (name, f)
    assert got[~moved].tobytes() == pts[~moved].tobytes(), name
    step = xyz_of(got)[moved].astype(np.float64) - xyz_of(pts)[moved].astype(np.float64)
    assert np.all(np.sqrt((step ** 2).sum(axis=1)) < radius), name
    ok = moved & (gap >= GAP_MIN)
    steps = ulp_steps(xyz_of(got)[ok], xyz_of(want)[ok])
    print("%s: %d points, %d moved, %d compared with eigh (gap >= %g), %d coordinates adjacent, none further" % (
        name, len(pts), moved.sum(), ok.sum(), GAP_MIN, int((steps == 1).sum())))
    assert steps.max(initial=0) <= 1, (name, int(steps.max()), int((steps > 1).sum()))
    if cap is not None:
        assert moved.sum() > 0 and (moved & ~ok).sum() <= cap * moved.sum(), (name, int((moved & ~ok).sum()), int(moved.sum()))
    return moved, ok, int((steps == 1).sum())


# ---------------------------------------------------------------------------
# O(n^2) restatements with Python integers
# ---------------------------------------------------------------------------
def brute_force_neighbours(xyz, radius, tiles=None):
    """[N(i) as a sorted list of indices] over every pair"""
    xyz = _xyz(xyz)
    n = len(xyz)
    r2 = np.float64(radius) * np.float64(radius)
    finite = np.isfinite(xyz).all(axis=1)
    res = []
    for i in range(n):
        if not finite[i]:
            res.append([])
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            _, d2 = _offsets(np.broadcast_to(xyz[i], (n, 3)), xyz)
        near = finite & (d2 < r2)
        if tiles is not None:
            near &= np.asarray(tiles) == tiles[i]
        res.append(np.flatnonzero(near).tolist())
    return res


def brute_force_sums(xyz, radius, tiles=None):
    """the ten sums and cnt per point as Python integers: [(W, [S1], [S2], cnt)]"""
    xyz = _xyz(xyz)
    r2 = float(np.float64(radius) * np.float64(radius))
    s = 65536.0 / float(radius)
    res = []
    for i, near in enumerate(brute_force_neighbours(xyz, radius, tiles)):
        W, S1, S2 = 0, [0, 0, 0], [0] * 6
        for j in near:
            d = [float(xyz[j, a]) - float(xyz[i, a]) for a in range(3)]
            d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
            o = [int(np.rint(d[a] * s)) for a in range(3)]
            t = 1.0 - d2 / r2
            w = int(np.rint(4096.0 * (t * t)))
            W += w
            for a in range(3):
                S1[a] += w * o[a]
            for k, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
                S2[k] += w * o[a] * o[b]
        res.append((W, S1, S2, len(near)))
    return res
