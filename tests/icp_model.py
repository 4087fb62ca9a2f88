"""numpy model of the point-to-point ICP contracts (csrc/kernels_icp.hip, csrc/rigid_fit.hpp, include/cwipc_util_amd/hip_ext.h):
the moved point, the brute-force correspondence with its tie rule, the fit sums, umeyama without scaling, the loop of open3d's
registration_icp.  A restatement of the published algorithm, not a copy of any implementation: open3d is not needed."""
import math

import numpy as np

NONE = 0xFFFFFFFF


def move(T, src):
    """px = ((T00*x + T01*y) + T02*z) + T03 in f64 from float32 coordinates, every operation rounded on its own."""
    T = np.asarray(T, dtype=np.float64)
    s = np.asarray(src, dtype=np.float32).astype(np.float64)
    return np.stack([((T[r, 0] * s[:, 0] + T[r, 1] * s[:, 1]) + T[r, 2] * s[:, 2]) + T[r, 3] for r in range(3)], axis=1)


def correspondences(src, ref, T=None, max_distance=np.inf, chunk=256, tree=False):
    """(idx uint32, d2 float64) per source point: brute force over the finite reference points, d2 = (dx*dx + dy*dy) + dz*dz with
    dx = px - (double)qx, only d2 < max_distance^2, the first minimum (= the smallest index); NONE / inf where there is none, also
    for a source point that is not finite before or after T.
    tree=True: the same answer for big clouds -- a KD-tree only names the candidates (see _with_tree)."""
    src = np.asarray(src, dtype=np.float32).reshape(-1, 3)
    ref = np.asarray(ref, dtype=np.float32).reshape(-1, 3)
    p = move(np.eye(4) if T is None else T, src)
    n = len(src)
    idx = np.full(n, NONE, dtype=np.uint32)
    d2 = np.full(n, np.inf, dtype=np.float64)
    ok_ref = np.flatnonzero(np.isfinite(ref).all(axis=1))
    if n == 0 or len(ok_ref) == 0:
        return idx, d2
    q = ref[ok_ref].astype(np.float64)
    ok_src = np.isfinite(src).all(axis=1) & np.isfinite(p).all(axis=1)
    max2 = float(max_distance) * float(max_distance)
    if tree:
        return _with_tree(p, q, ok_src, ok_ref, max_distance, max2, idx, d2)
    for lo in range(0, n, chunk):
        sel = np.flatnonzero(ok_src[lo:lo + chunk]) + lo
        if len(sel) == 0:
            continue
        dx = p[sel, None, 0] - q[None, :, 0]
        dy = p[sel, None, 1] - q[None, :, 1]
        dz = p[sel, None, 2] - q[None, :, 2]
        dd = (dx * dx + dy * dy) + dz * dz
        dd[~(dd < max2)] = np.inf
        j = np.argmin(dd, axis=1)        # the first minimum: ok_ref ascends, so the smallest original index
        best = dd[np.arange(len(sel)), j]
        hit = np.isfinite(best)
        idx[sel[hit]] = ok_ref[j[hit]].astype(np.uint32)
        d2[sel[hit]] = best[hit]
    return idx, d2


def _with_tree(p, q, ok_src, ok_ref, max_distance, max2, idx, d2, k=4):
    """The brute force's answer without its n * m distances.  scipy's cKDTree names, per query, the k nearest reference points by
    ITS f64 distance; every point whose tree distance is within 1e-12 (relative) of the nearest one's is a candidate, and the
    stated d2, the strict bound and the smallest-index rule decide among the candidates.  The brute force's winner is among them:
    its stated d2 is not above the tree's first point's, and the two ways of rounding a distance differ by some 1e-16 of it.  A
    query all of whose k points are candidates (more ties than k) is done by brute force.  test_icp_model.py checks the two
    against each other."""
    from scipy.spatial import cKDTree
    sel = np.flatnonzero(ok_src)
    if len(sel) == 0:
        return idx, d2
    k = min(k, len(q))
    ub = np.inf if np.isinf(max_distance) else float(max_distance) * (1 + 1e-9)
    dist, j = cKDTree(q).query(p[sel], k=k, distance_upper_bound=ub)
    dist, j = dist.reshape(len(sel), k), j.reshape(len(sel), k)
    cand = dist <= dist[:, :1] * (1 + 1e-12)
    cand &= np.isfinite(dist)
    brute = cand.all(axis=1) & (k < len(q))
    jj = np.where(cand, j, 0)
    dx = p[sel, None, 0] - q[jj, 0]
    dy = p[sel, None, 1] - q[jj, 1]
    dz = p[sel, None, 2] - q[jj, 2]
    dd = (dx * dx + dy * dy) + dz * dz
    dd[~cand | ~(dd < max2)] = np.inf
    best = dd.min(axis=1)
    orig = np.where(dd == best[:, None], ok_ref[jj], np.iinfo(np.int64).max).min(axis=1)
    hit = np.isfinite(best) & ~brute
    idx[sel[hit]] = orig[hit].astype(np.uint32)
    d2[sel[hit]] = best[hit]
    for i in sel[brute]:
        dx, dy, dz = p[i, 0] - q[:, 0], p[i, 1] - q[:, 1], p[i, 2] - q[:, 2]
        one = (dx * dx + dy * dy) + dz * dz
        one[~(one < max2)] = np.inf
        m = int(np.argmin(one))
        if np.isfinite(one[m]):
            idx[i], d2[i] = ok_ref[m], one[m]
    return idx, d2


def sum_terms(src, ref, T, idx, d2, cp, cq):
    """The terms of the 16 sums, one row per matched source point: a (3) | b (3) | a_i b_j (9) | d2."""
    ref = np.asarray(ref, dtype=np.float32).reshape(-1, 3)
    m = idx != NONE
    a = move(T, np.asarray(src, dtype=np.float32).reshape(-1, 3)[m]) - np.asarray(cp, dtype=np.float64)
    b = ref[idx[m]].astype(np.float64) - np.asarray(cq, dtype=np.float64)
    ab = (a[:, :, None] * b[:, None, :]).reshape(-1, 9)
    return np.concatenate([a, b, ab, d2[m][:, None]], axis=1)


def sums(terms, exact=False):
    """(n, 16 sums) with numpy.sum, or with math.fsum (exact=True)."""
    n = len(terms)
    if n == 0:
        return 0, np.zeros(16)
    if exact:
        return n, np.array([math.fsum(terms[:, v]) for v in range(16)])
    return n, terms.sum(axis=0)


def umeyama(n, s, cp, cq):
    """Eigen's umeyama without scaling from the sums: R, t with q ~ R p + t."""
    if n == 0:
        return np.eye(3), np.zeros(3)
    sa, sb, sab = s[0:3], s[3:6], s[6:15].reshape(3, 3)
    mu_a, mu_b = sa / n, sb / n
    sigma = (sab.T - np.outer(sb, sa) / n) / n
    U, d, Vt = np.linalg.svd(sigma)
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2, 2] = -1.0
    R = U @ S @ Vt
    t = (np.asarray(cq) + mu_b) - R @ (np.asarray(cp) + mu_a)
    return R, t


def centroid(pts):
    """The pivot: the mean in f64, (0, 0, 0) when it is not finite."""
    pts = np.asarray(pts, dtype=np.float32).reshape(-1, 3)
    c = pts.astype(np.float64).mean(axis=0) if len(pts) else np.zeros(3)
    return c if np.isfinite(c).all() else np.zeros(3)


def icp(src, ref, max_distance, init=None, relative_fitness=1e-6, relative_rmse=1e-6, max_iteration=30, exact=False, tree=False):
    """open3d's registration_icp with the point-to-point estimate, T applied to the original float32 source every time.
    Returns (T, fitness, rmse, iterations, [T_0, T_1, ...] the matrix of every evaluation)."""
    src = np.asarray(src, dtype=np.float32).reshape(-1, 3)
    ref = np.asarray(ref, dtype=np.float32).reshape(-1, 3)
    T = np.eye(4) if init is None else np.array(init, dtype=np.float64)
    trail = [T.copy()]
    if len(src) == 0 or len(ref) == 0:
        return T, 0.0, 0.0, 0, trail
    cp0, cq = centroid(src), centroid(ref)

    def evaluate(T):
        cp = ((T[:3, 0] * cp0[0] + T[:3, 1] * cp0[1]) + T[:3, 2] * cp0[2]) + T[:3, 3]   # the pivot follows the cloud
        idx, d2 = correspondences(src, ref, T, max_distance, tree=tree)
        n, s = sums(sum_terms(src, ref, T, idx, d2, cp, cq), exact)
        fit = n / len(src) if n else 0.0
        rmse = math.sqrt(s[15] / n) if n else 0.0
        return n, s, cp, fit, rmse

    n, s, cp, fit, rmse = evaluate(T)
    done = 0
    if n:
        for it in range(max_iteration):
            R, t = umeyama(n, s, cp, cq)
            U = np.eye(4)
            U[:3, :3] = R
            U[:3, 3] = t
            T = U @ T
            trail.append(T.copy())
            before = (fit, rmse)
            n, s, cp, fit, rmse = evaluate(T)
            done = it + 1
            if abs(before[0] - fit) < relative_fitness and abs(before[1] - rmse) < relative_rmse:
                break
    return T, fit, rmse, done, trail


# ---- the test clouds, shared by the CPU and the GPU tests ----
def rigid(deg, axis, t):
    axis = np.asarray(axis, dtype=np.float64)
    axis = axis / np.linalg.norm(axis)
    a = math.radians(deg)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + math.sin(a) * K + (1 - math.cos(a)) * (K @ K)
    T[:3, 3] = t
    return T


def surface(rng, n):
    """A bumpy, closed surface about 1 m across and 1.7 m high, a metre or two from the origin: float32 (n, 3)."""
    u = rng.uniform(0, 2 * np.pi, n)
    v = rng.uniform(0, 1, n)
    r = 0.3 + 0.08 * np.sin(3 * u) * np.cos(5 * v) + 0.05 * np.cos(7 * v + u)
    pts = np.stack([r * np.cos(u) + 1.2, 1.7 * v + 0.04 * np.sin(4 * u), r * np.sin(u) - 0.8], axis=1)
    return pts.astype(np.float32)


def moved_copy(rng, ref, T):
    """A permuted copy of ref under the inverse of T, rounded to float32: T maps it back onto ref up to that rounding."""
    inv = np.linalg.inv(T)
    p = ref[rng.permutation(len(ref))].astype(np.float64)
    return (p @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)


def test_pair_5k():
    """A 5 k cloud and its moved copy: 2 degrees, 1 cm.  (ref, src, T_true)"""
    rng = np.random.default_rng(11)
    ref = surface(rng, 5000)
    T = rigid(2.0, (0.3, 1.0, 0.2), (0.006, -0.005, 0.0062))
    return ref, moved_copy(rng, ref, T), T


def test_pair_tiles():
    """Two 36 k camera tiles of one synthetic frame: the halves x' > -0.1 and x' < 0.1 (x' across the figure) of one surface
    sampled twice, the second a little out of place (1 degree, 8 mm)."""
    rng = np.random.default_rng(12)
    a, b = surface(rng, 72000), surface(rng, 72000)
    ref = a[a[:, 0] - 1.2 > -0.1][:36000]
    part = b[b[:, 0] - 1.2 < 0.1][:36000]
    T = rigid(1.0, (0.1, 1.0, -0.2), (0.005, 0.004, -0.0048))
    inv = np.linalg.inv(T)
    src = (part.astype(np.float64) @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)
    return ref, src, T


test_pair_5k.__test__ = False
test_pair_tiles.__test__ = False
