"""numpy model of the point-to-plane ICP contracts (csrc/kernels_icp.hip, csrc/plane_fit.hpp, include/cwipc_util_amd/hip_ext.h): the
terms of a matched pair, the sums, the 6x6 solve with open3d's check_det rule, the motion of its solution, the loop of open3d's
registration_icp.  Built on icp_model (the moved point, the correspondences, the test clouds).  A restatement of the published
algorithm (open3d's TransformationEstimationPointToPlane), not a copy of any implementation: open3d is not needed."""
import math

import numpy as np

import icp_model as im

NSUM = 29
MIN_DET = 1e-6
TRIU = np.triu_indices(6)


def plane_terms(src, ref, normals, T, idx, d2):
    """The terms of the 29 sums, one row per matched source point: J_i J_j for i <= j (21, row-major) | J_i r (6) | r^2 | d2, with
    p the moved source point, q the matched reference point, m its normal (float32 as f64), e = p - q,
    r = (e0*m0 + e1*m1) + e2*m2, J = (p x m, m); every operation rounded on its own."""
    ref = np.asarray(ref, dtype=np.float32).reshape(-1, 3)
    normals = np.asarray(normals, dtype=np.float32).reshape(-1, 3)
    hit = idx != im.NONE
    p = im.move(T, np.asarray(src, dtype=np.float32).reshape(-1, 3)[hit])
    q = ref[idx[hit]].astype(np.float64)
    m = normals[idx[hit]].astype(np.float64)
    e = p - q
    r = (e[:, 0] * m[:, 0] + e[:, 1] * m[:, 1]) + e[:, 2] * m[:, 2]
    c = np.stack([p[:, 1] * m[:, 2] - p[:, 2] * m[:, 1], p[:, 2] * m[:, 0] - p[:, 0] * m[:, 2], p[:, 0] * m[:, 1] - p[:, 1] * m[:, 0]], axis=1)
    J = np.concatenate([c, m], axis=1)
    JJ = J[:, TRIU[0]] * J[:, TRIU[1]]
    return np.concatenate([JJ, J * r[:, None], (r * r)[:, None], d2[hit][:, None]], axis=1)


def plane_sums(terms, exact=False):
    """(n, 29 sums) with numpy.sum, or with math.fsum (exact=True)."""
    n = len(terms)
    if n == 0:
        return 0, np.zeros(NSUM)
    if exact:
        return n, np.array([math.fsum(terms[:, v]) for v in range(NSUM)])
    return n, terms.sum(axis=0)


def system(s):
    """A = sum J J^T (6x6) and b = sum J r from the sums"""
    A = np.zeros((6, 6))
    A[TRIU] = s[:21]
    A = A + np.triu(A, 1).T
    return A, s[21:27]


def solve6(A, b):
    """x with A x = -b, or None where open3d's check_det rule says identity: |det| < 1e-6 or something not finite."""
    if not (np.isfinite(A).all() and np.isfinite(b).all()):
        return None
    det = np.linalg.det(A)
    if not np.isfinite(det) or abs(det) < MIN_DET:
        return None
    x = np.linalg.solve(A, -b)
    return x if np.isfinite(x).all() else None


def motion(x):
    """The 4x4 of x = (alpha, beta, gamma, t): R = Rz(gamma) Ry(beta) Rx(alpha); the identity for None."""
    U = np.eye(4)
    if x is None:
        return U
    sa, ca, sb, cb, sc, cc = math.sin(x[0]), math.cos(x[0]), math.sin(x[1]), math.cos(x[1]), math.sin(x[2]), math.cos(x[2])
    Rx = np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]])
    Ry = np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])
    Rz = np.array([[cc, -sc, 0], [sc, cc, 0], [0, 0, 1]])
    U[:3, :3] = Rz @ Ry @ Rx
    U[:3, 3] = x[3:]
    return U


def icp_plane(src, ref, normals, max_distance, init=None, relative_fitness=1e-6, relative_rmse=1e-6, max_iteration=30, exact=False, tree=False):
    """open3d's registration_icp with the point-to-plane estimate, T applied to the original float32 source every time.
    Returns (T, fitness, rmse, iterations, [T_0, T_1, ...] the matrix of every evaluation,
    [(|fitness change|, |rmse change|), ...] what every stop decision looked at)."""
    src = np.asarray(src, dtype=np.float32).reshape(-1, 3)
    ref = np.asarray(ref, dtype=np.float32).reshape(-1, 3)
    T = np.eye(4) if init is None else np.array(init, dtype=np.float64)
    trail, decisions = [T.copy()], []
    if len(src) == 0 or len(ref) == 0:
        return T, 0.0, 0.0, 0, trail, decisions

    def evaluate(T):
        idx, d2 = im.correspondences(src, ref, T, max_distance, tree=tree)
        n, s = plane_sums(plane_terms(src, ref, normals, T, idx, d2), exact)
        fit = n / len(src) if n else 0.0
        rmse = math.sqrt(s[28] / n) if n else 0.0
        return n, s, fit, rmse

    n, s, fit, rmse = evaluate(T)
    done = 0
    if n:
        for it in range(max_iteration):
            T = motion(solve6(*system(s))) @ T
            trail.append(T.copy())
            before = (fit, rmse)
            n, s, fit, rmse = evaluate(T)
            done = it + 1
            decisions.append((abs(before[0] - fit), abs(before[1] - rmse)))
            if decisions[-1][0] < relative_fitness and decisions[-1][1] < relative_rmse:
                break
    return T, fit, rmse, done, trail, decisions


def estimate_normals(pts, radius, max_nn):
    """A plain f64 estimate for the CPU tests: per point the unit eigenvector (numpy.linalg.eigh) of the smallest eigenvalue of the
    covariance of its max_nn nearest points within radius (itself among them), (0, 0, 1) for fewer than 3.  float32 (n, 3)."""
    from scipy.spatial import cKDTree
    p = np.asarray(pts, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    dist, j = cKDTree(p).query(p, k=min(max_nn, len(p)), distance_upper_bound=radius)
    dist, j = dist.reshape(len(p), -1), j.reshape(len(p), -1)
    out = np.tile(np.float32([0, 0, 1]), (len(p), 1))
    for i in range(len(p)):
        near = p[j[i][np.isfinite(dist[i])]]
        if len(near) >= 3:
            d = near - near.mean(axis=0)
            out[i] = np.linalg.eigh(d.T @ d)[1][:, 0]
    return out, np.isfinite(dist).sum(axis=1)


def test_pair_tiles_plane():
    """icp_model.test_pair_tiles() from another seed (19 instead of 12): two 36 k camera tiles of one synthetic frame, the second
    1 degree and 8 mm out of place.  With seed 12 the point-to-plane loop's last stop decision sees an rmse change of 1.4e-8,
    between 0.1 and 10 times the criterion 1e-7 (tests/test_icp_plane_model.py wants every decision outside that band); 19 is
    the first seed after 12 whose decisions are all outside it.  (ref, src, T_true)"""
    rng = np.random.default_rng(19)
    a, b = im.surface(rng, 72000), im.surface(rng, 72000)
    ref = a[a[:, 0] - 1.2 > -0.1][:36000]
    part = b[b[:, 0] - 1.2 < 0.1][:36000]
    T = im.rigid(1.0, (0.1, 1.0, -0.2), (0.005, 0.004, -0.0048))
    inv = np.linalg.inv(T)
    src = (part.astype(np.float64) @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)
    return ref, src, T


test_pair_tiles_plane.__test__ = False
