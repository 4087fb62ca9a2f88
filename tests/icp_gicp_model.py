"""numpy model of the generalized ICP contracts (csrc/gicp_terms.hpp, csrc/kernels_icp.hip, include/cwipc_util_amd/hip_ext.h): the
orientation of the normals, the covariance of a point from its normal, the terms of a matched pair in the N = M^-1 form, the sums,
the loop of open3d's registration_generalized_icp.  Built on icp_model (the moved point, the correspondences, the test clouds) and
icp_plane_model (the 6x6 solve, the motion).  A restatement of the published algorithm (open3d's
TransformationEstimationForGeneralizedICP, epsilon 1e-3, L2 loss), not a copy of any implementation: open3d is not needed.

Every operation is rounded on its own, in f64, in the order written here: csrc/gicp_terms.hpp states the same order, and
tests/test_gicp_terms_host.py holds the two to each other bit for bit.  The published form with W = (M^-1)^(1/2) is here too
(pair_system_w), for tests/test_icp_gicp_model.py to compare the N form with."""
import math

import numpy as np

import icp_model as im
import icp_plane_model as pm

NSUM = 29
EPSILON = 1e-3
TRIU3 = np.triu_indices(3)
TRIU6 = np.triu_indices(6)


def mean(pts):
    """A cloud's mean in f64 (not finite where a coordinate is not); zeros for no points."""
    pts = np.asarray(pts, dtype=np.float32).reshape(-1, 3)
    return pts.astype(np.float64).mean(axis=0) if len(pts) else np.zeros(3)


def directions(src, ref):
    """(the source's direction, the reference's): cs - o and ct - o with o = (cs + ct) / 2, the reference's _fix_normal_direction."""
    cs, ct = mean(src), mean(ref)
    o = (cs + ct) / 2
    return cs - o, ct - o


def orient(normals, direction):
    """open3d's OrientNormalsToAlignWithDirection on float32 normals as f64: a zero normal becomes the direction, a normal with
    (m0*d0 + m1*d1) + m2*d2 < 0 is negated (false for NaN).  direction None: the normals as they are.  f64 (n, 3)."""
    m = np.asarray(normals, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    if direction is None:
        return m
    d = np.asarray(direction, dtype=np.float64)
    zero = (m == 0).all(axis=1)
    with np.errstate(invalid="ignore"):
        flip = ~zero & ((m[:, 0] * d[0] + m[:, 1] * d[1]) + m[:, 2] * d[2] < 0)
    m[flip] = -m[flip]
    m[zero] = d
    return m


def covariances(normals, direction=None, eps=EPSILON):
    """Per normal, oriented first, open3d's GetRotationFromE1ToX and C = Rx diag(eps, 1, 1) Rx^T: six values 00, 01, 02, 11, 12,
    22.  Rx = I where m0 < -0.99 (open3d's rule).  f64 (n, 6)."""
    m = orient(normals, direction)
    n = len(m)
    m1, m2 = m[:, 1], m[:, 2]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        f = 1.0 / (1.0 + m[:, 0])
        Rx = np.empty((n, 3, 3))
        Rx[:, 0, 0] = 1.0 - f * (m1 * m1 + m2 * m2)
        Rx[:, 0, 1] = -m1
        Rx[:, 0, 2] = -m2
        Rx[:, 1, 0] = m1
        Rx[:, 1, 1] = 1.0 - f * (m1 * m1)
        Rx[:, 1, 2] = -(f * (m1 * m2))
        Rx[:, 2, 0] = m2
        Rx[:, 2, 1] = -(f * (m1 * m2))
        Rx[:, 2, 2] = 1.0 - f * (m2 * m2)
        Rx[m[:, 0] < -0.99] = np.eye(3)
        return np.stack([((eps * Rx[:, i, 0]) * Rx[:, j, 0] + Rx[:, i, 1] * Rx[:, j, 1]) + Rx[:, i, 2] * Rx[:, j, 2] for i, j in zip(*TRIU3)], axis=1)


def full3(C6):
    """(n, 6) upper triangles -> (n, 3, 3) symmetric"""
    C = np.empty((len(C6), 3, 3))
    for v, (i, j) in enumerate(zip(*TRIU3)):
        C[:, i, j] = C[:, j, i] = C6[:, v]
    return C


def pair_m(Cs, Ct, R):
    """M = Ct + (R Cs) R^T per pair, as its six values"""
    cs = full3(Cs)
    R = np.asarray(R, dtype=np.float64)
    B = np.empty((len(Cs), 3, 3))
    for i in range(3):
        for j in range(3):
            B[:, i, j] = (R[i, 0] * cs[:, 0, j] + R[i, 1] * cs[:, 1, j]) + R[i, 2] * cs[:, 2, j]
    return np.stack([Ct[:, v] + ((B[:, i, 0] * R[j, 0] + B[:, i, 1] * R[j, 1]) + B[:, i, 2] * R[j, 2]) for v, (i, j) in enumerate(zip(*TRIU3))], axis=1)


def pair_a(p):
    """A = [-skew(p) | I], (n, 3, 6)"""
    A = np.zeros((len(p), 3, 6))
    A[:, 0, 1], A[:, 0, 2] = p[:, 2], -p[:, 1]
    A[:, 1, 0], A[:, 1, 2] = -p[:, 2], p[:, 0]
    A[:, 2, 0], A[:, 2, 1] = p[:, 1], -p[:, 0]
    A[:, 0, 3] = A[:, 1, 4] = A[:, 2, 5] = 1.0
    return A


def pair_terms(p, q, Cs, Ct, R, d2):
    """The 29 terms per pair, the N form: (A^T N A)_ij for i <= j (21) | (A^T g)_i (6) | e^T g | d2, with N = M^-1 by cofactors,
    e = p - q, g = N e, H = N A first and A^T H after it."""
    M = pair_m(Cs, Ct, R)
    M00, M01, M02, M11, M12, M22 = (M[:, v] for v in range(6))
    k00, k01, k02 = M11 * M22 - M12 * M12, M02 * M12 - M01 * M22, M01 * M12 - M02 * M11
    k11, k12, k22 = M00 * M22 - M02 * M02, M01 * M02 - M00 * M12, M00 * M11 - M01 * M01
    det = (M00 * k00 + M01 * k01) + M02 * k02
    N = full3(np.stack([k00 / det, k01 / det, k02 / det, k11 / det, k12 / det, k22 / det], axis=1))
    e = p - q
    g = np.stack([(N[:, i, 0] * e[:, 0] + N[:, i, 1] * e[:, 1]) + N[:, i, 2] * e[:, 2] for i in range(3)], axis=1)
    A = pair_a(p)
    H = np.empty((len(p), 3, 6))
    for i in range(3):
        for j in range(6):
            H[:, i, j] = (N[:, i, 0] * A[:, 0, j] + N[:, i, 1] * A[:, 1, j]) + N[:, i, 2] * A[:, 2, j]
    AHA = [(A[:, 0, i] * H[:, 0, j] + A[:, 1, i] * H[:, 1, j]) + A[:, 2, i] * H[:, 2, j] for i, j in zip(*TRIU6)]
    Ag = [(A[:, 0, i] * g[:, 0] + A[:, 1, i] * g[:, 1]) + A[:, 2, i] * g[:, 2] for i in range(6)]
    eg = (e[:, 0] * g[:, 0] + e[:, 1] * g[:, 1]) + e[:, 2] * g[:, 2]
    return np.stack(AHA + Ag + [eg, np.asarray(d2, dtype=np.float64)], axis=1)


def pair_system_w(p, q, Cs, Ct, R):
    """The published form, per pair: W = (M^-1)^(1/2) = V diag(lambda^-1/2) V^T from numpy.linalg.eigh of M, J = W A, r = W e.
    (J^T J (n, 6, 6), J^T r (n, 6), r^T r (n,))"""
    lam, V = np.linalg.eigh(full3(pair_m(Cs, Ct, R)))
    W = (V * (lam ** -0.5)[:, None, :]) @ np.swapaxes(V, 1, 2)
    J = W @ pair_a(p)
    r = (W @ (p - q)[:, :, None])[:, :, 0]
    return np.swapaxes(J, 1, 2) @ J, (np.swapaxes(J, 1, 2) @ r[:, :, None])[:, :, 0], (r * r).sum(axis=1)


def gicp_terms(src, ref, cov_src, cov_ref, T, idx, d2):
    """pair_terms over the matched source points: p the moved source point, q its correspondence (float32 as f64), Cs the source
    point's covariance, Ct the correspondence's, R the 3x3 block of T."""
    ref = np.asarray(ref, dtype=np.float32).reshape(-1, 3)
    T = np.asarray(T, dtype=np.float64)
    hit = idx != im.NONE
    p = im.move(T, np.asarray(src, dtype=np.float32).reshape(-1, 3)[hit])
    q = ref[idx[hit]].astype(np.float64)
    return pair_terms(p, q, cov_src[hit], cov_ref[idx[hit]], T[:3, :3], d2[hit])


def gicp_sums(terms, exact=False):
    """(n, 29 sums) with numpy.sum, or with math.fsum (exact=True): the plane sums' layout."""
    return pm.plane_sums(terms, exact)


def cloud_covariances(src, ref, normals_src, normals_ref, eps=EPSILON):
    """Both clouds' covariances as the sums and the loop see them: each cloud's normals turned to its own direction."""
    ds, dt = directions(src, ref)
    return covariances(normals_src, ds, eps), covariances(normals_ref, dt, eps)


def icp_generalized(src, ref, normals_src, normals_ref, max_distance, init=None, relative_fitness=1e-6, relative_rmse=1e-6, max_iteration=30,
                    eps=EPSILON, exact=False, tree=False):
    """open3d's registration_generalized_icp: icp_plane_model.icp_plane's loop with the generalized sums; the covariances once per
    run, from the original clouds; T and its rotation applied to the original source points and covariances every time.
    Returns (T, fitness, rmse, iterations, [T_0, T_1, ...] the matrix of every evaluation,
    [(|fitness change|, |rmse change|), ...] what every stop decision looked at)."""
    src = np.asarray(src, dtype=np.float32).reshape(-1, 3)
    ref = np.asarray(ref, dtype=np.float32).reshape(-1, 3)
    T = np.eye(4) if init is None else np.array(init, dtype=np.float64)
    trail, decisions = [T.copy()], []
    if len(src) == 0 or len(ref) == 0:
        return T, 0.0, 0.0, 0, trail, decisions
    cov_src, cov_ref = cloud_covariances(src, ref, normals_src, normals_ref, eps)

    def evaluate(T):
        idx, d2 = im.correspondences(src, ref, T, max_distance, tree=tree)
        n, s = gicp_sums(gicp_terms(src, ref, cov_src, cov_ref, T, idx, d2), exact)
        fit = n / len(src) if n else 0.0
        rmse = math.sqrt(s[28] / n) if n else 0.0
        return n, s, fit, rmse

    n, s, fit, rmse = evaluate(T)
    done = 0
    if n:
        for it in range(max_iteration):
            T = pm.motion(pm.solve6(*pm.system(s))) @ T
            trail.append(T.copy())
            before = (fit, rmse)
            n, s, fit, rmse = evaluate(T)
            done = it + 1
            decisions.append((abs(before[0] - fit), abs(before[1] - rmse)))
            if decisions[-1][0] < relative_fitness and decisions[-1][1] < relative_rmse:
                break
    return T, fit, rmse, done, trail, decisions


def test_pair_5k_gicp():
    """icp_model.test_pair_5k() from another seed (26 instead of 11): a 5 k cloud and its moved copy, 2 degrees and 1 cm.  Generalized
    ICP converges faster than point-to-plane, and on this construction its third rmse change is about 2e-7 whatever the seed (2.6e-8
    to 2.8e-7 on the seeds 11 to 25, 2.2e-7 on 11): between 0.1 and 10 times the criterion 1e-7, where
    tests/test_icp_gicp_model.py wants no stop decision.  26 is the first seed after 11 whose decisions are all outside that band.
    (ref, src, T_true)"""
    rng = np.random.default_rng(26)
    ref = im.surface(rng, 5000)
    T = im.rigid(2.0, (0.3, 1.0, 0.2), (0.006, -0.005, 0.0062))
    return ref, im.moved_copy(rng, ref, T), T


def test_pair_tiles_gicp():
    """icp_plane_model.test_pair_tiles_plane() from another seed (64 instead of 19): two 36 k camera tiles of one synthetic frame,
    the second 1 degree and 8 mm out of place.  With seed 19 the third stop decision sees an rmse change of 2.2e-7, inside the band
    (see test_pair_5k_gicp), and so it is with every seed from 20 to 63 (1.3e-7 to 3.9e-7, or a last change between 1e-8 and
    2.7e-8).  64 is the first whose decisions are all outside it.  (ref, src, T_true)"""
    rng = np.random.default_rng(64)
    a, b = im.surface(rng, 72000), im.surface(rng, 72000)
    ref = a[a[:, 0] - 1.2 > -0.1][:36000]
    part = b[b[:, 0] - 1.2 < 0.1][:36000]
    T = im.rigid(1.0, (0.1, 1.0, -0.2), (0.005, 0.004, -0.0048))
    inv = np.linalg.inv(T)
    src = (part.astype(np.float64) @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)
    return ref, src, T


test_pair_5k_gicp.__test__ = False
test_pair_tiles_gicp.__test__ = False
