"""Generalized ICP on the GPU (kernels_icp.hip: gicp_covariance_kernel, icp_sums_partial_kernel<GicpPair>, icp_generalized;
gicp_terms.hpp; registration/fine.py) against the numpy model of its contracts (tests/icp_gicp_model.py, checked on the CPU by
tests/test_icp_gicp_model.py and, bit for bit against the header, by tests/test_gicp_terms_host.py).  open3d is not available: the
model restates the published algorithm, nothing here is compared with open3d's output.  Unless a test says otherwise the model's
normals are the library's own, downloaded with cwipc_hip_estimate_normals (tests/test_gpu_direction.py checks those), and the
library is called without normals, so it estimates the same ones on the device.

Bars:
  * covariances: numpy.array_equal with the model (IEEE f64 with one stated order on both sides);
  * one matched pair: n == 1 and the 29 sums array_equal with the model's one term -- adding zeros is exact, so this holds the
    device's term arithmetic, division included, to the model bit for bit;
  * sums on lattice clouds (coordinates multiples of 1/64 within +-2, axis normals on both clouds, epsilon 1: every Rx is a signed
    permutation, every covariance the identity, M = 2 I, N = I / 2 and every term and sum exact in f64): n and all 29 sums
    array_equal with the model;
  * sums on jittered clouds: n exact, each sum within (n + 3) * 2^-53 * sum |term| of math.fsum over the model's terms -- the worst
    case of any summation order plus the terms' own roundings: derived, not measured (as tests/test_gpu_icp.py);
  * repeated calls, estimated against passed normals, threads, negated caller's normals: the same bytes;
  * the loop: at each of the model's iterates the library's sums are within the bound above; the library's own loop ends after the
    model's number of iterations with T, fitness and rmse within 100 x GICP_CPU_SPREAD (tests/test_icp_gicp_model.py) of the
    model's -- the factor of tests/test_gpu_icp.py; the 5 k pair ends within ten times the CPU-measured error of the motion it was
    made with.

The model's directions come from numpy's mean of each cloud, the library's from its own f64 mean: the two differ in the last
places, and only the sign of a normal's product with the direction is used -- except for a zero normal, which no test here feeds
to the sums entries (the covariance entry takes the direction from the caller)."""
import threading

import numpy as np
import pytest

import icp_model as im
import icp_gicp_model as gm
from test_gpu_icp import as_points, cloud, SMALL_T, FAR_T, TRANSFORMS
from test_gpu_icp_plane import lattice_points, LATTICE_T
from test_icp_gicp_model import GICP_CPU_SPREAD, GICP_MOTION_ERROR_MEASURED, CRITERIA, MAXD, PAIRS
from test_gicp_terms_host import BAND, unit_normals

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
EPS = 1e-3
AXES = np.float32([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]])
QUARTER_Y = np.array([[0.0, 0, 1, 1 / 64], [0, 1, 0, -3 / 64], [-1, 0, 0, 2 / 64], [0, 0, 0, 1]])


def sums_within_bound(got_n, got, terms, label):
    n, want = gm.gicp_sums(terms, exact=True)
    assert got_n == n, (label, got_n, n)
    bound = (n + 3) * U * np.abs(terms).sum(axis=0) if n else np.zeros(gm.NSUM)
    err = np.abs(got - want)
    print("%s: n %d, largest error over bound %.3f" % (label, n, float(np.max(err / np.maximum(bound, 1e-300))) if n else 0.0))
    assert np.all(err <= bound), (label, err, bound)


def model_terms(src_xyz, ref_xyz, normals_src, normals_ref, T, maxd, eps=EPS, tree=False):
    T = np.eye(4) if T is None else T
    cov_src, cov_ref = gm.cloud_covariances(src_xyz, ref_xyz, normals_src, normals_ref, eps)
    idx, d2 = im.correspondences(src_xyz, ref_xyz, T, maxd, tree=tree)
    return gm.gicp_terms(src_xyz, ref_xyz, cov_src, cov_ref, T, idx, d2)


@pytest.fixture(scope="module")
def pairs(gpu):
    """The loop's two pairs, the library's normals of both clouds and the model's run with them (numpy sums), computed once."""
    out = {}
    for name, (make, tree, radius, max_nn) in PAIRS.items():
        ref, src, T_true = make()
        normals = []
        for xyz in (src, ref):
            pc = cloud(gpu, xyz)
            normals.append(gpu.cwipc_hip_estimate_normals(pc, radius, max_nn)[0])
            pc.free()
        run = gm.icp_generalized(src, ref, normals[0], normals[1], MAXD, None, *CRITERIA, tree=tree)
        out[name] = (ref, src, T_true, tree, radius, max_nn, normals[0], normals[1], run)
    return out


# ---------------------------------------------------------------------------
# covariances
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 255, 256, 257, 4099])
def test_covariances_equal_the_model(gpu, count):
    rng = np.random.default_rng(count)
    xyz = im.surface(rng, count)
    pc = cloud(gpu, xyz)
    normals = unit_normals(rng, count)
    special = np.float32([m for m, _ in BAND] + [(0, 0, 0)])
    k = min(count, len(special))
    normals[:k] = special[:k] if count > 1 else special[-1:]
    for eps in (EPS, 1.0):
        for direction in (None, (0.6, 0.0, 0.8), (-1.0, 0.0, 0.0), rng.normal(size=3)):
            got = gpu.cwipc_hip_gicp_covariances(pc, normals, 0.02, 30, direction, eps)
            assert got.shape == (count, 6) and np.array_equal(got, gm.covariances(normals, direction, eps)), (count, eps, direction)
    # estimated normals: the library's own, downloaded
    estimated = gpu.cwipc_hip_estimate_normals(pc, 0.05, 30)[0]
    for direction in (None, (0.0, 1.0, 0.0)):
        got = gpu.cwipc_hip_gicp_covariances(pc, None, 0.05, 30, direction, EPS)
        assert np.array_equal(got, gm.covariances(estimated, direction, EPS))
    # a NaN direction flips nothing and makes a zero normal's covariance NaN
    got = gpu.cwipc_hip_gicp_covariances(pc, normals, 0.02, 30, (np.nan, 0.0, 0.0), EPS)
    assert np.array_equal(got, gm.covariances(normals, (np.nan, 0.0, 0.0), EPS), equal_nan=True)
    zero = (normals == 0).all(axis=1)
    assert zero.any() and np.isnan(got[zero]).all() and np.isfinite(got[~zero]).all()
    pc.free()


# ---------------------------------------------------------------------------
# sums
# ---------------------------------------------------------------------------
def test_one_source_point_is_the_models_term(gpu):
    rng = np.random.default_rng(32)
    ref_xyz = lattice_points(rng, 4096)          # (a lattice: its mean is exact in any order, so both sides turn the normals alike)
    ref_normals = unit_normals(rng, 4096)
    ref = cloud(gpu, ref_xyz)
    points = rng.uniform(-2, 2, size=(32, 3)).astype(np.float32)
    src_normals = unit_normals(rng, 32)
    turned = im.rigid(25.0, (0.3, -1.0, 0.5), (0.01, 0.02, -0.03))
    for k in range(32):
        src = cloud(gpu, points[k:k + 1])
        for T in (None, SMALL_T, turned):
            for eps in (EPS, 1.0):
                n, s = gpu.cwipc_hip_icp_gicp_sums(src, ref, T, np.inf, src_normals[k:k + 1], ref_normals, 0.02, 30, eps)
                terms = model_terms(points[k:k + 1], ref_xyz, src_normals[k:k + 1], ref_normals, T, np.inf, eps)
                assert n == 1 and terms.shape == (1, 29) and np.array_equal(s, terms[0]), (k, eps, s - terms[0])
        src.free()
    ref.free()


@pytest.fixture(scope="module")
def lattice_reference():
    rng = np.random.default_rng(4096)
    return lattice_points(rng, 4096), AXES[rng.integers(0, 6, 4096)]


@pytest.mark.parametrize("nsrc", [1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 4099, 1024 * 1024 + 1])
def test_sums_are_exact_on_lattice_clouds(gpu, lattice_reference, nsrc):
    ref_xyz, ref_normals = lattice_reference
    rng = np.random.default_rng(nsrc)
    src_xyz = lattice_points(rng, nsrc)
    src_normals = AXES[rng.integers(0, 6, nsrc)]
    src, ref = cloud(gpu, src_xyz), cloud(gpu, ref_xyz)
    big = nsrc > 100000     # (1024 * 1024 + 1: the first size whose chunk doubles; one case, the model's side takes a few seconds)
    cases = ((LATTICE_T, 10 / 64),) if big else ((None, np.inf), (None, 10 / 64), (LATTICE_T, np.inf), (LATTICE_T, 10 / 64), (QUARTER_Y, np.inf),
                                                 (QUARTER_Y, 10 / 64))
    for T, maxd in cases:
        n, s = gpu.cwipc_hip_icp_gicp_sums(src, ref, T, maxd, src_normals, ref_normals, 0.02, 30, 1.0)
        terms = model_terms(src_xyz, ref_xyz, src_normals, ref_normals, T, maxd, 1.0, tree=big)
        wn, ws = gm.gicp_sums(terms, exact=True)
        assert np.array_equal(ws, terms.sum(axis=0))   # (exact: every order gives this)
        assert n == wn and np.array_equal(s, ws), (nsrc, maxd, n, wn)
        if n:
            assert s[15] == s[18] == s[20] == n / 2     # (N = I / 2: the diagonal of the translation block of A^T N A)
        if np.isfinite(maxd) and nsrc >= 255:
            assert 0 < n < nsrc
        if not np.isfinite(maxd):
            assert n == nsrc
    src.free()
    ref.free()


@pytest.mark.parametrize("nsrc", [1, 1000, 1024, 1025, 5000, 36000])
def test_sums_on_jittered_clouds(gpu, nsrc):
    rng = np.random.default_rng(nsrc)
    ref_xyz, src_xyz = im.surface(rng, 5000), im.surface(rng, nsrc)
    src, ref = cloud(gpu, src_xyz), cloud(gpu, ref_xyz)
    src_normals, ref_normals = gpu.cwipc_hip_estimate_normals(src, 0.05, 30)[0], gpu.cwipc_hip_estimate_normals(ref, 0.05, 30)[0]
    cov_src, cov_ref = gm.cloud_covariances(src_xyz, ref_xyz, src_normals, ref_normals, EPS)
    matched = 0
    for tname, T in TRANSFORMS.items():
        for maxd in (np.inf, 0.01):
            n, s = gpu.cwipc_hip_icp_gicp_sums(src, ref, T, maxd, None, None, 0.05, 30, EPS)
            idx, d2 = im.correspondences(src_xyz, ref_xyz, T, maxd, tree=nsrc >= 5000)
            terms = gm.gicp_terms(src_xyz, ref_xyz, cov_src, cov_ref, np.eye(4) if T is None else T, idx, d2)
            sums_within_bound(n, s, terms, "jittered %d, %s, max %g" % (nsrc, tname, maxd))
            matched += n
            if tname == "far" and np.isfinite(maxd):
                assert n == 0 and np.array_equal(s, np.zeros(29))
    assert matched >= 3 * nsrc
    src.free()
    ref.free()


def test_the_orientation_step_undoes_a_negation(gpu, pairs):
    ref_xyz, src_xyz, _, _, _, _, src_normals, ref_normals, _ = pairs["5k"]
    src, ref = cloud(gpu, src_xyz), cloud(gpu, ref_xyz)
    n, s = gpu.cwipc_hip_icp_gicp_sums(src, ref, SMALL_T, MAXD, src_normals, ref_normals)
    flipped = ref_normals.copy()
    flipped[::3] = -flipped[::3]
    for a, b in ((-src_normals, ref_normals), (src_normals, -ref_normals), (-src_normals, flipped)):
        n2, s2 = gpu.cwipc_hip_icp_gicp_sums(src, ref, SMALL_T, MAXD, a, b)
        assert n2 == n and n > 0 and s2.tobytes() == s.tobytes()
    x = gpu.cwipc_hip_icp_generalized(src, ref, MAXD, None, src_normals, ref_normals, 0.02, 30, EPS, *CRITERIA)
    y = gpu.cwipc_hip_icp_generalized(src, ref, MAXD, None, -src_normals, flipped, 0.02, 30, EPS, *CRITERIA)
    assert x[0].tobytes() == y[0].tobytes() and x[1:] == y[1:] and x[3] > 0
    # ... and without a direction the sign reaches the covariance
    plain, negated = gpu.cwipc_hip_gicp_covariances(ref, ref_normals), gpu.cwipc_hip_gicp_covariances(ref, -ref_normals)
    assert plain.tobytes() != negated.tobytes()
    assert np.array_equal(plain, gm.covariances(ref_normals)) and np.array_equal(negated, gm.covariances(-ref_normals))
    d = gm.directions(src_xyz, ref_xyz)[1]
    assert gpu.cwipc_hip_gicp_covariances(ref, ref_normals, direction=d).tobytes() == gpu.cwipc_hip_gicp_covariances(ref, -ref_normals, direction=d).tobytes()


@pytest.mark.parametrize("radius,max_nn", [(0.02, 30), (0.05, 8)])
def test_estimated_normals_are_the_passed_ones(gpu, pairs, radius, max_nn):
    ref_xyz, src_xyz = pairs["5k"][:2]
    src, ref = cloud(gpu, src_xyz), cloud(gpu, ref_xyz)
    ns, nr = gpu.cwipc_hip_estimate_normals(src, radius, max_nn)[0], gpu.cwipc_hip_estimate_normals(ref, radius, max_nn)[0]
    n, s = gpu.cwipc_hip_icp_gicp_sums(src, ref, SMALL_T, MAXD, None, None, radius, max_nn)
    assert n > 0
    for a, b in ((ns, nr), (None, nr), (ns, None)):
        n2, s2 = gpu.cwipc_hip_icp_gicp_sums(src, ref, SMALL_T, MAXD, a, b, radius, max_nn)
        assert n == n2 and s.tobytes() == s2.tobytes()
    x = gpu.cwipc_hip_icp_generalized(src, ref, MAXD, None, None, None, radius, max_nn, EPS, *CRITERIA)
    y = gpu.cwipc_hip_icp_generalized(src, ref, MAXD, None, ns, nr, 1.0, 1, EPS, *CRITERIA)
    assert x[0].tobytes() == y[0].tobytes() and x[1:] == y[1:] and x[3] > 0


# ---------------------------------------------------------------------------
# the loop
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["5k", "tiles"])
def test_loop_in_lockstep_with_the_model(gpu, pairs, name):
    ref_xyz, src_xyz, T_true, tree, radius, max_nn, src_normals, ref_normals, (wT, wfit, wrmse, wit, trail, decisions) = pairs[name]
    print("%s: the model's stop decisions saw %s" % (name, ", ".join("%.1e / %.1e" % d for d in decisions)))
    src, ref = cloud(gpu, src_xyz), cloud(gpu, ref_xyz)
    cov_src, cov_ref = gm.cloud_covariances(src_xyz, ref_xyz, src_normals, ref_normals, EPS)
    assert len(trail) == wit + 1
    for k, T in enumerate(trail):
        n, s = gpu.cwipc_hip_icp_gicp_sums(src, ref, T, MAXD, None, None, radius, max_nn, EPS)
        idx, d2 = im.correspondences(src_xyz, ref_xyz, T, MAXD, tree=tree)
        sums_within_bound(n, s, gm.gicp_terms(src_xyz, ref_xyz, cov_src, cov_ref, T, idx, d2), "%s, iterate %d" % (name, k))
    T, fit, rmse, it = gpu.cwipc_hip_icp_generalized(src, ref, MAXD, None, None, None, radius, max_nn, EPS, *CRITERIA)
    print("%s: %d iterations (model %d); |T - T_model| %.3e, fitness %.3e, rmse %.3e apart; bar %.1e; |T - T_true| %.3e"
          % (name, it, wit, np.abs(T - wT).max(), abs(fit - wfit), abs(rmse - wrmse), 100 * GICP_CPU_SPREAD, np.abs(T - T_true).max()))
    assert it == wit
    assert np.abs(T - wT).max() <= 100 * GICP_CPU_SPREAD
    assert abs(fit - wfit) <= 100 * GICP_CPU_SPREAD and abs(rmse - wrmse) <= 100 * GICP_CPU_SPREAD
    if name == "5k":
        assert np.abs(T - T_true).max() <= 10 * GICP_MOTION_ERROR_MEASURED


# ---------------------------------------------------------------------------
# the class
# ---------------------------------------------------------------------------
def test_the_aligner_class(gpu, pairs):
    from conftest import make_cloud
    from cwipc_util_amd.registration import (RegistrationComputer_ICP_Generalized, RegistrationComputer_ICP_Point2Plane,
                                             RegistrationComputer_ICP_Point2Point)
    from cwipc_util_amd.registration.fine import RegistrationComputer
    ref_xyz, src_xyz = pairs["tiles"][:2]
    other = im.surface(np.random.default_rng(1), 3000)
    src = make_cloud(gpu, np.concatenate([as_points(src_xyz, 1), as_points(other, 2)]))
    ref = make_cloud(gpu, np.concatenate([as_points(ref_xyz, 4), as_points(other, 2)]))
    icp = RegistrationComputer_ICP_Generalized()
    assert isinstance(icp, RegistrationComputer) and isinstance(icp, RegistrationComputer_ICP_Point2Plane)
    assert not isinstance(icp, RegistrationComputer_ICP_Point2Point)
    assert (icp.epsilon, icp.relative_fitness, icp.relative_rmse, icp.max_iteration, icp.normal_radius, icp.normal_max_nn) == (1e-3, 1e-7, 1e-7, 60, 0.02, 30)
    icp.set_source_pointcloud(src, 1)
    icp.set_reference_pointcloud(ref, 4)
    icp.set_correspondence(MAXD)
    assert icp.run()
    s1, r4 = cloud(gpu, src_xyz, 1), cloud(gpu, ref_xyz, 4)
    T, fit, rmse, it = gpu.cwipc_hip_icp_generalized(s1, r4, MAXD, None, None, None, 0.02, 30, 1e-3, 1e-7, 1e-7, 60)
    assert icp.get_result_transformation().tobytes() == T.tobytes() and (icp.fitness, icp.inlier_rmse, icp.iterations) == (fit, rmse, it)
    assert it > 0 and not np.array_equal(T, np.eye(4))
    plane = gpu.cwipc_hip_icp_point2plane(s1, r4, MAXD, None, None, 0.02, 30, 1e-7, 1e-7, 60)[0]
    assert plane.tobytes() != T.tobytes()          # (another algorithm than its parent class's)
    moved = icp.get_result_pointcloud()
    assert moved.get_numpy_array().tobytes() == gpu.cwipc_transform(icp.get_source_pointcloud(), T).get_numpy_array().tobytes()
    assert moved.count() == len(src_xyz) and icp.get_result_pointcloud_full().count() == len(src_xyz) + len(ref_xyz)
    # epsilon and the normals' parameters reach the call
    icp.epsilon = 1e-2
    assert icp.run()
    T_eps = gpu.cwipc_hip_icp_generalized(s1, r4, MAXD, None, None, None, 0.02, 30, 1e-2, 1e-7, 1e-7, 60)[0]
    assert icp.get_result_transformation().tobytes() == T_eps.tobytes() and T_eps.tobytes() != T.tobytes()
    icp.epsilon = 1e-3
    # filters: the alignment is computed from the filtered clouds, the result is the whole source cloud, moved
    icp.normal_radius, icp.normal_max_nn = 0.05, 8
    icp.apply_source_filter(lambda pc: gpu.cwipc_crop(pc, (-9, 9, 0.2, 9, -9, 9)))
    icp.apply_reference_filter(lambda pc: gpu.cwipc_crop(pc, (-9, 9, 0.1, 9, -9, 9)))
    assert icp.run()
    T2 = gpu.cwipc_hip_icp_generalized(icp.get_filtered_source_pointcloud(), icp.get_filtered_reference_pointcloud(), MAXD, None, None, None, 0.05, 8,
                                       1e-3, 1e-7, 1e-7, 60)[0]
    assert icp.get_result_transformation().tobytes() == T2.tobytes() and T2.tobytes() != T.tobytes()
    assert 0 < icp.get_filtered_source_pointcloud().count() < len(src_xyz) and icp.get_result_pointcloud().count() == len(src_xyz)
    # correspondence 0: half the distance between the centroids, height left out
    icp.set_correspondence(0)
    assert icp.run() and icp.correspondence > 0


# ---------------------------------------------------------------------------
# determinism, edges, errors
# ---------------------------------------------------------------------------
def test_same_bytes_on_every_call_and_thread(gpu, pairs):
    ref_xyz, src_xyz, _, _, _, _, _, _, _ = pairs["5k"]
    src, ref = cloud(gpu, src_xyz), cloud(gpu, ref_xyz)
    ns, nr = gpu.cwipc_hip_estimate_normals(src, 0.05, 30)[0], gpu.cwipc_hip_estimate_normals(ref, 0.05, 30)[0]

    def everything():
        out = []
        for a, b in ((None, None), (ns, nr)):
            n, s = gpu.cwipc_hip_icp_gicp_sums(src, ref, SMALL_T, MAXD, a, b, 0.05, 30, EPS)
            T, fit, rmse, it = gpu.cwipc_hip_icp_generalized(src, ref, MAXD, None, a, b, 0.05, 30, EPS, *CRITERIA)
            out.append(np.array([n]).tobytes() + s.tobytes() + T.tobytes() + np.array([fit, rmse, it]).tobytes())
        assert out[0] == out[1]          # estimated normals against the same normals passed in
        return out[0] + gpu.cwipc_hip_gicp_covariances(ref, None, 0.05, 30, (0.0, 0.0, 1.0)).tobytes()

    first = everything()
    assert everything() == first
    results = [None] * 4

    def worker(i):
        gpu.cwipc_hip_set_device(0)
        results[i] = everything()

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert all(r == first for r in results)


def test_edges(gpu, pairs):
    dll = gpu.util.cwipc_util_dll_load()
    ref_xyz, src_xyz = pairs["5k"][:2]
    src_xyz = src_xyz[:700]
    src, ref, empty = cloud(gpu, src_xyz), cloud(gpu, ref_xyz), cloud(gpu, np.zeros((0, 3)))
    for pc in (src, ref):
        gpu.cwipc_hip_upload(pc, drop_host_copy=True)
    before = gpu.cwipc_dangling_allocations(False)
    # an empty source, an empty reference, both
    for a, b in ((empty, ref), (src, empty), (empty, empty)):
        n, s = gpu.cwipc_hip_icp_gicp_sums(a, b, SMALL_T, MAXD)
        assert n == 0 and np.array_equal(s, np.zeros(29))
        T, fit, rmse, it = gpu.cwipc_hip_icp_generalized(a, b, MAXD, SMALL_T)
        assert np.array_equal(T, SMALL_T) and (fit, rmse, it) == (0.0, 0.0, 0)
    assert gpu.cwipc_hip_gicp_covariances(empty).shape == (0, 6)
    # no correspondence at all: init comes back
    T, fit, rmse, it = gpu.cwipc_hip_icp_generalized(src, ref, 1e-7, FAR_T)
    assert np.array_equal(T, FAR_T) and (fit, rmse, it) == (0.0, 0.0, 0)
    # max_iteration 0 evaluates at init
    T, fit, rmse, it = gpu.cwipc_hip_icp_generalized(src, ref, MAXD, SMALL_T, None, None, 0.05, 30, EPS, 1e-7, 1e-7, 0)
    assert it == 0 and np.array_equal(T, SMALL_T) and fit > 0 and rmse > 0
    # one source point: A^T N A of one pair has rank 3, the update is the identity, the loop stops after one iteration at init
    one = cloud(gpu, src_xyz[:1])
    for init in (None, SMALL_T):
        T, fit, rmse, it = gpu.cwipc_hip_icp_generalized(one, ref, MAXD, init, None, None, 0.05, 30, EPS, *CRITERIA)
        assert it == 1 and T.tobytes() == (np.eye(4) if init is None else init).tobytes() and fit == 1.0 and rmse > 0
    one.free()
    # NaN and inf points in the source: they have no correspondence (the source's mean, and with it both directions, is not finite:
    # nothing is turned, which is the contract)
    bad_src = src_xyz.copy()
    bad_src[[3, 64, 699], [0, 1, 2]] = [np.nan, np.inf, -np.inf]
    bs = cloud(gpu, bad_src)
    ns, nr = gpu.cwipc_hip_estimate_normals(bs, 0.05, 30)[0], gpu.cwipc_hip_estimate_normals(ref, 0.05, 30)[0]
    n, s = gpu.cwipc_hip_icp_gicp_sums(bs, ref, SMALL_T, np.inf, None, None, 0.05, 30)
    assert n == 697 and np.isfinite(ns).all()
    cov_src, cov_ref = gm.covariances(ns, None, EPS), gm.covariances(nr, None, EPS)
    idx, d2 = im.correspondences(bad_src, ref_xyz, SMALL_T, np.inf)
    sums_within_bound(n, s, gm.gicp_terms(bad_src, ref_xyz, cov_src, cov_ref, SMALL_T, idx, d2), "non-finite source points")
    bs.free()
    # the clouds stayed where they were, and as they were
    for pc in (src, ref):
        assert dll.cwipc_hip_is_device_resident(pc.as_cwipc_p()) == 1
    assert gpu.cwipc_dangling_allocations(False) == before
    assert src.get_numpy_array().tobytes() == as_points(src_xyz).tobytes() and ref.get_numpy_array().tobytes() == as_points(ref_xyz).tobytes()


def test_error_paths(gpu):
    dll = gpu.util.cwipc_util_dll_load()
    logged = []
    gpu.cwipc_log_configure(gpu.CWIPC_LOG_LEVEL_WARNING, lambda level, msg: logged.append((level, msg)))
    try:
        pc = cloud(gpu, im.surface(np.random.default_rng(1), 300))
        p = pc.as_cwipc_p()
        inf, nan = float("inf"), float("nan")
        good = np.eye(4)
        bad = np.eye(4)
        bad[1, 3] = nan
        planes = np.zeros((3, 300), dtype=np.float32)
        planes[2] = 1
        n, s = np.full(1, 7, dtype=np.uint64), np.full(29, -1.0)
        T_out, f3 = np.zeros(16), np.zeros(3)
        it = np.zeros(1, dtype=np.int32)
        cov = np.zeros((300, 6))

        def failed(call):
            k = len(logged)
            rc = call()
            return rc == -1 and len(logged) == k + 1

        def ptr(a):
            return None if a is None else a.ctypes.data

        def both(s_, r_, T, maxd, ns, nr, radius, max_nn, eps):
            assert failed(lambda: dll.cwipc_hip_icp_gicp_sums(s_, r_, T.ctypes.data, maxd, ptr(ns), ptr(nr), radius, max_nn, eps, n.ctypes.data, s.ctypes.data))
            assert n[0] == 0 and np.array_equal(s, np.zeros(29))
            assert failed(lambda: dll.cwipc_hip_icp_generalized(s_, r_, maxd, T.ctypes.data, ptr(ns), ptr(nr), radius, max_nn, eps, 1e-7, 1e-7, 60,
                                                               T_out.ctypes.data, f3.ctypes.data, f3.ctypes.data + 8, it.ctypes.data))

        # what the plane entries reject: a NULL cloud, a bad max_distance, a matrix that is not finite
        for s_, r_, T, maxd in ((None, p, good, inf), (p, None, good, inf), (p, p, good, nan), (p, p, good, 0.0), (p, p, bad, 1.0)):
            both(s_, r_, T, maxd, planes, planes, 0.02, 30, 1e-3)
        assert failed(lambda: dll.cwipc_hip_gicp_covariances(None, planes.ctypes.data, 0.02, 30, None, 1e-3, cov.ctypes.data, 300))
        # epsilon
        for eps in (0.0, -1e-3, nan, inf):
            both(p, p, good, 1.0, planes, planes, 0.02, 30, eps)
            assert failed(lambda: dll.cwipc_hip_gicp_covariances(p, planes.ctypes.data, 0.02, 30, None, eps, cov.ctypes.data, 300))
        # a normal that is not finite, in either array
        for where, what in (((0, 0), nan), ((1, 150), inf), ((2, 299), -inf)):
            broken = planes.copy()
            broken[where] = what
            both(p, p, good, 1.0, broken, planes, 0.02, 30, 1e-3)
            both(p, p, good, 1.0, planes, broken, 0.02, 30, 1e-3)
            assert failed(lambda: dll.cwipc_hip_gicp_covariances(p, broken.ctypes.data, 0.02, 30, None, 1e-3, cov.ctypes.data, 300))
        # radius and max_nn, when either cloud's normals are to be estimated
        for radius, max_nn in ((0.0, 30), (0.02, 129)):
            for ns, nr in ((None, None), (planes, None), (None, planes)):
                both(p, p, good, 1.0, ns, nr, radius, max_nn, 1e-3)
            assert failed(lambda: dll.cwipc_hip_gicp_covariances(p, None, radius, max_nn, None, 1e-3, cov.ctypes.data, 300))
            k = len(logged)
            assert dll.cwipc_hip_icp_gicp_sums(p, p, None, 1.0, planes.ctypes.data, planes.ctypes.data, radius, max_nn, 1e-3, None, None) == 0
            assert len(logged) == k
        # the criteria, a short cap
        assert failed(lambda: dll.cwipc_hip_icp_generalized(p, p, 1.0, None, None, None, 0.02, 30, 1e-3, 1e-7, 1e-7, -1, None, None, None, None))
        assert failed(lambda: dll.cwipc_hip_icp_generalized(p, p, 1.0, None, None, None, 0.02, 30, 1e-3, nan, 1e-7, 5, None, None, None, None))
        assert failed(lambda: dll.cwipc_hip_icp_generalized(p, p, 1.0, None, None, None, 0.02, 30, 1e-3, 1e-7, nan, 5, None, None, None, None))
        assert failed(lambda: dll.cwipc_hip_gicp_covariances(p, planes.ctypes.data, 0.02, 30, None, 1e-3, cov.ctypes.data, 299))
        assert all(level == gpu.CWIPC_LOG_LEVEL_ERROR for level, _ in logged)
        # every optional output may be NULL
        k = len(logged)
        assert dll.cwipc_hip_icp_gicp_sums(p, p, None, inf, None, None, 0.02, 30, 1e-3, None, None) == 0
        assert dll.cwipc_hip_icp_generalized(p, p, 1.0, None, None, None, 0.02, 30, 1e-3, 1e-7, 1e-7, 3, None, None, None, None) == 0
        assert len(logged) == k
        # the wrappers
        for call in (lambda: gpu.cwipc_hip_icp_gicp_sums(pc, pc, bad, 1.0), lambda: gpu.cwipc_hip_icp_generalized(pc, pc, 0.0),
                     lambda: gpu.cwipc_hip_icp_generalized(pc, pc, 1.0, None, None, None, 0.0, 30),
                     lambda: gpu.cwipc_hip_icp_generalized(pc, pc, 1.0, epsilon=0.0),
                     lambda: gpu.cwipc_hip_icp_gicp_sums(pc, pc, None, 1.0, np.full((300, 3), nan)),
                     lambda: gpu.cwipc_hip_gicp_covariances(pc, epsilon=-1.0)):
            with pytest.raises(gpu.CwipcError):
                call()
        for call in (lambda: gpu.cwipc_hip_icp_gicp_sums(pc, pc, None, 1.0, np.zeros((299, 3))),
                     lambda: gpu.cwipc_hip_icp_gicp_sums(pc, pc, None, 1.0, None, np.zeros((301, 3))),
                     lambda: gpu.cwipc_hip_icp_generalized(pc, pc, 1.0, None, np.zeros((300, 2))),
                     lambda: gpu.cwipc_hip_gicp_covariances(pc, np.zeros((299, 3))),
                     lambda: gpu.cwipc_hip_icp_generalized(pc, pc, 1.0, np.eye(3))):
            with pytest.raises(ValueError):
                call()
        # a cloud against itself: every point is its own correspondence, every residual is 0
        n1, s1 = gpu.cwipc_hip_icp_gicp_sums(pc, pc, None, inf, planes.T, planes.T)
        assert n1 == 300 and np.array_equal(s1[21:], np.zeros(8)) and s1[20] > 0
    finally:
        gpu.cwipc_log_configure(gpu.CWIPC_LOG_LEVEL_WARNING, None)
