"""Point-to-plane ICP on the GPU (kernels_icp.hip: icp_plane_sums_*, icp_point2plane; plane_fit.hpp; registration/fine.py) against
the numpy model of its contracts (tests/icp_plane_model.py, checked on the CPU by tests/test_icp_plane_model.py).  open3d is not
available: the model restates the published algorithm, nothing here is compared with open3d's output.  Unless a test says
otherwise the model's normals are the library's own, downloaded with cwipc_hip_estimate_normals (tests/test_gpu_direction.py
checks those), and the library is called without normals, so it estimates the same ones on the device.

Bars:
  * sums on lattice clouds (coordinates multiples of 1/64 within +-2, normals with components in {0, +-0.5, +-1}, T the identity or a
    lattice translation: every term and every sum is exact in f64): n and all 29 sums numpy.array_equal with the model;
  * sums on jittered clouds: n exact, each sum within (n + 3) * 2^-53 * sum |term| of math.fsum over the model's terms -- the worst
    case of any summation order plus the terms' own roundings: derived, not measured (as tests/test_gpu_icp.py);
  * negated normals, estimated against passed normals, repeated calls and threads: the same bytes;
  * the loop: at each of the model's iterates the library's sums are within the bound above; the library's own loop ends after the
    model's number of iterations with T, fitness and rmse within 100 x PLANE_CPU_SPREAD (tests/test_icp_plane_model.py) of the
    model's -- the factor of tests/test_gpu_icp.py and the KDE tests; the 5 k pair ends within ten times the CPU-measured error of
    the motion it was made with.  (tests/test_icp_plane_model.py asserts that the model's stop decisions on these pairs are clear
    ones; the decisions of the runs here, with the library's normals, are printed.)"""
import threading

import numpy as np
import pytest

import icp_model as im
import icp_plane_model as pm
from test_gpu_icp import as_points, cloud, SMALL_T, FAR_T, TRANSFORMS
from test_icp_plane_model import PLANE_CPU_SPREAD, PLANE_MOTION_ERROR_MEASURED, CRITERIA, MAXD, PAIRS

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


def sums_within_bound(got_n, got, terms, label):
    n, want = pm.plane_sums(terms, exact=True)
    assert got_n == n, (label, got_n, n)
    bound = (n + 3) * U * np.abs(terms).sum(axis=0) if n else np.zeros(pm.NSUM)
    err = np.abs(got - want)
    print("%s: n %d, largest error over bound %.3f" % (label, n, float(np.max(err / np.maximum(bound, 1e-300))) if n else 0.0))
    assert np.all(err <= bound), (label, err, bound)


@pytest.fixture(scope="module")
def pairs(gpu):
    """The loop's two pairs, the library's normals of the reference cloud and the model's run with them (numpy sums), computed once."""
    out = {}
    for name, (make, tree, radius, max_nn) in PAIRS.items():
        ref, src, T_true = make()
        pc = cloud(gpu, ref)
        normals, _, _ = gpu.cwipc_hip_estimate_normals(pc, radius, max_nn)
        pc.free()
        out[name] = (ref, src, T_true, tree, radius, max_nn, normals, pm.icp_plane(src, ref, normals, MAXD, None, *CRITERIA, tree=tree))
    return out


# ---------------------------------------------------------------------------
# sums
# ---------------------------------------------------------------------------
def lattice_points(rng, n):
    return (rng.integers(-128, 129, size=(n, 3)) / 64.0).astype(np.float32)


LATTICE_T = im.rigid(0.0, (0, 1, 0), (3 / 64, -2 / 64, 1 / 64))


@pytest.fixture(scope="module")
def lattice_reference():
    rng = np.random.default_rng(4096)
    ref = lattice_points(rng, 4096)
    normals = rng.choice(np.float32([0, 0.5, -0.5, 1, -1]), size=(4096, 3))
    return ref, normals


@pytest.mark.parametrize("nsrc", [1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 4099, 1024 * 1024 + 1])
def test_sums_are_exact_on_lattice_clouds(gpu, lattice_reference, nsrc):
    ref_xyz, normals = lattice_reference
    src_xyz = lattice_points(np.random.default_rng(nsrc), nsrc)
    src, ref = cloud(gpu, src_xyz), cloud(gpu, ref_xyz)
    big = nsrc > 100000     # (1024 * 1024 + 1: the first size whose chunk doubles; one case, the model's side takes a few seconds)
    for T, maxd in ((LATTICE_T, 10 / 64),) if big else ((None, np.inf), (None, 10 / 64), (LATTICE_T, np.inf), (LATTICE_T, 10 / 64)):
        n, s = gpu.cwipc_hip_icp_plane_sums(src, ref, T, maxd, normals)
        idx, d2 = im.correspondences(src_xyz, ref_xyz, T, maxd, tree=big)
        terms = pm.plane_terms(src_xyz, ref_xyz, normals, np.eye(4) if T is None else T, idx, d2)
        wn, ws = pm.plane_sums(terms, exact=True)
        assert np.array_equal(ws, terms.sum(axis=0))   # (exact: every order gives this)
        assert n == wn and np.array_equal(s, ws), (nsrc, maxd, n, wn)
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
    normals, _, _ = gpu.cwipc_hip_estimate_normals(ref, 0.05, 30)
    matched = 0
    for tname, T in TRANSFORMS.items():
        for maxd in (np.inf, 0.01):
            n, s = gpu.cwipc_hip_icp_plane_sums(src, ref, T, maxd, None, 0.05, 30)
            idx, d2 = im.correspondences(src_xyz, ref_xyz, T, maxd, tree=nsrc >= 5000)
            terms = pm.plane_terms(src_xyz, ref_xyz, normals, np.eye(4) if T is None else T, idx, d2)
            sums_within_bound(n, s, terms, "jittered %d, %s, max %g" % (nsrc, tname, maxd))
            matched += n
            if tname == "far" and np.isfinite(maxd):
                assert n == 0 and np.array_equal(s, np.zeros(29))
    assert matched >= 3 * nsrc


def test_the_sign_of_a_normal_does_not_matter(gpu, pairs):
    ref_xyz, src_xyz, _, _, _, _, normals, _ = pairs["5k"]
    src, ref = cloud(gpu, src_xyz), cloud(gpu, ref_xyz)
    n, s = gpu.cwipc_hip_icp_plane_sums(src, ref, SMALL_T, MAXD, normals)
    flipped = normals.copy()
    flipped[::3] = -flipped[::3]
    for other in (-normals, flipped):
        n2, s2 = gpu.cwipc_hip_icp_plane_sums(src, ref, SMALL_T, MAXD, other)
        assert n2 == n and n > 0 and s2.tobytes() == s.tobytes()
    a = gpu.cwipc_hip_icp_point2plane(src, ref, MAXD, None, normals, 0.02, 30, *CRITERIA)
    b = gpu.cwipc_hip_icp_point2plane(src, ref, MAXD, None, -normals, 0.02, 30, *CRITERIA)
    assert a[0].tobytes() == b[0].tobytes() and a[1:] == b[1:]


@pytest.mark.parametrize("radius,max_nn", [(0.02, 30), (0.05, 8)])
def test_estimated_normals_are_the_passed_ones(gpu, pairs, radius, max_nn):
    ref_xyz, src_xyz, _, _, _, _, _, _ = pairs["5k"]
    src, ref = cloud(gpu, src_xyz), cloud(gpu, ref_xyz)
    normals, _, _ = gpu.cwipc_hip_estimate_normals(ref, radius, max_nn)
    n, s = gpu.cwipc_hip_icp_plane_sums(src, ref, SMALL_T, MAXD, None, radius, max_nn)
    n2, s2 = gpu.cwipc_hip_icp_plane_sums(src, ref, SMALL_T, MAXD, normals)
    assert n == n2 and n > 0 and s.tobytes() == s2.tobytes()
    a = gpu.cwipc_hip_icp_point2plane(src, ref, MAXD, None, None, radius, max_nn, *CRITERIA)
    b = gpu.cwipc_hip_icp_point2plane(src, ref, MAXD, None, normals, 1.0, 1, *CRITERIA)
    assert a[0].tobytes() == b[0].tobytes() and a[1:] == b[1:] and a[3] > 0


# ---------------------------------------------------------------------------
# the loop
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["5k", "tiles"])
def test_loop_in_lockstep_with_the_model(gpu, pairs, name):
    ref_xyz, src_xyz, T_true, tree, radius, max_nn, normals, (wT, wfit, wrmse, wit, trail, decisions) = pairs[name]
    print("%s: the model's stop decisions saw %s" % (name, ", ".join("%.1e / %.1e" % d for d in decisions)))
    src, ref = cloud(gpu, src_xyz), cloud(gpu, ref_xyz)
    assert len(trail) == wit + 1
    for k, T in enumerate(trail):
        n, s = gpu.cwipc_hip_icp_plane_sums(src, ref, T, MAXD, None, radius, max_nn)
        idx, d2 = im.correspondences(src_xyz, ref_xyz, T, MAXD, tree=tree)
        sums_within_bound(n, s, pm.plane_terms(src_xyz, ref_xyz, normals, T, idx, d2), "%s, iterate %d" % (name, k))
    T, fit, rmse, it = gpu.cwipc_hip_icp_point2plane(src, ref, MAXD, None, None, radius, max_nn, *CRITERIA)
    print("%s: %d iterations (model %d); |T - T_model| %.3e, fitness %.3e, rmse %.3e apart; bar %.1e; |T - T_true| %.3e"
          % (name, it, wit, np.abs(T - wT).max(), abs(fit - wfit), abs(rmse - wrmse), 100 * PLANE_CPU_SPREAD, np.abs(T - T_true).max()))
    assert it == wit
    assert np.abs(T - wT).max() <= 100 * PLANE_CPU_SPREAD
    assert abs(fit - wfit) <= 100 * PLANE_CPU_SPREAD and abs(rmse - wrmse) <= 100 * PLANE_CPU_SPREAD
    if name == "5k":
        assert np.abs(T - T_true).max() <= 10 * PLANE_MOTION_ERROR_MEASURED


def test_singular_geometry_leaves_init_alone(gpu):
    g = np.stack(np.meshgrid(np.arange(40), np.arange(40), indexing="ij"), axis=-1).reshape(-1, 2) / 64.0
    ref_xyz = np.concatenate([g, np.zeros((len(g), 1))], axis=1).astype(np.float32)
    src_xyz = ref_xyz + np.float32([0, 0, 1 / 64])
    normals = np.tile(np.float32([0, 0, 1]), (len(g), 1))
    src, ref = cloud(gpu, src_xyz), cloud(gpu, ref_xyz)
    T, fit, rmse, it = gpu.cwipc_hip_icp_point2plane(src, ref, np.inf, None, normals, 0.02, 30, *CRITERIA)
    assert it == 1 and T.tobytes() == np.eye(4).tobytes() and fit == 1.0 and rmse == 1 / 64
    want = pm.icp_plane(src_xyz, ref_xyz, normals, np.inf, None, *CRITERIA)
    assert want[3] == 1 and np.array_equal(want[0], np.eye(4)) and want[1:3] == (1.0, 1 / 64)
    # ... whatever init is: every normal is the same one, so the system has rank 3
    T, fit, rmse, it = gpu.cwipc_hip_icp_point2plane(src, ref, np.inf, SMALL_T, normals, 0.02, 30, *CRITERIA)
    assert it == 1 and T.tobytes() == SMALL_T.tobytes() and fit == 1.0


# ---------------------------------------------------------------------------
# the class
# ---------------------------------------------------------------------------
def test_the_aligner_class(gpu, pairs):
    from conftest import make_cloud
    from cwipc_util_amd.registration import RegistrationComputer_ICP_Point2Plane, RegistrationComputer_ICP_Point2Point
    from cwipc_util_amd.registration.fine import RegistrationComputer
    ref_xyz, src_xyz, _, _, _, _, _, _ = pairs["tiles"]
    other = im.surface(np.random.default_rng(1), 3000)
    src = make_cloud(gpu, np.concatenate([as_points(src_xyz, 1), as_points(other, 2)]))
    ref = make_cloud(gpu, np.concatenate([as_points(ref_xyz, 4), as_points(other, 2)]))
    icp = RegistrationComputer_ICP_Point2Plane()
    assert isinstance(icp, RegistrationComputer) and not isinstance(icp, RegistrationComputer_ICP_Point2Point)
    assert (icp.relative_fitness, icp.relative_rmse, icp.max_iteration, icp.normal_radius, icp.normal_max_nn) == (1e-7, 1e-7, 60, 0.02, 30)
    icp.set_source_pointcloud(src, 1)
    icp.set_reference_pointcloud(ref, 4)
    icp.set_correspondence(MAXD)
    assert icp.run()
    s1, r4 = cloud(gpu, src_xyz, 1), cloud(gpu, ref_xyz, 4)
    T, fit, rmse, it = gpu.cwipc_hip_icp_point2plane(s1, r4, MAXD, None, None, 0.02, 30, 1e-7, 1e-7, 60)
    assert icp.get_result_transformation().tobytes() == T.tobytes() and (icp.fitness, icp.inlier_rmse, icp.iterations) == (fit, rmse, it)
    assert it > 0 and not np.array_equal(T, np.eye(4))
    moved = icp.get_result_pointcloud()
    assert moved.get_numpy_array().tobytes() == gpu.cwipc_transform(icp.get_source_pointcloud(), T).get_numpy_array().tobytes()
    assert moved.count() == len(src_xyz) and icp.get_result_pointcloud_full().count() == len(src_xyz) + len(ref_xyz)
    # filters: the alignment is computed from the filtered clouds, the result is the whole source cloud, moved
    icp.normal_radius, icp.normal_max_nn = 0.05, 8
    icp.apply_source_filter(lambda pc: gpu.cwipc_crop(pc, (-9, 9, 0.2, 9, -9, 9)))
    icp.apply_reference_filter(lambda pc: gpu.cwipc_crop(pc, (-9, 9, 0.1, 9, -9, 9)))
    assert icp.run()
    T2 = gpu.cwipc_hip_icp_point2plane(icp.get_filtered_source_pointcloud(), icp.get_filtered_reference_pointcloud(), MAXD, None, None, 0.05, 8,
                                       1e-7, 1e-7, 60)[0]
    assert icp.get_result_transformation().tobytes() == T2.tobytes() and T2.tobytes() != T.tobytes()
    assert 0 < icp.get_filtered_source_pointcloud().count() < len(src_xyz) and icp.get_result_pointcloud().count() == len(src_xyz)
    # correspondence 0: half the distance between the centroids, height left out
    icp.set_correspondence(0)
    assert icp.run() and icp.correspondence > 0


# ---------------------------------------------------------------------------
# determinism, edges, errors
# ---------------------------------------------------------------------------
def test_same_bytes_on_every_call_and_thread(gpu, pairs):
    ref_xyz, src_xyz, _, _, _, _, normals, _ = pairs["5k"]
    src, ref = cloud(gpu, src_xyz), cloud(gpu, ref_xyz)

    def everything():
        out = b""
        for given in (None, normals):
            n, s = gpu.cwipc_hip_icp_plane_sums(src, ref, SMALL_T, MAXD, given, 0.05, 30)
            T, fit, rmse, it = gpu.cwipc_hip_icp_point2plane(src, ref, MAXD, None, given, 0.05, 30, *CRITERIA)
            out += np.array([n]).tobytes() + s.tobytes() + T.tobytes() + np.array([fit, rmse, it]).tobytes()
        return out

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


def against_model(gpu, src_xyz, ref_xyz, init, max_iteration=CRITERIA[2], radius=0.05, max_nn=30, maxd=MAXD):
    """One run of the library, without normals, against the model with the library's normals"""
    src, ref = cloud(gpu, src_xyz), cloud(gpu, ref_xyz)
    normals, _, _ = gpu.cwipc_hip_estimate_normals(ref, radius, max_nn)
    want = pm.icp_plane(src_xyz, ref_xyz, normals, maxd, init, CRITERIA[0], CRITERIA[1], max_iteration)
    T, fit, rmse, it = gpu.cwipc_hip_icp_point2plane(src, ref, maxd, init, None, radius, max_nn, CRITERIA[0], CRITERIA[1], max_iteration)
    assert it == want[3] and np.abs(T - want[0]).max() <= 100 * PLANE_CPU_SPREAD
    assert abs(fit - want[1]) <= 100 * PLANE_CPU_SPREAD and abs(rmse - want[2]) <= 100 * PLANE_CPU_SPREAD
    src.free()
    ref.free()
    return T, fit, rmse, it, normals


def test_edges(gpu, pairs):
    dll = gpu.util.cwipc_util_dll_load()
    ref_xyz, src_xyz, _, _, _, _, _, _ = pairs["5k"]
    src_xyz = src_xyz[:700]
    src, ref, empty = cloud(gpu, src_xyz), cloud(gpu, ref_xyz), cloud(gpu, np.zeros((0, 3)))
    for pc in (src, ref):
        gpu.cwipc_hip_upload(pc, drop_host_copy=True)
    before = gpu.cwipc_dangling_allocations(False)
    # an empty source, an empty reference
    for a, b in ((empty, ref), (src, empty), (empty, empty)):
        n, s = gpu.cwipc_hip_icp_plane_sums(a, b, SMALL_T, MAXD)
        assert n == 0 and np.array_equal(s, np.zeros(29))
        T, fit, rmse, it = gpu.cwipc_hip_icp_point2plane(a, b, MAXD, SMALL_T)
        assert np.array_equal(T, SMALL_T) and (fit, rmse, it) == (0.0, 0.0, 0)
    # no correspondence at all: init comes back
    T, fit, rmse, it = gpu.cwipc_hip_icp_point2plane(src, ref, 1e-7, FAR_T)
    assert np.array_equal(T, FAR_T) and (fit, rmse, it) == (0.0, 0.0, 0)
    # init given; max_iteration 0 evaluates at init
    for init in (None, SMALL_T):
        against_model(gpu, src_xyz, ref_xyz, init)
        T, fit, rmse, it, _ = against_model(gpu, src_xyz, ref_xyz, init, max_iteration=0)
        assert it == 0 and np.array_equal(T, np.eye(4) if init is None else init) and fit > 0
    # a reference of one point and of two: their normals are (0, 0, +-1) by the fewer-than-three rule, the system is singular
    # (no bound on the distance: every source point is matched; under 5 cm none is, and init comes back after no iteration)
    for nref in (1, 2):
        T, fit, rmse, it, normals = against_model(gpu, src_xyz, ref_xyz[:nref], None, maxd=np.inf)
        assert np.array_equal(np.abs(normals), np.tile(np.float32([0, 0, 1]), (nref, 1)))
        assert it == 1 and np.array_equal(T, np.eye(4)) and fit == 1.0 and rmse > 0
        against_model(gpu, src_xyz, ref_xyz[:nref], None)
    against_model(gpu, src_xyz[:1], ref_xyz, None)
    # NaN and inf points in either cloud
    bad_src, bad_ref = src_xyz.copy(), ref_xyz.copy()
    bad_src[[3, 64, 699], [0, 1, 2]] = [np.nan, np.inf, -np.inf]
    bad_ref[[0, 100, 4999], [2, 0, 1]] = [np.nan, -np.inf, np.nan]
    T, fit, rmse, it, normals = against_model(gpu, bad_src, ref_xyz, None)
    assert it > 0 and fit == 697 / 700
    T, fit, rmse, it, normals = against_model(gpu, bad_src, bad_ref, None)
    assert it > 0 and np.isfinite(normals).all()
    bs, br = cloud(gpu, bad_src), cloud(gpu, bad_ref)
    n, s = gpu.cwipc_hip_icp_plane_sums(bs, br, SMALL_T, np.inf, None, 0.05, 30)
    idx, d2 = im.correspondences(bad_src, bad_ref, SMALL_T, np.inf)
    assert n == 697 and not np.isin(idx, [0, 100, 4999]).any()
    sums_within_bound(n, s, pm.plane_terms(bad_src, bad_ref, normals, SMALL_T, idx, d2), "non-finite points")
    bs.free()
    br.free()
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
        empty = cloud(gpu, np.zeros((0, 3)))
        p = pc.as_cwipc_p()
        inf, nan = float("inf"), float("nan")
        good = np.eye(4)
        bad = np.eye(4)
        bad[1, 3] = nan
        worse = np.eye(4)
        worse[0, 0] = inf
        planes = np.zeros((3, 300), dtype=np.float32)
        planes[2] = 1
        n, s = np.full(1, 7, dtype=np.uint64), np.full(29, -1.0)
        T_out, f3 = np.zeros(16), np.zeros(3)
        it = np.zeros(1, dtype=np.int32)

        def failed(call):
            k = len(logged)
            rc = call()
            return rc == -1 and len(logged) > k

        def both(s_, r_, T, maxd, normals, radius, max_nn):
            nrm = None if normals is None else normals.ctypes.data
            assert failed(lambda: dll.cwipc_hip_icp_plane_sums(s_, r_, T.ctypes.data, maxd, nrm, radius, max_nn, n.ctypes.data, s.ctypes.data))
            assert n[0] == 0 and np.array_equal(s, np.zeros(29))
            assert failed(lambda: dll.cwipc_hip_icp_point2plane(s_, r_, maxd, T.ctypes.data, nrm, radius, max_nn, 1e-7, 1e-7, 60, T_out.ctypes.data,
                                                               f3.ctypes.data, f3.ctypes.data + 8, it.ctypes.data))

        # a NULL cloud, a bad max_distance, a matrix that is not finite
        for s_, r_, T, maxd in ((None, p, good, inf), (p, None, good, inf), (p, p, good, nan), (p, p, good, 0.0), (p, p, good, -1.0), (p, p, bad, 1.0),
                                (p, p, worse, 1.0)):
            both(s_, r_, T, maxd, planes, 0.02, 30)
        # radius and max_nn as direction_normals rejects them -- when the normals are to be estimated (also for empty clouds)
        for radius, max_nn in ((0.0, 30), (-1.0, 30), (inf, 30), (nan, 30), (0.02, 0), (0.02, 129), (0.02, -5)):
            both(p, p, good, 1.0, None, radius, max_nn)
            both(empty.as_cwipc_p(), p, good, 1.0, None, radius, max_nn)
            k = len(logged)
            assert dll.cwipc_hip_icp_plane_sums(p, p, None, 1.0, planes.ctypes.data, radius, max_nn, None, None) == 0 and len(logged) == k
        # caller's normals that are not finite
        for where, what in (((0, 0), nan), ((1, 150), inf), ((2, 299), -inf)):
            broken = planes.copy()
            broken[where] = what
            both(p, p, good, 1.0, broken, 0.02, 30)
        assert failed(lambda: dll.cwipc_hip_icp_point2plane(p, p, 1.0, None, None, 0.02, 30, 1e-7, 1e-7, -1, None, None, None, None))
        assert failed(lambda: dll.cwipc_hip_icp_point2plane(p, p, 1.0, None, None, 0.02, 30, nan, 1e-7, 5, None, None, None, None))
        assert all(level == gpu.CWIPC_LOG_LEVEL_ERROR for level, _ in logged)
        # every optional output may be NULL
        k = len(logged)
        assert dll.cwipc_hip_icp_plane_sums(p, p, None, inf, None, 0.02, 30, None, None) == 0
        assert dll.cwipc_hip_icp_point2plane(p, p, 1.0, None, None, 0.02, 30, 1e-7, 1e-7, 3, None, None, None, None) == 0
        assert len(logged) == k
        for call in (lambda: gpu.cwipc_hip_icp_plane_sums(pc, pc, bad, 1.0), lambda: gpu.cwipc_hip_icp_point2plane(pc, pc, 0.0),
                     lambda: gpu.cwipc_hip_icp_point2plane(pc, pc, 1.0, None, None, 0.0, 30),
                     lambda: gpu.cwipc_hip_icp_plane_sums(pc, pc, None, 1.0, np.full((300, 3), nan))):
            with pytest.raises(gpu.CwipcError):
                call()
        with pytest.raises(ValueError):
            gpu.cwipc_hip_icp_plane_sums(pc, pc, None, 1.0, np.zeros((299, 3)))
        with pytest.raises(ValueError):
            gpu.cwipc_hip_icp_point2plane(pc, pc, 1.0, np.eye(3))
        # a cloud against itself: every point is its own correspondence, every residual is 0
        n1, s1 = gpu.cwipc_hip_icp_plane_sums(pc, pc, None, inf, planes.T)
        assert n1 == 300 and np.array_equal(s1[21:], np.zeros(8)) and s1[20] == 300.0
    finally:
        gpu.cwipc_log_configure(gpu.CWIPC_LOG_LEVEL_WARNING, None)
