"""The numpy model of generalized ICP (tests/icp_gicp_model.py) checked on the CPU: its N = M^-1 form against the published
W = (M^-1)^(1/2) form, its loop against a known motion, how far two f64 summation orders move its result, that its stop decisions on
the test pairs are clear ones, and the covariance in and around the band where open3d's Rx is the identity.  Plus, without a GPU,
the boundary: the library exports the three new symbols, the header and the wrapper declare them, the class has the reference's
constants.

open3d is not available, so no reference output exists: the model restates the published algorithm (open3d's
registration_generalized_icp with TransformationEstimationForGeneralizedICP, epsilon 1e-3), and the GPU tests
(tests/test_gpu_icp_gicp.py) compare the library with it.  The normals here come from a plain f64 estimate
(icp_plane_model.estimate_normals), on both clouds.

PAIRS: the loop's two inputs, shared with the GPU tests: a 5 k pair with normals from the 30 nearest points within 0.05 and two 36 k
tiles at the pipeline's radius 0.02 and max_nn 30; max distance 0.05 and the class's criteria (1e-7, 1e-7, 60) on both.  They are
icp_model.test_pair_5k and icp_plane_model.test_pair_tiles_plane from other seeds (icp_gicp_model.test_pair_5k_gicp, seed 26, and
test_pair_tiles_gicp, seed 64): on the original seeds the third stop decision of either pair sees an rmse change of 2.2e-7, between
0.1 and 10 times the criterion 1e-7, and the condition below stays while the input goes.  The generators' docstrings have the scan.

N_AGAINST_W_MEASURED: the largest difference between the N form's and the W form's J^T J, J^T r and r^T r over the 5000 matched pairs
of the 5 k pair at the model's second iterate, relative to the pair's largest |entry| of the W form: 5.41e-13 measured, 5.5e-13
recorded; 100 times it is allowed.  (Above 1e-9 one of the two forms would be wrong.  numpy.linalg.eigh of a 3x3 with
eigenvalues from 2e-3 to 2 leaves about cond * 2^-53 = 1e-13 in W: the difference is the W form's.)

GICP_MOTION_ERROR_MEASURED: the largest entry of |T_model - T_true| on the 5 k pair: 7.60e-9 measured, 7.7e-9 recorded, reached after 3
updates of the model's 4 (|T_k - T_true| 3.3e-2, 1.3e-3, 1.5e-6, 7.6e-9, 7.6e-9) (2.70e-9 on icp_model.test_pair_5k itself, which the issue names: the same test asserts it).  The GPU bar is
ten times the figure.

GICP_CPU_SPREAD: the largest difference in the final T, fitness and rmse between the model run with numpy.sum and with math.fsum
sums, over the two pairs: 1.15e-16 measured (the tiles; 7.5e-17 on the 5 k pair), 1.2e-16 recorded -- the
counterpart of PLANE_CPU_SPREAD: the GPU tests allow 100 times it.

The condition on the inputs: at every stop decision of both runs of both pairs each |change| is below 0.1 x or above 10 x its
criterion, so no rounding difference between two correct implementations changes the iteration count.  Measured (fitness / rmse
change per decision): the 5 k pair stops after 4 iterations, 2.0e-4 / 2.8e-2, 0 / 9.7e-4, 0 / 1.1e-6, 0 / 1.2e-14; the tiles
after 4, 3.6e-3 / 1.2e-2, 1.9e-4 / 4.0e-6, 2.8e-5 / 5.6e-6, 0 / 7.6e-9 (the same to two digits in both runs)."""
import os

import numpy as np
import pytest

import icp_model as im
import icp_plane_model as pm
import icp_gicp_model as gm
from test_icp_plane_model import decisions_are_clear

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_AGAINST_W_MEASURED = 5.5e-13
GICP_MOTION_ERROR_MEASURED = 7.7e-9
GICP_CPU_SPREAD = 1.2e-16
CRITERIA = (1e-7, 1e-7, 60)
MAXD = 0.05
#: name -> (the pair, whether the model takes its candidates from a KD-tree, the normals' radius and max_nn)
PAIRS = {"5k": (gm.test_pair_5k_gicp, True, 0.05, 30), "tiles": (gm.test_pair_tiles_gicp, True, 0.02, 30)}
ITERATIONS = {"5k": 4, "tiles": 4}
NEW_SYMBOLS = ("cwipc_hip_gicp_covariances", "cwipc_hip_icp_gicp_sums", "cwipc_hip_icp_generalized")


def model_run(src, ref, radius, max_nn, tree, exact=False):
    ns, nr = pm.estimate_normals(src, radius, max_nn)[0], pm.estimate_normals(ref, radius, max_nn)[0]
    return ns, nr, gm.icp_generalized(src, ref, ns, nr, MAXD, None, *CRITERIA, exact=exact, tree=tree)


@pytest.fixture(scope="module")
def runs():
    """name -> (ref, src, T_true, the source's normals, the reference's, the model's run with numpy.sum, with math.fsum)"""
    out = {}
    for name, (make, tree, radius, max_nn) in PAIRS.items():
        ref, src, T_true = make()
        ns, nr, a = model_run(src, ref, radius, max_nn, tree)
        b = gm.icp_generalized(src, ref, ns, nr, MAXD, None, *CRITERIA, exact=True, tree=tree)
        out[name] = (ref, src, T_true, ns, nr, a, b)
    return out


def test_the_n_form_is_the_published_w_form(runs):
    ref, src, _, ns, nr, a, _ = runs["5k"]
    T = a[4][1]
    cov_src, cov_ref = gm.cloud_covariances(src, ref, ns, nr)
    idx, d2 = im.correspondences(src, ref, T, MAXD, tree=True)
    hit = idx != im.NONE
    assert hit.sum() >= 1000
    p, q = im.move(T, src[hit]), ref[idx[hit]].astype(np.float64)
    terms = gm.pair_terms(p, q, cov_src[hit], cov_ref[idx[hit]], T[:3, :3], d2[hit])
    JJ, Jr, rr = gm.pair_system_w(p, q, cov_src[hit], cov_ref[idx[hit]], T[:3, :3])
    want = np.concatenate([JJ[:, gm.TRIU6[0], gm.TRIU6[1]], Jr, rr[:, None]], axis=1)
    worst = float((np.abs(terms[:, :28] - want) / np.abs(want).max(axis=1)[:, None]).max())
    print("N form against W form over %d pairs: largest relative difference %.3e" % (hit.sum(), worst))
    assert N_AGAINST_W_MEASURED <= 1e-9 and worst <= 100 * N_AGAINST_W_MEASURED


def test_loop_recovers_a_rigid_motion(runs):
    ref, src, T_true, _, _, (T, fitness, rmse, iterations, trail, _), _ = runs["5k"]
    errs = [float(np.abs(Tk - T_true).max()) for Tk in trail]
    print("generalized model on the 5 k pair: %d iterations, fitness %.6f, rmse %.3e, |T_k - T_true| %s"
          % (iterations, fitness, rmse, " ".join("%.2e" % e for e in errs)))
    assert iterations == ITERATIONS["5k"] and fitness == 1.0
    assert 0 < errs[-1] <= GICP_MOTION_ERROR_MEASURED
    # the pair the other aligners' tests use (its stop decisions are not clear ones, which this figure does not need)
    ref, src, T_true = im.test_pair_5k()
    _, _, (T, fitness, _, iterations, _, _) = model_run(src, ref, 0.05, 30, True)
    err = float(np.abs(T - T_true).max())
    print("... and on icp_model.test_pair_5k: %d iterations, |T - T_true| %.3e" % (iterations, err))
    assert fitness == 1.0 and err <= GICP_MOTION_ERROR_MEASURED


def test_gicp_cpu_spread_and_clear_stop_decisions(runs):
    worst = 0.0
    for name, (_, src, _, _, _, a, b) in runs.items():
        assert a[3] == b[3] == ITERATIONS[name] < CRITERIA[2]
        for run in (a, b):
            assert len(run[5]) == run[3]
            decisions_are_clear(run[5], CRITERIA)
        spread = max(float(np.abs(a[0] - b[0]).max()), abs(a[1] - b[1]), abs(a[2] - b[2]))
        print("gicp_cpu_spread, %s, %d source points, %d iterations: %.3e; the stop decisions saw %s"
              % (name, len(src), a[3], spread, ", ".join("%.1e / %.1e" % d for d in a[5])))
        worst = max(worst, spread)
    assert 0 < worst <= GICP_CPU_SPREAD


def test_the_band_around_minus_x():
    eps = 1e-3
    flat = np.array([eps, 0, 0, 1, 0, 1.0])                      # diag(eps, 1, 1)

    def cov(m, d=None):
        return gm.covariances(np.float32([m]), d, eps)[0]

    s995, s98 = np.sqrt(1 - 0.995 ** 2), np.sqrt(1 - 0.98 ** 2)
    # inside the band Rx is the identity whatever the normal: the covariance is flat along x, not along the normal
    assert np.array_equal(cov((-1, 0, 0)), flat) and np.array_equal(cov((-0.995, s995, 0)), flat)
    # outside it the covariance is flat along the normal: m^T C m = eps, and the trace is 2 + eps
    for m in ((-0.98, s98, 0), (1, 0, 0), (0, 0, 1), (0.995, -s995, 0)):
        C = gm.full3(cov(m)[None])[0]
        m64 = np.float32(m).astype(np.float64)
        tol = 8 * 2.0 ** -24 / (1 + m64[0])   # (a float32 normal is a unit vector to 2^-24 per component, and f = 1 / (1 + m0) carries that into Rx)
        assert abs(m64 @ C @ m64 - eps) <= tol and abs(np.trace(C) - (2 + eps)) <= tol, m
    assert np.array_equal(cov((1, 0, 0)), flat)
    assert np.allclose(cov((0, 0, 1)), [1, 0, 0, 1, 0, eps], atol=1e-15)
    # the sign reaches the covariance inside the band: (0.995, -s, 0) turned to face -x lands in it
    inside, outside = cov((0.995, -s995, 0), (-1, 0, 0)), cov((0.995, -s995, 0), (1, 0, 0))
    assert np.array_equal(inside, flat) and np.abs(inside - outside).max() > 1e-3
    # ... and outside the band only at rounding level
    a, b = cov((0.6, 0.48, 0.64)), cov((-0.6, -0.48, -0.64))
    assert 0 < np.abs(a - b).max() <= 1e-6 or np.array_equal(a, b)
    # a zero normal takes the direction; without one it stays zero, and Rx is the identity again
    C = gm.full3(cov((0, 0, 0), (0.6, 0, 0.8))[None])[0]
    assert abs(np.array([0.6, 0, 0.8]) @ C @ [0.6, 0, 0.8] - eps) <= 1e-15 and abs(np.trace(C) - (2 + eps)) <= 1e-15
    zero_turned = gm.orient(np.float32([[0, 0, 0]]), (0.6, 0, 0.8))[0]
    assert np.array_equal(zero_turned, [0.6, 0, 0.8]) and np.array_equal(cov((0, 0, 0)), flat)
    # a NaN direction never flips a normal, and a zero normal becomes NaN with it
    nan = (np.nan, np.nan, np.nan)
    assert np.array_equal(gm.orient(np.float32([[0, -1, 0]]), nan)[0], [0, -1, 0]) and np.array_equal(cov((0, -1, 0), nan), cov((0, -1, 0)))
    assert np.array_equal(gm.orient(np.float32([[0, -1, 0]]), (0, 1, np.nan))[0], [0, -1, 0])
    assert np.isnan(cov((0, 0, 0), nan)).all()
    # orientation: against the direction is negated, along it and perpendicular to it is kept
    got = gm.orient(np.float32([[0, 0, 1], [0, 0, -1], [1, 0, 0]]), (0, 0, 2.0))
    assert np.array_equal(got, [[0, 0, 1], [0, 0, 1], [1, 0, 0]])


def test_new_symbols_are_exported_and_declared(cwipc):
    from cwipc_util_amd.util import _SIGNATURES
    dll = cwipc.cwipc_util_dll_load()
    header = open(os.path.join(ROOT, "include", "cwipc_util_amd", "hip_ext.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(dll, name) and name in _SIGNATURES and name in cwipc.util.__all__, name
        assert "_CWIPC_UTIL_EXPORT int %s(cwipc_pointcloud *" % name in header, name
    import cwipc_util_amd.registration as reg
    from cwipc_util_amd.registration import fine
    G = reg.RegistrationComputer_ICP_Generalized
    assert issubclass(G, reg.RegistrationComputer_ICP_Point2Plane) and "RegistrationComputer_ICP_Generalized" in fine.__all__
    assert (G.epsilon, G.relative_fitness, G.relative_rmse, G.max_iteration, G.normal_radius, G.normal_max_nn) == (1e-3, 1e-7, 1e-7, 60, 0.02, 30)
    # the default and the list stay as tests/test_gpu_icp.py asserts them
    assert fine.DEFAULT_FINE_ALIGNMENT_ALGORITHM is reg.RegistrationComputer_ICP_Point2Point and G not in fine.ALL_FINE_ALIGNMENT_ALGORITHMS
