"""The numpy model of point-to-plane ICP (tests/icp_plane_model.py) checked on the CPU: its loop against a known motion, how far
two f64 summation orders move its result, that its stop decisions on the test pairs are clear ones, and that a normal's sign does
not reach a term.  Plus, without a GPU, the boundary: the library exports the two new symbols, the header and the wrapper declare them.

open3d is not available, so no reference output exists: the model restates the published algorithm (open3d's
TransformationEstimationPointToPlane inside registration_icp), and the GPU tests (tests/test_gpu_icp_plane.py) compare the
library with it.  The normals here come from a plain f64 estimate (icp_plane_model.estimate_normals: KD-tree, numpy.linalg.eigh).

PAIRS: the loop's two inputs, shared with the GPU tests.  The 5 k pair (icp_model.test_pair_5k) with normals from the 30 nearest
points within 0.05 -- at the pipeline's 0.02 a 5 k cloud is too sparse (the median neighbourhood holds 12 points at 0.05) -- and two
36 k tiles (icp_plane_model.test_pair_tiles_plane) at the pipeline's radius 0.02 and max_nn 30; max distance 0.05 and the
point-to-plane class's criteria (1e-7, 1e-7, 60) on both.

PLANE_MOTION_ERROR_MEASURED: the largest entry of |T_model - T_true| on the 5 k pair, measured here: 3.17e-9, reached after 3
updates (4 iterations; point-to-point needs its whole loop for 1.1e-9), with cond(A) = 5.2e2 and det(A) = 1.6e16 at the first
iterate.  The bar is ten times that.

PLANE_CPU_SPREAD: the largest difference in the final T, fitness and rmse between the model run with numpy.sum and with math.fsum
sums, over the two pairs: 2.13e-16 measured (the tiles; 1.35e-16 on the 5 k pair), 2.2e-16 recorded -- the counterpart of
ICP_CPU_SPREAD (tests/test_icp_model.py): the GPU tests allow 100 times it.

The condition on the inputs: at every stop decision of both runs of both pairs each |change| is below 0.1 x or above 10 x its
criterion, so no rounding difference between two correct implementations changes the iteration count.  Measured: the 5 k pair
stops after 4 iterations, its rmse changes 2.8e-2, 1.1e-3, 6.6e-6, 3.5e-17 (fitness: 0 throughout); the tiles after 7, the
decisive changes 2.8e-5 / 2.3e-6, 0 / 1.1e-6, 0 / 7.8e-10.  An input that violates it is replaced (another seed), the condition stays."""
import os

import numpy as np
import pytest

import icp_model as im
import icp_plane_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANE_MOTION_ERROR_MEASURED = 3.2e-9
PLANE_CPU_SPREAD = 2.2e-16
CRITERIA = (1e-7, 1e-7, 60)
MAXD = 0.05
#: name -> (the pair, whether the model takes its candidates from a KD-tree, the normals' radius and max_nn)
PAIRS = {"5k": (im.test_pair_5k, False, 0.05, 30), "tiles": (pm.test_pair_tiles_plane, True, 0.02, 30)}
NEW_SYMBOLS = ("cwipc_hip_icp_plane_sums", "cwipc_hip_icp_point2plane")


def decisions_are_clear(decisions, criteria=CRITERIA):
    for k, changes in enumerate(decisions):
        for change, criterion in zip(changes, criteria[:2]):
            assert change < 0.1 * criterion or change > 10 * criterion, (k, changes)


@pytest.fixture(scope="module")
def runs():
    """name -> (ref, src, T_true, normals, the model's run with numpy.sum, with math.fsum)"""
    out = {}
    for name, (make, tree, radius, max_nn) in PAIRS.items():
        ref, src, T_true = make()
        normals, count = pm.estimate_normals(ref, radius, max_nn)
        print("%s: the median neighbourhood holds %d points" % (name, np.median(count)))
        both = [pm.icp_plane(src, ref, normals, MAXD, None, *CRITERIA, exact=exact, tree=tree) for exact in (False, True)]
        out[name] = (ref, src, T_true, normals, both[0], both[1])
    return out


def test_loop_recovers_a_rigid_motion(runs):
    ref, src, T_true, normals, (T, fitness, rmse, iterations, trail, _), _ = runs["5k"]
    errs = [float(np.abs(Tk - T_true).max()) for Tk in trail]
    idx, d2 = im.correspondences(src, ref, None, MAXD)
    A, _ = pm.system(pm.plane_sums(pm.plane_terms(src, ref, normals, np.eye(4), idx, d2))[1])
    print("point-to-plane model on the 5 k pair: %d iterations, fitness %.6f, rmse %.3e, |T_k - T_true| %s; cond(A) %.3g, det(A) %.3g"
          % (iterations, fitness, rmse, " ".join("%.2e" % e for e in errs), np.linalg.cond(A), np.linalg.det(A)))
    assert iterations == 4 and fitness == 1.0
    assert errs[3] <= 10 * PLANE_MOTION_ERROR_MEASURED and errs[-1] <= 10 * PLANE_MOTION_ERROR_MEASURED


def test_plane_cpu_spread_and_clear_stop_decisions(runs):
    worst = 0.0
    for name, (_, src, _, _, a, b) in runs.items():
        assert a[3] == b[3] and 0 < a[3] < CRITERIA[2]
        for run in (a, b):
            assert len(run[5]) == run[3]
            decisions_are_clear(run[5])
        spread = max(float(np.abs(a[0] - b[0]).max()), abs(a[1] - b[1]), abs(a[2] - b[2]))
        print("plane_cpu_spread, %s, %d source points, %d iterations: %.3e; the stop decisions saw %s"
              % (name, len(src), a[3], spread, ", ".join("%.1e / %.1e" % d for d in a[5])))
        worst = max(worst, spread)
    assert runs["5k"][4][3] == 4 and runs["tiles"][4][3] == 7
    assert 0 < worst <= PLANE_CPU_SPREAD


def test_negated_normals_give_the_same_terms(runs):
    for name, (ref, src, _, normals, a, _) in runs.items():
        T = a[4][1]
        idx, d2 = im.correspondences(src[:3000], ref, T, MAXD, tree=True)
        flipped = normals.copy()
        flipped[::3] = -flipped[::3]
        want = pm.plane_terms(src[:3000], ref, normals, T, idx, d2)
        assert len(want) > 1000 and want.shape[1] == pm.NSUM
        for other in (-normals, flipped):
            assert np.array_equal(pm.plane_terms(src[:3000], ref, other, T, idx, d2), want)


def test_the_solve_keeps_open3ds_rule():
    A = np.diag([1.0, 1.0, 1.0, 1.0, 1.0, 0.999e-6])
    assert pm.solve6(A, np.ones(6)) is None and np.array_equal(pm.motion(None), np.eye(4))
    A[5, 5] = 1.001e-6
    assert np.allclose(pm.solve6(A, np.ones(6)), [-1, -1, -1, -1, -1, -1 / 1.001e-6])
    assert pm.solve6(np.full((6, 6), np.nan), np.ones(6)) is None
    U = pm.motion(np.array([0.1, -0.2, 0.3, 1.0, 2.0, 3.0]))
    assert np.allclose(U[:3, :3] @ U[:3, :3].T, np.eye(3)) and np.array_equal(U[:3, 3], [1.0, 2.0, 3.0])
    assert np.allclose(pm.motion(np.array([0.1, 0, 0, 0, 0, 0]))[:3, :3] @ [0, 1, 0], [0, np.cos(0.1), np.sin(0.1)])   # about x, y towards z


def test_new_symbols_are_exported_and_declared(cwipc):
    from cwipc_util_amd.util import _SIGNATURES
    dll = cwipc.cwipc_util_dll_load()
    header = open(os.path.join(ROOT, "include", "cwipc_util_amd", "hip_ext.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(dll, name) and name in _SIGNATURES and name in cwipc.util.__all__, name
        assert "_CWIPC_UTIL_EXPORT int %s(cwipc_pointcloud *source, cwipc_pointcloud *reference," % name in header, name
    from cwipc_util_amd.registration import RegistrationComputer_ICP_Point2Plane as P
    assert (P.relative_fitness, P.relative_rmse, P.max_iteration, P.normal_radius, P.normal_max_nn) == (1e-7, 1e-7, 60, 0.02, 30)
