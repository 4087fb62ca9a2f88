"""The numpy model of point-to-point ICP (tests/icp_model.py) checked on the CPU: its search against scipy's KD-tree, its loop
against a known motion, and how far two f64 summation orders move its result.  No GPU, no library symbol.

open3d is not available, so no reference output exists: the model restates the published algorithm (nearest neighbour under a
strict bound, Eigen's umeyama without scaling, open3d's registration_icp loop), and the GPU tests (tests/test_gpu_icp.py) compare
the library with it.

ICP_MOTION_ERROR_MEASURED: the largest entry of |T_model - T_true| on the 5 k pair (2 degrees, 1 cm, coordinates rounded to
float32, a permuted copy, max distance 5 cm), measured here: 1.12e-9 -- what float32 rounding of the moved copy (6e-8 per
coordinate, averaged over 5000 points) leaves.  The bar is ten times that; the test is about the algorithm, not about rounding.

ICP_CPU_SPREAD: the largest difference in the final T, fitness and rmse between the model run with numpy.sum and with math.fsum
sums, over the two test pairs: 2.6e-15 measured (the tiles; 1.4e-15 on the 5 k pair), 3e-15 recorded -- the ICP counterpart of
kde_cpu_spread (tests/test_analyze_oracle.py, tests/test_gpu_analyze.py): the GPU tests allow 100 times it."""
import numpy as np
import pytest
from scipy.spatial import cKDTree

import icp_model as im

ICP_MOTION_ERROR_MEASURED = 1.12e-9
ICP_CPU_SPREAD = 3e-15


@pytest.fixture(scope="module")
def pair5k():
    return im.test_pair_5k()


@pytest.mark.parametrize("bound", [np.inf, 0.05, 0.004])
def test_distances_and_counts_equal_scipy_at_the_identity(pair5k, bound):
    ref, src, _ = pair5k
    idx, d2 = im.correspondences(src, ref, None, bound)
    dist, j = cKDTree(ref.astype(np.float64)).query(src.astype(np.float64), distance_upper_bound=bound)
    assert np.array_equal(np.sqrt(d2), dist)
    hit = np.isfinite(dist)
    assert np.array_equal(idx[hit], j[hit].astype(np.uint32))   # (no ties in this cloud)
    assert np.all(idx[~hit] == im.NONE)
    if np.isfinite(bound) and bound < 0.01:
        assert 0 < hit.sum() < len(src)


@pytest.mark.parametrize("bound", [np.inf, 0.05, 0.004])
def test_count_of_matches_equals_scipy(pair5k, bound):
    ref, src, _ = pair5k
    _, d2 = im.correspondences(src, ref, None, bound)
    dist, _ = cKDTree(ref.astype(np.float64)).query(src.astype(np.float64), distance_upper_bound=bound)
    assert np.isfinite(d2).sum() == np.isfinite(dist).sum()


def test_tree_candidates_give_the_brute_force_answer(pair5k):
    ref, src, T = pair5k
    lattice = (np.stack(np.meshgrid(*[np.arange(6)] * 3, indexing="ij"), axis=-1).reshape(-1, 3) / 64).astype(np.float32)
    mids = (lattice[:100] + np.float32(1 / 128)).astype(np.float32)                 # cell midpoints: eight equally distant points
    for s, r, Tq, bound in ((src, ref, T, 0.05), (src, ref, im.rigid(1, (0, 1, 0), (0.01, 0, 0)), 0.02), (src, ref, None, np.inf),
                            (mids, lattice, None, np.inf), (mids, np.concatenate([lattice, lattice]), None, 0.02)):
        a, b = im.correspondences(s, r, Tq, bound), im.correspondences(s, r, Tq, bound, tree=True)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_loop_recovers_a_rigid_motion(pair5k):
    ref, src, T = pair5k
    got, fitness, rmse, iterations, _ = im.icp(src, ref, 0.05, None, 1e-3, 1e-6, 30)
    err = float(np.abs(got - T).max())
    print("ICP model on the 5 k pair: %d iterations, fitness %.6f, rmse %.3e, largest |T - T_true| %.3e" % (iterations, fitness, rmse, err))
    assert 0 < iterations < 30 and fitness == 1.0
    assert err <= 10 * ICP_MOTION_ERROR_MEASURED


def test_icp_cpu_spread(pair5k):
    worst = 0.0
    for (ref, src, _), tree in ((pair5k, False), (im.test_pair_tiles(), True)):
        a = im.icp(src, ref, 0.05, None, 1e-3, 1e-6, 30, exact=False, tree=tree)
        b = im.icp(src, ref, 0.05, None, 1e-3, 1e-6, 30, exact=True, tree=tree)
        assert a[3] == b[3]
        spread = max(float(np.abs(a[0] - b[0]).max()), abs(a[1] - b[1]), abs(a[2] - b[2]))
        print("icp_cpu_spread, %d source points, %d iterations: %.3e" % (len(src), a[3], spread))
        worst = max(worst, spread)
    assert 0 < worst <= ICP_CPU_SPREAD
