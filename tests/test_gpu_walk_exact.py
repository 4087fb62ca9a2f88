"""The three users of the exact grid walk (point_grid.hpp: walk_exact) agree with each other and with brute force.

cwipc_hip_correspondences' d2, cwipc_hip_nn_distance2 at nth = 0 and one unrestricted job of cwipc_hip_nn_distance2_jobs answer the
same question for T = identity: the squared f64 distance to the nearest reference point under max_distance.  They share the walk,
so the same 257 doubles must come back bit for bit, and they are the brute-force value of tests/icp_model.py."""
import ctypes

import numpy as np
import pytest

from conftest import make_cloud
import icp_model as im
from test_gpu_icp import as_points

pytestmark = pytest.mark.gpu

NREF, NSRC = 37, 257
FINITE = 0.3


@pytest.fixture(scope="module")
def clouds():
    """(reference xyz, source xyz): the reference fills a box of half a metre and holds one exact duplicate pair; a good part of the
    source lies outside that box, on every side, and one source point sits on the duplicate pair (a tie at distance 0)."""
    rng = np.random.default_rng(37257)
    ref = rng.uniform(0.0, 0.5, (NREF, 3)).astype(np.float32)
    ref[NREF - 1] = ref[5]
    src = rng.uniform(-0.4, 0.9, (NSRC, 3)).astype(np.float32)
    src[100] = ref[5]
    inside = ((src >= ref.min(axis=0)) & (src <= ref.max(axis=0))).all(axis=1)
    assert 10 < inside.sum() < NSRC - 100
    return ref, src


@pytest.mark.parametrize("max_distance", [np.inf, FINITE], ids=["inf", "finite"])
def test_three_searches_one_answer(gpu, clouds, max_distance):
    ref_xyz, src_xyz = clouds
    ref, src = make_cloud(gpu, as_points(ref_xyz)), make_cloud(gpu, as_points(src_xyz))
    dll = gpu.cwipc_util_dll_load()

    idx, d2_icp = gpu.cwipc_hip_correspondences(src, ref, None, max_distance)

    d2_nn = np.full(NSRC, -1.0)
    assert dll.cwipc_hip_nn_distance2(src.as_cwipc_p(), ref.as_cwipc_p(), 0, float(max_distance), d2_nn.ctypes.data, NSRC) == 0

    table = (gpu.NNJob * 1)(gpu.NNJob(nth=0, max_distance=max_distance))
    d2_job = np.full((1, NSRC), -1.0)
    assert dll.cwipc_hip_nn_distance2_jobs(src.as_cwipc_p(), ref.as_cwipc_p(), ctypes.addressof(table), 1, d2_job.ctypes.data, NSRC) == 0

    want_idx, want = im.correspondences(src_xyz, ref_xyz, None, max_distance)
    assert want.shape == (NSRC,) and want[100] == 0.0 and want_idx[100] == 5
    if np.isfinite(max_distance):
        assert np.isposinf(want).any() and np.isfinite(want).any()   # the bound cuts through this source
    else:
        assert np.isfinite(want).all()
    assert d2_icp.tobytes() == want.tobytes()
    assert d2_nn.tobytes() == want.tobytes()
    assert d2_job[0].tobytes() == want.tobytes()
    assert np.array_equal(idx, want_idx)
    src.free()
    ref.free()
