"""Point-to-point ICP on the GPU (kernels_icp.hip, rigid_fit.hpp, registration/fine.py, OverlapAnalyzer) against the numpy model
of its contracts (tests/icp_model.py, checked on the CPU by tests/test_icp_model.py).  open3d is not available: the model restates
the published algorithm, nothing here is compared with open3d's output.

Bars:
  * correspondences: idx and dist2 numpy.array_equal with the model (first minimum = smallest index, strict bound) -- for clouds
    of 20 k points and more the model takes its candidates from a KD-tree and decides among them by the stated arithmetic
    (icp_model._with_tree; test_icp_model.py checks that against the brute force);
  * ties: on lattice clouds (spacing 1/64, queries at edge, face and cell midpoints: 2, 4, 8 equidistant points) idx is the
    smallest index, for duplicated and permuted references too;
  * sums: n exact; on lattice clouds (every product and sum exact in f64) equal to numpy's; on jittered clouds each sum within
    (n + 3) * 2^-53 * sum |term| of math.fsum over the model's terms -- the worst case of any summation order plus the terms' own
    roundings: derived, not measured;
  * the loop: at each of the model's iterates the library's idx equals the model's and its sums are within the bound above; the
    library's own loop ends after the model's number of iterations with T, fitness and rmse within 100 x ICP_CPU_SPREAD (3e-15,
    tests/test_icp_model.py) of the model's -- the factor of the KDE tests (test_gpu_analyze.py);
  * OverlapAnalyzer: fitness equals scipy's count / n, rmse within n * 2^-53 (relative) of the fsum value."""
import math
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from conftest import make_cloud
import icp_model as im
from test_icp_model import ICP_CPU_SPREAD

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
CRITERIA = (1e-3, 1e-6, 30)
MAXD = 0.05


def as_points(xyz, tile=1):
    from cwipc_util_amd import cwipc_point_numpy_dtype
    xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    pts = np.zeros(len(xyz), dtype=cwipc_point_numpy_dtype)
    if len(xyz):
        pts["x"], pts["y"], pts["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    pts["tile"] = tile
    return pts


def cloud(gpu, xyz, tile=1):
    return make_cloud(gpu, as_points(xyz, tile))


SMALL_T = im.rigid(1.5, (0.2, 1.0, -0.3), (0.004, -0.003, 0.002))
FAR_T = im.rigid(0.0, (0, 1, 0), (10.0, -7.0, 5.0))
TRANSFORMS = {"identity": None, "small": SMALL_T, "far": FAR_T}


@pytest.fixture(scope="module")
def pairs():
    """The loop's two pairs with the model's runs on them (numpy sums), computed once."""
    out = {}
    for name, (ref, src, T), tree in (("5k", im.test_pair_5k(), False), ("tiles", im.test_pair_tiles(), True)):
        out[name] = (ref, src, tree, im.icp(src, ref, MAXD, None, *CRITERIA, tree=tree))
    return out


def sums_within_bound(got_n, got, terms, label):
    n, want = im.sums(terms, exact=True)
    assert got_n == n, (label, got_n, n)
    bound = (n + 3) * U * np.abs(terms).sum(axis=0) if n else np.zeros(16)
    err = np.abs(got - want)
    print("%s: n %d, largest error over bound %.3f" % (label, n, float(np.max(err / np.maximum(bound, 1e-300))) if n else 0.0))
    assert np.all(err <= bound), (label, err, bound)


# ---------------------------------------------------------------------------
# correspondences
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nref", [1, 2, 37, 5000])
def test_correspondences_equal_the_model(gpu, nref):
    rng = np.random.default_rng(100 + nref)
    ref_xyz = im.surface(rng, nref)
    src_all = im.surface(rng, 1000)
    ref = cloud(gpu, ref_xyz)
    for nsrc in (1, 63, 64, 65, 127, 128, 129, 1000):
        src_xyz = src_all[:nsrc]
        src = cloud(gpu, src_xyz)
        for tname, T in TRANSFORMS.items():
            for maxd in (np.inf, 0.05, 1e-7):
                idx, d2 = gpu.cwipc_hip_correspondences(src, ref, T, maxd)
                widx, wd2 = im.correspondences(src_xyz, ref_xyz, T, maxd)
                assert idx.dtype == np.uint32 and d2.dtype == np.float64 and idx.shape == (nsrc,)
                assert np.array_equal(idx, widx) and np.array_equal(d2, wd2), (nref, nsrc, tname, maxd)
                if maxd == 1e-7 or (tname == "far" and np.isfinite(maxd)):
                    assert np.all(idx == im.NONE) and np.all(np.isposinf(d2))
                if maxd == np.inf:
                    assert np.all(idx != im.NONE)
        src.free()
    ref.free()


_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import torch  # noqa: F401  (as the test session: torch's HIP runtime first)
import cwipc_util_amd as cw
from conftest import make_cloud
cw.cwipc_hip_set_device(0)
d = np.load(sys.argv[2])
a, b = make_cloud(cw, d["a"]), make_cloud(cw, d["b"])
out = {}
for name in ("identity", "small", "far"):
    T = None if name == "identity" else d["T_" + name]
    for bound, maxd in (("inf", np.inf), ("cut", 0.05)):
        out["idx_%s_%s" % (name, bound)], out["d2_%s_%s" % (name, bound)] = cw.cwipc_hip_correspondences(a, b, T, maxd)
n, s = cw.cwipc_hip_icp_sums(a, b, d["T_small"], 0.05, d["cp"], d["cq"])
out["n"], out["sums"] = np.array([n]), s
T, fit, rmse, it = cw.cwipc_hip_icp_point2point(a, b, 0.05, None, 1e-3, 1e-6, 5)
out["icp_T"], out["icp"] = T, np.array([fit, rmse, it])
np.savez(sys.argv[3], **out)
"""


# the library's three grid flows, each forced where the size alone would not take it: small clouds, the dense layout, the sparse one
@pytest.mark.parametrize("nref,env", [(20000, {}), (30000, {"CWIPC_SOR_SMALL_CELLS": "0"}), (40000, {"CWIPC_SOR_SPARSE": "1"})])
def test_each_grid_flow(gpu, nref, env, tmp_path):
    rng = np.random.default_rng(nref)
    b = im.surface(rng, nref)
    a = im.surface(rng, nref // 2 + 77)
    cp, cq = im.centroid(a), im.centroid(b)
    inp, out = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(inp, a=as_points(a), b=as_points(b), T_small=SMALL_T, T_far=FAR_T, cp=cp, cq=cq)
    subprocess.run([sys.executable, "-c", _CHILD, ROOT, inp, out], check=True, timeout=600, env=dict(os.environ, **env))
    got = np.load(out)
    for name, T in TRANSFORMS.items():
        for bound, maxd in (("inf", np.inf), ("cut", 0.05)):
            widx, wd2 = im.correspondences(a, b, T, maxd, tree=True)
            assert np.array_equal(got["idx_%s_%s" % (name, bound)], widx), (nref, env, name, bound)
            assert np.array_equal(got["d2_%s_%s" % (name, bound)], wd2), (nref, env, name, bound)
    widx, wd2 = im.correspondences(a, b, SMALL_T, 0.05, tree=True)
    sums_within_bound(int(got["n"][0]), got["sums"], im.sum_terms(a, b, SMALL_T, widx, wd2, cp, cq), "flow %s" % env)
    want = im.icp(a, b, 0.05, None, 1e-3, 1e-6, 5, tree=True)
    assert int(got["icp"][2]) == want[3]
    assert np.abs(got["icp_T"] - want[0]).max() <= 100 * ICP_CPU_SPREAD
    assert abs(got["icp"][0] - want[1]) <= 100 * ICP_CPU_SPREAD and abs(got["icp"][1] - want[2]) <= 100 * ICP_CPU_SPREAD


# ---------------------------------------------------------------------------
# ties
# ---------------------------------------------------------------------------
def lattice(side=16):
    g = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    return (g / 64.0 + np.array([1.0, 0.5, -1.0])).astype(np.float32)


def midpoints(lat, side=16):
    """{ties: queries}: edge (2), face (4) and cell (8) midpoints of the lattice's inner cells."""
    g = lat.reshape(side, side, side, 3)[:-1, :-1, :-1].reshape(-1, 3)
    h = np.float32(1 / 128)
    return {2: g + np.array([h, 0, 0], dtype=np.float32), 4: g + np.array([h, h, 0], dtype=np.float32), 8: g + np.array([h, h, h], dtype=np.float32),
            "2z": g + np.array([0, 0, h], dtype=np.float32), "4yz": g + np.array([0, h, h], dtype=np.float32)}


def test_ties_go_to_the_smallest_index(gpu):
    lat = lattice()
    rng = np.random.default_rng(5)
    perm = rng.permutation(len(lat))
    refs = {"lattice": lat, "duplicated": np.concatenate([lat, lat]), "permuted": lat[perm], "duplicated, permuted": np.concatenate([lat, lat])[rng.permutation(2 * len(lat))]}
    for rname, ref_xyz in refs.items():
        ref = cloud(gpu, ref_xyz)
        for ties, q in midpoints(lat).items():
            q = q.astype(np.float32)
            src = cloud(gpu, q)
            for maxd in (np.inf, 0.05):
                idx, d2 = gpu.cwipc_hip_correspondences(src, ref, None, maxd)
                widx, wd2 = im.correspondences(q, ref_xyz, None, maxd)
                assert np.array_equal(d2, wd2) and np.array_equal(idx, widx), (rname, ties, maxd, int(np.sum(idx != widx)))
            # the model's answer IS the smallest index among as many equals as the construction says
            dd = ((q[:50, None, :].astype(np.float64) - ref_xyz[None].astype(np.float64)) ** 2).sum(axis=2)
            equal = dd == dd.min(axis=1, keepdims=True)
            want_ties = int(str(ties)[0]) * (2 if "duplicated" in rname else 1)
            assert np.all(equal.sum(axis=1) == want_ties)
            assert np.array_equal(idx[:50], np.argmax(equal, axis=1).astype(np.uint32))
            src.free()
        ref.free()
    # a permuted reference gives the permuted answer: the same points, under their new numbers
    src = cloud(gpu, midpoints(lat)[8])
    a, _ = gpu.cwipc_hip_correspondences(src, cloud(gpu, lat), None, np.inf)
    b, _ = gpu.cwipc_hip_correspondences(src, cloud(gpu, lat[perm]), None, np.inf)
    inverse = np.argsort(perm)   # the new number of every lattice point
    for i in range(0, len(a), 97):
        near = np.flatnonzero(((lat.astype(np.float64) - midpoints(lat)[8][i].astype(np.float64)) ** 2).sum(axis=1) == 3 / 128 ** 2)
        assert len(near) == 8 and a[i] == near.min() and b[i] == inverse[near].min()


# ---------------------------------------------------------------------------
# sums
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nsrc", [16875, 1024 * 1024 + 1])
def test_sums_are_exact_on_lattice_clouds(gpu, nsrc):
    """16875: every midpoint once.  1024 * 1024 + 1: the first source count whose chunk doubles (ICP_CHUNK << 1 in IcpWork::alloc), the
    midpoints over and over -- a source point's correspondence and terms do not depend on the others, so the model's answer for
    the midpoints is repeated in the same way; every sum is still exact (integers in units of 2^-14 far below 2^53)."""
    lat = lattice()
    once = np.concatenate([v for v in midpoints(lat).values()]).astype(np.float32)
    assert len(once) == 16875
    q = np.resize(once, (nsrc, 3))
    T = im.rigid(0.0, (0, 1, 0), (2 / 64, -1 / 64, 3 / 64))
    cp, cq = np.array([1.125, 0.625, -0.875]), np.array([1.0 + 7 / 64, 0.5 + 9 / 64, -1.0 + 5 / 64])
    src, ref = cloud(gpu, q), cloud(gpu, lat)
    for maxd in (np.inf, 1 / 64):
        n, s = gpu.cwipc_hip_icp_sums(src, ref, T, maxd, cp, cq)
        idx, d2 = im.correspondences(once, lat, T, maxd)
        idx, d2 = np.resize(idx, nsrc), np.resize(d2, nsrc)
        terms = im.sum_terms(q, lat, T, idx, d2, cp, cq)
        wn, ws = im.sums(terms, exact=True)
        assert np.array_equal(ws, terms.sum(axis=0))   # (exact: every order gives this)
        assert n == wn and 0 < n and np.array_equal(s, ws), (maxd, n, wn)
        if np.isfinite(maxd):
            assert n < len(q)
    src.free()
    ref.free()


@pytest.mark.parametrize("nsrc", [1, 1000, 1024, 1025, 5000, 36000])
def test_sums_on_jittered_clouds(gpu, nsrc):
    rng = np.random.default_rng(nsrc)
    ref_xyz, src_xyz = im.surface(rng, 5000), im.surface(rng, nsrc)
    src, ref = cloud(gpu, src_xyz), cloud(gpu, ref_xyz)
    cq = im.centroid(ref_xyz)
    for T, maxd in ((np.eye(4), np.inf), (SMALL_T, 0.01), (SMALL_T, 1e-7)):
        cp = ((T[:3, 0] * cq[0] + T[:3, 1] * cq[1]) + T[:3, 2] * cq[2]) + T[:3, 3]
        n, s = gpu.cwipc_hip_icp_sums(src, ref, T, maxd, cp, cq)
        idx, d2 = im.correspondences(src_xyz, ref_xyz, T, maxd, tree=nsrc >= 5000)
        sums_within_bound(n, s, im.sum_terms(src_xyz, ref_xyz, T, idx, d2, cp, cq), "jittered %d, max %g" % (nsrc, maxd))
        n0, s0 = gpu.cwipc_hip_icp_sums(src, ref, T, maxd)   # no pivots
        sums_within_bound(n0, s0, im.sum_terms(src_xyz, ref_xyz, T, idx, d2, np.zeros(3), np.zeros(3)), "no pivots")


# ---------------------------------------------------------------------------
# the loop
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["5k", "tiles"])
def test_loop_in_lockstep_with_the_model(gpu, pairs, name):
    ref_xyz, src_xyz, tree, (wT, wfit, wrmse, wit, trail) = pairs[name]
    src, ref = cloud(gpu, src_xyz), cloud(gpu, ref_xyz)
    cp0, cq = im.centroid(src_xyz), im.centroid(ref_xyz)
    assert len(trail) == wit + 1
    for k, T in enumerate(trail):
        idx, d2 = gpu.cwipc_hip_correspondences(src, ref, T, MAXD)
        widx, wd2 = im.correspondences(src_xyz, ref_xyz, T, MAXD, tree=tree)
        assert np.array_equal(idx, widx) and np.array_equal(d2, wd2), (name, k)
        cp = ((T[:3, 0] * cp0[0] + T[:3, 1] * cp0[1]) + T[:3, 2] * cp0[2]) + T[:3, 3]
        n, s = gpu.cwipc_hip_icp_sums(src, ref, T, MAXD, cp, cq)
        sums_within_bound(n, s, im.sum_terms(src_xyz, ref_xyz, T, widx, wd2, cp, cq), "%s, iterate %d" % (name, k))
    T, fit, rmse, it = gpu.cwipc_hip_icp_point2point(src, ref, MAXD, None, *CRITERIA)
    print("%s: %d iterations (model %d); |T - T_model| %.3e, fitness %.3e, rmse %.3e apart; bar %.1e"
          % (name, it, wit, np.abs(T - wT).max(), abs(fit - wfit), abs(rmse - wrmse), 100 * ICP_CPU_SPREAD))
    assert it == wit
    assert np.abs(T - wT).max() <= 100 * ICP_CPU_SPREAD
    assert abs(fit - wfit) <= 100 * ICP_CPU_SPREAD and abs(rmse - wrmse) <= 100 * ICP_CPU_SPREAD


# ---------------------------------------------------------------------------
# the classes
# ---------------------------------------------------------------------------
def test_overlap_analyzer_and_the_aligner(gpu, pairs):
    from scipy.spatial import cKDTree
    from cwipc_util_amd.registration import OverlapAnalyzer, RegistrationAnalyzer, RegistrationComputer, RegistrationComputer_ICP_Point2Point
    from cwipc_util_amd.registration.fine import ALL_FINE_ALIGNMENT_ALGORITHMS, DEFAULT_FINE_ALIGNMENT_ALGORITHM
    assert ALL_FINE_ALIGNMENT_ALGORITHMS == [RegistrationComputer, RegistrationComputer_ICP_Point2Point]
    assert DEFAULT_FINE_ALIGNMENT_ALGORITHM is RegistrationComputer_ICP_Point2Point
    ref_xyz, src_xyz, _, _ = pairs["tiles"]
    other = im.surface(np.random.default_rng(1), 3000)
    src_pts = np.concatenate([as_points(src_xyz, 1), as_points(other, 2)])
    ref_pts = np.concatenate([as_points(ref_xyz, 4), as_points(other, 2)])
    src, ref = make_cloud(gpu, src_pts), make_cloud(gpu, ref_pts)
    for corr in (0.02, np.inf):
        a = OverlapAnalyzer()
        a.set_source_pointcloud(src, 1)
        a.set_reference_pointcloud(ref, 4)
        a.set_correspondence(corr)
        assert a.run()
        r = a.get_results()
        dist, _ = cKDTree(ref_xyz.astype(np.float64)).query(src_xyz.astype(np.float64), distance_upper_bound=corr)
        hit = np.isfinite(dist)
        n = int(hit.sum())
        assert r.fitness == n / len(src_xyz) and 0 < n
        _, wd2 = im.correspondences(src_xyz, ref_xyz, None, corr, tree=True)
        assert np.array_equal(np.isfinite(wd2), hit)
        want = math.sqrt(math.fsum(wd2[hit]) / n)
        assert abs(r.rmse - want) <= n * U * want
        assert (r.sourcePointCount, r.referencePointCount, r.tilemask, r.referenceTilemask) == (len(src_xyz), len(ref_xyz), 1, 4)

    def mean_distance(pc):
        an = RegistrationAnalyzer()
        an.set_source_pointcloud(pc, 1)
        an.set_reference_pointcloud(ref, 4)
        an.set_max_correspondence_distance(MAXD)
        an.set_correspondence_measure("mean")
        assert an.run()
        return an.get_results().mean

    base = RegistrationComputer()
    base.set_source_pointcloud(src, 1)
    base.set_reference_pointcloud(ref, 4)
    assert base.run() and np.array_equal(base.get_result_transformation(), np.eye(4))
    icp = RegistrationComputer_ICP_Point2Point()
    icp.set_source_pointcloud(src, 1)
    icp.set_reference_pointcloud(ref, 4)
    icp.set_correspondence(MAXD)
    assert icp.run()
    before = mean_distance(src)
    moved = icp.get_result_pointcloud()
    after = mean_distance(moved)
    print("RegistrationAnalyzer mean distance: %.5f before, %.5f after %d iterations" % (before, after, icp.iterations))
    assert after < before and moved.count() == len(src_xyz)
    assert icp.get_result_pointcloud_full().count() == len(src_xyz) + len(ref_xyz)
    # correspondence 0: half the distance between the centroids, height left out
    icp.set_correspondence(0)
    icp.apply_source_filter(lambda pc: gpu.cwipc_crop(pc, (-9, 9, 0.2, 9, -9, 9)))
    assert icp.run()
    cs = np.array(gpu.cwipc_center(icp.get_filtered_source_pointcloud()), dtype=np.float32)
    cr = np.array(gpu.cwipc_center(icp.get_filtered_reference_pointcloud()), dtype=np.float32)
    cs[1] = cr[1] = 0
    assert icp.correspondence == float(np.linalg.norm(cs - cr)) / 2 and icp.correspondence > 0


# ---------------------------------------------------------------------------
# determinism, edges, errors
# ---------------------------------------------------------------------------
def test_same_bytes_on_every_call_and_thread(gpu, pairs):
    ref_xyz, src_xyz, _, _ = pairs["5k"]
    src, ref = cloud(gpu, src_xyz), cloud(gpu, ref_xyz)

    def everything():
        idx, d2 = gpu.cwipc_hip_correspondences(src, ref, SMALL_T, MAXD)
        n, s = gpu.cwipc_hip_icp_sums(src, ref, SMALL_T, MAXD, (1.2, 0.8, -0.8), (1.2, 0.8, -0.8))
        T, fit, rmse, it = gpu.cwipc_hip_icp_point2point(src, ref, MAXD, None, *CRITERIA)
        return idx.tobytes() + d2.tobytes() + np.array([n]).tobytes() + s.tobytes() + T.tobytes() + np.array([fit, rmse, it]).tobytes()

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
    ref_xyz, src_xyz, _, _ = pairs["5k"]
    src_xyz = src_xyz[:700]
    src, ref, empty = cloud(gpu, src_xyz), cloud(gpu, ref_xyz), cloud(gpu, np.zeros((0, 3)))
    for pc in (src, ref):
        gpu.cwipc_hip_upload(pc, drop_host_copy=True)
    before = gpu.cwipc_dangling_allocations(False)
    # an empty source, an empty reference
    idx, d2 = gpu.cwipc_hip_correspondences(empty, ref)
    assert idx.shape == (0,) and d2.shape == (0,)
    idx, d2 = gpu.cwipc_hip_correspondences(src, empty)
    assert np.all(idx == im.NONE) and np.all(np.isposinf(d2)) and idx.shape == (700,)
    for a, b in ((empty, ref), (src, empty), (empty, empty)):
        n, s = gpu.cwipc_hip_icp_sums(a, b, SMALL_T, MAXD)
        assert n == 0 and np.array_equal(s, np.zeros(16))
        T, fit, rmse, it = gpu.cwipc_hip_icp_point2point(a, b, MAXD, SMALL_T)
        assert np.array_equal(T, SMALL_T) and (fit, rmse, it) == (0.0, 0.0, 0)
    # no correspondence at all: init comes back
    T, fit, rmse, it = gpu.cwipc_hip_icp_point2point(src, ref, 1e-7, FAR_T)
    assert np.array_equal(T, FAR_T) and (fit, rmse, it) == (0.0, 0.0, 0)
    # init given; max_iteration 0 evaluates at init
    for init in (None, SMALL_T):
        want = im.icp(src_xyz, ref_xyz, MAXD, init, *CRITERIA)
        T, fit, rmse, it = gpu.cwipc_hip_icp_point2point(src, ref, MAXD, init, *CRITERIA)
        assert it == want[3] and np.abs(T - want[0]).max() <= 100 * ICP_CPU_SPREAD
        assert abs(fit - want[1]) <= 100 * ICP_CPU_SPREAD and abs(rmse - want[2]) <= 100 * ICP_CPU_SPREAD
        want = im.icp(src_xyz, ref_xyz, MAXD, init, 1e-3, 1e-6, 0)
        T, fit, rmse, it = gpu.cwipc_hip_icp_point2point(src, ref, MAXD, init, 1e-3, 1e-6, 0)
        assert it == 0 and np.array_equal(T, np.eye(4) if init is None else init) and fit == want[1]
        assert abs(rmse - want[2]) <= 100 * ICP_CPU_SPREAD and fit > 0
    # NaN and inf points in either cloud
    bad_src, bad_ref = src_xyz.copy(), ref_xyz.copy()
    bad_src[[3, 64, 699], [0, 1, 2]] = [np.nan, np.inf, -np.inf]
    bad_ref[[0, 100, 4999], [2, 0, 1]] = [np.nan, -np.inf, np.nan]
    bs, br = cloud(gpu, bad_src), cloud(gpu, bad_ref)
    for T in (None, SMALL_T):
        idx, d2 = gpu.cwipc_hip_correspondences(bs, br, T, np.inf)
        widx, wd2 = im.correspondences(bad_src, bad_ref, T, np.inf)
        assert np.array_equal(idx, widx) and np.array_equal(d2, wd2)
        assert np.all(idx[[3, 64, 699]] == im.NONE) and not np.isin(idx, [0, 100, 4999]).any() and (idx != im.NONE).sum() == 697
    want = im.icp(bad_src, bad_ref, MAXD, None, *CRITERIA)
    T, fit, rmse, it = gpu.cwipc_hip_icp_point2point(bs, br, MAXD, None, *CRITERIA)
    assert it == want[3] and np.abs(T - want[0]).max() <= 100 * ICP_CPU_SPREAD and abs(fit - want[1]) <= 100 * ICP_CPU_SPREAD
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
        p = pc.as_cwipc_p()
        idx, d2 = np.full(300, 7, dtype=np.uint32), np.full(300, -1.0)
        inf, nan = float("inf"), float("nan")
        good = np.eye(4)
        bad = np.eye(4)
        bad[1, 3] = nan
        worse = np.eye(4)
        worse[0, 0] = inf

        def failed(call):
            n = len(logged)
            rc = call()
            return rc == -1 and len(logged) > n

        def corr(s, r, T, maxd, cap=300):
            return lambda: dll.cwipc_hip_correspondences(s, r, None if T is None else T.ctypes.data, maxd, idx.ctypes.data, d2.ctypes.data, cap)

        for args in ((None, p, None, inf), (p, None, None, inf), (p, p, None, nan), (p, p, None, 0.0), (p, p, None, -1.0), (p, p, None, inf, 299),
                     (p, p, bad, inf), (p, p, worse, inf)):
            assert failed(corr(*args)), args
        assert np.all(idx == 7) and np.all(d2 == -1.0)                                  # nothing was written
        n, s = np.zeros(1, dtype=np.uint64), np.zeros(16)
        T_out, f3 = np.zeros(16), np.zeros(3)
        it = np.zeros(1, dtype=np.int32)
        for s_, r_, T, maxd in ((None, p, good, inf), (p, None, good, inf), (p, p, good, nan), (p, p, good, 0.0), (p, p, bad, 1.0), (p, p, worse, 1.0)):
            assert failed(lambda: dll.cwipc_hip_icp_sums(s_, r_, T.ctypes.data, maxd, None, None, n.ctypes.data, s.ctypes.data)), (T, maxd)
            assert failed(lambda: dll.cwipc_hip_icp_point2point(s_, r_, maxd, T.ctypes.data, 1e-3, 1e-6, 30, T_out.ctypes.data, f3.ctypes.data,
                                                               f3.ctypes.data + 8, it.ctypes.data)), (T, maxd)
        assert failed(lambda: dll.cwipc_hip_icp_point2point(p, p, 1.0, None, 1e-3, 1e-6, -1, None, None, None, None))
        bad_pivot = np.array([0.0, nan, 0.0])
        assert failed(lambda: dll.cwipc_hip_icp_sums(p, p, None, 1.0, bad_pivot.ctypes.data, None, n.ctypes.data, s.ctypes.data))
        assert all(level == gpu.CWIPC_LOG_LEVEL_ERROR for level, _ in logged)
        # every optional output may be NULL
        k = len(logged)
        assert dll.cwipc_hip_correspondences(p, p, None, inf, None, None, 300) == 0
        assert dll.cwipc_hip_icp_sums(p, p, None, inf, None, None, None, None) == 0
        assert dll.cwipc_hip_icp_point2point(p, p, 1.0, None, 1e-3, 1e-6, 3, None, None, None, None) == 0
        assert len(logged) == k
        for call in (lambda: gpu.cwipc_hip_correspondences(pc, pc, None, nan), lambda: gpu.cwipc_hip_icp_sums(pc, pc, bad, 1.0),
                     lambda: gpu.cwipc_hip_icp_point2point(pc, pc, 0.0)):
            with pytest.raises(gpu.CwipcError):
                call()
        with pytest.raises(ValueError):
            gpu.cwipc_hip_correspondences(pc, pc, np.eye(3))
        # a cloud against itself: every point is its own correspondence
        own, z = gpu.cwipc_hip_correspondences(pc, pc)
        assert np.array_equal(own, np.arange(300, dtype=np.uint32)) and np.all(z == 0.0)
    finally:
        gpu.cwipc_log_configure(gpu.CWIPC_LOG_LEVEL_WARNING, None)
