"""The direction filter on the GPU (cwipc_hip_direction_filter, cwipc_hip_estimate_normals) against the numpy oracle of
tests/direction_oracle.py.

Bars: neighbourhood sizes equal except at ties at the cutoff or points at the radius; normals within 1e-3 rad of the oracle's
where the relative eigengap is at least 1e-2 (and the orientation is not decided by rounding); the filter's output the oracle's
mask, in input order, with every record's bytes, where the dot product is not within 1e-3 of the threshold.  The points left
out stay under 5 % of each cloud.  The synthetic source's points lie on a lattice, whose equal distances make ties at the
cutoff common: it is jittered by 10 um (which breaks them) where the 5 % bound is checked, and also checked as it is.
"""
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from conftest import make_cloud
import direction_oracle as do

pytestmark = pytest.mark.gpu

ANGLE_TOL = 1e-3
GAP_MIN = 1e-2
ORIENT_MIN = 2e-3    # an angle error of 1e-3 rad cannot flip the orientation of a normal with more margin than this
DOT_MARGIN = 1e-3


def xyz_of(pts):
    return np.column_stack([pts["x"], pts["y"], pts["z"]]).astype(np.float32)


def with_ids(pts, seed=0):
    """The points with rgb = their index (24 bits) and a random tile byte: every output record names its input."""
    out = pts.copy()
    i = np.arange(len(out), dtype=np.uint32)
    out["r"], out["g"], out["b"] = i & 0xff, (i >> 8) & 0xff, (i >> 16) & 0xff
    out["tile"] = np.random.default_rng(seed).integers(0, 256, len(out), dtype=np.uint8)
    return out


def ids_of(pts):
    return pts["r"].astype(np.int64) | (pts["g"].astype(np.int64) << 8) | (pts["b"].astype(np.int64) << 16)


def jittered_synthetic(synth, n, seed=0):
    pts, cs = synth(n)
    pts = pts.copy()
    rng = np.random.default_rng(seed)
    for a in "xyz":
        pts[a] = (pts[a] + rng.uniform(-1e-5, 1e-5, len(pts))).astype(np.float32)
    return pts, cs


def check_normals(xyz, normals, nn, cen, query=None, radius=0.02, max_nn=30, max_left_out=0.05):
    """Compare the GPU's normals / counts (of every point) with the oracle at `query`; returns the oracle's estimate."""
    est = do.estimate(xyz, radius=radius, max_nn=max_nn, query=query)
    q = est["index"]
    if len(xyz):
        assert np.allclose(cen, est["centroid"], rtol=1e-6, atol=1e-6 * np.abs(xyz).max())
    clean = ~est["tie"] & ~est["boundary"]
    assert np.array_equal(nn[q][clean], est["nn"][clean])
    good = clean & (est["gap"] >= GAP_MIN) & (est["orient"] >= ORIENT_MIN)
    cosang = np.clip((normals[q][good].astype(np.float64) * est["normals"][good]).sum(axis=1), -1.0, 1.0)
    ang = np.arccos(cosang)
    assert ang.size == 0 or ang.max() <= ANGLE_TOL, (ang.max(), np.argmax(ang))
    if max_left_out is not None and len(q):
        assert (~good).mean() < max_left_out, (~good).mean()
    return est


def normals_of(gpu, pts, cs=0.0, **kw):
    return gpu.cwipc_hip_estimate_normals(make_cloud(gpu, pts, cs), **kw)


# ---------------------------------------------------------------------------
# normals against the oracle
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("npoints", [36000, 300000])
def test_normals_synthetic(gpu, synth, npoints):
    pts, cs = jittered_synthetic(synth, npoints)
    normals, nn, cen = normals_of(gpu, pts, cs)
    assert normals.shape == (len(pts), 3) and nn.shape == (len(pts),)
    query = None if npoints < 100000 else np.random.default_rng(1).choice(len(pts), 30000, replace=False)
    est = check_normals(xyz_of(pts), normals, nn, cen, query)
    if npoints < 100000:   # a camera tile's density: the radius bounds most neighbourhoods
        assert np.mean(est["nn"] < 30) > 0.5
    else:                  # and at 300 k points max_nn bounds them
        assert np.mean(nn == 30) > 0.95


def test_normals_synthetic_lattice_as_it_is(gpu, synth):
    pts, cs = synth(36000)
    normals, nn, cen = normals_of(gpu, pts, cs)
    check_normals(xyz_of(pts), normals, nn, cen, max_left_out=0.15)


def box_surface(n, side=0.5, seed=0):
    rng = np.random.default_rng(seed)
    face = rng.integers(0, 6, n)
    uv = rng.uniform(0, side, (n, 2))
    xyz = np.empty((n, 3))
    axis, high = face // 2, face % 2
    for a in range(3):
        sel = axis == a
        others = [b for b in range(3) if b != a]
        xyz[sel, a] = high[sel] * side
        xyz[sel, others[0]] = uv[sel, 0]
        xyz[sel, others[1]] = uv[sel, 1]
    return xyz.astype(np.float32)


def sphere_shell(n, r=0.3, seed=0):
    v = np.random.default_rng(seed).normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True) * r).astype(np.float32)


def blobs_and_isolated(seed=0):
    rng = np.random.default_rng(seed)
    parts = [rng.normal(0, 0.004, (3000, 3)) * np.array([1.0, 1.0, 0.2]) + rng.uniform(-1, 1, 3) for _ in range(6)]
    parts.append(rng.uniform(-3, 3, (300, 3)))   # isolated points: fewer than 3 neighbours, the (0, 0, 1) rule
    return np.vstack(parts).astype(np.float32)


def coincident_stacks(seed=0):
    rng = np.random.default_rng(seed)
    at = rng.uniform(-1, 1, (400, 3))
    sizes = rng.integers(1, 8, 400)   # up to 7 copies of a point: zero covariances, under max_nn
    return np.repeat(at, sizes, axis=0).astype(np.float32)


def as_points(xyz):
    from cwipc_util_amd import cwipc_point_numpy_dtype
    pts = np.zeros(len(xyz), dtype=cwipc_point_numpy_dtype)
    if len(xyz):
        pts["x"], pts["y"], pts["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    return with_ids(pts)


@pytest.mark.parametrize("shape", ["box", "sphere", "blobs", "coincident"])
def test_normals_shapes(gpu, shape):
    xyz = {"box": lambda: box_surface(60000), "sphere": lambda: sphere_shell(40000), "blobs": blobs_and_isolated,
           "coincident": coincident_stacks}[shape]()
    normals, nn, cen = normals_of(gpu, as_points(xyz))
    est = check_normals(xyz, normals, nn, cen)
    if shape == "coincident":
        # every neighbourhood is a stack: (0, 0, 1) turned away from the centroid, exactly
        want = np.where((xyz[:, 2].astype(np.float64) < est["centroid"][2])[:, None], [0, 0, -1.0], [0, 0, 1.0])
        assert np.array_equal(normals.astype(np.float64), want)
    if shape == "blobs":
        iso = nn < 3
        assert iso.sum() >= 250
        assert np.all(np.abs(normals[iso][:, 2]) == 1.0) and np.all(normals[iso][:, :2] == 0)


def test_stack_above_max_nn(gpu):
    xyz = np.vstack([np.zeros((40, 3)), [[1.0, 1.0, 1.0]]]).astype(np.float32)
    normals, nn, cen = normals_of(gpu, as_points(xyz))
    assert np.all(nn[:40] >= 30) and nn[40] == 1   # (a tie at the cutoff: every tied point is in)
    assert np.array_equal(normals[:40], np.tile([0, 0, -1.0], (40, 1)).astype(np.float32))


@pytest.mark.parametrize("npoints", [0, 1, 2, 3])
def test_normals_tiny_clouds(gpu, npoints):
    xyz = np.array([[0, 0, 0], [0.01, 0, 0], [0, 0.01, 0.001]], dtype=np.float32)[:npoints]
    normals, nn, cen = normals_of(gpu, as_points(xyz))
    assert len(normals) == npoints and len(nn) == npoints
    if npoints:
        check_normals(xyz, normals, nn, cen, max_left_out=None)
        assert list(nn) == [npoints] * npoints


# ---------------------------------------------------------------------------
# the filter
# ---------------------------------------------------------------------------
def expected_ids(xyz, direction, threshold):
    est = do.estimate(xyz)
    keep, margin = do.direction_mask(est, direction, threshold)
    sure = do.reliable(est, GAP_MIN, ORIENT_MIN) & (margin >= DOT_MARGIN)
    return keep, sure


def check_filter_output(src_pts, out, direction, threshold, ts=4321, cs=0.0):
    got = out.get_numpy_array()
    ids = ids_of(got)
    assert np.all(np.diff(ids) > 0)                                   # input order
    assert got.tobytes() == src_pts[ids].tobytes()                    # every record as it was
    assert out.timestamp() == ts and out.cellsize() == np.float32(cs)
    keep, sure = expected_ids(xyz_of(src_pts), direction, threshold)
    kept = np.zeros(len(src_pts), bool)
    kept[ids] = True
    assert np.array_equal(kept[sure], keep[sure])
    assert (~sure).mean() < 0.05, (~sure).mean()
    return kept


@pytest.mark.parametrize("direction,threshold", [((0, 0, 1), 0.5), ((1, 0.5, 0), 0.0), ((0, -2, 0), -0.3)])
def test_filter_against_oracle(gpu, synth, direction, threshold):
    pts, cs = jittered_synthetic(synth, 36000)
    pts = with_ids(pts)
    out = gpu.cwipc_direction_filter(make_cloud(gpu, pts, cs, 4321), direction, threshold)
    kept = check_filter_output(pts, out, direction, threshold, cs=cs)
    assert 0 < kept.sum() < len(pts)


def test_filter_keeps_all_or_nothing(gpu, synth):
    pts, cs = synth(36000)
    pts = with_ids(pts)
    pc = make_cloud(gpu, pts, cs, 99)
    everything = gpu.cwipc_direction_filter(pc, (0, 1, 0), -1.0)
    assert everything.get_numpy_array().tobytes() == pts.tobytes()
    nothing = gpu.cwipc_direction_filter(pc, (0, 1, 0), 1.01)
    assert nothing.count() == 0 and nothing.timestamp() == 99 and nothing.cellsize() == np.float32(cs)
    assert gpu.cwipc_direction_filter(pc, (0, 0, 0), 0.0).count() == len(pts)
    assert gpu.cwipc_direction_filter(pc, (0, 0, 0), 1e-9).count() == 0


def test_filter_empty_input_and_bad_arguments(gpu):
    from cwipc_util_amd import cwipc_point_numpy_dtype, CwipcError
    empty = make_cloud(gpu, np.zeros(0, dtype=cwipc_point_numpy_dtype), 0.25, 17)
    out = gpu.cwipc_direction_filter(empty, (0, 0, 1), 0.5)
    assert out.count() == 0 and out.timestamp() == 17 and out.cellsize() == np.float32(0.25)
    pc = make_cloud(gpu, as_points(sphere_shell(1000)))
    for kw in (dict(radius=0.0), dict(radius=-1.0), dict(radius=float("inf")), dict(radius=float("nan")), dict(max_nn=0)):
        with pytest.raises(CwipcError):
            gpu.cwipc_direction_filter(pc, (0, 0, 1), 0.5, **kw)
        with pytest.raises(CwipcError):
            gpu.cwipc_hip_estimate_normals(pc, **{"radius": 0.02, "max_nn": 30, **kw})


def test_filter_other_radius_and_max_nn(gpu):
    xyz = sphere_shell(40000)
    pts = as_points(xyz)
    for radius, max_nn in ((0.05, 10), (0.03, 50)):
        normals, nn, cen = normals_of(gpu, pts, radius=radius, max_nn=max_nn)
        check_normals(xyz, normals, nn, cen, radius=radius, max_nn=max_nn)


def test_filter_on_a_pending_downsample(gpu, synth):
    pts, cs = synth(300000)
    pc = make_cloud(gpu, with_ids(pts), cs, 5)
    pending = gpu.cwipc_downsample(pc, 0.008)
    got = gpu.cwipc_direction_filter(pending, (0, 0, 1), 0.2)
    settled = make_cloud(gpu, pending.get_numpy_array(), pending.cellsize(), pending.timestamp())
    want = gpu.cwipc_direction_filter(settled, (0, 0, 1), 0.2)
    assert got.get_numpy_array().tobytes() == want.get_numpy_array().tobytes()
    assert got.timestamp() == pending.timestamp() and got.cellsize() == pending.cellsize()
    assert 0 < got.count() < pending.count()


def test_center(gpu, synth):
    pts, _ = synth(36000)
    c = gpu.cwipc_center(make_cloud(gpu, pts))
    want = xyz_of(pts).mean(axis=0, dtype=np.float64)
    assert np.allclose(c, want, rtol=1e-6, atol=1e-7)


# ---------------------------------------------------------------------------
# large clouds: sampled
# ---------------------------------------------------------------------------
_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import torch  # noqa: F401  (as the test session: torch's HIP runtime first)
import cwipc_util_amd as cw
from oracle import oracle as o
from conftest import make_cloud
o.load()
cw.cwipc_hip_set_device(0)
pts, cs = o.synthetic(int(sys.argv[2]))
normals, nn, cen = cw.cwipc_hip_estimate_normals(make_cloud(cw, pts, cs))
np.savez(sys.argv[3], normals=normals, nn=nn, cen=cen)
"""


@pytest.mark.parametrize("sparse", ["0", "1"])
def test_normals_2m_both_layouts(gpu, synth, sparse, tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "normals.npz")
    subprocess.run([sys.executable, "-c", _CHILD, root, "2000000", out], check=True, timeout=600,
                   env=dict(os.environ, CWIPC_SOR_SPARSE=sparse))
    r = np.load(out)
    pts, _ = synth(2000000)
    q = np.random.default_rng(2).choice(len(pts), 20000, replace=False)
    check_normals(xyz_of(pts), r["normals"], r["nn"], r["cen"], q, max_left_out=0.6)


def test_normals_10m(gpu, synth):
    pts, cs = synth(10000000)
    normals, nn, cen = normals_of(gpu, pts, cs)
    q = np.random.default_rng(3).choice(len(pts), 20000, replace=False)
    check_normals(xyz_of(pts), normals, nn, cen, q, max_left_out=0.6)


# ---------------------------------------------------------------------------
# determinism, threads, the plugin
# ---------------------------------------------------------------------------
def test_two_calls_give_the_same_bits(gpu, synth):
    for n in (36000, 300000):
        pts, cs = synth(n)
        pc = make_cloud(gpu, pts, cs)
        a = gpu.cwipc_hip_estimate_normals(pc)
        b = gpu.cwipc_hip_estimate_normals(pc)
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()


def test_four_threads_as_one(gpu, synth):
    clouds = []
    for i, n in enumerate((36000, 50000, 120000, 300000)):
        pts, cs = synth(n, angle=0.3 * i)
        clouds.append(make_cloud(gpu, with_ids(pts, i), cs))
    dirs = [(0, 0, 1), (1, 0, 0), (0, 1, 1), (-1, 0, 0.5)]
    alone = [gpu.cwipc_direction_filter(pc, d, 0.3).get_numpy_array().tobytes() for pc, d in zip(clouds, dirs)]
    normals_alone = [gpu.cwipc_hip_estimate_normals(pc)[0].tobytes() for pc in clouds]
    got, got_n, errors = [None] * 4, [None] * 4, []

    def work(i):
        try:
            for _ in range(3):
                got[i] = gpu.cwipc_direction_filter(clouds[i], dirs[i], 0.3).get_numpy_array().tobytes()
                got_n[i] = gpu.cwipc_hip_estimate_normals(clouds[i])[0].tobytes()
        except Exception as e:   # pragma: no cover - reported below
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors
    assert got == alone and got_n == normals_alone


def test_plugin_behind_voxelize(gpu, synth):
    from cwipc_util_amd.filters import factory
    pts, cs = synth(300000)
    pc = make_cloud(gpu, with_ids(pts), cs, 8)
    chain = [factory("voxelize(0.01)"), factory("direction(0, 0, 1, 0.5)")]
    out = pc
    for f in chain:
        out = f.filter(out)
    want = gpu.cwipc_direction_filter(gpu.cwipc_downsample(pc, 0.01), (0, 0, 1), 0.5)
    assert out.get_numpy_array().tobytes() == want.get_numpy_array().tobytes()
    assert out.timestamp() == 8 and 0 < out.count()
    assert chain[1].pointcounts == [out.count()] and len(chain[1].times) == 1
