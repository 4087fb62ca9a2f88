"""The direction filter on the GPU (cwipc_hip_direction_filter, cwipc_hip_estimate_normals) against the numpy oracle of
tests/direction_oracle.py -- its exact-neighbourhood estimator (estimate_exact), which restates the kernel's definition of N(p).

Bars:
  nn       equal to the oracle's for EVERY queried point: ties at the cutoff (all in) and points at the radius (out) included.
  normals  where the relative eigengap is at least GAP_MIN and the orientation margin at least ORIENT_MIN: within ANGLE_BAR_Q of the
           normal of the kernel's own fixed-point matrix (only the eigen-solver and the float32 store lie between the two), within
           ANGLE_TOL = 1e-3 rad of the f64 covariance's normal (the outer bar), and on the oracle's side.
           ANGLE_BAR_Q = 2 * (STORE_TERM + EIG_TERM): a unit vector's components round to float32 by at most 2^-25 each, sqrt(3) * 2^-25
           rad; the eigen-solver's term is what tests/test_eigvec_host.py bounds on the host against numpy.linalg.eigh at this gap,
           1.42e-12 rad; twice the sum as headroom for eigh's own error.  1.03e-7 rad.
  mask     the filter's output is the oracle's mask, in input order, with every record's bytes, where the dot product is not within
           DOT_MARGIN of the threshold.
  left out the share of queries that the gap and orientation criteria leave out of the NORMAL checks has a cap per input, a
           condition computed on the CPU from the oracle alone before any GPU run (never from the GPU's output); nn has none.
The synthetic source's points lie on a lattice, whose equal distances make ties at the cutoff common: its neighbourhood sizes are
checked as they are; the normals' caps are met on the lattice jittered by 10 um.
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
STORE_TERM = np.sqrt(3.0) * 2.0 ** -25          # the float32 store of a unit vector
EIG_TERM = 64 * np.finfo(np.float64).eps / GAP_MIN   # the eigen-solver against eigh at this gap (tests/test_eigvec_host.py: EIG_TERM)
ANGLE_BAR_Q = 2.0 * (STORE_TERM + EIG_TERM)
WIDTHS = [1, 2, 3, 4, 31, 32, 33, 34, 64, 65, 127, 128]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# The large lattice clouds' samples: what gap and orientation alone leave out of the normal checks, from the oracle on the CPU for
# those very samples (2 M, seed 2: 0.0150; 10 M, seed 3: 0.0138; all of it the gap), rounded up.  Was 0.6 with the f64 oracle.
LEFT_2M = 0.02
LEFT_10M = 0.02
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


def angle(a, b):
    """The angle between the lines of a and b (up to sign), accurate for small angles."""
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=-1), np.abs((a * b).sum(axis=-1)))


def sample(n, m, seed):
    return np.arange(n) if n <= m else np.sort(np.random.default_rng(seed).choice(n, m, replace=False))


def check_normals(xyz, normals, nn, cen, query=None, radius=0.02, max_nn=30, max_left_out=0.05, what="", est=None, oriented=True):
    """Compare the GPU's normals / counts (of every point) with the exact oracle at `query`; returns the oracle's estimate.
    max_left_out: the cap on the share that gap and orientation leave out of the normal checks (None: nn only is the point of
    the case, normals are checked where they can be).  oriented=False: the caller's centroid is not the kernel's; up to sign."""
    if est is None:
        est = do.estimate_exact(xyz, radius=radius, max_nn=max_nn, query=query)
    q = est["index"]
    if len(xyz) and oriented:
        assert np.allclose(cen, est["centroid"], rtol=1e-6, atol=1e-6 * np.abs(xyz).max())
    bad = np.flatnonzero(nn[q] != est["nn"])
    assert bad.size == 0, (what, radius, max_nn, len(bad), q[bad[:5]], nn[q][bad[:5]], est["nn"][bad[:5]])   # EVERY query
    good = est["gap"] >= GAP_MIN
    if oriented:
        good &= est["orient"] >= ORIENT_MIN
    got = normals[q][good].astype(np.float64)
    ang_q, ang_u = angle(got, est["normals_q"][good]), angle(got, est["normals"][good])
    left = float((~good).mean()) if len(q) else 0.0
    print("direction %s radius %g max_nn %d: %d queries, nn max %d, left out %.4f, angle to quantised %.3g (bar %.3g), to f64 %.3g"
          % (what, radius, max_nn, len(q), est["nn"].max() if len(q) else 0, left, ang_q.max() if ang_q.size else 0.0, ANGLE_BAR_Q,
             ang_u.max() if ang_u.size else 0.0))
    assert ang_q.size == 0 or ang_q.max() <= ANGLE_BAR_Q, (what, ang_q.max(), np.argmax(ang_q))
    assert ang_u.size == 0 or ang_u.max() <= ANGLE_TOL, (what, ang_u.max(), np.argmax(ang_u))
    if oriented:
        assert np.all((got * est["normals_q"][good]).sum(axis=1) > 0), what
    if max_left_out is not None and len(q):
        assert left <= max_left_out, (what, left)
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
    est = check_normals(xyz_of(pts), normals, nn, cen, max_left_out=0.01, what="lattice as it is")   # (the oracle alone: 0.0000)
    assert (est["nn"] > 30).sum() > 100   # ties at the cutoff, all in: checked with the rest


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
    assert np.all(nn[:40] == 40) and nn[40] == 1   # (a tie at the cutoff: every tied point is in)
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
def expected_ids(xyz, direction, threshold, radius=0.02, max_nn=30):
    est = do.estimate_exact(xyz, radius=radius, max_nn=max_nn)
    keep, margin = do.direction_mask(est, direction, threshold, normals="normals_q")
    sure = do.reliable(est, GAP_MIN, ORIENT_MIN) & (margin >= DOT_MARGIN)
    return keep, sure


def check_filter_output(src_pts, out, direction, threshold, ts=4321, cs=0.0, radius=0.02, max_nn=30):
    got = out.get_numpy_array()
    ids = ids_of(got)
    assert np.all(np.diff(ids) > 0)                                   # input order
    assert got.tobytes() == src_pts[ids].tobytes()                    # every record as it was
    assert out.timestamp() == ts and out.cellsize() == np.float32(cs)
    keep, sure = expected_ids(xyz_of(src_pts), direction, threshold, radius, max_nn)
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
if len(sys.argv) > 4:   # jittered_synthetic(synth, n, seed)
    rng = np.random.default_rng(int(sys.argv[4]))
    for a in "xyz":
        pts[a] = (pts[a] + rng.uniform(-1e-5, 1e-5, len(pts))).astype(np.float32)
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
    check_normals(xyz_of(pts), r["normals"], r["nn"], r["cen"], q, max_left_out=LEFT_2M, what="2 M lattice sparse=" + sparse)


@pytest.mark.parametrize("sparse", ["0", "1"])
def test_normals_2m_jittered_both_layouts(gpu, synth, sparse, tmp_path):
    out = str(tmp_path / "normals.npz")
    subprocess.run([sys.executable, "-c", _CHILD, ROOT, "2000000", out, "0"], check=True, timeout=600,
                   env=dict(os.environ, CWIPC_SOR_SPARSE=sparse))
    r = np.load(out)
    pts, _ = jittered_synthetic(synth, 2000000)
    q = np.random.default_rng(2).choice(len(pts), 20000, replace=False)
    check_normals(xyz_of(pts), r["normals"], r["nn"], r["cen"], q, max_left_out=0.05, what="2 M jittered sparse=" + sparse)


def test_normals_10m(gpu, synth):
    pts, cs = synth(10000000)
    normals, nn, cen = normals_of(gpu, pts, cs)
    q = np.random.default_rng(3).choice(len(pts), 20000, replace=False)
    check_normals(xyz_of(pts), normals, nn, cen, q, max_left_out=LEFT_10M, what="10 M lattice")


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


# ---------------------------------------------------------------------------
# list widths x grid flows
# ---------------------------------------------------------------------------
# Caps on the share left out of the normal checks (gap, orientation), by width, for sphere_shell(40000) and box_surface(60000) at
# radius 0.02 to 0.08: conditions, from the f64 oracle alone on 3 000 sampled queries (3: 19.0-19.8 % left out, 4: 3.5-3.6 %,
# every other width at most 0.3 %).  Every other input's cap is 0.05, met by the oracle alone on the CPU before any GPU run.
OTHER_CAP = 0.05   # (at max_nn 3 and 4 a fifth and a twentieth of ANY cloud's points have no eigengap: other inputs get no cap there)


def width_cap(max_nn):
    return {3: 0.25, 4: 0.06}.get(max_nn, 0.01)


def width_radius(max_nn):
    return 0.02 if max_nn <= 34 else 0.04   # about 44 / 178 points of sphere_shell(40000) in reach: max_nn bounds most lists


def tight_blobs(seed=5):
    """400 flat blobs of 150 points, each far smaller than a cell of the census's grid: so many points per occupied cell that the
    small flow does NOT coarsen its grid after the census, at any width."""
    rng = np.random.default_rng(seed)
    at = rng.uniform(0, 1, (400, 3))
    return (at[:, None, :] + rng.normal(0, 0.0005, (400, 150, 3)) * np.array([1.0, 1.0, 0.2])).reshape(-1, 3).astype(np.float32)


def census_points_per_cell(xyz):
    """Points per occupied cell of the grid the small flow's census counts in (kernels_grid.hip, finest_grid: the cloud's extent
    / 1024, widened by 1.25 until the grid has at most max(2^16, 8 n) cells); the flow coarsens iff this is under max_nn / 2."""
    lo, hi = xyz.min(axis=0), xyz.max(axis=0)
    ext = hi.astype(np.float64) - lo.astype(np.float64)
    cap = max(1 << 16, 8 * len(xyz))
    h = ext.max() / 1024.0
    while np.prod(np.floor(ext / h) + 1) > cap:
        h *= 1.25
    dim = (np.floor(ext / h) + 1).astype(np.int64)
    c = np.clip(np.floor((xyz.astype(np.float64) - lo.astype(np.float64)) * (1.0 / h)).astype(np.int64), 0, dim - 1)
    return len(xyz) / len(np.unique(c[:, 0] + dim[0] * (c[:, 1] + dim[1] * c[:, 2])))


_EST = {}


def cached_estimate(name, xyz, radius, max_nn, query):
    key = (name, radius, max_nn)
    if key not in _EST:
        _EST[key] = do.estimate_exact(xyz, radius=radius, max_nn=max_nn, query=query)
    return _EST[key]


@pytest.mark.parametrize("cloud", ["sphere", "box_surface", "tight_blobs"])
def test_widths_small_flow(gpu, cloud):
    """Every list width through the small clouds' flow (at most 65 536 points, two GridMeta slots): direction_kernel<33>, <65> (33
    to 64; 33 is the one width that takes <65> THROUGH this flow) and <129> (wider ones leave it for the medium flow: all_layouts).
    The two surfaces are coarsened after the census, the blobs are not."""
    xyz = {"sphere": lambda: sphere_shell(40000), "box_surface": lambda: box_surface(60000), "tight_blobs": tight_blobs}[cloud]()
    assert len(xyz) <= 65536
    ppc = census_points_per_cell(xyz)
    query = sample(len(xyz), 3000, 21)
    pc = make_cloud(gpu, as_points(xyz))
    for max_nn in WIDTHS:
        assert (ppc >= 0.5 * max_nn) if cloud == "tight_blobs" else (ppc < 0.5 * max_nn) or max_nn <= 4, (cloud, max_nn, ppc)
        radius = 0.002 if cloud == "tight_blobs" else width_radius(max_nn)
        normals, nn, cen = gpu.cwipc_hip_estimate_normals(pc, radius=radius, max_nn=max_nn)
        est = cached_estimate(cloud, xyz, radius, max_nn, query)
        check_normals(xyz, normals, nn, cen, radius=radius, max_nn=max_nn, est=est, what="small flow " + cloud,
                      max_left_out=width_cap(max_nn) if cloud != "tight_blobs" else OTHER_CAP if max_nn > 4 else None)


def test_widths_medium_dense_flow(gpu):
    xyz = sphere_shell(100000, r=0.47)   # (the density of sphere_shell(40000))
    query = sample(len(xyz), 3000, 22)
    pc = make_cloud(gpu, as_points(xyz))
    for max_nn in WIDTHS:
        radius = width_radius(max_nn)
        normals, nn, cen = gpu.cwipc_hip_estimate_normals(pc, radius=radius, max_nn=max_nn)
        check_normals(xyz, normals, nn, cen, query, radius=radius, max_nn=max_nn, what="medium dense flow",
                      max_left_out=OTHER_CAP if max_nn > 4 else None)


_CHILD_XYZ = r"""
import sys, json, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import torch  # noqa: F401  (as the test session: torch's HIP runtime first)
import cwipc_util_amd as cw
from conftest import make_cloud
cw.cwipc_hip_set_device(0)
xyz = np.load(sys.argv[2])["xyz"]
pts = np.zeros(len(xyz), dtype=cw.cwipc_point_numpy_dtype)
pts["x"], pts["y"], pts["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
pc = make_cloud(cw, pts)
out = {}
for i, (radius, max_nn) in enumerate(json.loads(sys.argv[4])):
    out["normals%d" % i], out["nn%d" % i], out["cen%d" % i] = cw.cwipc_hip_estimate_normals(pc, radius=radius, max_nn=max_nn)
np.savez(sys.argv[3], **out)
"""


def normals_in_a_child(xyz, configs, env, tmp_path):
    """[(normals, nn, cen)] per (radius, max_nn) of configs, from a fresh process with `env` (the grid flow knobs are read once)."""
    inp, out = str(tmp_path / "xyz.npz"), str(tmp_path / "normals.npz")
    np.savez(inp, xyz=xyz)
    subprocess.run([sys.executable, "-c", _CHILD_XYZ, ROOT, inp, out, json.dumps(configs)], check=True, timeout=600, env=dict(os.environ, **env))
    r = np.load(out)
    return [(r["normals%d" % i], r["nn%d" % i], r["cen%d" % i]) for i in range(len(configs))]


@pytest.mark.parametrize("env", [{"CWIPC_SOR_SMALL_CELLS": "0"}, {"CWIPC_SOR_SPARSE": "1"}])
def test_widths_forced_flows(gpu, env, tmp_path):
    """The same small cloud forced off the small flow: onto the medium clouds' dense flow, and onto the sparse layout -- which takes
    the widths up to 33 (direction_kernel<33, true> and, for 33 alone, <65, true>); wider lists stay on the dense layout."""
    xyz = sphere_shell(40000)
    query = sample(len(xyz), 3000, 21)
    configs = [(width_radius(w), w) for w in WIDTHS]
    for (radius, max_nn), (normals, nn, cen) in zip(configs, normals_in_a_child(xyz, configs, env, tmp_path)):
        est = cached_estimate("sphere", xyz, radius, max_nn, query)
        check_normals(xyz, normals, nn, cen, radius=radius, max_nn=max_nn, est=est, what="forced flow %s" % env, max_left_out=width_cap(max_nn))


def test_width_33_above_a_million_points(gpu):
    """2^20 points and more take the sparse layout, and max_nn = 33 is the one width that runs direction_kernel<65, true> there."""
    xyz = sphere_shell(1100000, r=1.55)
    assert len(xyz) >= 1 << 20
    normals, nn, cen = normals_of(gpu, as_points(xyz), max_nn=33)
    check_normals(xyz, normals, nn, cen, sample(len(xyz), 3000, 23), max_nn=33, what="1.1 M sparse")


@pytest.mark.parametrize("max_nn", [64, 128])
def test_wide_lists_at_2m(gpu, max_nn):
    """Lists wider than 33 stay on the medium clouds' dense flow at any size: here at 2 M points, a size that flow is not chosen for
    otherwise (192 MB of cell arrays: 8 cells per point)."""
    import time
    xyz = sphere_shell(2000000, r=2.1)
    pc = make_cloud(gpu, as_points(xyz))
    t0 = time.time()
    normals, nn, cen = gpu.cwipc_hip_estimate_normals(pc, radius=0.04, max_nn=max_nn)
    print("direction 2 M points max_nn %d: %.3f s per call (with the download of the normals)" % (max_nn, time.time() - t0))
    check_normals(xyz, normals, nn, cen, sample(len(xyz), 3000, 24), radius=0.04, max_nn=max_nn, what="2 M dense")


def test_max_nn_out_of_range(gpu):
    from cwipc_util_amd import CwipcError
    pc = make_cloud(gpu, as_points(sphere_shell(1000)))
    for max_nn in (129, -1, 2 ** 31 - 1):
        with pytest.raises(CwipcError):
            gpu.cwipc_hip_estimate_normals(pc, radius=0.02, max_nn=max_nn)
        with pytest.raises(CwipcError):
            gpu.cwipc_direction_filter(pc, (0, 0, 1), 0.5, max_nn=max_nn)


# ---------------------------------------------------------------------------
# radius regimes, on a lattice whose spacing is exact
# ---------------------------------------------------------------------------
SPACING = 0.125


def exact_lattice(nx=24, ny=24, nz=12):
    g = np.arange(max(nx, ny, nz), dtype=np.float64) * SPACING
    return np.stack(np.meshgrid(g[:nx], g[:ny], g[:nz], indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)


@pytest.mark.parametrize("regime,radius,max_nn", [("a hundredth of the spacing", SPACING / 100, 30), ("the spacing itself", SPACING, 30),
                                                  ("twice the spacing", 2 * SPACING, 128), ("about one cell", 2.5 * SPACING, 30),
                                                  ("more than ten cells", 13 * SPACING, 4), ("more than ten cells, a wide list", 8 * SPACING, 128)])
def test_radius_regimes_on_a_lattice(gpu, regime, radius, max_nn):
    """The cell size comes from max_nn and the density (about max_nn / 2 points per occupied cell: 2.5 spacings at max_nn 30, 1.3 at
    4, 4 at 128), not from the radius.  A cubic lattice is all ties: nn is the assertion (every point, every tied point in, points at
    exactly the radius out); its covariances are mostly degenerate, so normals are checked where the gap allows, without a cap."""
    xyz = exact_lattice()
    normals, nn, cen = normals_of(gpu, as_points(xyz), radius=radius, max_nn=max_nn)
    est = check_normals(xyz, normals, nn, cen, sample(len(xyz), 1500, 25), radius=radius, max_nn=max_nn, max_left_out=None, what=regime)
    if radius <= SPACING:
        assert np.all(nn == 1)
        assert np.all(np.abs(normals[:, 2]) == 1.0) and np.all(normals[:, :2] == 0)
    if regime == "twice the spacing":
        assert est["nn"].max() == 27   # (the 3 x 3 x 3 block: the points two spacings away, at exactly the radius, are out)


def test_radius_above_the_cloud_with_fewer_points_than_max_nn(gpu):
    """The shell loop runs to the grid's edge and the list never fills: every neighbourhood is the whole cloud."""
    xyz = (np.random.default_rng(26).uniform(-1, 1, (100, 3)) * np.array([1.0, 1.0, 0.1])).astype(np.float32)
    for max_nn in (101, 128):
        normals, nn, cen = normals_of(gpu, as_points(xyz), radius=10.0, max_nn=max_nn)
        assert np.all(nn == 100)
        est = check_normals(xyz, normals, nn, cen, radius=10.0, max_nn=max_nn, max_left_out=None, what="radius above the cloud")
        # one covariance, so one normal up to the orientation -- and up to the fixed point, whose offsets are taken from each query
        assert np.all(angle(est["raw"], est["raw"][:1]) <= 1e-9)
        assert np.all(angle(normals.astype(np.float64), est["raw"][:1]) <= ANGLE_TOL)


def test_radius_one_float_either_side_of_a_decimal_lattice(gpu):
    """Coordinates k * 0.02 rounded to float32: the distances between lattice neighbours scatter around float32(0.02)^2 by a rounding
    error, and which of them are under r2 changes with the last bit of the radius -- exactly where the oracle says."""
    g = (np.arange(20, dtype=np.float64) * 0.02).astype(np.float32)
    xyz = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    r = np.float32(0.02)
    seen = []
    for radius in (float(np.nextafter(r, np.float32(0))), float(r), float(np.nextafter(r, np.float32(1)))):
        normals, nn, cen = normals_of(gpu, as_points(xyz), radius=radius, max_nn=30)
        est = check_normals(xyz, normals, nn, cen, radius=radius, max_nn=30, max_left_out=None, what="decimal lattice")
        seen.append(est["nn"])
    # the case is what it says (the oracle alone: no point changes between the radius below and 0.02f, 4 625 of 8 000 do above it)
    assert (seen[0] != seen[1]).any() or (seen[1] != seen[2]).any()


# ---------------------------------------------------------------------------
# geometry: the shapes of the outlier filter's tests
# ---------------------------------------------------------------------------
def plane_and_blob(seed=27):
    rng = np.random.default_rng(seed)
    plane = np.column_stack([rng.uniform(0, 0.4, (20000, 2)), np.full(20000, 0.25)])
    blob = rng.normal(0, 0.01, (2000, 3)) * np.array([1.0, 1.0, 0.2]) + np.array([0.2, 0.2, -1.0])   # puts the centroid under the plane
    return np.vstack([plane, blob]).astype(np.float32)


def stacks_among_points(seed=28):
    rng = np.random.default_rng(seed)
    sheet = np.column_stack([rng.uniform(0, 0.3, (20000, 2)), 0.02 * np.sin(rng.uniform(0, 6, 20000))])
    stacks = np.repeat(sheet[rng.choice(20000, 40, replace=False)], 50, axis=0)   # 51 copies: more than max_nn = 30
    xyz = np.vstack([sheet, stacks])
    return xyz[rng.permutation(len(xyz))].astype(np.float32)   # ... next to ordinary points in the same waves


def far_outliers(seed=29):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(20000, 3))
    return np.vstack([v / np.linalg.norm(v, axis=1, keepdims=True) * 0.2, rng.uniform(-30, 30, (20, 3))]).astype(np.float32)


GEOMETRY = {
    "shifted by +100": lambda: (sphere_shell(40000, r=0.6).astype(np.float64) + 100.0, 0.04),
    "shifted by -3": lambda: (sphere_shell(40000).astype(np.float64) - 3.0, 0.02),
    "scale 1e-3": lambda: (sphere_shell(40000).astype(np.float64) * 1e-3, 0.02e-3),
    "scale 0.1": lambda: (sphere_shell(40000).astype(np.float64) * 0.1, 0.002),
    "scale 25": lambda: (sphere_shell(40000).astype(np.float64) * 25.0, 0.5),
    "exact plane": lambda: (plane_and_blob(), 0.02),
    "stacks above max_nn": lambda: (stacks_among_points(), 0.02),
    "far outliers": lambda: (far_outliers(), 0.02),
}


@pytest.mark.parametrize("shape", sorted(GEOMETRY))
@pytest.mark.parametrize("max_nn", [30, 64])
def test_normals_hard_geometry(gpu, shape, max_nn):
    xyz, radius = GEOMETRY[shape]()
    xyz = xyz.astype(np.float32)
    normals, nn, cen = normals_of(gpu, as_points(xyz), radius=radius, max_nn=max_nn)
    est = check_normals(xyz, normals, nn, cen, sample(len(xyz), 4000, 30), radius=radius, max_nn=max_nn, what=shape)
    if shape == "exact plane":
        on = est["index"] < 20000
        assert np.array_equal(normals[est["index"][on]], np.tile(np.float32([0, 0, 1]), (on.sum(), 1)))   # smallest eigenvalue 0: exactly z
    if shape == "stacks above max_nn":
        assert (est["nn"] > max_nn).any() or max_nn > 51


@pytest.mark.parametrize("max_nn", [4, 30, 128])
def test_line_counts_only(gpu, max_nn):
    """A line: two eigenvalues are 0, the gap is 0, no normal is defined -- nn only is asserted, for every point."""
    t = np.random.default_rng(31).random(5000)
    xyz = np.stack([t * 3.0, np.full(5000, 0.5), np.full(5000, -0.25)], axis=1).astype(np.float32)
    normals, nn, cen = normals_of(gpu, as_points(xyz), radius=0.02, max_nn=max_nn)
    est = check_normals(xyz, normals, nn, cen, radius=0.02, max_nn=max_nn, max_left_out=None, what="line")
    assert np.all(np.isfinite(normals)) and (est["gap"] < GAP_MIN).mean() > 0.9


@pytest.mark.parametrize("max_nn", [30, 33])
def test_thin_wide_strip_through_the_sparse_layout(gpu, max_nn, tmp_path):
    """40 m by 0.02 m: every query is an edge query (second and third shells), and the rows cross empty segments.  The strip is a
    wavy band, its centroid in its middle: normals are checked where the orientation allows, nn for every point."""
    rng = np.random.default_rng(32)
    x = rng.random(65536) * 40.0
    xyz = np.stack([x, rng.random(65536) * 0.02, 0.3 * np.sin(x)], axis=1).astype(np.float32)
    (normals, nn, cen), = normals_in_a_child(xyz, [(0.2, max_nn)], {"CWIPC_SOR_SPARSE": "1"}, tmp_path)
    check_normals(xyz, normals, nn, cen, sample(len(xyz), 4000, 33), radius=0.2, max_nn=max_nn, max_left_out=None, what="strip, sparse")
    normals, nn, cen = normals_of(gpu, as_points(xyz), radius=0.2, max_nn=max_nn)
    check_normals(xyz, normals, nn, cen, sample(len(xyz), 4000, 33), radius=0.2, max_nn=max_nn, max_left_out=None, what="strip, small flow")


# ---------------------------------------------------------------------------
# non-finite points (they sit in clamped cells, are nobody's neighbour, and make the centroid NaN)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("max_nn", [30, 64])
def test_non_finite_points(gpu, max_nn):
    xyz = sphere_shell(40000)
    rng = np.random.default_rng(34)
    bad = rng.choice(len(xyz), 60, replace=False)
    xyz[bad, rng.integers(0, 3, 60)] = rng.choice(np.float32([np.nan, np.inf, -np.inf]), 60)
    xyz[bad[0]] = np.nan
    finite = np.isfinite(xyz).all(axis=1)
    normals, nn, cen = normals_of(gpu, as_points(xyz), max_nn=max_nn)          # the call returns
    assert np.all(np.isnan(cen))                                               # as numpy.mean of the reference
    assert np.all(nn[~finite] == 0)                                            # no distance to or from such a point compares
    assert np.all(normals[~finite] == np.float32([0, 0, -1]))
    # the finite points: the finite sub-cloud's neighbourhoods, and its normals up to sign (a NaN centroid orients nothing)
    sub = xyz[finite]
    check_normals(sub, normals[finite], nn[finite], cen, sample(len(sub), 4000, 35), max_nn=max_nn, oriented=False, what="non-finite")


# ---------------------------------------------------------------------------
# random configurations
# ---------------------------------------------------------------------------
def random_configuration(seed):
    rng = np.random.default_rng(7000 + seed)
    n = int(rng.choice([40, 200, 1000, 5000, 30000]))
    max_nn = int(rng.choice(WIDTHS))
    kind = str(rng.choice(["box", "clusters", "line", "sheet", "dupes"]))
    scale = float(rng.choice([0.1, 1.0, 25.0]))
    if kind == "box":
        xyz = rng.random((n, 3)) * scale
        spacing = scale / n ** (1 / 3)
    elif kind == "clusters":
        centres = rng.random((5, 3)) * scale
        xyz = centres[rng.integers(0, 5, n)] + rng.normal(0, scale * 0.003, (n, 3))
        spacing = scale * 0.003 * 4 / (n / 5) ** (1 / 3)
    elif kind == "line":
        xyz = np.stack([rng.random(n) * scale, np.zeros(n), np.zeros(n)], axis=1)
        spacing = scale / n
    elif kind == "sheet":
        xyz = np.stack([rng.random(n) * scale, rng.random(n) * scale, np.full(n, 0.25)], axis=1)
        spacing = scale / n ** 0.5
    else:   # many coincident points
        base = rng.random((max(n // 10, 1), 3)) * scale
        xyz = base[rng.integers(0, len(base), n)]
        spacing = scale / len(base) ** (1 / 3)
    xyz += rng.choice([0.0, -3.0, 100.0])
    radius = float(rng.choice([0.3, 1.0, 3.0, 10.0])) * spacing
    return xyz.astype(np.float32), radius, max_nn, kind


@pytest.mark.parametrize("seed", range(40))
def test_normals_random_configurations(gpu, seed):
    """Differential test over random shapes, sizes, widths and radii (0.3 to 10 mean spacings): nn for every sampled point, normals
    where gap and orientation allow (lines, flat sheets and stacks are degenerate by design: no cap)."""
    xyz, radius, max_nn, kind = random_configuration(seed)
    normals, nn, cen = normals_of(gpu, as_points(xyz), radius=radius, max_nn=max_nn)
    check_normals(xyz, normals, nn, cen, sample(len(xyz), 1000, seed), radius=radius, max_nn=max_nn, max_left_out=None,
                  what="random %d %s n %d" % (seed, kind, len(xyz)))


# ---------------------------------------------------------------------------
# the order of the input
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("max_nn", [30, 65])
def test_permuted_input(gpu, max_nn):
    xyz = box_surface(60000)
    perm = np.random.default_rng(36).permutation(len(xyz))
    radius = width_radius(max_nn)
    a_n, a_nn, _ = normals_of(gpu, as_points(xyz), radius=radius, max_nn=max_nn)
    b_n, b_nn, _ = normals_of(gpu, as_points(xyz[perm]), radius=radius, max_nn=max_nn)
    back = np.argsort(perm)
    b_n, b_nn = b_n[back], b_nn[back]
    assert np.array_equal(a_nn, b_nn)
    query = sample(len(xyz), 6000, 37)
    est = do.estimate_exact(xyz, radius=radius, max_nn=max_nn, query=query)
    firm = est["orient"] >= ORIENT_MIN     # only the centroid's slice sums depend on the order, and only the orientation on them
    assert firm.mean() > 0.95
    assert np.array_equal(a_n[query][firm], b_n[query][firm])
    assert np.array_equal(np.abs(a_n), np.abs(b_n))


# ---------------------------------------------------------------------------
# the filter's mask at the wide lists
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("max_nn", [64, 128])
def test_filter_against_oracle_wide_lists(gpu, max_nn):
    pts = as_points(sphere_shell(40000))
    out = gpu.cwipc_direction_filter(make_cloud(gpu, pts, 0.0, 4321), (1, 0.5, 0), 0.2, radius=0.04, max_nn=max_nn)
    kept = check_filter_output(pts, out, (1, 0.5, 0), 0.2, radius=0.04, max_nn=max_nn)
    assert 0 < kept.sum() < len(pts)
