"""Euclidean clusters on the GPU (cwipc_hip_clusters, cwipc_hip_cluster_filter; RULE K of hip_ext.h) held to the numpy and scipy model
of tests/cluster_model.py: labels and sizes equal, the filtered cloud's bytes equal.

The cases that a grid's layout could break -- ties at the radius on lattices whose points lie on cell faces, long chains in every
index order, the single link between two chains -- run in one child process per grid flow (small clouds, dense, sparse), as
tests/test_gpu_walk_exact.py::test_each_flow does; the model's answers are computed once for the three."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import make_cloud
import cluster_model as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

FILTERS = ((1, 0), (2, 0), (1, 1), (3, 2))     # (min_points, max_clusters) tried on every flow case


def as_points(xyz, tile=1, seed=0):
    from cwipc_util_amd import cwipc_point_numpy_dtype
    xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    pts = np.zeros(len(xyz), dtype=cwipc_point_numpy_dtype)
    if len(xyz):
        pts["x"], pts["y"], pts["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
        rng = np.random.default_rng(seed)
        pts["r"], pts["g"], pts["b"] = rng.integers(0, 256, (3, len(xyz)))
    pts["tile"] = tile
    return pts


def xyz_of(pts):
    return np.stack([pts["x"], pts["y"], pts["z"]], axis=1)


def lattice(side, spacing, offset):
    g = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    return (g * spacing + np.array(offset)).astype(np.float32)


def line(n, spacing, order, seed=0):
    """n points along x, `spacing` apart; index i sits at position order(i)"""
    pos = {"ascending": np.arange(n), "descending": np.arange(n)[::-1], "shuffled": np.random.default_rng(seed).permutation(n)}[order]
    xyz = np.zeros((n, 3))
    xyz[:, 0] = pos * spacing
    return xyz.astype(np.float32)


def serpentine(spacing, length=30, rows=8, layers=8):
    """One path that folds through a cube: runs along x, three steps apart in y (2.7 r: rows do not link), joined at alternating
    ends by two points; layers three steps apart in z, joined the same way.  Only consecutive points are within r."""
    path, y, ydir = [], 0, 1
    x = 0
    xdir = 1
    for k in range(layers):
        for j in range(rows):
            for _ in range(length):
                path.append((x, y, 3 * k))
                x += xdir
            x -= xdir
            xdir = -xdir
            if j + 1 < rows:
                path += [(x, y + ydir, 3 * k), (x, y + 2 * ydir, 3 * k)]
                y += 3 * ydir
        ydir = -ydir
        if k + 1 < layers:
            path += [(x, y, 3 * k + 1), (x, y, 3 * k + 2)]
    return (np.array(path, dtype=np.float64) * spacing).astype(np.float32)


def two_chains(gap):
    """Chain A along x on y = 0; chain B a V whose apex hangs `gap` above A's middle point and whose arms rise at 45 degrees.  r = 0.25,
    spacing 0.9 r: the apex and the point under it are the only pair of the two chains that can be within r."""
    r, n = 0.25, 400
    s = np.float32(0.9 * r)
    a = np.zeros((2 * n + 1, 3), dtype=np.float32)
    a[:, 0] = (np.arange(2 * n + 1) * np.float64(s)).astype(np.float32)
    mid = a[n]
    step = np.float64(s) / np.sqrt(2.0)
    k = np.arange(1, n + 1)
    left = np.stack([mid[0] - k * step, gap + k * step, np.zeros(n)], axis=1)
    right = np.stack([mid[0] + k * step, gap + k * step, np.zeros(n)], axis=1)
    b = np.concatenate([left[::-1], [[mid[0], gap, 0.0]], right]).astype(np.float32)
    assert b[n, 0] == mid[0] and b[n, 1] == np.float32(gap)
    return np.concatenate([a, b])


def flow_cases():
    """{name: (points, radius, same_tile)}"""
    cases = {}
    quarter = np.float32(0.25)
    for offset in ((0.0, 0.0, 0.0), (1.0, 0.5, -1.0), (0.125, -0.375, 0.0625)):
        lat = lattice(12, 0.25, offset)
        cases["lattice at %s, r = spacing" % (offset,)] = (as_points(lat), 0.25, False)
        cases["lattice at %s, r one step above" % (offset,)] = (as_points(lat), float(np.nextafter(0.25, 1)), False)
    perm = np.random.default_rng(12).permutation(12 ** 3)
    cases["lattice permuted, r one step above"] = (as_points(lattice(12, 0.25, (0, 0, 0))[perm]), float(np.nextafter(0.25, 1)), False)
    r = 0.01
    for order in ("ascending", "descending", "shuffled"):
        cases["chain " + order] = (as_points(line(20000, 0.9 * r, order, 5)), r, False)
    snake = serpentine(0.9 * r)
    cases["serpentine"] = (as_points(snake), r, False)
    cases["serpentine reversed"] = (as_points(snake[::-1]), r, False)
    cases["serpentine shuffled"] = (as_points(snake[np.random.default_rng(6).permutation(len(snake))]), r, False)
    for name, gap in (("under", np.nextafter(quarter, np.float32(0))), ("at", quarter), ("one step past", np.nextafter(quarter, np.float32(1)))):
        cases["two chains, apex %s r" % name] = (as_points(two_chains(gap)), 0.25, False)
    return cases


def model_answers(cases):
    want = {}
    for name, (pts, radius, same) in cases.items():
        labels, sizes = cm.cluster_labels(xyz_of(pts), radius, pts["tile"] if same else None)
        want[name] = (labels, sizes, [pts[cm.keep_mask(labels, sizes, mp, mc)] for mp, mc in FILTERS])
    return want


_FLOW_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import torch  # noqa: F401  (as the test session: torch's HIP runtime first)
import cwipc_util_amd as cw
from conftest import make_cloud
cw.cwipc_hip_set_device(0)
d = np.load(sys.argv[2])
out = {}
for c in range(int(d["ncases"])):
    pc = make_cloud(cw, d["pts_%d" % c])
    radius, same = float(d["radius_%d" % c]), bool(d["same_%d" % c])
    out["labels_%d" % c], out["sizes_%d" % c] = cw.cwipc_cluster_labels(pc, radius, same)
    for k, (mp, mc) in enumerate(d["filters"]):
        kept = cw.cwipc_cluster_filter(pc, radius, int(mp), int(mc), same)
        out["kept_%d_%d" % (c, k)] = kept.get_numpy_array()
        kept.free()
    pc.free()
np.savez(sys.argv[3], **out)
"""


@pytest.fixture(scope="module")
def flow_model():
    cases = flow_cases()
    want = model_answers(cases)
    # the constructions do what they say
    for name, (labels, sizes, _) in want.items():
        if "r = spacing" in name:
            assert len(sizes) == 1728 and np.array_equal(labels, np.arange(1728))
        elif name.startswith("lattice") or name.startswith("chain") or name.startswith("serpentine") or name == "two chains, apex under r":
            assert sizes.tolist() == [len(labels)] and not labels.any(), name
        else:
            assert sizes.tolist() == [801, 801], name
    snake = xyz_of(cases["serpentine"][0])
    assert len(cm.links(snake, 0.01)) == len(snake) - 1 and np.ptp(snake, axis=0).min() > 0.15     # a path, and it fills a box
    return cases, want


@pytest.mark.parametrize("env", [{}, {"CWIPC_SOR_SMALL_CELLS": "0"}, {"CWIPC_SOR_SPARSE": "1"}], ids=["small clouds", "dense", "sparse"])
def test_each_flow(gpu, flow_model, env, tmp_path):
    cases, want = flow_model
    inp, out = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    arrays = {"ncases": np.array(len(cases)), "filters": np.array(FILTERS)}
    for c, (pts, radius, same) in enumerate(cases.values()):
        arrays["pts_%d" % c], arrays["radius_%d" % c], arrays["same_%d" % c] = pts, np.float64(radius), np.array(same)
    np.savez(inp, **arrays)
    subprocess.run([sys.executable, "-c", _FLOW_CHILD, ROOT, inp, out], check=True, timeout=300, env=dict(os.environ, **env))
    got = np.load(out)
    for c, name in enumerate(cases):
        labels, sizes, kept = want[name]
        assert got["labels_%d" % c].dtype == np.uint32 and got["sizes_%d" % c].dtype == np.uint32
        assert np.array_equal(got["sizes_%d" % c], sizes), (env, name, len(got["sizes_%d" % c]), len(sizes))
        assert np.array_equal(got["labels_%d" % c], labels), (env, name)
        for k in range(len(FILTERS)):
            assert got["kept_%d_%d" % (c, k)].tobytes() == kept[k].tobytes(), (env, name, FILTERS[k])


# ---------------------------------------------------------------------------
# in this process (whatever flow the cloud's size selects)
# ---------------------------------------------------------------------------
def check(gpu, pts, radius, same_tile=False, filters=((1, 0), (2, 0), (1, 1), (1, 2))):
    """labels, sizes and the filtered clouds of one cloud against the model -> (labels, sizes)"""
    pc = make_cloud(gpu, pts, cellsize=0.0078125, timestamp=4711)
    labels, sizes = gpu.cwipc_cluster_labels(pc, radius, same_tile)
    wl, ws = cm.cluster_labels(xyz_of(pts), radius, pts["tile"] if same_tile else None)
    assert labels.dtype == np.uint32 and sizes.dtype == np.uint32
    assert np.array_equal(sizes, ws), (len(sizes), len(ws))
    assert np.array_equal(labels, wl)
    for mp, mc in filters:
        kept = gpu.cwipc_cluster_filter(pc, radius, mp, mc, same_tile)
        assert kept.get_numpy_array().tobytes() == pts[cm.keep_mask(wl, ws, mp, mc)].tobytes(), (mp, mc)
        assert kept.timestamp() == 4711 and kept.cellsize() == np.float32(0.0078125)
        kept.free()
    assert pc.get_numpy_array().tobytes() == pts.tobytes()     # neither consumed nor changed
    pc.free()
    return labels, sizes


@pytest.fixture(scope="module")
def random_xyz():
    return np.random.default_rng(4097).uniform(0, 1, (4097, 3)).astype(np.float32)


@pytest.mark.parametrize("factor", [0.05, 0.5, 1.0, 1.5, 10.0])
def test_radius_against_cell_size(gpu, random_xyz, factor):
    """Random points in the unit cube, radius from a twentieth of the mean spacing to ten times it: all singletons to one cluster."""
    spacing = len(random_xyz) ** (-1.0 / 3.0)
    labels, sizes = check(gpu, as_points(random_xyz), factor * spacing)
    if factor == 0.05:
        assert len(sizes) >= len(random_xyz) - 3 and sizes.max() <= 2
    if factor == 10.0:
        assert len(sizes) == 1
    if factor == 1.0:
        assert 100 < len(sizes) < 4000 and sizes.max() > 10


def test_radius_larger_than_the_cloud(gpu, random_xyz):
    for radius in (2.0, 1e6, 1e30):
        labels, sizes = check(gpu, as_points(random_xyz[:1500]), radius)
        assert sizes.tolist() == [1500]


def test_duplicates(gpu):
    labels, sizes = check(gpu, as_points(np.tile(np.float32([[0.5, 0.25, 0.75]]), (64, 1))), 1e-6)
    assert sizes.tolist() == [64] and not labels.any()
    # ... and among other points: every copy in the cluster of the first
    xyz = np.random.default_rng(64).uniform(0, 1, (300, 3)).astype(np.float32)
    xyz[100:164] = xyz[7]
    labels, sizes = check(gpu, as_points(xyz), 1e-4)
    assert np.all(labels[100:164] == labels[7]) and sizes[labels[7]] == 65


def test_non_finite_points(gpu, random_xyz):
    xyz = random_xyz[:3000].copy()
    rng = np.random.default_rng(3000)
    bad = rng.choice(3000, 40, replace=False)
    for k, i in enumerate(bad):
        xyz[i, k % 3] = (np.nan, np.inf, -np.inf)[(k // 3) % 3]
    xyz[bad[0]] = np.nan
    radius = 1.2 * 3000 ** (-1.0 / 3.0)
    labels, sizes = check(gpu, as_points(xyz), radius)
    assert np.all(labels[bad] == cm.NONE) and (labels == cm.NONE).sum() == 40 and sizes.sum() == 2960
    # their neighbours' clusters are what they are without them
    finite = np.setdiff1d(np.arange(3000), bad)
    wl, ws = cm.cluster_labels(xyz[finite], radius)
    assert np.array_equal(labels[finite], wl) and np.array_equal(sizes, ws)
    # a cloud without a single finite point
    labels, sizes = check(gpu, as_points(np.full((70, 3), np.nan)), 0.5)
    assert len(sizes) == 0 and np.all(labels == cm.NONE)


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 255, 256, 257, 4097])
def test_sizes(gpu, random_xyz, n):
    xyz = random_xyz[:n]
    spacing = max(n, 1) ** (-1.0 / 3.0)
    labels, sizes = check(gpu, as_points(xyz), 0.9 * spacing)
    assert len(labels) == n and sizes.sum() == n
    # every point isolated
    labels, sizes = check(gpu, as_points(xyz), 1e-5)
    assert np.array_equal(labels, np.arange(n)) and np.array_equal(sizes, np.ones(n))


def test_two_points(gpu):
    for second, want in (((0.5, 0, 0), [2]), ((1.5, 0, 0), [1, 1]), ((1.0, 0, 0), [1, 1]), ((0, 0, 0), [2])):
        labels, sizes = check(gpu, as_points(np.float32([(0, 0, 0), second])), 1.0)
        assert sizes.tolist() == want


def blobs(seed=8):
    """Two interpenetrating blobs (tiles 1 and 2) and three far clumps of 40, 40 and 7 points (tile 4)."""
    rng = np.random.default_rng(seed)
    a = rng.normal((0.0, 0, 0), 0.05, (600, 3))
    b = rng.normal((0.03, 0, 0), 0.05, (500, 3))
    c1 = rng.normal((2.0, 0, 0), 0.004, (40, 3))
    c2 = rng.normal((0, 2.0, 0), 0.004, (40, 3))
    c3 = rng.normal((0, 0, 2.0), 0.004, (7, 3))
    xyz = np.concatenate([a, b, c1, c2, c3]).astype(np.float32)
    tile = np.concatenate([np.full(600, 1), np.full(500, 2), np.full(87, 4)]).astype(np.uint8)
    perm = rng.permutation(len(xyz))
    return as_points(xyz[perm], tile[perm], seed)


def test_same_tile(gpu):
    pts = blobs()
    core = (np.abs(xyz_of(pts)) < 0.05).all(axis=1)
    labels, sizes = check(gpu, pts, 0.03)
    assert len(set(labels[core].tolist())) == 1                      # without the flag the two blobs' cores are one cluster
    labels, sizes = check(gpu, pts, 0.03, same_tile=True)
    assert len(set(labels[core & (pts["tile"] == 1)].tolist())) == 1 and len(set(labels[core & (pts["tile"] == 2)].tolist())) == 1
    assert len(set(labels[core].tolist())) == 2                      # with it they are two
    for c in range(len(sizes)):
        assert len(set(pts["tile"][labels == c].tolist())) == 1


def test_filter(gpu):
    pts = blobs()
    wl, ws = cm.cluster_labels(xyz_of(pts), 0.03)
    C = len(ws)
    by_size = sorted(ws.tolist(), reverse=True)
    assert by_size.count(40) == 2 and 7 in by_size and C >= 4
    big = by_size[0]
    filters = [(40, 0), (41, 0), (7, 0), (8, 0), (big, 0), (big + 1, 0), (1, 1), (1, 2), (1, 3), (1, C), (1, C + 5), (40, 2), (40, 3), (2 ** 40, 0), (1, 2 ** 32 - 1)]
    check(gpu, pts, 0.03, filters=filters)
    # two clusters of equal size at max_clusters = 1: the lower number stays.  (Only the two clumps of 40 here.)
    clumps = pts[np.isin(wl, np.flatnonzero(ws == 40))]
    labels, sizes = check(gpu, clumps, 0.03, filters=[(1, 1), (1, 2), (41, 1)])
    assert sizes.tolist() == [40, 40]
    pc = make_cloud(gpu, clumps)
    kept = gpu.cwipc_cluster_filter(pc, 0.03, 1, 1)
    assert kept.get_numpy_array().tobytes() == clumps[labels == 0].tobytes()
    kept.free()
    pc.free()


def test_filter_result_stays_on_the_device(gpu):
    """The result is fed on to cwipc_downsample and cwipc_remove_outliers without leaving the device; the factory's filter does the same."""
    from cwipc_util_amd import filters
    dll = gpu.cwipc_util_dll_load()
    pts = blobs()
    wl, ws = cm.cluster_labels(xyz_of(pts), 0.03)
    want = pts[cm.keep_mask(wl, ws, 41, 0)]
    pc = make_cloud(gpu, pts, cellsize=0.001)
    kept = gpu.cwipc_cluster_filter(pc, 0.03, min_points=41)
    assert dll.cwipc_hip_is_device_resident(kept.as_cwipc_p()) == 1
    ref = make_cloud(gpu, want, cellsize=0.001)
    for op in (lambda p: gpu.cwipc_downsample(p, 0.01), lambda p: gpu.cwipc_remove_outliers(p, 8, 1.0, False)):
        a, b = op(kept), op(ref)
        assert dll.cwipc_hip_is_device_resident(a.as_cwipc_p()) == 1
        assert a.count() > 0 and a.get_numpy_array().tobytes() == b.get_numpy_array().tobytes()
        a.free()
        b.free()
    f = filters.factory("cluster(0.03, 41)")
    again = f.filter(pc)
    assert again.get_numpy_array().tobytes() == want.tobytes()
    for c in (again, kept, ref, pc):
        c.free()


def test_order_independence(gpu, random_xyz):
    xyz = random_xyz[:3000]
    radius = 1.1 * 3000 ** (-1.0 / 3.0)
    perm = np.random.default_rng(1).permutation(3000)
    la, sa = check(gpu, as_points(xyz), radius, filters=())
    lb, sb = check(gpu, as_points(xyz[perm]), radius, filters=())
    # the same partition: the smallest ORIGINAL index of a point's cluster, computed from either labelling
    first_a = np.full(len(sa), 3000)
    np.minimum.at(first_a, la, np.arange(3000))
    first_b = np.full(len(sb), 3000)
    np.minimum.at(first_b, lb, perm)
    back = np.empty(3000, dtype=np.int64)
    back[perm] = np.arange(3000)
    assert len(sa) == len(sb) and np.array_equal(first_a[la], first_b[lb][back])
    assert sorted(sa.tolist()) == sorted(sb.tolist())
    # the same call twice: the same bytes
    pc = make_cloud(gpu, as_points(xyz))
    one, two = gpu.cwipc_cluster_labels(pc, radius), gpu.cwipc_cluster_labels(pc, radius)
    assert one[0].tobytes() == two[0].tobytes() and one[1].tobytes() == two[1].tobytes()
    k1, k2 = gpu.cwipc_cluster_filter(pc, radius, 5, 3), gpu.cwipc_cluster_filter(pc, radius, 5, 3)
    assert k1.get_numpy_array().tobytes() == k2.get_numpy_array().tobytes()
    for c in (k1, k2, pc):
        c.free()


def test_link_statistics(gpu, random_xyz):
    pc = make_cloud(gpu, as_points(random_xyz))
    radius = 1.5 * len(random_xyz) ** (-1.0 / 3.0)
    stats = gpu.cwipc_hip_cluster_link_stats(pc, radius)
    assert stats["links"] == len(cm.links(random_xyz, radius))      # each unordered pair seen once
    assert 0 < stats["unions"] <= stats["links"] and stats["max_loads_one_union"] <= stats["find_loads"]
    pc.free()


def test_refusals(gpu):
    dll = gpu.cwipc_util_dll_load()
    logged = []
    gpu.cwipc_log_configure(gpu.CWIPC_LOG_LEVEL_WARNING, lambda level, msg: logged.append((level, msg)))
    try:
        pc = make_cloud(gpu, as_points(np.random.default_rng(2).uniform(0, 1, (300, 3))))
        p = pc.as_cwipc_p()
        labels, sizes = np.full(300, 7, dtype=np.uint32), np.full(300, 7, dtype=np.uint32)
        count = ctypes.c_uint32(7)
        inf, nan = float("inf"), float("nan")

        def refused(cloud, radius, flags):
            n = len(logged)
            rc = dll.cwipc_hip_clusters(cloud, radius, flags, labels.ctypes.data, sizes.ctypes.data, 300, ctypes.byref(count))
            out = dll.cwipc_hip_cluster_filter(cloud, radius, flags, 1, 0)
            return rc == -1 and not out and len(logged) == n + 2

        for args in ((p, nan, 0), (p, 0.0, 0), (p, -1.0, 0), (p, inf, 0), (p, 0.1, 2), (p, 0.1, -1), (None, 0.1, 0)):
            assert refused(*args), args
        n = len(logged)
        assert dll.cwipc_hip_clusters(p, 0.1, 0, labels.ctypes.data, sizes.ctypes.data, 299, ctypes.byref(count)) == -1 and len(logged) == n + 1
        assert all(level == gpu.CWIPC_LOG_LEVEL_ERROR for level, _ in logged)
        assert np.all(labels == 7) and np.all(sizes == 7) and count.value == 7          # nothing was written
        # either array may be NULL
        n = len(logged)
        assert dll.cwipc_hip_clusters(p, 0.1, 0, None, None, 0, ctypes.byref(count)) == 0 and 0 < count.value <= 300
        assert dll.cwipc_hip_clusters(p, 0.1, 1, labels.ctypes.data, None, 300, None) == 0 and labels.max() == count.value - 1
        assert len(logged) == n
        for call in (lambda: gpu.cwipc_cluster_labels(pc, nan), lambda: gpu.cwipc_cluster_filter(pc, 0.0), lambda: gpu.cwipc_cluster_filter(pc, -2.0, 1, 1)):
            with pytest.raises(gpu.CwipcError):
                call()
        pc.free()
    finally:
        gpu.cwipc_log_configure(gpu.CWIPC_LOG_LEVEL_WARNING, None)
