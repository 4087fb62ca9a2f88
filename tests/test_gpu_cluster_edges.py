"""Euclidean clusters on the GPU, the paths that tests/test_gpu_cluster.py leaves unrun; every comparison is exact (bytes, or
integer equality with tests/cluster_model.py).

  three flows  one child process per grid flow (small clouds, dense, sparse): the tile flag (a bridge of another tile, twins at
               identical coordinates with tile bytes 0, 128 and 255, two interpenetrating chains), non-finite points, a radius of
               many cells, far outliers that collapse the cloud into one cell, a translated cloud whose coordinates tie.  Every case
               also runs the link statistics with its flag: all four instantiations of the link kernel are launched.
  scale        the 102^3 jittered lattice in a child without knobs: 2^20 points select the sparse flow themselves, every grid-stride
               loop takes a second trip, and 424 919 clusters send the ranking histogram's loop round again as well.
  contention   a clique of 3000, 4096 duplicates in one cell, a chain in bit-reversed index order, a cluster of 68 921 points (the
               third byte of the radix selection through the public filter).
  ranking      cwipc_hip_cluster_rank_keep: the filter's ranking kernels on chosen size words, all four bytes.
  radius       1e-170 (r2 = 0: nothing links) to 1e200 (r2 = inf: every finite pair links).
  host state   a work block that an earlier, bigger call left dirty, device-resident input, four host threads."""
import functools
import os
import subprocess
import sys
import threading
import time

import numpy as np
import pytest

from conftest import make_cloud
import cluster_model as cm
from test_gpu_cluster import FILTERS, as_points, check, lattice, xyz_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

FLT_MAX = float(np.finfo(np.float32).max)


# ---------------------------------------------------------------------------
# the constructions (CPU only; the fixtures assert that each does what its name says)
# ---------------------------------------------------------------------------
def random_xyz():
    return np.random.default_rng(4097).uniform(0, 1, (4097, 3)).astype(np.float32)


def tile_bridge(order):
    """600 points along x, 0.9 r apart, r = 0.01; all of tile 1 but the one at position 200, tile 2: the chain's only bridge there"""
    n, r = 600, 0.01
    pos = {"ascending": np.arange(n), "reversed": np.arange(n)[::-1], "shuffled": np.random.default_rng(600).permutation(n)}[order]
    xyz = np.zeros((n, 3))
    xyz[:, 0] = pos * (0.9 * r)
    tile = np.where(pos == 200, 2, 1).astype(np.uint8)
    return as_points(xyz, tile), r


def tile_twins():
    """the 8 x 8 x 8 lattice of spacing 0.25, every position held by three points of tiles 0, 128 and 255; shuffled"""
    lat = lattice(8, 0.25, (0.0, 0.0, 0.0))
    xyz = np.concatenate([lat, lat, lat])
    tile = np.repeat(np.uint8([0, 128, 255]), len(lat))
    perm = np.random.default_rng(1536).permutation(len(xyz))
    return as_points(xyz[perm], tile[perm])


def tile_chains():
    """two x-chains of 400, 0.9 r apart along x and 0.3 r from each other in y, tiles 7 and 200, interleaved in index order"""
    n, r = 400, 0.01
    xyz = np.zeros((2 * n, 3))
    xyz[0::2, 0] = xyz[1::2, 0] = np.arange(n) * (0.9 * r)
    xyz[1::2, 1] = 0.3 * r
    tile = np.tile(np.uint8([7, 200]), n)
    return as_points(xyz, tile), r


def non_finite(tiles):
    """the construction of test_gpu_cluster.test_non_finite_points: 3000 points, 40 with a NaN or an infinity -> (points, radius, bad)"""
    xyz = random_xyz()[:3000].copy()
    rng = np.random.default_rng(3000)
    bad = rng.choice(3000, 40, replace=False)
    for k, i in enumerate(bad):
        xyz[i, k % 3] = (np.nan, np.inf, -np.inf)[(k // 3) % 3]
    xyz[bad[0]] = np.nan
    tile = rng.choice(np.uint8([0, 3, 255]), 3000) if tiles else 1
    return as_points(xyz, tile), 1.2 * 3000 ** (-1.0 / 3.0), bad


OUTLIERS = np.float32([(1e6, 0, 0), (-1e6, .5, .5), (3e38, 0, 0), (-3e38, 3e38, -3e38), (FLT_MAX, FLT_MAX, FLT_MAX), (1e6, 0, 0.05)])


def far_outliers():
    """3000 uniform points in the unit cube with six far points at indices 1500 .. 1505: the grid's box is theirs"""
    xyz = np.random.default_rng(3006).uniform(0, 1, (3000, 3)).astype(np.float32)
    return as_points(np.concatenate([xyz[:1500], OUTLIERS, xyz[1500:]]))


def translated():
    """4000 uniform points in the unit cube moved to (16384, -16384, 8192): float32 keeps steps of 1/512 (x) and 1/1024 (y, z)"""
    xyz = np.random.default_rng(4000).uniform(0, 1, (4000, 3)) + np.array([16384.0, -16384.0, 8192.0])
    return as_points(xyz.astype(np.float32))


def edge_cases():
    """{name: (points, radius, same_tile)}"""
    cases = {}
    for order in ("ascending", "reversed", "shuffled"):
        pts, r = tile_bridge(order)
        cases["tile bridge %s, same tile" % order] = (pts, r, True)
        cases["tile bridge %s, any tile" % order] = (pts, r, False)
    twins = tile_twins()
    above = float(np.nextafter(0.25, 1))
    cases["tile twins, r one step above, same tile"] = (twins, above, True)
    cases["tile twins, r one step above, any tile"] = (twins, above, False)
    cases["tile twins, r = spacing, same tile"] = (twins, 0.25, True)
    cases["tile twins, r = spacing, any tile"] = (twins, 0.25, False)
    pts, r = tile_chains()
    cases["tile chains, same tile"] = (pts, r, True)
    cases["tile chains, any tile"] = (pts, r, False)
    pts, r, _ = non_finite(False)
    cases["non-finite"] = (pts, r, False)
    pts, r, _ = non_finite(True)
    cases["non-finite, same tile"] = (pts, r, True)
    cases["all NaN"] = (as_points(np.full((70, 3), np.nan)), 0.5, False)
    xyz = random_xyz()
    cases["radius of many cells"] = (as_points(xyz), 3.0 * len(xyz) ** (-1.0 / 3.0), False)
    cases["far outliers, r = 0.08"] = (far_outliers(), 0.08, False)
    cases["far outliers, r = 1e30"] = (far_outliers(), 1e30, False)
    cases["translated"] = (translated(), 0.06, False)
    return cases


@functools.lru_cache(maxsize=None)
def edge_answers():
    """(cases, {name: (labels, sizes, the kept points per filter, the number of links)}) by the model, with the constructions held to
    what their names say: a wrong generator fails here, without a GPU (tests/test_cluster_model.py calls this too)"""
    cases = edge_cases()
    want = {}
    with np.errstate(over="ignore", invalid="ignore"):
        for name, (pts, radius, same) in cases.items():
            tiles = pts["tile"] if same else None
            labels, sizes = cm.cluster_labels(xyz_of(pts), radius, tiles)
            want[name] = (labels, sizes, [pts[cm.keep_mask(labels, sizes, mp, mc)] for mp, mc in FILTERS], len(cm.links(xyz_of(pts), radius, tiles)))
    # the constructions do what they say
    for order in ("ascending", "reversed", "shuffled"):
        labels, sizes = want["tile bridge %s, same tile" % order][:2]
        assert sorted(sizes.tolist()) == [1, 200, 399], order
        assert sizes.tolist() == {"ascending": [200, 1, 399], "reversed": [399, 1, 200]}.get(order, sizes.tolist()), order
        pts = cases["tile bridge %s, same tile" % order][0]
        assert sizes[labels[pts["tile"] == 2][0]] == 1 and (pts["tile"] == 2).sum() == 1
        assert want["tile bridge %s, any tile" % order][1].tolist() == [600]
    twins = cases["tile twins, r = spacing, any tile"][0]
    labels, sizes = want["tile twins, r one step above, same tile"][:2]
    assert sizes.tolist() == [512, 512, 512] and all(len(set(twins["tile"][labels == c].tolist())) == 1 for c in range(3))
    assert sorted(set(twins["tile"].tolist())) == [0, 128, 255]
    assert want["tile twins, r one step above, any tile"][1].tolist() == [1536]
    assert want["tile twins, r = spacing, same tile"][1].tolist() == [1] * 1536 and want["tile twins, r = spacing, same tile"][3] == 0
    assert want["tile twins, r = spacing, any tile"][1].tolist() == [3] * 512 and want["tile twins, r = spacing, any tile"][3] == 3 * 512
    labels, sizes = want["tile chains, same tile"][:2]
    assert sizes.tolist() == [400, 400] and labels.tolist() == [0, 1] * 400 and want["tile chains, any tile"][1].tolist() == [800]
    for tiles in (False, True):
        pts, radius, bad = non_finite(tiles)
        labels, sizes = want["non-finite, same tile" if tiles else "non-finite"][:2]
        assert np.all(labels[bad] == cm.NONE) and (labels == cm.NONE).sum() == 40 and sizes.sum() == 2960 and 1 < len(sizes) < 2960
        assert not tiles or sorted(set(pts["tile"].tolist())) == [0, 3, 255]
    assert len(want["all NaN"][1]) == 0 and np.all(want["all NaN"][0] == cm.NONE)
    assert want["radius of many cells"][1].tolist() == [4097] and want["radius of many cells"][3] > 30 * 4097
    labels, sizes = want["far outliers, r = 0.08"][:2]
    far = labels[1500:1506]
    assert far[0] == far[5] and sizes[far[0]] == 2 and np.all(sizes[far[1:5]] == 1) and len(set(far.tolist())) == 5
    labels, sizes = want["far outliers, r = 1e30"][:2]
    assert sorted(sizes.tolist()) == [1, 1, 1, 3003] and np.all(sizes[labels[1502:1505]] == 1)
    pts = cases["translated"][0]
    assert len(np.unique(pts["x"])) <= 513 and len(np.unique(pts["y"])) <= 1025 and len(np.unique(pts["z"])) <= 1025     # coordinates tie
    sizes = want["translated"][1]
    assert 1 < len(sizes) < 4000 and sizes.max() > 20
    return cases, want


@pytest.fixture(scope="module")
def edge_model():
    return edge_answers()


_EDGE_CHILD = r"""
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
    s = cw.cwipc_hip_cluster_link_stats(pc, radius, same)
    out["stats_%d" % c] = np.array([s["links"], s["unions"], s["find_loads"], s["max_loads_one_union"]], dtype=np.uint64)
    pc.free()
np.savez(sys.argv[3], **out)
"""


@pytest.mark.parametrize("env", [{}, {"CWIPC_SOR_SMALL_CELLS": "0"}, {"CWIPC_SOR_SPARSE": "1"}], ids=["small clouds", "dense", "sparse"])
def test_each_flow(gpu, edge_model, env, tmp_path):
    cases, want = edge_model
    inp, out = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    arrays = {"ncases": np.array(len(cases)), "filters": np.array(FILTERS)}
    for c, (pts, radius, same) in enumerate(cases.values()):
        arrays["pts_%d" % c], arrays["radius_%d" % c], arrays["same_%d" % c] = pts, np.float64(radius), np.array(same)
    np.savez(inp, **arrays)
    subprocess.run([sys.executable, "-c", _EDGE_CHILD, ROOT, inp, out], check=True, timeout=300, env=dict(os.environ, **env))
    got = np.load(out)
    for c, name in enumerate(cases):
        labels, sizes, kept, nlinks = want[name]
        assert got["labels_%d" % c].dtype == np.uint32 and got["sizes_%d" % c].dtype == np.uint32
        assert np.array_equal(got["sizes_%d" % c], sizes), (env, name, len(got["sizes_%d" % c]), len(sizes))
        assert np.array_equal(got["labels_%d" % c], labels), (env, name)
        for k in range(len(FILTERS)):
            assert got["kept_%d_%d" % (c, k)].tobytes() == kept[k].tobytes(), (env, name, FILTERS[k])
        links, unions, loads, deepest = (int(v) for v in got["stats_%d" % c])
        assert links == nlinks, (env, name, links, nlinks)
        assert 0 <= unions <= links and (unions > 0) == (links > 0), (env, name, unions, links)
        assert deepest <= loads, (env, name, deepest, loads)


# ---------------------------------------------------------------------------
# scale: 2^20 points, 424 919 clusters
# ---------------------------------------------------------------------------
_SCALE_CHILD = r"""
import sys, time, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import torch  # noqa: F401
import cwipc_util_amd as cw
from conftest import make_cloud
cw.cwipc_hip_set_device(0)
d = np.load(sys.argv[2])
radius = float(d["radius"])
t0 = time.perf_counter()
pc = make_cloud(cw, d["pts"])
labels, sizes = cw.cwipc_cluster_labels(pc, radius)
np.save(sys.argv[3] + "/labels.npy", labels)
np.save(sys.argv[3] + "/sizes.npy", sizes)
for k, (mp, mc) in enumerate(d["filters"]):
    kept = cw.cwipc_cluster_filter(pc, radius, int(mp), int(mc))
    np.save(sys.argv[3] + "/kept_%d.npy" % k, kept.get_numpy_array())
    kept.free()
pc.free()
print("scale child: %d points, %d clusters, %.2f s on the device and in copies" % (len(labels), len(sizes), time.perf_counter() - t0))
"""


@functools.lru_cache(maxsize=None)
def scale_case():
    """(points, radius, the model's labels and sizes, the model's seconds) of test_scale, held to its purpose without a GPU"""
    rng = np.random.default_rng(11)
    side, step, radius = 102, 0.01, 0.0085
    g = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    xyz = ((g + rng.uniform(-0.3, 0.3, g.shape)) * step).astype(np.float32)
    pts = as_points(xyz[rng.permutation(len(xyz))])
    n = len(pts)
    t0 = time.perf_counter()
    labels, sizes = cm.cluster_labels(xyz_of(pts), radius)
    t_model = time.perf_counter() - t0
    C = len(sizes)
    assert n == 1061208 and n > 4096 * 256 and C > 262144 and sizes.max() > 8, (n, C)     # the case is as large as its purpose needs
    return pts, radius, labels, sizes, t_model


def test_scale(gpu, tmp_path):
    """The 102^3 lattice of spacing 0.01, jittered by +-0.3 of a step and shuffled, r = 0.0085: 1 061 208 points, so that the sparse
    flow selects itself and cluster_init, cluster_roots (its ballot loop included), cluster_label, cluster_keep and cluster_rank_flag
    go round their grid-stride loops a second time (4096 workgroups of 256 cover 1 048 576); more than 262 144 clusters, so that
    cluster_rank_hist (1024 workgroups of 256) does too."""
    pts, radius, labels, sizes, t_model = scale_case()
    n, C = len(pts), len(sizes)
    filters = [(1, 0), (3, 1000), (1, 262145), (2, 1), (1, C - 1)]
    inp = str(tmp_path / "in.npz")
    np.savez(inp, pts=pts, radius=np.float64(radius), filters=np.array(filters))
    t0 = time.perf_counter()
    # time limit: three times the first measured run -- 3.4 s for this test on an MI355X, of which the model 0.8 s and the child
    # process 2.4 s (0.15 s from the upload to the last filtered cloud; the rest is the interpreter's start and the files)
    subprocess.run([sys.executable, "-c", _SCALE_CHILD, ROOT, inp, str(tmp_path)], check=True, timeout=10, env=dict(os.environ))
    print("scale: model %.2f s (%d clusters, the largest of %d), child process %.2f s" % (t_model, C, int(sizes.max()), time.perf_counter() - t0))
    got_sizes = np.load(str(tmp_path / "sizes.npy"))
    assert np.array_equal(got_sizes, sizes), (len(got_sizes), C)
    assert np.array_equal(np.load(str(tmp_path / "labels.npy")), labels)
    for k, (mp, mc) in enumerate(filters):
        assert np.load(str(tmp_path / ("kept_%d.npy" % k))).tobytes() == pts[cm.keep_mask(labels, sizes, mp, mc)].tobytes(), (mp, mc)


# ---------------------------------------------------------------------------
# contention and crowded cells (in this process)
# ---------------------------------------------------------------------------
def isolated(count, spacing, corner):
    """`count` points of a lattice: each `spacing` from its nearest neighbours, in the box that begins at `corner`"""
    side = int(np.ceil(count ** (1.0 / 3.0)))
    return lattice(side, spacing, corner)[:count]


def ball(rng, count, centre, diameter):
    """`count` points inside the ball (float32 rounding stays far inside the 2 % that the callers leave to the radius)"""
    d = rng.normal(size=(count, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (np.array(centre) + d * (0.5 * diameter * rng.uniform(0, 1, (count, 1)) ** (1.0 / 3.0))).astype(np.float32)


def test_clique(gpu):
    """3000 points of which every pair is linked (4.5 M unions asked of one root), shuffled among 2000 isolated points."""
    rng = np.random.default_rng(3000)
    xyz = np.concatenate([ball(rng, 3000, (0, 0, 0), 0.049), isolated(2000, 0.1, (1.0, 1.0, 1.0))])
    perm = rng.permutation(len(xyz))
    pts = as_points(xyz[perm])
    assert len(cm.links(xyz[:3000], 0.05)) == 3000 * 2999 // 2
    labels, sizes = check(gpu, pts, 0.05, filters=((1, 0), (2, 0), (1, 1), (1, 2), (3000, 1), (3001, 0)))
    assert len(sizes) == 2001 and sorted(sizes.tolist())[-2:] == [1, 3000]
    pc = make_cloud(gpu, pts)
    one, two = gpu.cwipc_cluster_labels(pc, 0.05), gpu.cwipc_cluster_labels(pc, 0.05)
    assert one[0].tobytes() == two[0].tobytes() == labels.tobytes() and one[1].tobytes() == two[1].tobytes() == sizes.tobytes()
    k1, k2 = gpu.cwipc_cluster_filter(pc, 0.05, 2, 1), gpu.cwipc_cluster_filter(pc, 0.05, 2, 1)
    assert k1.count() == 3000 and k1.get_numpy_array().tobytes() == k2.get_numpy_array().tobytes()
    for c in (k1, k2, pc):
        c.free()


def test_many_duplicates_in_one_cell(gpu):
    rng = np.random.default_rng(4096)
    xyz = np.concatenate([np.tile(np.float32([[0.5, 0.25, 0.75]]), (4096, 1)), isolated(500, 0.1, (1.0, 1.0, 1.0))])
    pts = as_points(xyz[rng.permutation(len(xyz))])
    labels, sizes = check(gpu, pts, 1e-6, filters=((1, 0), (2, 0), (1, 1), (1, 2), (4096, 0), (4097, 0)))
    assert sorted(sizes.tolist()) == [1] * 500 + [4096]


def test_halving_order(gpu):
    """A chain of 20 000 whose index order is the bit reversal of position: neighbours in space are far apart in index at every scale,
    so unions merge trees pairwise level by level instead of extending one."""
    n, r = 20000, 0.01
    k = np.arange(1 << 15)
    rev = np.zeros_like(k)
    for b in range(15):
        rev |= ((k >> b) & 1) << (14 - b)
    pos = rev[rev < n]
    assert len(pos) == n and np.array_equal(np.sort(pos), np.arange(n)) and pos[:4].tolist() == [0, 16384, 8192, 4096]
    xyz = np.zeros((n, 3))
    xyz[:, 0] = pos * (0.9 * r)
    labels, sizes = check(gpu, as_points(xyz), r)
    assert sizes.tolist() == [n] and not labels.any()


def test_a_cluster_of_68921(gpu):
    """The 41^3 lattice is one cluster of 0x10D39 points: with 300 singletons and three clumps of 300, the public filter's radix
    selection has data in its third byte."""
    rng = np.random.default_rng(41)
    clumps = [ball(rng, 300, centre, 0.009) for centre in ((2.0, 0, 0), (0, 2.0, 0), (0, 0, 2.0))]
    xyz = np.concatenate([lattice(41, 0.01, (0.0, 0.0, 0.0)), isolated(300, 0.05, (3.0, 3.0, 3.0))] + clumps)
    pts = as_points(xyz[rng.permutation(len(xyz))])
    labels, sizes = check(gpu, pts, 0.011, filters=((1, 1), (1, 2), (1, 4), (301, 0)))
    assert sorted(sizes.tolist()) == [1] * 300 + [300] * 3 + [68921]


# ---------------------------------------------------------------------------
# the ranking kernels on chosen sizes: all four bytes of the radix selection
# ---------------------------------------------------------------------------
def rank_check(gpu, sizes, min_points, max_clusters):
    sizes = np.asarray(sizes, dtype=np.uint32)
    got = gpu.cwipc_hip_cluster_rank_keep(sizes, min_points, max_clusters)
    want = cm.keep_mask(np.arange(len(sizes), dtype=np.uint32), sizes, min_points, max_clusters)
    assert got.dtype == bool and np.array_equal(got, want), (len(sizes), min_points, max_clusters, int(got.sum()), int(want.sum()),
                                                             np.flatnonzero(got != want)[:5].tolist())


def test_rank_random_words(gpu):
    C = 300000
    sizes = np.random.default_rng(300000).integers(0, 2 ** 32, C, dtype=np.uint64).astype(np.uint32)
    for mc in (1, 2, 255, 256, 257, 12345, C - 1, C, C + 1, 2 ** 32 - 1):
        for mp in (1, 2 ** 31, 2 ** 40):
            rank_check(gpu, sizes, mp, mc)
    rank_check(gpu, sizes, 2 ** 31, 0)


@pytest.mark.parametrize("value", [1, 0x01000000, 0xFFFFFFFF])
def test_rank_all_equal(gpu, value):
    """Every cluster of one size: the number alone decides."""
    C = 5000
    for mc in (1, C // 2, C - 1):
        rank_check(gpu, np.full(C, value, dtype=np.uint32), 1, mc)


@pytest.mark.parametrize("byte", [0, 1, 2, 3])
def test_rank_one_byte_differs(gpu, byte):
    """Sizes that differ in one byte only, the other three 0xA5: 40 of each of the 256 values, the limit inside a run of equals."""
    rng = np.random.default_rng(byte)
    v = np.repeat(np.arange(256, dtype=np.uint32), 40)
    sizes = (np.uint32(0xA5A5A5A5) & ~np.uint32(0xFF << (8 * byte))) | (v[rng.permutation(len(v))] << np.uint32(8 * byte))
    for mc in (1, 17, 40, 41, 40 * 100 + 7, 40 * 255 + 39, len(v) - 1):
        rank_check(gpu, sizes, 1, mc)


@pytest.mark.parametrize("T", [0x00010000, 0x01000000, 0x80000000])
def test_rank_around_a_carry(gpu, T):
    """T - 1, T and T + 1 interleaved, 300 of each: T - 1 differs from T in every byte below the carry.  need = 1, the middle, all."""
    sizes = np.tile(np.array([T - 1, T, T + 1], dtype=np.uint64), 300).astype(np.uint32)
    sizes = sizes[np.random.default_rng(T % 1000).permutation(len(sizes))]
    for mc in (299, 300, 301, 450, 599, 600, 601, 899):
        for mp in (1, T, T + 1):
            rank_check(gpu, sizes, mp, mc)


@pytest.mark.parametrize("C", [1, 2, 255, 256, 257, 262144, 262145])
def test_rank_counts(gpu, C):
    """The histogram's launch holds 262 144 clusters in one trip of its loop."""
    sizes = np.random.default_rng(C).integers(1, 2 ** 32, C, dtype=np.uint64).astype(np.uint32)
    sizes[C // 2:] = sizes[:C - C // 2]     # every value twice (all but one for an odd C)
    for mc in sorted({1, max(C // 2, 1), max(C - 1, 1), C, C + 1}):
        rank_check(gpu, sizes, 1, mc)
    rank_check(gpu, sizes, 2 ** 31, 0)


def test_rank_zero_sizes(gpu):
    """No cloud produces a cluster of size 0; the entry ranks it last all the same."""
    sizes = np.random.default_rng(0).integers(0, 4, 1000).astype(np.uint32) * np.uint32(0x00800000)
    assert (sizes == 0).sum() > 100
    for mc in (1, 500, int((sizes > 0).sum()), int((sizes > 0).sum()) + 1, 999, 1000):
        for mp in (0, 1):
            rank_check(gpu, sizes, mp, mc)
    rank_check(gpu, np.zeros(300, dtype=np.uint32), 0, 7)
    assert gpu.cwipc_hip_cluster_rank_keep(np.zeros(0, dtype=np.uint32), 1, 1).shape == (0,)


# ---------------------------------------------------------------------------
# radius extremes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("radius,want", [(1e-170, [1] * 60), (1e-160, [1] * 50 + [10]), (1e-150, [1] * 50 + [10]), (1e-30, [1] * 50 + [10]),
                                         (1e160, [60]), (1e200, [60])])
def test_radius_extremes(gpu, radius, want):
    """r2 = radius * radius in float64 is 0 below about 1.5e-162 (nothing links, not even identical coordinates), subnormal at 1e-160,
    and inf above about 1.3e154 (every pair of finite points links)."""
    rng = np.random.default_rng(60)
    base = rng.uniform(0, 1, (51, 3)).astype(np.float32)
    xyz = np.concatenate([base[:50], np.tile(base[50:], (10, 1))])[rng.permutation(60)]     # 50 points and 10 copies of another
    assert len(np.unique(xyz, axis=0)) == 51
    assert (radius * radius == 0.0) == (radius == 1e-170) and np.isinf(radius * radius) == (radius >= 1e160)
    with np.errstate(over="ignore", under="ignore"):     # (the model squares the radius as the library does)
        labels, sizes = check(gpu, as_points(xyz), radius)
    assert sorted(sizes.tolist()) == want


# ---------------------------------------------------------------------------
# host state
# ---------------------------------------------------------------------------
def test_dirty_pool(gpu):
    """The work block comes from the pool uncleared, and the parents' words are used again for the ranks among equals: a big cloud,
    then a small one, limits on and off, nothing freed in between."""
    big = as_points(random_xyz())
    small = as_points(np.random.default_rng(300).uniform(0, 1, (300, 3)).astype(np.float32), seed=3)
    rb, rs = 1.0 * 4097 ** (-1.0 / 3.0), 0.9 * 300 ** (-1.0 / 3.0)
    wb, ws = cm.cluster_labels(xyz_of(big), rb), cm.cluster_labels(xyz_of(small), rs)
    assert wb[1].max() > 10 and sorted(wb[1].tolist())[-4] >= 2 and len(ws[1]) > 20 and ws[1].max() > 2
    pb, ps = make_cloud(gpu, big), make_cloud(gpu, small)
    results = []

    def filtered(pc, pts, radius, want, mp, mc):
        kept = gpu.cwipc_cluster_filter(pc, radius, mp, mc)
        results.append(kept)
        assert kept.get_numpy_array().tobytes() == pts[cm.keep_mask(want[0], want[1], mp, mc)].tobytes(), (len(pts), mp, mc)

    def labelled(pc, radius, want):
        labels, sizes = gpu.cwipc_cluster_labels(pc, radius)
        assert np.array_equal(sizes, want[1]) and np.array_equal(labels, want[0])

    filtered(pb, big, rb, wb, 1, 3)
    labelled(ps, rs, ws)
    filtered(ps, small, rs, ws, 2, 1)
    filtered(ps, small, rs, ws, 1, 0)
    filtered(pb, big, rb, wb, 1, 2)
    labelled(pb, rb, wb)
    for c in results + [pb, ps]:
        c.free()


def test_device_resident_input(gpu):
    """Clustering a filter's output where it lies."""
    dll = gpu.cwipc_util_dll_load()
    pts = as_points(np.random.default_rng(9000).uniform(0, 1, (9000, 3)).astype(np.float32), tile=1)
    pc = make_cloud(gpu, pts, cellsize=0.001)
    kept, twin = gpu.cwipc_downsample(pc, 0.04), gpu.cwipc_downsample(pc, 0.04)
    assert dll.cwipc_hip_is_device_resident(kept.as_cwipc_p()) == 1
    radius = 0.05
    labels, sizes = gpu.cwipc_cluster_labels(kept, radius)
    out = gpu.cwipc_cluster_filter(kept, radius, 3, 5)
    assert dll.cwipc_hip_is_device_resident(kept.as_cwipc_p()) == 1 and dll.cwipc_hip_is_device_resident(out.as_cwipc_p()) == 1
    after = kept.get_numpy_array()
    assert 1000 < len(after) < 9000 and after.tobytes() == twin.get_numpy_array().tobytes()      # unchanged: what the same call gives again
    wl, ws = cm.cluster_labels(xyz_of(after), radius)
    assert 10 < len(ws) < len(after) and ws.max() >= 3
    assert np.array_equal(sizes, ws) and np.array_equal(labels, wl)
    assert out.get_numpy_array().tobytes() == after[cm.keep_mask(wl, ws, 3, 5)].tobytes()
    assert out.timestamp() == kept.timestamp() and out.cellsize() == kept.cellsize()
    for c in (out, kept, twin, pc):
        c.free()


def test_four_threads(gpu):
    """Four host threads, each with a cloud, a radius and a flag of its own, three rounds of labels and filter each."""
    jobs = []
    for i, (n, factor, same) in enumerate(((3000, 1.0, False), (4097, 0.8, False), (2000, 1.1, True), (1000, 1.3, False))):
        rng = np.random.default_rng(100 + i)
        pts = as_points(rng.uniform(0, 1, (n, 3)).astype(np.float32), tile=rng.integers(0, 3, n).astype(np.uint8), seed=i)
        radius = factor * n ** (-1.0 / 3.0)
        labels, sizes = cm.cluster_labels(xyz_of(pts), radius, pts["tile"] if same else None)
        assert 1 < len(sizes) < n
        jobs.append((pts, radius, same, labels, sizes, pts[cm.keep_mask(labels, sizes, 2, 3)]))
    clouds = [make_cloud(gpu, job[0]) for job in jobs]
    results = [[] for _ in jobs]

    def worker(i):
        gpu.cwipc_hip_set_device(0)
        pts, radius, same = jobs[i][:3]
        for _ in range(3):
            labels, sizes = gpu.cwipc_cluster_labels(clouds[i], radius, same)
            kept = gpu.cwipc_cluster_filter(clouds[i], radius, 2, 3, same)
            results[i].append((labels, sizes, kept.get_numpy_array()))
            kept.free()

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for i, (pts, radius, same, labels, sizes, kept) in enumerate(jobs):
        assert len(results[i]) == 3, i
        for got in results[i]:
            assert np.array_equal(got[1], sizes) and np.array_equal(got[0], labels) and got[2].tobytes() == kept.tobytes(), i
    for c in clouds:
        c.free()
