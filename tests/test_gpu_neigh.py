"""Fixed-radius neighbourhoods on the GPU (RULE N of include/cwipc_util_amd/hip_ext.h): cwipc_radius_counts,
cwipc_radius_outlier_filter and cwipc_smooth against tests/neigh_model.py and the host twin cwipc_hip_smooth_host.

  counts, filter   compared EXACTLY (integer equality, bytes) with the model, every case in one child process per grid flow (small
                   clouds, dense, sparse): the 12^3 lattice at three offsets with r = spacing (every count 0) and one float64 step
                   above (6 / 5 / 4 / 3 by position), the lattice permuted, three tiles per lattice position under SAME_TILE,
                   non-finite points, an all-NaN cloud, 4096 duplicates, a radius of many cells, far outliers out to FLT_MAX, r2 = 0
                   and r2 = inf, a plane with scattered strays; the filter with min_neighbours 0, 1, 6 and 7 on each of them.
  smoothing        the three inputs of neigh_model.SMOOTH_INPUTS through every flow: BYTE-EQUAL to cwipc_hip_smooth_host (the same
                   header text on the host); against the eigh model equal or adjacent where the eigengap allows, with the caps (the
                   argument is in tests/test_smooth_host.py).  In this process: a permuted input, two calls, two sheets of different
                   tiles under SAME_TILE, points that must not move, iterations through the filter class, the noisy plane's rms.
  the 2^18 cap     262144 and 262145 points inside a ball of diameter below the radius: all moved, then none.
  host state       empty clouds, device-resident input, timestamp and cellsize, four host threads."""
import functools
import os
import subprocess
import sys
import threading
import time

import numpy as np
import pytest

from conftest import make_cloud
import neigh_model as nm
from neigh_model import as_points, xyz_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

FLT_MAX = float(np.finfo(np.float32).max)
MIN_NEIGHBOURS = (0, 1, 6, 7)          # the filter's thresholds tried on every flow case
FLOWS = {"small clouds": {}, "dense": {"CWIPC_SOR_SMALL_CELLS": "0"}, "sparse": {"CWIPC_SOR_SPARSE": "1"}}


def lattice(side, spacing, offset):
    g = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    return (g * spacing + np.array(offset)).astype(np.float32)


def lattice_inner(side):
    """per lattice position on how many axes it is not at the border: 3 interior, 2 face, 1 edge, 0 corner"""
    g = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    return ((g > 0) & (g < side - 1)).sum(axis=1)


def plane_with_strays():
    """the first 2500 points of the noisy plane and 60 strays around it, two of them a pair 0.005 apart; shuffled"""
    rng = np.random.default_rng(2560)
    pts, radius = nm.noisy_plane()
    strays = nm.PLANE_ORIGIN + rng.uniform(-1, 1, (60, 3)) + 3.0 * nm.PLANE_NORMAL * rng.choice([-1, 1], (60, 1))
    strays[1] = strays[0] + [0.005, 0, 0]
    both = np.concatenate([pts[:2500], as_points(strays, tile=9, seed=4)])
    return both[rng.permutation(len(both))], radius


OUTLIERS = np.float32([(1e6, 0, 0), (-1e6, .5, .5), (3e38, 0, 0), (-3e38, 3e38, -3e38), (FLT_MAX, FLT_MAX, FLT_MAX), (1e6, 0, 0.05)])


def count_cases():
    """{name: (points, radius, same_tile)}"""
    cases = {}
    above = float(np.nextafter(0.25, 1))
    for offset in ((0.0, 0.0, 0.0), (1.0, 0.5, -1.0), (0.125, -0.375, 0.0625)):
        lat = as_points(lattice(12, 0.25, offset))
        cases["lattice at %s, r = spacing" % (offset,)] = (lat, 0.25, False)
        cases["lattice at %s, one step above" % (offset,)] = (lat, above, False)
    perm = np.random.default_rng(1728).permutation(1728)
    lat = as_points(lattice(12, 0.25, (0.0, 0.0, 0.0)))[perm]
    cases["lattice permuted, r = spacing"] = (lat, 0.25, False)
    cases["lattice permuted, one step above"] = (lat, above, False)
    small = lattice(8, 0.25, (0.0, 0.0, 0.0))
    mix = np.random.default_rng(1536).permutation(1536)
    twins = as_points(np.concatenate([small, small, small])[mix], np.repeat(np.uint8([0, 128, 255]), 512)[mix])
    cases["tile twins, one step above, same tile"] = (twins, above, True)
    cases["tile twins, one step above, any tile"] = (twins, above, False)
    cases["tile twins, r = spacing, same tile"] = (twins, 0.25, True)
    cases["tile twins, r = spacing, any tile"] = (twins, 0.25, False)
    rng = np.random.default_rng(3000)
    xyz = rng.uniform(0, 1, (3000, 3)).astype(np.float32)
    bad = rng.choice(3000, 40, replace=False)
    for k, i in enumerate(bad):
        xyz[i, k % 3] = (np.nan, np.inf, -np.inf)[(k // 3) % 3]
    xyz[bad[0]] = np.nan
    cases["non-finite"] = (as_points(xyz), 1.2 * 3000 ** (-1.0 / 3.0), False)
    cases["non-finite, same tile"] = (as_points(xyz, rng.choice(np.uint8([0, 3, 255]), 3000)), 1.2 * 3000 ** (-1.0 / 3.0), True)
    cases["all NaN"] = (as_points(np.full((70, 3), np.nan)), 0.5, False)
    cases["4096 duplicates"] = (as_points(np.tile(np.float32([[0.3, -1.7, 2.9]]), (4096, 1))), 0.01, False)
    cube = np.random.default_rng(4097).uniform(0, 1, (4097, 3)).astype(np.float32)
    cases["radius of many cells"] = (as_points(cube), 3.0 * 4097 ** (-1.0 / 3.0), False)
    far = as_points(np.concatenate([cube[:1500], OUTLIERS, cube[1500:3000]]))
    cases["far outliers, r = 0.08"] = (far, 0.08, False)
    few = far[1000:2006]              # (a radius beyond the cloud is n * n / 2 pairs for the model too: 1006 points, the outliers at 500 .. 505)
    cases["far outliers, r = 1e30"] = (few, 1e30, False)
    cases["radius 1e-170"] = (as_points(np.concatenate([cube[:500], cube[:500]])), 1e-170, False)
    cases["radius 1e200"] = (few, 1e200, False)
    cases["radius 1e200, same tile"] = (as_points(xyz_of(few), np.arange(len(few)) % 3), 1e200, True)
    pts, radius = plane_with_strays()
    cases["plane with strays"] = (pts, radius, False)
    return cases


@functools.lru_cache(maxsize=None)
def count_answers():
    """(cases, {name: (counts, the kept points per threshold)}) by the model, the constructions held to what their names say"""
    cases = count_cases()
    want = {}
    for name, (pts, radius, same) in cases.items():
        cnt = nm.counts(xyz_of(pts), radius, pts["tile"] if same else None)
        want[name] = (cnt, [pts[nm.keep_mask(xyz_of(pts), cnt, mn)] for mn in MIN_NEIGHBOURS])
    for name in cases:
        if name.startswith("lattice") and "r = spacing" in name:
            assert np.all(want[name][0] == 0) and len(want[name][1][0]) == 1728 and len(want[name][1][1]) == 0, name
        if name.startswith("lattice at") and "one step above" in name:
            assert np.array_equal(want[name][0], 3 + lattice_inner(12)), name
            assert [len(k) for k in want[name][1]] == [1728, 1728, 1000, 0], name
    assert sorted(want["lattice permuted, one step above"][0].tolist()) == sorted((3 + lattice_inner(12)).tolist())
    assert np.all(want["tile twins, r = spacing, same tile"][0] == 0) and np.all(want["tile twins, r = spacing, any tile"][0] == 2)
    c = want["tile twins, one step above, same tile"][0]
    assert sorted(set(c.tolist())) == [3, 4, 5, 6] and np.array_equal(want["tile twins, one step above, any tile"][0], 3 * c + 2)
    bad = ~np.isfinite(xyz_of(cases["non-finite"][0])).all(axis=1)
    assert bad.sum() == 40 and np.all(want["non-finite"][0][bad] == 0) and want["non-finite"][0].max() > 6
    assert len(want["non-finite"][1][0]) == 2960 and np.all(want["all NaN"][0] == 0) and len(want["all NaN"][1][0]) == 0
    assert np.all(want["4096 duplicates"][0] == 4095)
    c = want["radius of many cells"][0]      # 113 in a ball of three spacings, an eighth of that at a corner
    assert c.min() >= 5 and 60 < np.median(c) < 113 and c.max() < 250
    far = want["far outliers, r = 0.08"][0][1500:1506]
    assert far.tolist() == [1, 0, 0, 0, 0, 1]
    assert np.all(want["radius 1e-170"][0] == 0) and len(want["radius 1e-170"][1][0]) == 1000
    assert np.all(want["radius 1e200"][0] == 1005)      # (3 * FLT_MAX^2 is far from overflowing a double)
    c = want["far outliers, r = 1e30"][0]
    assert c[502:505].tolist() == [0, 0, 0] and np.all(np.delete(c, [502, 503, 504]) == 1002)
    assert sorted(set(want["radius 1e200, same tile"][0].tolist())) == [334, 335]
    c, kept = want["plane with strays"]
    stray = cases["plane with strays"][0]["tile"] == 9
    assert stray.sum() == 60 and sorted(c[stray].tolist()) == [0] * 58 + [1, 1] and np.median(c[~stray]) >= 6
    assert [len(k) for k in kept[:2]] == [2560, 2502] and np.all(kept[3]["tile"] != 9)
    return cases, want


@functools.lru_cache(maxsize=None)
def smooth_inputs():
    """{name: (points, radius, the host twin's bytes)}: cwipc_hip_smooth_host, which runs csrc/smooth_terms.hpp on the host"""
    import cwipc_util_amd as cw
    res = {}
    for name, (make, _) in nm.SMOOTH_INPUTS.items():
        pts, radius = make()
        res[name] = (pts, radius, cw.cwipc_hip_smooth_host(pts, radius))
    return res


_CHILD = r"""
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
    out["counts_%d" % c] = cw.cwipc_radius_counts(pc, radius, same)
    for k, mn in enumerate(d["thresholds"]):
        kept = cw.cwipc_radius_outlier_filter(pc, radius, int(mn), same)
        out["kept_%d_%d" % (c, k)] = kept.get_numpy_array()
        kept.free()
    pc.free()
for c in range(int(d["nsmooth"])):
    pc = make_cloud(cw, d["spts_%d" % c])
    res = cw.cwipc_smooth(pc, float(d["sradius_%d" % c]))
    out["smooth_%d" % c] = res.get_numpy_array()
    res.free()
    pc.free()
np.savez(sys.argv[3], **out)
"""

_flow_cache = {}


@pytest.fixture(scope="module")
def flow(gpu, tmp_path_factory):
    """flow(name) -> what the child process of that grid flow computed for every case, each child run once"""
    def run(name):
        if name not in _flow_cache:
            cases, _ = count_answers()
            tmp = tmp_path_factory.mktemp("neigh_flow")
            inp, out = str(tmp / "in.npz"), str(tmp / "out.npz")
            arrays = {"ncases": np.array(len(cases)), "thresholds": np.array(MIN_NEIGHBOURS), "nsmooth": np.array(len(smooth_inputs()))}
            for c, (pts, radius, same) in enumerate(cases.values()):
                arrays["pts_%d" % c], arrays["radius_%d" % c], arrays["same_%d" % c] = pts, np.float64(radius), np.array(same)
            for c, (pts, radius, _) in enumerate(smooth_inputs().values()):
                arrays["spts_%d" % c], arrays["sradius_%d" % c] = pts, np.float64(radius)
            np.savez(inp, **arrays)
            subprocess.run([sys.executable, "-c", _CHILD, ROOT, inp, out], check=True, timeout=300, env=dict(os.environ, **FLOWS[name]))
            _flow_cache[name] = dict(np.load(out))
        return _flow_cache[name]
    return run


# ---------------------------------------------------------------------------
# counts and the radius outlier filter: exact
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FLOWS))
def test_counts_each_flow(flow, name):
    cases, want = count_answers()
    got = flow(name)
    for c, case in enumerate(cases):
        counts = got["counts_%d" % c]
        assert counts.dtype == np.uint32 and np.array_equal(counts, want[case][0]), (name, case, np.flatnonzero(counts != want[case][0])[:5])


@pytest.mark.parametrize("name", list(FLOWS))
def test_radius_outlier_filter_each_flow(flow, name):
    cases, want = count_answers()
    got = flow(name)
    for c, case in enumerate(cases):
        for k, mn in enumerate(MIN_NEIGHBOURS):
            assert got["kept_%d_%d" % (c, k)].tobytes() == want[case][1][k].tobytes(), (name, case, mn)


def test_filter_metadata_empty_and_device_resident_input(gpu):
    dll = gpu.cwipc_util_dll_load()
    pts, radius = plane_with_strays()
    pc = make_cloud(gpu, pts, cellsize=0.0078125, timestamp=4711)
    kept = gpu.cwipc_radius_outlier_filter(pc, radius, 6)
    assert (kept.timestamp(), kept.cellsize()) == (4711, 0.0078125) and dll.cwipc_hip_is_device_resident(kept.as_cwipc_p()) == 1
    assert kept.get_numpy_array().tobytes() == nm.radius_outlier_filter(pts, radius, 6).tobytes()
    smoothed = gpu.cwipc_smooth(pc, radius)
    assert (smoothed.timestamp(), smoothed.cellsize(), smoothed.count()) == (4711, 0.0078125, len(pts))
    assert dll.cwipc_hip_is_device_resident(smoothed.as_cwipc_p()) == 1
    # a filter's output where it lies: counts, filter and smoothing of the device-resident result
    sub = gpu.cwipc_radius_outlier_filter(pc, radius, 1)
    assert dll.cwipc_hip_is_device_resident(sub.as_cwipc_p()) == 1
    counts, again, smooth2 = gpu.cwipc_radius_counts(sub, radius), gpu.cwipc_radius_outlier_filter(sub, radius, 8), gpu.cwipc_smooth(sub, radius, 3)
    after = sub.get_numpy_array()
    assert after.tobytes() == nm.radius_outlier_filter(pts, radius, 1).tobytes()
    assert np.array_equal(counts, nm.counts(xyz_of(after), radius))
    assert again.get_numpy_array().tobytes() == nm.radius_outlier_filter(after, radius, 8).tobytes()
    assert smooth2.get_numpy_array().tobytes() == gpu.cwipc_hip_smooth_host(after, radius, 3).tobytes()
    # empty in, empty out
    empty = make_cloud(gpu, pts[:0], cellsize=0.5, timestamp=99)
    assert len(gpu.cwipc_radius_counts(empty, radius)) == 0
    for res in (gpu.cwipc_radius_outlier_filter(empty, radius, 1), gpu.cwipc_smooth(empty, radius)):
        assert (res.count(), res.timestamp(), res.cellsize()) == (0, 99, 0.5)
        res.free()
    # a cap below the cloud's count is refused
    small = np.zeros(10, dtype=np.uint32)
    assert dll.cwipc_hip_radius_counts(pc.as_cwipc_p(), radius, 0, small.ctypes.data, 10) == -1
    for c in (kept, smoothed, sub, again, smooth2, empty, pc):
        c.free()


# ---------------------------------------------------------------------------
# smoothing
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FLOWS))
def test_smoothing_each_flow(flow, name):
    """The output is byte-equal to the host twin (the same header text; f64 division and square root are correctly rounded on both
    sides, contraction is off), and equal or adjacent to the eigh model where the eigengap allows, with the caps."""
    got = flow(name)
    for c, (case, (pts, radius, twin)) in enumerate(smooth_inputs().items()):
        res = got["smooth_%d" % c]
        differ = np.flatnonzero((xyz_of(res).view(np.uint32) != xyz_of(twin).view(np.uint32)).any(axis=1)) if len(res) == len(twin) else None
        print("%s, %s: %s points differ from the host twin" % (name, case, "?" if differ is None else len(differ)))
        nm.check_against_model("%s, %s" % (name, case), pts, res, radius, cap=nm.SMOOTH_INPUTS[case][1])
        assert res.tobytes() == twin.tobytes(), (name, case, None if differ is None else differ[:5])


def test_noisy_plane_rms(gpu):
    pts, radius, twin = smooth_inputs()["noisy plane"]
    pc = make_cloud(gpu, pts)
    res = gpu.cwipc_smooth(pc, radius)
    before, after, model = nm.plane_rms(xyz_of(pts)), nm.plane_rms(xyz_of(res.get_numpy_array())), nm.plane_rms(xyz_of(nm.smooth(pts, radius)[0]))
    print("noisy plane: rms distance to the true plane %.6e before, %.15e after, the model's %.15e" % (before, after, model))
    assert after < before
    assert abs(after - model) <= 1e-12 * model
    res.free()
    pc.free()


def test_permuted_input_and_two_calls(gpu):
    """Permuting the input permutes the output byte for byte (what the integer sums buy); two calls give the same bytes."""
    rng = np.random.default_rng(8)
    for name, (pts, radius, twin) in smooth_inputs().items():
        perm = rng.permutation(len(pts))
        pc, pp = make_cloud(gpu, pts), make_cloud(gpu, pts[perm])
        a, b, c = gpu.cwipc_smooth(pc, radius), gpu.cwipc_smooth(pc, radius), gpu.cwipc_smooth(pp, radius)
        first = a.get_numpy_array()
        assert first.tobytes() == b.get_numpy_array().tobytes(), name
        assert c.get_numpy_array().tobytes() == first[perm].tobytes(), name
        for cloud in (a, b, c, pc, pp):
            cloud.free()


def test_two_sheets_of_different_tiles(gpu):
    """Two sheets 0.3 r apart, tiles 3 and 200: with SAME_TILE each is smoothed as if alone."""
    pts, radius = nm.noisy_plane()
    a = pts[:2000].copy()
    b = a.copy()
    a["tile"], b["tile"] = 3, 200
    for f, v in zip("xyz", 0.3 * radius * nm.PLANE_NORMAL):
        b[f] = (b[f].astype(np.float64) + v).astype(np.float32)
    mix = np.random.default_rng(4000).permutation(4000)
    both = np.concatenate([a, b])[mix]
    clouds = [make_cloud(gpu, p) for p in (both, a, b)]
    same, alone_a, alone_b, any_tile = (gpu.cwipc_smooth(clouds[0], radius, 2, True), gpu.cwipc_smooth(clouds[1], radius),
                                        gpu.cwipc_smooth(clouds[2], radius), gpu.cwipc_smooth(clouds[0], radius, 2, False))
    back = np.empty_like(both)
    back[mix] = same.get_numpy_array()
    assert back[:2000].tobytes() == alone_a.get_numpy_array().tobytes() and back[2000:].tobytes() == alone_b.get_numpy_array().tobytes()
    assert same.get_numpy_array().tobytes() == gpu.cwipc_hip_smooth_host(both, radius, 2, True).tobytes()
    mixed = any_tile.get_numpy_array()
    assert mixed.tobytes() != same.get_numpy_array().tobytes() and mixed.tobytes() == gpu.cwipc_hip_smooth_host(both, radius, 2, False).tobytes()
    for c in clouds + [same, alone_a, alone_b, any_tile]:
        c.free()


def test_points_that_keep_their_bytes(gpu):
    """Fewer than three neighbours, non-finite coordinates, min_neighbours above every count."""
    pts, radius = nm.noisy_plane()
    pts = pts[:3000].copy()
    pts["x"][10], pts["y"][20], pts["z"][30] = np.nan, np.inf, -np.inf
    pts[11] = pts[12]
    pts["x"][11], pts["z"][12] = np.nan, np.nan                # (a NaN with the other coordinates of a neighbour)
    pts["x"][40:43] += 5.0                                     # three lonely points ...
    pts["y"][41], pts["y"][42] = pts["y"][41] + 1.0, pts["y"][42] + 2.0
    pts[50] = pts[40]
    pts["z"][50] += np.float32(0.001)                          # ... one of them with one neighbour,
    pts[60:62] = pts[41]
    pts["x"][60], pts["y"][61] = pts["x"][60] + np.float32(0.002), pts["y"][61] + np.float32(0.002)     # one with two
    pc = make_cloud(gpu, pts)
    res = gpu.cwipc_smooth(pc, radius).get_numpy_array()
    moved, _, _ = nm.check_against_model("odd points", pts, res, radius)
    assert not moved[[10, 20, 30, 11, 12, 40, 50, 42]].any() and moved[[41, 60, 61]].all()
    still = [10, 20, 30, 11, 12, 40, 50, 42]
    assert res[still].tobytes() == pts[still].tobytes()
    assert res.tobytes() == gpu.cwipc_hip_smooth_host(pts, radius).tobytes()
    cnt = nm.counts(xyz_of(pts), radius)
    for mn in (int(cnt.max()), int(cnt.max()) + 1, 2 ** 32 - 1):
        res = gpu.cwipc_smooth(pc, radius, mn).get_numpy_array()
        want = gpu.cwipc_hip_smooth_host(pts, radius, mn)
        assert res.tobytes() == want.tobytes() and (res.tobytes() == pts.tobytes()) == (mn > cnt.max()), mn
    pc.free()


def test_iterations_through_the_filter_class(gpu):
    from cwipc_util_amd import filters
    pts, radius, twin = smooth_inputs()["noisy sphere"]
    pc = make_cloud(gpu, pts, cellsize=0.25, timestamp=77)
    f = filters.factory("smooth(%r, 2, 3)" % radius)
    got = f.filter(pc)
    step = pc
    for _ in range(3):
        step = gpu.cwipc_smooth(step, radius)
    want = pts
    for _ in range(3):
        want = gpu.cwipc_hip_smooth_host(want, radius)
    res = got.get_numpy_array()
    assert res.tobytes() == step.get_numpy_array().tobytes() and res.tobytes() == want.tobytes() and res.tobytes() != twin.tobytes()
    assert (got.timestamp(), got.cellsize()) == (77, 0.25)
    one = filters.factory("smooth(%r)" % radius).filter(pc)
    assert one.get_numpy_array().tobytes() == twin.tobytes()
    g = filters.factory("radius_outliers(%r, 20)" % radius)
    assert g.filter(pc).get_numpy_array().tobytes() == nm.radius_outlier_filter(pts, radius, 20).tobytes()
    f.statistics()
    g.statistics()


def test_four_host_threads(gpu):
    jobs = []
    for k, (name, (pts, radius, twin)) in enumerate(list(smooth_inputs().items()) + [("plane again", smooth_inputs()["noisy plane"])]):
        jobs.append((pts, radius, twin, nm.counts(xyz_of(pts), radius), nm.radius_outlier_filter(pts, radius, 10 + k)))
    clouds = [make_cloud(gpu, j[0]) for j in jobs]
    results = [[] for _ in jobs]

    def worker(i):
        gpu.cwipc_hip_set_device(0)
        for _ in range(3):
            counts = gpu.cwipc_radius_counts(clouds[i], jobs[i][1])
            kept = gpu.cwipc_radius_outlier_filter(clouds[i], jobs[i][1], 10 + i)
            res = gpu.cwipc_smooth(clouds[i], jobs[i][1])
            results[i].append((counts, kept.get_numpy_array(), res.get_numpy_array()))

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for i, (pts, radius, twin, counts, kept) in enumerate(jobs):
        assert len(results[i]) == 3, i
        for got_counts, got_kept, got_smooth in results[i]:
            assert np.array_equal(got_counts, counts) and got_kept.tobytes() == kept.tobytes() and got_smooth.tobytes() == twin.tobytes(), i


# ---------------------------------------------------------------------------
# the 2^18 cap on the device
# ---------------------------------------------------------------------------
_CAP_CHILD = r"""
import sys, time, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import torch  # noqa: F401
import cwipc_util_amd as cw
from conftest import make_cloud
cw.cwipc_hip_set_device(0)
pts = np.load(sys.argv[2])
pc = make_cloud(cw, pts)
t0 = time.perf_counter()
res = cw.cwipc_smooth(pc, float(sys.argv[4]))
out = res.get_numpy_array()
print("cap child: %d points, %.2f s from the call to the result on the host" % (len(pts), time.perf_counter() - t0))
np.save(sys.argv[3], out)
"""


def flat_ball(n):
    """n points inside the ellipsoid of half axes 0.3, 0.3, 0.06 around (1, 2, 3): every pair is closer than r = 1"""
    rng = np.random.default_rng(n)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d *= rng.uniform(0, 1, (n, 1)) ** (1.0 / 3.0)
    return as_points(np.array([1.0, 2.0, 3.0]) + d * [0.3, 0.3, 0.06]), 1.0


@pytest.mark.parametrize("n", [262144, 262145])
def test_the_cap_of_2_to_18_neighbours(gpu, tmp_path, n):
    """262144 points that are all neighbours of one another: every point moves (cnt = 2^18: the sums are still exact).  One point
    more: none does, the cloud comes back bit for bit.  n * n = 7e10 pair tests per call, run once each in a child under a time limit
    (the first measured run on an MI355X: 0.55 s from the call to the result on the host, either case)."""
    pts, radius = flat_ball(n)
    xyz = xyz_of(pts).astype(np.float64)
    assert np.linalg.norm(xyz.max(axis=0) - xyz.min(axis=0)) < 0.95 * radius          # the box's diagonal: every pair is within r
    inp, out = str(tmp_path / "in.npy"), str(tmp_path / "out.npy")
    np.save(inp, pts)
    subprocess.run([sys.executable, "-c", _CAP_CHILD, ROOT, inp, out, repr(radius)], check=True, timeout=60, env=dict(os.environ))
    got = np.load(out)
    for f in ("r", "g", "b", "tile"):
        assert np.array_equal(got[f], pts[f])
    if n > nm.MAX_CNT:
        assert got.tobytes() == pts.tobytes()
        return
    # every point's neighbourhood is the whole ellipsoid, weighted towards the point: the fitted plane is close to the equatorial
    # plane wherever the point lies, so the cloud gets thinner along z; a point stays where it is only if its step rounds to
    # nothing, |n . c| under 1e-7 of a coordinate with |n . c| spread over +-0.06: a share of 1e-6
    changed = (xyz_of(got).view(np.uint32) != xyz_of(pts).view(np.uint32)).any(axis=1)
    assert changed.sum() > 0.99 * n
    step = np.linalg.norm(xyz_of(got).astype(np.float64) - xyz, axis=1)
    assert np.all(step < radius)
    assert xyz_of(got)[:, 2].astype(np.float64).std() < xyz[:, 2].std()
