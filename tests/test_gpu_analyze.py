"""The registration analyzer on the GPU: cwipc_hip_nn_distance, cwipc_hip_gaussian_kde and cwipc_util_amd.registration.analyze
against the reference's own recorded results (tests/golden/analyze_vectors.npz) and the numpy oracle (tests/analyze_oracle.py).

Bars:
  * distances: numpy.array_equal with the golden arrays and with the oracle (inf positions included, no point left out);
  * density curves: at most 100 x kde_cpu_spread (the fixture's record: 6e-15, so 6e-13) of the curve's maximum away from the
    oracle's / the golden curve -- a bound on rounding: another tree of partial sums and the device's exp over up to 2 x 10^6 terms;
  * the analyzer's reductions with use_kde off: exactly the golden numbers (same array, same numpy calls); with use_kde on the
    curve within the bound above and the mode's bin equal (the fixture's generator checked that no recorded curve has its two
    highest values closer than the bound).
"""
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from conftest import make_cloud
import analyze_oracle as ao

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NTHS = (0, 1, 3, 31)
SAMPLED = 30000


@pytest.fixture(scope="module")
def vectors():
    v = np.load(os.path.join(GOLDEN, "analyze_vectors.npz"))
    return v, json.loads(bytes(v["meta_json"]).decode())


def load_distances(v, pair, way, ignore, bound_name):
    full = v[f"{pair}_dist_{way}_n{ignore}_inf"]
    if bound_name == "inf":
        return full
    finite = np.unpackbits(v[f"{pair}_dist_{way}_n{ignore}_cut_finite"])[:len(full)].astype(bool)
    return np.where(finite, full, np.inf)


def clouds_of(v, meta, pair):
    src = v[f"{pair}_source"]
    ref = src if meta["pairs"][pair]["same_cloud"] else v[f"{pair}_reference"]
    return src, ref


def xyz_of(p):
    return np.column_stack([p["x"], p["y"], p["z"]]).astype(np.float32)


def as_points(xyz, tile=1):
    from cwipc_util_amd import cwipc_point_numpy_dtype
    xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    pts = np.zeros(len(xyz), dtype=cwipc_point_numpy_dtype)
    if len(xyz):
        pts["x"], pts["y"], pts["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    pts["tile"] = tile
    return pts


def jittered(pts, seed=0):
    out = pts.copy()
    rng = np.random.default_rng(seed)
    for a in "xyz":
        out[a] = (out[a] + rng.uniform(-1e-5, 1e-5, len(out))).astype(np.float32)
    return out


def check_against_oracle(gpu, src_pts, ref_pts, nths=NTHS, bounds=(np.inf,), seed=0):
    """Bit-equality with the oracle, at every source point or at SAMPLED of them where there are more."""
    src, ref = make_cloud(gpu, src_pts), make_cloud(gpu, ref_pts)
    sx, rx = xyz_of(src_pts), xyz_of(ref_pts)
    q = np.arange(len(sx)) if len(sx) <= SAMPLED else np.sort(np.random.default_rng(seed).choice(len(sx), SAMPLED, replace=False))
    wants = ao.nn_distance2_grid_many(sx[q], rx, nths, bounds, per_cell=48)
    for nth in nths:
        for bound in bounds:
            got = gpu.cwipc_hip_nn_distance(src, ref, nth, bound)
            assert got.shape == (len(sx),) and got.dtype == np.float64
            want = np.sqrt(wants[(nth, bound)])
            assert np.array_equal(got[q], want), (nth, bound, int(np.sum(got[q] != want)))
    src.free()
    ref.free()


# ---------------------------------------------------------------------------
# distances
# ---------------------------------------------------------------------------
def test_distances_equal_the_golden_arrays(gpu, vectors):
    v, meta = vectors
    for pair, rec in meta["pairs"].items():
        sp, rp = clouds_of(v, meta, pair)
        src = make_cloud(gpu, sp)
        ref = src if rec["same_cloud"] else make_cloud(gpu, rp)
        for ignore in (0, 1, 3):
            for bound_name in ("inf", "cut"):
                bound = np.inf if bound_name == "inf" else rec["cut"]
                assert np.array_equal(gpu.cwipc_hip_nn_distance(src, ref, ignore, bound), load_distances(v, pair, "fwd", ignore, bound_name)), (pair, ignore, bound_name)
                assert np.array_equal(gpu.cwipc_hip_nn_distance(ref, src, ignore, bound), load_distances(v, pair, "back", ignore, bound_name)), (pair, ignore, bound_name)


@pytest.mark.parametrize("npoints", [36000, 300000])
@pytest.mark.parametrize("jitter", [False, True])
def test_tile_against_tile_of_one_frame(gpu, synth, npoints, jitter):
    pts, _ = synth(2 * npoints)
    if jitter:
        pts = jittered(pts)
    tiles = sorted(set(np.unique(pts["tile"]).tolist()) - {0})
    a, b = pts[pts["tile"] == tiles[0]], pts[pts["tile"] == tiles[1]]
    assert len(a) > npoints // 2 and len(b) > npoints // 2
    check_against_oracle(gpu, a, b, bounds=(np.inf, 0.01))


@pytest.mark.parametrize("npoints", [36000, 300000])
def test_cloud_against_its_transformed_copy(gpu, synth, npoints):
    pts, cs = synth(npoints)
    pts = jittered(pts, 3)
    a = np.radians(0.5)
    m = np.array([[np.cos(a), 0, np.sin(a), 0.003], [0, 1, 0, 0.0], [-np.sin(a), 0, np.cos(a), 0.0], [0, 0, 0, 1.0]])
    moved = gpu.cwipc_transform(make_cloud(gpu, pts, cs), m).get_numpy_array()
    check_against_oracle(gpu, moved, pts, nths=(0, 1))
    check_against_oracle(gpu, pts, moved, nths=(0, 3))


def test_downsampled_against_full(gpu, synth):
    pts, cs = synth(300000)
    down = gpu.cwipc_downsample(make_cloud(gpu, pts, cs), 0.01).get_numpy_array()
    assert 1000 < len(down) < len(pts) // 4
    check_against_oracle(gpu, down, pts, nths=(0, 1, 31))
    check_against_oracle(gpu, pts, down, nths=(0, 3))


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
for nth in (0, 1, 3, 31):
    out["n%d" % nth] = cw.cwipc_hip_nn_distance(a, b, nth)
out["self1"] = cw.cwipc_hip_nn_distance(b, b, 1)
np.savez(sys.argv[3], **out)
"""


# the library's three grid flows, each forced where the size alone would not take it: small clouds, the dense layout, the sparse one
# (reference: one tile of a frame; source: the tile moved by 2 mm, every fourth point, in a shuffled order)
@pytest.mark.parametrize("npoints,env", [(72000, {}), (72000, {"CWIPC_SOR_SMALL_CELLS": "0"}), (72000, {"CWIPC_SOR_SPARSE": "1"}),
                                         (600000, {}), (600000, {"CWIPC_SOR_SPARSE": "1"}), (4000000, {})])
def test_each_grid_flow(gpu, synth, npoints, env, tmp_path):
    pts, _ = synth(npoints)
    tiles = sorted(set(np.unique(pts["tile"]).tolist()) - {0})
    b = jittered(pts[pts["tile"] == tiles[0]], 6)
    rng = np.random.default_rng(7)
    a = b[rng.permutation(len(b))[:len(b) // 4]].copy()
    a["x"] += np.float32(0.002)
    a["z"] -= np.float32(0.001)
    inp, out = str(tmp_path / "in.npz"), str(tmp_path / "d.npz")
    np.savez(inp, a=a, b=b)
    subprocess.run([sys.executable, "-c", _CHILD, ROOT, inp, out], check=True, timeout=600, env=dict(os.environ, **env))
    got = np.load(out)
    a, b = xyz_of(a), xyz_of(b)
    q = np.arange(len(a)) if len(a) <= SAMPLED else np.sort(np.random.default_rng(4).choice(len(a), SAMPLED, replace=False))
    wants = ao.nn_distance2_grid_many(a[q], b, NTHS, per_cell=48)
    for nth in NTHS:
        assert got["n%d" % nth].shape == (len(a),)
        assert np.array_equal(got["n%d" % nth][q], np.sqrt(wants[(nth, np.inf)])), (npoints, env, nth)
    qb = np.arange(len(b)) if len(b) <= SAMPLED else np.sort(np.random.default_rng(5).choice(len(b), SAMPLED, replace=False))
    assert np.array_equal(got["self1"][qb], np.sqrt(ao.nn_distance2_grid(b[qb], b, 1, per_cell=48)))


def test_small_and_degenerate_clouds(gpu):
    rng = np.random.default_rng(11)
    ref = rng.normal(0, 0.2, (5000, 3)).astype(np.float32)
    src = rng.normal(0, 0.3, (700, 3)).astype(np.float32)
    for nth in NTHS:
        one = gpu.cwipc_hip_nn_distance(make_cloud(gpu, as_points(src[:1])), make_cloud(gpu, as_points(ref)), nth)
        assert np.array_equal(one, ao.nn_distance(src[:1], ref, nth))                                   # a source of one point
        got = gpu.cwipc_hip_nn_distance(make_cloud(gpu, as_points(src)), make_cloud(gpu, as_points(ref[:1])), nth)
        assert np.array_equal(got, ao.nn_distance(src, ref[:1], nth))                                   # a reference of one point
        if nth:
            got = gpu.cwipc_hip_nn_distance(make_cloud(gpu, as_points(src)), make_cloud(gpu, as_points(ref[:nth])), nth)
            assert got.shape == (len(src),) and np.all(np.isposinf(got))                                # ... of nth points: no (nth + 1)-th
        got = gpu.cwipc_hip_nn_distance(make_cloud(gpu, as_points(src)), make_cloud(gpu, as_points(ref[:nth + 1])), nth)
        assert np.array_equal(got, ao.nn_distance(src, ref[:nth + 1], nth))
    # every query outside the reference's box, near and far, with and without a bound
    far = (src * 0.1 + np.array([3.0, -2.0, 5.0])).astype(np.float32)
    near = (np.abs(src) * 0.01 + ref.max(axis=0)).astype(np.float32)
    for q in (far, near):
        for nth in NTHS:
            for bound in (np.inf, 0.05, 7.0):
                got = gpu.cwipc_hip_nn_distance(make_cloud(gpu, as_points(q)), make_cloud(gpu, as_points(ref)), nth, bound)
                assert np.array_equal(got, ao.nn_distance(q, ref, nth, bound)), (nth, bound)
    # both clouds identical: the same object, and two clouds of the same points
    pc = make_cloud(gpu, as_points(ref))
    for nth in NTHS:
        want = ao.nn_distance(ref, ref, nth)
        assert np.array_equal(gpu.cwipc_hip_nn_distance(pc, pc, nth), want)
        assert np.array_equal(gpu.cwipc_hip_nn_distance(pc, make_cloud(gpu, as_points(ref)), nth), want)
    assert np.all(gpu.cwipc_hip_nn_distance(pc, pc, 0) == 0.0)
    # coincident reference points: ties are values
    stack = np.repeat(ref[:50], 4, axis=0)
    for nth in (0, 3, 4):
        assert np.array_equal(gpu.cwipc_hip_nn_distance(make_cloud(gpu, as_points(src)), make_cloud(gpu, as_points(stack)), nth), ao.nn_distance(src, stack, nth))
    # an empty source: nothing; an empty reference: inf everywhere
    empty = make_cloud(gpu, as_points(np.zeros((0, 3))))
    assert gpu.cwipc_hip_nn_distance(empty, pc).shape == (0,)
    got = gpu.cwipc_hip_nn_distance(pc, empty, 0)
    assert got.shape == (len(ref),) and np.all(np.isposinf(got))


def test_two_calls_and_four_threads_give_the_same_bytes(gpu, synth):
    pts, _ = synth(72000)
    pts = jittered(pts, 9)
    tiles = sorted(set(np.unique(pts["tile"]).tolist()) - {0})
    a, b = make_cloud(gpu, pts[pts["tile"] == tiles[0]]), make_cloud(gpu, pts[pts["tile"] == tiles[1]])
    jobs = [(a, b, 0, np.inf), (b, a, 1, np.inf), (a, b, 3, 0.01), (a, a, 1, np.inf)]
    alone = [gpu.cwipc_hip_nn_distance(*j).tobytes() for j in jobs]
    assert alone == [gpu.cwipc_hip_nn_distance(*j).tobytes() for j in jobs]
    d = gpu.cwipc_hip_nn_distance(a, b)
    at = np.linspace(0, d.max(), 401)[1:]
    kde_alone = gpu.cwipc_hip_gaussian_kde(d, at).tobytes()
    assert kde_alone == gpu.cwipc_hip_gaussian_kde(d, at).tobytes()
    got, got_kde, errors = [None] * 4, [None] * 4, []

    def work(i):
        try:
            gpu.cwipc_hip_set_device(0)
            for _ in range(3):
                got[i] = gpu.cwipc_hip_nn_distance(*jobs[i]).tobytes()
                got_kde[i] = gpu.cwipc_hip_gaussian_kde(d, at).tobytes()
        except Exception as e:   # pragma: no cover - reported below
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors
    assert got == alone and got_kde == [kde_alone] * 4


# ---------------------------------------------------------------------------
# the density estimate
# ---------------------------------------------------------------------------
def kde_bound(meta):
    return 100 * meta["kde_cpu_spread"]


@pytest.mark.parametrize("m", [1, 7, 400, 5000])
def test_kde_on_the_golden_distances(gpu, vectors, m):
    v, meta = vectors
    worst = 0.0
    for pair in meta["pairs"]:
        for ignore in (0, 1):
            d = load_distances(v, pair, "fwd", ignore, "cut")
            d = d[np.isfinite(d)]
            if d.min() == d.max():
                continue
            at = np.linspace(0, d.max(), m + 1)[1:]
            for bw in (None, "silverman", 0.25):
                got, want = gpu.cwipc_hip_gaussian_kde(d, at, bw), ao.gaussian_kde(d, at, bw)
                assert got.shape == (m,)
                worst = max(worst, float(np.max(np.abs(got - want)) / np.max(want)))
    print("kde, golden distances, m=%d: largest difference relative to the curve's maximum %.3g (bound %.3g)" % (m, worst, kde_bound(meta)))
    assert worst <= kde_bound(meta)


@pytest.mark.parametrize("m", [1, 7, 400, 5000])
def test_kde_on_two_million_samples(gpu, vectors, m):
    _, meta = vectors
    rng = np.random.default_rng(2)
    # the shape the analyzer sees: a narrow peak of matched points and a long tail
    d = np.abs(np.concatenate([rng.normal(0.004, 0.0015, 1500000), rng.gamma(2.0, 0.01, 500000)]))
    at = np.linspace(0, d.max(), m + 1)[1:]
    got, want = gpu.cwipc_hip_gaussian_kde(d, at), ao.gaussian_kde(d, at)
    diff = float(np.max(np.abs(got - want)) / np.max(want))
    print("kde, 2e6 samples, m=%d: largest difference relative to the curve's maximum %.3g (bound %.3g)" % (m, diff, kde_bound(meta)))
    assert diff <= kde_bound(meta)


def test_kde_sizes_around_the_chunking(gpu, vectors):
    _, meta = vectors
    rng = np.random.default_rng(8)
    for n in (2, 3, 1023, 1024, 1025, 4099, (1 << 20) + 5):
        d = rng.gamma(2.0, 0.01, n)
        at = np.linspace(0, d.max(), 66)[1:]
        got, want = gpu.cwipc_hip_gaussian_kde(d, at), ao.gaussian_kde(d, at)
        assert np.max(np.abs(got - want)) <= kde_bound(meta) * np.max(want), n


# ---------------------------------------------------------------------------
# the analyzers
# ---------------------------------------------------------------------------
def run_analyzer(gpu, v, meta, run):
    from cwipc_util_amd.registration import analyze
    sp, rp = clouds_of(v, meta, run["pair"])
    s = run["settings"]
    a = getattr(analyze, run["analyzer"])()
    a.use_kde = run["use_kde"]
    src, ref = make_cloud(gpu, sp, timestamp=1), make_cloud(gpu, rp, timestamp=2)
    a.set_source_pointcloud(src, s.get("source_tilemask"))
    a.set_reference_pointcloud(ref, s.get("reference_tilemask"))
    a.set_correspondence_measure(run["measure"], *[m for m in ("mean", "tmean", "median", "mode") if m != run["measure"]])
    if "min_correspondence_distance" in s:
        a.set_min_correspondence_distance(s["min_correspondence_distance"])
    if "max_correspondence_distance" in s:
        a.set_max_correspondence_distance(meta["pairs"][run["pair"]]["cut"])
    if "ignore_nearest" in s:
        a.set_ignore_nearest(s["ignore_nearest"])
    if s.get("ignore_floor"):
        a.set_ignore_floor(True)
    return a, a.run(), a.get_results()


def test_analyzers_against_every_golden_result(gpu, vectors):
    v, meta = vectors
    bound, worst = kde_bound(meta), 0.0
    for run in meta["runs"]:
        a, ok, r = run_analyzer(gpu, v, meta, run)
        where = (run["config"], run["analyzer"], run["use_kde"], run["measure"])
        hist, edges = v[run["histogram"] + "_histogram"], v[run["histogram"] + "_edges"]
        assert ok == run["ok"]
        assert (r.sourcePointCount, r.referencePointCount) == (run["sourcePointCount"], run["referencePointCount"]), where
        assert (r.tilemask, r.referenceTilemask, r.algorithm, r.variant) == (run["tilemask"], run["referenceTilemask"], run["algorithm"], run["variant"]), where
        assert (a.histogram_bincount, a.histogram_binsize) == (run["bincount"], run["binsize"]), where
        for f in ("mean", "stddev", "median", "tmean"):
            assert getattr(r, f) == run[f], where + (f,)
        assert np.array_equal(r.histogramEdges, edges), where
        if run["use_kde"]:
            diff = float(np.max(np.abs(r.histogram - hist)) / np.max(hist))
            worst = max(worst, diff)
            assert diff <= bound, where + (diff,)
            top = np.sort(hist)[-2:]
            assert (top[1] - top[0]) > bound * top[1]          # (the generator's check: the mode's bin does not hang on rounding)
            assert np.argmax(r.histogram) == np.argmax(hist), where
        else:
            assert np.array_equal(r.histogram, hist), where
        assert r.mode == run["mode"], where
        assert r.minCorrespondence == run["minCorrespondence"] and r.minCorrespondenceCount == run["minCorrespondenceCount"], where
        assert r.tostr() == run["tostr"], where
    print("analyzer curves: largest difference from the golden ones, relative to the curve's maximum %.3g (bound %.3g)" % (worst, bound))


def test_floor_filter_is_the_reference_predicate(gpu, vectors):
    from cwipc_util_amd.registration.analyze import _floor_filter
    v, meta = vectors
    for pts in clouds_of(v, meta, "floor"):
        pts = pts.copy()
        pts["y"][5:9] = np.nextafter(np.float32(0.1), np.float32(-1))
        kept = _floor_filter(make_cloud(gpu, pts)).get_numpy_array()
        want = pts[pts["y"] > 0.1]           # (a float32 column against 0.1: numpy compares in float32, as the reference's line does)
        assert len(want) < len(pts) and kept.tobytes() == want.tobytes()
        assert np.array_equal(pts["y"] > 0.1, pts["y"] > np.float32(0.1))


def test_all_distances_the_same(gpu, capsys):
    from cwipc_util_amd.registration.analyze import RegistrationAnalyzer, RegistrationAnalyzerSymmetric
    g = np.stack(np.meshgrid(np.arange(4.0), np.arange(4.0), [0.0]), -1).reshape(-1, 3).astype(np.float32)
    for cls in (RegistrationAnalyzer, RegistrationAnalyzerSymmetric):
        a = cls()
        a.set_source_pointcloud(make_cloud(gpu, as_points(g + np.float32([0, 0, 0.25]))))
        a.set_reference_pointcloud(make_cloud(gpu, as_points(g)))
        assert a.run() is False
        r = a.get_results()
        n = len(g) * (2 if cls is RegistrationAnalyzerSymmetric else 1)
        assert r.minCorrespondence == 0.25 and r.minCorrespondenceCount == n
        assert np.array_equal(r.histogram, [0.25]) and np.array_equal(r.histogramEdges, [0.25, 0.25])
        assert (r.sourcePointCount, r.referencePointCount) == (len(g), len(g))     # (not adjusted: the run stopped before)
    assert "all distances are the same" in capsys.readouterr().out


def test_analyzer_leaves_its_clouds_on_the_device_and_unchanged(gpu, vectors):
    from cwipc_util_amd.registration.analyze import RegistrationAnalyzerSymmetric
    v, meta = vectors
    dll = gpu.util.cwipc_util_dll_load()
    sp, rp = clouds_of(v, meta, "floor")
    src, ref = make_cloud(gpu, sp), make_cloud(gpu, rp)
    for pc in (src, ref):
        gpu.cwipc_hip_upload(pc, drop_host_copy=True)
        assert dll.cwipc_hip_is_device_resident(pc.as_cwipc_p()) == 1
    before = gpu.cwipc_dangling_allocations(False)
    for settings in ({}, {"floor": True}, {"mask": 1}):
        a = RegistrationAnalyzerSymmetric()
        a.set_source_pointcloud(src, settings.get("mask"))
        a.set_reference_pointcloud(ref, settings.get("mask"))
        if settings.get("floor"):
            a.set_ignore_floor(True)
        assert a.run()
        masked = [pc for pc in (a.get_source_pointcloud(), a.get_reference_pointcloud()) if pc is not src and pc is not ref]
        for pc in masked:
            assert dll.cwipc_hip_is_device_resident(pc.as_cwipc_p()) == 1
            pc.free()
        for pc in (src, ref):
            assert dll.cwipc_hip_is_device_resident(pc.as_cwipc_p()) == 1
    assert gpu.cwipc_dangling_allocations(False) == before
    assert src.get_numpy_array().tobytes() == sp.tobytes() and ref.get_numpy_array().tobytes() == rp.tobytes()


# ---------------------------------------------------------------------------
# errors
# ---------------------------------------------------------------------------
def test_error_paths(gpu):
    import ctypes
    dll = gpu.util.cwipc_util_dll_load()
    logged = []
    gpu.cwipc_log_configure(gpu.CWIPC_LOG_LEVEL_WARNING, lambda level, msg: logged.append((level, msg)))
    try:
        rng = np.random.default_rng(1)
        pc = make_cloud(gpu, as_points(rng.normal(0, 0.1, (300, 3))))
        before = gpu.cwipc_dangling_allocations(False)
        buf = np.full(300, -1.0)
        inf = float("inf")

        def nn(src, ref, nth, maxd, cap=300):
            n = len(logged)
            rc = dll.cwipc_hip_nn_distance2(src, ref, nth, maxd, buf.ctypes.data, cap)
            return rc, len(logged) - n

        p = pc.as_cwipc_p()
        for args in ((None, p, 0, inf), (p, None, 0, inf), (p, p, -1, inf), (p, p, 32, inf), (p, p, 0, float("nan")), (p, p, 0, 0.0),
                     (p, p, 0, -1.0), (p, p, 0, inf, 299)):
            rc, n = nn(*args)
            assert rc == -1 and n >= 1, args
        assert np.all(buf == -1.0)                                  # nothing was written
        assert nn(p, p, 31, inf) == (0, 0) and nn(p, p, 0, 1e-30) == (0, 0)
        for bad in ((-1, inf), (32, inf), (0, float("nan")), (0, 0.0)):
            with pytest.raises(gpu.CwipcError):
                gpu.cwipc_hip_nn_distance(pc, pc, *bad)

        s, at, dens = rng.gamma(2.0, 0.01, 100), np.linspace(0, 0.1, 10), np.full(10, -1.0)

        def kde(n, h, samples=s):
            k = len(logged)
            rc = dll.cwipc_hip_gaussian_kde(samples.ctypes.data if samples is not None else None, n, h, at.ctypes.data, 10, dens.ctypes.data)
            return rc, len(logged) - k

        for args in ((0, 0.01), (100, 0.0), (100, -0.01), (100, inf), (100, float("nan")), (100, 0.01, None)):
            rc, n = kde(*args)
            assert rc == -1 and n >= 1, args
        assert np.all(dens == -1.0)
        assert kde(100, 0.01) == (0, 0)
        with pytest.raises(gpu.CwipcError):
            gpu.cwipc_hip_gaussian_kde(np.array([1.0]), at)         # one sample has no standard deviation
        with pytest.raises(gpu.CwipcError):
            gpu.cwipc_hip_gaussian_kde(np.array([1.0, 1.0, 1.0]), at)   # ... and equal samples a zero bandwidth
        with pytest.raises(ValueError):
            gpu.cwipc_hip_gaussian_kde(s, at, "nonsense")
        assert all(level == gpu.CWIPC_LOG_LEVEL_ERROR for level, _ in logged)
        assert gpu.cwipc_dangling_allocations(False) == before
    finally:
        gpu.cwipc_log_configure(gpu.CWIPC_LOG_LEVEL_WARNING, None)
