"""The numpy oracle of the registration analyzer (tests/analyze_oracle.py) against what the reference's own analyzer recorded in
tests/golden/analyze_vectors.npz (made by tests/golden/make_analyze_vectors.py), and against live scipy where it can be imported.
CPU only: numpy and the fixture, no GPU, no library symbol.

Bars: distances bit for bit (inf positions included); density curves within kde_cpu_spread of the curve's maximum -- the fixture's
own record of how far two f64 summation orders of that sum lie apart (scipy's and the oracle's, 5.5e-15 measured when the fixture
was made, 6e-15 recorded); the reductions exactly, since they are the same numpy calls on the same array.
"""
import json
import os
import sys

import numpy as np
import pytest

import analyze_oracle as ao

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)


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
    return np.column_stack([p["x"], p["y"], p["z"]])


def prepared(v, meta, run):
    """The two coordinate arrays a recorded run took its distances between (tile mask, floor filter), and its settings."""
    src, ref = clouds_of(v, meta, run["pair"])
    s = run["settings"]
    if s.get("source_tilemask"):
        src = src[(src["tile"] & s["source_tilemask"]) != 0]
    if s.get("reference_tilemask"):
        ref = ref[(ref["tile"] & s["reference_tilemask"]) != 0]
    if s.get("ignore_floor"):
        src, ref = src[src["y"] > np.float32(0.1)], ref[ref["y"] > np.float32(0.1)]
    bound = meta["pairs"][run["pair"]]["cut"] if "max_correspondence_distance" in s else np.inf
    return xyz_of(src), xyz_of(ref), s.get("ignore_nearest", 0), bound, s.get("min_correspondence_distance", 0.0)


def run_distances(v, meta, run):
    sx, rx, ignore, bound, binsize = prepared(v, meta, run)
    d = ao.nn_distance(sx, rx, ignore, bound)
    if run["analyzer"].endswith("Symmetric"):
        d = np.concatenate([d, ao.nn_distance(rx, sx, ignore, bound)])
    return d, len(sx), len(rx), binsize


def test_fixture_is_what_the_issue_asks_for(vectors):
    v, meta = vectors
    assert set(meta["pairs"]) == {"patches", "outside", "floor", "self"}
    assert meta["scipy"] and meta["numpy"] and 0 < meta["kde_cpu_spread"] < 1e-12
    for pair, rec in meta["pairs"].items():
        assert 0.25 < rec["cut_fraction"] < 0.42
    src, ref = clouds_of(v, meta, "outside")
    outside = np.zeros(len(src), dtype=bool)
    for a in "xyz":
        outside |= (src[a] < ref[a].min()) | (src[a] > ref[a].max())
    assert np.mean(outside) > 0.25                               # part of the source lies outside the reference's box
    src, ref = clouds_of(v, meta, "floor")
    assert np.mean(src["y"] <= np.float32(0.1)) > 0.1 and np.any(src["y"] == np.float32(0.1))
    assert len(meta["runs"]) == 5 * 2 * 2 * 6


def test_distances_bit_for_bit(vectors):
    v, meta = vectors
    for pair, rec in meta["pairs"].items():
        src, ref = clouds_of(v, meta, pair)
        for ignore in (0, 1, 3):
            for bound_name in ("inf", "cut"):
                bound = np.inf if bound_name == "inf" else rec["cut"]
                assert np.array_equal(ao.nn_distance(xyz_of(src), xyz_of(ref), ignore, bound), load_distances(v, pair, "fwd", ignore, bound_name)), (pair, ignore, bound_name)
                assert np.array_equal(ao.nn_distance(xyz_of(ref), xyz_of(src), ignore, bound), load_distances(v, pair, "back", ignore, bound_name)), (pair, ignore, bound_name)
                if bound_name == "cut":
                    # the strict `<` is not decided by rounding anywhere in the fixture
                    full = load_distances(v, pair, "fwd", ignore, "inf")
                    assert not np.any(np.abs(full - bound) <= 1e-9 * bound)


def test_self_pair_nearest_is_the_point_itself(vectors):
    v, meta = vectors
    assert np.all(load_distances(v, "self", "fwd", 0, "inf") == 0.0)
    assert np.all(load_distances(v, "self", "fwd", 1, "inf") > 0.0)


def test_analyzer_results(vectors):
    v, meta = vectors
    worst = 0.0
    for run in meta["runs"]:
        d, ns, nr, binsize = run_distances(v, meta, run)
        others = [m for m in ("mean", "tmean", "median", "mode") if m != run["measure"]]
        r = ao.analyze(d, ns, nr, run["measure"], others, run["use_kde"], binsize=binsize, symmetric=run["analyzer"].endswith("Symmetric"))
        hist, edges = v[run["histogram"] + "_histogram"], v[run["histogram"] + "_edges"]
        assert r["ok"] == run["ok"] is True
        assert (r["sourcePointCount"], r["referencePointCount"]) == (run["sourcePointCount"], run["referencePointCount"])
        assert np.array_equal(r["histogramEdges"], edges) and len(hist) == run["bincount"]
        for f in ("mean", "stddev", "median", "tmean"):
            assert r[f] == run[f], (run["config"], run["analyzer"], f)
        if run["use_kde"]:
            spread = np.max(np.abs(r["histogram"] - hist)) / np.max(hist)
            worst = max(worst, spread)
            assert spread <= meta["kde_cpu_spread"], (run["config"], spread)
            assert np.argmax(r["histogram"]) == np.argmax(hist)
        else:
            assert np.array_equal(r["histogram"], hist)
        assert r["mode"] == run["mode"]
        if run["use_kde"] and run["measure"] in ("mode", "2mode") or not run["measure"].startswith(("mode", "2mode")):
            assert r["minCorrespondence"] == run["minCorrespondence"]
            assert r["minCorrespondenceCount"] == run["minCorrespondenceCount"]
    print("largest oracle-to-scipy curve difference, relative to the curve's maximum: %.3g" % worst)


def test_known_answers():
    # two points against three: by hand
    src = np.array([[0, 0, 0], [1, 0, 0]], dtype=np.float32)
    ref = np.array([[0, 0, 1], [0, 3, 0], [1, 0, 0.5]], dtype=np.float32)
    assert np.array_equal(ao.nn_distance(src, ref, 0), [1.0, 0.5])
    assert np.array_equal(ao.nn_distance(src, ref, 1), [np.sqrt(1.25), np.sqrt(2.0)])
    assert np.array_equal(ao.nn_distance(src, ref, 2), [3.0, np.sqrt(10.0)])
    assert np.all(np.isinf(ao.nn_distance(src, ref, 3)))
    assert np.array_equal(ao.nn_distance(src, ref, 0, 1.0), [np.inf, 0.5])          # a point AT the bound is not under it
    assert np.array_equal(ao.nn_distance(src, ref[:0], 0), [np.inf, np.inf])
    # one sample: the Gaussian itself
    got = ao.gaussian_kde_h([0.5], 0.25, [0.5, 0.75])
    want = np.exp([-0.0, -0.5]) / (0.25 * np.sqrt(2 * np.pi))
    assert np.allclose(got, want, rtol=1e-15)
    x = np.linspace(-6, 8, 4001)
    dens = ao.gaussian_kde(np.random.default_rng(0).normal(1.0, 1.0, 5000), x)
    assert abs(np.sum(dens) * (x[1] - x[0]) - 1.0) < 1e-6                            # a density: integrates to 1
    assert ao.trim_mean(np.arange(10.0), 0.1) == 4.5


def test_grid_search_gives_the_brute_force_bits(vectors):
    v, meta = vectors
    for pair in meta["pairs"]:
        src, ref = clouds_of(v, meta, pair)
        for nth, bound in ((0, np.inf), (3, meta["pairs"][pair]["cut"]), (31, np.inf)):
            want = ao.nn_distance2(xyz_of(src), xyz_of(ref), nth, bound)
            assert np.array_equal(ao.nn_distance2_grid(xyz_of(src), xyz_of(ref), nth, bound, per_cell=24), want), (pair, nth)
            assert np.array_equal(ao.nn_distance2_grid(xyz_of(src), xyz_of(ref), nth, bound), want), (pair, nth)


def test_against_live_scipy():
    spatial = pytest.importorskip("scipy.spatial")
    stats = pytest.importorskip("scipy.stats")
    rng = np.random.default_rng(5)
    ref = rng.normal(0, 0.3, (5000, 3)).astype(np.float32)
    src = (rng.normal(0, 0.4, (3000, 3)) + 0.1).astype(np.float32)
    tree = spatial.KDTree(ref)
    for nth in (0, 1, 3, 31):
        for bound in (np.inf, 0.05):
            want, _ = tree.query(src, k=[nth + 1], distance_upper_bound=bound)
            assert np.array_equal(ao.nn_distance(src, ref, nth, bound), want.reshape(-1)), (nth, bound)
    d = ao.nn_distance(src, ref)
    at = np.linspace(0, d.max(), 401)[1:]
    for bw in (None, "silverman", 0.3):
        want = stats.gaussian_kde(d, bw_method=bw).evaluate(at)
        assert np.max(np.abs(ao.gaussian_kde(d, at, bw) - want)) <= 1e-13 * want.max()
    assert ao.trim_mean(d, 0.1) == stats.trim_mean(d, 0.1)
