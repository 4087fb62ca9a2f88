"""Generate tests/golden/analyze_vectors.npz from the REFERENCE's own registration analyzer.

Runs only where the reference tree and scipy are (the build container); the test suite uses the committed .npz.  What runs
UNMODIFIED, loaded by path from where it lies:

  * `RegistrationAnalyzer`, `RegistrationAnalyzerSymmetric`     /root/reference/python/cwipc/registration/analyze.py
  * `AnalysisResults`                                            /root/reference/python/cwipc/registration/abstract.py
  * `BaseAlgorithm`, `cwipc_tilefilter_masked`                   /root/reference/python/cwipc/registration/util.py

with the stand-ins of make_helper_vectors.py (which this script imports): `open3d` as an in-memory placeholder, and this
repository's libcwipc_util.so behind the reference's `cwipc.util` wrapper for the container calls only (cwipc_from_numpy_array,
get_numpy_matrix, count: byte copies on the host).  The KD-tree and the density estimate are scipy's.

Recorded, per pair of clouds: the inputs; the raw `_kdtree_get_distances_for_points` array, both ways round, for ignore_nearest
in {0, 1, 3} and max_correspondence_distance in {inf, a value that cuts off about a third of the source points} (the bounded
arrays as the unbounded ones plus one bit per point, see load_distances; a cloud paired with itself is stored once); every field of
`AnalysisResults` for both analyzers, use_kde on and off, each measure as the primary one (the others named as additional
measures, so that every field is filled in).  The histogram of a run does not depend on the measure: it is stored once per
(configuration, analyzer, use_kde), and the script checks that.

Refuses to write the file when
  * a recorded distance lies within 1e-9 (relative) of a bound used (the strict `<` must stay away from a coincidence), or
  * the two highest values of a recorded density curve are closer than 100 x kde_cpu_spread of the curve's maximum (the mode's bin
    must not hang on rounding).
kde_cpu_spread (in the meta record) is the largest difference, relative to a curve's maximum, between scipy's curves and the numpy
oracle's (tests/analyze_oracle.py) over everything recorded here -- two f64 summation orders of one sum -- rounded up to one digit.

Usage: python tests/golden/make_analyze_vectors.py
"""
import json
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_helper_vectors as mhv   # noqa: E402
import analyze_oracle as ao         # noqa: E402

OUT = os.path.join(HERE, "analyze_vectors.npz")
MEASURES = ["mean", "tmean", "median", "mode", "2mode", "q=75"]
FIELDS = ["mean", "stddev", "tmean", "mode", "median"]


def surface(rng, n, x_range=(0.0, 1.0), y_range=(0.0, 1.0), jitter=5e-4):
    """Points on a quarter cylinder (radius 1 about the y axis), jittered."""
    u = rng.uniform(*x_range, n)
    y = rng.uniform(*y_range, n)
    ang = u * (math.pi / 2)
    xyz = np.column_stack([np.sin(ang), y, np.cos(ang)]) + rng.normal(0, jitter, (n, 3))
    return xyz


def misalign(xyz, shift=0.003, degrees=0.5):
    a = math.radians(degrees)
    rot = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1.0]])
    return xyz @ rot.T + np.array([shift, -shift / 2, shift / 3])


def as_points(rng, xyz):
    p = np.zeros(len(xyz), dtype=mhv.POINT_DTYPE)
    p['x'], p['y'], p['z'] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    p['r'], p['g'], p['b'] = rng.integers(0, 256, len(p)), rng.integers(0, 256, len(p)), rng.integers(0, 256, len(p))
    p['tile'] = rng.choice(np.array([1, 2], dtype=np.uint8), len(p))
    return p


def make_pairs(rng):
    pairs = {}
    a = surface(rng, 2000)
    pairs["patches"] = (as_points(rng, a), as_points(rng, misalign(surface(rng, 2100))))
    # a third of the source lies beyond the reference's box
    pairs["outside"] = (as_points(rng, misalign(surface(rng, 1600, x_range=(0.0, 1.5)))), as_points(rng, surface(rng, 1800)))
    # floor points: y from -0.05 up, a good part of both clouds at or under 0.1; a few exactly at float32(0.1)
    f1, f2 = surface(rng, 1900, y_range=(-0.05, 0.6)), misalign(surface(rng, 1700, y_range=(-0.05, 0.6)))
    p1, p2 = as_points(rng, f1), as_points(rng, f2)
    p1['y'][:5] = np.float32(0.1)
    p2['y'][:5] = np.nextafter(np.float32(0.1), np.float32(1))
    pairs["floor"] = (p1, p2)
    s = as_points(rng, surface(rng, 1700))
    pairs["self"] = (s, s)
    return pairs


# configuration name -> (pair, settings)
CONFIGS = {
    "patches": ("patches", {}),
    "patches_tiles_binsize": ("patches", {"source_tilemask": 1, "reference_tilemask": 2, "min_correspondence_distance": 0.0005}),
    "outside_max": ("outside", {"max_correspondence_distance": "cut"}),
    "floor": ("floor", {"ignore_floor": True}),
    "self_ignore1": ("self", {"ignore_nearest": 1}),
}


def load_distances(vectors, pair, way, ignore, bound_name):
    """The recorded `_kdtree_get_distances_for_points` array of a pair: way 'fwd' (source against the reference's tree) or 'back'."""
    full = vectors[f"{pair}_dist_{way}_n{ignore}_inf"]
    if bound_name == "inf":
        return full
    finite = np.unpackbits(vectors[f"{pair}_dist_{way}_n{ignore}_cut_finite"])[:len(full)].astype(bool)
    return np.where(finite, full, np.inf)


def main():
    import scipy
    cwipc, reg, _sync, _tf = mhv.load_reference()
    # (registration/util.py has pulled in registration/abstract.py already, through the package stand-in's path: the same module
    # serves analyze.py; registration/__init__.py is not executed)
    an = mhv.load_by_path("cwipc.registration.analyze", os.path.join(mhv.REF_ROOT, "python/cwipc/registration/analyze.py"))
    rng = np.random.default_rng(20261016)
    out = {}
    meta = {"scipy": scipy.__version__, "numpy": np.__version__, "pairs": {}, "runs": [], "notes": __doc__.split("Usage:")[0]}
    pairs = make_pairs(rng)
    bounds_ok = True
    spread = 0.0
    curves = []

    for name, (src, ref) in pairs.items():
        out[f"{name}_source"] = src
        if ref is not src:   # (a cloud against itself is stored once; the pair's record says so)
            out[f"{name}_reference"] = ref
        pcs = cwipc.cwipc_from_numpy_array(src, 1), cwipc.cwipc_from_numpy_array(ref, 2)
        mats = [pc.get_numpy_matrix(onlyGeometry=True) for pc in pcs]
        probe = an.RegistrationAnalyzer()
        trees = [an.KD_TREE_TYPE(m) for m in mats]
        d0 = probe._kdtree_get_distances_for_points(trees[1], mats[0]).reshape(-1)
        if d0.max() == 0:   # a cloud against itself: the bound comes from the distances to the nearest OTHER point
            probe.ignore_nearest = 1
            d0 = probe._kdtree_get_distances_for_points(trees[1], mats[0]).reshape(-1)
        cut = float(np.format_float_positional(np.quantile(d0, 2.0 / 3.0), precision=3, unique=False, fractional=False))
        meta["pairs"][name] = {"cut": cut, "source_count": len(src), "reference_count": len(ref), "same_cloud": ref is src}
        for ignore in (0, 1, 3):
            for bound_name, bound in (("inf", np.inf), ("cut", cut)):
                probe.ignore_nearest, probe.max_correspondence_distance = ignore, bound
                fwd = probe._kdtree_get_distances_for_points(trees[1], mats[0]).reshape(-1)
                back = probe._kdtree_get_distances_for_points(trees[0], mats[1]).reshape(-1)
                if bound_name == "inf":
                    out[f"{name}_dist_fwd_n{ignore}_inf"], out[f"{name}_dist_back_n{ignore}_inf"] = fwd, back
                else:
                    # with a bound scipy returns the unbounded run's values where they are under it and inf elsewhere (checked here):
                    # the file holds which, as packed bits, and load_distances() below puts the array together again
                    for way, d in (("fwd", fwd), ("back", back)):
                        full = out[f"{name}_dist_{way}_n{ignore}_inf"]
                        assert np.array_equal(d, np.where(np.isfinite(d), full, np.inf))
                        out[f"{name}_dist_{way}_n{ignore}_cut_finite"] = np.packbits(np.isfinite(d))
                if bound_name == "inf":
                    for d in (fwd, back):
                        near = np.abs(d[np.isfinite(d)] - cut) <= 1e-9 * cut
                        bounds_ok = bounds_ok and not near.any()
                    if ignore == (1 if src is ref else 0):
                        meta["pairs"][name]["cut_fraction"] = float(np.mean(fwd >= cut))

    for cname, (pname, settings) in CONFIGS.items():
        src, ref = pairs[pname]
        for cls in (an.RegistrationAnalyzer, an.RegistrationAnalyzerSymmetric):
            for use_kde in (True, False):
                hist_key = f"{cname}_{cls.__name__}_{'kde' if use_kde else 'hist'}"
                for measure in MEASURES:
                    a = cls()
                    a.use_kde = use_kde
                    pcs = cwipc.cwipc_from_numpy_array(src, 1), cwipc.cwipc_from_numpy_array(ref, 2)
                    a.set_source_pointcloud(pcs[0], settings.get("source_tilemask"))
                    a.set_reference_pointcloud(pcs[1], settings.get("reference_tilemask"))
                    a.set_correspondence_measure(measure, *[m for m in ("mean", "tmean", "median", "mode") if m != measure])
                    if "min_correspondence_distance" in settings:
                        a.set_min_correspondence_distance(settings["min_correspondence_distance"])
                    if "max_correspondence_distance" in settings:
                        a.set_max_correspondence_distance(meta["pairs"][pname]["cut"])
                    if "ignore_nearest" in settings:
                        a.set_ignore_nearest(settings["ignore_nearest"])
                    if settings.get("ignore_floor"):
                        a.set_ignore_floor(True)
                    ok = a.run()
                    r = a.get_results()
                    hist, edges = np.asarray(r.histogram), np.asarray(r.histogramEdges)
                    if hist_key + "_histogram" in out:
                        assert np.array_equal(out[hist_key + "_histogram"], hist) and np.array_equal(out[hist_key + "_edges"], edges)
                    else:
                        out[hist_key + "_histogram"], out[hist_key + "_edges"] = hist, edges
                        if use_kde:
                            curves.append((hist_key, a, hist, edges))
                    run = {"config": cname, "pair": pname, "settings": settings, "analyzer": cls.__name__, "use_kde": use_kde, "measure": measure,
                           "ok": bool(ok), "histogram": hist_key, "bincount": int(a.histogram_bincount), "binsize": float(a.histogram_binsize),
                           "minCorrespondence": float(r.minCorrespondence), "minCorrespondenceCount": int(r.minCorrespondenceCount),
                           "sourcePointCount": int(r.sourcePointCount), "referencePointCount": int(r.referencePointCount),
                           "tilemask": r.tilemask, "referenceTilemask": r.referenceTilemask, "algorithm": r.algorithm, "variant": r.variant,
                           "tostr": r.tostr()}
                    for f in FIELDS:
                        v = getattr(r, f)
                        run[f] = None if v is None else float(v)
                    meta["runs"].append(run)

    # the oracle against scipy's curves: the distances of each run from the oracle's own brute force (bit-equal, checked below)
    def xyz(p):
        return np.column_stack([p['x'], p['y'], p['z']])

    for hist_key, a, hist, edges in curves:
        s, r = a.source_ndarray, a.reference_ndarray
        d = ao.nn_distance(s, r, a.ignore_nearest, a.max_correspondence_distance)
        if isinstance(a, an.RegistrationAnalyzerSymmetric):
            d = np.concatenate([d, ao.nn_distance(r, s, a.ignore_nearest, a.max_correspondence_distance)])
        d = d[np.isfinite(d)]
        mine = ao.gaussian_kde(d, edges[1:])
        spread = max(spread, float(np.max(np.abs(mine - hist)) / np.max(hist)))
    digit = 10.0 ** math.floor(math.log10(spread))
    meta["kde_cpu_spread_measured"] = spread
    meta["kde_cpu_spread"] = math.ceil(spread / digit) * digit
    for hist_key, a, hist, edges in curves:
        top = np.sort(hist)[-2:]
        assert (top[1] - top[0]) > 100 * meta["kde_cpu_spread"] * top[1], ("the mode of %s hangs on rounding" % hist_key)
    assert bounds_ok, "a recorded distance lies within 1e-9 of the bound used: change the seed or the bound"
    for name, (src, ref) in pairs.items():
        for ignore in (0, 1, 3):
            for bound_name in ("inf", "cut"):
                bound = np.inf if bound_name == "inf" else meta["pairs"][name]["cut"]
                assert np.array_equal(ao.nn_distance(xyz(src), xyz(ref), ignore, bound), load_distances(out, name, "fwd", ignore, bound_name))

    out["meta_json"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", len(meta["runs"]), "analyzer runs; kde_cpu_spread", meta["kde_cpu_spread"],
          "(measured %.3g)" % spread, {k: v.get("cut_fraction") for k, v in meta["pairs"].items()})


if __name__ == "__main__":
    main()
