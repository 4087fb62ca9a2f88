"""Per-call time of the registration analyzer's GPU steps, against the outlier filter's self-search on the same reference cloud.

    python scratch/analyze_timing.py [out.json]

  * cwipc_hip_nn_distance(source, reference, nth) for 36 k / 300 k / 2 M points a side, nth in {0, 1}: source = the reference moved
    by 3 mm and 0.5 degrees (cwipc_transform), its points in the reference's order; next to it cwipc_hip_knn_mean_dist(reference,
    nth + 1) -- the self-search, the yardstick -- from the same run; the search kernels alone from hipEvents (cwipc_hip_profile);
  * cwipc_hip_gaussian_kde for n in {36 k, 600 k, 4 M} x m = 400, with the f64 exp rate it amounts to;
  * one RegistrationAnalyzerSymmetric.run() for 300 k against 300 k, split into search, KDE and the host's numpy;
  * the CPU side (scipy's KDTree with 16 workers, gaussian_kde) where scipy can be imported.
Per call: the median wall time of a call that is waited for (settled) and the mean of 20 calls back to back (in a stream; both
entry points wait for their result, so the two differ by little)."""
import json
import os
import sys
import time

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import numpy as np
import torch  # noqa: F401
import cwipc_util_amd as cw
from bench import make_input

sync = cw.util.cwipc_util_dll_load().cwipc_hip_synchronize


def timed(fn, reps=10, profile=True):
    for _ in range(3):
        fn()
    sync()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); sync(); t.append(time.perf_counter() - t0)
    out = {"settled_ms": round(float(np.median(t)) * 1e3, 4)}
    t0 = time.perf_counter()
    for _ in range(20):
        fn()
    sync()
    out["in_stream_ms"] = round((time.perf_counter() - t0) / 20 * 1e3, 4)
    if profile:
        with cw.cwipc_hip_profile() as prof:
            fn()
        out["kernels_ms"] = {k: round(v[0], 4) for k, v in prof.kernels.items()}
    return out


def main():
    res = {"nn_distance": {}, "kde": {}}
    a = np.radians(0.5)
    m = np.array([[np.cos(a), 0, np.sin(a), 0.003], [0, 1, 0, 0.0], [-np.sin(a), 0, np.cos(a), 0.0], [0, 0, 0, 1.0]])
    try:
        import scipy.spatial
        import scipy.stats
    except ImportError:
        scipy = None
    for label, npts, down in (("36k", 300000, 0.01), ("300k", 300000, None), ("2m", 2000000, None)):
        ref = make_input(cw, npts, 0.0)
        cw.cwipc_hip_upload(ref, drop_host_copy=True)
        if down:
            ref = cw.cwipc_downsample(ref, down)
        src = cw.cwipc_transform(ref, m)
        r = {"points": ref.count()}
        for nth in (0, 1):
            r["nn_distance_nth%d" % nth] = timed(lambda: cw.cwipc_hip_nn_distance(src, ref, nth))
            r["knn_mean_dist_k%d" % (nth + 1)] = timed(lambda: cw.cwipc_hip_knn_mean_dist(ref, nth + 1))
            kn, ks = r["nn_distance_nth%d" % nth]["kernels_ms"], r["knn_mean_dist_k%d" % (nth + 1)]["kernels_ms"]
            r["search_kernel_ratio_nth%d" % nth] = round(kn.get("nn_distance2", 0.0) / max(ks.get("sor_knn_mean_dist", 0.0), 1e-9), 3)
            r["call_ratio_nth%d" % nth] = round(r["nn_distance_nth%d" % nth]["settled_ms"] / r["knn_mean_dist_k%d" % (nth + 1)]["settled_ms"], 3)
        if scipy is not None:
            rx, sx = ref.get_numpy_matrix(onlyGeometry=True), src.get_numpy_matrix(onlyGeometry=True)
            t0 = time.perf_counter(); tree = scipy.spatial.KDTree(rx); t1 = time.perf_counter()
            tree.query(sx, k=[1], workers=16); t2 = time.perf_counter()
            r["scipy_cpu_ms"] = {"tree": round((t1 - t0) * 1e3, 2), "query_16_workers": round((t2 - t1) * 1e3, 2)}
        res["nn_distance"][label] = r
        print(label, json.dumps(r), flush=True)
        if label == "300k":
            from cwipc_util_amd.registration.analyze import RegistrationAnalyzerSymmetric
            an = RegistrationAnalyzerSymmetric()
            an.set_source_pointcloud(src)
            an.set_reference_pointcloud(ref)
            an.set_correspondence_measure("mode", "mean", "median", "tmean")
            an.run()
            t0 = time.perf_counter(); an.run(); whole = time.perf_counter() - t0
            t0 = time.perf_counter()
            d = np.concatenate((cw.cwipc_hip_nn_distance(src, ref), cw.cwipc_hip_nn_distance(ref, src)))
            t1 = time.perf_counter()
            edges = np.linspace(0, d.max(), 401)
            cw.cwipc_hip_gaussian_kde(d, edges[1:])
            t2 = time.perf_counter()
            res["analyzer_symmetric_300k"] = {"run_ms": round(whole * 1e3, 3), "search_and_transfer_ms": round((t1 - t0) * 1e3, 3), "kde_ms": round((t2 - t1) * 1e3, 3),
                                              "numpy_ms": round((whole - (t2 - t0)) * 1e3, 3), "distances": int(len(d))}
            print("analyzer", json.dumps(res["analyzer_symmetric_300k"]), flush=True)
    rng = np.random.default_rng(0)
    for label, n in (("36k", 36000), ("600k", 600000), ("4m", 4000000)):
        d = np.abs(np.concatenate([rng.normal(0.004, 0.0015, n - n // 4), rng.gamma(2.0, 0.01, n // 4)]))
        at = np.linspace(0, d.max(), 401)[1:]
        r = timed(lambda: cw.cwipc_hip_gaussian_kde(d, at))
        k = r["kernels_ms"].get("kde_partial", 0.0)
        r["exp_per_s_kernel"] = round(n * 400 / max(k, 1e-9) * 1e3, -6)
        if scipy is not None and n <= 600000:
            t0 = time.perf_counter(); scipy.stats.gaussian_kde(d).evaluate(at); r["scipy_cpu_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        res["kde"][label] = r
        print("kde", label, json.dumps(r), flush=True)
    if len(sys.argv) > 1 and not sys.argv[1].startswith("--"):
        os.makedirs(os.path.dirname(sys.argv[1]) or ".", exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
