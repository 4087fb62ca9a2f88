"""Per-call time of Euclidean clustering (cwipc_cluster_filter, cwipc_cluster_labels; RULE K) against the filter it stands beside in a
chain, remove_outliers(16, 1.0), on the same cloud in the same run, and against the numpy and scipy model on the CPU.

    python scratch/cluster_timing.py [out.json] [--no-model]

Clouds: the synthetic source at 299 k and 2.0 M points with radius at 3 x and 8 x its cellsize; a 300 k-point sphere with 200 clumps of
20 to 500 points around it (what the filter is for: keep the sphere, min_points = 1000).  Per call: the median wall time of 10 calls
that are waited for (settled) after 3 warm-up calls; the kernels' split from hipEvents (cwipc_hip_profile), the link kernel's share
of it; what the link kernel did (cwipc_hip_cluster_link_stats: links, unions, parent words loaded) per point."""
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


def timed(fn, reps=10):
    for _ in range(3):
        fn()
    sync()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); sync(); t.append(time.perf_counter() - t0)
    with cw.cwipc_hip_profile() as prof:
        fn()
    kernels = {k: round(v[0], 4) for k, v in prof.kernels.items()}
    return {"settled_ms": round(float(np.median(t)) * 1e3, 4), "min_ms": round(float(np.min(t)) * 1e3, 4), "kernels_ms": kernels}


def sphere_with_clumps(seed=300):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(300000, 3))
    parts = [v / np.linalg.norm(v, axis=1, keepdims=True)]
    for _ in range(200):
        c = rng.normal(size=3)
        c *= rng.uniform(1.15, 1.6) / np.linalg.norm(c)
        parts.append(c + rng.normal(scale=0.004, size=(int(rng.integers(20, 501)), 3)))
    xyz = np.concatenate(parts).astype(np.float32)
    xyz = xyz[rng.permutation(len(xyz))]
    pts = np.zeros(len(xyz), dtype=cw.cwipc_point_numpy_dtype)
    pts["x"], pts["y"], pts["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    pts["tile"] = 1
    return cw.cwipc_from_numpy_array(pts, 0)


def measure(pc, radius, min_points, with_model):
    n = pc.count()
    r = {"points": n, "radius": radius, "min_points": min_points}
    labels, sizes = cw.cwipc_cluster_labels(pc, radius)
    kept = cw.cwipc_cluster_filter(pc, radius, min_points)
    r["clusters"], r["largest"], r["kept_points"] = int(len(sizes)), int(sizes.max()) if len(sizes) else 0, kept.count()
    kept.free()
    r["cluster_filter"] = timed(lambda: cw.cwipc_cluster_filter(pc, radius, min_points).free())
    r["cluster_filter_ranked"] = timed(lambda: cw.cwipc_cluster_filter(pc, radius, 1, 3).free())
    r["cluster_labels_to_host"] = timed(lambda: cw.cwipc_cluster_labels(pc, radius))
    r["remove_outliers_16"] = timed(lambda: cw.cwipc_remove_outliers(pc, 16, 1.0, False).free())
    k = r["cluster_filter"]["kernels_ms"]
    r["link_kernel_share"] = round(k.get("cluster_link", 0.0) / max(sum(k.values()), 1e-9), 3)
    r["ratio_to_remove_outliers"] = round(r["cluster_filter"]["settled_ms"] / r["remove_outliers_16"]["settled_ms"], 2)
    stats = cw.cwipc_hip_cluster_link_stats(pc, radius)
    r["link_stats"] = stats
    r["links_per_point"] = round(stats["links"] / n, 2)
    r["unions_per_point"] = round(stats["unions"] / n, 3)
    r["find_loads_per_union"] = round(stats["find_loads"] / max(stats["unions"], 1), 2)
    if with_model:
        import cluster_model as cm
        arr = pc.get_numpy_array()
        xyz = np.column_stack([arr["x"], arr["y"], arr["z"]])
        t0 = time.perf_counter()
        ml, ms = cm.cluster_labels(xyz, radius)
        r["model_cpu_s"] = round(time.perf_counter() - t0, 2)
        r["model_agrees"] = bool(np.array_equal(ml, labels) and np.array_equal(ms, sizes))
    return r


def main():
    with_model = "--no-model" not in sys.argv
    res = {}
    for label, npts in (("synthetic_299k", 299000), ("synthetic_2m", 2000000)):
        pc = make_input(cw, npts, 0.0)
        cw.cwipc_hip_upload(pc, drop_host_copy=False)
        for mult in (3, 8):
            name = "%s_r%dx" % (label, mult)
            res[name] = measure(pc, mult * float(pc.cellsize()), 100, with_model and not (npts > 1000000 and mult == 8))
            res[name]["cellsize"] = float(pc.cellsize())
            print(name, json.dumps(res[name]), flush=True)
        pc.free()
    pc = sphere_with_clumps()
    cw.cwipc_hip_upload(pc, drop_host_copy=False)
    res["sphere_300k_200_clumps"] = measure(pc, 0.02, 1000, with_model)
    print("sphere_300k_200_clumps", json.dumps(res["sphere_300k_200_clumps"]), flush=True)
    if len(sys.argv) > 1 and not sys.argv[1].startswith("--"):
        os.makedirs(os.path.dirname(sys.argv[1]) or ".", exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
