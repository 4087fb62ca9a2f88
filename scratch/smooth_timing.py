"""Per-call time of the fixed-radius neighbourhood entries (cwipc_radius_counts, cwipc_radius_outlier_filter, cwipc_smooth; RULE N)
against their neighbours in a chain -- remove_outliers(16, 1.0), the cluster filter and the direction filter -- on the same cloud, at
the same radius, in the same run, and against the numpy and scipy model on the CPU.

    python scratch/smooth_timing.py [out.json] [--no-model]

Clouds: a camera tile (the 300 k synthetic cloud voxelized at 0.01: about 36 k points) and the synthetic source at 300 k and 2.0 M
points, radius = 3 x the cloud's cellsize.  Per entry: the median wall time of 10 calls that are waited for (settled) after 3 warm-up
calls; the time per call of 20 calls issued back to back and waited for once (in a stream); the kernels' split from hipEvents
(cwipc_hip_profile) and the search kernel's share of it."""
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


def timed(fn, search=None, reps=10):
    for _ in range(3):
        fn()
    sync()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); sync(); t.append(time.perf_counter() - t0)
    sync()
    t0 = time.perf_counter()
    for _ in range(20):
        fn()
    sync()
    stream = (time.perf_counter() - t0) / 20
    with cw.cwipc_hip_profile() as prof:
        fn()
    kernels = {k: round(v[0], 4) for k, v in prof.kernels.items()}
    out = {"settled_ms": round(float(np.median(t)) * 1e3, 4), "min_ms": round(float(np.min(t)) * 1e3, 4), "in_stream_ms": round(stream * 1e3, 4),
           "kernels_ms": kernels}
    if search:
        out["search_kernel"] = search
        out["search_kernel_share"] = round(kernels.get(search, 0.0) / max(sum(kernels.values()), 1e-9), 3)
    return out


def measure(pc, radius, with_model):
    n = pc.count()
    r = {"points": n, "radius": radius}
    counts = cw.cwipc_radius_counts(pc, radius)
    r["mean_neighbours"] = round(float(counts.mean()), 2)
    r["max_neighbours"] = int(counts.max())
    kept = cw.cwipc_radius_outlier_filter(pc, radius, 6)
    r["kept_min6"] = kept.count()
    kept.free()
    r["radius_counts_to_host"] = timed(lambda: cw.cwipc_radius_counts(pc, radius), "neigh_count")
    r["radius_outlier_filter"] = timed(lambda: cw.cwipc_radius_outlier_filter(pc, radius, 6).free(), "neigh_count")
    r["smooth"] = timed(lambda: cw.cwipc_smooth(pc, radius).free(), "neigh_smooth")
    r["remove_outliers_16"] = timed(lambda: cw.cwipc_remove_outliers(pc, 16, 1.0, False).free(), "sor_knn_mean_dist")
    r["cluster_filter"] = timed(lambda: cw.cwipc_cluster_filter(pc, radius, 100).free(), "cluster_link")
    r["direction_filter_nn30"] = timed(lambda: cw.cwipc_direction_filter(pc, (0.0, 0.0, 1.0), 0.0, radius=radius, max_nn=30).free(), "direction_normals")
    r["count_kernel_to_link_kernel"] = round(r["radius_outlier_filter"]["kernels_ms"].get("neigh_count", 0.0) /
                                             max(r["cluster_filter"]["kernels_ms"].get("cluster_link", 0.0), 1e-9), 3)
    r["smooth_kernel_to_direction_kernel"] = round(r["smooth"]["kernels_ms"].get("neigh_smooth", 0.0) /
                                                   max(r["direction_filter_nn30"]["kernels_ms"].get("direction_normals", 0.0), 1e-9), 3)
    if with_model:
        import neigh_model as nm
        arr = pc.get_numpy_array()
        xyz = nm.xyz_of(arr)
        t0 = time.perf_counter()
        mc = nm.counts(xyz, radius)
        t1 = time.perf_counter()
        out, moved, gap, _ = nm.smooth_xyz(xyz, radius)
        t2 = time.perf_counter()
        r["model_cpu_s"] = {"counts": round(t1 - t0, 2), "smooth": round(t2 - t1, 2)}
        res = cw.cwipc_smooth(pc, radius)
        got = nm.xyz_of(res.get_numpy_array())
        res.free()
        ok = moved & (gap >= nm.GAP_MIN)
        steps = nm.ulp_steps(got[ok], out[ok])
        r["model_agrees"] = {"counts": bool(np.array_equal(mc, counts)), "moved": int(moved.sum()), "compared": int(ok.sum()),
                             "coordinates_adjacent": int((steps == 1).sum()), "coordinates_further": int((steps > 1).sum()),
                             "unmoved_bytes_equal": bool(got[~moved].tobytes() == xyz[~moved].tobytes())}
    return r


def main():
    with_model = "--no-model" not in sys.argv
    res = {}
    for label, npts, down in (("tile_36k", 300000, 0.01), ("synthetic_300k", 300000, None), ("synthetic_2m", 2000000, None)):
        pc = make_input(cw, npts, 0.0)
        cw.cwipc_hip_upload(pc, drop_host_copy=False)
        if down:
            small = cw.cwipc_downsample(pc, down)
            pc.free()
            pc = small
        res[label] = measure(pc, 3 * float(pc.cellsize()), with_model and pc.count() <= 1000000)      # (the model at 2 M points: minutes)
        res[label]["cellsize"] = float(pc.cellsize())
        print(label, json.dumps(res[label]), flush=True)
        pc.free()
    if len(sys.argv) > 1 and not sys.argv[1].startswith("--"):
        os.makedirs(os.path.dirname(sys.argv[1]) or ".", exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
