"""Per-call time of the generalized ICP entry points at 36 k and 300 k points, device-resident, with point-to-plane on the same
pairs next to them.

    python scratch/icp_gicp_timing.py [out.json]

Source and reference are the two tiles of the synthetic figure, the source moved by 1 degree and 8 mm (the pairs of
scratch/icp_timing.py).  Per entry point: the median wall time of 30 calls (every one of them waits for its result before it
returns), after 5 warm-up calls, and the kernels' own time from hipEvents (cwipc_hip_profile, a run of its own).  The normals are
estimated inside every call (radius 0.02, max_nn 30; on both clouds for generalized ICP): their share is the direction_* kernels
in kernels_ms, the covariances' is gicp_covariance.  Both loops run with their classes' criteria (1e-7, 1e-7, 60) at a
correspondence of 5 cm, generalized ICP with epsilon 1e-3; their iteration counts are recorded next to the times."""
import json
import math
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import numpy as np
import torch  # noqa: F401
import cwipc_util_amd as cw
from bench import make_input

sync = cw.util.cwipc_util_dll_load().cwipc_hip_synchronize


def timed(fn, reps=30):
    for _ in range(5):
        fn()
    sync()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); sync(); t.append(time.perf_counter() - t0)
    out = {"call_ms_median": round(float(np.median(t)) * 1e3, 4), "call_ms_min": round(float(np.min(t)) * 1e3, 4),
           "call_ms_max": round(float(np.max(t)) * 1e3, 4)}
    with cw.cwipc_hip_profile() as prof:
        fn()
    out["kernels_ms"] = {k: round(v[0], 4) for k, v in prof.kernels.items()}
    out["kernels_ms_sum"] = round(sum(v[0] for v in prof.kernels.values()), 4)
    return out


def main():
    a = math.radians(1.0)
    move = np.array([[math.cos(a), 0, math.sin(a), 0.005], [0, 1, 0, 0.004], [-math.sin(a), 0, math.cos(a), -0.0048], [0, 0, 0, 1.0]])
    res = {}
    for label, npts in (("36k", 72000), ("300k", 600000)):
        pc = make_input(cw, npts, 0.0)
        ref = cw.cwipc_tilefilter(pc, 1)
        src = cw.cwipc_transform(cw.cwipc_tilefilter(pc, 2), move)
        for c in (ref, src):
            cw.cwipc_hip_upload(c, drop_host_copy=True)
        r = {"source_points": src.count(), "reference_points": ref.count()}
        ns, nr = cw.cwipc_hip_estimate_normals(src, 0.02, 30)[0], cw.cwipc_hip_estimate_normals(ref, 0.02, 30)[0]
        r["cwipc_hip_gicp_covariances"] = timed(lambda: cw.cwipc_hip_gicp_covariances(ref, None, 0.02, 30, (0.0, 0.0, 1.0), 1e-3))
        r["cwipc_hip_icp_gicp_sums"] = timed(lambda: cw.cwipc_hip_icp_gicp_sums(src, ref, None, 0.05, None, None, 0.02, 30, 1e-3))
        r["cwipc_hip_icp_gicp_sums, normals passed"] = timed(lambda: cw.cwipc_hip_icp_gicp_sums(src, ref, None, 0.05, ns, nr, 0.02, 30, 1e-3))
        r["cwipc_hip_icp_plane_sums"] = timed(lambda: cw.cwipc_hip_icp_plane_sums(src, ref, None, 0.05, None, 0.02, 30))
        T, fitness, rmse, iterations = cw.cwipc_hip_icp_generalized(src, ref, 0.05, None, None, None, 0.02, 30, 1e-3, 1e-7, 1e-7, 60)
        r["generalized"] = {"iterations": iterations, "fitness": fitness, "inlier_rmse": rmse}
        r["cwipc_hip_icp_generalized"] = timed(lambda: cw.cwipc_hip_icp_generalized(src, ref, 0.05, None, None, None, 0.02, 30, 1e-3, 1e-7, 1e-7, 60))
        T, fitness, rmse, iterations = cw.cwipc_hip_icp_point2plane(src, ref, 0.05, None, None, 0.02, 30, 1e-7, 1e-7, 60)
        r["point2plane"] = {"iterations": iterations, "fitness": fitness, "inlier_rmse": rmse}
        r["cwipc_hip_icp_point2plane"] = timed(lambda: cw.cwipc_hip_icp_point2plane(src, ref, 0.05, None, None, 0.02, 30, 1e-7, 1e-7, 60))
        res[label] = r
        print(label, json.dumps(r), flush=True)
    if len(sys.argv) > 1 and not sys.argv[1].startswith("--"):
        os.makedirs(os.path.dirname(sys.argv[1]) or ".", exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
