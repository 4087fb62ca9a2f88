"""Per-call time of the seeded random filters -- cwipc_hip_noise, soft simulatecams -- and of the analysis-test creator end to end at
300 k, 2 M and 10 M points, device-resident, against the path the library had for the same work before them.

    python scratch/scene_timing.py [out.json]

Device path: the median wall time of 30 calls (every one waits for its result), after 5 warm-up calls, and the kernels' own time from
hipEvents (cwipc_hip_profile, a run of its own).  Yardstick, on the same clouds: the numpy expression of the reference's NoiseFilter
(python/cwipc/filters/noise.py:31-50) between its two copies across the bus (get_numpy_matrix, cwipc_from_numpy_matrix + upload), and
the host fallback SimulatecamsFilter(hard=False) had (dot products, sort, numpy.random draws and the rebuild in numpy); fewer calls of
those, they take seconds at 10 M.  The soft rule is timed through the filter both ways, centroid included (one download, unchanged)."""
import json
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import numpy as np
import torch  # noqa: F401
import cwipc_util_amd as cw
from bench import make_input
from cwipc_util_amd.filters.simulatecams import SimulatecamsFilter
from cwipc_util_amd.scripts.cwipc_create_analysis_test import AnalysisTestCreator, build_parser

sync = cw.util.cwipc_util_dll_load().cwipc_hip_synchronize
NCAM = 4


def timed(fn, reps=30, warm=5, profile=True):
    for _ in range(warm):
        fn()
    sync()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); sync(); t.append(time.perf_counter() - t0)
    out = {"calls": reps, "call_ms_median": round(float(np.median(t)) * 1e3, 4), "call_ms_min": round(float(np.min(t)) * 1e3, 4),
           "call_ms_max": round(float(np.max(t)) * 1e3, 4)}
    if profile:
        with cw.cwipc_hip_profile() as prof:
            fn()
        out["kernels_ms"] = {k: round(v[0], 4) for k, v in prof.kernels.items()}
        out["kernels_ms_sum"] = round(sum(v[0] for v in prof.kernels.values()), 4)
    return out


def host_noise(pc, distance):
    """the reference filter's numpy expression, the cloud down and up again"""
    m = pc.get_numpy_matrix()
    n = m.shape[0]
    vec = np.random.uniform(-1, 1, (n, 3))
    unif = np.random.uniform(0, 1, n)
    vec = vec / np.expand_dims(np.linalg.norm(vec, axis=1) / unif, axis=1)
    xyz = m[:, :3]
    xyz += vec * distance
    out = cw.cwipc_from_numpy_matrix(m, pc.timestamp())
    out._set_cellsize(pc.cellsize())
    cw.cwipc_hip_upload(out)
    return out


def host_soft_cameras(pc, cams, skew):
    """SimulatecamsFilter(hard=False) as it was: everything behind the centroid on the host"""
    m = pc.get_numpy_matrix()
    centroid = np.mean(m[:, :3], axis=0)
    centroid[1] = 0.0
    flat = m[:, :3].copy()
    flat[:, 1] = 0.0
    flat -= centroid
    dots = flat.astype(float) @ cams.T
    order = np.argsort(dots, axis=1, kind="stable")[:, ::-1]
    first, second = order[:, 0], order[:, 1]
    rows = np.arange(len(flat))
    w0, w1 = dots[rows, first] ** skew, dots[rows, second] ** skew
    chance = np.random.uniform(-w0, w1)
    m[:, 6] = (1 << np.where(chance < 0, first, second)).astype(np.float32)
    out = cw.cwipc_from_numpy_matrix(m, pc.timestamp())
    out._set_cellsize(pc.cellsize())
    cw.cwipc_hip_upload(out)
    return out


def main():
    res = {}
    for label, npts in (("300k", 300000), ("2m", 2000000), ("10m", 10000000)):
        pc = make_input(cw, npts, 0.0)
        cw.cwipc_hip_upload(pc)
        slow = 3 if npts > 2000000 else 5
        r = {"points": pc.count(), "cameras": NCAM}
        r["cwipc_hip_noise"] = timed(lambda: cw.cwipc_hip_noise(pc, 0.005, 1))
        r["host_noise"] = timed(lambda: host_noise(pc, 0.005), reps=slow, warm=1, profile=False)
        soft, cams = SimulatecamsFilter(NCAM, False, 1.0, seed=1), SimulatecamsFilter(NCAM, True).camera_vectors
        r["simulatecams_soft_filter"] = timed(lambda: soft.filter(pc), reps=10, warm=2)
        centroid = np.zeros(3, dtype=np.float32)
        r["cwipc_hip_simulatecams_soft"] = timed(lambda: cw.cwipc_hip_simulatecams_soft(pc, cams, centroid, 1.0, seed=1))
        r["cwipc_hip_simulatecams_soft_skew2.5"] = timed(lambda: cw.cwipc_hip_simulatecams_soft(pc, cams, centroid, 2.5, seed=1))
        r["host_simulatecams_soft"] = timed(lambda: host_soft_cameras(pc, cams, 1.0), reps=slow, warm=1, profile=False)
        args = build_parser().parse_args(["in.ply", "out.ply", "--ncamera", str(NCAM), "--move", "0", "--move", "0.03", "--rotate", "0", "--rotate", "0",
                                          "--rotate", "0.02", "--noise", "0.005", "--seed", "42"])

        def create():
            c = AnalysisTestCreator(args, input_pc=pc)
            c.run()
            return c.output_pc
        r["creator_end_to_end"] = timed(create, reps=10, warm=2, profile=False)
        res[label] = r
        print(label, json.dumps(r), flush=True)
    if len(sys.argv) > 1 and not sys.argv[1].startswith("--"):
        os.makedirs(os.path.dirname(sys.argv[1]) or ".", exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
