"""One _pre_analyse pass of the multi-camera layer on a 4-camera frame, with batch_analysis on and off, device-resident.

    python scratch/multicamera_timing.py [out.json]

The frame is the synthetic figure cut into four cameras by overlapping angular sectors, with a floor band (tests/multicam_frames.py),
at about 72 k and 600 k points.  Per pass -- every camera against all the others with the symmetric analyzer (eight searches), and
every camera against itself (four) -- and per mode: the median wall time of 20 passes after 3 warm-up passes (a pass waits for its
results: it reads the distances back), and the kernels' own time from hipEvents (cwipc_hip_profile, a pass of its own).  The density
estimate and the host reductions are the same work in both modes and are inside both numbers."""
import json
import os
import sys
import time

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import numpy as np
import torch  # noqa: F401
import cwipc_util_amd as cw
from cwipc_util_amd.registration import MultiCameraOneToAllOthers, RegistrationAnalyzerSymmetric
from oracle import oracle
from multicam_frames import make_frame

sync = cw.util.cwipc_util_dll_load().cwipc_hip_synchronize


def timed(fn, reps=20):
    for _ in range(3):
        fn()
    sync()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); sync(); t.append(time.perf_counter() - t0)
    out = {"pass_ms_median": round(float(np.median(t)) * 1e3, 3), "pass_ms_min": round(float(np.min(t)) * 1e3, 3),
           "pass_ms_max": round(float(np.max(t)) * 1e3, 3)}
    with cw.cwipc_hip_profile() as prof:
        fn()
    out["kernels_ms"] = {k: round(v[0], 4) for k, v in prof.kernels.items()}
    out["kernels_ms_sum"] = round(sum(v[0] for v in prof.kernels.values()), 4)
    return out


def main():
    oracle.load()
    res = {}
    for label, npts in (("72k", 72000), ("600k", 600000)):
        pts, _ = oracle.synthetic(int(npts / 1.12), 0.0)
        pc = cw.cwipc_from_numpy_array(make_frame(pts, 4, seed=1), 0)
        cw.cwipc_hip_upload(pc, drop_host_copy=True)
        r = {"points": pc.count()}
        for batch in (True, False):
            alg = MultiCameraOneToAllOthers()
            alg.batch_analysis = batch
            alg.set_analyzer_class(RegistrationAnalyzerSymmetric)
            alg.set_tiled_pointcloud(pc)
            alg._init_transformations()
            mode = "batched" if batch else "per_analyzer"
            r["to_others_" + mode] = timed(lambda: alg._pre_analyse(toSelf=False, ignoreFloor=True))
            r["to_self_" + mode] = timed(lambda: alg._pre_analyse(toSelf=True, ignoreFloor=True))
        res[label] = r
        print(label, json.dumps(r), flush=True)
    if len(sys.argv) > 1 and not sys.argv[1].startswith("--"):
        os.makedirs(os.path.dirname(sys.argv[1]) or ".", exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
