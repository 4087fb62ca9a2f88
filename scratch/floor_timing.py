"""Per-call time of the floor and tile helpers of the registration pipeline at 300 k and 2 M points, device-resident.

    python scratch/floor_timing.py [out.json]

The cloud is the synthetic figure (y from 0 to 2: a twentieth of it below the default level 0.1, tiles 1 and 2).  Per helper: the
median wall time of 30 calls (every one of them waits for its result before it returns), after 5 warm-up calls, and the kernels'
own time from hipEvents (cwipc_hip_profile, a run of its own).  cwipc_floor_filter is timed both ways (keep=False moves 95 % of the
cloud, keep=True 5 %)."""
import json
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
    res = {}
    for label, npts in (("300k", 300000), ("2m", 2000000)):
        pc = make_input(cw, npts, 0.0)
        cw.cwipc_hip_upload(pc, drop_host_copy=True)
        radius = cw.cwipc_compute_radius(pc)
        r = {"points": pc.count(), "floor_points": cw.cwipc_floor_filter(pc, keep=True).count(), "radius": [float(v) for v in radius]}
        r["cwipc_floor_filter"] = timed(lambda: cw.cwipc_floor_filter(pc))
        r["cwipc_floor_filter_keep"] = timed(lambda: cw.cwipc_floor_filter(pc, keep=True))
        r["cwipc_randomize_floor"] = timed(lambda: cw.cwipc_randomize_floor(pc, seed=1))
        r["cwipc_compute_tile_occupancy"] = timed(lambda: cw.cwipc_compute_tile_occupancy(pc))
        r["cwipc_compute_tile_occupancy_filterfloor"] = timed(lambda: cw.cwipc_compute_tile_occupancy(pc, 0, True))
        r["cwipc_compute_radius"] = timed(lambda: cw.cwipc_compute_radius(pc))
        r["cwipc_limit_floor_to_radius"] = timed(lambda: cw.cwipc_limit_floor_to_radius(pc, radius[2] * np.float32(0.5)))
        r["cwipc_hip_bounds"] = timed(lambda: cw.cwipc_hip_bounds(pc))
        # the yardstick from the same run: a tile filter that keeps about half of the cloud
        r["cwipc_tilefilter_1"] = timed(lambda: cw.cwipc_tilefilter(pc, 1))
        res[label] = r
        print(label, json.dumps(r), flush=True)
    if len(sys.argv) > 1 and not sys.argv[1].startswith("--"):
        os.makedirs(os.path.dirname(sys.argv[1]) or ".", exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
