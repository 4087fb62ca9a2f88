"""Per-call time of cwipc_hip_render at 36 k, 300 k, 2 M and 10 M points, 1920 x 1080, point sizes 1 and 5, device-resident.

    python scratch/render_timing.py [out.json] [--max-points N]

The cloud is a synthetic one: points spread evenly over the box x in [-1, 1], y in [0, 2], z in [-0.5, 0.5] (a person's volume),
random colours, seeded.  The view is default_view() with the extrinsic look_at((0, 1, -3), (0, 1, 0), up).  Per case: the median wall
time of 20 calls (every call waits for its images, which it copies to the caller's arrays, before it returns), after 3 warm-up calls,
and the three kernels' own time from hipEvents (cwipc_hip_profile, a run of its own), with the share of covered pixels."""
import json
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import numpy as np
import torch  # noqa: F401
import cwipc_util_amd as cw
from cwipc_util_amd.registration.render import default_view, look_at

sync = cw.util.cwipc_util_dll_load().cwipc_hip_synchronize


def timed(fn, reps=20):
    for _ in range(3):
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


def make_cloud(npts, seed=1):
    rng = np.random.default_rng(seed)
    pts = np.zeros(npts, dtype=cw.cwipc_point_numpy_dtype)
    pts['x'] = rng.uniform(-1.0, 1.0, npts)
    pts['y'] = rng.uniform(0.0, 2.0, npts)
    pts['z'] = rng.uniform(-0.5, 0.5, npts)
    pts['r'], pts['g'], pts['b'] = rng.integers(0, 256, (3, npts))
    pts['tile'] = 1
    pc = cw.cwipc_from_numpy_array(pts, 0)
    cw.cwipc_hip_upload(pc, drop_host_copy=True)
    return pc


def main():
    max_points = int(sys.argv[sys.argv.index("--max-points") + 1]) if "--max-points" in sys.argv else 10_000_000
    view = default_view(extrinsic=look_at((0, 1, -3), (0, 1, 0), (0, 1, 0))).as_struct()
    res = {"image": [view.width, view.height]}
    for label, npts in (("36k", 36_000), ("300k", 300_000), ("2M", 2_000_000), ("10M", 10_000_000)):
        if npts > max_points:
            continue
        pc = make_cloud(npts)
        r = {"points": pc.count()}
        for point_size in (1, 5):
            _rgb, _depth, index = cw.cwipc_hip_render(pc, view, point_size)
            case = timed(lambda: cw.cwipc_hip_render(pc, view, point_size))
            case["covered_share"] = round(float((index >= 0).mean()), 4)
            r["point_size_%d" % point_size] = case
        res[label] = r
        print(label, json.dumps(r), flush=True)
    if len(sys.argv) > 1 and not sys.argv[1].startswith("--"):
        os.makedirs(os.path.dirname(sys.argv[1]) or ".", exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
