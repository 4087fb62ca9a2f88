"""Per-call time of the direction filter against the outlier filter of the same search width (remove_outliers(29, 1.0):
max_nn = 30 neighbours, the point itself among them) on one cloud, and the numpy oracle's CPU time for context.

    python scratch/direction_timing.py [out.json]

Sizes: a camera tile as config 5 filters it (the synthetic 300 k cloud through downsample(0.01), ~36 k points), the 300 k
tile itself, the synthetic source at 2 M and 10 M points.  Per call: the median wall time of a call that is waited for
(settled) and the mean of 20 calls back to back on the thread's stream with one wait at the end (in a stream); the kernels'
split from hipEvents (cwipc_hip_profile)."""
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
    settled = float(np.median(t)) * 1e3
    t0 = time.perf_counter()
    for _ in range(20):
        fn()
    sync()
    stream = (time.perf_counter() - t0) / 20 * 1e3
    with cw.cwipc_hip_profile() as prof:
        fn()
    return {"settled_ms": round(settled, 4), "in_stream_ms": round(stream, 4), "kernels_ms": {k: round(v[0], 4) for k, v in prof.kernels.items()}}


def main():
    res = {}
    for label, npts, down in (("tile_36k", 300000, 0.01), ("tile_300k", 300000, None), ("synthetic_2m", 2000000, None), ("synthetic_10m", 10000000, None)):
        pc = make_input(cw, npts, 0.0)
        cw.cwipc_hip_upload(pc, drop_host_copy=True)
        if down:
            pc = cw.cwipc_downsample(pc, down)
        n = pc.count()
        r = {"points": n,
             "direction": timed(lambda: cw.cwipc_direction_filter(pc, (0, 0, 1), 0.5)),
             "remove_outliers_29": timed(lambda: cw.cwipc_remove_outliers(pc, 29, 1.0, False)),
             "remove_outliers_16": timed(lambda: cw.cwipc_remove_outliers(pc, 16, 1.0, False))}   # (README's row: unchanged by the grid's new caller)
        r["ratio_settled"] = round(r["direction"]["settled_ms"] / r["remove_outliers_29"]["settled_ms"], 3)
        # the oracle (numpy, one CPU thread): the whole cloud up to 300 k points, else 20 k sampled queries scaled up
        if "--no-oracle" not in sys.argv:
            import direction_oracle as do
            arr = pc.get_numpy_array()
            xyz = np.column_stack([arr["x"], arr["y"], arr["z"]])
            q = None if n <= 40000 else np.random.default_rng(0).choice(n, 20000, replace=False)
            t0 = time.perf_counter()
            do.estimate(xyz, query=q)
            dt = time.perf_counter() - t0
            r["oracle_cpu_s"] = round(dt, 2)
            r["oracle_cpu_note"] = "whole cloud" if q is None else "20 k sampled queries against the whole cloud (its grid build included)"
        res[label] = r
        print(label, json.dumps(r), flush=True)
    if len(sys.argv) > 1 and not sys.argv[1].startswith("--"):
        os.makedirs(os.path.dirname(sys.argv[1]) or ".", exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
