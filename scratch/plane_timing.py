"""Per-call time of plane segmentation (cwipc_find_plane with and without the refit, cwipc_plane_filter, the level_floor filter;
RULE S) against two neighbours in a chain -- remove_outliers(16, 1.0) and cwipc_hip_floor_partition -- on the same cloud in the same
run, and against the numpy model on the CPU where that is feasible.

    python scratch/plane_timing.py [out.json] [--no-model]

Clouds: a camera tile (the 300 k synthetic cloud voxelized at 0.01: about 36 k points) and the synthetic source at 300 k and 2.0 M
points, each with a noisy tilted floor added that holds 30 % of the result (the synthetic source is a figure without a floor).
distance = 0.01; H = 256, 1024, 4096.  Per entry: the median wall time of 10 calls that are waited for (settled) after 3 warm-up
calls; the time per call of 20 calls issued back to back (in a stream); the kernels' split from hipEvents (cwipc_hip_profile), the
score kernel's share of it and its time per (point x hypothesis)."""
import json
import os
import sys
import time

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import numpy as np
import torch  # noqa: F401
import cwipc_util_amd as cw
from cwipc_util_amd import filters
from bench import make_input

sync = cw.util.cwipc_util_dll_load().cwipc_hip_synchronize
DISTANCE = 0.01


def timed(fn, reps=10):
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
    return {"settled_ms": round(float(np.median(t)) * 1e3, 4), "min_ms": round(float(np.min(t)) * 1e3, 4), "in_stream_ms": round(stream * 1e3, 4),
            "kernels_ms": kernels}


def with_floor(pc):
    """the cloud's points and a tilted noisy floor under them, shuffled"""
    import plane_model as pm
    arr = pc.get_numpy_array()
    rng = np.random.default_rng(1)
    nf = int(len(arr) * 0.3 / 0.7)
    lo = float(arr["y"].min())
    floor = np.stack([rng.uniform(-1.5, 1.5, nf), lo + rng.normal(0, 0.004, nf), rng.uniform(-1.5, 1.5, nf)], axis=1)
    fl = np.zeros(nf, dtype=arr.dtype)
    both = np.concatenate([arr, fl])
    xyz = np.stack([both["x"], both["y"], both["z"]], axis=1).astype(np.float64)
    xyz[len(arr):] = floor
    xyz = xyz @ pm.rotation_about((1.0, 0.0, 0.5), 7.0).T
    both["x"], both["y"], both["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    both["tile"][len(arr):] = 1
    out = cw.cwipc_from_numpy_array(both[rng.permutation(len(both))], 1)
    cw.cwipc_hip_upload(out, drop_host_copy=False)
    return out


def measure(pc, with_model):
    n = pc.count()
    r = {"points": n, "distance": DISTANCE}
    for H in (256, 1024, 4096):
        found = cw.cwipc_find_plane(pc, DISTANCE, H)
        e = {"count": found.count, "recount": found.recount, "refined": found.refined, "valid": found.valid}
        e["find_plane_refine"] = timed(lambda: cw.cwipc_find_plane(pc, DISTANCE, H))
        e["find_plane_no_refine"] = timed(lambda: cw.cwipc_find_plane(pc, DISTANCE, H, refine=False))
        k = e["find_plane_no_refine"]["kernels_ms"]
        e["score_kernel_share"] = round(k.get("plane_score", 0.0) / max(sum(k.values()), 1e-9), 3)
        e["score_ps_per_point_hypothesis"] = round(k.get("plane_score", 0.0) * 1e9 / (n * found.valid), 4)
        e["score_share_of_settled_call"] = round(k.get("plane_score", 0.0) / e["find_plane_no_refine"]["settled_ms"], 3)
        r["H_%d" % H] = e
    plane = cw.cwipc_find_plane(pc, DISTANCE, 1024).plane
    r["plane_filter_rest"] = timed(lambda: cw.cwipc_plane_filter(pc, plane, DISTANCE).free())
    level = filters.factory("level_floor(%r)" % DISTANCE)
    r["level_floor_filter_H4096"] = timed(lambda: level.filter(pc).free())
    r["remove_outliers_16"] = timed(lambda: cw.cwipc_remove_outliers(pc, 16, 1.0, False).free())
    r["floor_partition"] = timed(lambda: cw.cwipc_hip_floor_partition(pc, 0.1, 3)[0].free())
    if with_model:
        import plane_model as pm
        arr = pc.get_numpy_array()
        xyz = np.stack([arr["x"], arr["y"], arr["z"]], axis=1)
        t0 = time.perf_counter()
        want = pm.find(xyz, DISTANCE, 1024)
        r["model_cpu_s_H1024"] = round(time.perf_counter() - t0, 2)
        r["model_agrees_H1024"] = bool(want.tobytes() == cw.cwipc_find_plane(pc, DISTANCE, 1024).tobytes())
    return r


def main():
    with_model = "--no-model" not in sys.argv
    res = {}
    for label, npts, down in (("tile_36k", 300000, 0.01), ("synthetic_300k", 300000, None), ("synthetic_2m", 2000000, None)):
        pc = make_input(cw, int(npts * 0.7), 0.0)
        if down:
            cw.cwipc_hip_upload(pc, drop_host_copy=False)
            small = cw.cwipc_downsample(pc, down)
            pc.free()
            pc = small
        full = with_floor(pc)
        pc.free()
        res[label] = measure(full, with_model and full.count() <= 1000000)      # (the model at 2 M points and 1024 hypotheses: minutes)
        print(label, json.dumps(res[label]), flush=True)
        full.free()
    if len(sys.argv) > 1 and not sys.argv[1].startswith("--"):
        os.makedirs(os.path.dirname(sys.argv[1]) or ".", exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
