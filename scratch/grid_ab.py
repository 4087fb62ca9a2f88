"""One side of the A/B: the library comes from CWIPC_LIBRARY_DIR (unset: this tree's).  Workloads and method of
scratch/sor_small.py, scratch/direction_timing.py, scratch/analyze_timing.py (settled median of 10 waited-for calls,
20 calls in a stream), without their CPU oracles; the search kernel from hipEvents as the median of 15 calls profiled one by
one (those scripts profile one call: too few to compare two builds of a 30 us kernel).  argv[1]: out.json; --hash: also sha256
of results."""
import hashlib, json, os, sys, time
sys.path.insert(0, os.getcwd())
import numpy as np
import torch  # noqa: F401
import cwipc_util_amd as cw
from bench import make_input
sync = cw.util.cwipc_util_dll_load().cwipc_hip_synchronize

def timed(fn, reps=10):
    for _ in range(3): fn()
    sync()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); sync(); t.append(time.perf_counter() - t0)
    out = {"settled_ms": round(float(np.median(t)) * 1e3, 4)}
    t0 = time.perf_counter()
    for _ in range(20): fn()
    sync()
    out["in_stream_ms"] = round((time.perf_counter() - t0) / 20 * 1e3, 4)
    ks = {}
    for _ in range(15):
        with cw.cwipc_hip_profile() as prof:
            fn()
        for k, v in prof.kernels.items():
            if k in ("sor_knn_mean_dist", "direction_normals", "nn_distance2"): ks.setdefault(k, []).append(v[0])
    out["kernels_ms"] = {k: round(float(np.median(v)), 4) for k, v in ks.items()}
    return out

def h(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]

res, hashes = {"lib": cw.util.cwipc_util_dll_load()._name}, {}
want_hash = "--hash" in sys.argv
a = np.radians(0.5)
m = np.array([[np.cos(a), 0, np.sin(a), 0.003], [0, 1, 0, 0.0], [-np.sin(a), 0, np.cos(a), 0.0], [0, 0, 0, 1.0]])
for label, npts, down in (("36k", 300000, 0.01), ("300k", 300000, None), ("2m", 2000000, None), ("10m", 10000000, None)):
    pc = make_input(cw, npts, 0.0)
    cw.cwipc_hip_upload(pc, drop_host_copy=True)
    if down: pc = cw.cwipc_downsample(pc, down)
    r = {"points": pc.count()}
    r["sor16"] = timed(lambda: cw.cwipc_remove_outliers(pc, 16, 1.0, False))
    r["sor29"] = timed(lambda: cw.cwipc_remove_outliers(pc, 29, 1.0, False))
    r["direction30"] = timed(lambda: cw.cwipc_direction_filter(pc, (0, 0, 1), 0.5))
    if label != "10m":
        r["direction64"] = timed(lambda: cw.cwipc_direction_filter(pc, (0, 0, 1), 0.5, max_nn=64))
    src = cw.cwipc_transform(pc, m)
    for nth in (0, 1):
        r["nn%d" % nth] = timed(lambda: cw.cwipc_hip_nn_distance(src, pc, nth))
    res[label] = r
    print(label, json.dumps(r), flush=True)
    if want_hash and label != "10m":
        for k in (1, 2, 16, 29, 32, 40):
            d, thr = cw.cwipc_hip_knn_mean_dist(pc, k)
            hashes["%s_knn%d" % (label, k)] = h(d) + ":" + repr(float(thr))
        for nn in (30, 64, 128):
            if nn > 30 and label == "2m": continue
            out = cw.cwipc_hip_estimate_normals(pc, 0.02, nn)
            hashes["%s_normals%d" % (label, nn)] = "-".join(h(x) for x in out)
        for nth in (0, 1, 3, 7):
            hashes["%s_nn%d" % (label, nth)] = h(cw.cwipc_hip_nn_distance(src, pc, nth))
        hashes["%s_nn0_max" % label] = h(cw.cwipc_hip_nn_distance(src, pc, 0, 0.004))
        hashes["%s_sor16_out" % label] = h(cw.cwipc_remove_outliers(pc, 16, 1.0, False).get_numpy_array())
        hashes["%s_dir_out" % label] = h(cw.cwipc_direction_filter(pc, (0, 0, 1), 0.5).get_numpy_array())
        print(label, "hashes done", flush=True)
if want_hash: res["hashes"] = hashes
os.makedirs(os.path.dirname(sys.argv[1]) or ".", exist_ok=True)
json.dump(res, open(sys.argv[1], "w"), indent=1)
