"""One side of the downsample A/B: the library comes from CWIPC_LIBRARY_DIR (unset: this tree's).  argv[1]: out.json.
--hash: sha256 of the four output planes (x, y, z, colour and tile) for cell sizes +0.01, -0.01 and +0.05 on the synthetic cloud at
36 k, 300 k, 2 M and 10 M points, the permuted 10 M cloud (five calls in a row: the partition pass engages), a 40-call stream
(deferred results) and the many-leaves random cloud.  --time: a single waited call at 300 k and 10 M and on the permuted 10 M cloud
(median of 10 after warm-up, ms).  Style of scratch/grid_ab.py: one side per process, compare the files."""
import hashlib, json, os, sys, time
sys.path.insert(0, os.getcwd())
import numpy as np
import torch  # noqa: F401
import cwipc_util_amd as cw
from bench import make_input
sync = cw.util.cwipc_util_dll_load().cwipc_hip_synchronize
CELLS = (0.01, -0.01, 0.05)

def planes(pc):
    a = pc.get_numpy_array()
    cols = np.stack([a['r'], a['g'], a['b'], a['tile']], axis=1)
    return "%d:" % len(a) + "-".join(hashlib.sha256(np.ascontiguousarray(p).tobytes()).hexdigest()[:16] for p in (a['x'], a['y'], a['z'], cols))

def waited(pc, cell, reps=10):
    for _ in range(5): cw.cwipc_downsample(pc, cell).count()
    sync()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); cw.cwipc_downsample(pc, cell).count(); sync(); t.append(time.perf_counter() - t0)
    return round(float(np.median(t)) * 1e3, 4)

def from_array(pts, cellsize):
    pc = cw.cwipc_from_numpy_array(pts, 4242)
    pc._set_cellsize(cellsize)
    cw.cwipc_hip_upload(pc, drop_host_copy=True)
    return pc

res = {"lib": cw.util.cwipc_util_dll_load()._name}
clouds = {}
for label, npts in (("300k", 300000), ("2m", 2000000), ("10m", 10000000)):
    pc = make_input(cw, npts, 0.0)
    cw.cwipc_hip_upload(pc, drop_host_copy=True)
    clouds[label] = pc
clouds["36k"] = cw.cwipc_downsample(clouds["300k"], 0.01)
big = make_input(cw, 10000000, 0.0)
pts = big.get_numpy_array()
clouds["10m_permuted"] = from_array(pts[np.random.default_rng(77).permutation(len(pts))], big.cellsize())
del big, pts

if "--hash" in sys.argv:
    hashes = {}
    for label in ("36k", "300k", "2m", "10m"):
        for cell in CELLS:
            hashes["%s %+.2f" % (label, cell)] = planes(cw.cwipc_downsample(clouds[label], cell))
    for cell in CELLS:
        hashes["10m_permuted %+.2f" % cell] = [planes(cw.cwipc_downsample(clouds["10m_permuted"], cell)) for _ in range(5)]
        outs = [cw.cwipc_downsample(clouds["300k"], cell) for _ in range(40)]
        hashes["stream40 %+.2f" % cell] = sorted(set(planes(o) for o in outs))
    rng = np.random.default_rng(33)
    n = 150000
    many = np.zeros(n, dtype=clouds["300k"].get_numpy_array().dtype)
    many['x'], many['y'], many['z'] = rng.random(n) * 3.0 - 1.5, rng.random(n) * 3.0, rng.random(n) * 3.0 - 1.0
    many['r'], many['g'], many['b'] = rng.integers(0, 256, n), rng.integers(0, 256, n), rng.integers(0, 256, n)
    many['tile'] = 1 << rng.integers(0, 8, n)
    pc = from_array(many, 0.0)
    for cell in CELLS:
        hashes["many_leaves %+.2f" % cell] = planes(cw.cwipc_downsample(pc, cell))
    res["hashes"] = hashes
if "--time" in sys.argv:
    res["waited_ms"] = {"300k": waited(clouds["300k"], 0.01), "10m": waited(clouds["10m"], 0.01), "10m_permuted": waited(clouds["10m_permuted"], 0.01)}
os.makedirs(os.path.dirname(sys.argv[1]) or ".", exist_ok=True)
json.dump(res, open(sys.argv[1], "w"), indent=1)
print(json.dumps(res)[:400], flush=True)
