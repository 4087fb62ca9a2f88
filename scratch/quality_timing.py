"""Per-call time of cwipc_hip_distortion at 300 k, 2 M and 10 M points, device-resident, against a decoded copy of the same cloud at 9,
10 and 12 octree bits, with and without CWIPC_HIP_DISTORTION_NO_PLANE; next to it the numpy model of the same rule
(tests/quality_model.py, tree=True: scipy's cKDTree names the candidates) on the same clouds where it finishes in reasonable time
(up to 2 M points), and one rate_distortion table of the synthetic cloud.

    python scratch/quality_timing.py [out.json] [--sizes 300000,2000000,10000000]

Per case: the median wall time of 10 calls (every one of them waits for its results before it returns), after 3 warm-up calls, and
the kernels' own time from hipEvents (cwipc_hip_profile, a run of its own).  With the plane term the original's normals are
estimated inside every call (radius 0.02, max_nn 30): their share is the direction_* kernels in kernels_ms; "normals passed" hands
them over instead.  What the numbers are measured against is the host model on the same clouds: it runs once, on one core, and its
time includes the two KD-tree builds."""
import json
import os
import sys
import time

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import numpy as np
import torch  # noqa: F401
import cwipc_util_amd as cw
import cwipc_util_amd.codec as codec
from cwipc_util_amd import quality
from bench import make_input

sync = cw.util.cwipc_util_dll_load().cwipc_hip_synchronize
MODEL_LIMIT = 2_000_000


def timed(fn, reps=10, warmup=3):
    for _ in range(warmup):
        fn()
    sync()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); sync(); t.append(time.perf_counter() - t0)
    out = {"call_ms_median": round(float(np.median(t)) * 1e3, 4), "call_ms_min": round(float(np.min(t)) * 1e3, 4),
           "call_ms_max": round(float(np.max(t)) * 1e3, 4), "reps": reps}
    with cw.cwipc_hip_profile() as prof:
        fn()
    out["kernels_ms"] = {k: round(v[0], 4) for k, v in prof.kernels.items()}
    out["kernels_ms_sum"] = round(sum(v[0] for v in prof.kernels.values()), 4)
    return out


def decoded_copy(pc, bits):
    enc, dec = codec.cwipc_new_encoder(octree_bits=bits, jpeg_quality=85), codec.cwipc_new_decoder()
    enc.feed(pc)
    assert enc.available(True)
    packet = enc.get_bytes()
    dec.feed(packet)
    assert dec.available(True)
    return dec.get(), len(packet)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    sizes = (300000, 2000000, 10000000)
    if "--sizes" in sys.argv:
        sizes = tuple(int(v) for v in sys.argv[sys.argv.index("--sizes") + 1].split(","))
        args = [a for a in args if a != sys.argv[sys.argv.index("--sizes") + 1]]
    res = {"cases": {}}
    for npts in sizes:
        pc = make_input(cw, npts, 0.0)
        cw.cwipc_hip_upload(pc, drop_host_copy=False)
        normals = cw.cwipc_hip_estimate_normals(pc, 0.02, 30)[0]
        for bits in (9, 10, 12):
            dec, nbytes = decoded_copy(pc, bits)
            r = {"original_points": pc.count(), "decoded_points": dec.count(), "packet_bytes": nbytes}
            r["cwipc_hip_distortion"] = timed(lambda: cw.cwipc_hip_distortion(pc, dec))
            r["cwipc_hip_distortion, normals passed"] = timed(lambda: cw.cwipc_hip_distortion(pc, dec, normals=normals))
            r["cwipc_hip_distortion, NO_PLANE"] = timed(lambda: cw.cwipc_hip_distortion(pc, dec, plane=False))
            got = quality.cloud_distortion(pc, dec, normals=normals)
            r["psnr"] = {k: getattr(got, k) for k in ("psnr_d1", "psnr_d2", "psnr_y", "psnr_u", "psnr_v")}
            if pc.count() <= MODEL_LIMIT:
                import quality_model as qm
                A, B = pc.get_numpy_array(), dec.get_numpy_array()
                t0 = time.perf_counter()
                fwd, bwd = qm.distortion(A, B, np.inf, normals, tree=True)
                sums = qm.sums(fwd), qm.sums(bwd)
                r["numpy_model_s"] = round(time.perf_counter() - t0, 3)
                r["numpy_model_agrees"] = bool(fwd["n"] == got.forward.n and bwd["n"] == got.backward.n and sums[0]["sum_rgb2"] ==
                                               [round(m * got.forward.n) for m in got.forward.mse_rgb])
            res["cases"]["%d points, %d bits" % (npts, bits)] = r
            print(npts, bits, json.dumps(r), flush=True)
            del dec
        if npts == sizes[0]:
            settings = [dict(octree_bits=b, jpeg_quality=q, entropy=e) for b in (7, 8, 9, 10, 12) for q in (60, 85) for e in (False, True)]
            res["rate_distortion"] = {"points": pc.count(), "rows": quality.rate_distortion(pc, settings)}
    if args:
        os.makedirs(os.path.dirname(args[0]) or ".", exist_ok=True)
        with open(args[0], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
