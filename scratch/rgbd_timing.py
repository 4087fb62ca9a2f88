"""Per-frame time of the RGB-D source (cwipc_hip_from_rgbd) for a capture of four cameras, against the host path it replaces (the
numpy model of the same arithmetic, then cwipc_from_points and the upload of 16 bytes per point).

    python scratch/rgbd_timing.py [out.json]

Frames: 4 x 1280 x 720 and 4 x 640 x 480, RGB8, depth with about 30 % holes, the depth-range and radius filters on.  Per frame:
the whole call waited for (median of 10), with the images in ordinary memory and in page-locked memory; its kernels from hipEvents
(cwipc_hip_profile); and, for the uploads, the same number of bytes copied from page-locked memory to the device by torch, waited for:
what the bus takes for them."""
import json
import os
import sys
import time

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import numpy as np
import torch
import cwipc_util_amd as cw
import rgbd_model as rm
from cwipc_util_amd.rgbd import RgbdCamera, RgbdFilter, from_rgbd

sync = cw.util.cwipc_util_dll_load().cwipc_hip_synchronize


def median_ms(fn, reps=10, warm=3):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); sync(); t.append(time.perf_counter() - t0)
    return round(float(np.median(t)) * 1e3, 4)


def pinned_copy(a, keep):
    raw = cw.cwipc_hip_pinned_points((a.nbytes + 15) // 16)
    keep.append(raw)
    out = raw.view(np.uint8)[:a.nbytes].view(a.dtype).reshape(a.shape)
    out[...] = a
    return out


def main():
    cw.cwipc_hip_set_device(0)
    rng = np.random.default_rng(1)
    flt, model_flt = RgbdFilter(0.4, 3.5, radius=3.0), rm.Filter(0.4, 3.5, radius=3.0)
    res = {}
    for label, width, height in (("4x1280x720", 1280, 720), ("4x640x480", 640, 480)):
        cams, model_cams, frame = [], [], []
        for k in range(4):
            m = rm.random_rigid(rng, 1.0)
            fx = 0.9 * width
            cams.append(RgbdCamera(width, height, fx, fx, width / 2.0, height / 2.0, 0.001, m, 1 << k, "cam%d" % k))
            model_cams.append(rm.Camera(fx, fx, width / 2.0, height / 2.0, 0.001, m, 1 << k, 3))
            depth = rng.integers(300, 4000, (height, width)).astype(np.uint16)
            depth[rng.random((height, width)) < 0.3] = 0
            frame.append((depth, rng.integers(0, 256, (height, width, 3)).astype(np.uint8)))
        keep = []
        pinned_frame = [(pinned_copy(d, keep), pinned_copy(c, keep)) for d, c in frame]
        nbytes = sum(d.nbytes + c.nbytes for d, c in frame)
        points = from_rgbd(cams, frame, flt).count()
        r = {"pixels": 4 * width * height, "points": points, "image_bytes": nbytes,
             "call_pageable_ms": median_ms(lambda: from_rgbd(cams, frame, flt)),
             "call_pinned_ms": median_ms(lambda: from_rgbd(cams, pinned_frame, flt))}
        with cw.cwipc_hip_profile() as prof:
            from_rgbd(cams, pinned_frame, flt)
        r["kernels_ms"] = {k: round(v[0], 4) for k, v in prof.kernels.items()}
        r["kernels_total_ms"] = round(sum(v[0] for v in prof.kernels.values()), 4)
        host = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
        dev = torch.empty(nbytes, dtype=torch.uint8, device="cuda")

        def upload():
            dev.copy_(host, non_blocking=True)
            torch.cuda.synchronize()
        r["upload_same_bytes_pinned_ms"] = median_ms(upload)
        # the host path: the model's points (numpy, one thread), then a cloud from them, made device-resident

        def host_path():
            pts = rm.cloud(model_cams, frame, model_flt)
            cw.cwipc_hip_upload(cw.cwipc_from_numpy_array(pts, 0))
        r["numpy_then_from_points_ms"] = median_ms(host_path, reps=3, warm=1)
        pts = rm.cloud(model_cams, frame, model_flt)
        r["from_points_and_upload_alone_ms"] = median_ms(lambda: cw.cwipc_hip_upload(cw.cwipc_from_numpy_array(pts, 0)))
        res[label] = r
        print(label, json.dumps(r), flush=True)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(sys.argv[1]) or ".", exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
