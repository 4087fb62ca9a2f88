"""Per-frame time of the RGB-D source's raw entry (cwipc_hip_rgbd_rig_grab) for a capture of four cameras, beside the aligned entry
(cwipc_hip_from_rgbd) at the same depth sizes and beside the numpy model of the same arithmetic on the same frames.

    python scratch/rgbd_raw_timing.py [out.json]

Frames: 4 x (640 x 576 depth, 1280 x 720 colour) and 4 x (640 x 480 depth, 640 x 480 colour), RGB8, rational lenses on both sensors,
the colour sensor 32 mm to the side, depth with rectangular holes (about 15 %), erosion 2 / 2, the depth-range and radius filters on.
Per frame: the whole call waited for (median of 10), images in ordinary and in page-locked memory; its kernels from hipEvents
(cwipc_hip_profile) with their launch counts; the bytes uploaded; the rig's creation (ray tables, once).  The aligned entry gets
depth-sized colour images of the same cameras without lenses; the parent commit's run of it is quoted from profiles/rgbd_timing.json."""
import json
import os
import sys
import time

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import numpy as np
import torch  # noqa: F401  (first: it brings the HIP runtime the library then shares)
import cwipc_util_amd as cw
import rgbd_lens_model as lm
import rgbd_model as rm
from cwipc_util_amd.rgbd import RgbdCamera, RgbdFilter, RgbdPrep, RgbdRig, RgbdSensor, from_rgbd

sync = cw.util.cwipc_util_dll_load().cwipc_hip_synchronize
DEPTH_LENS = (4.9, 3.1, 1e-4, -5e-5, 0.16, 5.2, 4.8, 0.85)
COLOUR_LENS = (0.4569, -2.7217, 4.7e-4, -1.6e-4, 1.5964, 0.3335, -2.5460, 1.5223)


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


def holed_depth(rng, width, height):
    depth = rng.integers(300, 4000, (height, width)).astype(np.uint16)
    for _ in range(40):
        w, h = rng.integers(8, 60, 2)
        u, v = rng.integers(0, width - w), rng.integers(0, height - h)
        depth[v:v + h, u:u + w] = 0
    return depth


def main():
    cw.cwipc_hip_set_device(0)
    rng = np.random.default_rng(1)
    flt, model_flt = RgbdFilter(0.4, 3.5, radius=3.0), rm.Filter(0.4, 3.5, radius=3.0)
    prep = RgbdPrep(2, 2)
    d2c = np.identity(4)
    d2c[0, 3] = -0.032
    res = {}
    for label, (w, h), (wc, hc) in (("4x640x576+1280x720", (640, 576), (1280, 720)), ("4x640x480+640x480", (640, 480), (640, 480))):
        fx, fy, cx, cy = 504.0 * w / 640, 504.0 * h / 576, 320.0 * w / 640, 330.0 * h / 576
        cfx, cfy, ccx, ccy = 607.0 * wc / 1280, 607.0 * hc / 720, 638.0 * wc / 1280, 367.0 * hc / 720
        sensors, models, aligned, frame, aligned_frame = [], [], [], [], []
        for k in range(4):
            m = rm.random_rigid(rng, 1.0)
            sensors.append(RgbdSensor(w, h, fx, fy, cx, cy, wc, hc, cfx, cfy, ccx, ccy, DEPTH_LENS, COLOUR_LENS, d2c, 0.001, m, 1 << k, "cam%d" % k))
            models.append(lm.Sensor(w, h, fx, fy, cx, cy, DEPTH_LENS, 0.001, (wc, hc), 3, (cfx, cfy, ccx, ccy), COLOUR_LENS, d2c, m, 1 << k))
            aligned.append(RgbdCamera(w, h, fx, fy, cx, cy, 0.001, m, 1 << k, "cam%d" % k))
            depth = holed_depth(rng, w, h)
            frame.append((depth, rng.integers(0, 256, (hc, wc, 3)).astype(np.uint8)))
            aligned_frame.append((depth, rng.integers(0, 256, (h, w, 3)).astype(np.uint8)))
        keep = []
        pinned_frame = [(pinned_copy(d, keep), pinned_copy(c, keep)) for d, c in frame]
        pinned_aligned = [(pinned_copy(d, keep), pinned_copy(c, keep)) for d, c in aligned_frame]
        t0 = time.perf_counter()
        rig = RgbdRig(sensors)
        create_ms = round((time.perf_counter() - t0) * 1e3, 2)
        r = {"depth_pixels": 4 * w * h, "colour_pixels": 4 * wc * hc, "holes_share": round(float(np.mean([(d == 0).mean() for d, _c in frame])), 4),
             "points": rig.grab(frame, flt, prep).count(), "uploaded_bytes_per_call": sum(d.nbytes + c.nbytes for d, c in frame),
             "ray_table_bytes_on_device": 4 * w * h * 16, "rig_create_ms": create_ms,
             "call_pageable_ms": median_ms(lambda: rig.grab(frame, flt, prep)), "call_pinned_ms": median_ms(lambda: rig.grab(pinned_frame, flt, prep)),
             "call_pinned_no_erosion_ms": median_ms(lambda: rig.grab(pinned_frame, flt))}
        with cw.cwipc_hip_profile() as prof:
            rig.grab(pinned_frame, flt, prep)
        r["kernels_ms"] = {k: round(v[0], 4) for k, v in prof.kernels.items()}
        r["kernel_launches"] = {k: int(v[1]) for k, v in prof.kernels.items()}
        r["launches_per_call"] = int(sum(v[1] for v in prof.kernels.values()))
        r["kernels_total_ms"] = round(sum(v[0] for v in prof.kernels.values()), 4)
        # the aligned entry at the same depth size (this build; its code is the parent commit's)
        a = {"points": from_rgbd(aligned, aligned_frame, flt).count(), "uploaded_bytes_per_call": sum(d.nbytes + c.nbytes for d, c in aligned_frame),
             "call_pageable_ms": median_ms(lambda: from_rgbd(aligned, aligned_frame, flt)), "call_pinned_ms": median_ms(lambda: from_rgbd(aligned, pinned_aligned, flt))}
        with cw.cwipc_hip_profile() as prof:
            from_rgbd(aligned, pinned_aligned, flt)
        a["kernels_ms"] = {k: round(v[0], 4) for k, v in prof.kernels.items()}
        a["kernels_total_ms"] = round(sum(v[0] for v in prof.kernels.values()), 4)
        a["launches_per_call"] = int(sum(v[1] for v in prof.kernels.values()))
        r["aligned_entry_same_depth_size"] = a
        r["raw_over_aligned_pinned"] = round(r["call_pinned_ms"] / a["call_pinned_ms"], 3)
        # the numpy model on the same frames (its ray tables made beforehand, as the rig's are)
        tables = [lm.ray_table(w, h, fx, fy, cx, cy, DEPTH_LENS)] * 4
        r["numpy_model_ms"] = median_ms(lambda: lm.cloud(models, frame, model_flt, 2, 2, tables), reps=2, warm=0)
        rig.free()
        res[label] = r
        print(label, json.dumps(r), flush=True)
    parent = os.path.join(os.getcwd(), "profiles", "rgbd_timing.json")
    if os.path.exists(parent):
        with open(parent) as f:
            res["parent_commit_aligned_entry_4x640x480"] = json.load(f).get("4x640x480")
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(sys.argv[1]) or ".", exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
