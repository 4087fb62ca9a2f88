"""Per-frame time of the raw entry with the occlusion test (cwipc_hip_rgbd_rig_grab_occluded) at splat 0, 1 and 2 beside
cwipc_hip_rgbd_rig_grab on the same frames in the same run.

    python scratch/rgbd_occlusion_timing.py [out.json]

Frames: those of scratch/rgbd_raw_timing.py, made the same way from the same seed -- 4 x (640 x 576 depth, 1280 x 720 colour) and
4 x (640 x 480 depth, 640 x 480 colour), RGB8, rational lenses on both sensors, the colour sensor 32 mm to the side, depth drawn
uniformly per pixel with rectangular holes, erosion 2 / 2, the depth-range and radius filters on, images in page-locked memory.  A
per-pixel random depth is the hardest case for the z-buffer (every neighbour is a different depth) and not what a camera sees, so each
size is run a second time with a smooth depth image (a few surfaces, steps between them, the same holes).  Per variant: the whole call
waited for (median of 10, and the spread of three such medians for the plain grab), the kernels from hipEvents (cwipc_hip_profile;
rgbd_zfill is the z-buffer's memset) and the points that remain.  margin is 0.02 m throughout."""
import json
import os
import sys
import time

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import numpy as np
import torch  # noqa: F401  (first: it brings the HIP runtime the library then shares)
import cwipc_util_amd as cw
import rgbd_model as rm
from cwipc_util_amd.rgbd import RgbdFilter, RgbdOcclusion, RgbdPrep, RgbdRig, RgbdSensor

sync = cw.util.cwipc_util_dll_load().cwipc_hip_synchronize
DEPTH_LENS = (4.9, 3.1, 1e-4, -5e-5, 0.16, 5.2, 4.8, 0.85)
COLOUR_LENS = (0.4569, -2.7217, 4.7e-4, -1.6e-4, 1.5964, 0.3335, -2.5460, 1.5223)
MARGIN = 0.02


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


def smooth_depth(holed, k):
    """A wavy wall at 2 - 3 m with a few nearer boxes in front of it, millimetres; the holes of `holed`."""
    height, width = holed.shape
    v, u = np.meshgrid(np.arange(height), np.arange(width), indexing='ij')
    depth = 2500 + 400 * np.sin(u / 90.0 + k) * np.cos(v / 70.0)
    for i in range(5):
        u0, v0 = (97 * (i + k) + 40) % (width - 160), (61 * (i + 2 * k) + 30) % (height - 200)
        depth[v0:v0 + 200, u0:u0 + 160] = 900 + 150 * i + 0.5 * (u[v0:v0 + 200, u0:u0 + 160] - u0)
    return np.where(holed != 0, depth, 0).astype(np.uint16)


def profile(fn):
    with cw.cwipc_hip_profile() as prof:
        fn()
    kernels = {k: round(v[0], 4) for k, v in prof.kernels.items()}
    return kernels, round(sum(kernels.values()), 4)


def main():
    cw.cwipc_hip_set_device(0)
    rng = np.random.default_rng(1)
    flt = RgbdFilter(0.4, 3.5, radius=3.0)
    prep = RgbdPrep(2, 2)
    d2c = np.identity(4)
    d2c[0, 3] = -0.032
    res = {}
    for label, (w, h), (wc, hc) in (("4x640x576+1280x720", (640, 576), (1280, 720)), ("4x640x480+640x480", (640, 480), (640, 480))):
        fx, fy, cx, cy = 504.0 * w / 640, 504.0 * h / 576, 320.0 * w / 640, 330.0 * h / 576
        cfx, cfy, ccx, ccy = 607.0 * wc / 1280, 607.0 * hc / 720, 638.0 * wc / 1280, 367.0 * hc / 720
        sensors, frame = [], []
        for k in range(4):
            m = rm.random_rigid(rng, 1.0)
            sensors.append(RgbdSensor(w, h, fx, fy, cx, cy, wc, hc, cfx, cfy, ccx, ccy, DEPTH_LENS, COLOUR_LENS, d2c, 0.001, m, 1 << k, "cam%d" % k))
            depth = holed_depth(rng, w, h)
            frame.append((depth, rng.integers(0, 256, (hc, wc, 3)).astype(np.uint8)))
            rng.integers(0, 256, (h, w, 3))   # (rgbd_raw_timing.py draws the aligned entry's colour image here: the same stream)
        keep = []
        frames = {"random_depth": [(pinned_copy(d, keep), pinned_copy(c, keep)) for d, c in frame],
                  "smooth_depth": [(pinned_copy(smooth_depth(d, k), keep), pinned_copy(c, keep)) for k, (d, c) in enumerate(frame)]}
        rig = RgbdRig(sensors)
        r = {"depth_pixels": 4 * w * h, "colour_pixels": 4 * wc * hc, "zbuffer_bytes": 4 * wc * hc * 8,
             "rule_of_thumb_splat_at_least": int(np.ceil(max(cfx / fx, cfy / fy))) - 1}
        for name, pinned in frames.items():
            plain = {"points": rig.grab(pinned, flt, prep).count(),
                     "call_pinned_ms_three_medians": [median_ms(lambda: rig.grab(pinned, flt, prep)) for _ in range(3)]}
            plain["call_pinned_ms"] = float(np.median(plain["call_pinned_ms_three_medians"]))
            plain["kernels_ms"], plain["kernels_total_ms"] = profile(lambda: rig.grab(pinned, flt, prep))
            s = {"rig_grab": plain}
            for splat in (0, 1, 2):
                occ = RgbdOcclusion(splat, MARGIN)
                o = {"points": rig.grab(pinned, flt, prep, occlusion=occ).count(),
                     "call_pinned_ms": median_ms(lambda: rig.grab(pinned, flt, prep, occlusion=occ))}
                o["kernels_ms"], o["kernels_total_ms"] = profile(lambda: rig.grab(pinned, flt, prep, occlusion=occ))
                o["kernels_over_rig_grab"] = round(o["kernels_total_ms"] / plain["kernels_total_ms"], 3)
                o["call_over_rig_grab"] = round(o["call_pinned_ms"] / plain["call_pinned_ms"], 3)
                s["occluded_splat_%d" % splat] = o
            # the plain grab once more, behind the occluded ones on a rig that has its z-buffer by now
            plain["call_pinned_ms_afterwards"] = median_ms(lambda: rig.grab(pinned, flt, prep))
            r[name] = s
        rig.free()
        res[label] = r
        print(label, json.dumps(r), flush=True)
    parent = os.path.join(os.getcwd(), "profiles", "rgbd_raw_timing.json")
    if os.path.exists(parent):
        with open(parent) as f:
            raw = json.load(f)
        res["parent_commit_rig_grab"] = {k: {"call_pinned_ms": v["call_pinned_ms"], "call_pageable_ms": v["call_pageable_ms"], "kernels_ms": v["kernels_ms"],
                                             "kernels_total_ms": v["kernels_total_ms"], "points": v["points"]}
                                         for k, v in raw.items() if isinstance(v, dict) and "call_pinned_ms" in v}
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(sys.argv[1]) or ".", exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
