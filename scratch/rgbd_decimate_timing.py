"""Per-frame time of the raw entry on decimated rigs (cwipc_hip_rgbd_rig_create_decimated) and with hole filling
(cwipc_hip_rgbd_rig_grab_filled), beside the plain grab and the `both` filter row of scratch/rgbd_depthfilter_timing.py as they are,
in the same run.

    python scratch/rgbd_decimate_timing.py [out.json]

Frames: those of scratch/rgbd_depthfilter_timing.py, made the same way from the same seed -- 4 x (640 x 576 depth, 1280 x 720 colour)
and 4 x (640 x 480 depth, 640 x 480 colour), RGB8, rational lenses on both sensors, a wavy wall with boxes in front of it, rectangular
holes, a noise of +-6 depth units.  Erosion 2 / 2, the depth-range and radius filters on, images in page-locked memory.  Per
decimation 1 (cwipc_hip_rgbd_rig_create), 2, 3 and 4: the plain grab and `both` (spatial magnitude 2 and temporal); on the undecimated
rig also every hole-fill mode alone.  Per variant: the whole call waited for (median of 10), the kernels from hipEvents
(cwipc_hip_profile) and the points that remain.  The upload is the same in every variant: the full-size images."""
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
from cwipc_util_amd.rgbd import RgbdDepthFilter, RgbdFilter, RgbdHoleFill, RgbdPrep, RgbdRig, RgbdSensor

sync = cw.util.cwipc_util_dll_load().cwipc_hip_synchronize
DEPTH_LENS = (4.9, 3.1, 1e-4, -5e-5, 0.16, 5.2, 4.8, 0.85)
COLOUR_LENS = (0.4569, -2.7217, 4.7e-4, -1.6e-4, 1.5964, 0.3335, -2.5460, 1.5223)
BOTH = RgbdDepthFilter(2, 0.5, 20.0, True, 0.4, 20.0, 3)


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


def noisy_smooth_depth(holed, k, noise):
    """A wavy wall at 2 - 3 m with a few nearer boxes in front of it, millimetres, plus the noise; the holes of `holed`."""
    height, width = holed.shape
    v, u = np.meshgrid(np.arange(height), np.arange(width), indexing='ij')
    depth = 2500 + 400 * np.sin(u / 90.0 + k) * np.cos(v / 70.0)
    for i in range(5):
        u0, v0 = (97 * (i + k) + 40) % (width - 160), (61 * (i + 2 * k) + 30) % (height - 200)
        depth[v0:v0 + 200, u0:u0 + 160] = 900 + 150 * i + 0.5 * (u[v0:v0 + 200, u0:u0 + 160] - u0)
    return np.where(holed != 0, depth + noise, 0).astype(np.uint16)


def measure(rig, grab):
    """points, the call waited for, the kernels"""
    rig.reset_history()
    o = {"points": grab().count(), "call_pinned_ms": median_ms(grab)}
    with cw.cwipc_hip_profile() as prof:
        grab()
    o["kernels_ms"] = {k: round(v[0], 4) for k, v in prof.kernels.items()}
    o["launches"] = {k: int(v[1]) for k, v in prof.kernels.items()}
    o["kernels_total_ms"] = round(sum(o["kernels_ms"].values()), 4)
    return o


def main():
    cw.cwipc_hip_set_device(0)
    rng = np.random.default_rng(1)
    noise_rng = np.random.default_rng(2)
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
            frame.append((noisy_smooth_depth(depth, k, noise_rng.integers(-6, 7, (h, w))), rng.integers(0, 256, (hc, wc, 3)).astype(np.uint8)))
            rng.integers(0, 256, (h, w, 3))   # (rgbd_raw_timing.py draws the aligned entry's colour image here: the same stream)
        keep = []
        pinned = [(pinned_copy(d, keep), pinned_copy(c, keep)) for d, c in frame]
        r = {"depth_pixels": 4 * w * h}
        for k in (1, 2, 3, 4):
            t0 = time.perf_counter()
            rig = RgbdRig(sensors, k)
            o = {"create_ms": round((time.perf_counter() - t0) * 1e3, 2), "grid": [rig.grid_sensors[0].width, rig.grid_sensors[0].height],
                 "plain": measure(rig, lambda: rig.grab(pinned, flt, prep)),
                 "both": measure(rig, lambda: rig.grab(pinned, flt, prep, depthfilter=BOTH))}
            if k == 1:
                for mode in (1, 2, 3):
                    o["holefill_%d" % mode] = measure(rig, lambda: rig.grab(pinned, flt, prep, holefill=RgbdHoleFill(mode)))
                base = o
            for name in [n for n in o if isinstance(o[n], dict)]:
                ref = base[name] if name in base else base["plain"]
                o[name]["call_over_decimation_1"] = round(o[name]["call_pinned_ms"] / ref["call_pinned_ms"], 3)
                o[name]["kernels_over_decimation_1"] = round(o[name]["kernels_total_ms"] / ref["kernels_total_ms"], 3)
            rig.free()
            r["decimation_%d" % k] = o
        rig = RgbdRig(sensors)
        base["plain"]["call_pinned_ms_afterwards"] = median_ms(lambda: rig.grab(pinned, flt, prep))
        rig.free()
        for mode in (1, 2, 3):
            o = base["holefill_%d" % mode]
            o["call_over_plain"] = round(o["call_pinned_ms"] / base["plain"]["call_pinned_ms"], 3)
            o["fill_kernels_ms"] = round(sum(v for n, v in o["kernels_ms"].items() if n.startswith("rgbd_holefill")), 4)
        r["both_decimation_2_over_both_decimation_1"] = {"call": r["decimation_2"]["both"]["call_over_decimation_1"],
                                                         "kernels": r["decimation_2"]["both"]["kernels_over_decimation_1"]}
        res[label] = r
        print(label, json.dumps(r), flush=True)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(sys.argv[1]) or ".", exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
