"""Per-frame time of the raw entry with the depth post-processing (cwipc_hip_rgbd_rig_grab_filtered): spatial magnitude 2 alone, temporal
alone, and both, beside cwipc_hip_rgbd_rig_grab on the same frames in the same run.

    python scratch/rgbd_depthfilter_timing.py [out.json]

Frames: those of scratch/rgbd_occlusion_timing.py's smooth variant, made the same way from the same seed -- 4 x (640 x 576 depth,
1280 x 720 colour) and 4 x (640 x 480 depth, 640 x 480 colour), RGB8, rational lenses on both sensors, a wavy wall with boxes in front
of it and rectangular holes -- with a noise of +-6 depth units per pixel on top, which is what the filters are there for (delta 20:
the noise blends, the steps between the surfaces do not).  Erosion 2 / 2, the depth-range and radius filters on, images in
page-locked memory.  Per variant: the whole call waited for (median of 10; three such medians for the plain grab), the kernels from
hipEvents (cwipc_hip_profile) and the points that remain.  The host alternative: the numpy model's stages (tests/
rgbd_depthfilter_model.py, which runs all lines of an image at once, position by position) on the same frames, once."""
import json
import os
import sys
import time

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import numpy as np
import torch  # noqa: F401  (first: it brings the HIP runtime the library then shares)
import cwipc_util_amd as cw
import rgbd_depthfilter_model as dm
import rgbd_model as rm
from cwipc_util_amd.rgbd import RgbdDepthFilter, RgbdFilter, RgbdPrep, RgbdRig, RgbdSensor

sync = cw.util.cwipc_util_dll_load().cwipc_hip_synchronize
DEPTH_LENS = (4.9, 3.1, 1e-4, -5e-5, 0.16, 5.2, 4.8, 0.85)
COLOUR_LENS = (0.4569, -2.7217, 4.7e-4, -1.6e-4, 1.5964, 0.3335, -2.5460, 1.5223)
VARIANTS = {"spatial_2": RgbdDepthFilter(2, 0.5, 20.0, False), "temporal": RgbdDepthFilter(0, 0.5, 20.0, True, 0.4, 20.0, 3),
            "spatial_2_temporal": RgbdDepthFilter(2, 0.5, 20.0, True, 0.4, 20.0, 3)}


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


def profile(fn):
    with cw.cwipc_hip_profile() as prof:
        fn()
    kernels = {k: round(v[0], 4) for k, v in prof.kernels.items()}
    launches = {k: int(v[1]) for k, v in prof.kernels.items()}
    return kernels, launches, round(sum(kernels.values()), 4)


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
        rig = RgbdRig(sensors)
        plain = {"points": rig.grab(pinned, flt, prep).count(),
                 "call_pinned_ms_three_medians": [median_ms(lambda: rig.grab(pinned, flt, prep)) for _ in range(3)]}
        plain["call_pinned_ms"] = float(np.median(plain["call_pinned_ms_three_medians"]))
        plain["kernels_ms"], _launches, plain["kernels_total_ms"] = profile(lambda: rig.grab(pinned, flt, prep))
        r = {"depth_pixels": 4 * w * h, "rows": 4 * h, "columns": 4 * w, "state_bytes": 4 * w * h * 9, "rig_grab": plain}
        for name, df in VARIANTS.items():
            rig.reset_history()
            o = {"points": rig.grab(pinned, flt, prep, depthfilter=df).count(),
                 "call_pinned_ms": median_ms(lambda: rig.grab(pinned, flt, prep, depthfilter=df))}
            o["kernels_ms"], o["launches"], o["kernels_total_ms"] = profile(lambda: rig.grab(pinned, flt, prep, depthfilter=df))
            added = [k for k in o["kernels_ms"] if k.startswith(("rgbd_spatial", "rgbd_temporal", "rgbd_history"))]
            o["filter_kernels_ms"] = round(sum(o["kernels_ms"][k] for k in added), 4)
            o["kernels_over_rig_grab"] = round(o["kernels_total_ms"] / plain["kernels_total_ms"], 3)
            o["call_over_rig_grab"] = round(o["call_pinned_ms"] / plain["call_pinned_ms"], 3)
            r[name] = o
        plain["call_pinned_ms_afterwards"] = median_ms(lambda: rig.grab(pinned, flt, prep))
        rig.free()
        # the host alternative: the model's stages on the same depth images
        t0 = time.perf_counter()
        smoothed = [dm.spatial(d, 2, 0.5, 20.0) for d, _c in frame]
        t1 = time.perf_counter()
        hists = [dm.History(h, w) for _ in frame]
        for hist, d in zip(hists, smoothed):
            hist.temporal(d, 0.4, 20.0, 3)
        t2 = time.perf_counter()
        r["numpy_model_ms"] = {"spatial_2": round((t1 - t0) * 1e3, 2), "temporal": round((t2 - t1) * 1e3, 2)}
        r["numpy_spatial_2_over_filter_kernels"] = round(r["numpy_model_ms"]["spatial_2"] / r["spatial_2"]["filter_kernels_ms"], 1)
        res[label] = r
        print(label, json.dumps(r), flush=True)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(sys.argv[1]) or ".", exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
