"""One side of the A/B of the RGB-D source's host driver: the library comes from CWIPC_LIBRARY_DIR (unset: this tree's).

    python scratch/rgbd_ab.py OUT.json               one process: both frame sizes, every workload
    python scratch/rgbd_ab.py --table DIR OUT.txt    the rows of profiles/rgbd_split_ab.txt from DIR/{parent,this}_I.json

Frames and per-call method are those of scratch/rgbd_raw_timing.py and rgbd_decimate_timing.py: 4 x (640 x 576 depth, 1280 x 720
colour) and 4 x (640 x 480, 640 x 480), RGB8, rational lenses, a noisy wavy wall with boxes and rectangular holes, erosion 2 / 2, the
depth-range and radius filters on, every image in page-locked memory; settled = the median of STEPS waited-for calls after WARMUP;
launches = the kernels of one profiled call.  Workloads: cwipc_hip_from_rgbd (depth-sized colour images), the plain grab, the occluded
grab (splat 1), the filtered grab (spatial magnitude 2 and temporal), the filled grab (mode 2) on a rig of decimation 2.  sha256 of
every workload's cloud -- the first call on a rig whose history has been reset -- and of the history the filtered grab leaves."""
import hashlib
import json
import os
import sys
import time

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "scratch"))
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import numpy as np

WARMUP, STEPS = 3, 10
CASES = (("4x640x576+1280x720", (640, 576), (1280, 720)), ("4x640x480+640x480", (640, 480), (640, 480)))


def run(out):
    import torch  # noqa: F401  (first: it brings the HIP runtime the library then shares)
    import cwipc_util_amd as cw
    import rgbd_model as rm
    from cwipc_util_amd.rgbd import RgbdCamera, RgbdFilter, RgbdHoleFill, RgbdOcclusion, RgbdPrep, RgbdRig, RgbdSensor, from_rgbd
    from rgbd_decimate_timing import BOTH, COLOUR_LENS, DEPTH_LENS, holed_depth, noisy_smooth_depth, pinned_copy

    sync = cw.util.cwipc_util_dll_load().cwipc_hip_synchronize

    def sha(data):
        return hashlib.sha256(data).hexdigest()[:16]

    def settled_ms(fn):
        for _ in range(WARMUP):
            fn()
        t = []
        for _ in range(STEPS):
            t0 = time.perf_counter(); fn(); sync(); t.append(time.perf_counter() - t0)
        return round(float(np.median(t)) * 1e3, 4)

    cw.cwipc_hip_set_device(0)
    rng, noise_rng = np.random.default_rng(1), np.random.default_rng(2)
    flt, prep = RgbdFilter(0.4, 3.5, radius=3.0), RgbdPrep(2, 2)
    d2c = np.identity(4)
    d2c[0, 3] = -0.032
    res = {"lib": cw.util.cwipc_util_dll_load()._name, "warmup": WARMUP, "steps": STEPS, "rows": {}, "sha256": {}}
    for label, (w, h), (wc, hc) in CASES:
        fx, fy, cx, cy = 504.0 * w / 640, 504.0 * h / 576, 320.0 * w / 640, 330.0 * h / 576
        cfx, cfy, ccx, ccy = 607.0 * wc / 1280, 607.0 * hc / 720, 638.0 * wc / 1280, 367.0 * hc / 720
        sensors, aligned, frame, aligned_frame, keep = [], [], [], [], []
        for k in range(4):
            m = rm.random_rigid(rng, 1.0)
            sensors.append(RgbdSensor(w, h, fx, fy, cx, cy, wc, hc, cfx, cfy, ccx, ccy, DEPTH_LENS, COLOUR_LENS, d2c, 0.001, m, 1 << k, "cam%d" % k))
            aligned.append(RgbdCamera(w, h, fx, fy, cx, cy, 0.001, m, 1 << k, "cam%d" % k))
            depth = pinned_copy(noisy_smooth_depth(holed_depth(rng, w, h), k, noise_rng.integers(-6, 7, (h, w))), keep)
            frame.append((depth, pinned_copy(rng.integers(0, 256, (hc, wc, 3)).astype(np.uint8), keep)))
            aligned_frame.append((depth, pinned_copy(rng.integers(0, 256, (h, w, 3)).astype(np.uint8), keep)))

        def record(name, call, rig=None):
            if rig is not None:
                rig.reset_history()
            pc = call()
            res["sha256"]["%s.%s.cloud" % (label, name)] = sha(np.ascontiguousarray(pc.get_numpy_array()).tobytes())
            if name == "filtered":
                for i in range(4):
                    value, history = rig.history(i)
                    res["sha256"]["%s.%s.history%d" % (label, name, i)] = sha(np.ascontiguousarray(value).tobytes() + np.ascontiguousarray(history).tobytes())
            r = {"points": pc.count(), "settled_ms": settled_ms(call)}
            with cw.cwipc_hip_profile() as prof:
                call()
            r["launches"] = {k: int(v[1]) for k, v in prof.kernels.items()}
            res["rows"]["%s.%s" % (label, name)] = r
            print(label, name, json.dumps(r), flush=True)

        record("from_rgbd", lambda: from_rgbd(aligned, aligned_frame, flt))
        with RgbdRig(sensors) as rig:
            record("plain", lambda: rig.grab(frame, flt, prep), rig)
            record("occluded", lambda: rig.grab(frame, flt, prep, occlusion=RgbdOcclusion(1, 0.02)), rig)
            record("filtered", lambda: rig.grab(frame, flt, prep, depthfilter=BOTH), rig)
        with RgbdRig(sensors, 2) as rig:
            record("filled_decimation_2", lambda: rig.grab(frame, flt, prep, holefill=RgbdHoleFill(2)), rig)
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


def table(directory, out):
    runs = {side: [] for side in ("parent", "this")}
    for side in runs:
        i = 0
        while os.path.exists(os.path.join(directory, "%s_%d.json" % (side, i))):
            with open(os.path.join(directory, "%s_%d.json" % (side, i))) as f:
                runs[side].append(json.load(f))
            i += 1
    hashes = {json.dumps(r["sha256"], sort_keys=True) for side in runs for r in runs[side]}
    lines = ["%d + %d processes; %d sha256 per process, %s" % (len(runs["parent"]), len(runs["this"]), len(runs["this"][0]["sha256"]),
                                                                "identical in every process of both libraries" if len(hashes) == 1 else "DIFFERENT"),
             "%-46s %9s %9s %9s | %-29s %s" % ("measure", "par.min", "par.med", "par.max", "this, process by process", "verdict")]
    for label in runs["this"][0]["rows"]:
        launches = {json.dumps(r["rows"][label]["launches"], sort_keys=True) for side in runs for r in runs[side]}
        lines.append("%-46s launches %s: %s" % (label, "equal" if len(launches) == 1 else "DIFFERENT", json.dumps(runs["this"][0]["rows"][label]["launches"], sort_keys=True)))
        par = sorted(r["rows"][label]["settled_ms"] for r in runs["parent"])
        this = [r["rows"][label]["settled_ms"] for r in runs["this"]]
        spread = par[-1] - par[0]
        inside = all(par[0] - spread <= t <= par[-1] + spread for t in this)
        verdict = "within" if inside else "OUTSIDE (median %+.1f %% of the parent's)" % (100 * (float(np.median(this)) / float(np.median(par)) - 1))
        lines.append("%-46s %9.4f %9.4f %9.4f | %-29s %s" % (label + ".settled_ms", par[0], float(np.median(par)), par[-1], " ".join("%.4f" % t for t in this), verdict))
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    if sys.argv[1] == "--table":
        table(sys.argv[2], sys.argv[3])
    else:
        run(sys.argv[1])
