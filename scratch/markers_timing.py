"""Per-call time of the marker detector on a 1920 x 1080 view of a board with two markers (321 k points, point size 5), device-resident.

    python scratch/markers_timing.py DICTIONARY.json [out.json]

DICTIONARY.json: the marker payloads (a list of 5 x 5 lists of 0/1 in id order; the test suite's fixture serves).  The cloud is a
white board in the plane y = 0, 1.6 m x 0.8 m, sampled every 2 mm, with markers 0 and 1 of the dictionary painted in, 17.4 cm wide;
the camera looks down at it from 1.45 m.  Three cases, per case the median wall time of 20 calls after 3 warm-up calls and the kernels'
own time from hipEvents (cwipc_hip_profile, a run of its own):
  detect            cwipc_hip_detect_markers on the rendered image, a host array (the image goes up, the corners come back)
  render_detect     cwipc_hip_render_detect_markers (no image leaves the GPU)
  render_then_detect  cwipc_hip_render to host arrays followed by cwipc_hip_detect_markers on them"""
import json
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import numpy as np
import torch  # noqa: F401
import cwipc_util_amd as cw
from cwipc_util_amd.registration import MarkerDictionary, default_view, look_at

sync = cw.util.cwipc_util_dll_load().cwipc_hip_synchronize


def timed(fn, reps=20):
    for _ in range(3):
        fn()
    sync()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); sync(); t.append(time.perf_counter() - t0)
    out = {"call_ms_median": round(float(np.median(t)) * 1e3, 4), "call_ms_min": round(float(np.min(t)) * 1e3, 4),
           "call_ms_max": round(float(np.max(t)) * 1e3, 4)}
    with cw.cwipc_hip_profile() as prof:
        fn()
    out["kernels_ms"] = {k: round(v[0], 4) for k, v in prof.kernels.items()}
    out["kernels_ms_sum"] = round(sum(v[0] for v in prof.kernels.values()), 4)
    return out


def make_board(bits, spacing=0.002, half=0.087, seed=1):
    x, z = np.meshgrid(np.arange(-0.35, 1.25 + spacing / 2, spacing), np.arange(-0.4, 0.4 + spacing / 2, spacing), indexing='ij')
    x, z = x.reshape(-1), z.reshape(-1)
    shade = np.full(len(x), 255, dtype=np.uint8)
    for m, offset in ((0, 0.0), (1, 0.9)):
        cells = np.zeros((7, 7), dtype=np.uint8)
        cells[1:6, 1:6] = bits[m]
        u, v = 7.0 * (half - (x - offset)) / (2 * half), 7.0 * (half - z) / (2 * half)
        inside = (u >= 0) & (u < 7) & (v >= 0) & (v < 7)
        shade[inside & (cells[np.clip(v.astype(np.int64), 0, 6), np.clip(u.astype(np.int64), 0, 6)] == 0)] = 0
    order = np.random.default_rng(seed).permutation(len(x))
    pts = np.zeros(len(x), dtype=cw.cwipc_point_numpy_dtype)
    pts['x'], pts['z'] = x[order], z[order]
    pts['r'] = pts['g'] = pts['b'] = shade[order]
    pts['tile'] = 1
    pc = cw.cwipc_from_numpy_array(pts, 0)
    cw.cwipc_hip_upload(pc, drop_host_copy=True)
    return pc


def main():
    with open(sys.argv[1]) as f:
        bits = np.asarray(json.load(f), dtype=np.uint8)
    words = MarkerDictionary.from_bits(bits).words
    pc = make_board(bits)
    view = default_view(extrinsic=look_at((0.40, 1.45, -0.10), (0.45, 0.0, 0.02), (1.0, 0.0, 0.1))).as_struct()
    rgb, _depth, _index = cw.cwipc_hip_render(pc, view, 5)
    ids, corners, found = cw.cwipc_hip_detect_markers(rgb, words)
    res = {"image": [view.width, view.height], "points": pc.count(), "found": ids.tolist(), "corners": corners.tolist()}
    assert found == 2, found

    def render_then_detect():
        img = cw.cwipc_hip_render(pc, view, 5)[0]
        return cw.cwipc_hip_detect_markers(img, words)

    res["detect"] = timed(lambda: cw.cwipc_hip_detect_markers(rgb, words))
    res["render_detect"] = timed(lambda: cw.cwipc_hip_render_detect_markers(pc, view, words, 5))
    res["render_then_detect"] = timed(render_then_detect)
    both = cw.cwipc_hip_render_detect_markers(pc, view, words, 5)
    assert both[0].tolist() == ids.tolist() and np.array_equal(both[1], corners)
    print(json.dumps(res), flush=True)
    if len(sys.argv) > 2:
        os.makedirs(os.path.dirname(sys.argv[2]) or ".", exist_ok=True)
        with open(sys.argv[2], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
