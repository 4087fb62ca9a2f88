"""Time and size of the entropy-coded packet form (cwipc_util_amd.codec with entropy=True; RULE E) beside the plain form, same run.

    python scratch/codec_entropy_timing.py CASE OUT_DIR        one cloud, its record to OUT_DIR/CASE.json
    python scratch/codec_entropy_timing.py --merge OUT_DIR OUT.json

One process per cloud, so that each can run under a time limit of its own and a step that fails ends the chain:

    for c in synthetic_300k synthetic_2m synthetic_10m structured_2m; do
        timeout -k 10 240 python scratch/codec_entropy_timing.py $c out || exit 1
    done && python scratch/codec_entropy_timing.py --merge out profiles/codec_entropy_timing.json

Clouds: the three of codec_timing.py (the synthetic source at 300 k, 2 M and 10 M points with octree_bits 9 / 10 / 12: random-looking
colours, most points in a cell of their own) and a structured one (2 M points on a sphere's surface, a smooth colour, two tiles by
hemisphere, 10 bits: what a camera rig gives).  jpeg_quality 85.  Per cloud, for the plain and the entropy encoder:
  encode      single settled calls (feed, wait, take the bytes; median of STEPS after WARMUP) and a stream of calls (STEPS feeds back
              to back, then the STEPS packets; total / STEPS); the kernels of one call from hipEvents, in a call of their own
  packet      bytes and bytes per leaf in both forms; per stream kind how many streams are coded and their raw and coded bytes
  decode      settled calls and a stream of calls for both forms, the kernels, and the time of the feed() call alone: the entropy
              decoder waits once inside feed for the check, the plain one returns with everything in flight
No target was set in advance; the file records what was measured and how many steps."""
import json
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import numpy as np
import torch  # noqa: F401  (first: it brings the HIP runtime the library then shares)
import cwipc_util_amd as cw
import cwipc_util_amd.codec as codec
from cwipc_util_amd.capture import _synthetic_cloud

sync = cw.util.cwipc_util_dll_load().cwipc_hip_synchronize
WARMUP, STEPS = 3, 10
QUALITY = 85
CASES = {"synthetic_300k": (300_000, 9), "synthetic_2m": (2_000_000, 10), "synthetic_10m": (10_000_000, 12), "structured_2m": (2_000_000, 10)}


def structured_cloud(n):
    rng = np.random.default_rng(0)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    pts = np.zeros(n, dtype=[('x', '<f4'), ('y', '<f4'), ('z', '<f4'), ('r', 'u1'), ('g', 'u1'), ('b', 'u1'), ('tile', 'u1')])
    pts['x'], pts['y'], pts['z'] = d[:, 0], d[:, 1], d[:, 2]
    pts['r'] = np.clip(128 + 100 * d[:, 0], 0, 255)
    pts['g'] = np.clip(128 + 100 * d[:, 1], 0, 255)
    pts['b'] = np.clip(128 + 100 * np.sin(3 * d[:, 2]), 0, 255)
    pts['tile'] = np.where(d[:, 0] < 0, 1, 2)
    host = cw.cwipc_from_numpy_array(pts, 0)
    return cw.cwipc_tilefilter(host, 0)        # device-resident, like the synthetic ones


def settled_ms(fn):
    for _ in range(WARMUP):
        fn()
    sync()
    t = []
    for _ in range(STEPS):
        t0 = time.perf_counter(); fn(); sync(); t.append(time.perf_counter() - t0)
    return {"median_ms": round(float(np.median(t)) * 1e3, 4), "min_ms": round(min(t) * 1e3, 4), "max_ms": round(max(t) * 1e3, 4)}


def stream_ms(feed, take):
    for _ in range(WARMUP):
        feed()
    for _ in range(WARMUP):
        take()
    sync()
    t0 = time.perf_counter()
    for _ in range(STEPS):
        feed()
    for _ in range(STEPS):
        take()
    sync()
    return round((time.perf_counter() - t0) / STEPS * 1e3, 4)


def profile(fn):
    with cw.cwipc_hip_profile() as prof:
        fn()
    kernels = {k: round(v[0], 4) for k, v in prof.kernels.items()}
    return {"kernels_ms": kernels, "launches": {k: int(v[1]) for k, v in prof.kernels.items()}, "kernels_total_ms": round(sum(kernels.values()), 4)}


def encoder_record(pc, bits, entropy):
    enc = codec.cwipc_new_encoder(octree_bits=bits, jpeg_quality=QUALITY, entropy=entropy)
    packets = []

    def once():
        enc.feed(pc)
        assert enc.available(True)
        packets[:] = [enc.get_bytes()]

    def take():
        assert enc.available(True)
        packets[:] = [enc.get_bytes()]

    r = {"settled_call": settled_ms(once), "stream_call_ms": stream_ms(lambda: enc.feed(pc), take)}
    r.update(profile(once))
    return r, bytes(packets[0])


def decoder_record(packet, leaves):
    dec = codec.cwipc_new_decoder()
    clouds, feeds = [], []

    def once():
        t0 = time.perf_counter()
        dec.feed(packet)
        feeds.append(time.perf_counter() - t0)
        assert dec.available(True)
        clouds[:] = [dec.get()]

    def take():
        assert dec.available(True)
        clouds[:] = [dec.get()]

    r = {"settled_call": settled_ms(once)}
    r["feed_call_median_ms"] = round(float(np.median(feeds[WARMUP:])) * 1e3, 4)
    r["stream_call_ms"] = stream_ms(lambda: dec.feed(packet), take)
    r.update(profile(once))
    assert clouds[0].count() == leaves
    return r


def run_case(name, out_dir):
    cw.cwipc_hip_set_device(0)
    npoints, bits = CASES[name]
    pc = structured_cloud(npoints) if name.startswith("structured") else _synthetic_cloud(npoints, 0.0)
    r = {"points": pc.count(), "octree_bits": bits, "jpeg_quality": QUALITY, "warmup": WARMUP, "steps": STEPS}
    r["encode_plain"], plain = encoder_record(pc, bits, False)
    r["encode_entropy"], coded = encoder_record(pc, bits, True)
    assert bytes(codec.entropy_unpack(coded)) == plain
    info = codec.entropy_info(coded)
    leaves = info["nleaves"]
    kinds = {}
    for (kind, _, symbols), (mode, size) in zip(info["kinds"], info["streams"]):
        k = kinds.setdefault(kind, {"streams": 0, "coded": 0, "symbols": 0, "payload_bytes": 0})
        k["streams"] += 1
        k["coded"] += mode
        k["symbols"] += symbols
        k["payload_bytes"] += size
    r["packet"] = {"leaves": leaves, "plain_bytes": len(plain), "entropy_bytes": len(coded), "entropy_over_plain": round(len(coded) / len(plain), 4),
                   "plain_bytes_per_leaf": round(len(plain) / max(1, leaves), 4), "entropy_bytes_per_leaf": round(len(coded) / max(1, leaves), 4),
                   "streams": kinds}
    e, p = r["encode_entropy"], r["encode_plain"]
    r["encode_entropy_over_plain"] = {"settled": round(e["settled_call"]["median_ms"] / p["settled_call"]["median_ms"], 3),
                                      "stream": round(e["stream_call_ms"] / p["stream_call_ms"], 3)}
    r["decode_plain"] = decoder_record(plain, leaves)
    r["decode_entropy"] = decoder_record(coded, leaves)
    e, p = r["decode_entropy"], r["decode_plain"]
    r["decode_entropy_over_plain"] = {"settled": round(e["settled_call"]["median_ms"] / p["settled_call"]["median_ms"], 3),
                                      "stream": round(e["stream_call_ms"] / p["stream_call_ms"], 3)}
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, name + ".json"), "w") as f:
        json.dump(r, f, indent=1)
    print(name, json.dumps(r), flush=True)


def merge(out_dir, out):
    res = {"clouds": {}}
    for name in CASES:
        path = os.path.join(out_dir, name + ".json")
        if os.path.exists(path):
            with open(path) as f:
                res["clouds"][name] = json.load(f)
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    if sys.argv[1] == "--merge":
        merge(sys.argv[2], sys.argv[3])
    else:
        run_case(sys.argv[1], sys.argv[2])
