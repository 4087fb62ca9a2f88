"""Time and distortion of level-of-detail decoding (cwipc_util_amd.codec.cwipc_new_decoder(max_octree_bits=t); RULE L) beside the
full decode of the same packet, same run.

    python scratch/codec_lod_timing.py CASE OUT_DIR        one cloud, its record to OUT_DIR/CASE.json
    python scratch/codec_lod_timing.py --merge OUT_DIR OUT.json

One process per cloud, so that each can run under a time limit of its own and a step that fails ends the chain:

    for c in synthetic_300k synthetic_2m; do
        timeout -k 10 240 python scratch/codec_lod_timing.py $c out || exit 1
    done && python scratch/codec_lod_timing.py --merge out profiles/codec_lod_timing.json

Clouds: the synthetic source at 300 k points (9 bits) and 2 M points (10 bits).  Per cloud and per form ("cwae", "cwat" at quality 85):
  decode      for t = b (the full decode: the limit changes nothing), b - 1, b - 2, b - 4: settled call, the feed() call alone, a
              stream of calls (codec_entropy_timing.py's measures), the kernels of one call from hipEvents in a call of their own with
              their launches, the points handed out; `over_full`: the settled median over that of t = b in this run
  lod_kernels the kernels of kernels_lod.hip alone, [ms, launches]
  quality     "coded at b, decoded at t" beside "coded at t" (quality.codec_distortion, plane=False): bytes, Y-PSNR and D1-PSNR
No target was set in advance; the file records what was measured and how many steps."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "scratch"))
import torch  # noqa: F401  (first: it brings the HIP runtime the library then shares)
import cwipc_util_amd as cw
import cwipc_util_amd.codec as codec
from cwipc_util_amd import quality
from cwipc_util_amd.capture import _synthetic_cloud
from codec_entropy_timing import WARMUP, STEPS, profile, settled_ms, stream_ms

QUALITY = 85
CASES = {"synthetic_300k": (300_000, 9), "synthetic_2m": (2_000_000, 10)}
FORMS = {"cwae": dict(entropy=True), "cwat": dict(colour_transform=True)}


def decoder_record(packet, t):
    dec = codec.cwipc_new_decoder(max_octree_bits=t)
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

    r = {"decode_bits": t, "settled_call": settled_ms(once)}
    r["feed_call_median_ms"] = round(float(np.median(feeds[WARMUP:])) * 1e3, 4)
    r["stream_call_ms"] = stream_ms(lambda: dec.feed(packet), take)
    r.update(profile(once))
    r["points_out"] = clouds[0].count()
    r["lod_kernels"] = {k: [v, r["launches"][k]] for k, v in r["kernels_ms"].items() if k.startswith("lod_")}
    dec.free()
    return r


def quality_rows(pc, bits, form):
    rows = []
    for t in (bits, bits - 1, bits - 2, bits - 4):
        cut, nbytes = quality.codec_distortion(pc, octree_bits=bits, jpeg_quality=QUALITY, plane=False, decode_bits=t, **FORMS[form])
        native, native_bytes = quality.codec_distortion(pc, octree_bits=t, jpeg_quality=QUALITY, plane=False, **FORMS[form])
        rows.append({"t": t, "coded_at_b_decoded_at_t": {"bytes": nbytes, "psnr_y": round(cut.psnr_y, 3), "psnr_d1": round(cut.psnr_d1, 3)},
                     "coded_at_t": {"bytes": native_bytes, "psnr_y": round(native.psnr_y, 3), "psnr_d1": round(native.psnr_d1, 3)}})
    return rows


def run_case(name, out_dir):
    cw.cwipc_hip_set_device(0)
    npoints, bits = CASES[name]
    pc = _synthetic_cloud(npoints, 0.0)
    r = {"points": pc.count(), "octree_bits": bits, "jpeg_quality": QUALITY, "warmup": WARMUP, "steps": STEPS, "forms": {}}
    for form, kw in FORMS.items():
        enc = codec.cwipc_new_encoder(octree_bits=bits, jpeg_quality=QUALITY, **kw)
        enc.feed(pc)
        assert enc.available(True)
        packet = bytes(enc.get_bytes())
        enc.free()
        rows = [decoder_record(packet, t) for t in (bits, bits - 1, bits - 2, bits - 4)]
        for row in rows:
            row["over_full"] = round(row["settled_call"]["median_ms"] / rows[0]["settled_call"]["median_ms"], 3)
        r["forms"][form] = {"packet_bytes": len(packet), "decode": rows, "quality": quality_rows(pc, bits, form)}
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
