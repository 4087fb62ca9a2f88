"""Time, size and distortion of transform colour coding (cwipc_util_amd.codec with colour_transform=True; RULE T) beside the
entropy-coded form (RULE E), same run.

    python scratch/codec_transform_timing.py CASE OUT_DIR        one cloud, its record to OUT_DIR/CASE.json
    python scratch/codec_transform_timing.py --merge OUT_DIR OUT.json

One process per cloud, so that each can run under a time limit of its own and a step that fails ends the chain:

    for c in sphere_400k synthetic_300k synthetic_2m; do
        timeout -k 10 240 python scratch/codec_transform_timing.py $c out || exit 1
    done && python scratch/codec_transform_timing.py --merge out profiles/codec_transform_timing.json

Clouds: the sphere of tests/transform_model.sphere_cloud (400 k points, 9 bits, a smooth colour field plus noise of sigma 3) and the
synthetic source at 300 k and 2 M points (9 and 10 bits: random-looking colours, most points in a cell of their own).  Per cloud:
  table       for jpeg_quality 100, 85, 50, 24, 10 and both forms: packet bytes, colour payload bytes (with their directory entries)
              per leaf, the symmetric Y-PSNR and RGB mse of quality.codec_distortion (plane=False).  The losing rows included.
  encode      at quality 24, for "cwae" and "cwat": single settled calls and a stream of calls (codec_entropy_timing.py's measures), the
              kernels of one call from hipEvents in a call of their own, their launches
  decode      the same for the decoder, and the time of the feed() call alone
No target was set in advance; the file records what was measured and how many steps."""
import json
import os
import sys

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "scratch"))
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import torch  # noqa: F401  (first: it brings the HIP runtime the library then shares)
import cwipc_util_amd as cw
import cwipc_util_amd.codec as codec
from cwipc_util_amd import quality
from cwipc_util_amd.capture import _synthetic_cloud
from codec_entropy_timing import WARMUP, STEPS, decoder_record, profile, settled_ms, stream_ms

QUALITIES = (100, 85, 50, 24, 10)
TIMED_QUALITY = 24
CASES = {"sphere_400k": (400_000, 9), "synthetic_300k": (300_000, 9), "synthetic_2m": (2_000_000, 10)}


def sphere_cloud():
    import transform_model as tm
    return cw.cwipc_tilefilter(cw.cwipc_from_numpy_array(tm.sphere_cloud(), 0), 0)        # device-resident, like the synthetic ones


def encoder_record(pc, bits, **form):
    enc = codec.cwipc_new_encoder(octree_bits=bits, jpeg_quality=TIMED_QUALITY, **form)
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


def table_row(pc, bits, q, form):
    kw = dict(entropy=True) if form == "cwae" else dict(colour_transform=True)
    enc = codec.cwipc_new_encoder(octree_bits=bits, jpeg_quality=q, **kw)
    enc.feed(pc)
    assert enc.available(True)
    packet = bytes(enc.get_bytes())
    enc.free()
    if form == "cwae":
        info = codec.entropy_info(packet)
        colour = sum(size + 8 for (mode, size), (kind, _, _) in zip(info["streams"], info["kinds"]) if kind == "colour")
    else:
        info = codec.transform_info(packet)
        colour = info["colour_bytes"]
    result, nbytes = quality.codec_distortion(pc, octree_bits=bits, jpeg_quality=q, plane=False, **kw)
    assert nbytes == len(packet)
    leaves = info["nleaves"]
    return {"form": form, "jpeg_quality": q, "leaves": leaves, "packet_bytes": len(packet), "colour_bytes": colour, "colour_bytes_per_leaf": round(colour / leaves, 4),
            "psnr_y": round(result.psnr_y, 3), "mse_rgb": [round(v, 4) for v in result.symmetric.mse_rgb]}


def run_case(name, out_dir):
    cw.cwipc_hip_set_device(0)
    npoints, bits = CASES[name]
    pc = sphere_cloud() if name.startswith("sphere") else _synthetic_cloud(npoints, 0.0)
    r = {"points": pc.count(), "octree_bits": bits, "timed_jpeg_quality": TIMED_QUALITY, "warmup": WARMUP, "steps": STEPS}
    r["table"] = [table_row(pc, bits, q, form) for q in QUALITIES for form in ("cwae", "cwat")]
    r["encode_entropy"], coded = encoder_record(pc, bits, entropy=True)
    r["encode_transform"], transformed = encoder_record(pc, bits, colour_transform=True)
    t, e = r["encode_transform"], r["encode_entropy"]
    r["encode_transform_over_entropy"] = {"settled": round(t["settled_call"]["median_ms"] / e["settled_call"]["median_ms"], 3),
                                          "stream": round(t["stream_call_ms"] / e["stream_call_ms"], 3)}
    r["transform_kernels_encode"] = {k: [v, t["launches"][k]] for k, v in t["kernels_ms"].items() if k.startswith("transform_")}
    leaves = codec.transform_info(transformed)["nleaves"]
    r["decode_entropy"] = decoder_record(coded, leaves)
    r["decode_transform"] = decoder_record(transformed, leaves)
    t, e = r["decode_transform"], r["decode_entropy"]
    r["decode_transform_over_entropy"] = {"settled": round(t["settled_call"]["median_ms"] / e["settled_call"]["median_ms"], 3),
                                          "stream": round(t["stream_call_ms"] / e["stream_call_ms"], 3)}
    r["transform_kernels_decode"] = {k: [v, t["launches"][k]] for k, v in t["kernels_ms"].items() if k.startswith("transform_")}
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
