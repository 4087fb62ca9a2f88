"""Time and size of inter-frame coding (cwipc_util_amd.codec with do_inter_frame; RULE P) beside the entropy-coded intra form, same run.

    python scratch/inter_timing.py CASE OUT_DIR        one sequence, its record to OUT_DIR/CASE.json
    python scratch/inter_timing.py --merge OUT_DIR OUT.json

One process per sequence, so that each can run under a time limit of its own and a step that fails ends the chain:

    for c in turning_300k still_300k turning_2m still_2m; do
        timeout -k 10 240 python scratch/inter_timing.py $c out || exit 1
    done && python scratch/inter_timing.py --merge out profiles/codec_inter_timing.json

Sequences: the synthetic source at 300 k points with octree_bits 9 and at 2 M points with 10, turning by its angle from frame to frame
(1/30 s a frame: its geometry stays, its colours move) and held still.  gop_size 8, exp_factor 1.25, jpeg_quality 85, entropy on.
FRAMES frames after one GOP of warm-up, each fed, waited for and taken before the next.  Per sequence:
  bytes       per frame by kind, beside the frame's "cwae" packet from a plain encoder (its own cube, so a key packet is a little larger)
  encode      the whole call (feed, wait, take the bytes) and the feed() call alone, medians by kind, against the "cwae" encoder on the
              same frames; a delta's feed holds both of its waits, a key's and the intra encoder's the one of the sort, so the
              difference of the feed times bounds what the second wait and the match in front of it cost
  decode      the same for the decoder: the packets of the inter encoder against the "cwae" packets
  kernels     hipEvent times of one GOP's encode and decode, in calls of their own
No target was set in advance; the file records what was measured and how many frames."""
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
GOP, EXP, QUALITY, FRAMES = 8, 1.25, 85, 24
CASES = {"turning_300k": (300_000, 9, 1.0 / 30.0), "still_300k": (300_000, 9, 0.0), "turning_2m": (2_000_000, 10, 1.0 / 30.0), "still_2m": (2_000_000, 10, 0.0)}


def by_kind(kinds, values, scale=1e3):
    out = {}
    for kind in sorted(set(kinds)):
        v = [x for k, x in zip(kinds, values) if k == kind]
        out[kind] = {"count": len(v), "median": round(float(np.median(v)) * scale, 4), "min": round(min(v) * scale, 4), "max": round(max(v) * scale, 4)}
    return out


def encode(enc, frames, warmup):
    """(packets, whole-call seconds, feed-call seconds) for the frames behind the warm-up."""
    packets, whole, feeds = [], [], []
    for i, pc in enumerate(frames):
        sync()
        t0 = time.perf_counter()
        enc.feed(pc)
        t1 = time.perf_counter()
        assert enc.available(True)
        packet = bytes(enc.get_bytes())
        t2 = time.perf_counter()
        if i >= warmup:
            packets.append(packet)
            whole.append(t2 - t0)
            feeds.append(t1 - t0)
    return packets, whole, feeds


def decode(dec, packets, warmup):
    whole, feeds = [], []
    for i, packet in enumerate(packets):
        sync()
        t0 = time.perf_counter()
        dec.feed(packet)
        t1 = time.perf_counter()
        assert dec.available(True)
        pc = dec.get()
        sync()
        t2 = time.perf_counter()
        assert pc is not None
        if i >= warmup:
            whole.append(t2 - t0)
            feeds.append(t1 - t0)
    return whole, feeds


def profile(fn):
    with cw.cwipc_hip_profile() as prof:
        fn()
        sync()
    kernels = {k: round(v[0], 4) for k, v in prof.kernels.items()}
    return {"kernels_ms": kernels, "launches": {k: int(v[1]) for k, v in prof.kernels.items()}, "kernels_total_ms": round(sum(kernels.values()), 4)}


def run_case(name, out_dir):
    cw.cwipc_hip_set_device(0)
    npoints, bits, step = CASES[name]
    frames = [_synthetic_cloud(npoints, step * i) for i in range(GOP + FRAMES)]
    r = {"points": frames[0].count(), "octree_bits": bits, "jpeg_quality": QUALITY, "gop_size": GOP, "exp_factor": EXP, "angle_step": step,
         "warmup_frames": GOP, "frames": FRAMES}
    inter = codec.cwipc_new_encoder(do_inter_frame=True, gop_size=GOP, exp_factor=EXP, octree_bits=bits, jpeg_quality=QUALITY, entropy=True)
    intra = codec.cwipc_new_encoder(octree_bits=bits, jpeg_quality=QUALITY, entropy=True)
    all_inter, _, _ = encode(inter, frames[:GOP], 0)                     # the warm-up GOP, kept for the decoder's
    packets, whole, feeds = encode(inter, frames[GOP:], 0)
    all_intra, _, _ = encode(intra, frames[:GOP], 0)
    intra_packets, intra_whole, intra_feeds = encode(intra, frames[GOP:], 0)
    kinds = [codec.inter_info(p)["kind"] for p in packets]
    r["bytes"] = by_kind(kinds, [len(p) for p in packets], 1)
    r["bytes"]["cwae"] = by_kind(["cwae"] * FRAMES, [len(p) for p in intra_packets], 1)["cwae"]
    r["delta_over_cwae_bytes"] = round(r["bytes"]["delta"]["median"] / r["bytes"]["cwae"]["median"], 4)
    r["gop_over_cwae_bytes"] = round(sum(len(p) for p in packets) / sum(len(p) for p in intra_packets), 4)
    info = codec.inter_info(next(p for p, k in zip(packets, kinds) if k == "delta"))
    r["a_delta"] = {"nleaves": info["nleaves"], "ref_nleaves": info["ref_nleaves"], "nadded": info["nadded"],
                    "streams": [(k[0], k[2], m, b) for k, (m, b) in zip(info["kinds"], info["streams"])]}
    r["encode_call_ms"] = by_kind(kinds, whole)
    r["encode_call_ms"]["cwae"] = by_kind(["cwae"] * FRAMES, intra_whole)["cwae"]
    r["encode_feed_ms"] = by_kind(kinds, feeds)
    r["encode_feed_ms"]["cwae"] = by_kind(["cwae"] * FRAMES, intra_feeds)["cwae"]
    r["second_wait_and_match_ms_at_most"] = round(r["encode_feed_ms"]["delta"]["median"] - r["encode_feed_ms"]["key"]["median"], 4)
    dec, dec_intra = codec.cwipc_new_decoder(), codec.cwipc_new_decoder()
    whole, feeds = decode(dec, all_inter + packets, GOP)
    intra_whole, intra_feeds = decode(dec_intra, all_intra + intra_packets, GOP)
    r["decode_call_ms"] = by_kind(kinds, whole)
    r["decode_call_ms"]["cwae"] = by_kind(["cwae"] * FRAMES, intra_whole)["cwae"]
    r["decode_feed_ms"] = by_kind(kinds, feeds)
    r["decode_feed_ms"]["cwae"] = by_kind(["cwae"] * FRAMES, intra_feeds)["cwae"]
    fresh = codec.cwipc_new_encoder(do_inter_frame=True, gop_size=GOP, exp_factor=EXP, octree_bits=bits, jpeg_quality=QUALITY, entropy=True)
    gop_packets = []
    r["encode_one_gop"] = profile(lambda: gop_packets.extend(encode(fresh, frames[:GOP], 0)[0]))
    r["decode_one_gop"] = profile(lambda: decode(codec.cwipc_new_decoder(), gop_packets, 0))
    r["encode_one_gop_cwae"] = profile(lambda: encode(intra, frames[:GOP], 0))
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, name + ".json"), "w") as f:
        json.dump(r, f, indent=1)
    print(name, json.dumps(r), flush=True)


def merge(out_dir, out):
    res = {"sequences": {}}
    for name in CASES:
        path = os.path.join(out_dir, name + ".json")
        if os.path.exists(path):
            with open(path) as f:
                res["sequences"][name] = json.load(f)
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    if sys.argv[1] == "--merge":
        merge(sys.argv[2], sys.argv[3])
    else:
        run_case(sys.argv[1], sys.argv[2])
