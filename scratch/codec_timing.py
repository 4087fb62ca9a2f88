"""Time of the octree codec (cwipc_util_amd.codec) beside get_packet() of the same cloud in the same run.

    python scratch/codec_timing.py [out.json]

Clouds: the synthetic source at 300 k, 2 M and 10 M points, device-resident, with octree_bits 9 / 10 / 12 and jpeg_quality 85.  Per cloud:
  encode      single settled calls (feed, wait, take the bytes; the stream waited for before the clock stops; median of STEPS after
              WARMUP) and a stream of calls (STEPS feeds back to back, then the STEPS packets; total / STEPS), reported separately;
              the kernels of one call from hipEvents (cwipc_hip_profile), in a call of their own
  packet      bytes, bytes per input point, leaves
  get_packet  the thing the codec replaces at the sink end: get_packet() of a cloud with the same planes and no host copy yet,
              settled calls, same STEPS
  decode      settled calls, a stream of calls, kernels, as for encode
  group       an encoder group of 3 octree_bits (bits - 2, bits - 1, bits) against three lone encoders fed one after the other,
              settled calls
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
CASES = ((300_000, 9), (2_000_000, 10), (10_000_000, 12))
QUALITY = 85


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


def main():
    cw.cwipc_hip_set_device(0)
    res = {"warmup": WARMUP, "steps": STEPS, "jpeg_quality": QUALITY, "clouds": {}}
    for npoints, bits in CASES:
        pc = _synthetic_cloud(npoints, 0.0)
        n = pc.count()
        enc = codec.cwipc_new_encoder(octree_bits=bits, jpeg_quality=QUALITY)
        packets = []

        def encode_once():
            enc.feed(pc)
            assert enc.available(True)
            packets[:] = [enc.get_bytes()]

        def take_packet():
            assert enc.available(True)
            packets[:] = [enc.get_bytes()]

        r = {"points": n, "octree_bits": bits}
        r["encode"] = {"settled_call": settled_ms(encode_once), "stream_call_ms": stream_ms(lambda: enc.feed(pc), take_packet)}
        r["encode"].update(profile(encode_once))
        packet = bytes(packets[0])
        info = codec.packet_info(packet)
        r["packet"] = {"bytes": len(packet), "bytes_per_input_point": round(len(packet) / n, 4), "leaves": info["nleaves"],
                       "bytes_per_leaf": round(len(packet) / max(1, info["nleaves"]), 4), "tile_mode": info["tile_mode"]}

        def get_packet_once():
            fresh = cw.cwipc_tilefilter(pc, 0)      # the same planes, no host copy: every call brings the points across
            return fresh.get_packet()

        r["get_packet"] = {"bytes": len(get_packet_once()), "settled_call": settled_ms(get_packet_once)}
        r["get_packet"]["bytes_over_packet_bytes"] = round(r["get_packet"]["bytes"] / len(packet), 2)
        r["encode_settled_over_get_packet_settled"] = round(r["encode"]["settled_call"]["median_ms"] / r["get_packet"]["settled_call"]["median_ms"], 3)

        dec = codec.cwipc_new_decoder()
        clouds = []

        def decode_once():
            dec.feed(packet)
            assert dec.available(True)
            clouds[:] = [dec.get()]

        def take_cloud():
            assert dec.available(True)
            clouds[:] = [dec.get()]

        r["decode"] = {"settled_call": settled_ms(decode_once), "stream_call_ms": stream_ms(lambda: dec.feed(packet), take_cloud)}
        r["decode"].update(profile(decode_once))
        assert clouds[0].count() == info["nleaves"]

        three = [bits - 2, bits - 1, bits]
        group = codec.cwipc_new_encodergroup()
        members = [group.addencoder(octree_bits=b, jpeg_quality=QUALITY) for b in three]
        lone = [codec.cwipc_new_encoder(octree_bits=b, jpeg_quality=QUALITY) for b in three]
        sizes = {}

        def group_once():
            group.feed(pc)
            sizes["group"] = [len(e.get_bytes()) for e in members if e.available(True)]

        def lone_once():
            for e in lone:
                e.feed(pc)
            sizes["lone"] = [len(e.get_bytes()) for e in lone if e.available(True)]

        r["group_of_3"] = {"octree_bits": three, "group_settled_call": settled_ms(group_once), "three_lone_settled_call": settled_ms(lone_once)}
        assert sizes["group"] == sizes["lone"] and len(sizes["group"]) == 3
        r["group_of_3"]["packet_bytes"] = sizes["group"]
        r["group_of_3"]["group_over_lone"] = round(r["group_of_3"]["group_settled_call"]["median_ms"] / r["group_of_3"]["three_lone_settled_call"]["median_ms"], 3)
        group.free()
        res["clouds"][str(npoints)] = r
        print(npoints, json.dumps(r), flush=True)
        del clouds[:], packets[:], pc
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(sys.argv[1]) or ".", exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
