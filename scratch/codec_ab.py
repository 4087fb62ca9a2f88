"""One side of the A/B of the octree codec's host driver: the library comes from CWIPC_LIBRARY_DIR (unset: this tree's).

    python scratch/codec_ab.py CASE OUT.json          CASE: synthetic_300k (9 bits) or structured_2m (10 bits)
    python scratch/codec_ab.py --table DIR OUT.txt    the rows of profiles/codec_split_ab.txt from DIR/{parent,this}_CASE_I.json

Workloads and per-call method are those of scratch/codec_timing.py, codec_entropy_timing.py, codec_transform_timing.py,
codec_lod_timing.py and inter_timing.py (settled: the median of STEPS waited-for calls after WARMUP; stream: STEPS feeds back to back,
then the STEPS results, total / STEPS; feed: the decoder's feed() call alone, median; launches: the kernels of one profiled call),
without their size and quality records.  Every packet form, encode and decode: "cwao", "cwae", "cwat", and "cwap" as one GOP a call
(a key and three deltas; the synthetic cloud turns from frame to frame, the structured one stands still); the decoder also with
max_octree_bits two below the packet's.  sha256 of every packet and every decoded cloud."""
import hashlib
import json
import os
import sys
import time

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "scratch"))
import numpy as np

QUALITY, GOP = 85, 4
CASES = {"synthetic_300k": (300_000, 9), "structured_2m": (2_000_000, 10)}
FORMS = {"cwao": dict(), "cwae": dict(entropy=True), "cwat": dict(colour_transform=True)}
TIMES = ("settled_ms", "stream_ms", "feed_ms")


def run_case(name, out):
    import torch  # noqa: F401  (first: it brings the HIP runtime the library then shares)
    import cwipc_util_amd as cw
    import cwipc_util_amd.codec as codec
    from cwipc_util_amd.capture import _synthetic_cloud
    from codec_entropy_timing import WARMUP, STEPS, profile, settled_ms, stream_ms, structured_cloud

    def sha(data):
        return hashlib.sha256(data).hexdigest()[:16]

    def cloud_sha(pc):
        return sha(np.ascontiguousarray(pc.get_numpy_array()).tobytes())

    cw.cwipc_hip_set_device(0)
    npoints, bits = CASES[name]
    structured = name.startswith("structured")
    pc = structured_cloud(npoints) if structured else _synthetic_cloud(npoints, 0.0)
    frames = [pc] * GOP if structured else [_synthetic_cloud(npoints, i / 30.0) for i in range(GOP)]
    for i, frame in enumerate([pc] + frames):   # (the synthetic source stamps its clouds with the time of day, and a packet carries the stamp)
        frame._set_timestamp(1000 + i)
    res = {"lib": cw.util.cwipc_util_dll_load()._name, "points": pc.count(), "octree_bits": bits, "warmup": WARMUP, "steps": STEPS, "rows": {}, "sha256": {}}

    def record(label, once, feed, take, feeds=None):
        r = {"settled_ms": settled_ms(once)["median_ms"]}
        if feeds is not None:
            r["feed_ms"] = round(float(np.median(feeds[WARMUP:])) * 1e3, 4)
        r["stream_ms"] = stream_ms(feed, take)
        r["launches"] = profile(once)["launches"]
        res["rows"][label] = r
        print(label, json.dumps(r), flush=True)

    def encoder_rows(label, enc, clouds):
        packets = []

        def feed():
            for c in clouds:
                enc.feed(c)

        def take():
            packets.clear()
            for _ in clouds:
                assert enc.available(True)
                packets.append(bytes(enc.get_bytes()))

        def once():
            feed()
            take()

        record(label + ".encode", once, feed, take)
        for i, p in enumerate(packets):
            res["sha256"]["%s.packet%d" % (label, i)] = sha(p)
        enc.free()
        return list(packets)

    def decoder_rows(label, packets, t):
        dec = codec.cwipc_new_decoder(max_octree_bits=t)
        clouds, feeds = [], []

        def feed():
            t0 = time.perf_counter()
            for p in packets:
                dec.feed(p)
            feeds.append(time.perf_counter() - t0)

        def take():
            clouds.clear()
            for _ in packets:
                assert dec.available(True)
                clouds.append(dec.get())

        def once():
            feed()
            take()

        record(label, once, feed, take, feeds)
        for i, c in enumerate(clouds):
            res["sha256"]["%s.cloud%d" % (label, i)] = cloud_sha(c)
        dec.free()

    for form, kw in FORMS.items():
        packets = encoder_rows(form, codec.cwipc_new_encoder(octree_bits=bits, jpeg_quality=QUALITY, **kw), [pc])
        decoder_rows(form + ".decode", packets, 0)
        decoder_rows(form + ".decode_cut", packets, bits - 2)
    packets = encoder_rows("cwap", codec.cwipc_new_encoder(do_inter_frame=True, gop_size=GOP, exp_factor=1.25, octree_bits=bits, jpeg_quality=QUALITY, entropy=True), frames)
    assert [codec.inter_info(p)["kind"] for p in packets] == ["key"] + ["delta"] * (GOP - 1)
    decoder_rows("cwap.decode", packets, 0)
    decoder_rows("cwap.decode_cut", packets, bits - 2)
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


def table(directory, out):
    lines = []
    for case in CASES:
        runs = {side: [] for side in ("parent", "this")}
        for side in runs:
            i = 0
            while os.path.exists(os.path.join(directory, "%s_%s_%d.json" % (side, case, i))):
                with open(os.path.join(directory, "%s_%s_%d.json" % (side, case, i))) as f:
                    runs[side].append(json.load(f))
                i += 1
        if not runs["parent"] or not runs["this"]:
            continue
        hashes = {json.dumps(r["sha256"], sort_keys=True) for side in runs for r in runs[side]}
        lines.append("%s: %d points, %d bits; %d + %d processes; %d sha256 per process, %s" % (
            case, runs["this"][0]["points"], runs["this"][0]["octree_bits"], len(runs["parent"]), len(runs["this"]), len(runs["this"][0]["sha256"]),
            "identical in every process of both libraries" if len(hashes) == 1 else "DIFFERENT"))
        for label in runs["this"][0]["rows"]:
            launches = {json.dumps(r["rows"][label]["launches"], sort_keys=True) for side in runs for r in runs[side]}
            lines.append("%-46s launches %s: %s" % (case + "." + label, "equal" if len(launches) == 1 else "DIFFERENT", json.dumps(runs["this"][0]["rows"][label]["launches"], sort_keys=True)))
            for key in TIMES:
                if key not in runs["this"][0]["rows"][label]:
                    continue
                par = sorted(r["rows"][label][key] for r in runs["parent"])
                this = float(np.median([r["rows"][label][key] for r in runs["this"]]))
                verdict = "within" if par[0] <= this <= par[-1] else "faster" if this < par[0] else "OUTSIDE (%+.1f %% of the parent's median)" % (100 * (this / float(np.median(par)) - 1))
                lines.append("%-46s %9.4f %9.4f %9.4f | %9.4f  %s" % (case + "." + label + "." + key, par[0], float(np.median(par)), par[-1], this, verdict))
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    if sys.argv[1] == "--table":
        table(sys.argv[2], sys.argv[3])
    else:
        run_case(sys.argv[1], sys.argv[2])
