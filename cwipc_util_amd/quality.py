"""Cloud distortion: what a degraded cloud lost against its original, in the measures of MPEG's pc_error -- point-to-point (D1) and
point-to-plane (D2) geometry error and colour PSNR in BT.709 YUV, each in both directions and combined symmetrically.

The sums are made on the GPU by one call (`cwipc_hip_distortion`, RULE Q of include/cwipc_util_amd/hip_ext.h) and nothing per point
leaves the device; this module turns them into mean squared errors and PSNRs, and wraps the codec in an encode -> decode -> compare
loop in which no cloud becomes a host array.  `sequence_rate` says what inter-frame coding (RULE P) saves on a sequence of frames.

Not pc_error's: a degraded point inherits the normal of its nearest original point (pc_error averages the normals of equally near
points); `peak` defaults to the largest extent of the original's finite bounding box; there is no reflectance.
"""
from __future__ import annotations

import math
from typing import Any, Dict, Iterable, List, Optional, Tuple

from . import util
from .util import cwipc_hip_distortion_sums, cwipc_pointcloud_wrapper

__all__ = ["DirectionalDistortion", "DistortionResults", "psnr", "default_peak", "cloud_distortion", "codec_distortion", "rate_distortion", "sequence_rate"]

NAN = float("nan")


def _ratio(total: float, count: int) -> float:
    return float(total) / float(count) if count else NAN


def _larger(a: float, b: float) -> float:
    """The larger of two mean squared errors; NaN propagates."""
    return NAN if math.isnan(a) or math.isnan(b) else max(a, b)


def psnr(peak2: float, mse: float) -> float:
    """10 log10(peak2 / mse): +inf for an mse of 0, NaN for an mse (or a peak) that is NaN."""
    if math.isnan(mse) or math.isnan(peak2):
        return NAN
    if mse == 0.0:
        return math.inf
    if peak2 == 0.0:
        return -math.inf
    return 10.0 * math.log10(peak2 / mse)


class DirectionalDistortion:
    """One direction: every point of `n_source` source points is matched to its nearest reference point; `n` found one, `n_plane` of
    those pairs have a normal.  mse_d1 = sum d2 / n, mse_d2 = sum r^2 / n_plane, hausdorff = sqrt(max d2), mse_rgb and mse_yuv three
    values each, over n.  A denominator of 0 gives NaN; without a pair hausdorff is 0."""

    __slots__ = ("n_source", "n", "n_plane", "mse_d1", "mse_d2", "hausdorff", "mse_rgb", "mse_yuv")

    def __init__(self, sums: cwipc_hip_distortion_sums):
        self.n_source = int(sums.n_source)
        self.n = int(sums.n)
        self.n_plane = int(sums.n_plane)
        self.mse_d1 = _ratio(sums.sum_d2, self.n)
        self.mse_d2 = _ratio(sums.sum_r2, self.n_plane)
        self.hausdorff = math.sqrt(sums.max_d2)   # (0 without a pair: max d2 is 0 then)
        self.mse_rgb = tuple(_ratio(int(v), self.n) for v in sums.sum_rgb2)
        self.mse_yuv = tuple(_ratio(v, self.n) for v in sums.sum_yuv2)

    def as_dict(self) -> Dict[str, Any]:
        return {name: getattr(self, name) for name in self.__slots__}

    def __eq__(self, other: object) -> bool:
        """Field for field, NaN equal to NaN."""
        return isinstance(other, DirectionalDistortion) and repr(self.as_dict()) == repr(other.as_dict())

    def __repr__(self) -> str:
        return "DirectionalDistortion(%r)" % (self.as_dict(),)


class _Symmetric:
    """The larger mse of the two directions, as in pc_error."""

    __slots__ = ("mse_d1", "mse_d2", "hausdorff", "mse_rgb", "mse_yuv")

    def __init__(self, forward: DirectionalDistortion, backward: DirectionalDistortion):
        self.mse_d1 = _larger(forward.mse_d1, backward.mse_d1)
        self.mse_d2 = _larger(forward.mse_d2, backward.mse_d2)
        self.hausdorff = _larger(forward.hausdorff, backward.hausdorff)
        self.mse_rgb = tuple(_larger(a, b) for a, b in zip(forward.mse_rgb, backward.mse_rgb))
        self.mse_yuv = tuple(_larger(a, b) for a, b in zip(forward.mse_yuv, backward.mse_yuv))

    def as_dict(self) -> Dict[str, Any]:
        return {name: getattr(self, name) for name in self.__slots__}


class DistortionResults:
    """`forward` (source: the original), `backward` (source: the degraded cloud) and `symmetric`; psnr_d1 and psnr_d2 are
    10 log10(3 peak^2 / mse), psnr_y, psnr_u and psnr_v 10 log10(255^2 / mse), of the symmetric mse: +inf for an mse of 0, NaN for NaN."""

    def __init__(self, forward: cwipc_hip_distortion_sums, backward: cwipc_hip_distortion_sums, peak: float):
        self.forward = DirectionalDistortion(forward)
        self.backward = DirectionalDistortion(backward)
        self.symmetric = _Symmetric(self.forward, self.backward)
        self.peak = float(peak)
        geometry = 3.0 * self.peak * self.peak
        self.psnr_d1 = psnr(geometry, self.symmetric.mse_d1)
        self.psnr_d2 = psnr(geometry, self.symmetric.mse_d2)
        self.psnr_y, self.psnr_u, self.psnr_v = (psnr(255.0 * 255.0, m) for m in self.symmetric.mse_yuv)

    def as_dict(self) -> Dict[str, Any]:
        return dict(forward=self.forward.as_dict(), backward=self.backward.as_dict(), symmetric=self.symmetric.as_dict(), peak=self.peak,
                    psnr_d1=self.psnr_d1, psnr_d2=self.psnr_d2, psnr_y=self.psnr_y, psnr_u=self.psnr_u, psnr_v=self.psnr_v)

    def __eq__(self, other: object) -> bool:
        """Field for field, NaN equal to NaN."""
        return isinstance(other, DistortionResults) and repr(self.as_dict()) == repr(other.as_dict())

    def __repr__(self) -> str:
        return "DistortionResults(%r)" % (self.as_dict(),)


def default_peak(original: cwipc_pointcloud_wrapper) -> float:
    """The largest extent of the original's finite bounding box (NaN for a cloud without a finite point)."""
    box = util.cwipc_hip_bounds(original)
    extents = [float(box[3 + a]) - float(box[a]) for a in range(3)]
    return max(extents) if all(math.isfinite(e) and e >= 0.0 for e in extents) else NAN


def cloud_distortion(original: cwipc_pointcloud_wrapper, degraded: cwipc_pointcloud_wrapper, *, max_distance: float = math.inf, normals: Any = None,
                     radius: float = 0.02, max_nn: int = 30, plane: bool = True, peak: Optional[float] = None) -> DistortionResults:
    """The distortion of `degraded` against `original` (cwipc_hip_distortion's arguments), with the PSNRs for `peak` (None: the
    largest extent of the original's finite bounding box)."""
    forward, backward = util.cwipc_hip_distortion(original, degraded, max_distance, normals, radius, max_nn, plane)
    return DistortionResults(forward, backward, default_peak(original) if peak is None else peak)


def _through_the_codec(pc: cwipc_pointcloud_wrapper, entropy: bool, encoder_kwargs: Dict[str, Any], colour_transform: bool = False,
                       decode_bits: Optional[int] = None) -> Tuple[cwipc_pointcloud_wrapper, int]:
    """(the decoded cloud, device-resident; the packet's size in bytes)"""
    from . import codec
    enc = codec.cwipc_new_encoder(entropy=entropy, colour_transform=colour_transform, **encoder_kwargs)
    dec = codec.cwipc_new_decoder(max_octree_bits=decode_bits)
    try:
        enc.feed(pc)
        if not enc.available(True):
            raise util.CwipcError("codec_distortion: the encoder delivered nothing")
        packet = enc.get_bytes()
        dec.feed(packet)
        if not dec.available(True):
            raise util.CwipcError("codec_distortion: the decoder delivered nothing")
        decoded = dec.get()
        if decoded is None:
            raise util.CwipcError("codec_distortion: the decoder delivered nothing")
        return decoded, len(packet)
    finally:
        enc.free()
        dec.free()


def codec_distortion(pc: cwipc_pointcloud_wrapper, *, entropy: bool = False, colour_transform: bool = False, decode_bits: Optional[int] = None,
                     **kwargs: Any) -> Tuple[DistortionResults, int]:
    """cwipc_new_encoder(**encoder keywords) -> cwipc_new_decoder -> cloud_distortion: (the distortion of the decoded cloud against
    `pc`, the packet's bytes).  The keywords max_distance, normals, radius, max_nn, plane and peak go to cloud_distortion, every
    other one to the encoder.  colour_transform=True: the packet is the transform-coded form (RULE T), jpeg_quality its quantiser.
    decode_bits=t: the decoder hands out at most t octree bits (RULE L): "coded at octree_bits, decoded at t".  The decoded cloud never
    becomes a host array."""
    measure = {k: kwargs.pop(k) for k in ("max_distance", "normals", "radius", "max_nn", "plane", "peak") if k in kwargs}
    decoded, nbytes = _through_the_codec(pc, entropy, kwargs, colour_transform, decode_bits)
    return cloud_distortion(pc, decoded, **measure), nbytes


def rate_distortion(pc: cwipc_pointcloud_wrapper, settings: Iterable[Dict[str, Any]]) -> List[Dict[str, Any]]:
    """One row per entry of `settings` (dicts of codec_distortion's keywords, `entropy` and `colour_transform` among them): `settings`, `bytes`,
    `bits_per_input_point` and the symmetric `psnr_d1`, `psnr_d2`, `psnr_y`, `psnr_u`, `psnr_v`.  The original's normals are estimated
    once (cwipc_hip_estimate_normals, with the first `radius` and `max_nn` found in the settings, else 0.02 and 30) and passed to
    every comparison."""
    settings = [dict(s) for s in settings]
    count = pc.count()
    radius = next((s["radius"] for s in settings if "radius" in s), 0.02)
    max_nn = next((s["max_nn"] for s in settings if "max_nn" in s), 30)
    normals = util.cwipc_hip_estimate_normals(pc, radius, max_nn)[0] if count and settings else None
    peak = default_peak(pc) if settings else NAN
    rows = []
    for s in settings:
        kw = dict(s)
        kw.setdefault("normals", normals)
        kw.setdefault("peak", peak)
        result, nbytes = codec_distortion(pc, **kw)
        rows.append(dict(settings=s, bytes=nbytes, bits_per_input_point=8.0 * nbytes / count if count else NAN, psnr_d1=result.psnr_d1,
                         psnr_d2=result.psnr_d2, psnr_y=result.psnr_y, psnr_u=result.psnr_u, psnr_v=result.psnr_v))
    return rows


def sequence_rate(frames: Iterable[cwipc_pointcloud_wrapper], *, entropy: bool = False, **encoder_kwargs: Any) -> List[Dict[str, Any]]:
    """The frames through ONE inter-mode encoder (cwipc_new_encoder's keywords: do_inter_frame=True, gop_size, exp_factor, ...), one row
    per frame: `kind` ("key" or "delta"), `bytes` of the packet, and `intra_bytes`: the same frame coded on its own in the same cube,
    which is the packet the delta stands for (cwipc_util_amd.codec.inter_unpack, on the host), entropy-coded when `entropy`."""
    from . import codec
    enc = codec.cwipc_new_encoder(entropy=entropy, **encoder_kwargs)
    rows: List[Dict[str, Any]] = []
    held: Optional[bytes] = None
    try:
        for pc in frames:
            enc.feed(pc)
            if not enc.available(True):
                raise util.CwipcError("sequence_rate: the encoder delivered nothing")
            packet = bytes(enc.get_bytes())
            info = codec.inter_info(packet)
            plain = bytes(codec.inter_unpack(held, packet))
            if info["kind"] == "key" and info["entropy"]:
                plain = bytes(codec.entropy_unpack(plain))
            intra = len(codec.entropy_pack(plain)) if entropy else len(plain)
            rows.append(dict(kind=info["kind"], gop_index=info["gop_index"], bytes=len(packet), intra_bytes=intra, nleaves=info["nleaves"]))
            held = plain if info["nleaves"] else None
    finally:
        enc.free()
    return rows
