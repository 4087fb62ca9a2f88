"""An octree codec whose packets are NOT interoperable with cwipc_codec, under the names the reference's callers use (`cwipc.codec`).

The interface is the reference's (`cwipc_new_encoder`, `cwipc_new_encodergroup`, `cwipc_new_decoder`, as
python/cwipc/net/sink_encoder.py and source_decoder.py use them), the bitstream is this library's own (RULE C,
include/cwipc_util_amd/hip_ext.h) and carries its own magic, the bytes ``cwao``.
Encoding and decoding run on the GPU; a decoder's clouds are ordinary device-resident clouds.

With ``entropy=True`` an encoder delivers the entropy-coded form of the same packets (RULE E, magic ``cwae``: occupancy, colour and
tile streams through an interleaved rANS coder on the GPU, each stream raw where coding would not shrink it); a decoder takes both
forms.  `entropy_pack`, `entropy_unpack` and `entropy_info` convert and inspect packets on the host.

With ``do_inter_frame=True, gop_size=n, exp_factor=f`` an encoder codes a stream of frames (RULE P, magic ``cwap``): a key packet
every `gop_size` frames (and whenever a frame leaves the GOP's cube, which is the key frame's cube grown by `exp_factor`), delta
packets against the frame before in between.  A decoder fed the packets in order hands out the clouds it would hand out for the
frames coded one by one.  `inter_pack`, `inter_unpack` and `inter_info` do the same on the host.

With ``colour_transform=True`` an encoder delivers transform-coded packets (RULE T, magic ``cwat``): the leaves' 8-bit colours go
through an integer region-adaptive hierarchical transform up the octree, `jpeg_quality` sets the quantiser (100 is exact), and the
coefficients, occupancy and tiles travel through RULE E's coder.  It is off unless asked for and is refused in inter mode.
`transform_pack`, `transform_unpack` and `transform_info` do the same on the host.

A decoder made with ``max_octree_bits=t`` (or told so later by `set_max_octree_bits`) hands out, for every packet of more than `t`
octree bits, the cloud of that packet's cut to `t` bits (RULE L): the geometry of the same cloud coded at `t` bits, each point's
colour the rounded mean of the leaves beneath it.  All four packet forms are covered; in a ``cwap`` chain the decoder's reference
stays the full frame.  `lod(packet, t)` makes the cut packet itself on the host, for ``cwao`` and ``cwae`` packets.

Out of scope: thinning ``cwat`` or ``cwap`` packets in one call, an encoder-side level-of-detail option, cwipc_codec's bitstream, JPEG colour coding, transform colour in inter mode, motion compensation, inter-frame coding inside an encoder
group, per-leaf point counts in the packet, sockets.
"""
from __future__ import annotations

import ctypes
from typing import Any, Dict, List, Optional, Union

from . import util
from .util import CwipcError, cwipc_pointcloud_wrapper

__all__ = [
    "cwipc_encoder_params", "cwipc_new_encoder_params", "cwipc_new_encoder", "cwipc_new_encodergroup", "cwipc_new_decoder",
    "cwipc_encoder_wrapper", "cwipc_encodergroup_wrapper", "cwipc_decoder_wrapper", "packet_info",
    "entropy_pack", "entropy_unpack", "entropy_info", "inter_pack", "inter_unpack", "inter_info",
    "transform_pack", "transform_unpack", "transform_info", "lod",
]


class cwipc_encoder_params(util.cwipc_hip_encoder_params):
    """do_inter_frame, gop_size, exp_factor, octree_bits, jpeg_quality, macroblock_size, tilenumber, voxelsize: positional in this
    order, settable by name."""


def cwipc_new_encoder_params() -> cwipc_encoder_params:
    """The defaults of the reference's sink_encoder: 9 octree bits, quality 85, every tile, no downsampling."""
    return cwipc_encoder_params(False, 1, 1.0, 9, 85, 16, 0, 0)


class cwipc_encoder_wrapper:
    """One encoder: feed(pc), then available(wait) and get_bytes(), first in first out."""

    def __init__(self, handle: int, group: Optional["cwipc_encodergroup_wrapper"] = None):
        self._enc: Optional[int] = handle
        self._group = group   # (an encoder of a group is freed with the group)

    def _handle(self) -> int:
        if not self._enc:
            raise CwipcError("cwipc_encoder_wrapper: used after free()")
        return self._enc

    def __del__(self):
        self.free()

    def free(self) -> None:
        if self._enc and self._group is None:
            util.cwipc_hip_encoder_free(self._enc)
        self._enc = None

    def close(self) -> None:
        util.cwipc_hip_encoder_close(self._handle())

    def set_entropy(self, on: bool = True) -> None:
        """Deliver the entropy-coded form (RULE E); legal before the first feed, CwipcError afterwards."""
        util.cwipc_hip_encoder_set_entropy(self._handle(), on)

    def set_colour_transform(self, on: bool = True) -> None:
        """Deliver the transform-coded form (RULE T); legal before the first feed, CwipcError afterwards and in inter mode."""
        util.cwipc_hip_encoder_set_colour_transform(self._handle(), on)

    def eof(self) -> bool:
        return util.cwipc_hip_encoder_eof(self._handle())

    def at_gop_boundary(self) -> bool:
        return util.cwipc_hip_encoder_at_gop_boundary(self._handle())

    def feed(self, pc: cwipc_pointcloud_wrapper) -> None:
        util.cwipc_hip_encoder_feed(self._handle(), pc)

    def available(self, wait: bool) -> bool:
        return util.cwipc_hip_encoder_available(self._handle(), wait)

    def get_encoded_size(self) -> int:
        return util.cwipc_hip_encoder_get_encoded_size(self._handle())

    def get_bytes(self) -> bytearray:
        """The oldest packet (waits for it when it is still being written)."""
        size = self.get_encoded_size()
        if size == 0:
            raise CwipcError("cwipc_encoder_wrapper.get_bytes: nothing has been fed")
        rv = bytearray(size)
        buffer = (ctypes.c_char * size).from_buffer(rv)
        if not util.cwipc_hip_encoder_copy_data(self._handle(), buffer, size):
            raise CwipcError("cwipc_encoder_wrapper.get_bytes: the copy failed")
        del buffer
        return rv


class cwipc_encodergroup_wrapper:
    """Encoders that are fed together: each delivers byte for byte what it would deliver alone, the filtering and the sort of
    encoders with equal (tilenumber, voxelsize) being made once."""

    def __init__(self, handle: int):
        self._group: Optional[int] = handle
        self._encoders: List[cwipc_encoder_wrapper] = []

    def _handle(self) -> int:
        if not self._group:
            raise CwipcError("cwipc_encodergroup_wrapper: used after free()")
        return self._group

    def __del__(self):
        self.free()

    def free(self) -> None:
        if self._group:
            for enc in self._encoders:
                enc._enc = None
            util.cwipc_hip_encodergroup_free(self._group)
        self._group = None
        self._encoders = []

    def close(self) -> None:
        util.cwipc_hip_encodergroup_close(self._handle())

    def addencoder(self, version: Optional[int] = None, params: Optional[cwipc_encoder_params] = None, **kwargs: Any) -> cwipc_encoder_wrapper:
        entropy = bool(kwargs.pop("entropy", False))
        colour_transform = bool(kwargs.pop("colour_transform", False))
        enc = cwipc_encoder_wrapper(util.cwipc_hip_encodergroup_addencoder(self._handle(), _params(params, kwargs)), self)
        self._encoders.append(enc)
        if entropy:
            enc.set_entropy(True)
        if colour_transform:
            enc.set_colour_transform(True)
        return enc

    def feed(self, pc: cwipc_pointcloud_wrapper) -> None:
        util.cwipc_hip_encodergroup_feed(self._handle(), pc)


class cwipc_decoder_wrapper:
    """feed(packet), then available(wait) and get(): a device-resident cloud per packet, first in first out."""

    def __init__(self, handle: int):
        self._dec: Optional[int] = handle

    def _handle(self) -> int:
        if not self._dec:
            raise CwipcError("cwipc_decoder_wrapper: used after free()")
        return self._dec

    def __del__(self):
        self.free()

    def free(self) -> None:
        if self._dec:
            util.cwipc_hip_decoder_free(self._dec)
        self._dec = None

    def close(self) -> None:
        util.cwipc_hip_decoder_close(self._handle())

    def eof(self) -> bool:
        return util.cwipc_hip_decoder_eof(self._handle())

    def feed(self, buffer: Union[bytes, bytearray, memoryview]) -> None:
        """CwipcError with the reason for a packet that is not valid; such a packet never reaches the device."""
        util.cwipc_hip_decoder_feed(self._handle(), buffer)

    def set_max_octree_bits(self, bits: Optional[int]) -> None:
        """From the next feed on, a packet of more than `bits` octree bits gives the cloud of its cut to `bits` (RULE L); None or 0:
        off.  CwipcError for anything outside 0..16."""
        util.cwipc_hip_decoder_set_max_octree_bits(self._handle(), 0 if bits is None else bits)

    def available(self, wait: bool) -> bool:
        return util.cwipc_hip_decoder_available(self._handle(), wait)

    def get(self) -> Optional[cwipc_pointcloud_wrapper]:
        return util.cwipc_hip_decoder_get(self._handle())


def _params(params: Optional[cwipc_encoder_params], kwargs: Dict[str, Any]) -> cwipc_encoder_params:
    if params is None:
        params = cwipc_new_encoder_params()
    elif kwargs:
        params = cwipc_encoder_params.from_buffer_copy(params)
    names = [f[0] for f in cwipc_encoder_params._fields_]
    for name, value in kwargs.items():
        if name not in names:
            raise CwipcError(f"cwipc_new_encoder: unknown parameter {name!r}")
        setattr(params, name, value)
    return params


def cwipc_new_encoder(version: Optional[int] = None, params: Optional[cwipc_encoder_params] = None, **kwargs: Any) -> cwipc_encoder_wrapper:
    """An encoder for `params` (default: cwipc_new_encoder_params()), single parameters overridden by keyword.  entropy=True: it
    delivers the entropy-coded form of its packets (RULE E).  colour_transform=True: it delivers transform-coded packets (RULE T)."""
    entropy = bool(kwargs.pop("entropy", False))
    colour_transform = bool(kwargs.pop("colour_transform", False))
    enc = cwipc_encoder_wrapper(util.cwipc_hip_new_encoder(_params(params, kwargs)))
    if entropy:
        enc.set_entropy(True)
    if colour_transform:
        enc.set_colour_transform(True)
    return enc


def cwipc_new_encodergroup() -> cwipc_encodergroup_wrapper:
    return cwipc_encodergroup_wrapper(util.cwipc_hip_new_encodergroup())


def cwipc_new_decoder(max_octree_bits: Optional[int] = None) -> cwipc_decoder_wrapper:
    """A decoder; max_octree_bits=t: it hands out clouds of at most t octree bits (RULE L, `set_max_octree_bits`)."""
    dec = cwipc_decoder_wrapper(util.cwipc_hip_new_decoder())
    if max_octree_bits:
        dec.set_max_octree_bits(max_octree_bits)
    return dec


def packet_info(packet: Union[bytes, bytearray, memoryview]) -> Dict[str, Any]:
    """The header of a valid packet (host code, no GPU); CwipcError with the reason otherwise."""
    info = util.cwipc_hip_codec_packet_info(packet)
    return dict(timestamp=info.timestamp, nleaves=info.nleaves, octree_bits=info.octree_bits, colour_bits=info.colour_bits,
                tile_mode=info.tile_mode, tile_value=info.tile_value, min=tuple(info.min), side=info.side,
                nodes=list(info.nodes)[:info.octree_bits], occupancy_offset=info.occupancy_offset, colour_offset=info.colour_offset,
                tile_offset=info.tile_offset, total_bytes=info.total_bytes)


def lod(packet: Union[bytes, bytearray, memoryview], bits: int) -> bytearray:
    """The cut of a valid "cwao" packet to `bits` octree bits (RULE L), or of a "cwae" packet in that form (host code, no GPU);
    CwipcError with the reason for "cwat" and "cwap" packets, a packet that is not valid, bits < 1 and bits above the packet's."""
    return util.cwipc_hip_codec_lod(packet, bits)


def entropy_pack(packet: Union[bytes, bytearray, memoryview]) -> bytearray:
    """The entropy-coded form ("cwae", RULE E) of a valid packet (host code, no GPU); CwipcError with the reason otherwise."""
    return util.cwipc_hip_codec_entropy_pack(packet)


def entropy_unpack(packet: Union[bytes, bytearray, memoryview]) -> bytearray:
    """The packet an entropy-coded packet stands for (host code, no GPU); CwipcError with the reason for one that is refused."""
    return util.cwipc_hip_codec_entropy_unpack(packet)


def entropy_info(packet: Union[bytes, bytearray, memoryview]) -> Dict[str, Any]:
    """The header and the directory of an entropy-coded packet after the container test (host code, no GPU): packet_info()'s keys for
    the packet it stands for, `streams`: [(mode, payload bytes)], `kinds`: [(kind, which, symbols)] and its own `total_bytes`."""
    d = util.cwipc_hip_codec_entropy_info(packet)
    info = d.packet
    names = ("occupancy", "colour", "tile")
    return dict(timestamp=info.timestamp, nleaves=info.nleaves, octree_bits=info.octree_bits, colour_bits=info.colour_bits,
                tile_mode=info.tile_mode, tile_value=info.tile_value, min=tuple(info.min), side=info.side,
                nodes=list(info.nodes)[:info.octree_bits], unpacked_bytes=info.total_bytes,
                streams=[(d.mode[i], d.payload_bytes[i]) for i in range(d.nstreams)],
                kinds=[(names[d.kind[i]], d.which[i], d.symbols[i]) for i in range(d.nstreams)], total_bytes=d.total_bytes)


def transform_pack(packet: Union[bytes, bytearray, memoryview], jpeg_quality: int = 100) -> bytearray:
    """The transform-coded form ("cwat", RULE T) of a valid packet with 8 colour bits at `jpeg_quality` (host code, no GPU)."""
    return util.cwipc_hip_codec_transform_pack(packet, jpeg_quality)


def transform_unpack(packet: Union[bytes, bytearray, memoryview]) -> bytearray:
    """The packet a transform-coded packet stands for (host code, no GPU); CwipcError with the reason for one that is refused."""
    return util.cwipc_hip_codec_transform_unpack(packet)


def transform_info(packet: Union[bytes, bytearray, memoryview]) -> Dict[str, Any]:
    """The header and the directory of a transform-coded packet after the container test (host code, no GPU): packet_info()'s keys for
    the packet it stands for, `q16`, `dc`, `nescapes`, `streams`: [(mode, payload bytes)], `kinds`: [(kind, which, symbols)],
    `colour_bytes` (the token and escape payloads with their directory entries) and its own `total_bytes`."""
    d = util.cwipc_hip_codec_transform_info(packet)
    info = d.packet
    names = {0: "occupancy", 2: "tile", 3: "token", 5: "escape"}
    kinds = [(names[d.kind[i]], d.which[i], d.symbols[i]) for i in range(d.nstreams)]
    return dict(timestamp=info.timestamp, nleaves=info.nleaves, octree_bits=info.octree_bits, colour_bits=info.colour_bits,
                tile_mode=info.tile_mode, tile_value=info.tile_value, min=tuple(info.min), side=info.side,
                nodes=list(info.nodes)[:info.octree_bits], unpacked_bytes=info.total_bytes, q16=d.q16, dc=list(d.dc), nescapes=list(d.nescapes),
                streams=[(d.mode[i], d.payload_bytes[i]) for i in range(d.nstreams)], kinds=kinds,
                colour_bytes=sum(d.payload_bytes[i] + 8 for i in range(d.nstreams) if kinds[i][0] in ("token", "escape")), total_bytes=d.total_bytes)


def inter_pack(reference: Union[bytes, bytearray, memoryview], packet: Union[bytes, bytearray, memoryview], gop_index: int = 1) -> bytearray:
    """The delta packet ("cwap", RULE P) of the plain packet `packet` against the plain packet `reference`, both with leaves and in
    one cube (host code, no GPU); CwipcError with the reason otherwise."""
    return util.cwipc_hip_codec_inter_pack(reference, packet, gop_index)


def inter_unpack(reference: Optional[Union[bytes, bytearray, memoryview]], packet: Union[bytes, bytearray, memoryview]) -> bytearray:
    """The plain packet an inter-frame packet stands for after `reference` (host code, no GPU); a key packet gives its embedded packet
    verbatim and needs no reference; CwipcError with the reason for a packet that is refused."""
    return util.cwipc_hip_codec_inter_unpack(reference, packet)


def inter_info_kind(packet: Union[bytes, bytearray, memoryview]) -> Optional[str]:
    """"key" or "delta" by the prefix of an inter-frame packet alone, None for anything else (no validity test)."""
    p = bytes(packet[:12])
    if len(p) < 12 or p[:4] != b"cwap":
        return None
    return {0: "key", 1: "delta"}.get(int.from_bytes(p[8:12], "little"))


def inter_info(packet: Union[bytes, bytearray, memoryview]) -> Dict[str, Any]:
    """An inter-frame packet after the container test (host code, no GPU): `kind` ("key" or "delta"), `gop_index`, `ref_timestamp`,
    `ref_nleaves`, the header fields of the packet it stands for, and for a delta `nadded`, `nodes_added`, `streams`: [(mode, payload
    bytes)] and `kinds`: [(name, which, symbols)]."""
    d = util.cwipc_hip_codec_inter_info(packet)
    info = d.packet
    names = {0: "occupancy", 3: "bytes", 4: "colour"}
    kinds = []
    for i in range(d.nstreams):
        name = names[d.kind_of[i]]
        if name == "bytes":
            name = "tile" if d.which[i] else "keep"
        kinds.append((name, d.which[i], d.symbols[i]))
    return dict(kind="delta" if d.kind else "key", gop_index=d.gop_index, ref_timestamp=d.ref_timestamp, ref_nleaves=d.ref_nleaves,
                entropy=bool(d.embedded_entropy), timestamp=info.timestamp, nleaves=info.nleaves, octree_bits=info.octree_bits,
                colour_bits=info.colour_bits, tile_mode=info.tile_mode, tile_value=info.tile_value, min=tuple(info.min), side=info.side,
                nadded=d.nadded, nodes_added=list(d.nodes_added)[:info.octree_bits],
                streams=[(d.mode[i], d.payload_bytes[i]) for i in range(d.nstreams)], kinds=kinds, total_bytes=d.total_bytes)
