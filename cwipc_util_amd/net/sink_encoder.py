"""A point cloud sink that compresses what it is fed and hands the packets to a raw sink.

The interface of reference python/cwipc/net/sink_encoder.py (`cwipc_sink_encoder(sink, verbose, nodrop)` with `set_encoder_params`,
`add_stream` through the raw sink, `feed`, `statistics`); written for this library's octree codec (cwipc_util_amd.codec), whose
packets are NOT interoperable with cwipc_codec.  One encoder per tile x octree_bits x jpeg_quality, all in one encoder group, one
stream of the raw sink per encoder, in that order.  With `gop_size` set the encoders code inter-frame (RULE P: key and delta
packets); an encoder group takes no such encoders, so they are lone encoders then, each fed in turn.

The raw sink is any object with `feed(packet, stream_index=...)` and, optionally, `add_stream(tile_index, tile_description,
quality_description)`, `set_fourcc`, `start`, `stop`, `set_producer`, `statistics`; a plain list works too: it is filled with one list of
packets per stream.

Two ways to run it.  After `start()` a thread takes the clouds from a queue of two, as the reference does (a cloud that finds the
queue full is dropped unless `nodrop`).  Without `start()`, `feed()` encodes on the calling thread and returns when the packets have
been handed on: the GPU work needs no thread of its own to overlap with the caller.
"""
from __future__ import annotations

import queue
import threading
import time
from typing import Any, Dict, List, Optional, Sequence, Union

from .. import codec
from ..abstract import cwipc_pointcloud_abstract, cwipc_tileinfo_dict

__all__ = ["cwipc_sink_encoder", "DEFAULT_OCTREE_BITS", "DEFAULT_JPEG_QUALITY"]

DEFAULT_OCTREE_BITS = 9
DEFAULT_JPEG_QUALITY = 85


class _ListSink:
    """A list as raw sink: entry i becomes the list of stream i's packets."""

    def __init__(self, streams: List[Any]):
        self.streams = streams

    def add_stream(self, tile_index: int, tile_description: Any, quality_description: Any) -> int:
        self.streams.append([])
        return len(self.streams) - 1

    def feed(self, packet: Union[bytes, bytearray], stream_index: int = 0) -> bool:
        while len(self.streams) <= stream_index:
            self.streams.append([])
        self.streams[stream_index].append(bytes(packet))
        return True


def _intlist(value: Union[int, Sequence[int], None], default: List[int]) -> List[int]:
    if value is None:
        return default
    if isinstance(value, int):
        return [value]
    return [int(v) for v in value]


class _SinkEncoder:
    FOURCC = "cwao"   # not the reference's "cwi1": the bitstream is another one
    QUEUE_FULL_TIMEOUT = 0.001

    def __init__(self, sink: Any, verbose: bool = False, nodrop: bool = False):
        self.sink = _ListSink(sink) if isinstance(sink, list) else sink
        if hasattr(self.sink, "set_fourcc"):
            self.sink.set_fourcc(self.FOURCC)
        self.verbose = verbose
        self.nodrop = nodrop
        self.producer: Any = None
        self.tiledescriptions: List[cwipc_tileinfo_dict] = [{}]
        self.octree_bits: List[int] = [DEFAULT_OCTREE_BITS]
        self.jpeg_quality: List[int] = [DEFAULT_JPEG_QUALITY]
        self.entropy = False
        self.colour_transform = False
        self.gop_size: Optional[int] = None
        self.exp_factor = 1.0
        self.encoder_group: Optional[codec.cwipc_encodergroup_wrapper] = None
        self.encoders: List[codec.cwipc_encoder_wrapper] = []
        self.streams: List[int] = []
        self.times_encode: List[float] = []
        self.pointcounts: List[int] = []
        self.packetsizes: List[int] = []
        self.input_queue: "queue.Queue[Optional[cwipc_pointcloud_abstract]]" = queue.Queue(maxsize=2)
        self.thread: Optional[threading.Thread] = None
        self.stopped = False

    def set_encoder_params(self, tiles: Optional[List[cwipc_tileinfo_dict]], octree_bits: Union[int, Sequence[int], None] = None,
                           jpeg_quality: Union[int, Sequence[int], None] = None, entropy: bool = False, gop_size: Optional[int] = None,
                           exp_factor: Optional[float] = None, colour_transform: bool = False) -> None:
        """entropy=True: every encoder delivers the entropy-coded form of its packets (cwipc_util_amd.codec, RULE E); a
        cwipc_source_decoder takes both forms.  gop_size (2 or more), with exp_factor (default 1.25): inter-frame coding, a key
        packet every gop_size frames and delta packets in between (RULE P).  colour_transform=True: every encoder delivers transform-coded
        packets (RULE T), jpeg_quality being the quantiser; not together with gop_size."""
        assert self.encoder_group is None and not self.encoders, "set_encoder_params comes before the first cloud"
        self.entropy = bool(entropy)
        self.colour_transform = bool(colour_transform)
        self.gop_size = int(gop_size) if gop_size is not None else None
        self.exp_factor = float(exp_factor) if exp_factor is not None else (1.25 if self.gop_size is not None else 1.0)
        self.tiledescriptions = tiles if tiles else [{}]
        self.octree_bits = _intlist(octree_bits, self.octree_bits)
        self.jpeg_quality = _intlist(jpeg_quality, self.jpeg_quality)

    def add_stream(self, tile_index: int, tile_description: Any, quality_description: Dict[str, int]) -> int:
        """A further stream of the raw sink (the encoders' own streams are added when the encoders are made)."""
        if hasattr(self.sink, "add_stream"):
            return self.sink.add_stream(tile_index, tile_description, quality_description)
        return len(self.streams)

    def set_producer(self, producer: Any) -> None:
        self.producer = producer
        if hasattr(self.sink, "set_producer"):
            self.sink.set_producer(producer)

    def _init_encoders(self) -> None:
        if self.encoder_group is not None or self.encoders:
            return
        inter = self.gop_size is not None
        if not inter:
            self.encoder_group = codec.cwipc_new_encodergroup()
        for tile_index, tile in enumerate(self.tiledescriptions):
            mask = int(tile.get("cameraMask", 0))
            for bits in self.octree_bits:
                for quality in self.jpeg_quality:
                    params = codec.cwipc_encoder_params(inter, self.gop_size if inter else 1, self.exp_factor, bits, quality, 16, mask, 0)
                    if inter:
                        self.encoders.append(codec.cwipc_new_encoder(params=params, entropy=self.entropy, colour_transform=self.colour_transform))
                    else:
                        self.encoders.append(self.encoder_group.addencoder(params=params, entropy=self.entropy, colour_transform=self.colour_transform))
                    self.streams.append(self.add_stream(tile_index, tile, dict(octree_bits=bits, jpeg_quality=quality)))
                    if self.verbose:
                        print(f"encoder: stream {self.streams[-1]}: tile={tile_index} mask={mask} octree_bits={bits} jpeg_quality={quality}")

    def _encode(self, pc: cwipc_pointcloud_abstract) -> None:
        self._init_encoders()
        self.pointcounts.append(pc.count())
        t0 = time.time()
        if self.encoder_group is not None:
            self.encoder_group.feed(pc)
        else:
            for enc in self.encoders:
                enc.feed(pc)
        packets = []
        for enc in self.encoders:
            if not enc.available(True):
                raise RuntimeError("encoder: no packet after feed")
            packets.append(enc.get_bytes())
        self.times_encode.append(time.time() - t0)
        self.packetsizes.extend(len(p) for p in packets)
        if len(packets) == 1:
            self.sink.feed(packets[0])
        else:
            for stream, packet in zip(self.streams, packets):
                self.sink.feed(packet, stream_index=stream)

    def start(self) -> None:
        self._init_encoders()
        self.thread = threading.Thread(target=self._run, name="cwipc_util._Sink_Encoder")
        self.thread.start()
        if hasattr(self.sink, "start"):
            self.sink.start()

    def stop(self) -> None:
        self.stopped = True
        if self.thread is not None:
            try:
                self.input_queue.put(None, block=self.nodrop)
            except queue.Full:
                pass
            self.thread.join()
            self.thread = None
        if hasattr(self.sink, "stop"):
            self.sink.stop()

    def is_alive(self) -> bool:
        return not self.stopped

    def _run(self) -> None:
        while True:
            try:
                pc = self.input_queue.get(timeout=0.1)
            except queue.Empty:
                if self.stopped:
                    break
                continue
            if pc is None:
                break
            self._encode(pc)

    def feed(self, pc: cwipc_pointcloud_abstract) -> None:
        if self.thread is None:
            self._encode(pc)
            return
        try:
            if self.nodrop:
                self.input_queue.put(pc)
            else:
                self.input_queue.put(pc, timeout=self.QUEUE_FULL_TIMEOUT)
        except queue.Full:
            if self.verbose:
                print("encoder: queue full, cloud dropped")

    def free(self) -> None:
        if self.encoder_group is not None:
            self.encoder_group.free()
        else:
            for enc in self.encoders:
                enc.free()
        self.encoder_group = None
        self.encoders = []

    def statistics(self) -> None:
        self._print1stat("encode_duration", self.times_encode)
        self._print1stat("encode_count", self.pointcounts, True)
        self._print1stat("packetsize", self.packetsizes, True)
        if hasattr(self.sink, "statistics"):
            self.sink.statistics()

    @staticmethod
    def _print1stat(name: str, values: Sequence[Union[int, float]], is_int: bool = False) -> None:
        if not values:
            print(f"encoder: {name}: count=0")
            return
        lo, hi = (f"{min(values):d}", f"{max(values):d}") if is_int else (f"{min(values):.3f}", f"{max(values):.3f}")
        print(f"encoder: {name}: count={len(values)}, average={sum(values) / len(values):.3f}, min={lo}, max={hi}")


def cwipc_sink_encoder(sink: Any, verbose: bool = False, nodrop: bool = False) -> _SinkEncoder:
    """A sink that compresses point clouds with this library's octree codec and forwards the packets to the raw sink."""
    return _SinkEncoder(sink, verbose=verbose, nodrop=nodrop)
