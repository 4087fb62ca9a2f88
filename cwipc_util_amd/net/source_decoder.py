"""A point cloud source that decompresses the packets of a raw source.

The interface of reference python/cwipc/net/source_decoder.py (`cwipc_source_decoder(source, verbose)`,
`cwipc_activesource_decoder(source, verbose)`); written for this library's octree codec (cwipc_util_amd.codec), whose packets are
NOT interoperable with cwipc_codec.  The clouds it hands out are device-resident, so `cwipc_source_synchronizer` joins them where
they are.

The raw source is any object with `get()` giving a packet (or None) and, optionally, `available(wait)`, `eof()`, `start`, `stop`,
`set_fourcc`, `statistics`; a plain list works too: its packets are taken from the front, and it is at its end when it is empty.

The reference decodes on a thread of its own.  Here `available()` and `get()` pull: a packet goes to the decoder, whose feed returns
with the kernels in flight, and the cloud that comes back orders whoever uses it behind them.  No thread, no queue to wait on.

Inter-frame packets (RULE P) need the packet before them: a delta packet that the decoder refuses (one was lost on the way, or the
stream was joined in the middle of a GOP) is logged and skipped, and so are the deltas behind it, until the next key packet.
"""
from __future__ import annotations

import time
from collections import deque
from typing import Any, Deque, List, Optional, Sequence, Union

from .. import codec
from ..util import CwipcError
from ..abstract import cwipc_activesource_abstract, cwipc_pointcloud_abstract, cwipc_source_abstract, cwipc_tileinfo_dict

__all__ = ["cwipc_source_decoder", "cwipc_activesource_decoder"]

FOURCC = "cwao"


class _ListSource:
    def __init__(self, packets: List[Any]):
        self.packets = packets

    def available(self, wait: bool = False) -> bool:
        return len(self.packets) > 0

    def eof(self) -> bool:
        return len(self.packets) == 0

    def get(self) -> Any:
        return self.packets.pop(0) if self.packets else None


class _Decoder(cwipc_activesource_abstract):
    def __init__(self, source: Any, verbose: bool = False, max_octree_bits: Optional[int] = None):
        self.max_octree_bits = max_octree_bits
        self.source = _ListSource(source) if isinstance(source, list) else source
        if hasattr(self.source, "set_fourcc"):
            self.source.set_fourcc(FOURCC)
        self.verbose = verbose
        self.running = False
        self.decomp: Optional[codec.cwipc_decoder_wrapper] = None
        self.output: Deque[cwipc_pointcloud_abstract] = deque()
        self.times_decode: List[float] = []
        self.pointcounts: List[int] = []
        self.skipped = 0   # delta packets refused for want of their reference

    def free(self) -> None:
        if self.decomp is not None:
            self.decomp.free()
        self.decomp = None
        self.output.clear()

    def start(self, startsource: bool = True) -> bool:
        self.running = True
        if startsource and hasattr(self.source, "start"):
            return bool(self.source.start())
        return True

    def stop(self) -> None:
        self.running = False
        if hasattr(self.source, "stop"):
            self.source.stop()

    def _source_eof(self) -> bool:
        return bool(self.source.eof()) if hasattr(self.source, "eof") else False

    def _source_available(self, wait: bool) -> bool:
        if hasattr(self.source, "available"):
            return bool(self.source.available(wait))
        return not self._source_eof()

    def _pull(self, wait: bool) -> bool:
        """One packet from the raw source, if it has one, through the decoder into the output."""
        if not self.running or self._source_eof() or not self._source_available(wait):
            return False
        packet = self.source.get()
        if not packet:
            return False
        if self.decomp is None:
            self.decomp = codec.cwipc_new_decoder(max_octree_bits=self.max_octree_bits)
        t0 = time.time()
        try:
            self.decomp.feed(packet)
        except CwipcError as e:
            if bytes(packet[:4]) != b"cwap" or codec.inter_info_kind(packet) != "delta":
                raise
            self.skipped += 1
            print(f"netdecoder: delta packet skipped, waiting for the next key packet: {e}", flush=True)
            return False
        if not self.decomp.available(True):
            return False
        pc = self.decomp.get()
        if pc is None:
            return False
        self.times_decode.append(time.time() - t0)
        self.pointcounts.append(pc.count())
        self.output.append(pc)
        if self.verbose:
            print(f"netdecoder: decoded pointcloud with {pc.count()} points", flush=True)
        return True

    def eof(self) -> bool:
        return not self.running or (not self.output and self._source_eof())

    def available(self, wait: bool = False) -> bool:
        if not self.running:
            return False
        return bool(self.output) or self._pull(wait)

    def get(self) -> Optional[cwipc_pointcloud_abstract]:
        if not self.output and not self._pull(True):
            return None
        return self.output.popleft()

    def statistics(self) -> None:
        self._print1stat("decode_time", self.times_decode)
        self._print1stat("decode_count", self.pointcounts, True)
        print(f"netdecoder: skipped_deltas: count={self.skipped}")
        if hasattr(self.source, "statistics"):
            self.source.statistics()

    @staticmethod
    def _print1stat(name: str, values: Sequence[Union[int, float]], is_int: bool = False) -> None:
        if not values:
            print(f"netdecoder: {name}: count=0")
            return
        lo, hi = (f"{min(values):d}", f"{max(values):d}") if is_int else (f"{min(values):.3f}", f"{max(values):.3f}")
        print(f"netdecoder: {name}: count={len(values)}, average={sum(values) / len(values):.3f}, min={lo}, max={hi}")

    # the rest of the active-source interface has no meaning for a decoder (as in the reference)
    def request_metadata(self, name: str) -> None:
        raise NotImplementedError

    def is_metadata_requested(self, name: str) -> bool:
        return False

    def reload_config(self, config: Union[str, bytes, None]) -> Any:
        raise NotImplementedError

    def get_config(self) -> bytes:
        raise NotImplementedError

    def seek(self, timestamp: int) -> bool:
        raise NotImplementedError

    def auxiliary_operation(self, op: str, inbuf: bytes, outbuf: bytearray) -> bool:
        raise NotImplementedError

    def maxtile(self) -> int:
        raise NotImplementedError

    def get_tileinfo_dict(self, tilenum: int) -> cwipc_tileinfo_dict:
        raise NotImplementedError


def cwipc_activesource_decoder(source: Any, verbose: bool = False, max_octree_bits: Optional[int] = None) -> cwipc_activesource_abstract:
    """A source that reads packets from an active raw source (started and stopped with it) and decompresses them.  max_octree_bits=t:
    clouds of at most t octree bits (RULE L), whatever the sender coded."""
    return _Decoder(source, verbose=verbose, max_octree_bits=max_octree_bits)


def cwipc_source_decoder(source: Any, verbose: bool = False, max_octree_bits: Optional[int] = None) -> cwipc_source_abstract:
    """A source that reads packets from a raw source and decompresses them; it is running when it is returned.  max_octree_bits: as above."""
    rv = _Decoder(source, verbose=verbose, max_octree_bits=max_octree_bits)
    rv.start(startsource=False)
    return rv
