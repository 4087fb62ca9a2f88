"""
Print the rate-distortion table of the octree codec on one point cloud.

The cloud is encoded and decoded at every combination of the given octree depths and colour qualities, and each decoded cloud is
compared with the original on the GPU: the packet's size, the bits it spends per input point, and the symmetric PSNRs of the
point-to-point error (D1), the point-to-plane error (D2) and the colour error in BT.709 YUV -- the measures of MPEG's pc_error,
by this library's RULE Q (include/cwipc_util_amd/hip_ext.h).  No decoded cloud leaves the device.  No reference counterpart.

With --decode-bits T every packet is also decoded by a decoder that hands out at most T octree bits (RULE L): the row "coded at b,
decoded at T" stands beside the row "coded at T", whose packet is the smaller one.

With --gop the table is another one: a sequence of frames (the synthetic source's, which turns from frame to frame, or the input
file over and over) goes through one inter-frame encoder (RULE P), and every frame gets a row with its packet's kind and size
beside the size of the same frame coded on its own.
"""
import argparse
from typing import Any, Dict, List, Optional, Sequence

from .. import util as cwipc
from .. import quality

__all__ = ["CodecQualityTable", "build_parser", "main"]

GOP_COLUMNS = ("frame", "kind", "bytes", "intra_bytes", "ratio")
COLUMNS = ("octree_bits", "jpeg_quality", "entropy", "bytes", "bits_per_input_point", "psnr_d1", "psnr_d2", "psnr_y", "psnr_u", "psnr_v")


class CodecQualityTable:
    """args: the namespace of build_parser(); input_pc: the cloud to measure on (or load_input() later)."""

    def __init__(self, args: argparse.Namespace, input_pc: Optional[cwipc.cwipc_pointcloud_wrapper] = None):
        self.args = args
        self.octree_bits: Sequence[int] = args.octree_bits or [9]
        self.jpeg_quality: Sequence[int] = args.jpeg_quality or [85]
        self.entropy = bool(args.entropy)
        self.colour_transform = bool(getattr(args, "colour_transform", False))
        self.decode_bits: Sequence[int] = getattr(args, "decode_bits", None) or []
        self.gop = int(getattr(args, "gop", 0) or 0)
        self.exp_factor = float(getattr(args, "exp_factor", 1.25))
        self.nframes = int(getattr(args, "frames", 0) or 0) or 2 * max(self.gop, 1)
        self.input_pc = input_pc
        self.frames: List[cwipc.cwipc_pointcloud_wrapper] = []
        self.rows: List[Dict[str, Any]] = []

    def load_input(self, source: Optional[str], synthetic: int = 0) -> None:
        if synthetic:
            src = cwipc.cwipc_synthetic(0, synthetic)
            src.start()
            self.input_pc = src.get()
            if self.gop:
                self.frames = [self.input_pc] + [src.get() for _ in range(self.nframes - 1)]
            src.stop()
        else:
            assert source
            self.input_pc = cwipc.cwipc_read(source, 0)

    def settings(self) -> List[Dict[str, Any]]:
        extra = dict(colour_transform=True) if self.colour_transform else {}
        rows = []
        for b in self.octree_bits:
            for q in self.jpeg_quality:
                rows.append(dict(octree_bits=b, jpeg_quality=q, entropy=self.entropy, **extra))
                rows += [dict(octree_bits=b, jpeg_quality=q, entropy=self.entropy, decode_bits=t, **extra) for t in self.decode_bits if t < b]
        return rows

    def run(self) -> None:
        assert self.input_pc
        if self.gop:
            frames = self.frames or [self.input_pc] * self.nframes
            self.rows = quality.sequence_rate(frames, entropy=self.entropy, do_inter_frame=True, gop_size=self.gop, exp_factor=self.exp_factor,
                                              octree_bits=self.octree_bits[0], jpeg_quality=self.jpeg_quality[0])
        else:
            self.rows = quality.rate_distortion(self.input_pc, self.settings())

    def table(self) -> str:
        if self.gop:
            lines = ["%6s %6s %10s %12s %6s" % GOP_COLUMNS]
            for i, row in enumerate(self.rows):
                lines.append("%6d %6s %10d %12d %6.3f" % (i, row["kind"], row["bytes"], row["intra_bytes"], row["bytes"] / row["intra_bytes"]))
            return "\n".join(lines)
        cut = bool(self.decode_bits)   # one more column, in front: the octree bits the decoder handed out
        lines = [("%11s " % "decode_bits" if cut else "") + "%11s %12s %7s %10s %20s %8s %8s %8s %8s %8s" % COLUMNS]
        for row in self.rows:
            flat = dict(row["settings"], **{k: v for k, v in row.items() if k != "settings"})
            lines.append(("%11d " % flat.get("decode_bits", flat["octree_bits"]) if cut else "") +
                         "%11d %12d %7s %10d %20.4f %8.2f %8.2f %8.2f %8.2f %8.2f" % tuple(flat[c] for c in COLUMNS))
        return "\n".join(lines)


def build_parser() -> argparse.ArgumentParser:
    assert __doc__ is not None
    parser = argparse.ArgumentParser(description=__doc__.strip(), formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("input", nargs="?", help="Input point cloud .ply file")
    parser.add_argument("--synthetic", type=int, metavar="NPOINTS", default=0, help="Measure on the synthetic cloud of about this many points instead of a file")
    parser.add_argument("--octree_bits", type=int, action="append", metavar="BITS", help="Octree depth to encode at. Repeat for each depth (default: 9)")
    parser.add_argument("--jpeg_quality", type=int, action="append", metavar="Q", help="Colour quality to encode at. Repeat for each quality (default: 85)")
    parser.add_argument("--entropy", action="store_true", help="Measure the entropy-coded packets (same distortion, fewer bytes)")
    parser.add_argument("--colour-transform", dest="colour_transform", action="store_true",
                        help="Measure transform-coded packets: --jpeg_quality sets the quantiser of the colour transform (100 is exact). Not with --gop")
    parser.add_argument("--decode-bits", dest="decode_bits", type=int, action="append", metavar="T",
                        help="Also decode every packet of more than T octree bits at T bits (level-of-detail decoding). Repeat for each T. Not with --gop")
    parser.add_argument("--gop", type=int, metavar="N", default=0, help="Inter-frame coding with a key packet every N frames (2 or more): print bytes per frame against intra "
                        "coding, at the first octree depth and quality given")
    parser.add_argument("--exp_factor", type=float, default=1.25, help="With --gop: how much larger than a key frame's cube the cube of its GOP is (default: 1.25)")
    parser.add_argument("--frames", type=int, default=0, help="With --gop: the number of frames (default: two GOPs)")
    return parser


def main() -> None:
    parser = build_parser()
    args = parser.parse_args()
    if bool(args.input) == bool(args.synthetic):
        parser.error("give either an input file or --synthetic NPOINTS")
    if args.colour_transform and args.gop:
        parser.error("--colour-transform is not available with --gop")
    if args.decode_bits and args.gop:
        parser.error("--decode-bits is not available with --gop")
    creator = CodecQualityTable(args)
    creator.load_input(args.input, args.synthetic)
    creator.run()
    print(creator.table())


if __name__ == '__main__':
    main()
