"""
Create a point cloud for testing analysis and registration.

A well-registered cloud is cut into the tiles of N simulated cameras (soft assignment), every tile is moved, rotated or tilted by a
known amount, the tiles are joined again and noise is added: a mis-registered N-camera frame whose ground truth -- the seed and every
tile's 4x4 transform -- goes into the description.  Counterpart of reference python/cwipc/scripts/cwipc_create_analysis_test.py
(same arguments, plus --seed); every step runs on the GPU and the result is reproducible from the seed.
"""
import argparse
import json
import os
import os.path
from typing import Any, Dict, List, Optional, Sequence

import numpy as np

from .. import util as cwipc
from ..filters.noise import NoiseFilter
from ..filters.simulatecams import SimulatecamsFilter

__all__ = ["AnalysisTestCreator", "build_parser", "main", "rotation_matrix"]


def rotation_matrix(axis: str, angle: float) -> np.ndarray:
    """The 4x4 matrix of the elementary rotation by `angle` radians about the x, y or z axis (right-handed, as scipy's from_euler)."""
    c, s = float(np.cos(angle)), float(np.sin(angle))
    m = np.identity(4)
    i, j = {'x': (1, 2), 'y': (2, 0), 'z': (0, 1)}[axis]
    m[i, i], m[i, j], m[j, i], m[j, j] = c, -s, s, c
    return m


def _amount(values: Optional[Sequence[float]], camnum: int) -> float:
    return float(values[camnum]) if values and camnum < len(values) else 0.0


class AnalysisTestCreator:
    """args: the namespace of build_parser(); input_pc: the cloud to start from (or load_input() later)."""

    def __init__(self, args: argparse.Namespace, input_pc: Optional[cwipc.cwipc_pointcloud_wrapper] = None):
        self.args = args
        self.verbose = args.verbose
        self.noise = args.noise
        self.ncamera = args.ncamera
        self.skew = args.skew
        self.per_camera_movement = args.move
        self.per_camera_rotate = args.rotate
        self.per_camera_tilt = args.tilt
        seed = getattr(args, "seed", None)
        self.seed = int.from_bytes(os.urandom(8), 'little') if seed is None else int(seed) & 0xFFFFFFFFFFFFFFFF
        self.input_pc = input_pc
        self.output_pc: Optional[cwipc.cwipc_pointcloud_wrapper] = None
        self.transforms: List[np.ndarray] = []
        self.description: Optional[Dict[str, Any]] = None
        if args.descr:
            self.create_default_description()

    def load_input(self, source: str) -> None:
        self.input_pc = cwipc.cwipc_read(source, 0)

    def save_output(self, target: str) -> None:
        assert self.output_pc
        cwipc.cwipc_write(target, self.output_pc)
        if self.description:
            with open(os.path.splitext(target)[0] + ".json", "w") as fp:
                json.dump(self.description, fp, indent=2)

    def create_default_description(self) -> None:
        self.description = dict(
            noise=0.0,
            seed=self.seed,
            tiles=[dict(corr=0, move=dict(x=0, y=0, z=0), rotate=dict(x=0, y=0, z=0), transform=np.identity(4).tolist()) for _ in range(self.ncamera)],
        )

    def tile_transform(self, camnum: int, rng: np.random.Generator) -> Optional[np.ndarray]:
        """The 4x4 matrix tile `camnum` is moved by (None: it stays), with the description's entries for it"""
        tile = self.description["tiles"][camnum] if self.description else None
        transform = np.identity(4)
        changed = False
        # a rotation about the y axis
        rotation = _amount(self.per_camera_rotate, camnum)
        if rotation != 0:
            transform = rotation_matrix('y', rotation) @ transform
            changed = True
            if tile:
                tile["rotate"]["y"] += rotation
                tile["corr"] += abs(0.2 * rotation)       # (a guess: points are about 20 cm from the y axis)
        # a tilt about the x or the z axis, whichever the generator picks
        tilt = _amount(self.per_camera_tilt, camnum)
        if tilt != 0:
            axis = ('x', 'z')[int(rng.integers(0, 2))]
            transform = rotation_matrix(axis, tilt) @ transform
            changed = True
            if tile:
                tile["rotate"][axis] += tilt
                tile["corr"] += abs(1.8 * tilt)           # (a guess: a human is about 1.8 m tall)
        # a move in a random direction of the y = 0 plane
        movement = _amount(self.per_camera_movement, camnum)
        if movement > 0:
            angle = float(rng.uniform(0, 2 * np.pi))
            delta_x, delta_z = movement * float(np.cos(angle)), movement * float(np.sin(angle))
            transform[0, 3] += delta_x
            transform[2, 3] += delta_z
            changed = True
            if tile:
                tile["move"]["x"] += delta_x
                tile["move"]["z"] += delta_z
                tile["corr"] += movement
        if tile:
            tile["transform"] = transform.tolist()
        return transform if changed else None

    def run(self) -> None:
        assert self.input_pc
        rng = np.random.default_rng(self.seed)
        tiled_pc = SimulatecamsFilter(self.ncamera, hard=False, skew=self.skew, seed=self.seed).filter(self.input_pc)
        if self.verbose:
            print(f"Input point cloud tiled into {self.ncamera} cameras, {tiled_pc.count()} points in total.")
        self.transforms = []
        per_tile_pcs = []
        for camnum in range(self.ncamera):
            per_tile_pc = cwipc.cwipc_tilefilter(tiled_pc, 1 << camnum)
            if self.verbose:
                print(f"Tile {camnum} has {per_tile_pc.count()} points")
            transform = self.tile_transform(camnum, rng)
            self.transforms.append(np.identity(4) if transform is None else transform)
            if transform is not None:
                if self.verbose:
                    print(f"Moving tile {camnum} by {transform}")
                per_tile_pc = cwipc.cwipc_transform(per_tile_pc, transform)
            per_tile_pcs.append(per_tile_pc)
        joined_pc = cwipc.cwipc_join_multi(per_tile_pcs)
        if self.noise > 0:
            if self.verbose:
                print(f"Adding noise of {self.noise} meters to the point cloud")
            if self.description is not None:
                self.description["noise"] = self.noise
            joined_pc = NoiseFilter(self.noise, seed=self.seed).filter(joined_pc)
        self.output_pc = joined_pc


def build_parser() -> argparse.ArgumentParser:
    assert __doc__ is not None
    parser = argparse.ArgumentParser(description=__doc__.strip(), formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("input", help="Input point cloud .ply file")
    parser.add_argument("output", help="Output point cloud .ply file")
    parser.add_argument("--ncamera", type=int, metavar="NUM", default=1, help="Number of cameras to simulate")
    parser.add_argument("--skew", type=float, metavar="FACTOR", default=1, help="Skew point camera distribution towards the closest one by this factor")
    parser.add_argument("--move", type=float, action="append", metavar="D", help="Distance to move a tile (in meters) in the Y=0 plane, random XZ angle. Repeat for each tile.")
    parser.add_argument("--rotate", type=float, action="append", metavar="RAD", help="Angle to rotate a tile (in radians) around the Y axis. Repeat for each tile.")
    parser.add_argument("--tilt", type=float, action="append", metavar="RAD", help="Angle to rotate a tile (in radians) around the X or Z axis. Repeat for each tile.")
    parser.add_argument("--noise", type=float, metavar="DIST", default=0.0, help="Add noise to each point (in meters)")
    parser.add_argument("--descr", action="store_true", help="Also store description of modifications as a JSON file")
    parser.add_argument("--verbose", action="store_true", help="Verbose output")
    parser.add_argument("--seed", type=int, metavar="SEED", default=None, help="Seed of every random choice (default: a fresh one, stored in the description)")
    return parser


def main() -> None:
    args = build_parser().parse_args()
    creator = AnalysisTestCreator(args)
    creator.load_input(args.input)
    creator.run()
    creator.save_output(args.output)


if __name__ == '__main__':
    main()
