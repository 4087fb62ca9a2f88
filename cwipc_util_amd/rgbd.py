"""The RGB-D source end: a capture box sends one depth image and one colour image per camera, and cwipc_hip_from_rgbd turns a frame
of them into a tiled, device-resident cloud on the GPU (include/cwipc_util_amd/hip_ext.h has the contract; the per-point filters are
those every camera plug-in of the reference applies, reference include/cwipc_util/internal/capturers.hpp:208-275).

`RgbdCamera` and `RgbdFilter` describe the cameras and the filters; `RgbdSource` is the grabber: it is fed frames, hands out clouds,
attaches the images as metadata when asked (request_metadata("rgb" / "depth")), and answers the two auxiliary operations the
registration tooling asks a grabber for, "map2d3d" and "mapcolordepth", with the struct layouts of the reference
(python/cwipc/registration/multicoarse.py:592-612).

`RgbdSensor`, `RgbdPrep`, `RgbdRig` and `RgbdRigSource` are the same for RAW sensor pairs (cwipc_hip_rgbd_rig_grab): a depth image that
is eroded first, a colour image of another size from a second sensor beside the depth sensor, both behind rational-model lenses.  The
rig holds what is constant per camera; the images it attaches are the depth image the cloud was made from and the colour image
registered onto the depth grid, so the registration tooling works on them as it does on aligned ones.  `RgbdOcclusion` asks a grab
to leave out the points the colour sensor cannot see (cwipc_hip_rgbd_rig_grab_occluded) instead of giving them a foreground colour;
`RgbdDepthFilter` asks it to smooth the depth images first, along their lines and over time (cwipc_hip_rgbd_rig_grab_filtered), the
rig keeping the temporal filter's state.  `RgbdRig(sensors, decimation=k)` decimates the depth images on the GPU before any of that:
the rig takes full-size frames and works on the grid of its `grid_sensors` from there on; `RgbdHoleFill` asks a grab to fill the
holes of the depth images in front of the erosion (cwipc_hip_rgbd_rig_grab_filled)."""
from __future__ import annotations

import struct
from dataclasses import dataclass, field, replace
from typing import Any, Callable, Dict, Iterable, Iterator, List, Optional, Sequence, Tuple, Union

import numpy

from . import util
from .abstract import cwipc_activesource_abstract, cwipc_tileinfo_dict

__all__ = ["RgbdCamera", "RgbdFilter", "RgbdSource", "Frame", "from_rgbd", "RgbdSensor", "RgbdPrep", "RgbdOcclusion", "RgbdDepthFilter", "RgbdHoleFill", "RgbdRig",
           "RgbdRigSource"]

#: one frame: per camera its (depth uint16[H, W], colour uint8[H, W, bpp]) images, the colour image aligned to the depth image
Frame = Sequence[Tuple[numpy.ndarray, numpy.ndarray]]


def _identity() -> numpy.ndarray:
    return numpy.identity(4, dtype=numpy.float64)


@dataclass
class RgbdCamera:
    """Image size, intrinsics, metres per depth unit, camera -> world matrix (4x4, float64), tile number, serial number and the colour
    format (bpp 3: R, G, B bytes; 4: B, G, R, A bytes) of one camera."""
    width: int
    height: int
    fx: float
    fy: float
    cx: float
    cy: float
    depth_scale: float = 0.001
    trafo: numpy.ndarray = field(default_factory=_identity)
    tile: int = 1
    serial: str = ""
    bpp: int = 3

    def as_struct(self, depth: Optional[numpy.ndarray] = None, colour: Optional[numpy.ndarray] = None) -> util.cwipc_hip_rgbd_camera:
        """The camera as the C structure, pointing at the two images (none: only good for the mappings).  The structure keeps the
        arrays it points at alive."""
        m = numpy.ascontiguousarray(numpy.asarray(self.trafo, dtype=numpy.float64))
        if m.shape != (4, 4):
            raise ValueError("RgbdCamera: trafo must be a 4x4 matrix")
        if not 0 <= int(self.tile) <= 255:
            raise ValueError("RgbdCamera: tile must be between 0 and 255")
        rv = util.cwipc_hip_rgbd_camera()
        rv.width, rv.height, rv.bpp, rv.tile = int(self.width), int(self.height), int(self.bpp), int(self.tile)
        rv.fx, rv.fy, rv.cx, rv.cy, rv.depth_scale = float(self.fx), float(self.fy), float(self.cx), float(self.cy), float(self.depth_scale)
        rv.trafo[:] = m.reshape(16).tolist()
        rv.serial = self.serial.encode('utf8')
        if depth is not None or colour is not None:
            if depth is None or colour is None:
                raise ValueError("RgbdCamera: a depth and a colour image, or neither")
            if depth.dtype != numpy.uint16 or depth.shape != (rv.height, rv.width) or not depth.flags['C_CONTIGUOUS']:
                raise ValueError("RgbdCamera: depth must be a contiguous uint16[height, width] array")
            if colour.dtype != numpy.uint8 or colour.shape != (rv.height, rv.width, rv.bpp) or not colour.flags['C_CONTIGUOUS']:
                raise ValueError("RgbdCamera: colour must be a contiguous uint8[height, width, bpp] array")
            rv.depth, rv.colour = depth.ctypes.data, colour.ctypes.data
            rv._images = (depth, colour)
        return rv


@dataclass
class RgbdFilter:
    """The per-point filters, in the order they run; the defaults are "off".  threshold_near / threshold_far: the depth range in metres
    along the camera's axis (off when far <= near); height_min / height_max: the world y range (off when equal); radius: the distance
    from the world's y axis (off when <= 0); greenscreen: drop green points."""
    threshold_near: float = 0.0
    threshold_far: float = 0.0
    height_min: float = 0.0
    height_max: float = 0.0
    radius: float = 0.0
    greenscreen: bool = False

    def as_struct(self) -> util.cwipc_hip_rgbd_filter:
        return util.cwipc_hip_rgbd_filter(float(self.threshold_near), float(self.threshold_far), float(self.height_min), float(self.height_max),
                                          float(self.radius), 1 if self.greenscreen else 0)


def from_rgbd(cameras: Sequence[RgbdCamera], frame: Frame, filter: Optional[RgbdFilter] = None, timestamp: int = 0, cellsize: float = 0.0,
              attach_flags: int = 0) -> util.cwipc_pointcloud_wrapper:
    """cwipc_hip_from_rgbd on dataclasses and arrays."""
    if len(cameras) != len(frame):
        raise ValueError("from_rgbd: one (depth, colour) pair per camera")
    structs = [cam.as_struct(depth, colour) for cam, (depth, colour) in zip(cameras, frame)]
    return util.cwipc_hip_from_rgbd(structs, filter.as_struct() if filter is not None else None, timestamp, cellsize, attach_flags)


class RgbdSource(cwipc_activesource_abstract):
    """A grabber over frames of camera images.  `frames`: an iterable of frames, or a callable that returns the next frame (None: the
    end).  Cloud i gets the timestamp first_timestamp + i."""

    def __init__(self, cameras: Sequence[RgbdCamera], frames: Union[Iterable[Frame], Callable[[], Optional[Frame]]], filter: Optional[RgbdFilter] = None,
                 cellsize: float = 0.0, first_timestamp: int = 0) -> None:
        self.cameras: List[RgbdCamera] = list(cameras)
        if not self.cameras:
            raise ValueError("RgbdSource: no cameras")
        self.filter = filter
        self.cellsize = cellsize
        self._next: Callable[[], Optional[Frame]]
        if callable(frames):
            self._next = frames
        else:
            it: Iterator[Frame] = iter(frames)
            self._next = lambda: next(it, None)
        self._pending: Optional[Frame] = None
        self._eof = False
        self._count = 0
        self._first_timestamp = int(first_timestamp)
        self._requested: set = set()
        self._mapping_structs: Dict[int, util.cwipc_hip_rgbd_camera] = {}

    # ---- cwipc_source_abstract ----
    def free(self) -> None:
        self._eof = True
        self._pending = None

    def eof(self) -> bool:
        return self._eof and self._pending is None

    def available(self, wait: bool) -> bool:
        if self._pending is None and not self._eof:
            self._pending = self._next()
            if self._pending is None:
                self._eof = True
        return self._pending is not None

    def get(self) -> Optional[util.cwipc_pointcloud_wrapper]:
        if not self.available(True):
            return None
        frame, self._pending = self._pending, None
        flags = (util.CWIPC_HIP_RGBD_ATTACH_RGB if "rgb" in self._requested else 0) | (util.CWIPC_HIP_RGBD_ATTACH_DEPTH if "depth" in self._requested else 0)
        assert frame is not None
        pc = from_rgbd(self.cameras, frame, self.filter, self._first_timestamp + self._count, self.cellsize, flags)
        self._count += 1
        return pc

    def statistics(self) -> None:
        print(f"RgbdSource: {self._count} frames")

    # ---- cwipc_activesource_abstract ----
    def start(self) -> bool:
        return True

    def stop(self) -> None:
        pass

    def reload_config(self, config: Union[str, bytes, None]) -> Any:
        return False   # (cameraconfig.json is not read: the cameras are given to the constructor)

    def get_config(self) -> bytes:
        return b""

    def seek(self, timestamp: int) -> bool:
        return False

    def maxtile(self) -> int:
        """The reference's numbering: tile 0 is every camera together, tile i + 1 is camera i."""
        return len(self.cameras) + 1

    def get_tileinfo_dict(self, tilenum: int) -> cwipc_tileinfo_dict:
        if tilenum == 0:
            mask = 0
            for cam in self.cameras:
                mask |= cam.tile
            return {"normal": {"x": 0.0, "y": 0.0, "z": 0.0}, "cameraName": None, "ncamera": len(self.cameras), "cameraMask": mask}
        cam = self.cameras[tilenum - 1]
        # the camera looks along +z: the tile's normal points back at it, the world direction of the camera's -z axis
        m = numpy.asarray(cam.trafo, dtype=numpy.float64)
        return {"normal": {"x": float(-m[0, 2]), "y": float(-m[1, 2]), "z": float(-m[2, 2])}, "cameraName": cam.serial.encode('utf8'), "ncamera": 1,
                "cameraMask": cam.tile}

    def request_metadata(self, name: str) -> None:
        self._requested.add(name)

    def is_metadata_requested(self, name: str) -> bool:
        return name in self._requested

    def serial_dict(self) -> Dict[int, str]:
        """tile number -> serial number, what MultiCameraCoarse.set_serial_dict takes."""
        return {cam.tile: cam.serial for cam in self.cameras}

    def _camera_struct(self, tilenum: int) -> Optional[util.cwipc_hip_rgbd_camera]:
        if tilenum not in self._mapping_structs:
            for cam in self.cameras:
                if cam.tile == tilenum:
                    self._mapping_structs[tilenum] = cam.as_struct()
                    break
            else:
                return None
        return self._mapping_structs[tilenum]

    def auxiliary_operation(self, op: str, inbuf: bytes, outbuf: bytearray) -> bool:
        """"map2d3d": "ffff" (tile, u, v, depth in depth units) -> "fff" (the world point); "mapcolordepth": "iii" (tile, u, v of the
        colour image) -> "ii" (u, v of the depth image).  False for another operation, a buffer of the wrong size, an unknown tile, and
        where the library says false (no depth; outside the image)."""
        if op == "map2d3d":
            if len(inbuf) != 16 or len(outbuf) != 12:
                return False
            tile, u, v, d = struct.unpack("ffff", inbuf)
            cam = self._camera_struct(int(tile)) if tile == int(tile) else None
            point = util.cwipc_hip_rgbd_map2d3d(cam, int(u), int(v), int(d)) if cam is not None else None
            if point is None:
                return False
            outbuf[:] = struct.pack("fff", *point)
            return True
        if op == "mapcolordepth":
            if len(inbuf) != 12 or len(outbuf) != 8:
                return False
            tile, u, v = struct.unpack("iii", inbuf)
            cam = self._camera_struct(tile)
            pixel = util.cwipc_hip_rgbd_mapcolordepth(cam, u, v) if cam is not None else None
            if pixel is None:
                return False
            outbuf[:] = struct.pack("ii", *pixel)
            return True
        return False


def _zeros8() -> Tuple[float, ...]:
    return (0.0,) * 8


@dataclass
class RgbdSensor:
    """One camera of a raw rig.  The depth side: image size, intrinsics, the eight lens coefficients k1 k2 p1 p2 k3 k4 k5 k6 (OpenCV's
    rational model; all zero: pinhole), metres per depth unit.  The colour side: its own size, bpp (3: R, G, B bytes; 4: B, G, R, A
    bytes), intrinsics and coefficients.  depth_to_colour: depth-camera -> colour-camera coordinates, trafo: camera -> world (4x4,
    float64).  Tile number and serial number."""
    width: int
    height: int
    fx: float
    fy: float
    cx: float
    cy: float
    colour_width: int
    colour_height: int
    colour_fx: float
    colour_fy: float
    colour_cx: float
    colour_cy: float
    coeffs: Sequence[float] = field(default_factory=_zeros8)
    colour_coeffs: Sequence[float] = field(default_factory=_zeros8)
    depth_to_colour: numpy.ndarray = field(default_factory=_identity)
    depth_scale: float = 0.001
    trafo: numpy.ndarray = field(default_factory=_identity)
    tile: int = 1
    serial: str = ""
    bpp: int = 3

    def as_struct(self) -> util.cwipc_hip_rgbd_sensor:
        m = numpy.ascontiguousarray(numpy.asarray(self.trafo, dtype=numpy.float64))
        d2c = numpy.ascontiguousarray(numpy.asarray(self.depth_to_colour, dtype=numpy.float64))
        if m.shape != (4, 4) or d2c.shape != (4, 4):
            raise ValueError("RgbdSensor: trafo and depth_to_colour must be 4x4 matrices")
        if len(self.coeffs) != 8 or len(self.colour_coeffs) != 8:
            raise ValueError("RgbdSensor: eight lens coefficients (k1 k2 p1 p2 k3 k4 k5 k6)")
        if not 0 <= int(self.tile) <= 255:
            raise ValueError("RgbdSensor: tile must be between 0 and 255")
        rv = util.cwipc_hip_rgbd_sensor()
        rv.width, rv.height, rv.tile = int(self.width), int(self.height), int(self.tile)
        rv.fx, rv.fy, rv.cx, rv.cy, rv.depth_scale = float(self.fx), float(self.fy), float(self.cx), float(self.cy), float(self.depth_scale)
        rv.coeffs[:] = [float(c) for c in self.coeffs]
        rv.colour_width, rv.colour_height, rv.colour_bpp = int(self.colour_width), int(self.colour_height), int(self.bpp)
        rv.colour_fx, rv.colour_fy, rv.colour_cx, rv.colour_cy = float(self.colour_fx), float(self.colour_fy), float(self.colour_cx), float(self.colour_cy)
        rv.colour_coeffs[:] = [float(c) for c in self.colour_coeffs]
        rv.depth_to_colour[:] = d2c.reshape(16).tolist()
        rv.trafo[:] = m.reshape(16).tolist()
        rv.serial = self.serial.encode('utf8')
        return rv


@dataclass
class RgbdPrep:
    """What is done to the raw depth images before anything else: box erosion of the validity mask by depth_x_erosion pixels to either
    side and depth_y_erosion up and down (0 .. 32, 0: off), which takes away the rim of a subject where background colours leak."""
    depth_x_erosion: int = 0
    depth_y_erosion: int = 0

    def as_struct(self) -> util.cwipc_hip_rgbd_prep:
        return util.cwipc_hip_rgbd_prep(int(self.depth_x_erosion), int(self.depth_y_erosion))


@dataclass
class RgbdOcclusion:
    """The occlusion test between a sensor's depth and colour camera.  Every depth sample is drawn into a z-buffer of the colour grid
    as a square of (2 splat + 1)^2 colour pixels (splat 0 .. 8); a sample is dropped when that buffer holds, at its own colour pixel,
    something more than `margin` metres nearer.  splat closes the gaps between the samples of a foreground surface where the colour
    grid is finer than the depth grid: at least ceil(max(colour_fx / fx, colour_fy / fy)) - 1.  margin keeps a slanted surface from
    hiding itself: the depth it gains over splat colour pixels, plus the depth noise."""
    splat: int = 1
    margin: float = 0.02

    def as_struct(self) -> util.cwipc_hip_rgbd_occlusion:
        return util.cwipc_hip_rgbd_occlusion(int(self.splat), float(self.margin))


@dataclass
class RgbdDepthFilter:
    """The depth post-processing a depth camera's vendor ships, on the GPU in front of everything else.  Spatial: spatial_magnitude
    iterations (0 .. 5, 0: off) of an edge-preserving smoother along rows, then columns: a pixel is blended with the running value of
    its line by spatial_alpha (0 < alpha <= 1; 1: no smoothing) when they differ by less than spatial_delta depth units.  Temporal:
    the same blend with the pixel's own running value of the earlier grabs, which the rig keeps; a pixel that has lost its depth takes
    the running value while temporal_persistency (0 .. 8, 0: never, 8: always) says its last eight grabs allow it."""
    spatial_magnitude: int = 2
    spatial_alpha: float = 0.5
    spatial_delta: float = 20.0
    temporal: bool = True
    temporal_alpha: float = 0.4
    temporal_delta: float = 20.0
    temporal_persistency: int = 3

    def as_struct(self) -> util.cwipc_hip_rgbd_depthfilter:
        return util.cwipc_hip_rgbd_depthfilter(int(self.spatial_magnitude), float(self.spatial_alpha), float(self.spatial_delta), int(bool(self.temporal)),
                                               float(self.temporal_alpha), float(self.temporal_delta), int(self.temporal_persistency))


@dataclass
class RgbdHoleFill:
    """Hole filling of the depth images, after the depth filters and in front of the erosion.  mode 1: a pixel without depth takes the
    nearest depth to its left in its row; 2: the farthest, 3: the nearest depth among its up to eight neighbours, as they were before
    the stage (nothing propagates); 0: off.  A pixel that has depth is never changed."""
    mode: int = 1

    def as_struct(self) -> util.cwipc_hip_rgbd_holefill:
        return util.cwipc_hip_rgbd_holefill(int(self.mode))


class RgbdRig:
    """cwipc_hip_rgbd_rig_* on dataclasses and arrays: what is constant per camera, made once.  A context manager; free() gives the
    device memory back.  decimation k (1 .. 8): the rig is handed full-size frames -- depth images of the size its `sensors` say --
    and decimates them by k on the GPU first; everything else (the attached images, history, ray_table, map2d3d, mapcolordepth)
    is on the decimated grid, whose sensors `grid_sensors` holds."""

    def __init__(self, sensors: Sequence[RgbdSensor], decimation: int = 1) -> None:
        self.sensors: List[RgbdSensor] = list(sensors)
        self.decimation = int(decimation)
        structs = [s.as_struct() for s in self.sensors]
        self._rig: Optional[int] = (util.cwipc_hip_rgbd_rig_create(structs) if self.decimation == 1
                                    else util.cwipc_hip_rgbd_rig_create_decimated(structs, self.decimation))
        self.grid_sensors: List[RgbdSensor] = []
        for i, s in enumerate(self.sensors):
            g = util.cwipc_hip_rgbd_rig_grid_sensor(self._rig, i)
            self.grid_sensors.append(replace(s, width=g.width, height=g.height, fx=g.fx, fy=g.fy, cx=g.cx, cy=g.cy))

    def __enter__(self) -> "RgbdRig":
        return self

    def __exit__(self, *exc: Any) -> None:
        self.free()

    def __del__(self) -> None:
        try:
            self.free()
        except Exception:   # (interpreter shutdown: the library may be gone already)
            pass

    def free(self) -> None:
        if getattr(self, "_rig", None):
            util.cwipc_hip_rgbd_rig_free(self._rig)
        self._rig = None

    def _handle(self) -> int:
        if not self._rig:
            raise util.CwipcError("RgbdRig: used after free()")
        return self._rig

    def grab(self, frame: Frame, filter: Optional[RgbdFilter] = None, prep: Optional[RgbdPrep] = None, timestamp: int = 0, cellsize: float = 0.0,
             attach_flags: int = 0, occlusion: Optional[RgbdOcclusion] = None, depthfilter: Optional[RgbdDepthFilter] = None,
             holefill: Optional[RgbdHoleFill] = None) -> util.cwipc_pointcloud_wrapper:
        """One cloud from one frame: per sensor its (depth uint16[H, W], colour uint8[Hc, Wc, bpp]) images, the depth image FULL-SIZE
        also on a decimated rig.  occlusion: leave out the points the colour sensor cannot see (None: cwipc_hip_rgbd_rig_grab as it
        is).  depthfilter: smooth the depth images first (None: the two other entries as they are).  holefill: fill the depth
        images' holes after that (None: the three other entries as they are)."""
        if len(frame) != len(self.sensors):
            raise ValueError("RgbdRig: one (depth, colour) pair per sensor")
        structs = []
        for s, (depth, colour) in zip(self.sensors, frame):
            if depth.dtype != numpy.uint16 or depth.shape != (s.height, s.width) or not depth.flags['C_CONTIGUOUS']:
                raise ValueError("RgbdRig: depth must be a contiguous uint16[height, width] array")
            if colour.dtype != numpy.uint8 or colour.shape != (s.colour_height, s.colour_width, s.bpp) or not colour.flags['C_CONTIGUOUS']:
                raise ValueError("RgbdRig: colour must be a contiguous uint8[colour_height, colour_width, bpp] array")
            structs.append(util.cwipc_hip_rgbd_frame(depth.ctypes.data, colour.ctypes.data))
        if holefill is not None:
            return util.cwipc_hip_rgbd_rig_grab_filled(self._handle(), structs, holefill.as_struct(), depthfilter.as_struct() if depthfilter is not None else None,
                                                       prep.as_struct() if prep is not None else None, occlusion.as_struct() if occlusion is not None else None,
                                                       filter.as_struct() if filter is not None else None, timestamp, cellsize, attach_flags)
        if depthfilter is not None:
            return util.cwipc_hip_rgbd_rig_grab_filtered(self._handle(), structs, depthfilter.as_struct(), prep.as_struct() if prep is not None else None,
                                                         occlusion.as_struct() if occlusion is not None else None,
                                                         filter.as_struct() if filter is not None else None, timestamp, cellsize, attach_flags)
        if occlusion is not None:
            return util.cwipc_hip_rgbd_rig_grab_occluded(self._handle(), structs, prep.as_struct() if prep is not None else None, occlusion.as_struct(),
                                                         filter.as_struct() if filter is not None else None, timestamp, cellsize, attach_flags)
        return util.cwipc_hip_rgbd_rig_grab(self._handle(), structs, prep.as_struct() if prep is not None else None,
                                            filter.as_struct() if filter is not None else None, timestamp, cellsize, attach_flags)

    def reset_history(self) -> None:
        """Make the temporal filter's state empty again: the next grab is a new rig's first."""
        util.cwipc_hip_rgbd_rig_reset_history(self._handle())

    def history(self, i: int) -> Tuple[numpy.ndarray, numpy.ndarray]:
        """Sensor i's temporal-filter state: (running values float64[height, width], history bytes uint8[height, width]), on the
        rig's grid."""
        if not 0 <= i < len(self.sensors):
            raise IndexError("RgbdRig: no such sensor")
        return util.cwipc_hip_rgbd_rig_history(self._handle(), i, self.grid_sensors[i].width, self.grid_sensors[i].height)

    def ray_table(self, i: int) -> numpy.ndarray:
        """Sensor i's ray table, float64[height, width, 2]: the undistorted normalised (x, y) of every depth pixel of the rig's grid,
        NaN where the lens model has none."""
        if not 0 <= i < len(self.sensors):
            raise IndexError("RgbdRig: no such sensor")
        return util.cwipc_hip_rgbd_rig_ray_table(self._handle(), i, self.grid_sensors[i].width, self.grid_sensors[i].height)

    def map2d3d(self, i: int, u: int, v: int, d: int) -> Optional[Tuple[float, float, float]]:
        return util.cwipc_hip_rgbd_rig_map2d3d(self._handle(), i, u, v, d)

    def mapcolordepth(self, i: int, u: int, v: int) -> Optional[Tuple[int, int]]:
        return util.cwipc_hip_rgbd_rig_mapcolordepth(self._handle(), i, u, v)


class RgbdRigSource(RgbdSource):
    """RgbdSource for raw sensor pairs: the same surface -- get, request_metadata, auxiliary_operation("map2d3d" / "mapcolordepth"),
    serial_dict -- over an RgbdRig, which it makes and frees.  The attached "rgb." image lies on the depth grid, so both mappings
    take depth-grid coordinates: those of the decimated grid when decimation > 1, which is also the size of the attached images."""

    def __init__(self, sensors: Sequence[RgbdSensor], frames: Union[Iterable[Frame], Callable[[], Optional[Frame]]], filter: Optional[RgbdFilter] = None,
                 prep: Optional[RgbdPrep] = None, cellsize: float = 0.0, first_timestamp: int = 0, occlusion: Optional[RgbdOcclusion] = None,
                 depthfilter: Optional[RgbdDepthFilter] = None, decimation: int = 1, holefill: Optional[RgbdHoleFill] = None) -> None:
        super().__init__(sensors, frames, filter, cellsize, first_timestamp)   # type: ignore[arg-type]  # (tile, serial, trafo: all it reads)
        self.prep = prep
        self.occlusion = occlusion
        self.depthfilter = depthfilter
        self.holefill = holefill
        self.rig = RgbdRig(sensors, decimation)

    def free(self) -> None:
        super().free()
        self.rig.free()

    def get(self) -> Optional[util.cwipc_pointcloud_wrapper]:
        if not self.available(True):
            return None
        frame, self._pending = self._pending, None
        flags = (util.CWIPC_HIP_RGBD_ATTACH_RGB if "rgb" in self._requested else 0) | (util.CWIPC_HIP_RGBD_ATTACH_DEPTH if "depth" in self._requested else 0)
        assert frame is not None
        pc = self.rig.grab(frame, self.filter, self.prep, self._first_timestamp + self._count, self.cellsize, flags, self.occlusion, self.depthfilter,
                           self.holefill)
        self._count += 1
        return pc

    def statistics(self) -> None:
        print(f"RgbdRigSource: {self._count} frames")

    def _sensor_index(self, tilenum: int) -> Optional[int]:
        for i, s in enumerate(self.cameras):
            if s.tile == tilenum:
                return i
        return None

    def auxiliary_operation(self, op: str, inbuf: bytes, outbuf: bytearray) -> bool:
        """As RgbdSource.auxiliary_operation, with (u, v) on the depth grid for both operations."""
        if op == "map2d3d":
            if len(inbuf) != 16 or len(outbuf) != 12:
                return False
            tile, u, v, d = struct.unpack("ffff", inbuf)
            i = self._sensor_index(int(tile)) if tile == int(tile) else None
            point = self.rig.map2d3d(i, int(u), int(v), int(d)) if i is not None else None
            if point is None:
                return False
            outbuf[:] = struct.pack("fff", *point)
            return True
        if op == "mapcolordepth":
            if len(inbuf) != 12 or len(outbuf) != 8:
                return False
            tile, u, v = struct.unpack("iii", inbuf)
            i = self._sensor_index(tile)
            pixel = self.rig.mapcolordepth(i, u, v) if i is not None else None
            if pixel is None:
                return False
            outbuf[:] = struct.pack("ii", *pixel)
            return True
        return False
