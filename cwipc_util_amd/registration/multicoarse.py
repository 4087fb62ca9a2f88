"""Coarse registration of a tiled capture from markers (reference python/cwipc/registration/multicoarse.py): the step that takes
cameras from "each in its own coordinates" to "roughly aligned", after which the fine algorithms of multicamera.py take over.

`MultiCameraCoarse` is the reference's loop on this project's types: every camera's markers are found once; a camera that sees a
marker whose position is known gets the rigid transformation that puts its four corners there; a registered camera that sees a
marker nobody knew yet hands its position on, and the loop passes over the cameras again for as long as a pass learns something.
The identity stands for "not registered".  No open3d cloud is kept per camera: a camera's tile is taken from the cloud with
cwipc_tilefilter when it is needed.

`MultiCameraCoarseAruco` finds the markers the way the reference does, without the reference's windows: the camera's tile is
rendered on the GPU through a pinhole view (render.py; by default the view from the origin, the reference's `from000`, which is the
physical camera's view of a tile that has not been registered), a detector finds marker corners in the colour image, and the depth
image takes them back to 3D.  The detector is a plug-in (`set_marker_detector`).  With a marker dictionary instead
(`set_marker_dictionary`, markers.py) the GPU finds the markers in the image where the renderer left it, and only the corners and their
depths come back (cwipc_hip_render_detect_markers).  With neither, cv2.aruco is asked for, as in the reference.

`MultiCameraCoarseArucoRgb` finds them in the cameras' own images instead of in a rendering: the colour and depth image a grabber
attached to the cloud's metadata (rgbd.RgbdSource does, when asked), by the camera's serial number; every corner goes through the
grabber's auxiliary operations "mapcolordepth" and "map2d3d", its depth being the mean of the 7 x 7 depths around it.  It is the class
the reference's cwipc_register picks when a capturer is present.  A camera without images falls back to the rendered path.

Out of scope, and not here: the interactive `MultiCameraCoarseColorTarget` (a person picks the corners in a window).
"""
import struct
from typing import Any, Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from ..util import cwipc_pointcloud_wrapper, cwipc_tilefilter, cwipc_join, cwipc_transform, get_tiles_used
from .abstract import MulticamAlignmentAlgorithm, RegistrationTransformation
from ..util import cwipc_hip_render_detect_markers, cwipc_hip_marker_params
from .render import PinholeView, default_view, render_pointcloud, deproject, deproject_depth, mean_depth
from .markers import MarkerDictionary, detect_markers
from .util import transformation_identity

__all__ = ['MarkerPosition', 'MarkerPositions', 'MarkerDetector', 'MultiCameraCoarse', 'MultiCameraCoarseAruco', 'MultiCameraCoarseArucoRgb']

#: the outline of a marker in 3D; marker id -> outline
MarkerPosition = List[Tuple[float, float, float]]
MarkerPositions = Dict[int, MarkerPosition]
#: rgb image (uint8[H, W, 3]) -> (per marker its corners as (u, v) pairs, the markers' ids)
MarkerDetector = Callable[[np.ndarray], Tuple[Sequence[Sequence[Sequence[float]]], Sequence[int]]]


class MultiCameraCoarse(MulticamAlignmentAlgorithm):
    """Align multiple cameras from markers whose corners are known in 3D.  Subclasses say how a camera's markers are found."""

    def __init__(self) -> None:
        MulticamAlignmentAlgorithm.__init__(self)
        self.debug = False
        self.original_pointcloud: Optional[cwipc_pointcloud_wrapper] = None
        self.per_camera_tilenum: List[int] = []
        self.serial_for_tilenum: Dict[int, str] = {}
        self.transformations: List[RegistrationTransformation] = []
        self.known_marker_positions: MarkerPositions = dict()
        self.markers: List[MarkerPositions] = []
        self.verbose = False

    def set_tiled_pointcloud(self, pc: cwipc_pointcloud_wrapper) -> None:
        """The cloud whose tiles are the cameras."""
        assert self.original_pointcloud is None
        self.original_pointcloud = pc

    def get_pointcloud_for_tilemask(self, tilenum: int) -> cwipc_pointcloud_wrapper:
        """The points of one tile number."""
        assert self.original_pointcloud
        return cwipc_tilefilter(self.original_pointcloud, tilenum)

    def camera_count(self) -> int:
        count = len(self.per_camera_tilenum)
        assert count > 0   # otherwise this has been called too early
        return count

    def set_serial_dict(self, sd: Dict[int, str]) -> None:
        self.serial_for_tilenum = sd

    def tilemask_for_camera_index(self, cam_index: int) -> int:
        return self.per_camera_tilenum[cam_index]

    def camera_index_for_tilemask(self, tilenum: int) -> int:
        for i, t in enumerate(self.per_camera_tilenum):
            if t == tilenum:
                return i
        assert False, f"Tilenum {tilenum} not known"

    def _init_transformations(self) -> None:
        if self.transformations == []:
            for _ in range(self.camera_count()):
                self.transformations.append(transformation_identity())

    def set_transformation(self, tilenum: int, trafo: RegistrationTransformation) -> None:
        self._init_transformations()
        self.transformations[tilenum] = trafo

    def _get_unregistered_tiles(self) -> List[int]:
        """The camera indices that still have the identity for a transformation."""
        self._init_transformations()
        identity = transformation_identity()
        return [i for i, t in enumerate(self.transformations) if (t == identity).all()]

    def _prepare(self) -> None:
        """The camera numbering: camera i is the i-th tile number that occurs in the cloud."""
        assert self.original_pointcloud
        tilenums = get_tiles_used(self.original_pointcloud)
        if tilenums == []:
            print(f"{self.__class__.__name__}: no points in cloud. Getting tile numbers from serial numbers")
            tilenums = list(self.serial_for_tilenum.keys())
        for t in tilenums:
            self.per_camera_tilenum.append(t)
        self._init_transformations()
        assert len(tilenums) == len(self.per_camera_tilenum) == len(self.transformations)

    def run(self) -> bool:
        """True when every camera has a transformation."""
        assert self.original_pointcloud
        self._prepare()
        self._find_markers_all_tiles()
        assert self.known_marker_positions
        another_pass_wanted = True
        while another_pass_wanted:
            another_pass_wanted = False   # set again when a pass learns something that may help the next one
            if self.verbose:
                print(f"cwipc_register: coarse: attempting to register tiles {self._get_unregistered_tiles()}")
            # Every camera is looked at, not only the unregistered ones: a camera registered in the last pass may see markers
            # nobody knew about then.
            for camindex in range(len(self.per_camera_tilenum)):
                tilenum = self.tilemask_for_camera_index(camindex)
                for id, area in self.markers[camindex].items():
                    if not self._check_marker(area):
                        continue
                    if id in self.known_marker_positions:
                        this_transform = self._align_marker(camindex, self.known_marker_positions[id], area)
                        if this_transform is None:
                            continue
                        old_transform = self.transformations[camindex]
                        had_transform = not (old_transform == transformation_identity()).all()   # (from another marker, or an earlier pass)
                        if had_transform:
                            # the first one stays; the new one is only compared with it
                            delta = np.add.reduce(np.abs(this_transform - old_transform), None)
                            if self.verbose:
                                print(f"cwipc_register: coarse: camera {tilenum} cameramask {camindex}: marker {id}: new registration matrix differs {delta} from old one")
                        else:
                            if self.verbose:
                                print(f"cwipc_register: coarse: camera {tilenum} cameramask {camindex}: marker {id}: created transformation matrix")
                            self.transformations[camindex] = this_transform
                    else:
                        if self.verbose:
                            print(f"cwipc_register: coarse: camera {tilenum} cameramask {camindex}: marker {id}: unknown marker found")
                        tile_transform = self.transformations[camindex]
                        if not (tile_transform == transformation_identity()).all():
                            # a registered camera sees a marker nobody knew: its corners, taken to world coordinates, are known now
                            new_area: MarkerPosition = []
                            for cam_point in area:
                                p = tile_transform @ np.array([float(cam_point[0]), float(cam_point[1]), float(cam_point[2]), 1])
                                new_area.append((float(p[0]), float(p[1]), float(p[2])))
                            if self.verbose:
                                print(f"cwipc_register: coarse: camera {tilenum} cameramask {camindex}: marker {id}: 3d-corners {new_area}")
                            self.known_marker_positions[id] = new_area
                            another_pass_wanted = True
        return self._get_unregistered_tiles() == []

    def _find_markers_all_tiles(self) -> None:
        self.markers = []
        for camindex in range(len(self.per_camera_tilenum)):
            markers = self._find_markers(0, camindex)
            if self.verbose:
                print(f"cwipc_register: find_markers_all_tiles: camera {camindex}: marker ids: {markers.keys()}")
                for mid, corners in markers.items():
                    for corner_idx, corner in enumerate(corners):
                        next_corner = corners[(corner_idx + 1) % len(corners)]
                        distance = np.linalg.norm(np.array(corner) - np.array(next_corner))
                        print(f"cwipc_register: find_markers_all_tiles: camera {camindex}: marker {mid}:  3D corner: {corner}, distance to next: {distance}")
            self.markers.append(markers)
        assert len(self.per_camera_tilenum) == len(self.markers)

    def _check_marker(self, marker: MarkerPosition) -> bool:
        """False if this cannot be a valid marker."""
        if len(marker) == 4:
            return True
        print(f"cwipc_register: Error: marker has {len(marker)} corners in stead of 4")
        return False

    def _find_markers(self, passnum: int, camindex: int) -> MarkerPositions:
        """All markers found in this camera's tile, by marker id, in the tile's coordinates."""
        return {}

    def _align_marker(self, camindex: int, target: MarkerPosition, dst: MarkerPosition) -> Optional[RegistrationTransformation]:
        """The rigid transformation (rotation and translation, no scaling) that takes the corners `dst`, as this camera sees them,
        as near as possible to the corners `target` in the least-squares sense, corner i onto corner i (the reference asks open3d's
        TransformationEstimationPointToPoint): with the centroids removed, the rotation is V diag(1, 1, det(V U^T)) U^T of the
        singular value decomposition U S V^T of sum dst_i target_i^T -- the determinant keeps it a rotation when the corners are
        given in a mirrored order and the best orthogonal matrix would be a reflection."""
        src = np.asarray(dst, dtype=np.float64).reshape(-1, 3)
        tgt = np.asarray(target, dtype=np.float64).reshape(-1, 3)
        if len(src) != len(tgt) or len(src) < 3 or not (np.isfinite(src).all() and np.isfinite(tgt).all()):
            return None
        src_mean, tgt_mean = src.mean(axis=0), tgt.mean(axis=0)
        u, _s, vt = np.linalg.svd((src - src_mean).T @ (tgt - tgt_mean))
        d = np.sign(np.linalg.det(vt.T @ u.T))
        rot = vt.T @ np.diag([1.0, 1.0, d if d != 0 else 1.0]) @ u.T
        transform = transformation_identity()
        transform[:3, :3] = rot
        transform[:3, 3] = tgt_mean - rot @ src_mean
        if self.verbose:
            moved = src @ rot.T + transform[:3, 3]
            rmse = float(np.sqrt(np.mean(np.sum((moved - tgt) ** 2, axis=1))))
            print(f"cwipc_register: _align_marker: camera {camindex}: rmse error={rmse}")
        return transform

    def get_result_transformations(self) -> List[RegistrationTransformation]:
        """The transformations found, by camera index; the identity for a camera without one."""
        return self.transformations

    def get_result_pointcloud_full(self) -> cwipc_pointcloud_wrapper:
        """All tiles together, each moved by its camera's matrix."""
        rv: Optional[cwipc_pointcloud_wrapper] = None
        assert len(self.transformations) == len(self.per_camera_tilenum)
        assert self.original_pointcloud
        for i in range(len(self.per_camera_tilenum)):
            partial_pc = cwipc_tilefilter(self.original_pointcloud, self.per_camera_tilenum[i])
            transformed_partial_pc = cwipc_transform(partial_pc, self.transformations[i])
            rv = transformed_partial_pc if rv is None else cwipc_join(rv, transformed_partial_pc)
        assert rv
        return rv


def _cv2_aruco_detector() -> MarkerDetector:
    """The reference's detector: cv2.aruco with the 5x5, 50 marker dictionary and default parameters (multicoarse.py:316-318, :492-527)."""
    try:
        import cv2
        import cv2.aruco
    except ImportError:
        raise RuntimeError("MultiCameraCoarseAruco: cv2.aruco is not available: a marker detector must be set with set_marker_detector(), "
                           "or a marker dictionary with set_marker_dictionary()") from None
    detector = cv2.aruco.ArucoDetector(cv2.aruco.getPredefinedDictionary(cv2.aruco.DICT_5X5_50), cv2.aruco.DetectorParameters())

    def detect(img: np.ndarray) -> Tuple[List[List[List[float]]], List[int]]:
        corners, ids, _rejected = detector.detectMarkers(img)
        rv_corners: List[List[List[float]]] = []
        rv_ids: List[int] = []
        if ids is not None:
            # (cv2 hands the ids over as a column and every marker's corners as a 1 x 4 x 2 array)
            for cur_id, area in zip(np.asarray(ids).reshape(-1), corners):
                rv_ids.append(int(cur_id))
                rv_corners.append(np.asarray(area).reshape(-1, 2).tolist())
        return rv_corners, rv_ids

    return detect


class MultiCameraCoarseAruco(MultiCameraCoarse):
    """Coarse alignment from Aruco markers: each camera's tile is rendered through a pinhole view, the markers are found in the colour
    image and their corners are taken back to 3D through the depth image."""

    def __init__(self) -> None:
        MultiCameraCoarse.__init__(self)
        # The Aruco is about 14x14cm.  Initially only the 3D position of the marker with id 0 is known.
        self.known_marker_positions = {
            0: [
                (+0.087, 0, +0.087),   # topright, red
                (-0.087, 0, +0.087),   # topleft, blue
                (-0.087, 0, -0.087),   # botleft, pink
                (+0.087, 0, -0.087),   # botright, yellow
            ]
        }
        self.point_size = 5
        self.default_view: PinholeView = default_view()
        self.per_camera_view: Dict[int, PinholeView] = {}
        self.marker_detector: Optional[MarkerDetector] = None
        self.marker_dictionary: Optional[MarkerDictionary] = None
        self.marker_params: Dict[str, int] = {}

    def set_view(self, camindex: Optional[int], view: PinholeView) -> None:
        """The view one camera's tile is rendered through, or (None) every camera's that has none of its own."""
        if camindex is None:
            self.default_view = view
        else:
            self.per_camera_view[camindex] = view

    def view_for_camera_index(self, camindex: int) -> PinholeView:
        return self.per_camera_view.get(camindex, self.default_view)

    def set_marker_detector(self, detector: Optional[MarkerDetector]) -> None:
        """detector(rgb image) -> (per marker its four (u, v) corners, the markers' ids); None: cv2.aruco."""
        self.marker_detector = detector

    def set_marker_dictionary(self, dictionary: Optional[MarkerDictionary], **params: int) -> None:
        """The markers to look for on the GPU when no detector is set (params: the fields of cwipc_hip_marker_params); None: none."""
        cwipc_hip_marker_params(**params)   # (a wrong name fails here)
        self.marker_dictionary = dictionary
        self.marker_params = dict(params)

    def _find_markers_on_device(self, camindex: int) -> MarkerPositions:
        """Render and detect in one call; the corners' depths come back with them."""
        assert self.marker_dictionary is not None
        view = self.view_for_camera_index(camindex)
        tile_pc = self.get_pointcloud_for_tilemask(self.per_camera_tilenum[camindex])
        ids, corners, corner_depth, _found = cwipc_hip_render_detect_markers(tile_pc, view.as_struct(), self.marker_dictionary.words, self.point_size,
                                                                             params=cwipc_hip_marker_params(**self.marker_params))
        rv: MarkerPositions = {}
        for id, area_2d, depths in zip(ids, corners, corner_depth):
            if self.debug:
                print(f"cwipc_register: camera {camindex}: find_markers: marker {id}: 2d-area={area_2d.tolist()}")
            corners_3d = [deproject_depth(view, int(uv[0]), int(uv[1]), d) for uv, d in zip(area_2d, depths)]
            rv[int(id)] = [c for c in corners_3d if c is not None]
        return rv

    def _find_markers(self, passnum: int, camindex: int) -> MarkerPositions:
        """Render this camera's tile, find the markers in the colour image, take their corners to 3D through the depth image.  An
        explicit detector comes first, then a dictionary (all on the GPU), then cv2.aruco."""
        if self.marker_detector is None and self.marker_dictionary is not None:
            return self._find_markers_on_device(camindex)
        detector = self.marker_detector if self.marker_detector is not None else _cv2_aruco_detector()
        view = self.view_for_camera_index(camindex)
        tile_pc = self.get_pointcloud_for_tilemask(self.per_camera_tilenum[camindex])
        rgb, depth, _index = render_pointcloud(tile_pc, view, self.point_size)
        areas_2d, ids = detector(rgb)
        rv: MarkerPositions = {}
        if ids is None:
            return rv
        for id, area_2d in zip(ids, areas_2d):
            if self.debug:
                print(f"cwipc_register: camera {camindex}: find_markers: marker {id}: 2d-area={area_2d}")
            # A corner outside the image or on the background has no 3D position: the marker then has fewer than four corners and
            # run() skips it.
            corners_3d = [deproject(view, depth, corner_2d) for corner_2d in area_2d]
            rv[int(id)] = [c for c in corners_3d if c is not None]
        return rv


class MultiCameraCoarseArucoRgb(MultiCameraCoarseAruco):
    """Coarse alignment from Aruco markers found in the cameras' own colour images (reference multicoarse.py:529-655): the images come
    from the cloud's metadata, the grabber maps a colour pixel to its depth pixel and a pixel with its depth to 3D."""

    def __init__(self) -> None:
        MultiCameraCoarseAruco.__init__(self)
        self.grabber: Any = None

    def set_grabber(self, grabber: Any) -> None:
        """The source the cloud came from: it answers auxiliary_operation("map2d3d" / "mapcolordepth") and, when it has a
        serial_dict() and no serial numbers have been set, says which serial number each tile has."""
        self.grabber = grabber
        if not self.serial_for_tilenum and hasattr(grabber, "serial_dict"):
            self.set_serial_dict(grabber.serial_dict())

    def _detect_in_image(self, rgb: np.ndarray) -> Tuple[Sequence[Sequence[Sequence[float]]], Sequence[int]]:
        """The parent's order: an explicit detector, then a dictionary (the GPU detector on the image), then cv2.aruco."""
        if self.marker_detector is not None:
            areas_2d, ids = self.marker_detector(rgb)
        elif self.marker_dictionary is not None:
            areas_2d, ids = detect_markers(rgb, self.marker_dictionary, **self.marker_params)
        else:
            areas_2d, ids = _cv2_aruco_detector()(rgb)
        return (areas_2d, ids) if ids is not None else ([], [])

    def _find_markers(self, passnum: int, camindex: int) -> MarkerPositions:
        tilenum = self.per_camera_tilenum[camindex]
        np_rgb_image, np_depth_image = self._get_rgb_depth_images(camindex)
        if np_rgb_image is None or np_depth_image is None:
            print(f"cwipc_register: camera {camindex}: Warning: RGB or Depth image not captured. Revert to the rendered image.")
            return MultiCameraCoarseAruco._find_markers(self, passnum, camindex)
        areas_2d, ids = self._detect_in_image(np_rgb_image)
        rv: MarkerPositions = {}
        if self.verbose:
            print(f"cwipc_register: camera {camindex}: _find_markers: Auruco-IDs: {ids}, 2D-Areas: {areas_2d}")
        for i in range(len(ids)):
            marker_id = int(ids[i])
            area_2d = areas_2d[i]
            assert len(area_2d) == 4
            area_3d: MarkerPosition = []
            for corner_2d_idx, corner_2d in enumerate(area_2d):
                u, v = int(corner_2d[0]), int(corner_2d[1])
                du, dv = self._map_color_to_depth(tilenum, u, v)
                d = self._get_depth_value(camindex, np_depth_image, du, dv)
                if d <= 0:
                    break   # (the marker keeps fewer than four corners: run() skips it)
                # (map2d3d wants the colour image's coordinates)
                corner_3d = self._map_2d_to_3d(tilenum, u, v, d)
                if self.verbose:
                    print(f"cwipc_register: camera {camindex}: find_markers: marker {i}, corner {corner_2d_idx}: u,v,d={(u, v, d)} 3d-point={corner_3d}")
                area_3d.append(corner_3d)
            if marker_id not in rv:
                rv[marker_id] = area_3d
            else:
                # A second marker with this id in view (one lying around, say): the one whose first corner is nearer the origin stays.
                # (One without a first corner is as far away as can be; the reference would fail on it.)
                old_area_3d = rv[marker_id]
                new_distance = float(np.linalg.norm(area_3d[0])) if area_3d else float('inf')
                old_distance = float(np.linalg.norm(old_area_3d[0])) if old_area_3d else float('inf')
                if new_distance < old_distance:
                    print(f"cwipc_register: camera {camindex}: Warning: duplicate marker {marker_id}. Use new at distance {new_distance}, old was at {old_distance}")
                    rv[marker_id] = area_3d
                else:
                    print(f"cwipc_register: camera {camindex}: Warning: duplicate marker {marker_id}. Keep old at distance {old_distance}, new was at {new_distance}")
        return rv

    def _map_2d_to_3d(self, tilenum: int, u: int, v: int, d: int) -> Tuple[float, float, float]:
        assert self.grabber
        inargs = struct.pack("ffff", float(tilenum), float(u), float(v), float(d))
        outargs = bytearray(12)
        if not self.grabber.auxiliary_operation("map2d3d", inargs, outargs):
            raise RuntimeError(f"MultiCameraCoarseArucoRgb: camera {tilenum}: map2d3d failed")
        rv_x, rv_y, rv_z = struct.unpack("fff", outargs)
        return rv_x, rv_y, rv_z

    def _map_color_to_depth(self, tilenum: int, cu: int, cv: int) -> Tuple[int, int]:
        assert self.grabber
        inargs = struct.pack("iii", tilenum, cu, cv)
        outargs = bytearray(8)
        if not self.grabber.auxiliary_operation("mapcolordepth", inargs, outargs):
            print(f"cwipc_register: Warning: camera {tilenum}: mapcolordepth failed")
            return cu, cv
        du, dv = struct.unpack("ii", outargs)
        return du, dv

    def _get_depth_value(self, camindex: int, np_depth_image: np.ndarray, x: int, y: int) -> int:
        """The depth at (x, y): the mean of the depths there are in the 7 x 7 pixels around it, 0 when there are fewer than 10."""
        return int(mean_depth(np_depth_image, x, y, 3, 10))

    def _get_rgb_depth_images(self, camindex: int) -> Tuple[Optional[np.ndarray], Optional[np.ndarray]]:
        """This camera's colour image (uint8[H, W, 3], R, G, B: what a MarkerDetector takes) and depth image (uint16[H, W]) from the
        cloud's metadata; (None, None) when the tile has no serial number or the cloud carries no images of it."""
        tilenum = self.per_camera_tilenum[camindex]
        serial = self.serial_for_tilenum.get(tilenum)
        if not serial:
            print(f"cwipc_register: camera {camindex}: get_rgb_depth_images: Unknown tilenum {tilenum}, no serial number known")
            return None, None
        assert self.original_pointcloud
        metadata = self.original_pointcloud.access_metadata()
        if not metadata or metadata.count() == 0:
            print(f"cwipc_register: camera {camindex}: get_rgb_depth_images: tilenum {tilenum}: no metadata")
            return None, None
        image_dict = metadata.get_all_images(serial)
        depth_image, bgr_image = image_dict.get("depth."), image_dict.get("rgb.")
        if depth_image is None or bgr_image is None:
            return None, None
        # (get_all_images hands colour out as B, G, R, which is what cv2 works on; this project's detectors take R, G, B)
        return np.ascontiguousarray(bgr_image[:, :, ::-1]), depth_image
