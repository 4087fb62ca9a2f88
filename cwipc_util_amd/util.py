"""ctypes wrapper around the MI355X libcwipc_util -- same surface as the reference's
``cwipc.util`` (reference python/cwipc/util.py), so pipeline code written against
``cwipc`` runs against ``cwipc_util_amd`` unchanged:

    import cwipc_util_amd as cwipc
    pc = cwipc.cwipc_synthetic().get()
    small = cwipc.cwipc_downsample(pc, 0.01)

Same names, argument meaning and error behaviour (CwipcError where the reference
raises it, wrapper objects around whatever the C call returns where it does not).
The per-point work happens in HIP kernels behind the C-ABI; this module never
computes on points itself and has no CPU fallback.  open3d is optional here (the
reference imports it unconditionally, util.py:24).
"""
from __future__ import annotations

import ctypes
import functools
import math
import os
import sys
import warnings
from typing import Any, Callable, Dict, Iterable, List, Optional, Sequence, Tuple, Union

import numpy
import numpy.typing

from .abstract import cwipc_pointcloud_abstract, cwipc_source_abstract, cwipc_activesource_abstract, cwipc_tileinfo_dict

__all__ = [
    'CWIPC_API_VERSION', 'CWIPC_POINT_PACKETHEADER_MAGIC', 'CWIPC_POINT_PACKETHEADER_MAGIC_C', 'cwipc_proxy_packet', 'cwipc_from_proxy_packet', 'CWIPC_FLAGS_BINARY', 'CwipcError',
    'CWIPC_LOG_LEVEL_NONE', 'CWIPC_LOG_LEVEL_ERROR', 'CWIPC_LOG_LEVEL_WARNING', 'CWIPC_LOG_LEVEL_TRACE', 'CWIPC_LOG_LEVEL_DEBUG',
    'cwipc_pointcloud_wrapper', 'cwipc_source_wrapper', 'cwipc_activesource_wrapper', 'cwipc_sink_wrapper', 'cwipc_metadata',
    'cwipc_point', 'cwipc_point_array', 'cwipc_point_numpy_dtype', 'cwipc_tileinfo_dict', 'cwipc_point_packetheader',
    'cwipc_util_dll_load',
    'cwipc_get_version', 'cwipc_log_configure', 'cwipc_log_default_callback', '_cwipc_log_emit', 'cwipc_dangling_allocations',
    'cwipc_read', 'cwipc_read_debugdump', 'cwipc_write', 'cwipc_write_debugdump',
    'cwipc_from_points', 'cwipc_from_packet', 'cwipc_from_numpy_array', 'cwipc_from_numpy_matrix', 'cwipc_from_o3d_pointcloud',
    'cwipc_synthetic', 'cwipc_capturer', 'cwipc_window', 'cwipc_proxy',
    'cwipc_downsample', 'cwipc_remove_outliers', 'cwipc_tilefilter', 'cwipc_tilemap', 'cwipc_colormap',
    'cwipc_join', 'cwipc_join_multi', 'cwipc_crop',
    # MI355X extensions (no reference counterpart)
    'cwipc_hip_device_count', 'cwipc_hip_set_device', 'cwipc_hip_upload', 'cwipc_hip_pinned_points', 'cwipc_hip_pin_array', 'cwipc_hip_colorize', 'cwipc_tilefilter_masked', 'cwipc_hip_device_planes',
    'cwipc_hip_profile', 'cwipc_hip_knn_mean_dist', 'cwipc_hip_from_device_aos', 'cwipc_hip_from_device_slots', 'cwipc_hip_copy_device_aos',
    'cwipc_transform', 'cwipc_offset_scale', 'cwipc_hip_flatten_y', 'get_tiles_used', 'cwipc_downsample_pertile', 'cwipc_hip_simulatecams', 'cwipc_hip_comm', 'cwipc_hip_comm_unique_id',
    'cwipc_direction_filter', 'cwipc_center', 'cwipc_hip_estimate_normals',
    'CWIPC_HIP_CLUSTER_SAME_TILE', 'cwipc_cluster_labels', 'cwipc_cluster_filter', 'cwipc_hip_cluster_link_stats', 'cwipc_hip_cluster_rank_keep',
    'CWIPC_HIP_NEIGH_SAME_TILE', 'cwipc_radius_counts', 'cwipc_radius_outlier_filter', 'cwipc_smooth', 'cwipc_hip_smooth_host',
    'cwipc_hip_nn_distance', 'cwipc_hip_gaussian_kde', 'NNJob', 'cwipc_hip_nn_distance_jobs', 'compact_job_rows',
    'cwipc_hip_correspondences', 'cwipc_hip_icp_sums', 'cwipc_hip_icp_point2point', 'cwipc_hip_icp_plane_sums', 'cwipc_hip_icp_point2plane',
    'cwipc_hip_gicp_covariances', 'cwipc_hip_icp_gicp_sums', 'cwipc_hip_icp_generalized',
    'cwipc_hip_distortion_sums', 'CWIPC_HIP_DISTORTION_NO_PLANE', 'cwipc_hip_distortion',
    'cwipc_floor_filter', 'cwipc_randomize_floor', 'cwipc_compute_tile_occupancy', 'cwipc_compute_radius', 'cwipc_limit_floor_to_radius',
    'cwipc_hip_floor_partition', 'cwipc_hip_floor_radius_stats', 'cwipc_hip_tile_counts', 'cwipc_hip_bounds',
    'CWIPC_HIP_FLOOR_KEEP_FLOOR', 'CWIPC_HIP_FLOOR_KEEP_REST', 'CWIPC_HIP_FLOOR_LIMIT_RADIUS',
    'cwipc_hip_noise', 'cwipc_hip_simulatecams_soft',
    'CWIPC_HIP_PLANE_REFINE', 'CWIPC_HIP_PLANE_KEEP_INLIERS', 'CWIPC_HIP_PLANE_KEEP_REST', 'CWIPC_HIP_PLANE_BELOW_IS_INLIER',
    'CWIPC_HIP_PLANE_SCORE_TILE', 'CWIPC_HIP_PLANE_SCORE_GRID', 'CWIPC_HIP_PLANE_SCORE_HBLOCK',
    'cwipc_hip_plane_params', 'cwipc_hip_plane_result', 'cwipc_plane_result', 'cwipc_plane_constraint',
    'cwipc_find_plane', 'cwipc_hip_plane_scores', 'cwipc_hip_plane_partition', 'cwipc_plane_filter', 'cwipc_hip_plane_level_matrix',
    'cwipc_level_to_plane', 'cwipc_find_planes', 'cwipc_hip_plane_find_host',
    'cwipc_hip_view', 'cwipc_hip_render',
    'cwipc_hip_marker_params', 'cwipc_hip_detect_markers', 'cwipc_hip_render_detect_markers', 'cwipc_hip_marker_labels',
    'cwipc_hip_rgbd_camera', 'cwipc_hip_rgbd_filter', 'CWIPC_HIP_RGBD_ATTACH_RGB', 'CWIPC_HIP_RGBD_ATTACH_DEPTH', 'cwipc_hip_from_rgbd',
    'cwipc_hip_rgbd_map2d3d', 'cwipc_hip_rgbd_mapcolordepth',
    'cwipc_hip_rgbd_sensor', 'cwipc_hip_rgbd_frame', 'cwipc_hip_rgbd_prep', 'cwipc_hip_rgbd_rig_create', 'cwipc_hip_rgbd_rig_free',
    'cwipc_hip_rgbd_rig_grab', 'cwipc_hip_rgbd_occlusion', 'cwipc_hip_rgbd_rig_grab_occluded', 'cwipc_hip_rgbd_depthfilter',
    'cwipc_hip_rgbd_rig_grab_filtered', 'cwipc_hip_rgbd_rig_create_decimated', 'cwipc_hip_rgbd_rig_decimation', 'cwipc_hip_rgbd_rig_grid_sensor',
    'cwipc_hip_rgbd_holefill', 'cwipc_hip_rgbd_rig_grab_filled', 'cwipc_hip_rgbd_rig_reset_history', 'cwipc_hip_rgbd_rig_history', 'cwipc_hip_rgbd_rig_ray_table', 'cwipc_hip_rgbd_rig_map2d3d', 'cwipc_hip_rgbd_rig_mapcolordepth',
    # the octree codec (cwipc_util_amd.codec has the names the reference's callers use)
    'cwipc_hip_encoder_params', 'cwipc_hip_codec_info', 'cwipc_hip_codec_packet_info',
    'cwipc_hip_new_encoder', 'cwipc_hip_encoder_free', 'cwipc_hip_encoder_feed', 'cwipc_hip_encoder_available', 'cwipc_hip_encoder_get_encoded_size',
    'cwipc_hip_encoder_copy_data', 'cwipc_hip_encoder_at_gop_boundary', 'cwipc_hip_encoder_eof', 'cwipc_hip_encoder_close',
    'cwipc_hip_new_encodergroup', 'cwipc_hip_encodergroup_addencoder', 'cwipc_hip_encodergroup_feed', 'cwipc_hip_encodergroup_close', 'cwipc_hip_encodergroup_free',
    'cwipc_hip_new_decoder', 'cwipc_hip_decoder_feed', 'cwipc_hip_decoder_available', 'cwipc_hip_decoder_get', 'cwipc_hip_decoder_eof', 'cwipc_hip_decoder_close',
    'cwipc_hip_decoder_free',
    'cwipc_hip_encoder_set_entropy', 'cwipc_hip_codec_entropy_directory', 'cwipc_hip_codec_entropy_pack', 'cwipc_hip_codec_entropy_unpack',
    'cwipc_hip_codec_entropy_info',
    'cwipc_hip_codec_inter_directory', 'cwipc_hip_codec_inter_pack', 'cwipc_hip_codec_inter_unpack', 'cwipc_hip_codec_inter_info',
    'cwipc_hip_encoder_set_colour_transform', 'cwipc_hip_codec_transform_directory', 'cwipc_hip_codec_transform_pack', 'cwipc_hip_codec_transform_unpack',
    'cwipc_hip_codec_transform_info',
    'cwipc_hip_decoder_set_max_octree_bits', 'cwipc_hip_codec_lod',
]

# reference util.py:86, 346, 348
CWIPC_API_VERSION = 0x20260129
CWIPC_POINT_PACKETHEADER_MAGIC = 0x20210208
CWIPC_FLAGS_BINARY = 1

# reference util.py:356-361
CWIPC_LOG_LEVEL_NONE = 0
CWIPC_LOG_LEVEL_ERROR = 1
CWIPC_LOG_LEVEL_WARNING = 2
CWIPC_LOG_LEVEL_TRACE = 3
CWIPC_LOG_LEVEL_DEBUG = 4


class CwipcError(RuntimeError):
    pass


# ---------------------------------------------------------------------------
# native handle and record types (reference util.py:236-340)
# ---------------------------------------------------------------------------
class cwipc_pointcloud_p(ctypes.c_void_p):
    """native pointer to a cwipc_pointcloud"""


class cwipc_source_p(ctypes.c_void_p):
    """native pointer to a cwipc_source"""


class cwipc_activesource_p(cwipc_source_p):
    """native pointer to a cwipc_activesource"""


class cwipc_sink_p(ctypes.c_void_p):
    """native pointer to a cwipc_sink"""


class cwipc_metadata_p(ctypes.c_void_p):
    """native pointer to a cwipc_metadata"""


class _FieldwiseEq(ctypes.Structure):
    def __eq__(self, other: Any) -> bool:
        return isinstance(other, type(self)) and all(getattr(self, f[0]) == getattr(other, f[0]) for f in self._fields_)

    def __ne__(self, other: Any) -> bool:
        return not self.__eq__(other)

    __hash__ = None  # type: ignore


class cwipc_point(_FieldwiseEq):
    """One point: x, y, z (float), r, g, b (0..255), tile (8 bit number or camera mask).  16 bytes."""
    _fields_ = [("x", ctypes.c_float), ("y", ctypes.c_float), ("z", ctypes.c_float),
                ("r", ctypes.c_ubyte), ("g", ctypes.c_ubyte), ("b", ctypes.c_ubyte), ("tile", ctypes.c_ubyte)]


cwipc_point_numpy_dtype = [('x', '<f4'), ('y', '<f4'), ('z', '<f4'), ('r', 'u1'), ('g', 'u1'), ('b', 'u1'), ('tile', 'u1')]
assert ctypes.sizeof(cwipc_point) == 16 and numpy.dtype(cwipc_point_numpy_dtype).itemsize == 16


class cwipc_vector(_FieldwiseEq):
    _fields_ = [("x", ctypes.c_double), ("y", ctypes.c_double), ("z", ctypes.c_double)]


class cwipc_tileinfo(ctypes.Structure):
    _fields_ = [("normal", cwipc_vector), ("cameraName", ctypes.c_char_p), ("ncamera", ctypes.c_uint8), ("cameraMask", ctypes.c_uint8)]


class cwipc_point_packetheader(ctypes.Structure):
    """Header for talking to a cwipc_proxy server (field order as the reference's Python side, util.py:335-344)."""
    _fields_ = [("hdr", ctypes.c_uint32), ("magic", ctypes.c_uint32), ("cellsize", ctypes.c_float),
                ("timestamp", ctypes.c_uint64), ("unused", ctypes.c_uint32), ("dataCount", ctypes.c_uint32)]


cwipc_log_callback_type = Callable[[int, bytes], None]
_cwipc_log_callback_t = ctypes.CFUNCTYPE(None, ctypes.c_int, ctypes.c_char_p)
_cwipc_log_callback_ref = None

# ---------------------------------------------------------------------------
# library loading (reference util.py:368-553)
# ---------------------------------------------------------------------------
_dll: Optional[ctypes.CDLL] = None

_c = ctypes
_ERR = _c.POINTER(_c.c_char_p)
_BYTES = _c.POINTER(_c.c_byte)

# name -> (argtypes, restype); every symbol the reference binds, then the extensions
_SIGNATURES: Dict[str, Tuple[list, Any]] = {
    'cwipc_get_version': ([], _c.c_char_p),
    'cwipc_log_configure': ([_c.c_int, _cwipc_log_callback_t], None),
    'cwipc_dangling_allocations': ([_c.c_bool], _c.c_int),
    '_cwipc_log_emit': ([_c.c_int, _c.c_char_p, _c.c_char_p], None),
    'cwipc_read': ([_c.c_char_p, _c.c_ulonglong, _ERR, _c.c_ulong], cwipc_pointcloud_p),
    'cwipc_write_ext': ([_c.c_char_p, cwipc_pointcloud_p, _c.c_int, _ERR], _c.c_int),
    'cwipc_from_points': ([_c.c_void_p, _c.c_size_t, _c.c_int, _c.c_ulonglong, _ERR, _c.c_ulong], cwipc_pointcloud_p),
    'cwipc_from_packet': ([_c.c_char_p, _c.c_size_t, _ERR, _c.c_ulong], cwipc_pointcloud_p),
    'cwipc_read_debugdump': ([_c.c_char_p, _ERR, _c.c_ulong], cwipc_pointcloud_p),
    'cwipc_write_debugdump': ([_c.c_char_p, cwipc_pointcloud_p, _ERR], _c.c_int),
    'cwipc_pointcloud_free': ([cwipc_pointcloud_p], None),
    'cwipc_pointcloud__shallowcopy': ([cwipc_pointcloud_p], cwipc_pointcloud_p),
    'cwipc_pointcloud_timestamp': ([cwipc_pointcloud_p], _c.c_ulonglong),
    'cwipc_pointcloud_cellsize': ([cwipc_pointcloud_p], _c.c_float),
    'cwipc_pointcloud__set_cellsize': ([cwipc_pointcloud_p, _c.c_float], None),
    'cwipc_pointcloud__set_timestamp': ([cwipc_pointcloud_p, _c.c_ulonglong], None),
    'cwipc_pointcloud_count': ([cwipc_pointcloud_p], _c.c_int),
    'cwipc_pointcloud_get_uncompressed_size': ([cwipc_pointcloud_p], _c.c_size_t),
    'cwipc_pointcloud_copy_uncompressed': ([cwipc_pointcloud_p, _BYTES, _c.c_size_t], _c.c_int),
    'cwipc_pointcloud_copy_packet': ([cwipc_pointcloud_p, _BYTES, _c.c_size_t], _c.c_size_t),
    'cwipc_pointcloud_access_metadata': ([cwipc_pointcloud_p], cwipc_metadata_p),
    'cwipc_activesource_start': ([cwipc_source_p], _c.c_bool),
    'cwipc_activesource_stop': ([cwipc_source_p], None),
    'cwipc_source_get': ([cwipc_source_p], cwipc_pointcloud_p),
    'cwipc_source_available': ([cwipc_source_p, _c.c_bool], _c.c_bool),
    'cwipc_source_eof': ([cwipc_source_p], _c.c_bool),
    'cwipc_source_free': ([cwipc_source_p], None),
    'cwipc_activesource_request_metadata': ([cwipc_source_p, _c.c_char_p], None),
    'cwipc_activesource_is_metadata_requested': ([cwipc_source_p, _c.c_char_p], _c.c_bool),
    'cwipc_activesource_reload_config': ([cwipc_activesource_p, _c.c_char_p], _c.c_bool),
    'cwipc_activesource_get_config': ([cwipc_activesource_p, _BYTES, _c.c_size_t], _c.c_size_t),
    'cwipc_activesource_seek': ([cwipc_activesource_p, _c.c_uint64], _c.c_bool),
    'cwipc_activesource_maxtile': ([cwipc_activesource_p], _c.c_int),
    'cwipc_activesource_get_tileinfo': ([cwipc_activesource_p, _c.c_int, _c.POINTER(cwipc_tileinfo)], _c.c_int),
    'cwipc_activesource_auxiliary_operation': ([cwipc_source_p, _c.c_char_p, _BYTES, _c.c_size_t, _BYTES, _c.c_size_t], _c.c_bool),
    'cwipc_sink_free': ([cwipc_sink_p], None),
    'cwipc_sink_feed': ([cwipc_sink_p, cwipc_pointcloud_p, _c.c_bool], _c.c_bool),
    'cwipc_sink_caption': ([cwipc_sink_p, _c.c_char_p], _c.c_bool),
    'cwipc_sink_interact': ([cwipc_sink_p, _c.c_char_p, _c.c_char_p, _c.c_int32], _c.c_char),
    'cwipc_synthetic': ([_c.c_int, _c.c_int, _ERR, _c.c_ulong], cwipc_activesource_p),
    'cwipc_capturer': ([_c.c_char_p, _ERR, _c.c_ulong], cwipc_activesource_p),
    'cwipc_window': ([_c.c_char_p, _ERR, _c.c_ulong], cwipc_sink_p),
    'cwipc_downsample': ([cwipc_pointcloud_p, _c.c_float], cwipc_pointcloud_p),
    'cwipc_remove_outliers': ([cwipc_pointcloud_p, _c.c_int, _c.c_float, _c.c_bool], cwipc_pointcloud_p),
    'cwipc_tilefilter': ([cwipc_pointcloud_p, _c.c_int], cwipc_pointcloud_p),
    'cwipc_tilemap': ([cwipc_pointcloud_p, _c.c_char_p], cwipc_pointcloud_p),
    'cwipc_colormap': ([cwipc_pointcloud_p, _c.c_ulong, _c.c_ulong], cwipc_pointcloud_p),
    'cwipc_crop': ([cwipc_pointcloud_p, _c.c_float * 6], cwipc_pointcloud_p),
    'cwipc_join': ([cwipc_pointcloud_p, cwipc_pointcloud_p], cwipc_pointcloud_p),
    'cwipc_proxy': ([_c.c_char_p, _c.c_int, _ERR, _c.c_ulong], cwipc_activesource_p),
    'cwipc_metadata_count': ([cwipc_metadata_p], _c.c_int),
    'cwipc_metadata_name': ([cwipc_metadata_p, _c.c_int], _c.c_char_p),
    'cwipc_metadata_description': ([cwipc_metadata_p, _c.c_int], _c.c_char_p),
    'cwipc_metadata_pointer': ([cwipc_metadata_p, _c.c_int], _c.c_void_p),
    'cwipc_metadata_size': ([cwipc_metadata_p, _c.c_int], _c.c_int),
    # ---- include/cwipc_util_amd/hip_ext.h ----
    'cwipc_hip_device_count': ([], _c.c_int),
    'cwipc_hip_set_device': ([_c.c_int], _c.c_int),
    'cwipc_hip_get_device': ([], _c.c_int),
    'cwipc_hip_last_error': ([], _c.c_char_p),
    'cwipc_hip_synchronize': ([], None),
    'cwipc_hip_pool_bytes': ([], _c.c_size_t),
    'cwipc_hip_pool_trim': ([], None),
    'cwipc_hip_workspace_trim': ([], _c.c_size_t),
    'cwipc_hip_host_alloc': ([_c.c_size_t], _c.c_void_p),
    'cwipc_hip_host_free': ([_c.c_void_p], None),
    'cwipc_hip_host_register': ([_c.c_void_p, _c.c_size_t], _c.c_int),
    'cwipc_hip_host_unregister': ([_c.c_void_p], _c.c_int),
    'cwipc_hip_upload': ([cwipc_pointcloud_p], _c.c_int),
    'cwipc_hip_drop_host_copy': ([cwipc_pointcloud_p], _c.c_int),
    'cwipc_hip_is_device_resident': ([cwipc_pointcloud_p], _c.c_int),
    'cwipc_hip_device_planes': ([cwipc_pointcloud_p, _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_void_p),
                                 _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_size_t)], _c.c_int),
    'cwipc_hip_copy_device_aos': ([cwipc_pointcloud_p, _c.c_void_p, _c.c_size_t], _c.c_long),
    'cwipc_hip_from_device_aos': ([_c.c_void_p, _c.c_size_t, _c.c_uint64, _c.c_float], cwipc_pointcloud_p),
    'cwipc_hip_from_device_slots': ([_c.c_void_p, _c.c_int, _c.c_size_t, _c.c_size_t, _c.POINTER(_c.c_uint32), _c.c_uint64, _c.c_float], cwipc_pointcloud_p),
    'cwipc_hip_from_device_slots_on_stream': ([_c.c_void_p, _c.c_int, _c.c_size_t, _c.c_size_t, _c.POINTER(_c.c_uint32), _c.c_uint64, _c.c_float, _c.c_void_p], cwipc_pointcloud_p),
    'cwipc_hip_copy_device_aos_on_stream': ([cwipc_pointcloud_p, _c.c_void_p, _c.c_size_t, _c.c_void_p], _c.c_long),
    'cwipc_hip_colorize': ([cwipc_pointcloud_p, _c.c_double, _c.c_void_p, _c.c_void_p], cwipc_pointcloud_p),
    'cwipc_hip_join_multi': ([_c.POINTER(cwipc_pointcloud_p), _c.c_int], cwipc_pointcloud_p),
    'cwipc_hip_simulatecams': ([cwipc_pointcloud_p, _c.c_int, _c.c_float, _c.c_float, _c.c_void_p], cwipc_pointcloud_p),
    'cwipc_hip_simulatecams_soft': ([cwipc_pointcloud_p, _c.c_int, _c.c_float, _c.c_float, _c.c_void_p, _c.c_double, _c.c_uint64], cwipc_pointcloud_p),
    'cwipc_hip_noise': ([cwipc_pointcloud_p, _c.c_double, _c.c_uint64], cwipc_pointcloud_p),
    'cwipc_hip_tilefilter_masked': ([cwipc_pointcloud_p, _c.c_int], cwipc_pointcloud_p),
    'cwipc_hip_transform': ([cwipc_pointcloud_p, _c.POINTER(_c.c_double)], cwipc_pointcloud_p),
    'cwipc_hip_flatten_y': ([cwipc_pointcloud_p], cwipc_pointcloud_p),
    'cwipc_hip_offset_scale': ([cwipc_pointcloud_p, _c.c_double, _c.c_double, _c.c_double, _c.c_double], cwipc_pointcloud_p),
    'cwipc_hip_tiles_used': ([cwipc_pointcloud_p, _c.POINTER(_c.c_ubyte)], _c.c_int),
    'cwipc_hip_knn_mean_dist': ([cwipc_pointcloud_p, _c.c_int, _c.c_void_p, _c.c_size_t, _c.POINTER(_c.c_double), _c.c_float], _c.c_int),
    'cwipc_hip_direction_filter': ([cwipc_pointcloud_p, _c.c_double, _c.c_double, _c.c_double, _c.c_double, _c.c_float, _c.c_int], cwipc_pointcloud_p),
    'cwipc_hip_estimate_normals': ([cwipc_pointcloud_p, _c.c_float, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_size_t], _c.c_int),
    'cwipc_hip_clusters': ([cwipc_pointcloud_p, _c.c_double, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.POINTER(_c.c_uint32)], _c.c_int),
    'cwipc_hip_cluster_filter': ([cwipc_pointcloud_p, _c.c_double, _c.c_int, _c.c_uint64, _c.c_uint32], cwipc_pointcloud_p),
    'cwipc_hip_cluster_link_stats': ([cwipc_pointcloud_p, _c.c_double, _c.c_int, _c.c_void_p], _c.c_int),
    'cwipc_hip_cluster_rank_keep': ([_c.c_void_p, _c.c_size_t, _c.c_uint64, _c.c_uint32, _c.c_void_p], _c.c_int),
    'cwipc_hip_radius_counts': ([cwipc_pointcloud_p, _c.c_double, _c.c_int, _c.c_void_p, _c.c_size_t], _c.c_int),
    'cwipc_hip_radius_outlier_filter': ([cwipc_pointcloud_p, _c.c_double, _c.c_int, _c.c_uint64], cwipc_pointcloud_p),
    'cwipc_hip_smooth': ([cwipc_pointcloud_p, _c.c_double, _c.c_int, _c.c_uint32], cwipc_pointcloud_p),
    'cwipc_hip_smooth_host': ([_c.c_void_p, _c.c_size_t, _c.c_double, _c.c_int, _c.c_uint32, _c.c_void_p], _c.c_int),
    'cwipc_hip_nn_distance2': ([cwipc_pointcloud_p, cwipc_pointcloud_p, _c.c_int, _c.c_double, _c.c_void_p, _c.c_size_t], _c.c_int),
    'cwipc_hip_correspondences': ([cwipc_pointcloud_p, cwipc_pointcloud_p, _c.c_void_p, _c.c_double, _c.c_void_p, _c.c_void_p, _c.c_size_t], _c.c_int),
    'cwipc_hip_icp_sums': ([cwipc_pointcloud_p, cwipc_pointcloud_p, _c.c_void_p, _c.c_double, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p], _c.c_int),
    'cwipc_hip_icp_point2point': ([cwipc_pointcloud_p, cwipc_pointcloud_p, _c.c_double, _c.c_void_p, _c.c_double, _c.c_double, _c.c_int, _c.c_void_p, _c.c_void_p,
                                   _c.c_void_p, _c.c_void_p], _c.c_int),
    'cwipc_hip_icp_plane_sums': ([cwipc_pointcloud_p, cwipc_pointcloud_p, _c.c_void_p, _c.c_double, _c.c_void_p, _c.c_float, _c.c_int, _c.c_void_p, _c.c_void_p], _c.c_int),
    'cwipc_hip_icp_point2plane': ([cwipc_pointcloud_p, cwipc_pointcloud_p, _c.c_double, _c.c_void_p, _c.c_void_p, _c.c_float, _c.c_int, _c.c_double, _c.c_double, _c.c_int,
                                   _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p], _c.c_int),
    'cwipc_hip_gicp_covariances': ([cwipc_pointcloud_p, _c.c_void_p, _c.c_float, _c.c_int, _c.c_void_p, _c.c_double, _c.c_void_p, _c.c_size_t], _c.c_int),
    'cwipc_hip_icp_gicp_sums': ([cwipc_pointcloud_p, cwipc_pointcloud_p, _c.c_void_p, _c.c_double, _c.c_void_p, _c.c_void_p, _c.c_float, _c.c_int, _c.c_double,
                                 _c.c_void_p, _c.c_void_p], _c.c_int),
    'cwipc_hip_icp_generalized': ([cwipc_pointcloud_p, cwipc_pointcloud_p, _c.c_double, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_float, _c.c_int, _c.c_double,
                                   _c.c_double, _c.c_double, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p], _c.c_int),
    'cwipc_hip_distortion': ([cwipc_pointcloud_p, cwipc_pointcloud_p, _c.c_double, _c.c_void_p, _c.c_float, _c.c_int, _c.c_int, _c.c_void_p], _c.c_int),
    'cwipc_hip_gaussian_kde': ([_c.c_void_p, _c.c_size_t, _c.c_double, _c.c_void_p, _c.c_size_t, _c.c_void_p], _c.c_int),
    'cwipc_hip_floor_partition': ([cwipc_pointcloud_p, _c.c_double, _c.c_int, _c.c_double, _c.POINTER(_c.c_uint64)], cwipc_pointcloud_p),
    'cwipc_hip_randomize_floor': ([cwipc_pointcloud_p, _c.c_double, _c.c_uint64], cwipc_pointcloud_p),
    'cwipc_hip_plane_find': ([cwipc_pointcloud_p, _c.c_void_p, _c.c_void_p], _c.c_int),
    'cwipc_hip_plane_scores': ([cwipc_pointcloud_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p], _c.c_int),
    'cwipc_hip_plane_partition': ([cwipc_pointcloud_p, _c.c_void_p, _c.c_double, _c.c_int, _c.POINTER(_c.c_uint64)], cwipc_pointcloud_p),
    'cwipc_hip_plane_level_matrix': ([_c.c_void_p, _c.c_void_p], _c.c_int),
    'cwipc_hip_plane_find_host': ([_c.c_void_p, _c.c_size_t, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p], _c.c_int),
    'cwipc_hip_floor_radius_stats': ([cwipc_pointcloud_p, _c.c_double, _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_float)], _c.c_int),
    'cwipc_hip_nn_distance2_jobs': ([cwipc_pointcloud_p, cwipc_pointcloud_p, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_size_t], _c.c_int),
    'cwipc_hip_tile_counts': ([cwipc_pointcloud_p, _c.c_int, _c.c_double, _c.POINTER(_c.c_uint64)], _c.c_int),
    'cwipc_hip_bounds': ([cwipc_pointcloud_p, _c.POINTER(_c.c_float)], _c.c_int),
    'cwipc_hip_render': ([cwipc_pointcloud_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p], _c.c_long),
    'cwipc_hip_detect_markers': ([_c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_size_t], _c.c_long),
    'cwipc_hip_render_detect_markers': ([cwipc_pointcloud_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_void_p,
                                         _c.c_void_p, _c.c_void_p, _c.c_size_t], _c.c_long),
    'cwipc_hip_marker_labels': ([_c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p], _c.c_int),
    'cwipc_hip_from_rgbd': ([_c.c_void_p, _c.c_int, _c.c_void_p, _c.c_uint64, _c.c_float, _c.c_int, _ERR], cwipc_pointcloud_p),
    'cwipc_hip_rgbd_map2d3d': ([_c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_float)], _c.c_int),
    'cwipc_hip_rgbd_mapcolordepth': ([_c.c_void_p, _c.c_int, _c.c_int, _c.POINTER(_c.c_int)], _c.c_int),
    'cwipc_hip_rgbd_rig_create': ([_c.c_void_p, _c.c_int, _ERR], _c.c_void_p),
    'cwipc_hip_rgbd_rig_free': ([_c.c_void_p], None),
    'cwipc_hip_rgbd_rig_grab': ([_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_float, _c.c_int, _ERR], cwipc_pointcloud_p),
    'cwipc_hip_rgbd_rig_grab_occluded': ([_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_float, _c.c_int, _ERR],
                                         cwipc_pointcloud_p),
    'cwipc_hip_rgbd_rig_grab_filtered': ([_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_float, _c.c_int,
                                          _ERR], cwipc_pointcloud_p),
    'cwipc_hip_rgbd_rig_create_decimated': ([_c.c_void_p, _c.c_int, _c.c_int, _ERR], _c.c_void_p),
    'cwipc_hip_rgbd_rig_decimation': ([_c.c_void_p], _c.c_int),
    'cwipc_hip_rgbd_rig_grid_sensor': ([_c.c_void_p, _c.c_int, _c.c_void_p], _c.c_int),
    'cwipc_hip_rgbd_rig_grab_filled': ([_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_float,
                                        _c.c_int, _ERR], cwipc_pointcloud_p),
    'cwipc_hip_rgbd_rig_reset_history': ([_c.c_void_p], None),
    'cwipc_hip_rgbd_rig_history': ([_c.c_void_p, _c.c_int, _c.c_void_p, _c.c_void_p], _c.c_int),
    'cwipc_hip_rgbd_rig_ray_table': ([_c.c_void_p, _c.c_int], _c.POINTER(_c.c_double)),
    'cwipc_hip_rgbd_rig_map2d3d': ([_c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_float)], _c.c_int),
    'cwipc_hip_rgbd_rig_mapcolordepth': ([_c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_int)], _c.c_int),
    'cwipc_hip_new_encoder': ([_c.c_void_p, _ERR], _c.c_void_p),
    'cwipc_hip_encoder_free': ([_c.c_void_p], None),
    'cwipc_hip_encoder_feed': ([_c.c_void_p, cwipc_pointcloud_p], _c.c_int),
    'cwipc_hip_encoder_available': ([_c.c_void_p, _c.c_bool], _c.c_bool),
    'cwipc_hip_encoder_get_encoded_size': ([_c.c_void_p], _c.c_size_t),
    'cwipc_hip_encoder_copy_data': ([_c.c_void_p, _c.c_void_p, _c.c_size_t], _c.c_bool),
    'cwipc_hip_encoder_at_gop_boundary': ([_c.c_void_p], _c.c_bool),
    'cwipc_hip_encoder_eof': ([_c.c_void_p], _c.c_bool),
    'cwipc_hip_encoder_close': ([_c.c_void_p], None),
    'cwipc_hip_new_encodergroup': ([_ERR], _c.c_void_p),
    'cwipc_hip_encodergroup_addencoder': ([_c.c_void_p, _c.c_void_p, _ERR], _c.c_void_p),
    'cwipc_hip_encodergroup_feed': ([_c.c_void_p, cwipc_pointcloud_p], _c.c_int),
    'cwipc_hip_encodergroup_close': ([_c.c_void_p], None),
    'cwipc_hip_encodergroup_free': ([_c.c_void_p], None),
    'cwipc_hip_new_decoder': ([_ERR], _c.c_void_p),
    'cwipc_hip_decoder_feed': ([_c.c_void_p, _c.c_void_p, _c.c_size_t], _c.c_int),
    'cwipc_hip_decoder_available': ([_c.c_void_p, _c.c_bool], _c.c_bool),
    'cwipc_hip_decoder_get': ([_c.c_void_p], cwipc_pointcloud_p),
    'cwipc_hip_decoder_eof': ([_c.c_void_p], _c.c_bool),
    'cwipc_hip_decoder_close': ([_c.c_void_p], None),
    'cwipc_hip_decoder_free': ([_c.c_void_p], None),
    'cwipc_hip_codec_packet_info': ([_c.c_void_p, _c.c_size_t, _c.c_void_p, _ERR], _c.c_int),
    'cwipc_hip_encoder_set_entropy': ([_c.c_void_p, _c.c_int], _c.c_int),
    'cwipc_hip_codec_entropy_pack': ([_c.c_void_p, _c.c_size_t, _c.c_void_p, _c.c_size_t, _ERR], _c.c_size_t),
    'cwipc_hip_codec_entropy_unpack': ([_c.c_void_p, _c.c_size_t, _c.c_void_p, _c.c_size_t, _ERR], _c.c_size_t),
    'cwipc_hip_codec_entropy_info': ([_c.c_void_p, _c.c_size_t, _c.c_void_p, _ERR], _c.c_int),
    'cwipc_hip_encoder_set_colour_transform': ([_c.c_void_p, _c.c_int], _c.c_int),
    'cwipc_hip_codec_transform_pack': ([_c.c_void_p, _c.c_size_t, _c.c_int, _c.c_void_p, _c.c_size_t, _ERR], _c.c_size_t),
    'cwipc_hip_codec_transform_unpack': ([_c.c_void_p, _c.c_size_t, _c.c_void_p, _c.c_size_t, _ERR], _c.c_size_t),
    'cwipc_hip_codec_transform_info': ([_c.c_void_p, _c.c_size_t, _c.c_void_p, _ERR], _c.c_int),
    'cwipc_hip_decoder_set_max_octree_bits': ([_c.c_void_p, _c.c_int], _c.c_int),
    'cwipc_hip_codec_lod': ([_c.c_void_p, _c.c_size_t, _c.c_int, _c.c_void_p, _c.c_size_t, _ERR], _c.c_size_t),
    'cwipc_hip_codec_inter_pack': ([_c.c_void_p, _c.c_size_t, _c.c_void_p, _c.c_size_t, _c.c_uint32, _c.c_void_p, _c.c_size_t, _ERR], _c.c_size_t),
    'cwipc_hip_codec_inter_unpack': ([_c.c_void_p, _c.c_size_t, _c.c_void_p, _c.c_size_t, _c.c_void_p, _c.c_size_t, _ERR], _c.c_size_t),
    'cwipc_hip_codec_inter_info': ([_c.c_void_p, _c.c_size_t, _c.c_void_p, _ERR], _c.c_int),
    'cwipc_hip_workspace_bytes': ([], _c.c_size_t),
    'cwipc_hip_comm_unique_id': ([_c.c_void_p, _c.POINTER(_c.c_char_p)], _c.c_int),
    'cwipc_hip_comm_create': ([_c.c_void_p, _c.c_int, _c.c_int, _c.POINTER(_c.c_char_p)], _c.c_void_p),
    'cwipc_hip_comm_free': ([_c.c_void_p], None),
    'cwipc_hip_comm_rank': ([_c.c_void_p], _c.c_int),
    'cwipc_hip_comm_nranks': ([_c.c_void_p], _c.c_int),
    'cwipc_hip_comm_join': ([_c.c_void_p, cwipc_pointcloud_p, _c.c_int], cwipc_pointcloud_p),
    'cwipc_hip_comm_submit': ([_c.c_void_p, cwipc_pointcloud_p, _c.c_int], cwipc_pointcloud_p),
    'cwipc_hip_proxy_packet': ([cwipc_pointcloud_p, _c.c_void_p, _c.c_size_t, _c.c_uint32], _c.c_size_t),
    'cwipc_hip_from_proxy_packet': ([_c.c_void_p, _c.c_size_t, _c.c_int, _c.POINTER(_c.c_char_p), _c.c_uint64], cwipc_pointcloud_p),
    'cwipc_hip_profile_enable': ([_c.c_int], None),
    'cwipc_hip_profile_reset': ([], None),
    'cwipc_hip_profile_count': ([], _c.c_int),
    'cwipc_hip_profile_get': ([_c.c_int, _c.POINTER(_c.c_char_p), _c.POINTER(_c.c_double), _c.POINTER(_c.c_long)], _c.c_int),
}


def _default_library_path() -> Optional[str]:
    here = os.path.dirname(os.path.abspath(__file__))
    candidates = []
    if 'CWIPC_LIBRARY_DIR' in os.environ:   # same override the reference honours (util.py:120-123)
        candidates.append(os.path.join(os.environ['CWIPC_LIBRARY_DIR'], 'libcwipc_util.so'))
    candidates.append(os.path.join(here, 'lib', 'libcwipc_util.so'))
    for c in candidates:
        if os.path.exists(c):
            return c
    return None


def cwipc_util_dll_load(libname: Optional[str] = None) -> ctypes.CDLL:
    """Load libcwipc_util and declare the signatures (once).  Raises RuntimeError when the
    library is missing: there is no pure-Python or CPU fallback behind this wrapper."""
    global _dll
    if _dll is not None:
        return _dll
    path = libname if libname and os.path.isabs(libname) else _default_library_path()
    if not path:
        raise RuntimeError('Dynamic library cwipc_util not found (build it with `python -m cwipc_util_amd._build`)')
    dll = ctypes.CDLL(path)
    for name, (argtypes, restype) in _SIGNATURES.items():
        fn = getattr(dll, name)   # AttributeError here = the library does not export the boundary
        fn.argtypes = argtypes
        fn.restype = restype
    _dll = dll
    return dll


# ---------------------------------------------------------------------------
# point arrays
# ---------------------------------------------------------------------------
cwipc_point_array_value_type = Union[None, bytearray, bytes, ctypes.Array, List[tuple]]
cwipc_point_numpy_array_value_type = numpy.typing.NDArray[Any]
cwipc_point_numpy_matrix_value_type = numpy.typing.NDArray[numpy.floating]


def cwipc_point_array(*, count: Optional[int] = None, values: Any = ()) -> ctypes.Array:
    """Array of cwipc_point: `count` zeroed points, or built from a sequence of
    (x, y, z, r, g, b, tile) tuples, or wrapped around / copied from raw bytes."""
    if count is None:
        count = len(values)
    allocator = cwipc_point * count
    if isinstance(values, bytearray):
        return allocator.from_buffer(values)
    if isinstance(values, bytes):
        return allocator.from_buffer_copy(values)
    if not isinstance(values, tuple):
        values = tuple(values)
    return allocator(*values)


def _raise_or_warn(errorString: ctypes.c_char_p, rv: Any, fatal_if_no_rv: bool = True) -> None:
    if errorString and errorString.value:
        msg = errorString.value.decode('utf8')
        if not rv or not fatal_if_no_rv:
            raise CwipcError(msg)
        warnings.warn(msg)


# ---------------------------------------------------------------------------
# wrappers (reference util.py:573-1083)
# ---------------------------------------------------------------------------
class cwipc_pointcloud_wrapper(cwipc_pointcloud_abstract):
    """Point cloud as an opaque native object; freed when the wrapper is collected."""

    def __init__(self, _cwipc: Optional[cwipc_pointcloud_p] = None):
        if _cwipc is not None and not isinstance(_cwipc, cwipc_pointcloud_p):
            raise CwipcError("Invalid cwipc_pointcloud_p pointer passed to cwipc_pointcloud_wrapper")
        self._cwipc = _cwipc
        self._points = None
        self._bytes = None
        self._must_be_freed = True

    def __del__(self):
        if getattr(self, '_must_be_freed', False):
            self.free(force=True)

    def as_cwipc_p(self) -> cwipc_pointcloud_p:
        assert self._cwipc
        return self._cwipc

    def free(self, *, force: bool = False) -> None:
        if self._cwipc and self._must_be_freed:
            if not force:
                cwipc_log_default_callback(CWIPC_LOG_LEVEL_WARNING, b"cwipc_pointcloud_wrapper.free() called explicitly.")
            cwipc_util_dll_load().cwipc_pointcloud_free(self.as_cwipc_p())
        self._cwipc = None
        self._must_be_freed = False

    def detach(self) -> 'cwipc_pointcloud_wrapper':
        """Hand the native pointer to a new wrapper that will NOT free it; this wrapper becomes invalid."""
        if self._cwipc is None:
            cwipc_log_default_callback(CWIPC_LOG_LEVEL_WARNING, b"detach() called on NULL pointer")
        rv = type(self)(self._cwipc)
        rv._must_be_freed = False
        self._cwipc = None
        self._must_be_freed = False
        return rv

    def clone(self) -> 'cwipc_pointcloud_wrapper':
        return type(self)(cwipc_util_dll_load().cwipc_pointcloud__shallowcopy(self.as_cwipc_p()))

    def timestamp(self) -> int:
        return cwipc_util_dll_load().cwipc_pointcloud_timestamp(self.as_cwipc_p())

    def cellsize(self) -> float:
        return cwipc_util_dll_load().cwipc_pointcloud_cellsize(self.as_cwipc_p())

    def _set_cellsize(self, cellsize: float) -> None:
        cwipc_util_dll_load().cwipc_pointcloud__set_cellsize(self.as_cwipc_p(), cellsize)

    def _set_timestamp(self, timestamp: int) -> None:
        cwipc_util_dll_load().cwipc_pointcloud__set_timestamp(self.as_cwipc_p(), timestamp)

    def count(self) -> int:
        return cwipc_util_dll_load().cwipc_pointcloud_count(self.as_cwipc_p())

    def get_uncompressed_size(self) -> int:
        return cwipc_util_dll_load().cwipc_pointcloud_get_uncompressed_size(self.as_cwipc_p())

    def get_points(self) -> ctypes.Array:
        if self._points is None:
            self._initialize_points_and_bytes()
        return self._points

    def get_bytes(self) -> bytearray:
        if self._bytes is None:
            self._initialize_points_and_bytes()
        return self._bytes

    def get_numpy_array(self) -> cwipc_point_numpy_array_value_type:
        """Structured numpy view (fields x,y,z,r,g,b,tile) of the point data."""
        return numpy.ctypeslib.as_array(self.get_points())

    def get_numpy_matrix(self, onlyGeometry: bool = False) -> cwipc_point_numpy_matrix_value_type:
        """float32 matrix N x 7 (x, y, z, r, g, b, tile) or N x 3."""
        pts = self.get_numpy_array()
        m = numpy.zeros((pts.shape[0], 3 if onlyGeometry else 7), numpy.float32)
        m[:, 0], m[:, 1], m[:, 2] = pts['x'], pts['y'], pts['z']
        if not onlyGeometry:
            m[:, 3], m[:, 4], m[:, 5], m[:, 6] = pts['r'], pts['g'], pts['b'], pts['tile']
        return m

    def get_o3d_pointcloud(self):
        import open3d   # optional dependency
        m = self.get_numpy_matrix()
        pc = open3d.geometry.PointCloud()
        pc.points = open3d.utility.Vector3dVector(m[:, 0:3])
        pc.colors = open3d.utility.Vector3dVector(m[:, 3:6] / 255.0)
        return pc

    def access_metadata(self) -> Optional['cwipc_metadata']:
        rv_p = cwipc_util_dll_load().cwipc_pointcloud_access_metadata(self.as_cwipc_p())
        return cwipc_metadata(rv_p) if rv_p else None

    def _initialize_points_and_bytes(self) -> None:
        assert self._cwipc
        dll = cwipc_util_dll_load()
        nBytes = dll.cwipc_pointcloud_get_uncompressed_size(self.as_cwipc_p())
        buffer = bytearray(nBytes)
        bufferArg = (ctypes.c_byte * nBytes).from_buffer(buffer)
        nPoints = dll.cwipc_pointcloud_copy_uncompressed(self.as_cwipc_p(), bufferArg, nBytes)
        if nPoints < 0:
            raise CwipcError("cwipc_pointcloud_copy_uncompressed failed")
        self._points = cwipc_point_array(count=nPoints, values=buffer)
        self._bytes = buffer

    def copy_into(self, np_points: numpy.ndarray) -> int:
        """The points into a caller's contiguous numpy array of the cwipc_point dtype with exactly count() elements (the C call
        cwipc_pointcloud_copy_uncompressed, reference src/cwipc_util.cpp:226-250, without the bytearray get_points() makes): an
        array in page-locked memory (cwipc_hip_pinned_points, cwipc_hip_pin_array) is written by the GPU directly."""
        assert self._cwipc
        if not np_points.flags['C_CONTIGUOUS'] or np_points.dtype.itemsize != 16:
            raise ValueError("copy_into: a contiguous array of 16-byte cwipc_point records is needed")
        n = cwipc_util_dll_load().cwipc_pointcloud_copy_uncompressed(self.as_cwipc_p(), ctypes.cast(np_points.ctypes.data, _BYTES), np_points.nbytes)
        if n < 0:
            raise CwipcError("cwipc_pointcloud_copy_uncompressed failed")
        return n

    def get_packet(self) -> bytearray:
        assert self._cwipc
        dll = cwipc_util_dll_load()
        nBytes = dll.cwipc_pointcloud_copy_packet(self.as_cwipc_p(), None, 0)
        buffer = bytearray(nBytes)
        bufferArg = (ctypes.c_byte * nBytes).from_buffer(buffer)
        rvNBytes = dll.cwipc_pointcloud_copy_packet(self.as_cwipc_p(), bufferArg, nBytes)
        assert rvNBytes == nBytes
        return buffer


class cwipc_source_wrapper(cwipc_source_abstract):
    """Point cloud source as an opaque native object."""

    def __init__(self, _cwipc_source: Optional[cwipc_source_p] = None):
        if _cwipc_source is not None and not isinstance(_cwipc_source, cwipc_source_p):
            raise CwipcError("Invalid cwipc_source_p pointer passed to cwipc_source_wrapper")
        self._cwipc_source = _cwipc_source
        self._must_be_freed = True

    def __del__(self):
        if getattr(self, '_must_be_freed', False):
            self.free(force=True)

    def as_cwipc_source_p(self) -> cwipc_source_p:
        assert self._cwipc_source
        return self._cwipc_source

    def free(self, *, force: bool = False) -> None:
        if self._cwipc_source and self._must_be_freed:
            if not force:
                cwipc_log_default_callback(CWIPC_LOG_LEVEL_WARNING, b"cwipc_source_wrapper.free() called explicitly.")
            cwipc_util_dll_load().cwipc_source_free(self.as_cwipc_source_p())
        self._cwipc_source = None
        self._must_be_freed = False

    def detach(self) -> 'cwipc_source_wrapper':
        if self._cwipc_source is None:
            cwipc_log_default_callback(CWIPC_LOG_LEVEL_WARNING, b"detach() called on NULL pointer")
        rv = type(self)(self._cwipc_source)
        rv._must_be_freed = False
        self._cwipc_source = None
        self._must_be_freed = False
        return rv

    def eof(self) -> bool:
        return cwipc_util_dll_load().cwipc_source_eof(self.as_cwipc_source_p())

    def available(self, wait: bool) -> bool:
        return cwipc_util_dll_load().cwipc_source_available(self.as_cwipc_source_p(), wait)

    def get(self) -> Optional[cwipc_pointcloud_wrapper]:
        rv = cwipc_util_dll_load().cwipc_source_get(self.as_cwipc_source_p())
        return cwipc_pointcloud_wrapper(rv) if rv else None

    def statistics(self) -> None:
        pass


class cwipc_activesource_wrapper(cwipc_source_wrapper, cwipc_activesource_abstract):
    """Active (tiled) point cloud source as an opaque native object."""

    def __init__(self, _cwipc_activesource: Optional[cwipc_activesource_p] = None):
        if _cwipc_activesource is not None and not isinstance(_cwipc_activesource, cwipc_activesource_p):
            raise CwipcError("Invalid cwipc_activesource_p passed to cwipc_activesource_wrapper")
        cwipc_source_wrapper.__init__(self, _cwipc_activesource)

    def reload_config(self, config: Union[str, bytes, None]) -> bool:
        if isinstance(config, str):
            config = config.encode('utf8')
        return cwipc_util_dll_load().cwipc_activesource_reload_config(self.as_cwipc_source_p(), config)

    def get_config(self) -> bytes:
        dll = cwipc_util_dll_load()
        nBytes = dll.cwipc_activesource_get_config(self.as_cwipc_source_p(), None, 0)
        if nBytes <= 0:
            raise CwipcError("this cwipc_activesource has no camera configuration")
        buffer = bytearray(nBytes)
        bufferArg = (ctypes.c_byte * nBytes).from_buffer(buffer)
        assert dll.cwipc_activesource_get_config(self.as_cwipc_source_p(), bufferArg, nBytes) == nBytes
        return buffer

    def start(self) -> bool:
        return cwipc_util_dll_load().cwipc_activesource_start(self.as_cwipc_source_p())

    def stop(self) -> None:
        cwipc_util_dll_load().cwipc_activesource_stop(self.as_cwipc_source_p())

    def seek(self, timestamp: int) -> bool:
        return cwipc_util_dll_load().cwipc_activesource_seek(self.as_cwipc_source_p(), timestamp)

    def maxtile(self) -> int:
        return cwipc_util_dll_load().cwipc_activesource_maxtile(self.as_cwipc_source_p())

    def get_tileinfo_raw(self, tilenum: int) -> Optional[cwipc_tileinfo]:
        info = cwipc_tileinfo()
        rv = cwipc_util_dll_load().cwipc_activesource_get_tileinfo(self.as_cwipc_source_p(), tilenum, ctypes.byref(info))
        return info if rv else None

    def get_tileinfo_dict(self, tilenum: int) -> cwipc_tileinfo_dict:
        info = self.get_tileinfo_raw(tilenum)
        if info is None:
            raise CwipcError(f"get_tileinfo_raw({tilenum}) returned None")
        normal = dict(x=info.normal.x, y=info.normal.y, z=info.normal.z)
        return dict(normal=normal, cameraName=info.cameraName, ncamera=info.ncamera, cameraMask=info.cameraMask)

    def request_metadata(self, name: str) -> None:
        cwipc_util_dll_load().cwipc_activesource_request_metadata(self.as_cwipc_source_p(), name.encode('utf8'))

    def is_metadata_requested(self, name: str) -> bool:
        return cwipc_util_dll_load().cwipc_activesource_is_metadata_requested(self.as_cwipc_source_p(), name.encode('utf8'))

    def auxiliary_operation(self, op: str, inbuf: bytes, outbuf: bytearray) -> bool:
        c_inbuf = (ctypes.c_byte * len(inbuf)).from_buffer_copy(inbuf)
        c_outbuf = (ctypes.c_byte * len(outbuf)).from_buffer(outbuf)
        return cwipc_util_dll_load().cwipc_activesource_auxiliary_operation(
            self.as_cwipc_source_p(), op.encode('utf8'), c_inbuf, len(inbuf), c_outbuf, len(outbuf))


class cwipc_sink_wrapper:
    """Point cloud sink as an opaque native object (no sink is implemented by the MI355X build)."""

    def __init__(self, _cwipc_sink: Optional[cwipc_sink_p] = None):
        if _cwipc_sink is not None and not isinstance(_cwipc_sink, cwipc_sink_p):
            raise CwipcError("Invalid cwipc_sink_p passed to cwipc_sink_wrapper")
        self._cwipc_sink = _cwipc_sink
        self._must_be_freed = True

    def __del__(self):
        if getattr(self, '_must_be_freed', False):
            self.free(force=True)

    def as_cwipc_sink_p(self) -> cwipc_sink_p:
        assert self._cwipc_sink
        return self._cwipc_sink

    def free(self, *, force: bool = False) -> None:
        if self._cwipc_sink and self._must_be_freed:
            cwipc_util_dll_load().cwipc_sink_free(self.as_cwipc_sink_p())
        self._cwipc_sink = None
        self._must_be_freed = False

    def feed(self, pc: Optional[cwipc_pointcloud_wrapper], clear: bool) -> bool:
        return cwipc_util_dll_load().cwipc_sink_feed(self.as_cwipc_sink_p(), pc.as_cwipc_p() if pc is not None else None, clear)

    def caption(self, caption: str) -> bool:
        return cwipc_util_dll_load().cwipc_sink_caption(self.as_cwipc_sink_p(), caption.encode('utf8'))

    def interact(self, prompt: Optional[str], responses: Optional[str], millis: int) -> str:
        rv = cwipc_util_dll_load().cwipc_sink_interact(
            self.as_cwipc_sink_p(), prompt.encode('utf8') if prompt is not None else None,
            responses.encode('utf8') if responses is not None else None, millis)
        return rv.decode('utf8')


class cwipc_metadata:
    """Additional data attached to a point cloud (reference util.py:946-1082), the image helpers included: a source that is asked for
    "rgb" or "depth" metadata attaches its cameras' images as "rgb.<serial>" and "depth.<serial>" (RgbdSource does)."""

    def __init__(self, _cwipc_metadata: Optional[cwipc_metadata_p] = None):
        if _cwipc_metadata is not None:
            assert isinstance(_cwipc_metadata, cwipc_metadata_p)
        self._cwipc_metadata = _cwipc_metadata

    def as_cwipc_metadata_p(self) -> cwipc_metadata_p:
        assert self._cwipc_metadata
        return self._cwipc_metadata

    def count(self) -> int:
        return cwipc_util_dll_load().cwipc_metadata_count(self.as_cwipc_metadata_p())

    def name(self, idx: int) -> str:
        return cwipc_util_dll_load().cwipc_metadata_name(self.as_cwipc_metadata_p(), idx).decode('utf8')

    def description(self, idx: int) -> str:
        return cwipc_util_dll_load().cwipc_metadata_description(self.as_cwipc_metadata_p(), idx).decode('utf8')

    def pointer(self, idx: int) -> int:
        return cwipc_util_dll_load().cwipc_metadata_pointer(self.as_cwipc_metadata_p(), idx)

    def size(self, idx: int) -> int:
        return cwipc_util_dll_load().cwipc_metadata_size(self.as_cwipc_metadata_p(), idx)

    def data(self, idx: int) -> bytes:
        size = self.size(idx)
        return bytearray((ctypes.c_ubyte * size).from_address(self.pointer(idx)))

    # the images among the items (reference util.py:993-1082)
    def _parse_aux_description(self, description: str) -> Dict[str, Any]:
        """"k=v,k=v,..." as a dictionary; a value that reads as an integer becomes one."""
        rv: Dict[str, Any] = {}
        for f in description.split(','):
            k, v = f.split('=')
            try:
                rv[k] = int(v)
            except ValueError:
                rv[k] = v
        return rv

    def get_image_description(self, idx: int) -> Dict[str, Any]:
        """Item idx's description as an image description, with "image_format" (and "bpp", where a "format" gives it) added."""
        desc = self._parse_aux_description(self.description(idx))
        if "bpp" in desc:
            by_bpp = {2: "Z16", 3: "RGB8", 4: "RGBA"}
            if desc["bpp"] in by_bpp:
                desc["image_format"] = by_bpp[desc["bpp"]]
        if "format" in desc:
            image_format = desc["format"]
            by_format = {2: (3, "RGB8"), 3: (4, "BGRA"), 4: (2, "Z16")}
            if image_format in by_format:
                desc["bpp"], desc["image_format"] = by_format[image_format]
            else:
                desc["image_format"] = image_format   # a format given by name (it overrides what bpp suggested)
        return desc

    def get_image(self, idx: int) -> numpy.typing.NDArray[Any]:
        """Item idx, an image, as an array: a colour image as uint8[height, width, 3] B, G, R, a depth image as uint16[height, width]."""
        descr = self.get_image_description(idx)
        image_format = descr["image_format"]
        image_data = self.data(idx)
        if image_format == "Z16":
            return numpy.reshape(numpy.frombuffer(image_data, numpy.uint16), (descr["height"], descr["width"]))
        if image_format == "RGB8":
            return numpy.reshape(numpy.frombuffer(image_data, numpy.uint8), (descr["height"], descr["width"], descr["bpp"]))[:, :, [2, 1, 0]]
        if image_format == "BGRA":
            return numpy.reshape(numpy.frombuffer(image_data, numpy.uint8), (descr["height"], descr["width"], descr["bpp"]))[:, :, [0, 1, 2]]
        raise CwipcError(f"Unknown auxiliary data image format: {repr(image_format)}")

    def get_all_images(self, pattern: str = "") -> Dict[str, numpy.typing.NDArray[Any]]:
        """The items named "rgb.*" and "depth.*" as arrays (get_image), by name.  With a pattern only those whose name contains it, and
        the pattern is taken out of the name: ".12345" gives "rgb" and "depth" of that serial number, "rgb." the serial numbers."""
        rv = {}
        for idx in range(self.count()):
            name = self.name(idx)
            if not name.startswith("rgb.") and not name.startswith("depth."):
                continue
            if pattern:
                if pattern not in name:
                    continue
                name = name.replace(pattern, '')
            rv[name] = self.get_image(idx)
        return rv


# ---------------------------------------------------------------------------
# module-level functions (reference util.py:1085-1343)
# ---------------------------------------------------------------------------
def cwipc_get_version() -> str:
    return cwipc_util_dll_load().cwipc_get_version().decode('utf8')


def cwipc_log_configure(level: int, callback: Optional[cwipc_log_callback_type] = None) -> None:
    global _cwipc_log_callback_ref
    _cwipc_log_callback_ref = _cwipc_log_callback_t(callback) if callback else _cwipc_log_callback_t(0)
    cwipc_util_dll_load().cwipc_log_configure(level, _cwipc_log_callback_ref)


def cwipc_log_default_callback(level: int, message: bytes) -> None:
    level_name = {1: "ERROR", 2: "WARNING", 3: "INFO", 4: "DEBUG"}.get(level, f"LEVEL{level}")
    print(f"{level_name}: cwipc: {message.decode('utf8')}", file=sys.stderr)


def _cwipc_log_emit(level: int, module: str, message: str) -> None:
    cwipc_util_dll_load()._cwipc_log_emit(level, module.encode('utf8'), message.encode('utf8'))


def cwipc_dangling_allocations(log: bool) -> int:
    return cwipc_util_dll_load().cwipc_dangling_allocations(log)


def cwipc_read(filename: str, timestamp: int) -> cwipc_pointcloud_wrapper:
    """Point cloud from a PLY file (ascii or binary; reference python/cwipc/util.py cwipc_read)."""
    errorString = ctypes.c_char_p()
    rv = cwipc_util_dll_load().cwipc_read(filename.encode('utf8'), timestamp, ctypes.byref(errorString), CWIPC_API_VERSION)
    _raise_or_warn(errorString, rv)
    if rv:
        return cwipc_pointcloud_wrapper(rv)
    raise CwipcError("cwipc_read: no pointcloud read, but no specific error returned from C library")


def cwipc_write(filename: str, pointcloud: cwipc_pointcloud_wrapper, flags: int = 0) -> int:
    errorString = ctypes.c_char_p()
    rv = cwipc_util_dll_load().cwipc_write_ext(filename.encode('utf8'), pointcloud.as_cwipc_p(), flags, ctypes.byref(errorString))
    _raise_or_warn(errorString, None)
    return rv


def cwipc_from_points(points: cwipc_point_array_value_type, timestamp: int) -> cwipc_pointcloud_wrapper:
    """Point cloud from a cwipc_point_array or a sequence of (x,y,z,r,g,b,tile) tuples."""
    if not isinstance(points, ctypes.Array):
        points = cwipc_point_array(values=points)
    errorString = ctypes.c_char_p()
    rv = cwipc_util_dll_load().cwipc_from_points(ctypes.addressof(points), ctypes.sizeof(points), len(points), timestamp,
                                                 ctypes.byref(errorString), CWIPC_API_VERSION)
    _raise_or_warn(errorString, None)
    if rv:
        return cwipc_pointcloud_wrapper(rv)
    raise CwipcError("cwipc_from_points: cannot create cwipc from given argument")


def cwipc_from_numpy_array(np_points: cwipc_point_numpy_array_value_type, timestamp: int) -> cwipc_pointcloud_wrapper:
    """Point cloud from a structured numpy array with the cwipc_point dtype."""
    nPoint = np_points.shape[0]
    np_points = numpy.ascontiguousarray(np_points)
    nBytes = nPoint * np_points.strides[0] if nPoint else 0
    errorString = ctypes.c_char_p()
    rv = cwipc_util_dll_load().cwipc_from_points(np_points.ctypes.data, nBytes, nPoint, timestamp, ctypes.byref(errorString), CWIPC_API_VERSION)
    _raise_or_warn(errorString, None)
    if rv:
        return cwipc_pointcloud_wrapper(rv)
    raise CwipcError("cwipc_from_numpy_array: cannot create cwipc from given argument")


def cwipc_from_numpy_matrix(np_points_matrix: cwipc_point_numpy_matrix_value_type, timestamp: int) -> cwipc_pointcloud_wrapper:
    """Point cloud from an N x 7 float matrix (x, y, z, r, g, b, tile)."""
    count = np_points_matrix.shape[0]
    assert np_points_matrix.shape == (count, 7)
    assert np_points_matrix.dtype in (numpy.float32, numpy.float64)
    np_points = numpy.zeros(count, cwipc_point_numpy_dtype)
    for col, name in enumerate(('x', 'y', 'z')):
        np_points[name] = np_points_matrix[:, col]
    for col, name in enumerate(('r', 'g', 'b', 'tile'), start=3):
        np_points[name] = np_points_matrix[:, col].astype(numpy.uint8)
    return cwipc_from_numpy_array(np_points, timestamp)


def cwipc_from_o3d_pointcloud(o3d_pc, timestamp: int) -> cwipc_pointcloud_wrapper:
    points = numpy.asarray(o3d_pc.points)
    colors = numpy.asarray(o3d_pc.colors)
    np_matrix = numpy.zeros((points.shape[0], 7))
    np_matrix[..., 0:3] = points
    np_matrix[..., 3:6] = colors * 256
    return cwipc_from_numpy_matrix(np_matrix, timestamp)


def cwipc_from_packet(packet: Union[bytes, bytearray]) -> cwipc_pointcloud_wrapper:
    nBytes = len(packet)
    byte_array_type = ctypes.c_char * nBytes
    try:
        c_packet = byte_array_type.from_buffer(packet)
    except TypeError:
        c_packet = byte_array_type.from_buffer_copy(packet)
    errorString = ctypes.c_char_p()
    rv = cwipc_util_dll_load().cwipc_from_packet(c_packet, nBytes, ctypes.byref(errorString), CWIPC_API_VERSION)
    _raise_or_warn(errorString, None)
    if rv:
        return cwipc_pointcloud_wrapper(rv)
    raise CwipcError("cwipc_from_packet: no pointcloud read, but no specific error returned from C library")


CWIPC_POINT_PACKETHEADER_MAGIC_C = 0x20201016   # what the reference's proxy SERVER checks (include/cwipc_util/api.h:110); the Python constant above is what its SENDER writes


def cwipc_proxy_packet(pc: cwipc_pointcloud_wrapper, magic: Optional[int] = None) -> bytes:
    """The bytes the reference's sender puts on the wire for `pc` (python/cwipc/scripts/cwipc_toproxy.py:51-57): a 24-byte
    cwipc_point_packetheader and the cwipc_point records.  magic: None = the C server's (0x20201016); the reference's Python
    sender writes CWIPC_POINT_PACKETHEADER_MAGIC (0x20210208), which its own server refuses."""
    dll = cwipc_util_dll_load()
    need = dll.cwipc_hip_proxy_packet(pc.as_cwipc_p(), None, 0, 0)
    if need == 0:
        raise CwipcError("cwipc_proxy_packet: NULL pointcloud")
    buf = bytearray(need)
    c_buf = (ctypes.c_char * need).from_buffer(buf)
    got = dll.cwipc_hip_proxy_packet(pc.as_cwipc_p(), ctypes.addressof(c_buf), need, 0 if magic is None else magic)
    del c_buf
    if got != need:
        raise CwipcError("cwipc_proxy_packet: could not build the packet")
    return bytes(buf)


def cwipc_from_proxy_packet(packet: Union[bytes, bytearray], accept_python_magic: bool = False) -> cwipc_pointcloud_wrapper:
    """What the reference's proxy server does with one packet (src/cwipc_proxy.cpp:179-216): the cloud, with the header's
    timestamp (the 8 bytes the server sends back) and cellsize."""
    n = len(packet)
    c_packet = (ctypes.c_char * n).from_buffer_copy(packet)
    errorString = ctypes.c_char_p()
    rv = cwipc_util_dll_load().cwipc_hip_from_proxy_packet(ctypes.addressof(c_packet), n, 1 if accept_python_magic else 0, ctypes.byref(errorString), CWIPC_API_VERSION)
    _raise_or_warn(errorString, None)
    if rv:
        return cwipc_pointcloud_wrapper(rv)
    raise CwipcError("cwipc_from_proxy_packet: no pointcloud read, but no specific error returned from C library")


def cwipc_read_debugdump(filename: str) -> cwipc_pointcloud_wrapper:
    errorString = ctypes.c_char_p()
    rv = cwipc_util_dll_load().cwipc_read_debugdump(filename.encode('utf8'), ctypes.byref(errorString), CWIPC_API_VERSION)
    _raise_or_warn(errorString, None)
    if rv:
        return cwipc_pointcloud_wrapper(rv)
    raise CwipcError("cwipc_read_debugdump: no pointcloud read, but no specific error returned from C library")


def cwipc_write_debugdump(filename: str, pointcloud: cwipc_pointcloud_wrapper) -> int:
    errorString = ctypes.c_char_p()
    rv = cwipc_util_dll_load().cwipc_write_debugdump(filename.encode('utf8'), pointcloud.as_cwipc_p(), ctypes.byref(errorString))
    _raise_or_warn(errorString, None)
    return rv


def cwipc_synthetic(fps: int = 0, npoints: int = 0) -> cwipc_activesource_wrapper:
    """Source producing synthetically generated point clouds on every get() call."""
    errorString = ctypes.c_char_p()
    rv = cwipc_util_dll_load().cwipc_synthetic(fps, npoints, ctypes.byref(errorString), CWIPC_API_VERSION)
    _raise_or_warn(errorString, None)
    if rv:
        return cwipc_activesource_wrapper(rv)
    raise CwipcError("cwipc_synthetic: cannot create synthetic source, but no specific error returned from C library")


def cwipc_capturer(conffile: Optional[str] = None) -> cwipc_activesource_wrapper:
    errorString = ctypes.c_char_p()
    rv = cwipc_util_dll_load().cwipc_capturer(conffile.encode('utf8') if conffile else None, ctypes.byref(errorString), CWIPC_API_VERSION)
    _raise_or_warn(errorString, rv)
    if rv:
        return cwipc_activesource_wrapper(rv)
    raise CwipcError("cwipc_capturer: cannot create capturer, but no specific error returned from C library")


def cwipc_window(title: str) -> cwipc_sink_wrapper:
    errorString = ctypes.c_char_p()
    rv = cwipc_util_dll_load().cwipc_window(title.encode('utf8'), ctypes.byref(errorString), CWIPC_API_VERSION)
    _raise_or_warn(errorString, None)
    if rv:
        return cwipc_sink_wrapper(rv)
    raise CwipcError("cwipc_window: cannot create window, but no specific error returned from C library")


def cwipc_proxy(host: str, port: int) -> cwipc_activesource_wrapper:
    errorString = ctypes.c_char_p()
    rv = cwipc_util_dll_load().cwipc_proxy(host.encode('utf8'), port, ctypes.byref(errorString), CWIPC_API_VERSION)
    _raise_or_warn(errorString, None)
    if rv:
        return cwipc_activesource_wrapper(rv)
    raise CwipcError("cwipc_proxy: cannot create capturer, but no specific error returned from C library")


# ---- the hot path (reference util.py:1284-1332) ----
# Unlike the reference thunks (which wrap whatever pointer comes back, NULL included),
# these raise CwipcError on NULL: on this build NULL usually means "no GPU", and a
# wrapper around NULL would only fail later and less legibly.
def _wrap_filter_result(name: str, rv: Any) -> cwipc_pointcloud_wrapper:
    if not rv:
        detail = cwipc_util_dll_load().cwipc_hip_last_error()
        raise CwipcError(f"{name}: C library returned NULL" + (f" ({detail.decode('utf8')})" if detail else ""))
    return cwipc_pointcloud_wrapper(rv)


def cwipc_downsample(pc: cwipc_pointcloud_wrapper, voxelsize: float) -> cwipc_pointcloud_wrapper:
    """Point cloud voxelized to cubes of the given size (negative: single pcl::VoxelGrid over the whole cloud)."""
    return _wrap_filter_result('cwipc_downsample', cwipc_util_dll_load().cwipc_downsample(pc.as_cwipc_p(), voxelsize))


def cwipc_remove_outliers(pc: cwipc_pointcloud_wrapper, kNeighbors: int, stdDesvMultThresh: float, perTile: bool) -> cwipc_pointcloud_wrapper:
    """Point cloud with statistical outliers removed."""
    return _wrap_filter_result('cwipc_remove_outliers',
                               cwipc_util_dll_load().cwipc_remove_outliers(pc.as_cwipc_p(), kNeighbors, stdDesvMultThresh, perTile))


def cwipc_tilefilter(pc: cwipc_pointcloud_wrapper, tile: int) -> cwipc_pointcloud_wrapper:
    """Only the points with the given tile number (0: all points)."""
    return _wrap_filter_result('cwipc_tilefilter', cwipc_util_dll_load().cwipc_tilefilter(pc.as_cwipc_p(), tile))


def cwipc_tilemap(pc: cwipc_pointcloud_wrapper, mapping: Union[List[int], Dict[int, int], bytes, bytearray]) -> cwipc_pointcloud_wrapper:
    """Every point's tile number replaced through a 256-entry table (list/bytes) or a dict of the entries to set."""
    if not isinstance(mapping, (bytes, bytearray, list)):
        m = [0] * 256
        for k in mapping:
            m[k] = mapping[k]
        mapping = m
    return _wrap_filter_result('cwipc_tilemap', cwipc_util_dll_load().cwipc_tilemap(pc.as_cwipc_p(), bytes(mapping)))


def cwipc_colormap(pc: cwipc_pointcloud_wrapper, clearBits: int, setBits: int) -> cwipc_pointcloud_wrapper:
    """Every point's packed colour word (tile<<24 | r<<16 | g<<8 | b) masked: word = (word & ~clearBits) | setBits."""
    return _wrap_filter_result('cwipc_colormap', cwipc_util_dll_load().cwipc_colormap(pc.as_cwipc_p(), clearBits, setBits))


def cwipc_crop(pc: cwipc_pointcloud_wrapper, bbox: Union[Tuple[float, float, float, float, float, float], List[float]]) -> cwipc_pointcloud_wrapper:
    """Points inside the half-open box minx, maxx, miny, maxy, minz, maxz."""
    return _wrap_filter_result('cwipc_crop', cwipc_util_dll_load().cwipc_crop(pc.as_cwipc_p(), (ctypes.c_float * 6)(*bbox)))


def cwipc_join(pc1: cwipc_pointcloud_wrapper, pc2: cwipc_pointcloud_wrapper) -> cwipc_pointcloud_wrapper:
    """Union of the two clouds: all points of pc1, then all points of pc2."""
    return _wrap_filter_result('cwipc_join', cwipc_util_dll_load().cwipc_join(pc1.as_cwipc_p(), pc2.as_cwipc_p()))


def cwipc_join_multi(pcs: Iterable[cwipc_pointcloud_wrapper]) -> cwipc_pointcloud_wrapper:
    """n-ary join.  The reference folds cwipc_join pairwise (util.py:1330-1332, copying O(n^2) bytes);
    this is one device pass with the same result (order, min timestamp, min cellsize)."""
    pcs = list(pcs)
    if not pcs:
        raise TypeError("cwipc_join_multi() of empty iterable")   # functools.reduce raises TypeError as well
    if len(pcs) == 1:
        return pcs[0]
    arr = (cwipc_pointcloud_p * len(pcs))(*[pc.as_cwipc_p() for pc in pcs])
    return _wrap_filter_result('cwipc_join_multi', cwipc_util_dll_load().cwipc_hip_join_multi(arr, len(pcs)))


# ---------------------------------------------------------------------------
# MI355X extensions
# ---------------------------------------------------------------------------
def cwipc_hip_device_count() -> int:
    return cwipc_util_dll_load().cwipc_hip_device_count()


def cwipc_hip_set_device(device: int) -> None:
    if cwipc_util_dll_load().cwipc_hip_set_device(device) != 0:
        raise CwipcError(f"cwipc_hip_set_device({device}) failed")


def cwipc_hip_pinned_points(npoints: int) -> cwipc_point_numpy_array_value_type:
    """A structured numpy array (cwipc_point dtype) of npoints records in page-locked memory (include/cwipc_util_amd/hip_ext.h,
    cwipc_hip_host_alloc): cwipc_from_numpy_array on it -- or on a slice of it -- is read by the GPU where it lies, without the
    copy into a staging buffer that ordinary host memory needs; copy_into() of a cloud writes it directly.  For buffers that are
    reused frame after frame (a capturer's output, a decoder's).  The memory is released with the array."""
    import weakref
    dll = cwipc_util_dll_load()
    nbytes = max(int(npoints), 1) * 16
    ptr = dll.cwipc_hip_host_alloc(nbytes)
    if not ptr:
        raise CwipcError("cwipc_hip_host_alloc failed (no GPU, or no page-locked memory left)")
    buf = (ctypes.c_byte * nbytes).from_address(ptr)
    arr = numpy.frombuffer(buf, dtype=cwipc_point_numpy_dtype, count=int(npoints))
    weakref.finalize(buf, dll.cwipc_hip_host_free, ptr)   # (arr.base keeps buf alive)
    return arr


class cwipc_hip_pin_array:
    """Page-lock the memory of an existing contiguous numpy array for as long as this object lives (cwipc_hip_host_register): the
    array can then be handed to cwipc_from_numpy_array / filled by copy_into() without a staging copy.  Use as a context manager or
    keep the object; registering costs about as much as copying the array a few times, so it pays for arrays that are reused."""

    def __init__(self, array: numpy.ndarray):
        if not array.flags['C_CONTIGUOUS']:
            raise ValueError("cwipc_hip_pin_array: the array must be contiguous")
        self._array = array
        self._ptr = array.ctypes.data
        if cwipc_util_dll_load().cwipc_hip_host_register(self._ptr, array.nbytes) != 0:
            self._ptr = None
            raise CwipcError("cwipc_hip_host_register failed")

    def release(self) -> None:
        if self._ptr:
            cwipc_util_dll_load().cwipc_hip_host_unregister(self._ptr)
            self._ptr = None

    def __enter__(self): return self._array
    def __exit__(self, *exc): self.release()
    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


def cwipc_hip_upload(pc: cwipc_pointcloud_wrapper, drop_host_copy: bool = False) -> None:
    """Make the cloud device-resident now (filters do it lazily)."""
    dll = cwipc_util_dll_load()
    if dll.cwipc_hip_upload(pc.as_cwipc_p()) != 0:
        raise CwipcError("cwipc_hip_upload failed: " + dll.cwipc_hip_last_error().decode('utf8'))
    if drop_host_copy:
        dll.cwipc_hip_drop_host_copy(pc.as_cwipc_p())


def cwipc_hip_device_planes(pc: cwipc_pointcloud_wrapper) -> Tuple[int, int, int, int, int]:
    """Device addresses of the cloud's planes (x, y, z: float32[n]; rgbt: uint32[n] = r | g << 8 | b << 16 | tile << 24) and n.
    Uploads the cloud if it is not resident.  For zero-copy hand-over to other device code (and for tests that ask whether
    two clouds share their planes)."""
    x, y, z, w = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    n = ctypes.c_size_t(0)
    if cwipc_util_dll_load().cwipc_hip_device_planes(pc.as_cwipc_p(), ctypes.byref(x), ctypes.byref(y), ctypes.byref(z), ctypes.byref(w), ctypes.byref(n)) != 0:
        raise CwipcError("cwipc_hip_device_planes failed")
    return (x.value or 0, y.value or 0, z.value or 0, w.value or 0, n.value)


def cwipc_hip_colorize(pc: cwipc_pointcloud_wrapper, weight: float, lut: numpy.ndarray, valid: numpy.ndarray) -> cwipc_pointcloud_wrapper:
    """Device implementation of ColorizeFilter._mapcolor; lut (256,3) float64, valid (256,) bool."""
    lut = numpy.ascontiguousarray(lut, dtype=numpy.float64).reshape(256, 3)
    valid = numpy.ascontiguousarray(valid, dtype=numpy.uint8).reshape(256)
    rv = cwipc_util_dll_load().cwipc_hip_colorize(pc.as_cwipc_p(), float(weight), lut.ctypes.data, valid.ctypes.data)
    return _wrap_filter_result('cwipc_hip_colorize', rv)


def cwipc_hip_simulatecams(pc: cwipc_pointcloud_wrapper, camera_vectors: numpy.ndarray, centroid: numpy.ndarray) -> cwipc_pointcloud_wrapper:
    """Hard camera assignment of SimulatecamsFilter on the GPU: camera_vectors (ncam, 3) float64 with y = 0, centroid (3,) float32."""
    cams = numpy.ascontiguousarray(numpy.asarray(camera_vectors, dtype=numpy.float64)[:, [0, 2]])
    rv = cwipc_util_dll_load().cwipc_hip_simulatecams(pc.as_cwipc_p(), int(cams.shape[0]), float(numpy.float32(centroid[0])), float(numpy.float32(centroid[2])),
                                                      cams.ctypes.data)
    return _wrap_filter_result("cwipc_hip_simulatecams", rv)


def _seed64(seed: Optional[int]) -> int:
    """The 64-bit seed of a random filter: the caller's, modulo 2^64, or (None) 64 bits from os.urandom."""
    if seed is None:
        return int.from_bytes(os.urandom(8), 'little')
    return int(seed) & 0xFFFFFFFFFFFFFFFF


def cwipc_hip_simulatecams_soft(pc: cwipc_pointcloud_wrapper, camera_vectors: numpy.ndarray, centroid: numpy.ndarray, skew: float = 1.0, *,
                                seed: Optional[int] = None) -> cwipc_pointcloud_wrapper:
    """Soft camera assignment of SimulatecamsFilter on the GPU: the nearest camera or the second nearest, with a chance in proportion to
    their dot products ** skew, by one draw per point of the stream of `seed` (None: 64 bits from os.urandom; the draws are stated in
    include/cwipc_util_amd/hip_ext.h).  Arguments as cwipc_hip_simulatecams; at least two cameras."""
    cams = numpy.ascontiguousarray(numpy.asarray(camera_vectors, dtype=numpy.float64)[:, [0, 2]])
    if cams.shape[0] < 2:
        raise ValueError("cwipc_hip_simulatecams_soft: the soft rule needs at least two cameras")
    rv = cwipc_util_dll_load().cwipc_hip_simulatecams_soft(pc.as_cwipc_p(), int(cams.shape[0]), float(numpy.float32(centroid[0])), float(numpy.float32(centroid[2])),
                                                           cams.ctypes.data, float(skew), _seed64(seed))
    return _wrap_filter_result("cwipc_hip_simulatecams_soft", rv)


def cwipc_hip_noise(pc: cwipc_pointcloud_wrapper, distance: float, seed: Optional[int] = None) -> cwipc_pointcloud_wrapper:
    """Every point moved along a random vector of length up to `distance` (reference python/cwipc/filters/noise.py:31-50), on the GPU:
    the reference's f64 arithmetic on four draws per point of the stream of `seed` (None: 64 bits from os.urandom; the draws are
    stated in include/cwipc_util_amd/hip_ext.h).  Colours, tiles, timestamp and cellsize are kept; the result stays on the device."""
    rv = cwipc_util_dll_load().cwipc_hip_noise(pc.as_cwipc_p(), float(distance), _seed64(seed))
    return _wrap_filter_result("cwipc_hip_noise", rv)


CWIPC_HIP_COMM_ID_BYTES = 128
CWIPC_HIP_JOIN_LOOPBACK = 1


def cwipc_hip_comm_unique_id() -> bytes:
    """The id one rank makes and hands to the others (by any means) before they all call cwipc_hip_comm(id, rank, nranks)."""
    buf = ctypes.create_string_buffer(CWIPC_HIP_COMM_ID_BYTES)
    err = ctypes.c_char_p()
    if cwipc_util_dll_load().cwipc_hip_comm_unique_id(buf, ctypes.byref(err)) != 0:
        raise CwipcError("cwipc_hip_comm_unique_id: " + (err.value.decode('utf8') if err.value else "failed"))
    return buf.raw


class cwipc_hip_comm:
    """This rank's end of the multi-GPU join inside the library (RCCL; include/cwipc_util_amd/hip_ext.h): join(pc) once per
    frame on every rank, one C call, no torch on the way.  Creation is collective."""

    def __init__(self, unique_id: bytes, rank: int, nranks: int):
        if len(unique_id) != CWIPC_HIP_COMM_ID_BYTES:
            raise ValueError("cwipc_hip_comm: the id has %d bytes" % CWIPC_HIP_COMM_ID_BYTES)
        err = ctypes.c_char_p()
        self._dll = cwipc_util_dll_load()
        self._comm = self._dll.cwipc_hip_comm_create(unique_id, rank, nranks, ctypes.byref(err))
        if not self._comm:
            raise CwipcError("cwipc_hip_comm_create: " + (err.value.decode('utf8') if err.value else "failed"))
        self.rank, self.nranks = rank, nranks

    def join(self, pc: Optional[cwipc_pointcloud_wrapper], loopback: bool = False) -> cwipc_pointcloud_wrapper:
        """The fused cloud of this frame: every rank's points in rank order.  pc = None: no tile on this rank this frame."""
        if not self._comm:
            raise CwipcError("cwipc_hip_comm: used after free()")
        rv = self._dll.cwipc_hip_comm_join(self._comm, pc.as_cwipc_p() if pc is not None else None, CWIPC_HIP_JOIN_LOOPBACK if loopback else 0)
        return _wrap_filter_result('cwipc_hip_comm_join', rv)

    def submit(self, pc: Optional[cwipc_pointcloud_wrapper], loopback: bool = False) -> cwipc_pointcloud_wrapper:
        """join() for a stream of frames: returns at once; the fused cloud settles when it is first used (the exchange runs
        on a thread of the communicator, in the order of the calls).  pc may be freed right away."""
        if not self._comm:
            raise CwipcError("cwipc_hip_comm: used after free()")
        rv = self._dll.cwipc_hip_comm_submit(self._comm, pc.as_cwipc_p() if pc is not None else None, CWIPC_HIP_JOIN_LOOPBACK if loopback else 0)
        return _wrap_filter_result('cwipc_hip_comm_submit', rv)

    def free(self) -> None:
        if self._comm:
            self._dll.cwipc_hip_comm_free(self._comm)
            self._comm = None


def cwipc_tilefilter_masked(pc: cwipc_pointcloud_wrapper, mask: int) -> cwipc_pointcloud_wrapper:
    """Points whose tile number ANDed with mask is non-zero (reference python/cwipc/registration/util.py:98-112)."""
    return _wrap_filter_result('cwipc_tilefilter_masked', cwipc_util_dll_load().cwipc_hip_tilefilter_masked(pc.as_cwipc_p(), mask))


# ---- the floor and tile helpers of the registration pipeline (reference python/cwipc/registration/util.py:146-229) ----
CWIPC_HIP_FLOOR_KEEP_FLOOR = 1
CWIPC_HIP_FLOOR_KEEP_REST = 2
CWIPC_HIP_FLOOR_LIMIT_RADIUS = 4


def _threshold(value: Any) -> float:
    """The double the kernels compare (double)v against so that the outcome is numpy's `float32_column < value`: numpy compares in
    result_type(float32, value) -- float32 for a Python float or int and for an np.float32 (weak scalars are rounded to the
    column's type first), float64 for an np.float64 scalar, which is passed as it is."""
    dtype = numpy.result_type(numpy.float32, value)
    if dtype == numpy.float32:
        return float(numpy.float32(value))
    return float(numpy.float64(value))


def cwipc_hip_floor_partition(pc: cwipc_pointcloud_wrapper, level: Any, flags: int, radius: Any = 0.0) -> Tuple[cwipc_pointcloud_wrapper, int]:
    """Stable two-class partition on the GPU (include/cwipc_util_amd/hip_ext.h): (cloud, number of class A points).  The result has
    the input's timestamp and cellsize 0, the cellsize of a cloud fresh from cwipc_from_numpy_matrix."""
    n_first = ctypes.c_uint64(0)
    rv = cwipc_util_dll_load().cwipc_hip_floor_partition(pc.as_cwipc_p(), _threshold(level), int(flags), _threshold(radius), ctypes.byref(n_first))
    return _wrap_filter_result('cwipc_hip_floor_partition', rv), int(n_first.value)


def cwipc_floor_filter(pc: cwipc_pointcloud_wrapper, level: float = 0.1, keep: bool = False) -> cwipc_pointcloud_wrapper:
    """Remove all points that are probably on the floor (y < level); keep=True: keep only those (reference registration/util.py:146-155).
    As in the reference the result has cellsize 0 (a cloud fresh from cwipc_from_numpy_matrix), not the input's."""
    return cwipc_hip_floor_partition(pc, level, CWIPC_HIP_FLOOR_KEEP_FLOOR if keep else CWIPC_HIP_FLOOR_KEEP_REST)[0]


def cwipc_randomize_floor(pc: cwipc_pointcloud_wrapper, level: float = 0.1, *, seed: Optional[int] = None) -> cwipc_pointcloud_wrapper:
    """Randomly assign all floor points (y < level) to different tiles (reference registration/util.py:157-168): the floor points
    first, the others behind them, the floor's tile numbers permuted among the floor points.  The permutation is the stable argsort
    of splitmix64 keys of `seed` (None: 64 bits from os.urandom) -- reproducible from the seed, not numpy's Mersenne shuffle.
    Cellsize 0, as in the reference."""
    if seed is None:
        seed = int.from_bytes(os.urandom(8), 'little')
    rv = cwipc_util_dll_load().cwipc_hip_randomize_floor(pc.as_cwipc_p(), _threshold(level), int(seed) & 0xFFFFFFFFFFFFFFFF)
    return _wrap_filter_result('cwipc_randomize_floor', rv)


def cwipc_hip_tile_counts(pc: cwipc_pointcloud_wrapper, nonfloor_only: bool = False, level: Any = 0.1) -> numpy.ndarray:
    """uint64[256]: the number of points per tile number, of all points or of those that are not floor (y < level)."""
    counts = numpy.zeros(256, dtype=numpy.uint64)
    rc = cwipc_util_dll_load().cwipc_hip_tile_counts(pc.as_cwipc_p(), 1 if nonfloor_only else 0, _threshold(level), counts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)))
    if rc != 0:
        raise CwipcError("cwipc_hip_tile_counts failed")
    return counts


def cwipc_compute_tile_occupancy(pc: cwipc_pointcloud_wrapper, cellsize: float = 0, filterfloor: bool = False) -> List[Tuple[int, int]]:
    """List of (tilenum, pointcount), optionally after removing the floor and / or downsampling with cellsize, sorted by point count
    (descending; equal counts by ascending tile number), empty tiles omitted (reference registration/util.py:184-200).  One histogram
    kernel instead of a tile filter per tile; without cellsize no intermediate cloud is made."""
    if cellsize != 0:
        if filterfloor:
            pc = cwipc_floor_filter(pc)
        pc = cwipc_downsample(pc, cellsize)
        filterfloor = False
    counts = cwipc_hip_tile_counts(pc, filterfloor)
    rv = [(t, int(counts[t])) for t in range(256) if counts[t]]
    rv.sort(key=lambda tp: tp[1], reverse=True)   # (stable: ties stay in ascending tile order, as in the reference)
    return rv


def cwipc_hip_floor_radius_stats(pc: cwipc_pointcloud_wrapper, level: Any = 0.1) -> Tuple[numpy.ndarray, numpy.ndarray]:
    """(count uint64[2], stat float32[4]) per class (0 floor, 1 not floor) on d = sqrt(x*x + z*z) in float32: stat[2c] = sorted(d)[lo],
    stat[2c + 1] = sorted(d)[min(lo + 1, count[c] - 1)], lo = floor(float32(count[c] - 1) * float32(0.99)); NaN for an empty class."""
    count = numpy.zeros(2, dtype=numpy.uint64)
    stat = numpy.full(4, numpy.nan, dtype=numpy.float32)
    rc = cwipc_util_dll_load().cwipc_hip_floor_radius_stats(pc.as_cwipc_p(), _threshold(level), count.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                                            stat.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
    if rc != 0:
        raise CwipcError("cwipc_hip_floor_radius_stats failed")
    return count, stat


def _percentile99_from_neighbours(n: int, a: numpy.float32, b: numpy.float32) -> numpy.float32:
    """numpy.percentile(d, 99) of n float32 values from sorted(d)[lo] and sorted(d)[min(lo + 1, n - 1)], in numpy's own arithmetic:
    for float32 data the quantile is 99 / float32(100), the virtual index (n - 1) * q and its fractional part g are float32, and the
    result is a + (b - a) * g, or b - (b - a) * (1 - g) where g >= 0.5."""
    if n == 0:
        return numpy.float32(numpy.nan)
    virtual = numpy.float32(n - 1) * numpy.float32(0.99)
    g = numpy.float32(virtual - numpy.floor(virtual))
    a, b = numpy.float32(a), numpy.float32(b)
    with numpy.errstate(invalid='ignore', over='ignore'):
        diff = numpy.float32(b - a)
        if g >= 0.5:
            return numpy.float32(b - diff * numpy.float32(numpy.float32(1) - g))
        return numpy.float32(a + diff * g)


def cwipc_compute_radius(pc: cwipc_pointcloud_wrapper, level: float = 0.1) -> Tuple[float, float, float]:
    """The radius in the XZ plane ignoring outliers (reference registration/util.py:202-216): (overall, not floor, floor), each the
    99th percentile (numpy.percentile, linear) of the float32 distances from the y axis.  The two neighbouring order statistics
    per class are selected exactly on the GPU, the interpolation between them is numpy's, on the host.  A stated departure: an empty
    class gives nan (the reference raises IndexError) and the overall radius is then the other class's."""
    count, stat = cwipc_hip_floor_radius_stats(pc, level)
    floor_max = _percentile99_from_neighbours(int(count[0]), stat[0], stat[1])
    nonfloor_max = _percentile99_from_neighbours(int(count[1]), stat[2], stat[3])
    if count[0] == 0:
        overall = nonfloor_max
    elif count[1] == 0:
        overall = floor_max
    else:
        overall = max(floor_max, nonfloor_max)
    return overall, nonfloor_max, floor_max


def cwipc_limit_floor_to_radius(pc: cwipc_pointcloud_wrapper, radius: float, level: float = 0.1) -> cwipc_pointcloud_wrapper:
    """The cloud with the floor points (y < level) at distance >= radius from the origin removed: the remaining floor points first,
    the others behind them (reference registration/util.py:218-229; the distance is the norm of all three coordinates, as the
    reference computes it).  Cellsize 0, as in the reference."""
    return cwipc_hip_floor_partition(pc, level, CWIPC_HIP_FLOOR_KEEP_FLOOR | CWIPC_HIP_FLOOR_KEEP_REST | CWIPC_HIP_FLOOR_LIMIT_RADIUS, radius)[0]


def cwipc_hip_bounds(pc: cwipc_pointcloud_wrapper) -> numpy.ndarray:
    """float32[6]: min x, min y, min z, max x, max y, max z, NaN skipped per coordinate (+inf / -inf for an empty cloud)."""
    minmax = numpy.zeros(6, dtype=numpy.float32)
    if cwipc_util_dll_load().cwipc_hip_bounds(pc.as_cwipc_p(), minmax.ctypes.data_as(ctypes.POINTER(ctypes.c_float))) != 0:
        raise CwipcError("cwipc_hip_bounds failed")
    return minmax


class cwipc_hip_view(ctypes.Structure):
    """A pinhole view (include/cwipc_util_amd/hip_ext.h: cwipc_hip_view): the image size, the intrinsics, the depth range and the
    world -> camera matrix (row-major).  The camera looks along +z, image x runs right, image y down."""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("fx", ctypes.c_double), ("fy", ctypes.c_double), ("cx", ctypes.c_double),
                ("cy", ctypes.c_double), ("near", ctypes.c_double), ("far", ctypes.c_double), ("extrinsic", ctypes.c_double * 16)]


def cwipc_hip_render(pc: cwipc_pointcloud_wrapper, view: cwipc_hip_view, point_size: int = 5, tilemask: int = 0,
                     background: Sequence[int] = (255, 255, 255), want_index: bool = True) -> Tuple[numpy.ndarray, numpy.ndarray, Optional[numpy.ndarray]]:
    """The cloud seen through a pinhole camera, every point a square of point_size x point_size pixels in a z-buffer on the GPU:
    (rgb uint8[H, W, 3], depth float32[H, W], index int32[H, W]).  A pixel no point covers has depth 0, the background colour and
    index -1; index is the winning point's position in `pc` (None with want_index=False).  tilemask != 0: only points with
    (tile & tilemask) != 0 are drawn.  Point size 5 and the white background are open3d's defaults, which the reference's
    MultiCameraCoarseAruco sees.  The exact contract is in include/cwipc_util_amd/hip_ext.h."""
    if pc is None or view is None:
        raise CwipcError("cwipc_hip_render: NULL argument")
    h, w = max(int(view.height), 0), max(int(view.width), 0)
    if h * w > (1 << 24):
        h = w = 0   # (the library turns the call away; no arrays of that size are made for it)
    rgb = numpy.zeros((h, w, 3), dtype=numpy.uint8)
    depth = numpy.zeros((h, w), dtype=numpy.float32)
    index = numpy.zeros((h, w), dtype=numpy.int32) if want_index else None
    bg = (ctypes.c_uint8 * 3)(*[int(v) for v in background])
    dll = cwipc_util_dll_load()
    # (a dummy address for empty arrays: the library checks the sizes before it looks at them)
    rc = dll.cwipc_hip_render(pc.as_cwipc_p(), ctypes.addressof(view), int(point_size), int(tilemask), ctypes.addressof(bg), rgb.ctypes.data or 1,
                              depth.ctypes.data or 1, index.ctypes.data or 1 if index is not None else None)
    if rc < 0:
        raise CwipcError("cwipc_hip_render failed: " + dll.cwipc_hip_last_error().decode('utf8'))
    return rgb, depth, index


class cwipc_hip_marker_params(ctypes.Structure):
    """The marker detector's parameters (include/cwipc_util_amd/hip_ext.h: cwipc_hip_marker_params); the defaults are the library's."""
    _fields_ = [("window_half", ctypes.c_int32), ("threshold_offset", ctypes.c_int32), ("min_side", ctypes.c_int32),
                ("max_border_errors", ctypes.c_int32), ("max_bit_errors", ctypes.c_int32)]

    def __init__(self, window_half: int = 40, threshold_offset: int = 7, min_side: int = 14, max_border_errors: int = 2, max_bit_errors: int = 0) -> None:
        ctypes.Structure.__init__(self, int(window_half), int(threshold_offset), int(min_side), int(max_border_errors), int(max_bit_errors))


def _marker_arguments(dictionary: Any, params: Optional[cwipc_hip_marker_params], cap: Optional[int]) -> Tuple[numpy.ndarray, int, int, numpy.ndarray, numpy.ndarray]:
    words = numpy.ascontiguousarray(numpy.asarray(dictionary, dtype=numpy.uint32).reshape(-1))
    if cap is None:
        cap = len(words)   # (every id comes out once at most)
    cap = max(int(cap), 0)
    return words, (ctypes.addressof(params) if params is not None else 0), cap, numpy.zeros(cap, dtype=numpy.int32), numpy.zeros((cap, 4, 2), dtype=numpy.float32)


def cwipc_hip_detect_markers(rgb: numpy.ndarray, dictionary: Any, params: Optional[cwipc_hip_marker_params] = None,
                             cap: Optional[int] = None) -> Tuple[numpy.ndarray, numpy.ndarray, int]:
    """The square binary markers (5 x 5 payload, one-cell black border) in an rgb image (uint8[H, W, 3]), found on the GPU:
    (ids int32[n], corners float32[n, 4, 2] as (u, v): the marker's top-left, top-right, bottom-right, bottom-left, number found).
    dictionary: one payload word per id (bit 24 - (5*row + col), set = white).  n = min(number found, cap); cap None: the size of
    the dictionary.  Sorted by id.  The exact contract is in include/cwipc_util_amd/hip_ext.h."""
    img = numpy.ascontiguousarray(rgb, dtype=numpy.uint8)
    if img.ndim != 3 or img.shape[2] != 3:
        raise CwipcError("cwipc_hip_detect_markers: rgb must be uint8[H, W, 3]")
    words, pp, cap, ids, corners = _marker_arguments(dictionary, params, cap)
    dll = cwipc_util_dll_load()
    # (a dummy address for empty arrays: the library checks the sizes before it looks at them)
    rc = dll.cwipc_hip_detect_markers(img.ctypes.data or 1, img.shape[1], img.shape[0], words.ctypes.data or 1, len(words), pp, ids.ctypes.data or None,
                                      corners.ctypes.data or None, cap)
    if rc < 0:
        raise CwipcError("cwipc_hip_detect_markers failed: " + dll.cwipc_hip_last_error().decode('utf8'))
    n = min(int(rc), cap)
    return ids[:n], corners[:n], int(rc)


def cwipc_hip_render_detect_markers(pc: cwipc_pointcloud_wrapper, view: cwipc_hip_view, dictionary: Any, point_size: int = 5, tilemask: int = 0,
                                    background: Sequence[int] = (255, 255, 255), params: Optional[cwipc_hip_marker_params] = None,
                                    cap: Optional[int] = None) -> Tuple[numpy.ndarray, numpy.ndarray, numpy.ndarray, int]:
    """cwipc_hip_render and cwipc_hip_detect_markers in one call, the image never leaving the GPU: (ids, corners, corner_depth
    float32[n, 4]: the depth image's value at each corner pixel, number found).  Equal to the two calls one after the other."""
    if pc is None or view is None:
        raise CwipcError("cwipc_hip_render_detect_markers: NULL argument")
    words, pp, cap, ids, corners = _marker_arguments(dictionary, params, cap)
    corner_depth = numpy.zeros((cap, 4), dtype=numpy.float32)
    bg = (ctypes.c_uint8 * 3)(*[int(v) for v in background])
    dll = cwipc_util_dll_load()
    rc = dll.cwipc_hip_render_detect_markers(pc.as_cwipc_p(), ctypes.addressof(view), int(point_size), int(tilemask), ctypes.addressof(bg),
                                             words.ctypes.data or 1, len(words), pp, ids.ctypes.data or None, corners.ctypes.data or None,
                                             corner_depth.ctypes.data or None, cap)
    if rc < 0:
        raise CwipcError("cwipc_hip_render_detect_markers failed: " + dll.cwipc_hip_last_error().decode('utf8'))
    n = min(int(rc), cap)
    return ids[:n], corners[:n], corner_depth[:n], int(rc)


def cwipc_hip_marker_labels(rgb: numpy.ndarray, params: Optional[cwipc_hip_marker_params] = None) -> numpy.ndarray:
    """For parity tests: int32[H, W], per dark pixel of the detector's mask the smallest linear index of its 4-connected component,
    -1 for a light pixel."""
    img = numpy.ascontiguousarray(rgb, dtype=numpy.uint8)
    if img.ndim != 3 or img.shape[2] != 3:
        raise CwipcError("cwipc_hip_marker_labels: rgb must be uint8[H, W, 3]")
    labels = numpy.zeros(img.shape[:2], dtype=numpy.int32)
    dll = cwipc_util_dll_load()
    if dll.cwipc_hip_marker_labels(img.ctypes.data or 1, img.shape[1], img.shape[0], ctypes.addressof(params) if params is not None else 0,
                                   labels.ctypes.data or 1) != 0:
        raise CwipcError("cwipc_hip_marker_labels failed: " + dll.cwipc_hip_last_error().decode('utf8'))
    return labels


class cwipc_hip_rgbd_camera(ctypes.Structure):
    """One camera of a frame (include/cwipc_util_amd/hip_ext.h: cwipc_hip_rgbd_camera): the image size, the addresses of its Z16 depth
    image and of the colour image aligned to it (bpp 3: R, G, B; 4: B, G, R, A), the tile, the intrinsics, metres per depth unit, the
    camera -> world matrix (row-major) and the serial number that names the attached images."""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("depth", ctypes.c_void_p), ("colour", ctypes.c_void_p), ("bpp", ctypes.c_int32),
                ("tile", ctypes.c_uint8), ("fx", ctypes.c_double), ("fy", ctypes.c_double), ("cx", ctypes.c_double), ("cy", ctypes.c_double),
                ("depth_scale", ctypes.c_double), ("trafo", ctypes.c_double * 16), ("serial", ctypes.c_char_p)]


class cwipc_hip_rgbd_filter(ctypes.Structure):
    """The per-point filters of cwipc_hip_from_rgbd (include/cwipc_util_amd/hip_ext.h: cwipc_hip_rgbd_filter); all zero: all off."""
    _fields_ = [("threshold_near", ctypes.c_double), ("threshold_far", ctypes.c_double), ("height_min", ctypes.c_double), ("height_max", ctypes.c_double),
                ("radius", ctypes.c_float), ("greenscreen", ctypes.c_int32)]


CWIPC_HIP_RGBD_ATTACH_RGB = 1
CWIPC_HIP_RGBD_ATTACH_DEPTH = 2


def cwipc_hip_from_rgbd(cameras: Sequence[cwipc_hip_rgbd_camera], filter: Optional[cwipc_hip_rgbd_filter] = None, timestamp: int = 0, cellsize: float = 0.0,
                        attach_flags: int = 0) -> cwipc_pointcloud_wrapper:
    """One device-resident cloud from the cameras' depth and colour images, built on the GPU: the cameras in the order given, each
    camera's surviving pixels in row-major order, every point with its pixel's colour and its camera's tile.  The images the
    structures point at must stay alive during the call (rgbd.RgbdCamera.as_struct keeps them).  attach_flags
    (CWIPC_HIP_RGBD_ATTACH_*): the images go into the cloud's metadata.  The exact contract is in include/cwipc_util_amd/hip_ext.h."""
    n = len(cameras)
    array = (cwipc_hip_rgbd_camera * max(n, 1))(*cameras)
    errorString = ctypes.c_char_p()
    rv = cwipc_util_dll_load().cwipc_hip_from_rgbd(ctypes.addressof(array), n, ctypes.addressof(filter) if filter is not None else None, int(timestamp),
                                                   float(cellsize), int(attach_flags), ctypes.byref(errorString))
    _raise_or_warn(errorString, rv)
    if rv:
        return cwipc_pointcloud_wrapper(rv)
    raise CwipcError("cwipc_hip_from_rgbd: no pointcloud created, but no specific error returned from C library")


def cwipc_hip_rgbd_map2d3d(camera: cwipc_hip_rgbd_camera, u: int, v: int, d: int) -> Optional[Tuple[float, float, float]]:
    """The world point of the camera's pixel (u, v) at depth d (in depth units), in the arithmetic of cwipc_hip_from_rgbd, as three
    float32 values; None where the library says false (d <= 0, a camera it would refuse)."""
    out = (ctypes.c_float * 3)()
    if not cwipc_util_dll_load().cwipc_hip_rgbd_map2d3d(ctypes.addressof(camera), int(u), int(v), int(d), out):
        return None
    return out[0], out[1], out[2]


def cwipc_hip_rgbd_mapcolordepth(camera: cwipc_hip_rgbd_camera, u: int, v: int) -> Optional[Tuple[int, int]]:
    """The depth pixel of colour pixel (u, v): the same pixel, the images being aligned; None outside the image."""
    out = (ctypes.c_int * 2)()
    if not cwipc_util_dll_load().cwipc_hip_rgbd_mapcolordepth(ctypes.addressof(camera), int(u), int(v), out):
        return None
    return out[0], out[1]


class cwipc_hip_rgbd_sensor(ctypes.Structure):
    """One camera of a raw rig (include/cwipc_util_amd/hip_ext.h: cwipc_hip_rgbd_sensor): the depth side (size, intrinsics, the eight
    lens coefficients k1 k2 p1 p2 k3 k4 k5 k6, metres per depth unit), the colour side (its own size, bpp, intrinsics and
    coefficients), the depth-camera -> colour-camera and camera -> world matrices (row-major), the tile and the serial number."""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("fx", ctypes.c_double), ("fy", ctypes.c_double), ("cx", ctypes.c_double),
                ("cy", ctypes.c_double), ("coeffs", ctypes.c_double * 8), ("depth_scale", ctypes.c_double), ("colour_width", ctypes.c_int32),
                ("colour_height", ctypes.c_int32), ("colour_bpp", ctypes.c_int32), ("colour_fx", ctypes.c_double), ("colour_fy", ctypes.c_double),
                ("colour_cx", ctypes.c_double), ("colour_cy", ctypes.c_double), ("colour_coeffs", ctypes.c_double * 8),
                ("depth_to_colour", ctypes.c_double * 16), ("trafo", ctypes.c_double * 16), ("tile", ctypes.c_uint8), ("serial", ctypes.c_char_p)]


class cwipc_hip_rgbd_frame(ctypes.Structure):
    """One camera's images of one frame: the addresses of its Z16 depth image and of its colour image."""
    _fields_ = [("depth", ctypes.c_void_p), ("colour", ctypes.c_void_p)]


class cwipc_hip_rgbd_prep(ctypes.Structure):
    """What happens to the depth images before anything else: the box erosion's half widths, 0 .. 32, 0: off."""
    _fields_ = [("depth_x_erosion", ctypes.c_int32), ("depth_y_erosion", ctypes.c_int32)]


def _rgbd_rig_create(symbol: str, sensors: Sequence[cwipc_hip_rgbd_sensor], *more: int) -> int:
    """The body of the rig constructors: the C entry point `symbol` with the sensor array, what it takes behind it, the error string."""
    n = len(sensors)
    array = (cwipc_hip_rgbd_sensor * max(n, 1))(*sensors)
    errorString = ctypes.c_char_p()
    rv = getattr(cwipc_util_dll_load(), symbol)(ctypes.addressof(array), n, *more, ctypes.byref(errorString))
    _raise_or_warn(errorString, rv)
    if rv:
        return rv
    raise CwipcError(symbol + ": no rig created, but no specific error returned from C library")


def cwipc_hip_rgbd_rig_create(sensors: Sequence[cwipc_hip_rgbd_sensor]) -> int:
    """The rig of these sensors (an opaque handle for the calls below; cwipc_hip_rgbd_rig_free gives it back): the sensor table and the
    depth cameras' ray tables, computed and uploaded once."""
    return _rgbd_rig_create("cwipc_hip_rgbd_rig_create", sensors)


def cwipc_hip_rgbd_rig_free(rig: int) -> None:
    cwipc_util_dll_load().cwipc_hip_rgbd_rig_free(rig)


def _rgbd_rig_grab(symbol: str, rig: int, frames: Sequence[cwipc_hip_rgbd_frame], structs: Sequence[Optional[ctypes.Structure]], timestamp: int,
                   cellsize: float, attach_flags: int) -> cwipc_pointcloud_wrapper:
    """The body of the grab entries: the C entry point `symbol` with the frame array, its optional structures in C order (None: a
    NULL pointer), the scalars and the error string."""
    array = (cwipc_hip_rgbd_frame * max(len(frames), 1))(*frames)
    errorString = ctypes.c_char_p()
    rv = getattr(cwipc_util_dll_load(), symbol)(rig, ctypes.addressof(array) if len(frames) else None,
                                                *[ctypes.addressof(s) if s is not None else None for s in structs], int(timestamp), float(cellsize),
                                                int(attach_flags), ctypes.byref(errorString))
    _raise_or_warn(errorString, rv)
    if rv:
        return cwipc_pointcloud_wrapper(rv)
    raise CwipcError(symbol + ": no pointcloud created, but no specific error returned from C library")


def cwipc_hip_rgbd_rig_grab(rig: int, frames: Sequence[cwipc_hip_rgbd_frame], prep: Optional[cwipc_hip_rgbd_prep] = None,
                            filter: Optional[cwipc_hip_rgbd_filter] = None, timestamp: int = 0, cellsize: float = 0.0,
                            attach_flags: int = 0) -> cwipc_pointcloud_wrapper:
    """One device-resident cloud from one frame of raw sensor images, built on the GPU: depth erosion, the ray tables, registration of
    the colour image onto the depth grid, then cwipc_hip_from_rgbd's filters and order.  frames: one entry per sensor of the rig, in
    their order; the images must stay alive during the call.  The exact contract is in include/cwipc_util_amd/hip_ext.h."""
    return _rgbd_rig_grab("cwipc_hip_rgbd_rig_grab", rig, frames, (prep, filter), timestamp, cellsize, attach_flags)


class cwipc_hip_rgbd_occlusion(ctypes.Structure):
    """The occlusion test between a sensor's depth and colour camera: the half width of a depth sample's square in the colour grid's
    z-buffer (0 .. 8 colour pixels) and the depth margin in metres (finite, >= 0)."""
    _fields_ = [("splat", ctypes.c_int32), ("margin", ctypes.c_double)]


def cwipc_hip_rgbd_rig_grab_occluded(rig: int, frames: Sequence[cwipc_hip_rgbd_frame], prep: Optional[cwipc_hip_rgbd_prep] = None,
                                     occlusion: Optional[cwipc_hip_rgbd_occlusion] = None, filter: Optional[cwipc_hip_rgbd_filter] = None,
                                     timestamp: int = 0, cellsize: float = 0.0, attach_flags: int = 0) -> cwipc_pointcloud_wrapper:
    """cwipc_hip_rgbd_rig_grab with the occlusion between the two sensors modelled: a depth pixel whose point the colour camera cannot
    see, something nearer lying in front of it there, gives no point instead of taking that thing's colour.  occlusion None: exactly
    cwipc_hip_rgbd_rig_grab.  The exact contract is in include/cwipc_util_amd/hip_ext.h."""
    return _rgbd_rig_grab("cwipc_hip_rgbd_rig_grab_occluded", rig, frames, (prep, occlusion, filter), timestamp, cellsize, attach_flags)


class cwipc_hip_rgbd_depthfilter(ctypes.Structure):
    """The depth post-processing of the raw entry: the spatial smoother's iterations (0 .. 5, 0: off), alpha (0 < alpha <= 1) and
    delta (depth units, > 0), the temporal smoother's switch, alpha, delta and persistency mode (0 .. 8)."""
    _fields_ = [("spatial_magnitude", ctypes.c_int32), ("spatial_alpha", ctypes.c_double), ("spatial_delta", ctypes.c_double),
                ("temporal", ctypes.c_int32), ("temporal_alpha", ctypes.c_double), ("temporal_delta", ctypes.c_double),
                ("temporal_persistency", ctypes.c_int32)]


def cwipc_hip_rgbd_rig_grab_filtered(rig: int, frames: Sequence[cwipc_hip_rgbd_frame], depthfilter: Optional[cwipc_hip_rgbd_depthfilter] = None,
                                     prep: Optional[cwipc_hip_rgbd_prep] = None, occlusion: Optional[cwipc_hip_rgbd_occlusion] = None,
                                     filter: Optional[cwipc_hip_rgbd_filter] = None, timestamp: int = 0, cellsize: float = 0.0,
                                     attach_flags: int = 0) -> cwipc_pointcloud_wrapper:
    """cwipc_hip_rgbd_rig_grab / cwipc_hip_rgbd_rig_grab_occluded with the depth images smoothed on the GPU first: an edge-preserving
    spatial filter, then a temporal one that keeps its state in the rig from grab to grab.  depthfilter None, or one with both stages
    off: exactly the other two entries.  The exact contract is in include/cwipc_util_amd/hip_ext.h."""
    return _rgbd_rig_grab("cwipc_hip_rgbd_rig_grab_filtered", rig, frames, (depthfilter, prep, occlusion, filter), timestamp, cellsize, attach_flags)


def cwipc_hip_rgbd_rig_create_decimated(sensors: Sequence[cwipc_hip_rgbd_sensor], decimation: int) -> int:
    """cwipc_hip_rgbd_rig_create for a rig that decimates its depth images by `decimation` (1 .. 8) on the device before anything
    else: it is handed full-size frames and works on the decimated grid with derived sensors from there on.  decimation 1: exactly
    cwipc_hip_rgbd_rig_create.  The exact contract (RULE D) is in include/cwipc_util_amd/hip_ext.h."""
    return _rgbd_rig_create("cwipc_hip_rgbd_rig_create_decimated", sensors, int(decimation))


def cwipc_hip_rgbd_rig_decimation(rig: int) -> int:
    """The rig's decimation, 1 .. 8."""
    return cwipc_util_dll_load().cwipc_hip_rgbd_rig_decimation(rig)


def cwipc_hip_rgbd_rig_grid_sensor(rig: int, cam: int) -> cwipc_hip_rgbd_sensor:
    """Camera cam's sensor on the rig's grid: the derived one of a decimated rig, the caller's own otherwise; serial is None in it."""
    out = cwipc_hip_rgbd_sensor()
    if cwipc_util_dll_load().cwipc_hip_rgbd_rig_grid_sensor(rig, int(cam), ctypes.addressof(out)) != 0:
        raise CwipcError("cwipc_hip_rgbd_rig_grid_sensor: no such camera")
    return out


class cwipc_hip_rgbd_holefill(ctypes.Structure):
    """Hole filling of the raw entry's depth images: 0 off, 1 from the left, 2 the farthest around, 3 the nearest around."""
    _fields_ = [("mode", ctypes.c_int32)]


def cwipc_hip_rgbd_rig_grab_filled(rig: int, frames: Sequence[cwipc_hip_rgbd_frame], holefill: Optional[cwipc_hip_rgbd_holefill] = None,
                                   depthfilter: Optional[cwipc_hip_rgbd_depthfilter] = None, prep: Optional[cwipc_hip_rgbd_prep] = None,
                                   occlusion: Optional[cwipc_hip_rgbd_occlusion] = None, filter: Optional[cwipc_hip_rgbd_filter] = None,
                                   timestamp: int = 0, cellsize: float = 0.0, attach_flags: int = 0) -> cwipc_pointcloud_wrapper:
    """cwipc_hip_rgbd_rig_grab_filtered with the holes of the depth images filled on the GPU between the temporal filter and the
    erosion.  holefill None, or mode 0: exactly cwipc_hip_rgbd_rig_grab_filtered.  The exact contract (rule 0c) is in
    include/cwipc_util_amd/hip_ext.h."""
    return _rgbd_rig_grab("cwipc_hip_rgbd_rig_grab_filled", rig, frames, (holefill, depthfilter, prep, occlusion, filter), timestamp, cellsize, attach_flags)


def cwipc_hip_rgbd_rig_reset_history(rig: int) -> None:
    """Make the temporal filter's state of the rig empty again, as a new rig's."""
    cwipc_util_dll_load().cwipc_hip_rgbd_rig_reset_history(rig)


def cwipc_hip_rgbd_rig_history(rig: int, cam: int, width: int, height: int) -> Tuple[numpy.ndarray, numpy.ndarray]:
    """Camera cam's temporal-filter state, for parity tests: (running values float64[height, width], history bytes uint8[height,
    width]); zeros for a rig that has none yet (width and height: that camera's depth image)."""
    value = numpy.zeros((int(height), int(width)), dtype=numpy.float64)
    history = numpy.zeros((int(height), int(width)), dtype=numpy.uint8)
    if cwipc_util_dll_load().cwipc_hip_rgbd_rig_history(rig, int(cam), value.ctypes.data, history.ctypes.data) != 0:
        raise CwipcError("cwipc_hip_rgbd_rig_history: no such camera, or the copy failed")
    return value, history


def cwipc_hip_rgbd_rig_ray_table(rig: int, cam: int, width: int, height: int) -> numpy.ndarray:
    """A copy of camera cam's ray table as float64[height, width, 2] (width and height: that camera's depth image)."""
    ptr = cwipc_util_dll_load().cwipc_hip_rgbd_rig_ray_table(rig, int(cam))
    if not ptr:
        raise CwipcError("cwipc_hip_rgbd_rig_ray_table: no such camera")
    return numpy.ctypeslib.as_array(ptr, shape=(int(height), int(width), 2)).copy()


def cwipc_hip_rgbd_rig_map2d3d(rig: int, cam: int, u: int, v: int, d: int) -> Optional[Tuple[float, float, float]]:
    """The world point of depth-grid pixel (u, v) of camera cam at depth d (in depth units), in the arithmetic of
    cwipc_hip_rgbd_rig_grab; None where the library says false (outside the image, d <= 0, a pixel without a ray)."""
    out = (ctypes.c_float * 3)()
    if not cwipc_util_dll_load().cwipc_hip_rgbd_rig_map2d3d(rig, int(cam), int(u), int(v), int(d), out):
        return None
    return out[0], out[1], out[2]


def cwipc_hip_rgbd_rig_mapcolordepth(rig: int, cam: int, u: int, v: int) -> Optional[Tuple[int, int]]:
    """The depth pixel of pixel (u, v) of the attached (registered) colour image: the same pixel; None outside the depth image."""
    out = (ctypes.c_int * 2)()
    if not cwipc_util_dll_load().cwipc_hip_rgbd_rig_mapcolordepth(rig, int(cam), int(u), int(v), out):
        return None
    return out[0], out[1]


def cwipc_transform(pc: cwipc_pointcloud_wrapper, transform: Any) -> cwipc_pointcloud_wrapper:
    """Apply a 4x4 affine transformation (reference python/cwipc/registration/util.py:295-309: numpy
    `rot @ p + t` in float64, stored as float32).  Runs on the GPU, the cloud stays device-resident."""
    m = numpy.ascontiguousarray(numpy.asarray(transform, dtype=numpy.float64))
    if m.shape != (4, 4):
        raise ValueError("cwipc_transform: transform must be a 4x4 matrix")
    rv = cwipc_util_dll_load().cwipc_hip_transform(pc.as_cwipc_p(), m.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    return _wrap_filter_result('cwipc_transform', rv)


def cwipc_hip_flatten_y(pc: cwipc_pointcloud_wrapper) -> cwipc_pointcloud_wrapper:
    """The cloud projected onto the plane y = 0: x, z, colours and tiles kept, y = +0.0, timestamp 0, cellsize 0 -- what the reference's
    MultiCameraToFloor._prepare_floor makes through numpy (registration/multicamera.py:399-403), here without leaving the device."""
    return _wrap_filter_result('cwipc_hip_flatten_y', cwipc_util_dll_load().cwipc_hip_flatten_y(pc.as_cwipc_p()))


def cwipc_offset_scale(pc: cwipc_pointcloud_wrapper, x: float, y: float, z: float, scale: float) -> cwipc_pointcloud_wrapper:
    """(p + (x, y, z)) * scale for every point, cellsize * scale (the loop of the reference's TransformFilter,
    python/cwipc/filters/transform.py:38-52, in the same float64 arithmetic)."""
    rv = cwipc_util_dll_load().cwipc_hip_offset_scale(pc.as_cwipc_p(), float(x), float(y), float(z), float(scale))
    return _wrap_filter_result('cwipc_offset_scale', rv)


def get_tiles_used(pc: cwipc_pointcloud_wrapper) -> List[int]:
    """Sorted list of the tile numbers that occur (reference python/cwipc/registration/util.py:285-293), without downloading the cloud."""
    used = (ctypes.c_ubyte * 256)()
    rc = cwipc_util_dll_load().cwipc_hip_tiles_used(pc.as_cwipc_p(), used)
    if rc < 0:
        raise CwipcError("get_tiles_used failed")
    return [t for t in range(256) if used[t]]


def cwipc_downsample_pertile(pc: cwipc_pointcloud_wrapper, cellsize: float) -> cwipc_pointcloud_wrapper:
    """Per-tile downsample, so points in different tiles are not combined (reference python/cwipc/registration/util.py:170-182):
    for every tile number that occurs, ascending, tilefilter -> downsample; the results joined in that order.  The reference
    folds pairwise joins; one n-ary join gives the same cloud (same order, ts = min, cellsize = min) in one pass."""
    tiles_used = get_tiles_used(pc)
    parts = [cwipc_downsample(cwipc_tilefilter(pc, tilenum), cellsize) for tilenum in tiles_used]
    assert parts
    return parts[0] if len(parts) == 1 else cwipc_join_multi(parts)


def cwipc_hip_knn_mean_dist(pc: cwipc_pointcloud_wrapper, kNeighbors: int, stddevMulThresh: float = 1.0) -> Tuple[numpy.ndarray, float]:
    """Intermediate result of remove_outliers: (d_i per point, threshold).  For parity tests."""
    n = pc.count()
    out = numpy.zeros(max(n, 1), dtype=numpy.float32)
    thr = ctypes.c_double(float('nan'))
    rc = cwipc_util_dll_load().cwipc_hip_knn_mean_dist(pc.as_cwipc_p(), kNeighbors, out.ctypes.data, out.size, ctypes.byref(thr), stddevMulThresh)
    if rc != 0:
        raise CwipcError("cwipc_hip_knn_mean_dist failed")
    return out[:n], float(thr.value)


def cwipc_direction_filter(pc: cwipc_pointcloud_wrapper, direction: Union[Tuple[float, float, float], Sequence[float], numpy.ndarray], threshold: float, *,
                           radius: float = 0.02, max_nn: int = 30) -> cwipc_pointcloud_wrapper:
    """Filter a point cloud to keep only points that are somewhat facing a direction (reference registration/util.py:114-143).

    Per point the normal of its neighbourhood (the max_nn nearest points within radius: the reference's open3d
    KDTreeSearchParamHybrid(0.02, 30)), turned to point away from the centroid; kept iff normal . direction / |direction| >= threshold."""
    d = numpy.asarray(direction, dtype=numpy.float64).reshape(-1)
    assert d.shape == (3,)
    rv = cwipc_util_dll_load().cwipc_hip_direction_filter(pc.as_cwipc_p(), float(d[0]), float(d[1]), float(d[2]), float(threshold), float(radius), int(max_nn))
    return _wrap_filter_result('cwipc_hip_direction_filter', rv)


CWIPC_HIP_CLUSTER_SAME_TILE = 1


def cwipc_cluster_labels(pc: cwipc_pointcloud_wrapper, radius: float, same_tile: bool = False) -> Tuple[numpy.ndarray, numpy.ndarray]:
    """Euclidean clusters of a cloud (include/cwipc_util_amd/hip_ext.h, RULE K): the connected components of "closer than radius",
    strictly, in float64.  Returns (labels, sizes), both uint32: labels[i] is the number of point i's cluster -- clusters are numbered
    in order of first appearance in the input -- or 0xFFFFFFFF for a point with a non-finite coordinate; sizes[c] is the point count of
    cluster c.  same_tile: only points with equal tile bytes are linked."""
    if pc is None:
        raise CwipcError("cwipc_cluster_labels: NULL pointcloud")
    n = pc.count()
    labels = numpy.zeros(max(n, 1), dtype=numpy.uint32)
    sizes = numpy.zeros(max(n, 1), dtype=numpy.uint32)
    nclusters = ctypes.c_uint32(0)
    flags = CWIPC_HIP_CLUSTER_SAME_TILE if same_tile else 0
    rc = cwipc_util_dll_load().cwipc_hip_clusters(pc.as_cwipc_p(), float(radius), flags, labels.ctypes.data, sizes.ctypes.data, labels.size, ctypes.byref(nclusters))
    if rc != 0:
        raise CwipcError("cwipc_hip_clusters failed")
    return labels[:n], sizes[:nclusters.value].copy()


def cwipc_cluster_filter(pc: cwipc_pointcloud_wrapper, radius: float, min_points: int = 1, max_clusters: int = 0, same_tile: bool = False) -> cwipc_pointcloud_wrapper:
    """Keep the points whose Euclidean cluster (cwipc_cluster_labels) has at least min_points points and is among the max_clusters
    largest (0: no limit; ties go to the cluster that appears first).  Input order, colours, tiles, timestamp and cellsize are kept."""
    if pc is None:
        raise CwipcError("cwipc_cluster_filter: NULL pointcloud")
    flags = CWIPC_HIP_CLUSTER_SAME_TILE if same_tile else 0
    rv = cwipc_util_dll_load().cwipc_hip_cluster_filter(pc.as_cwipc_p(), float(radius), flags, int(min_points), int(max_clusters))
    return _wrap_filter_result('cwipc_hip_cluster_filter', rv)


def cwipc_hip_cluster_link_stats(pc: cwipc_pointcloud_wrapper, radius: float, same_tile: bool = False) -> Dict[str, int]:
    """What the clusters' link kernel did on this cloud, for measurements: links seen (each unordered pair once), unions issued, parent
    words loaded by the finds, the most loaded by one union.  The last three depend on scheduling."""
    out = numpy.zeros(4, dtype=numpy.uint64)
    flags = CWIPC_HIP_CLUSTER_SAME_TILE if same_tile else 0
    if cwipc_util_dll_load().cwipc_hip_cluster_link_stats(pc.as_cwipc_p(), float(radius), flags, out.ctypes.data) != 0:
        raise CwipcError("cwipc_hip_cluster_link_stats failed")
    return {"links": int(out[0]), "unions": int(out[1]), "find_loads": int(out[2]), "max_loads_one_union": int(out[3])}


def cwipc_hip_cluster_rank_keep(sizes, min_points: int = 1, max_clusters: int = 0) -> numpy.ndarray:
    """An entry for tests: the cluster filter's ranking and keep kernels on cluster sizes that the caller gives (uint32, any values).
    Returns a bool array, keep[c]: sizes[c] >= min_points and cluster c among the max_clusters largest (0: no limit; ties go to the
    lower number)."""
    sizes = numpy.ascontiguousarray(sizes, dtype=numpy.uint32).reshape(-1)
    keep = numpy.zeros(max(sizes.size, 1), dtype=numpy.uint8)
    probe = sizes if sizes.size else numpy.zeros(1, dtype=numpy.uint32)
    if cwipc_util_dll_load().cwipc_hip_cluster_rank_keep(probe.ctypes.data, sizes.size, int(min_points), int(max_clusters), keep.ctypes.data) != 0:
        raise CwipcError("cwipc_hip_cluster_rank_keep failed")
    return keep[:sizes.size].astype(bool)


CWIPC_HIP_NEIGH_SAME_TILE = 1


def cwipc_radius_counts(pc: cwipc_pointcloud_wrapper, radius: float, same_tile: bool = False) -> numpy.ndarray:
    """Per point, how many OTHER points lie closer than radius (include/cwipc_util_amd/hip_ext.h, RULE N: strictly, in float64); 0
    for a point with a non-finite coordinate.  uint32.  same_tile: only points with the point's own tile byte count."""
    if pc is None:
        raise CwipcError("cwipc_radius_counts: NULL pointcloud")
    n = pc.count()
    counts = numpy.zeros(max(n, 1), dtype=numpy.uint32)
    flags = CWIPC_HIP_NEIGH_SAME_TILE if same_tile else 0
    if cwipc_util_dll_load().cwipc_hip_radius_counts(pc.as_cwipc_p(), float(radius), flags, counts.ctypes.data, counts.size) != 0:
        raise CwipcError("cwipc_hip_radius_counts failed")
    return counts[:n]


def cwipc_radius_outlier_filter(pc: cwipc_pointcloud_wrapper, radius: float, min_neighbours: int = 1, same_tile: bool = False) -> cwipc_pointcloud_wrapper:
    """Keep the points with at least min_neighbours other points closer than radius (cwipc_radius_counts).  Input order, colours,
    tiles, timestamp and cellsize are kept."""
    if pc is None:
        raise CwipcError("cwipc_radius_outlier_filter: NULL pointcloud")
    flags = CWIPC_HIP_NEIGH_SAME_TILE if same_tile else 0
    rv = cwipc_util_dll_load().cwipc_hip_radius_outlier_filter(pc.as_cwipc_p(), float(radius), flags, int(min_neighbours))
    return _wrap_filter_result('cwipc_hip_radius_outlier_filter', rv)


def cwipc_smooth(pc: cwipc_pointcloud_wrapper, radius: float, min_neighbours: int = 2, same_tile: bool = False) -> cwipc_pointcloud_wrapper:
    """Every point with at least max(2, min_neighbours) other points closer than radius moved onto the plane fitted to them with a
    compact biweight (first-order moving least squares; include/cwipc_util_amd/hip_ext.h, RULE N).  No point is removed; colours,
    tiles, order, timestamp and cellsize are kept.  The result stays on the device and is handed back with its kernel in flight."""
    if pc is None:
        raise CwipcError("cwipc_smooth: NULL pointcloud")
    flags = CWIPC_HIP_NEIGH_SAME_TILE if same_tile else 0
    rv = cwipc_util_dll_load().cwipc_hip_smooth(pc.as_cwipc_p(), float(radius), flags, int(min_neighbours))
    return _wrap_filter_result('cwipc_hip_smooth', rv)


def cwipc_hip_smooth_host(points: numpy.ndarray, radius: float, min_neighbours: int = 2, same_tile: bool = False) -> numpy.ndarray:
    """The host twin of cwipc_smooth on a structured array of cwipc_point records: the same arithmetic (csrc/smooth_terms.hpp) by
    brute force over all pairs, O(n * n), no GPU.  For tests and small clouds."""
    points = numpy.ascontiguousarray(points, dtype=cwipc_point_numpy_dtype).reshape(-1)
    out = numpy.zeros(max(points.size, 1), dtype=cwipc_point_numpy_dtype)
    flags = CWIPC_HIP_NEIGH_SAME_TILE if same_tile else 0
    probe = points if points.size else out
    if cwipc_util_dll_load().cwipc_hip_smooth_host(probe.ctypes.data, points.size, float(radius), flags, int(min_neighbours), out.ctypes.data) != 0:
        raise CwipcError("cwipc_hip_smooth_host failed")
    return out[:points.size]


# ---- plane segmentation (include/cwipc_util_amd/hip_ext.h, RULE S; no reference counterpart) ----
CWIPC_HIP_PLANE_REFINE = 1
CWIPC_HIP_PLANE_KEEP_INLIERS = 1
CWIPC_HIP_PLANE_KEEP_REST = 2
CWIPC_HIP_PLANE_BELOW_IS_INLIER = 4
# the score kernel's shape (csrc/internal.hpp), for tests that sit on its edges
CWIPC_HIP_PLANE_SCORE_TILE = 2048
CWIPC_HIP_PLANE_SCORE_GRID = 512
CWIPC_HIP_PLANE_SCORE_HBLOCK = 64


class cwipc_hip_plane_params(ctypes.Structure):
    _fields_ = [("distance", ctypes.c_double), ("seed", ctypes.c_uint64), ("axis", ctypes.c_double * 3), ("min_abs_cos", ctypes.c_double),
                ("iterations", ctypes.c_uint32), ("flags", ctypes.c_int32)]


class cwipc_hip_plane_result(ctypes.Structure):
    _fields_ = [("plane", ctypes.c_double * 4), ("hypothesis", ctypes.c_double * 4), ("sums", ctypes.c_int64 * 10), ("M", ctypes.c_double * 6),
                ("best", ctypes.c_uint32), ("triple", ctypes.c_uint32 * 3), ("count", ctypes.c_uint32), ("recount", ctypes.c_uint32),
                ("valid", ctypes.c_uint32), ("found", ctypes.c_int32), ("refined", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class cwipc_plane_result:
    """What a plane search found.  plane: the returned plane (n_x, n_y, n_z, d) as float64, oriented towards the axis (+Y when
    unconstrained); hypothesis: the best triple's plane; found / refined: bools; best, triple, count: the best hypothesis, its point
    indices and inliers; refit_count, sums, M: the refit's; recount: inliers of the refit plane; valid: number of valid hypotheses.
    raw is the C structure, whose bytes tests compare."""

    def __init__(self, raw: cwipc_hip_plane_result):
        self.raw = raw
        self.plane = numpy.array(raw.plane[:], dtype=numpy.float64)
        self.hypothesis = numpy.array(raw.hypothesis[:], dtype=numpy.float64)
        self.sums = numpy.array(raw.sums[:], dtype=numpy.int64)
        self.M = numpy.array(raw.M[:], dtype=numpy.float64)
        self.best = int(raw.best)
        self.triple = tuple(int(v) for v in raw.triple)
        self.count = int(raw.count)
        self.recount = int(raw.recount)
        self.refit_count = int(raw.sums[0])
        self.valid = int(raw.valid)
        self.found = bool(raw.found)
        self.refined = bool(raw.refined)

    def tobytes(self) -> bytes:
        return bytes(self.raw)

    def __repr__(self) -> str:
        return "cwipc_plane_result(found=%r, plane=%r, count=%d, refined=%r, recount=%d)" % (self.found, self.plane.tolist(), self.count, self.refined, self.recount)


def cwipc_plane_constraint(axis: Any = None, max_angle: Optional[float] = None) -> Tuple[Tuple[float, float, float], float]:
    """(unit axis, min_abs_cos) of RULE S from an axis and the largest angle, in DEGREES, between it and the plane's normal.  Neither
    given: unconstrained, ((0, 0, 0), 0).  max_angle alone: about +Y.  The trigonometry happens here, not in the rule."""
    if axis is None and max_angle is None:
        return (0.0, 0.0, 0.0), 0.0
    if max_angle is None:
        raise ValueError("cwipc_plane_constraint: an axis needs max_angle")
    a = numpy.array((0.0, 1.0, 0.0) if axis is None else axis, dtype=numpy.float64).reshape(-1)
    if a.shape != (3,) or not numpy.all(numpy.isfinite(a)) or not numpy.any(a != 0):
        raise ValueError("cwipc_plane_constraint: the axis must be three finite numbers, not all zero")
    if not (0.0 <= float(max_angle) <= 90.0):
        raise ValueError("cwipc_plane_constraint: max_angle must lie between 0 and 90 degrees")
    a = a / math.sqrt(float(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]))
    return (float(a[0]), float(a[1]), float(a[2])), min(1.0, max(0.0, math.cos(math.radians(float(max_angle)))))


def _plane_params(who: str, distance: float, iterations: int, seed: int, axis: Any, max_angle: Optional[float], refine: bool) -> cwipc_hip_plane_params:
    distance = float(distance)
    if not (1e-30 <= distance <= 1e30):
        raise ValueError("%s: distance must be finite and within [1e-30, 1e30]" % who)
    if not (1 <= int(iterations) <= 65536):
        raise ValueError("%s: iterations must lie between 1 and 65536" % who)
    if not (0 <= int(seed) < 2 ** 64):
        raise ValueError("%s: seed must be a uint64" % who)
    unit, mac = cwipc_plane_constraint(axis, max_angle)
    p = cwipc_hip_plane_params()
    p.distance = distance
    p.seed = int(seed)
    p.axis[0], p.axis[1], p.axis[2] = unit
    p.min_abs_cos = mac
    p.iterations = int(iterations)
    p.flags = CWIPC_HIP_PLANE_REFINE if refine else 0
    return p


def _plane4(who: str, plane: Any) -> numpy.ndarray:
    if isinstance(plane, cwipc_plane_result):
        if not plane.found:
            raise ValueError("%s: the search found no plane" % who)
        plane = plane.plane
    p = numpy.ascontiguousarray(numpy.asarray(plane, dtype=numpy.float64)).reshape(-1)
    if p.shape != (4,) or not numpy.all(numpy.isfinite(p)) or not numpy.any(p[:3] != 0):
        raise ValueError("%s: a plane is four finite numbers (n_x, n_y, n_z, d) with a normal that is not zero" % who)
    return p


def cwipc_find_plane(pc: cwipc_pointcloud_wrapper, distance: float, iterations: int = 1024, seed: int = 0, axis: Any = None,
                     max_angle: Optional[float] = None, refine: bool = True) -> cwipc_plane_result:
    """The dominant plane of the cloud by random-sample consensus on the GPU (RULE S): `iterations` seeded triples, each scored by
    the number of points within `distance`; the best one, refitted to its inliers when refine.  axis / max_angle (degrees) keep
    only planes whose normal lies within max_angle of the axis (cwipc_plane_constraint).  result.found is False when no triple gave
    a plane (fewer than 3 points, all points equal or collinear, ...)."""
    if pc is None:
        raise CwipcError("cwipc_find_plane: NULL pointcloud")
    params = _plane_params("cwipc_find_plane", distance, iterations, seed, axis, max_angle, refine)
    raw = cwipc_hip_plane_result()
    if cwipc_util_dll_load().cwipc_hip_plane_find(pc.as_cwipc_p(), ctypes.addressof(params), ctypes.addressof(raw)) != 0:
        raise CwipcError("cwipc_hip_plane_find failed")
    return cwipc_plane_result(raw)


def cwipc_hip_plane_scores(pc: cwipc_pointcloud_wrapper, distance: float, iterations: int = 1024, seed: int = 0, axis: Any = None,
                           max_angle: Optional[float] = None) -> Dict[str, numpy.ndarray]:
    """The whole hypothesis table of cwipc_find_plane, for tests and diagnostics: planes (H x 4 float64), counts (uint32), triples
    (H x 3 uint32), valid (bool)."""
    if pc is None:
        raise CwipcError("cwipc_hip_plane_scores: NULL pointcloud")
    params = _plane_params("cwipc_hip_plane_scores", distance, iterations, seed, axis, max_angle, False)
    H = int(iterations)
    planes = numpy.zeros((H, 4), dtype=numpy.float64)
    counts = numpy.zeros(H, dtype=numpy.uint32)
    triples = numpy.zeros((H, 3), dtype=numpy.uint32)
    valid = numpy.zeros(H, dtype=numpy.uint8)
    if cwipc_util_dll_load().cwipc_hip_plane_scores(pc.as_cwipc_p(), ctypes.addressof(params), planes.ctypes.data, counts.ctypes.data, triples.ctypes.data,
                                                    valid.ctypes.data) != 0:
        raise CwipcError("cwipc_hip_plane_scores failed")
    return {"planes": planes, "counts": counts, "triples": triples, "valid": valid.astype(bool)}


def cwipc_hip_plane_partition(pc: cwipc_pointcloud_wrapper, plane: Any, distance: float, flags: int) -> Tuple[cwipc_pointcloud_wrapper, int]:
    """Stable two-class partition by a plane on the GPU (RULE S): (cloud, number of class A points).  Class A, first: the points
    within `distance` of the plane (CWIPC_HIP_PLANE_KEEP_INLIERS; with CWIPC_HIP_PLANE_BELOW_IS_INLIER everything at most `distance`
    above it); class B: the others (CWIPC_HIP_PLANE_KEEP_REST).  Colours, tiles, timestamp and cellsize are the input's."""
    if pc is None:
        raise CwipcError("cwipc_hip_plane_partition: NULL pointcloud")
    p = _plane4("cwipc_hip_plane_partition", plane)
    n_first = ctypes.c_uint64(0)
    rv = cwipc_util_dll_load().cwipc_hip_plane_partition(pc.as_cwipc_p(), p.ctypes.data, float(distance), int(flags), ctypes.byref(n_first))
    return _wrap_filter_result('cwipc_hip_plane_partition', rv), int(n_first.value)


def cwipc_plane_filter(pc: cwipc_pointcloud_wrapper, plane: Any, distance: float, keep: str = "rest", below: bool = False) -> cwipc_pointcloud_wrapper:
    """Remove the points of a plane (keep="rest"), keep only them ("inliers") or put them first ("both").  below: everything under
    the plane counts as the plane -- the floor and what lies beneath it."""
    flags = {"rest": CWIPC_HIP_PLANE_KEEP_REST, "inliers": CWIPC_HIP_PLANE_KEEP_INLIERS, "both": CWIPC_HIP_PLANE_KEEP_INLIERS | CWIPC_HIP_PLANE_KEEP_REST}.get(keep)
    if flags is None:
        raise ValueError("cwipc_plane_filter: keep is 'rest', 'inliers' or 'both'")
    return cwipc_hip_plane_partition(pc, plane, distance, flags | (CWIPC_HIP_PLANE_BELOW_IS_INLIER if below else 0))[0]


def cwipc_hip_plane_level_matrix(plane: Any) -> numpy.ndarray:
    """The 4x4 motion that makes the plane y = 0: the minimal rotation taking its normal (towards +Y) to (0, 1, 0), then the shift
    along y (RULE S, Levelling).  Host arithmetic, no GPU."""
    p = _plane4("cwipc_hip_plane_level_matrix", plane)
    m = numpy.zeros((4, 4), dtype=numpy.float64)
    if cwipc_util_dll_load().cwipc_hip_plane_level_matrix(p.ctypes.data, m.ctypes.data) != 0:
        raise CwipcError("cwipc_hip_plane_level_matrix failed")
    return m


def cwipc_level_to_plane(pc: cwipc_pointcloud_wrapper, plane: Any) -> cwipc_pointcloud_wrapper:
    """The cloud moved so that the plane becomes y = 0 with its normal up: cwipc_hip_plane_level_matrix, then cwipc_transform."""
    return cwipc_transform(pc, cwipc_hip_plane_level_matrix(plane))


def cwipc_find_planes(pc: cwipc_pointcloud_wrapper, distance: float, max_planes: int, min_inliers: int = 3, iterations: int = 1024, seed: int = 0,
                      axis: Any = None, max_angle: Optional[float] = None, refine: bool = True) -> Tuple[List[cwipc_plane_result], cwipc_pointcloud_wrapper]:
    """Peel planes off the cloud: find the dominant plane, stop when it has fewer than min_inliers points within `distance` (the
    returned plane's: the recount when refined, else the count), otherwise take its inliers out and search what is left; at most
    max_planes times.  Every search uses the same seed.  The cloud stays on the device throughout.  Returns the planes and the
    remainder (the input itself when nothing was peeled)."""
    planes: List[cwipc_plane_result] = []
    rest = pc
    for _ in range(int(max_planes)):
        found = cwipc_find_plane(rest, distance, iterations, seed, axis, max_angle, refine)
        inliers = found.recount if found.refined else found.count
        if not found.found or inliers < int(min_inliers):
            break
        planes.append(found)
        peeled = cwipc_plane_filter(rest, found.plane, distance, keep="rest")
        if rest is not pc:
            rest.free()
        rest = peeled
    return planes, rest


def cwipc_hip_plane_find_host(points: numpy.ndarray, distance: float, iterations: int = 1024, seed: int = 0, axis: Any = None,
                              max_angle: Optional[float] = None, refine: bool = True) -> Tuple[cwipc_plane_result, Dict[str, numpy.ndarray]]:
    """The host twin of cwipc_find_plane and cwipc_hip_plane_scores on a structured array of cwipc_point records: the same
    arithmetic (csrc/plane_seg_terms.hpp) by brute force, O(n * iterations), no GPU.  (result, {planes, counts, valid})."""
    points = numpy.ascontiguousarray(points, dtype=cwipc_point_numpy_dtype).reshape(-1)
    params = _plane_params("cwipc_hip_plane_find_host", distance, iterations, seed, axis, max_angle, refine)
    H = int(iterations)
    planes = numpy.zeros((H, 4), dtype=numpy.float64)
    counts = numpy.zeros(H, dtype=numpy.uint32)
    valid = numpy.zeros(H, dtype=numpy.uint8)
    raw = cwipc_hip_plane_result()
    probe = points if points.size else numpy.zeros(1, dtype=cwipc_point_numpy_dtype)
    if cwipc_util_dll_load().cwipc_hip_plane_find_host(probe.ctypes.data, points.size, ctypes.addressof(params), ctypes.addressof(raw), planes.ctypes.data,
                                                       counts.ctypes.data, valid.ctypes.data) != 0:
        raise CwipcError("cwipc_hip_plane_find_host failed")
    return cwipc_plane_result(raw), {"planes": planes, "counts": counts, "valid": valid.astype(bool)}


def cwipc_center(pc: cwipc_pointcloud_wrapper) -> Tuple[float, float, float]:
    """Compute the center of a point cloud (reference registration/util.py:84-89): the mean of the points, summed in f64 on the device."""
    if pc.count() == 0:
        return (float('nan'), float('nan'), float('nan'))
    cen = numpy.zeros(3, dtype=numpy.float32)
    if cwipc_util_dll_load().cwipc_hip_estimate_normals(pc.as_cwipc_p(), 0.02, 30, None, None, cen.ctypes.data, 0) != 0:
        raise CwipcError("cwipc_center failed")
    return (float(cen[0]), float(cen[1]), float(cen[2]))


def cwipc_hip_estimate_normals(pc: cwipc_pointcloud_wrapper, radius: float = 0.02, max_nn: int = 30) -> Tuple[numpy.ndarray, numpy.ndarray, numpy.ndarray]:
    """Intermediate result of the direction filter: (normals float32 (n, 3) in their final orientation, neighbourhood size per point
    uint32 (n,), centroid float32 (3,)).  For parity tests."""
    n = pc.count()
    cap = max(n, 1)
    planes = numpy.zeros((3, cap), dtype=numpy.float32)
    nn = numpy.zeros(cap, dtype=numpy.uint32)
    cen = numpy.full(3, numpy.nan, dtype=numpy.float32)
    rc = cwipc_util_dll_load().cwipc_hip_estimate_normals(pc.as_cwipc_p(), float(radius), int(max_nn), planes.ctypes.data, nn.ctypes.data, cen.ctypes.data, cap)
    if rc != 0:
        raise CwipcError("cwipc_hip_estimate_normals failed")
    return numpy.ascontiguousarray(planes[:, :n].T), nn[:n], cen


def cwipc_hip_nn_distance(source: cwipc_pointcloud_wrapper, reference: cwipc_pointcloud_wrapper, nth: int = 0, max_distance: float = float('inf')) -> numpy.ndarray:
    """Per point of `source` the distance to its (nth + 1)-th nearest point of `reference`, inf when fewer than nth + 1 reference
    points lie closer than max_distance: scipy.spatial.KDTree(reference).query(source, k=[nth + 1], distance_upper_bound=max_distance)
    as the reference's registration analyzer calls it (registration/analyze.py:120-123), bit for bit -- the search runs on the
    GPU and returns squared f64 distances, the root is numpy's, on the host.  float64, shape (count(source),)."""
    if source is None or reference is None:
        raise CwipcError("cwipc_hip_nn_distance: NULL pointcloud")
    n = source.count()
    out = numpy.zeros(max(n, 1), dtype=numpy.float64)
    rc = cwipc_util_dll_load().cwipc_hip_nn_distance2(source.as_cwipc_p(), reference.as_cwipc_p(), int(nth), float(max_distance), out.ctypes.data, out.size)
    if rc != 0:
        raise CwipcError("cwipc_hip_nn_distance2 failed")
    return numpy.sqrt(out[:n])


class NNJob(ctypes.Structure):
    """One job of cwipc_hip_nn_distance_jobs (include/cwipc_util_amd/hip_ext.h: cwipc_hip_nn_job): which points of the source and of the
    reference cloud take part -- a tile mask (0: every tile) and an open y interval per side -- and the search's nth and bound.
    Keyword construction; the y limits go through _threshold, so that `y > 0.1` and `y < level` mean what numpy means by them on a
    float32 column: NNJob.ignore_floor() and NNJob.floor_only(level) give the two intervals the tooling uses."""
    _fields_ = [("source_mask", ctypes.c_uint8), ("reference_mask", ctypes.c_uint8), ("nth", ctypes.c_int32), ("max_distance", ctypes.c_double),
                ("source_y", ctypes.c_double * 2), ("reference_y", ctypes.c_double * 2)]

    def __init__(self, source_mask: int = 0, reference_mask: int = 0, nth: int = 0, max_distance: float = float('inf'),
                 source_y: Sequence[Any] = (-float('inf'), float('inf')), reference_y: Sequence[Any] = (-float('inf'), float('inf'))) -> None:
        super().__init__()
        self.source_mask = int(source_mask)
        self.reference_mask = int(reference_mask)
        self.nth = int(nth)
        self.max_distance = float(max_distance)
        self.source_y[0], self.source_y[1] = _threshold(source_y[0]), _threshold(source_y[1])
        self.reference_y[0], self.reference_y[1] = _threshold(reference_y[0]), _threshold(reference_y[1])

    @staticmethod
    def ignore_floor(level: Any = 0.1) -> Tuple[float, float]:
        """The interval of the points that are not floor: y > level."""
        return (_threshold(level), float('inf'))

    @staticmethod
    def floor_only(level: Any = 0.1) -> Tuple[float, float]:
        """The interval of cwipc_floor_filter(keep=True): y < level."""
        return (-float('inf'), _threshold(level))

    def __repr__(self) -> str:
        return (f"NNJob(source_mask={self.source_mask}, reference_mask={self.reference_mask}, nth={self.nth}, max_distance={self.max_distance}, "
                f"source_y={tuple(self.source_y)}, reference_y={tuple(self.reference_y)})")


def compact_job_rows(dist2: numpy.ndarray) -> List[numpy.ndarray]:
    """Per row of cwipc_hip_nn_distance2_jobs' result (squared distances, NaN where the source point takes no part in the row's job):
    the distances of the points that do take part, in source order, after the root."""
    return [numpy.sqrt(row[~numpy.isnan(row)]) for row in numpy.asarray(dist2, dtype=numpy.float64)]


def cwipc_hip_nn_distance_jobs(source: cwipc_pointcloud_wrapper, reference: cwipc_pointcloud_wrapper, jobs: Sequence[NNJob]) -> List[numpy.ndarray]:
    """cwipc_hip_nn_distance for a list of jobs over one pair of clouds, in one call and over one grid: per job the array that
    cwipc_hip_nn_distance(filtered source, filtered reference, job.nth, job.max_distance) returns, bit for bit, the filters being the
    job's tile masks and y intervals (NNJob).  Nothing is compacted on the device: the kernel writes NaN for a source point that
    takes no part in a job, and those entries are dropped here."""
    if source is None or reference is None:
        raise CwipcError("cwipc_hip_nn_distance_jobs: NULL pointcloud")
    jobs = list(jobs)
    table = (NNJob * max(len(jobs), 1))(*jobs)
    n = source.count()
    out = numpy.zeros((max(len(jobs), 1), max(n, 1)), dtype=numpy.float64)
    rc = cwipc_util_dll_load().cwipc_hip_nn_distance2_jobs(source.as_cwipc_p(), reference.as_cwipc_p(), ctypes.addressof(table), len(jobs), out.ctypes.data,
                                                           out.shape[1])
    if rc != 0:
        raise CwipcError("cwipc_hip_nn_distance2_jobs failed")
    return compact_job_rows(out[:len(jobs), :n])


def _matrix4(name: str, transform: Any) -> Optional[numpy.ndarray]:
    """None, or the 4x4 as contiguous float64 (the caller keeps it alive over the call)."""
    if transform is None:
        return None
    m = numpy.ascontiguousarray(numpy.asarray(transform, dtype=numpy.float64))
    if m.shape != (4, 4):
        raise ValueError(f"{name}: transform must be a 4x4 matrix")
    return m


def _p(a: Optional[numpy.ndarray]) -> Optional[int]:
    return None if a is None else a.ctypes.data


def cwipc_hip_correspondences(source: cwipc_pointcloud_wrapper, reference: cwipc_pointcloud_wrapper, transform: Any = None,
                              max_distance: float = float('inf')) -> Tuple[numpy.ndarray, numpy.ndarray]:
    """Per point of `source`, moved by the 4x4 `transform` (None: the identity) in f64, the index of its nearest point of `reference`
    (uint32, 0xFFFFFFFF: none) and the squared f64 distance (inf: none), among the reference points strictly closer than
    max_distance; among equally distant ones the smallest index.  The search of one ICP iteration, on the GPU."""
    if source is None or reference is None:
        raise CwipcError("cwipc_hip_correspondences: NULL pointcloud")
    m = _matrix4('cwipc_hip_correspondences', transform)
    n = source.count()
    idx = numpy.zeros(max(n, 1), dtype=numpy.uint32)
    d2 = numpy.zeros(max(n, 1), dtype=numpy.float64)
    rc = cwipc_util_dll_load().cwipc_hip_correspondences(source.as_cwipc_p(), reference.as_cwipc_p(), _p(m), float(max_distance), idx.ctypes.data, d2.ctypes.data,
                                                         idx.size)
    if rc != 0:
        raise CwipcError("cwipc_hip_correspondences failed")
    return idx[:n], d2[:n]


def cwipc_hip_icp_sums(source: cwipc_pointcloud_wrapper, reference: cwipc_pointcloud_wrapper, transform: Any = None, max_distance: float = float('inf'),
                       cp: Any = None, cq: Any = None) -> Tuple[int, numpy.ndarray]:
    """One correspondence search and the sums of a rigid fit over the matched pairs, nothing per point leaves the device: (n, sums)
    with sums = sum a (3) | sum b (3) | sum a b^T (9) | sum d2, a = moved source point - cp, b = matched reference point - cq
    (None: no pivot).  With the identity, n / count(source) and sqrt(sums[15] / n) are open3d's evaluate_registration."""
    if source is None or reference is None:
        raise CwipcError("cwipc_hip_icp_sums: NULL pointcloud")
    m = _matrix4('cwipc_hip_icp_sums', transform)
    pivots = [None if v is None else numpy.ascontiguousarray(numpy.asarray(v, dtype=numpy.float64).reshape(3)) for v in (cp, cq)]
    n = ctypes.c_uint64(0)
    sums = numpy.zeros(16, dtype=numpy.float64)
    rc = cwipc_util_dll_load().cwipc_hip_icp_sums(source.as_cwipc_p(), reference.as_cwipc_p(), _p(m), float(max_distance), _p(pivots[0]), _p(pivots[1]),
                                                  ctypes.addressof(n), sums.ctypes.data)
    if rc != 0:
        raise CwipcError("cwipc_hip_icp_sums failed")
    return int(n.value), sums


def cwipc_hip_icp_point2point(source: cwipc_pointcloud_wrapper, reference: cwipc_pointcloud_wrapper, max_distance: float, init: Any = None,
                              relative_fitness: float = 1e-6, relative_rmse: float = 1e-6, max_iteration: int = 30) -> Tuple[numpy.ndarray, float, float, int]:
    """open3d's registration_icp with the point-to-point estimate, on the GPU: (transformation 4x4 float64, fitness, inlier_rmse,
    iterations done).  The defaults are open3d's ICPConvergenceCriteria."""
    if source is None or reference is None:
        raise CwipcError("cwipc_hip_icp_point2point: NULL pointcloud")
    m = _matrix4('cwipc_hip_icp_point2point', init)
    T = numpy.zeros((4, 4), dtype=numpy.float64)
    fitness, rmse, iterations = ctypes.c_double(0.0), ctypes.c_double(0.0), ctypes.c_int(0)
    rc = cwipc_util_dll_load().cwipc_hip_icp_point2point(source.as_cwipc_p(), reference.as_cwipc_p(), float(max_distance), _p(m), float(relative_fitness),
                                                         float(relative_rmse), int(max_iteration), T.ctypes.data, ctypes.addressof(fitness),
                                                         ctypes.addressof(rmse), ctypes.addressof(iterations))
    if rc != 0:
        raise CwipcError("cwipc_hip_icp_point2point failed")
    return T, float(fitness.value), float(rmse.value), int(iterations.value)


def _normal_planes(name: str, normals: Any, reference: cwipc_pointcloud_wrapper) -> Optional[numpy.ndarray]:
    """None, or a cloud's normals (the reference's for point-to-plane, either cloud's for generalized ICP), given as (count, 3), as
    three contiguous float32 planes (the caller keeps them alive over the call)."""
    if normals is None:
        return None
    m = numpy.asarray(normals, dtype=numpy.float32)
    if m.shape != (reference.count(), 3):
        raise ValueError(f"{name}: normals must have the shape (count, 3) of their cloud")
    return numpy.ascontiguousarray(m.T)


def cwipc_hip_icp_plane_sums(source: cwipc_pointcloud_wrapper, reference: cwipc_pointcloud_wrapper, transform: Any = None, max_distance: float = float('inf'),
                             normals: Any = None, radius: float = 0.02, max_nn: int = 30) -> Tuple[int, numpy.ndarray]:
    """One correspondence search and the sums of a point-to-plane fit over the matched pairs, nothing per point leaves the device:
    (n, sums) with sums = sum J_i J_j for i <= j (21) | sum J_i r (6) | sum r^2 | sum d2, J = (p x m, m), r = (p - q) . m for the
    moved source point p, its correspondence q and q's normal m.  normals: the reference cloud's, float32 (count(reference), 3) as
    cwipc_hip_estimate_normals returns them, or None: estimated on the device with (radius, max_nn).  Their sign does not matter:
    negating a normal leaves every term's bits unchanged (the reference's _fix_normal_direction has nothing to fix here)."""
    if source is None or reference is None:
        raise CwipcError("cwipc_hip_icp_plane_sums: NULL pointcloud")
    m = _matrix4('cwipc_hip_icp_plane_sums', transform)
    planes = _normal_planes('cwipc_hip_icp_plane_sums', normals, reference)
    n = ctypes.c_uint64(0)
    sums = numpy.zeros(29, dtype=numpy.float64)
    rc = cwipc_util_dll_load().cwipc_hip_icp_plane_sums(source.as_cwipc_p(), reference.as_cwipc_p(), _p(m), float(max_distance), _p(planes), float(radius),
                                                        int(max_nn), ctypes.addressof(n), sums.ctypes.data)
    if rc != 0:
        raise CwipcError("cwipc_hip_icp_plane_sums failed")
    return int(n.value), sums


def cwipc_hip_icp_point2plane(source: cwipc_pointcloud_wrapper, reference: cwipc_pointcloud_wrapper, max_distance: float, init: Any = None,
                              normals: Any = None, radius: float = 0.02, max_nn: int = 30, relative_fitness: float = 1e-6, relative_rmse: float = 1e-6,
                              max_iteration: int = 30) -> Tuple[numpy.ndarray, float, float, int]:
    """open3d's registration_icp with the point-to-plane estimate, on the GPU: (transformation 4x4 float64, fitness, inlier_rmse,
    iterations done).  normals, radius, max_nn as for cwipc_hip_icp_plane_sums: only the reference cloud has normals, estimated once
    per run when none are given, and their orientation does not matter.  The criteria's defaults are open3d's."""
    if source is None or reference is None:
        raise CwipcError("cwipc_hip_icp_point2plane: NULL pointcloud")
    m = _matrix4('cwipc_hip_icp_point2plane', init)
    planes = _normal_planes('cwipc_hip_icp_point2plane', normals, reference)
    T = numpy.zeros((4, 4), dtype=numpy.float64)
    fitness, rmse, iterations = ctypes.c_double(0.0), ctypes.c_double(0.0), ctypes.c_int(0)
    rc = cwipc_util_dll_load().cwipc_hip_icp_point2plane(source.as_cwipc_p(), reference.as_cwipc_p(), float(max_distance), _p(m), _p(planes), float(radius),
                                                         int(max_nn), float(relative_fitness), float(relative_rmse), int(max_iteration), T.ctypes.data,
                                                         ctypes.addressof(fitness), ctypes.addressof(rmse), ctypes.addressof(iterations))
    if rc != 0:
        raise CwipcError("cwipc_hip_icp_point2plane failed")
    return T, float(fitness.value), float(rmse.value), int(iterations.value)


def cwipc_hip_gicp_covariances(pc: cwipc_pointcloud_wrapper, normals: Any = None, radius: float = 0.02, max_nn: int = 30, direction: Any = None,
                               epsilon: float = 1e-3) -> numpy.ndarray:
    """Intermediate result of generalized ICP: per point the covariance Rx diag(epsilon, 1, 1) Rx^T of its normal, as the six values
    00, 01, 02, 11, 12, 22, float64 (count, 6).  normals: float32 (count, 3), or None: estimated on the device with (radius, max_nn).
    direction: three numbers the normals are turned to face first (a zero normal becomes the direction), or None: no turning.
    For parity tests."""
    if pc is None:
        raise CwipcError("cwipc_hip_gicp_covariances: NULL pointcloud")
    planes = _normal_planes('cwipc_hip_gicp_covariances', normals, pc)
    d = None if direction is None else numpy.ascontiguousarray(numpy.asarray(direction, dtype=numpy.float64).reshape(3))
    n = pc.count()
    cov = numpy.zeros((max(n, 1), 6), dtype=numpy.float64)
    rc = cwipc_util_dll_load().cwipc_hip_gicp_covariances(pc.as_cwipc_p(), _p(planes), float(radius), int(max_nn), _p(d), float(epsilon), cov.ctypes.data,
                                                          len(cov))
    if rc != 0:
        raise CwipcError("cwipc_hip_gicp_covariances failed")
    return cov[:n]


def cwipc_hip_icp_gicp_sums(source: cwipc_pointcloud_wrapper, reference: cwipc_pointcloud_wrapper, transform: Any = None, max_distance: float = float('inf'),
                            source_normals: Any = None, reference_normals: Any = None, radius: float = 0.02, max_nn: int = 30,
                            epsilon: float = 1e-3) -> Tuple[int, numpy.ndarray]:
    """One correspondence search and the sums of a generalized ICP fit over the matched pairs, nothing per point leaves the device:
    (n, sums) with sums = sum (A^T N A)_ij for i <= j (21) | sum (A^T g)_i (6) | sum e^T g | sum d2, where A = [-skew(p) | I],
    N = (Ct + R Cs R^T)^-1, e = p - q, g = N e for the moved source point p, its correspondence q and their covariances Cs, Ct.
    Each cloud's normals: float32 (count, 3), or None: estimated on the device with (radius, max_nn).  They are turned as the
    reference's _fix_normal_direction turns them before the covariances are taken."""
    if source is None or reference is None:
        raise CwipcError("cwipc_hip_icp_gicp_sums: NULL pointcloud")
    m = _matrix4('cwipc_hip_icp_gicp_sums', transform)
    ps = _normal_planes('cwipc_hip_icp_gicp_sums', source_normals, source)
    pr = _normal_planes('cwipc_hip_icp_gicp_sums', reference_normals, reference)
    n = ctypes.c_uint64(0)
    sums = numpy.zeros(29, dtype=numpy.float64)
    rc = cwipc_util_dll_load().cwipc_hip_icp_gicp_sums(source.as_cwipc_p(), reference.as_cwipc_p(), _p(m), float(max_distance), _p(ps), _p(pr), float(radius),
                                                       int(max_nn), float(epsilon), ctypes.addressof(n), sums.ctypes.data)
    if rc != 0:
        raise CwipcError("cwipc_hip_icp_gicp_sums failed")
    return int(n.value), sums


def cwipc_hip_icp_generalized(source: cwipc_pointcloud_wrapper, reference: cwipc_pointcloud_wrapper, max_distance: float, init: Any = None,
                              source_normals: Any = None, reference_normals: Any = None, radius: float = 0.02, max_nn: int = 30, epsilon: float = 1e-3,
                              relative_fitness: float = 1e-6, relative_rmse: float = 1e-6, max_iteration: int = 30) -> Tuple[numpy.ndarray, float, float, int]:
    """open3d's registration_generalized_icp, on the GPU: (transformation 4x4 float64, fitness, inlier_rmse, iterations done).
    The normals, radius, max_nn and epsilon as for cwipc_hip_icp_gicp_sums: both clouds have normals, estimated once per run when
    none are given.  The criteria's defaults are open3d's."""
    if source is None or reference is None:
        raise CwipcError("cwipc_hip_icp_generalized: NULL pointcloud")
    m = _matrix4('cwipc_hip_icp_generalized', init)
    ps = _normal_planes('cwipc_hip_icp_generalized', source_normals, source)
    pr = _normal_planes('cwipc_hip_icp_generalized', reference_normals, reference)
    T = numpy.zeros((4, 4), dtype=numpy.float64)
    fitness, rmse, iterations = ctypes.c_double(0.0), ctypes.c_double(0.0), ctypes.c_int(0)
    rc = cwipc_util_dll_load().cwipc_hip_icp_generalized(source.as_cwipc_p(), reference.as_cwipc_p(), float(max_distance), _p(m), _p(ps), _p(pr), float(radius),
                                                         int(max_nn), float(epsilon), float(relative_fitness), float(relative_rmse), int(max_iteration),
                                                         T.ctypes.data, ctypes.addressof(fitness), ctypes.addressof(rmse), ctypes.addressof(iterations))
    if rc != 0:
        raise CwipcError("cwipc_hip_icp_generalized failed")
    return T, float(fitness.value), float(rmse.value), int(iterations.value)


CWIPC_HIP_DISTORTION_NO_PLANE = 1


class cwipc_hip_distortion_sums(ctypes.Structure):
    """One direction of cwipc_hip_distortion (include/cwipc_util_amd/hip_ext.h, RULE Q): the pass's source points, the matched pairs,
    those with a normal; over the matched pairs the sum and the maximum of d2, the sum of the squared point-to-plane residuals, of
    the squared colour differences in RGB (integers) and in BT.709 YUV."""
    _fields_ = [("n_source", ctypes.c_uint64), ("n", ctypes.c_uint64), ("n_plane", ctypes.c_uint64),
                ("sum_d2", ctypes.c_double), ("max_d2", ctypes.c_double), ("sum_r2", ctypes.c_double),
                ("sum_rgb2", ctypes.c_uint64 * 3), ("sum_yuv2", ctypes.c_double * 3)]


def cwipc_hip_distortion(original: cwipc_pointcloud_wrapper, degraded: cwipc_pointcloud_wrapper, max_distance: float = float('inf'), normals: Any = None,
                         radius: float = 0.02, max_nn: int = 30, plane: bool = True) -> Tuple[cwipc_hip_distortion_sums, cwipc_hip_distortion_sums]:
    """What `degraded` lost against `original`, nothing per point leaves the device: (forward, backward) sums of RULE Q -- forward
    matches every point of the original to its nearest point of the degraded cloud, backward the other way round, among the points
    strictly closer than max_distance.  normals: the ORIGINAL's, float32 (count(original), 3) as cwipc_hip_estimate_normals returns
    them, or None: estimated on the device with (radius, max_nn); a degraded point inherits the normal of its nearest original point.
    plane=False: no normals are made or read (n_plane and sum_r2 are 0).  cwipc_util_amd.quality turns the sums into mse and PSNR."""
    if original is None or degraded is None:
        raise CwipcError("cwipc_hip_distortion: NULL pointcloud")
    planes = _normal_planes('cwipc_hip_distortion', normals, original) if plane else None
    out = (cwipc_hip_distortion_sums * 2)()
    rc = cwipc_util_dll_load().cwipc_hip_distortion(original.as_cwipc_p(), degraded.as_cwipc_p(), float(max_distance), _p(planes), float(radius), int(max_nn),
                                                    0 if plane else CWIPC_HIP_DISTORTION_NO_PLANE, ctypes.addressof(out))
    if rc != 0:
        raise CwipcError("cwipc_hip_distortion failed")
    return cwipc_hip_distortion_sums.from_buffer_copy(out[0]), cwipc_hip_distortion_sums.from_buffer_copy(out[1])


def cwipc_hip_gaussian_kde(samples: Any, at: Any, bw_method: Union[None, str, float] = None) -> numpy.ndarray:
    """scipy.stats.gaussian_kde(samples, bw_method).evaluate(at) for one-dimensional samples, the sum on the GPU: the bandwidth is
    h = std(samples, ddof=1) * factor, factor = n**-0.2 (None, 'scott'), (n * 3 / 4)**-0.2 ('silverman') or the number given."""
    s = numpy.ascontiguousarray(numpy.asarray(samples, dtype=numpy.float64).reshape(-1))
    x = numpy.ascontiguousarray(numpy.asarray(at, dtype=numpy.float64).reshape(-1))
    n = s.size
    if n < 2:
        raise CwipcError("cwipc_hip_gaussian_kde: needs at least two samples")
    if bw_method is None or bw_method == 'scott':
        factor = float(n) ** -0.2
    elif bw_method == 'silverman':
        factor = (float(n) * 3.0 / 4.0) ** -0.2
    elif numpy.isscalar(bw_method) and not isinstance(bw_method, str):
        factor = float(bw_method)
    else:
        raise ValueError("bw_method should be 'scott', 'silverman' or a scalar")
    h = float(numpy.std(s, ddof=1)) * factor
    out = numpy.zeros(max(x.size, 1), dtype=numpy.float64)
    rc = cwipc_util_dll_load().cwipc_hip_gaussian_kde(s.ctypes.data, n, h, x.ctypes.data, x.size, out.ctypes.data)
    if rc != 0:
        raise CwipcError("cwipc_hip_gaussian_kde failed")
    return out[:x.size]


def cwipc_hip_from_device_aos(dev_ptr: int, npoint: int, timestamp: int, cellsize: float) -> cwipc_pointcloud_wrapper:
    """New cloud from npoint cwipc_point records at a DEVICE address (e.g. torch tensor .data_ptr())."""
    rv = cwipc_util_dll_load().cwipc_hip_from_device_aos(dev_ptr, npoint, timestamp, cellsize)
    return _wrap_filter_result('cwipc_hip_from_device_aos', rv)


def cwipc_hip_from_device_slots(dev_ptr: int, slot_rows: int, header_rows: int, counts: List[int], timestamp: int, cellsize: float,
                                stream: Optional[int] = None) -> cwipc_pointcloud_wrapper:
    """New cloud from the receive buffer of an all-gather at a DEVICE address: len(counts) slots of slot_rows
    16-byte rows, the records of slot s in rows [header_rows, header_rows + counts[s]); slot order = point order.
    stream (a hipStream_t as an integer, e.g. torch.cuda.current_stream().cuda_stream): run as a step of that stream
    and return without waiting."""
    arr = (ctypes.c_uint32 * len(counts))(*counts)
    if stream is None:
        rv = cwipc_util_dll_load().cwipc_hip_from_device_slots(dev_ptr, len(counts), slot_rows, header_rows, arr, timestamp, cellsize)
    else:
        rv = cwipc_util_dll_load().cwipc_hip_from_device_slots_on_stream(dev_ptr, len(counts), slot_rows, header_rows, arr, timestamp, cellsize, stream)
    return _wrap_filter_result('cwipc_hip_from_device_slots', rv)


def cwipc_hip_copy_device_aos(pc: cwipc_pointcloud_wrapper, dev_ptr: int, size: int, stream: Optional[int] = None) -> int:
    """Interleave the cloud into a DEVICE buffer of `size` bytes; returns the number of points.  stream (a hipStream_t
    as an integer): run as a step of that stream and return without waiting."""
    if stream is None:
        n = cwipc_util_dll_load().cwipc_hip_copy_device_aos(pc.as_cwipc_p(), dev_ptr, size)
    else:
        n = cwipc_util_dll_load().cwipc_hip_copy_device_aos_on_stream(pc.as_cwipc_p(), dev_ptr, size, stream)
    if n < 0:
        raise CwipcError("cwipc_hip_copy_device_aos failed")
    return n


# ---------------------------------------------------------------------------
# the octree codec's C boundary (hip_ext.h: RULE C).  Its packets are NOT interoperable with cwipc_codec; cwipc_util_amd.codec
# wraps these handles in the classes the reference's callers use.
# ---------------------------------------------------------------------------
class cwipc_hip_encoder_params(ctypes.Structure):
    """The reference's cwipc_encoder_params, fields in the order its callers pass them."""
    _fields_ = [("do_inter_frame", ctypes.c_bool), ("gop_size", ctypes.c_int), ("exp_factor", ctypes.c_float), ("octree_bits", ctypes.c_int),
                ("jpeg_quality", ctypes.c_int), ("macroblock_size", ctypes.c_int), ("tilenumber", ctypes.c_int), ("voxelsize", ctypes.c_float)]


class cwipc_hip_codec_info(ctypes.Structure):
    """A valid packet's header and where its parts lie."""
    _fields_ = [("timestamp", ctypes.c_uint64), ("nleaves", ctypes.c_uint32), ("octree_bits", ctypes.c_int32), ("colour_bits", ctypes.c_int32),
                ("tile_mode", ctypes.c_int32), ("tile_value", ctypes.c_int32), ("min", ctypes.c_float * 3), ("side", ctypes.c_double),
                ("nodes", ctypes.c_uint32 * 16), ("occupancy_offset", ctypes.c_uint64), ("colour_offset", ctypes.c_uint64),
                ("tile_offset", ctypes.c_uint64), ("total_bytes", ctypes.c_uint64)]


class cwipc_hip_codec_entropy_directory(ctypes.Structure):
    """The directory of an entropy-coded packet (hip_ext.h: RULE E): the header of the packet it stands for, and per stream its kind
    (0 occupancy, 1 colour, 2 tile), mode (0 raw, 1 coded), symbol count and payload."""
    _fields_ = [("packet", cwipc_hip_codec_info), ("nstreams", ctypes.c_int32), ("kind", ctypes.c_int32 * 20), ("which", ctypes.c_int32 * 20),
                ("mode", ctypes.c_int32 * 20), ("symbols", ctypes.c_uint32 * 20), ("payload_offset", ctypes.c_uint64 * 20),
                ("payload_bytes", ctypes.c_uint64 * 20), ("total_bytes", ctypes.c_uint64)]


class cwipc_hip_codec_transform_directory(ctypes.Structure):
    """The directory of a transform-coded packet (hip_ext.h: RULE T): the header of the packet it stands for, the quantiser scale, the
    root's values, the escape counts, and per stream its kind (0 occupancy, 2 tile, 3 tokens, 5 escapes), mode, symbol count and payload."""
    _fields_ = [("packet", cwipc_hip_codec_info), ("q16", ctypes.c_uint32), ("dc", ctypes.c_int32 * 3), ("nescapes", ctypes.c_uint32 * 3),
                ("nstreams", ctypes.c_int32), ("kind", ctypes.c_int32 * 23), ("which", ctypes.c_int32 * 23), ("mode", ctypes.c_int32 * 23),
                ("symbols", ctypes.c_uint32 * 23), ("payload_offset", ctypes.c_uint64 * 23), ("payload_bytes", ctypes.c_uint64 * 23),
                ("total_bytes", ctypes.c_uint64)]


class cwipc_hip_codec_inter_directory(ctypes.Structure):
    """An inter-frame packet (hip_ext.h: RULE P) after the container test: the prefix, the header of the packet it stands for, and
    for a delta packet the added leaves' counts and the directory of its streams."""
    _fields_ = [("kind", ctypes.c_uint32), ("gop_index", ctypes.c_uint32), ("ref_timestamp", ctypes.c_uint64), ("ref_nleaves", ctypes.c_uint32),
                ("embedded_entropy", ctypes.c_int32), ("packet", cwipc_hip_codec_info), ("nadded", ctypes.c_uint32), ("nodes_added", ctypes.c_uint32 * 16),
                ("nstreams", ctypes.c_int32), ("kind_of", ctypes.c_int32 * 21), ("which", ctypes.c_int32 * 21), ("mode", ctypes.c_int32 * 21),
                ("symbols", ctypes.c_uint32 * 21), ("payload_offset", ctypes.c_uint64 * 21), ("payload_bytes", ctypes.c_uint64 * 21),
                ("total_bytes", ctypes.c_uint64)]


def _codec_handle(name: str, rv: Any, errorString: ctypes.c_char_p) -> int:
    _raise_or_warn(errorString, rv)
    if rv:
        return rv
    raise CwipcError(f"{name}: nothing created, but no specific error returned from C library")


def _codec_last_error(name: str) -> CwipcError:
    detail = cwipc_util_dll_load().cwipc_hip_last_error()
    return CwipcError(f"{name} failed" + (f": {detail.decode('utf8')}" if detail else ""))


def cwipc_hip_new_encoder(params: cwipc_hip_encoder_params) -> int:
    """An encoder handle; CwipcError with the library's message for a parameter set it refuses."""
    errorString = ctypes.c_char_p()
    rv = cwipc_util_dll_load().cwipc_hip_new_encoder(ctypes.addressof(params), ctypes.byref(errorString))
    return _codec_handle('cwipc_hip_new_encoder', rv, errorString)


def cwipc_hip_encoder_free(enc: int) -> None:
    cwipc_util_dll_load().cwipc_hip_encoder_free(enc)


def cwipc_hip_encoder_feed(enc: int, pc: cwipc_pointcloud_wrapper) -> None:
    if cwipc_util_dll_load().cwipc_hip_encoder_feed(enc, pc.as_cwipc_p()) != 0:
        raise _codec_last_error('cwipc_hip_encoder_feed')


def cwipc_hip_encoder_available(enc: int, wait: bool) -> bool:
    return bool(cwipc_util_dll_load().cwipc_hip_encoder_available(enc, wait))


def cwipc_hip_encoder_get_encoded_size(enc: int) -> int:
    return cwipc_util_dll_load().cwipc_hip_encoder_get_encoded_size(enc)


def cwipc_hip_encoder_copy_data(enc: int, buffer: Any, size: int) -> bool:
    """The oldest packet into a writable ctypes buffer of at least `size` bytes; it leaves the queue."""
    return bool(cwipc_util_dll_load().cwipc_hip_encoder_copy_data(enc, ctypes.addressof(buffer), size))


def cwipc_hip_encoder_at_gop_boundary(enc: int) -> bool:
    return bool(cwipc_util_dll_load().cwipc_hip_encoder_at_gop_boundary(enc))


def cwipc_hip_encoder_eof(enc: int) -> bool:
    return bool(cwipc_util_dll_load().cwipc_hip_encoder_eof(enc))


def cwipc_hip_encoder_close(enc: int) -> None:
    cwipc_util_dll_load().cwipc_hip_encoder_close(enc)


def cwipc_hip_new_encodergroup() -> int:
    errorString = ctypes.c_char_p()
    rv = cwipc_util_dll_load().cwipc_hip_new_encodergroup(ctypes.byref(errorString))
    return _codec_handle('cwipc_hip_new_encodergroup', rv, errorString)


def cwipc_hip_encodergroup_addencoder(group: int, params: cwipc_hip_encoder_params) -> int:
    """A new encoder that belongs to the group (and is freed with it)."""
    errorString = ctypes.c_char_p()
    rv = cwipc_util_dll_load().cwipc_hip_encodergroup_addencoder(group, ctypes.addressof(params), ctypes.byref(errorString))
    return _codec_handle('cwipc_hip_encodergroup_addencoder', rv, errorString)


def cwipc_hip_encodergroup_feed(group: int, pc: cwipc_pointcloud_wrapper) -> None:
    if cwipc_util_dll_load().cwipc_hip_encodergroup_feed(group, pc.as_cwipc_p()) != 0:
        raise _codec_last_error('cwipc_hip_encodergroup_feed')


def cwipc_hip_encodergroup_close(group: int) -> None:
    cwipc_util_dll_load().cwipc_hip_encodergroup_close(group)


def cwipc_hip_encodergroup_free(group: int) -> None:
    cwipc_util_dll_load().cwipc_hip_encodergroup_free(group)


def cwipc_hip_new_decoder() -> int:
    errorString = ctypes.c_char_p()
    rv = cwipc_util_dll_load().cwipc_hip_new_decoder(ctypes.byref(errorString))
    return _codec_handle('cwipc_hip_new_decoder', rv, errorString)


def cwipc_hip_decoder_feed(dec: int, packet: Union[bytes, bytearray, memoryview]) -> None:
    """CwipcError with the validator's reason for a packet that is not valid: nothing reaches the device then."""
    data = bytes(packet)
    if cwipc_util_dll_load().cwipc_hip_decoder_feed(dec, data, len(data)) != 0:
        raise _codec_last_error('cwipc_hip_decoder_feed')


def cwipc_hip_decoder_set_max_octree_bits(dec: int, bits: int) -> None:
    """The decoder hands out clouds of at most `bits` octree bits from its next feed on (hip_ext.h: RULE L); 0: off.  CwipcError for
    anything but 0..16."""
    if cwipc_util_dll_load().cwipc_hip_decoder_set_max_octree_bits(dec, int(bits)) != 0:
        raise _codec_last_error('cwipc_hip_decoder_set_max_octree_bits')


def cwipc_hip_codec_lod(packet: Union[bytes, bytearray, memoryview], bits: int) -> bytearray:
    """The cut L(P, bits) of a "cwao" packet, or of a "cwae" packet in that form (hip_ext.h: RULE L; host code, no GPU); CwipcError with
    the reason for a packet or a `bits` that is refused."""
    data = bytes(packet)
    capacity = len(data) + 4 + 11 * 20
    for _ in range(2):
        out = bytearray(capacity)
        buffer = (ctypes.c_char * len(out)).from_buffer(out)
        errorString = ctypes.c_char_p()
        size = cwipc_util_dll_load().cwipc_hip_codec_lod(data, len(data), int(bits), ctypes.addressof(buffer), len(out), ctypes.byref(errorString))
        del buffer
        if size == 0:
            raise CwipcError(errorString.value.decode('utf8') if errorString.value else "cwipc_hip_codec_lod: not a valid packet")
        if size <= len(out):
            del out[size:]
            return out
        capacity = size   # (an entropy-coded cut that is larger than the packet it was cut from)
    raise CwipcError("cwipc_hip_codec_lod: the size of the result changed between two calls")


def cwipc_hip_decoder_available(dec: int, wait: bool) -> bool:
    return bool(cwipc_util_dll_load().cwipc_hip_decoder_available(dec, wait))


def cwipc_hip_decoder_get(dec: int) -> Optional[cwipc_pointcloud_wrapper]:
    rv = cwipc_util_dll_load().cwipc_hip_decoder_get(dec)
    return cwipc_pointcloud_wrapper(rv) if rv else None


def cwipc_hip_decoder_eof(dec: int) -> bool:
    return bool(cwipc_util_dll_load().cwipc_hip_decoder_eof(dec))


def cwipc_hip_decoder_close(dec: int) -> None:
    cwipc_util_dll_load().cwipc_hip_decoder_close(dec)


def cwipc_hip_decoder_free(dec: int) -> None:
    cwipc_util_dll_load().cwipc_hip_decoder_free(dec)


def cwipc_hip_codec_packet_info(packet: Union[bytes, bytearray, memoryview]) -> cwipc_hip_codec_info:
    """The validity test and the header of a packet, on the host (no GPU needed); CwipcError with the reason for one that is not valid."""
    data = bytes(packet)
    info = cwipc_hip_codec_info()
    errorString = ctypes.c_char_p()
    rv = cwipc_util_dll_load().cwipc_hip_codec_packet_info(data, len(data), ctypes.addressof(info), ctypes.byref(errorString))
    if rv != 0:
        raise CwipcError(errorString.value.decode('utf8') if errorString.value else "cwipc_hip_codec_packet_info: not a valid packet")
    return info


def cwipc_hip_encoder_set_entropy(enc: int, on: bool) -> None:
    """The encoder delivers the entropy-coded form (hip_ext.h: RULE E) from its first packet on; CwipcError once it has been fed."""
    if cwipc_util_dll_load().cwipc_hip_encoder_set_entropy(enc, 1 if on else 0) != 0:
        raise _codec_last_error('cwipc_hip_encoder_set_entropy')


def _codec_entropy_convert(name: str, packet: Union[bytes, bytearray, memoryview], capacity: int) -> bytearray:
    data = bytes(packet)
    out = bytearray(max(capacity, 1))
    buffer = (ctypes.c_char * len(out)).from_buffer(out)
    errorString = ctypes.c_char_p()
    size = getattr(cwipc_util_dll_load(), name)(data, len(data), ctypes.addressof(buffer), len(out), ctypes.byref(errorString))
    del buffer
    if size == 0 or size > len(out):
        raise CwipcError(errorString.value.decode('utf8') if errorString.value else f"{name}: not a valid packet")
    del out[size:]
    return out


def cwipc_hip_codec_entropy_pack(packet: Union[bytes, bytearray, memoryview]) -> bytearray:
    """A valid "cwao" packet in its entropy-coded form "cwae" (host code, no GPU)."""
    return _codec_entropy_convert('cwipc_hip_codec_entropy_pack', packet, len(packet) + 4 + 11 * 20)


def cwipc_hip_codec_entropy_info(packet: Union[bytes, bytearray, memoryview]) -> cwipc_hip_codec_entropy_directory:
    """The container test and the directory of a "cwae" packet (host code, no GPU; the coded blocks are not decoded)."""
    data = bytes(packet)
    info = cwipc_hip_codec_entropy_directory()
    errorString = ctypes.c_char_p()
    rv = cwipc_util_dll_load().cwipc_hip_codec_entropy_info(data, len(data), ctypes.addressof(info), ctypes.byref(errorString))
    if rv != 0:
        raise CwipcError(errorString.value.decode('utf8') if errorString.value else "cwipc_hip_codec_entropy_info: not a valid packet")
    return info


def cwipc_hip_codec_entropy_unpack(packet: Union[bytes, bytearray, memoryview]) -> bytearray:
    """The "cwao" packet a "cwae" packet stands for (host code, no GPU); CwipcError with the reason for one that is refused."""
    return _codec_entropy_convert('cwipc_hip_codec_entropy_unpack', packet, cwipc_hip_codec_entropy_info(packet).packet.total_bytes)


def cwipc_hip_encoder_set_colour_transform(enc: int, on: bool) -> None:
    """The encoder delivers the transform-coded form (hip_ext.h: RULE T) from its first packet on; CwipcError once it has been fed, and
    for an inter-mode encoder."""
    if cwipc_util_dll_load().cwipc_hip_encoder_set_colour_transform(enc, 1 if on else 0) != 0:
        raise _codec_last_error('cwipc_hip_encoder_set_colour_transform')


def cwipc_hip_codec_transform_pack(packet: Union[bytes, bytearray, memoryview], jpeg_quality: int) -> bytearray:
    """A valid "cwao" packet with 8 colour bits in its transform-coded form "cwat" at `jpeg_quality` (host code, no GPU)."""
    data = bytes(packet)
    out = bytearray(3 * len(data) + 300)
    buffer = (ctypes.c_char * len(out)).from_buffer(out)
    errorString = ctypes.c_char_p()
    size = cwipc_util_dll_load().cwipc_hip_codec_transform_pack(data, len(data), int(jpeg_quality), ctypes.addressof(buffer), len(out), ctypes.byref(errorString))
    del buffer
    if size == 0 or size > len(out):
        raise CwipcError(errorString.value.decode('utf8') if errorString.value else "cwipc_hip_codec_transform_pack: not a valid packet")
    del out[size:]
    return out


def cwipc_hip_codec_transform_info(packet: Union[bytes, bytearray, memoryview]) -> cwipc_hip_codec_transform_directory:
    """The container test and the directory of a "cwat" packet (host code, no GPU; the coded blocks are not decoded)."""
    data = bytes(packet)
    info = cwipc_hip_codec_transform_directory()
    errorString = ctypes.c_char_p()
    rv = cwipc_util_dll_load().cwipc_hip_codec_transform_info(data, len(data), ctypes.addressof(info), ctypes.byref(errorString))
    if rv != 0:
        raise CwipcError(errorString.value.decode('utf8') if errorString.value else "cwipc_hip_codec_transform_info: not a valid packet")
    return info


def cwipc_hip_codec_transform_unpack(packet: Union[bytes, bytearray, memoryview]) -> bytearray:
    """The "cwao" packet a "cwat" packet stands for (host code, no GPU); CwipcError with the reason for one that is refused."""
    return _codec_entropy_convert('cwipc_hip_codec_transform_unpack', packet, cwipc_hip_codec_transform_info(packet).packet.total_bytes)


def _codec_inter_convert(name: str, args: tuple, capacity: int) -> bytearray:
    out = bytearray(max(capacity, 1))
    buffer = (ctypes.c_char * len(out)).from_buffer(out)
    errorString = ctypes.c_char_p()
    size = getattr(cwipc_util_dll_load(), name)(*args, ctypes.addressof(buffer), len(out), ctypes.byref(errorString))
    del buffer
    if size == 0 or size > len(out):
        raise CwipcError(errorString.value.decode('utf8') if errorString.value else f"{name}: not a valid packet")
    del out[size:]
    return out


def cwipc_hip_codec_inter_pack(reference: Union[bytes, bytearray, memoryview], packet: Union[bytes, bytearray, memoryview], gop_index: int) -> bytearray:
    """The delta packet (hip_ext.h: RULE P) of the "cwao" packet `packet` against the "cwao" packet `reference` (host code, no GPU)."""
    r, p = bytes(reference), bytes(packet)
    return _codec_inter_convert('cwipc_hip_codec_inter_pack', (r, len(r), p, len(p), gop_index), len(p) + len(r) // 8 + 256)


def cwipc_hip_codec_inter_info(packet: Union[bytes, bytearray, memoryview]) -> cwipc_hip_codec_inter_directory:
    """The container test and the directory of a "cwap" packet (host code, no GPU; the coded blocks are not decoded)."""
    data = bytes(packet)
    info = cwipc_hip_codec_inter_directory()
    errorString = ctypes.c_char_p()
    rv = cwipc_util_dll_load().cwipc_hip_codec_inter_info(data, len(data), ctypes.addressof(info), ctypes.byref(errorString))
    if rv != 0:
        raise CwipcError(errorString.value.decode('utf8') if errorString.value else "cwipc_hip_codec_inter_info: not a valid packet")
    return info


def cwipc_hip_codec_inter_unpack(reference: Optional[Union[bytes, bytearray, memoryview]], packet: Union[bytes, bytearray, memoryview]) -> bytearray:
    """The "cwao" packet a "cwap" packet stands for after `reference` (host code, no GPU); a key packet's embedded packet verbatim
    (`reference` may be None); CwipcError with the reason for a packet that is refused."""
    r, d = (bytes(reference) if reference is not None else None), bytes(packet)
    info = cwipc_hip_codec_inter_info(d)
    h = info.packet
    # a delta's result: RULE C's layout for its header's counts, the occupancy bytes being at most one a leaf and depth
    capacity = len(d) if info.kind == 0 else 64 + 4 * h.octree_bits + (h.octree_bits + 4) * h.nleaves + 16
    return _codec_inter_convert('cwipc_hip_codec_inter_unpack', (r, len(r) if r is not None else 0, d, len(d)), capacity)


class cwipc_hip_profile:
    """Context manager collecting per-kernel device time (hipEvents on the library's stream).

        with cwipc_hip_profile() as prof:
            cwipc_downsample(pc, 0.01)
        prof.kernels  ->  {name: (total_ms, launches)}
    """

    def __enter__(self) -> 'cwipc_hip_profile':
        dll = cwipc_util_dll_load()
        dll.cwipc_hip_profile_reset()
        dll.cwipc_hip_profile_enable(1)
        self.kernels: Dict[str, Tuple[float, int]] = {}
        return self

    def __exit__(self, *exc) -> None:
        dll = cwipc_util_dll_load()
        dll.cwipc_hip_synchronize()
        dll.cwipc_hip_profile_enable(0)
        self.kernels = self.read()

    @staticmethod
    def read() -> Dict[str, Tuple[float, int]]:
        dll = cwipc_util_dll_load()
        out: Dict[str, Tuple[float, int]] = {}
        for i in range(dll.cwipc_hip_profile_count()):
            name, ms, cnt = ctypes.c_char_p(), ctypes.c_double(), ctypes.c_long()
            if dll.cwipc_hip_profile_get(i, ctypes.byref(name), ctypes.byref(ms), ctypes.byref(cnt)) == 0:
                out[name.value.decode('utf8')] = (ms.value, cnt.value)
        return out
