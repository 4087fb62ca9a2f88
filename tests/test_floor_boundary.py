"""The floor and tile helpers at the boundary without a GPU (the pattern of test_boundary.py): the library exports the new
symbols, the wrapper declares them, and every one of them fails loudly when no device is there."""
import ctypes

import numpy as np
import pytest

NEW_SYMBOLS = ("cwipc_hip_floor_partition", "cwipc_hip_randomize_floor", "cwipc_hip_floor_radius_stats", "cwipc_hip_tile_counts", "cwipc_hip_bounds")


def _cloud(cwipc):
    return cwipc.cwipc_from_points([(1, 2, 3, 0x10, 0x20, 0x30, 1), (4, 0, 6, 0x40, 0x50, 0x60, 2)], 77)


def test_new_symbols_are_exported_and_declared(cwipc):
    from cwipc_util_amd.util import _SIGNATURES
    dll = cwipc.cwipc_util_dll_load()
    for name in NEW_SYMBOLS:
        assert hasattr(dll, name) and name in _SIGNATURES, name
    assert (cwipc.CWIPC_HIP_FLOOR_KEEP_FLOOR, cwipc.CWIPC_HIP_FLOOR_KEEP_REST, cwipc.CWIPC_HIP_FLOOR_LIMIT_RADIUS) == (1, 2, 4)


def test_null_cloud_is_an_error(cwipc):
    dll = cwipc.cwipc_util_dll_load()
    n_first = ctypes.c_uint64(5)
    assert not dll.cwipc_hip_floor_partition(None, 0.1, 3, 0.0, ctypes.byref(n_first)) and n_first.value == 0
    assert not dll.cwipc_hip_randomize_floor(None, 0.1, 1)
    count, stat = (ctypes.c_uint64 * 2)(), (ctypes.c_float * 4)()
    assert dll.cwipc_hip_floor_radius_stats(None, 0.1, count, stat) == -1
    assert dll.cwipc_hip_tile_counts(None, 0, 0.1, (ctypes.c_uint64 * 256)()) == -1
    assert dll.cwipc_hip_bounds(None, (ctypes.c_float * 6)()) == -1


def test_floor_helpers_fail_loudly_without_gpu(cwipc):
    """No CPU fallback: without a device every helper reports an error."""
    if cwipc.cwipc_hip_device_count() > 0:
        pytest.skip("a GPU is visible")
    pc = _cloud(cwipc)
    messages = []
    cwipc.cwipc_log_configure(cwipc.CWIPC_LOG_LEVEL_ERROR, lambda level, msg: messages.append(msg.decode('utf8')))
    try:
        for call in (lambda: cwipc.cwipc_floor_filter(pc), lambda: cwipc.cwipc_floor_filter(pc, 0.1, True),
                     lambda: cwipc.cwipc_randomize_floor(pc, seed=1), lambda: cwipc.cwipc_limit_floor_to_radius(pc, 1.0),
                     lambda: cwipc.cwipc_compute_radius(pc), lambda: cwipc.cwipc_compute_tile_occupancy(pc),
                     lambda: cwipc.cwipc_compute_tile_occupancy(pc, 0.01, True), lambda: cwipc.cwipc_hip_bounds(pc),
                     lambda: cwipc.cwipc_hip_tile_counts(pc), lambda: cwipc.cwipc_hip_floor_radius_stats(pc)):
            before = len(messages)
            with pytest.raises(cwipc.CwipcError):
                call()
            assert any("no usable HIP device" in m for m in messages[before:]), messages[before:]
    finally:
        cwipc.cwipc_log_configure(cwipc.CWIPC_LOG_LEVEL_WARNING, None)


def test_filter_factory_knows_the_new_filters(cwipc):
    from cwipc_util_amd import filters
    f = filters.factory("randomize_floor")
    assert type(f).__name__ == "RandomizeFloorFilter" and f.level == 0.1 and f.seed is None
    assert filters.factory("randomize_floor(0.25)").level == 0.25
    a = filters.factory("analyze")
    assert type(a).__name__ == "AnalyzeFilter" and (a.min_x, a.max_y, a.sum_avg_z, a.count) == (999999, -999999, 0, 0)
