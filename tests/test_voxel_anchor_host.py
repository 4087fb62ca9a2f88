"""The downsample's host arithmetic (csrc/voxel_anchor.hpp) compiled for the host and checked against its definitions.  CPU only;
the host C++ compiler is required (a missing one fails the tests).

Face tables: the threshold T(m) of face m is by definition the smallest float p with floor((p - mn0) / res) >= m in double (the
octree's key), so T passes that test and the float below it does not.  Tv is the smallest float whose voxel floorf(p * inv_leaf)
(fp32 product) lies above tf, the voxel of T: Tv passes, the float below it does not.
Range plans: the ranges cover the cloud, never shrink, and none is longer than a workgroup's table allows."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CELLS = (0.001, 0.01, 0.05, 1.0)
POINTS = (1, 255, 256, 257, 65535, 300000, 1500000, 10000000, 2 ** 31 - 1)
CUS = (104, 248, 256)
STAGGER = (0, 15, 25, 40)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler: the anchor arithmetic cannot be checked"
    lib = str(tmp_path_factory.mktemp("voxel_anchor") / "libvoxel_anchor_host.so")
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "cwipc_util_amd", "csrc"),
                    os.path.join(ROOT, "tests", "abi", "voxel_anchor_host.cpp"), "-o", lib], check=True)
    dll = ctypes.CDLL(lib)
    for f in (dll.voxel_constants, dll.voxel_face_table, dll.voxel_general_plan, dll.voxel_fast_plan, dll.voxel_range_first_steps):
        f.restype = None
    dll.voxel_face_table.argtypes = [ctypes.c_void_p, ctypes.c_float] + [ctypes.c_void_p] * 5
    dll.voxel_general_plan.argtypes = [ctypes.c_ulong, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    dll.voxel_fast_plan.argtypes = [ctypes.c_ulong, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    dll.voxel_range_first_steps.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]
    c = (ctypes.c_long * 8)()
    dll.voxel_constants(c)
    dll.K1_WAVES, dll.WAVE_STEP, dll.MAX_POINTS_PER_WAVE, dll.FACES, dll.FT_T, dll.FT_TV, dll.FT_TF, dll.FACE_TABLE_WORDS = list(c)
    return dll


def anchors():
    rng = np.random.default_rng(7)
    fixed = [(0, 0, 0), (-5e-17, 0.3, -5e-17), (1e4, -1e4, 1e4), (-1e4, 1e4, -1e4)]
    return np.concatenate([np.array(fixed), rng.uniform(-3, 3, (150, 3)), rng.uniform(-2000, 2000, (50, 3))]).astype(np.float32)


@pytest.mark.parametrize("cell", CELLS)
def test_face_tables_hold_the_smallest_floats_that_pass(host, cell):
    F = host.FACES
    below = lambda v: np.nextafter(v, np.float32(-np.inf), dtype=np.float32)
    for anchor in anchors():
        table = np.zeros(host.FACE_TABLE_WORDS, dtype=np.uint32)
        mn0, res, inv_leaf, face_base = np.zeros(3), ctypes.c_double(), ctypes.c_float(), np.zeros(3, dtype=np.int32)
        host.voxel_face_table(anchor.ctypes.data, cell, table.ctypes.data, mn0.ctypes.data, ctypes.byref(res), ctypes.byref(inv_leaf), face_base.ctypes.data)
        res, inv = res.value, np.float32(inv_leaf.value)
        assert res == float(np.float32(64) * np.float32(cell)) and inv == np.float32(1) / np.float32(cell)
        for a in range(3):
            T = table[host.FT_T + a * F:host.FT_T + (a + 1) * F].view(np.float32)
            Tv = table[host.FT_TV + a * F:host.FT_TV + (a + 1) * F].view(np.float32)
            tf = table[host.FT_TF + a * F:host.FT_TF + (a + 1) * F].view(np.int32)
            m = (face_base[a] + np.arange(F)).astype(np.float64)
            assert np.isfinite(T).all() and np.isfinite(Tv).all(), (anchor, cell, a)
            key = lambda p: np.floor((p.astype(np.float64) - mn0[a]) / res)
            assert (key(T) >= m).all(), (anchor, cell, a)
            assert not (key(below(T)) >= m).any(), (anchor, cell, a)
            voxel = lambda p: np.floor(p * inv)          # fp32 product, as the kernels compute it
            assert (voxel(T).astype(np.int64) == tf).all(), (anchor, cell, a)
            assert (voxel(Tv) > tf.astype(np.float32)).all(), (anchor, cell, a)
            assert not (voxel(below(Tv)) > tf.astype(np.float32)).any(), (anchor, cell, a)


@pytest.mark.parametrize("cus", CUS)
@pytest.mark.parametrize("n", POINTS)
def test_fast_plan_ranges_cover_the_cloud_and_fit_a_workgroup(host, n, cus):
    steps_total = (n + host.WAVE_STEP - 1) // host.WAVE_STEP
    longest_allowed = host.MAX_POINTS_PER_WAVE * host.K1_WAVES // host.WAVE_STEP
    for stagger in STAGGER:
        p = np.zeros(4, dtype=np.uint32)
        host.voxel_fast_plan(n, cus, stagger, p.ctypes.data)
        blocks, per_wg, base_q, inc_q = (int(v) for v in p)
        assert blocks >= 1 and per_wg % host.WAVE_STEP == 0
        if base_q:
            first = np.zeros(blocks + 1, dtype=np.uint32)
            host.voxel_range_first_steps(blocks + 1, base_q, inc_q, first.ctypes.data)
            first = first.astype(np.int64)
        else:     # equal ranges of per_wg points
            assert inc_q == 0
            first = np.arange(blocks + 1, dtype=np.int64) * (per_wg // host.WAVE_STEP)
        lengths = np.diff(first)
        assert first[0] == 0 and first[-1] >= steps_total, (n, cus, stagger)
        assert (lengths >= 0).all(), (n, cus, stagger)
        assert lengths.max() <= longest_allowed and lengths.max() * host.WAVE_STEP <= per_wg, (n, cus, stagger)


@pytest.mark.parametrize("cus", CUS)
@pytest.mark.parametrize("n", POINTS)
def test_general_plan_waves_cover_the_cloud(host, n, cus):
    for shrink in (0, 6):
        nwaves, per_wave = ctypes.c_ulong(), ctypes.c_ulong()
        host.voxel_general_plan(n, cus, shrink, ctypes.byref(nwaves), ctypes.byref(per_wave))
        nwaves, per_wave = nwaves.value, per_wave.value
        assert nwaves % host.K1_WAVES == 0 and per_wave % host.WAVE_STEP == 0
        assert per_wave * nwaves >= n and per_wave <= host.MAX_POINTS_PER_WAVE, (n, cus, shrink)
