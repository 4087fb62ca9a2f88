"""The smoothing's per-point arithmetic (csrc/smooth_terms.hpp with csrc/smallest_eigvec.hpp) on the host: a stand-alone program
(tests/abi/smooth_host.cpp, its own main) built with -fsanitize=address,undefined and run as a program, and the library's exported
host twin cwipc_hip_smooth_host, which runs the same text unsanitised.  CPU only; the host C++ compiler is required (a missing one
fails the tests).

Against the eigh model (tests/neigh_model.py) each coordinate of a moved point must be EQUAL TO OR ADJACENT TO the model's float32
wherever the relative eigengap (w1 - w0) / w2 is at least 1e-2.  Why adjacent: tests/test_eigvec_host.py bounds the angle between
the two solvers' normals by 64 eps / gap = 1.42e-12 rad at that gap; the displacement n (n . c) with |c| < radius moves by less than
2 * radius * 1.42e-12 for it, and the f64 sum p + displacement by less than 4 * radius * 1.42e-12 with the roundings -- some 1e-13 of
a coordinate of these inputs, against a float32 step of 6e-8 of it.  The two float32 results therefore differ only when that interval
straddles a rounding boundary, and then by one step.  The share of moved points left out for a small gap is capped per input
(neigh_model.SMOOTH_INPUTS; measured with the model alone: 0, 0 and 0.4 %).  Everything else is asserted for every point:
an unmoved point's bytes, |p' - p| < radius for a moved one (the displacement is |n . c| <= |c|, plus one float32 rounding), colours and
tiles."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import neigh_model as nm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler: smooth_terms.hpp cannot be checked"
    tmp = tmp_path_factory.mktemp("smooth_host")
    exe = str(tmp / "smooth_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "cwipc_util_amd", "csrc"), os.path.join(ROOT, "tests", "abi", "smooth_host.cpp"), "-o", exe], check=True)

    class Host:
        def smooth(self, pts, radius, min_neighbours=2, same_tile=False):
            inp, out = str(tmp / "in.bin"), str(tmp / "out.bin")
            np.ascontiguousarray(pts).tofile(inp)
            subprocess.run([exe, "smooth", inp, out, repr(float(radius)), "1" if same_tile else "0", str(int(min_neighbours))], check=True, timeout=120)
            return np.fromfile(out, dtype=pts.dtype)

        def lines(self, *args):
            return [int(v) for v in subprocess.run([exe] + [str(a) for a in args], check=True, timeout=60, capture_output=True, text=True).stdout.split()]
    return Host()


_twin_cache = {}


@pytest.fixture(scope="module")
def twin(host):
    """twin(name) -> (points, radius, the sanitised program's result), each input run once"""
    def run(name):
        if name not in _twin_cache:
            pts, radius = nm.SMOOTH_INPUTS[name][0]()
            _twin_cache[name] = (pts, radius, host.smooth(pts, radius))
        return _twin_cache[name]
    return run


@pytest.mark.parametrize("name", list(nm.SMOOTH_INPUTS))
def test_host_twin_against_the_eigh_model(twin, name):
    pts, radius, got = twin(name)
    moved, compared, adjacent = nm.check_against_model(name, pts, got, radius, cap=nm.SMOOTH_INPUTS[name][1])
    assert compared.sum() > 0.9 * len(pts)
    if name == "noisy plane":
        before, after, model = nm.plane_rms(nm.xyz_of(pts)), nm.plane_rms(nm.xyz_of(got)), nm.plane_rms(nm.xyz_of(nm.smooth(pts, radius)[0]))
        assert after < before and abs(after - model) <= 1e-12 * model, (before, after, model)


def test_tiles_neighbour_threshold_and_odd_points(host):
    """SAME_TILE, min_neighbours above 2, and points that do not move: non-finite ones, lonely ones, duplicates of one another"""
    rng = np.random.default_rng(77)
    pts, radius = nm.noisy_plane()
    pts = pts[:1500].copy()
    pts["x"][10], pts["y"][20], pts["z"][30] = np.nan, np.inf, -np.inf
    pts["x"][40:43] += 5.0                                   # three lonely points, further than radius from each other too
    pts["y"][41], pts["y"][42] = pts["y"][41] + 1.0, pts["y"][42] + 2.0
    pts[50:60] = pts[50]                                     # ten copies of one point
    for mn, same in ((2, True), (12, False), (12, True), (5000, False)):
        got = host.smooth(pts, radius, mn, same)
        moved, compared, _ = nm.check_against_model("plane part, min %d, same tile %s" % (mn, same), pts, got, radius, mn, same)
        assert not moved[[10, 20, 30, 40, 41, 42]].any()
        assert moved.any() == (mn < 5000) and (mn != 12 or 0 < (~moved).sum() < len(pts))
    # two sheets of different tiles, 0.3 r apart: with SAME_TILE each is smoothed as if alone
    a = pts[:700].copy()
    b = a.copy()
    a["tile"], b["tile"] = 3, 200
    for f, v in zip("xyz", 0.3 * radius * nm.PLANE_NORMAL):
        b[f] = (b[f].astype(np.float64) + v).astype(np.float32)
    mix = rng.permutation(1400)
    both = np.concatenate([a, b])[mix]
    got = host.smooth(both, radius, 2, True)
    back = np.empty_like(got)
    back[mix] = got
    assert back[:700].tobytes() == host.smooth(a, radius).tobytes() and back[700:].tobytes() == host.smooth(b, radius).tobytes()
    assert host.smooth(both, radius, 2, False).tobytes() != got.tobytes()
    # a permuted input gives the permuted output, byte for byte: the integer sums do not depend on the order of the neighbours
    perm = rng.permutation(len(both))
    assert host.smooth(both[perm], radius, 2, True).tobytes() == got[perm].tobytes()


def test_move_decision_through_the_header(host):
    for mn in (0, 2, 7, 300000):
        need = max(2, mn)
        cnts = [0, 1, 2, 3, 4, mn, mn + 1, mn + 2, need, need + 1, 262144, 262145, 2 ** 32, 2 ** 63]
        want = [int(c - 1 >= need and c <= 262144) for c in cnts]
        assert host.lines("moves", mn, *cnts) == want, mn
    # cnt = 2 and 3 at the least threshold; min_neighbours and min_neighbours + 1 neighbours; the 2^18 cap
    assert host.lines("moves", 0, 2, 3) == [0, 1] and host.lines("moves", 7, 7, 8, 9) == [0, 1, 1]
    assert host.lines("moves", 2, 262144, 262145) == [1, 0] and host.lines("moves", 262143, 262144, 262145) == [1, 0]
    assert host.lines("moves", 262144, 262144, 262145) == [0, 0]


REFUSED = [float("nan"), float("inf"), -float("inf"), 0.0, -0.02, 9.9e-31, 1.1e30, 1e-170, 1e200]
ACCEPTED = [1e-30, 1e30, 0.02, 1.0]


def test_refused_radii(host, cwipc):
    assert host.lines("radius", *[repr(r) for r in REFUSED + ACCEPTED]) == [0] * len(REFUSED) + [1] * len(ACCEPTED)
    dll = cwipc.cwipc_util_dll_load()
    pts = nm.as_points(np.random.default_rng(1).uniform(0, 1, (50, 3)))
    out = np.zeros_like(pts)
    pc = cwipc.cwipc_from_numpy_array(pts, 1)
    messages = []
    cwipc.cwipc_log_configure(cwipc.CWIPC_LOG_LEVEL_ERROR, lambda level, msg: messages.append(msg.decode('utf8')))
    try:
        for r in REFUSED:
            before = len(messages)
            assert dll.cwipc_hip_smooth_host(pts.ctypes.data, len(pts), r, 0, 2, out.ctypes.data) == -1, r
            assert len(messages) > before and "radius" in messages[-1], r
            before = len(messages)
            assert not dll.cwipc_hip_smooth(pc.as_cwipc_p(), r, 0, 2), r          # refused before anything is launched: no GPU needed
            assert len(messages) > before and "radius" in messages[-1], r
            with pytest.raises(cwipc.CwipcError):
                cwipc.cwipc_smooth(pc, r)
        for r in ACCEPTED:
            assert dll.cwipc_hip_smooth_host(pts.ctypes.data, len(pts), r, 0, 2, out.ctypes.data) == 0, r
        # the other refusals: flag bits, NULL
        assert dll.cwipc_hip_smooth_host(pts.ctypes.data, len(pts), 0.1, 2, 2, out.ctypes.data) == -1
        assert dll.cwipc_hip_smooth_host(None, len(pts), 0.1, 0, 2, out.ctypes.data) == -1
        assert dll.cwipc_hip_smooth_host(None, 0, 0.1, 0, 2, None) == 0
        assert not dll.cwipc_hip_smooth(None, 0.1, 0, 2) and not dll.cwipc_hip_smooth(pc.as_cwipc_p(), 0.1, 4, 2)
        assert not dll.cwipc_hip_radius_outlier_filter(None, 0.1, 0, 1) and not dll.cwipc_hip_radius_outlier_filter(pc.as_cwipc_p(), 0.1, 2, 1)
        assert not dll.cwipc_hip_radius_outlier_filter(pc.as_cwipc_p(), float("nan"), 0, 1) and not dll.cwipc_hip_radius_outlier_filter(pc.as_cwipc_p(), -1.0, 0, 1)
        counts = np.zeros(50, dtype=np.uint32)
        assert dll.cwipc_hip_radius_counts(None, 0.1, 0, counts.ctypes.data, 50) == -1
        assert dll.cwipc_hip_radius_counts(pc.as_cwipc_p(), float("inf"), 0, counts.ctypes.data, 50) == -1
        assert dll.cwipc_hip_radius_counts(pc.as_cwipc_p(), 0.0, 0, counts.ctypes.data, 50) == -1
    finally:
        cwipc.cwipc_log_configure(cwipc.CWIPC_LOG_LEVEL_ERROR, None)
        pc.free()


@pytest.mark.parametrize("name", list(nm.SMOOTH_INPUTS))
def test_exported_twin_gives_the_programs_bytes(twin, cwipc, name):
    pts, radius, got = twin(name)
    assert cwipc.cwipc_hip_smooth_host(pts, radius).tobytes() == got.tobytes()


def test_exported_twin_with_tiles_and_threshold(host, cwipc):
    pts, radius = nm.noisy_sphere()
    pts = pts[:2000]
    for mn, same in ((2, True), (4, False), (4, True)):
        assert cwipc.cwipc_hip_smooth_host(pts, radius, mn, same).tobytes() == host.smooth(pts, radius, mn, same).tobytes(), (mn, same)
    assert len(cwipc.cwipc_hip_smooth_host(pts[:0], radius)) == 0


def test_new_symbols_are_exported_and_declared(cwipc):
    from cwipc_util_amd.util import _SIGNATURES
    dll = cwipc.cwipc_util_dll_load()
    header = open(os.path.join(ROOT, "include", "cwipc_util_amd", "hip_ext.h")).read()
    assert "RULE N." in header and header.index("RULE K.") < header.index("RULE N.")
    assert "#define CWIPC_HIP_NEIGH_SAME_TILE 1" in header and cwipc.CWIPC_HIP_NEIGH_SAME_TILE == 1
    for name in ("cwipc_hip_radius_counts", "cwipc_hip_radius_outlier_filter", "cwipc_hip_smooth", "cwipc_hip_smooth_host"):
        assert hasattr(dll, name) and name in _SIGNATURES, name
        assert re.search(r"_CWIPC_UTIL_EXPORT[^;]*\b%s\(" % name, header), name
    for public in ("cwipc_radius_counts", "cwipc_radius_outlier_filter", "cwipc_smooth", "cwipc_hip_smooth_host", "CWIPC_HIP_NEIGH_SAME_TILE"):
        assert public in cwipc.util.__all__ and hasattr(cwipc, public), public
    pc_p = _SIGNATURES["cwipc_hip_direction_filter"][0][0]
    # the header's parameter lists against the wrapper's argument types
    params = re.search(r"cwipc_hip_radius_counts\(([^)]*)\)", header).group(1)
    assert [p.strip().rsplit(" ", 1)[0] for p in params.split(",")] == ["cwipc_pointcloud", "double", "int", "uint32_t", "size_t"]
    assert _SIGNATURES["cwipc_hip_radius_counts"] == ([pc_p, ctypes.c_double, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t], ctypes.c_int)
    params = re.search(r"cwipc_hip_radius_outlier_filter\(([^)]*)\)", header).group(1)
    assert [p.strip().rsplit(" ", 1)[0] for p in params.split(",")] == ["cwipc_pointcloud", "double", "int", "uint64_t"]
    assert _SIGNATURES["cwipc_hip_radius_outlier_filter"] == ([pc_p, ctypes.c_double, ctypes.c_int, ctypes.c_uint64], pc_p)
    params = re.search(r"cwipc_hip_smooth\(([^)]*)\)", header).group(1)
    assert [p.strip().rsplit(" ", 1)[0] for p in params.split(",")] == ["cwipc_pointcloud", "double", "int", "uint32_t"]
    assert _SIGNATURES["cwipc_hip_smooth"] == ([pc_p, ctypes.c_double, ctypes.c_int, ctypes.c_uint32], pc_p)
    params = re.search(r"cwipc_hip_smooth_host\(([^)]*)\)", header).group(1)
    assert [p.strip().rsplit(" ", 1)[0] for p in params.split(",")] == ["const struct cwipc_point", "size_t", "double", "int", "uint32_t", "struct cwipc_point"]
    assert _SIGNATURES["cwipc_hip_smooth_host"] == ([ctypes.c_void_p, ctypes.c_size_t, ctypes.c_double, ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p], ctypes.c_int)
    assert nm.POINT_DTYPE == cwipc.cwipc_point_numpy_dtype


def test_factory_entries(cwipc):
    from cwipc_util_amd import filters
    from cwipc_util_amd.filters import radius_outliers, smooth
    f = filters.factory("radius_outliers(0.02, 4)")
    assert isinstance(f, radius_outliers.RadiusOutliersFilter) and f.filtername == "radius_outliers"
    assert (f.radius, f.min_neighbours, f.same_tile) == (0.02, 4, False)
    assert (filters.factory("radius_outliers(0.05)").min_neighbours, filters.factory("radius_outliers(0.05, 2, True)").same_tile) == (1, True)
    g = filters.factory("smooth(0.016, 5, 3)")
    assert isinstance(g, smooth.SmoothFilter) and g.filtername == "smooth"
    assert (g.radius, g.min_neighbours, g.iterations, g.same_tile) == (0.016, 5, 3, False)
    h = filters.factory("smooth(0.02)")
    assert (h.min_neighbours, h.iterations, h.same_tile) == (2, 1, False) and filters.factory("smooth(0.02, 2, 1, True)").same_tile is True
    for mod, name in ((radius_outliers, "radius_outliers"), (smooth, "smooth")):
        assert mod in filters.all_filters and name in filters.__doc__
    assert callable(f.filter) and callable(f.statistics) and callable(g.filter) and callable(g.statistics)
