"""The arithmetic of plane segmentation (csrc/plane_seg_terms.hpp, RULE S of include/cwipc_util_amd/hip_ext.h) on the host: a
stand-alone program (tests/abi/plane_seg_host.cpp, its own main) built with -fsanitize=address,undefined and run as a program, and
the library's exported host twin cwipc_hip_plane_find_host, which runs the same text unsanitised.  CPU only; the host C++ compiler
is required (a missing one fails the tests).

Against the model (tests/plane_model.py) everything is BYTE-EQUAL: the table (a -0.0 included), the valid bits, the counts, the best
hypothesis, the sums, M and -- because the model solves with a line-by-line port of csrc/smallest_eigvec.hpp -- the refined plane.
The refined normal is also held to numpy.linalg.eigh of the exact matrix within the angle tests/test_eigvec_host.py establishes,
EIG_C * eps / gap with gap = (w1 - w0) / w2: a plane's matrix has a gap near 1, so that is some 1e-14 rad."""
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import plane_model as pm
from test_eigvec_host import EIG_C, EPS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLT_MAX = float(np.finfo(np.float32).max)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler: plane_seg_terms.hpp cannot be checked"
    tmp = tmp_path_factory.mktemp("plane_seg_host")
    exe = str(tmp / "plane_seg_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "cwipc_util_amd", "csrc"), os.path.join(ROOT, "tests", "abi", "plane_seg_host.cpp"), "-o", exe], check=True)

    class Host:
        def find(self, xyz, distance, H, seed=0, axis=(0.0, 0.0, 0.0), mac=0.0, refine=True):
            """(result bytes, planes, counts, valid)"""
            inp, out = str(tmp / "in.bin"), str(tmp / "out.bin")
            pm.to_points(xyz).tofile(inp)
            subprocess.run([exe, "find", inp, out, repr(float(distance)), str(H), str(seed)] + [repr(float(a)) for a in axis] + [repr(float(mac)), "1" if refine else "0"],
                           check=True, timeout=120)
            raw = open(out, "rb").read()
            size = struct.calcsize(pm.RESULT_FORMAT)
            assert len(raw) == size + 37 * H
            return (raw[:size], np.frombuffer(raw[size:size + 32 * H], dtype=np.float64).reshape(H, 4), np.frombuffer(raw[size + 32 * H:size + 36 * H], dtype=np.uint32),
                    np.frombuffer(raw[size + 36 * H:], dtype=np.uint8).astype(bool))

        def lines(self, *args):
            return subprocess.run([exe] + [a if isinstance(a, str) else repr(a) for a in args], check=True, timeout=60, capture_output=True, text=True).stdout.split()
    return Host()


def lattice_with_steps():
    """a lattice on y = 0 (a lattice triple's plane is (0, +-1, 0, -+0): a -0.0 in the table either way) and two steps above it"""
    g = np.stack(np.meshgrid(np.arange(12), np.arange(12), indexing="ij"), axis=-1).reshape(-1, 2)
    lat = np.stack([g[:, 0] * 0.25, np.zeros(len(g)), g[:, 1] * 0.25], axis=1)
    return np.concatenate([lat, lat[:40] + [0.1, 0.5, 0.1], lat[:20] + [0.0, 1.25, 0.0]]).astype(np.float32)


def inputs():
    """{name: (xyz, distance, H, seed, axis, min_abs_cos)}"""
    scene = pm.scene(n=3000, seed=8)[0]
    y15 = ((0.0, 1.0, 0.0), math.cos(math.radians(15.0)))
    length = math.sqrt(0.3 * 0.3 + 1.0 + 0.2 * 0.2)
    tilted = ((0.3 / length, 1.0 / length, -0.2 / length), math.cos(math.radians(40.0)))
    rng = np.random.default_rng(6)
    holes = scene[:1200].copy()
    for k, i in enumerate(rng.choice(1200, 150, replace=False)):
        holes[i, k % 3] = (np.nan, np.inf, -np.inf)[(k // 3) % 3]
    far = np.float32([(1e6, 0, 0), (-1e6, .5, .5), (3e38, 0, 0), (-3e38, 3e38, -3e38), (FLT_MAX, FLT_MAX, FLT_MAX), (1e6, 0, 0.05)])
    t = np.arange(-100, 100, dtype=np.float32)
    return {
        "scene": (scene, 0.01, 300, 0, (0.0, 0.0, 0.0), 0.0),
        "scene, Y within 15 degrees": (scene, 0.01, 300, 0) + y15,
        "scene, a tilted axis": (scene, 0.02, 200, 12345678901234567890) + tilted,
        "lattice": (lattice_with_steps(), 0.125, 128, 5, (0.0, 0.0, 0.0), 0.0),
        "non-finite": (holes, 0.01, 256, 1, (0.0, 0.0, 0.0), 0.0),
        "far points": (np.concatenate([scene[:200], far, scene[200:400]]), 0.01, 512, 2, (0.0, 0.0, 0.0), 0.0),
        "collinear": (np.stack([t, 2 * t, -t], axis=1), 0.5, 64, 3, (0.0, 0.0, 0.0), 0.0),
        "duplicates": (np.tile(np.float32([[0.3, -1.7, 2.9]]), (500, 1)), 0.01, 64, 4, (0.0, 0.0, 0.0), 0.0),
        "two points": (scene[:2], 0.01, 32, 0, (0.0, 0.0, 0.0), 0.0),
        "empty": (scene[:0], 0.01, 32, 0, (0.0, 0.0, 0.0), 0.0),
        "wide distance": (scene[:500] * np.float32(1e20), 1e30, 64, 7, (0.0, 0.0, 0.0), 0.0),
        "narrow distance": (scene[:500], 1e-30, 64, 7, (0.0, 0.0, 0.0), 0.0),
    }


@pytest.mark.parametrize("name", list(inputs()))
@pytest.mark.parametrize("refine", [True, False])
def test_program_and_exported_twin_equal_the_model(host, cwipc, name, refine):
    xyz, distance, H, seed, axis, mac = inputs()[name]
    want = pm.find(xyz, distance, H, seed, axis, mac, refine)
    raw, planes, counts, valid = host.find(xyz, distance, H, seed, axis, mac, refine)
    assert planes.tobytes() == want.planes.tobytes() and np.array_equal(valid, want.valid_rows) and np.array_equal(counts, want.counts)
    assert raw == want.tobytes(), (struct.unpack(pm.RESULT_FORMAT, raw), struct.unpack(pm.RESULT_FORMAT, want.tobytes()))
    # the exported twin: the program's bytes.  (The wrapper takes the constraint as an axis and an angle; the C entry takes the cosine.)
    import ctypes
    params = cwipc.cwipc_hip_plane_params(distance, seed, (ctypes.c_double * 3)(*axis), mac, H, 1 if refine else 0)
    res = cwipc.cwipc_hip_plane_result()
    pts = pm.to_points(xyz)
    probe = pts if len(pts) else np.zeros(1, dtype=pts.dtype)
    t_planes, t_counts, t_valid = np.zeros((H, 4)), np.zeros(H, dtype=np.uint32), np.zeros(H, dtype=np.uint8)
    assert cwipc.cwipc_util_dll_load().cwipc_hip_plane_find_host(probe.ctypes.data, len(pts), ctypes.addressof(params), ctypes.addressof(res), t_planes.ctypes.data,
                                                                 t_counts.ctypes.data, t_valid.ctypes.data) == 0
    assert bytes(res) == raw and t_planes.tobytes() == planes.tobytes() and np.array_equal(t_counts, counts) and np.array_equal(t_valid.astype(bool), valid)
    if name == "lattice":
        assert np.signbit(planes[valid][:, 3]).any() and (planes[valid][:, 3] == 0).any()      # a -0.0 went through
    if name in ("collinear", "duplicates", "two points", "empty"):
        assert not want.found and want.valid == 0
    elif name != "narrow distance":
        assert want.found and (want.refined or not refine or want.recount < want.count or want.sums[0] < 3)


def test_refined_normal_against_eigh(host):
    xyz, distance, H, seed, axis, mac = inputs()["scene"]
    want = pm.find(xyz, distance, H, seed, axis, mac, True)
    assert want.refined
    M6, exact = pm.refit_matrix(want.sums)
    assert M6 == want.M and all(float(v) == m for v, m in zip(exact, M6))
    vec, w = pm.eigh_normal(exact)
    gap = (w[1] - w[0]) / w[2]
    n = np.array(want.plane[:3])
    ang = np.arctan2(np.linalg.norm(np.cross(n, vec)), abs(n @ vec))
    print("refined normal against eigh: gap %.3f, angle %.3g rad, bound %.3g" % (gap, ang, EIG_C * EPS / gap))
    assert gap > 0.1 and ang <= EIG_C * EPS / gap


def refit_args(distance, axis, mac, count, recount, anchor, hyp, sums):
    return ["refit", distance] + list(axis) + [mac, str(count), str(recount)] + list(anchor) + list(hyp) + [str(s) for s in sums]


def sums_of(offsets):
    o = np.asarray(offsets, dtype=object)
    out = [len(o)] + [int(o[:, a].sum()) for a in range(3)]
    for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)):
        out.append(int((o[:, a] * o[:, b]).sum()))
    return out


def test_accept_and_reject_of_the_refined_plane(host):
    """The four conditions: 3 <= cnt <= 2^26, n' finite, the constraint for n', recount >= count.  (n' of exact sums within the cnt
    range is always finite -- M's entries stay below 2^115 --, so that condition has no input that fails it; the other three do.)"""
    rng = np.random.default_rng(3)
    # offsets of a plane z = 0.1 x in fixed-point units, the hypothesis roughly along it
    o = np.stack([rng.integers(-2000, 2000, 400), rng.integers(-2000, 2000, 400), np.zeros(400, dtype=np.int64)], axis=1)
    o[:, 2] = o[:, 0] // 10
    sums, anchor, hyp, distance = sums_of(o), (0.5, -0.25, 2.0), (0.0, 0.0, 1.0, -2.0), 0.01

    def run(count, recount, s=sums, axis=(0.0, 0.0, 0.0), mac=0.0):
        out = host.lines(*refit_args(distance, axis, mac, count, recount, anchor, hyp, s))
        plane = [float.fromhex(v) for v in out[2:6]]
        return int(out[0]), int(out[1]), plane, [float.fromhex(v) for v in out[6:12]]

    ok, model_plane, M6 = pm.refit_plane(sums, anchor, hyp, distance)
    assert ok and pm.angle_deg(model_plane, (-0.1, 0.0, 1.0)) < 0.3
    wanted, refined, plane, M = run(400, 400)
    assert (wanted, refined) == (1, 1) and plane == pm.orient(model_plane) and M == M6
    assert run(400, 401)[:2] == (1, 1) and run(400, 399)[:3] == (1, 0, pm.orient(list(hyp)))       # recount >= count
    # cnt = 2 and 3; 2^26 and 2^26 + 1 (the sums of that many inliers scaled from these: only cnt matters to the decision)
    two, three = sums_of(o[:2]), sums_of(o[:3])
    assert run(2, 2, two)[:2] == (0, 0) and run(2, 2, two)[3] == [0.0] * 6
    assert run(3, 3, three)[0] == 1
    big = [2 ** 26] + [v * 1000 for v in sums[1:]]
    assert run(5, 2 ** 26, big)[:2] == (1, 1) and run(5, 2 ** 26, [2 ** 26 + 1] + big[1:])[:2] == (0, 0)
    assert run(5, 2 ** 26, big)[3] == pm.refit_matrix(big)[0]                                     # the 128-bit products, rounded once
    assert any(abs(v) > 2 ** 64 for v in pm.refit_matrix(big)[1])
    # the constraint for n': the hypothesis passes an axis that the refit's normal misses
    axis = (0.0, 0.0, 1.0)
    cos_n = abs(model_plane[2])
    assert run(400, 400, axis=axis, mac=cos_n)[:2] == (1, 1)
    assert run(400, 400, axis=axis, mac=float(np.nextafter(cos_n, 2)))[:3] == (0, 0, pm.orient(list(hyp), axis, 1.0))
    # the orientation of the returned plane follows the axis
    assert run(400, 400, axis=(0.0, 0.0, -1.0), mac=0.5)[2] == [-v for v in model_plane]


def test_offset_boundary(host):
    """|o| = 262144 takes part, 262145 does not; s = 16 / distance"""
    distance = 0.5            # s = 32 exactly
    for units, part in ((262144, 1), (262145, 0), (-262144, 1), (-262145, 0), (262144.5, 1), (262145.5, 0)):
        out = [int(v) for v in host.lines("offsets", distance, 1.0, 2.0, 3.0, 1.0 + units / 32.0, 2.0, 3.0 - 1.0 / 32.0)]
        assert (out == [1, int(np.rint(units)), 0, -1]) if part else (out[0] == 0), (units, out)
    for bad in ("nan", "inf", "-inf", "1e300"):
        assert host.lines("offsets", distance, 0.0, 0.0, 0.0, bad, "0.0", "0.0")[0] == "0"


def test_parameter_ranges(host, cwipc):
    def ok(distance, H=16, mac=0.0):
        return host.lines("rule", distance, str(H), mac) == ["1"]
    assert all(ok(d) for d in (1e-30, 1e30, 0.01)) and not any(ok(d) for d in (float("nan"), float("inf"), 0.0, -0.01, 9.9e-31, 1.1e30))
    assert ok(0.01, 1) and ok(0.01, 65536) and not ok(0.01, 0) and not ok(0.01, 65537)
    assert ok(0.01, 16, 1.0) and not ok(0.01, 16, float(np.nextafter(1.0, 2))) and not ok(0.01, 16, -1e-9) and not ok(0.01, 16, float("nan"))
    # the exported twin refuses the same, and unknown flag bits and NULL pointers, with -1
    import ctypes
    dll = cwipc.cwipc_util_dll_load()
    pts = pm.to_points(pm.scene(n=100)[0])
    res = cwipc.cwipc_hip_plane_result()

    def call(distance=0.01, H=16, mac=0.0, flags=1, axis=(0.0, 0.0, 0.0), points=pts.ctypes.data, result=None, params=True):
        p = cwipc.cwipc_hip_plane_params(distance, 0, (ctypes.c_double * 3)(*axis), mac, H, flags)
        return dll.cwipc_hip_plane_find_host(points, len(pts), ctypes.addressof(p) if params else None, ctypes.addressof(res) if result is None else result, None, None, None)
    assert call() == 0
    for kw in (dict(distance=0.0), dict(distance=float("nan")), dict(distance=2e30), dict(H=0), dict(H=65537), dict(mac=1.5), dict(mac=-0.5), dict(flags=2), dict(flags=-1),
               dict(axis=(float("nan"), 0.0, 0.0)), dict(axis=(float("inf"), 0.0, 0.0)), dict(points=None), dict(result=0), dict(params=False)):
        assert call(**kw) == -1, kw
