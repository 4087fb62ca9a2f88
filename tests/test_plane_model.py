"""tests/plane_model.py, the numpy model of RULE S (include/cwipc_util_amd/hip_ext.h), held to a pure-Python brute force on clouds of
at most 300 points; the Python wrappers' refusals and the filters' registration; the levelling matrix.  CPU only."""
import math

import numpy as np
import pytest

import plane_model as pm

PLANE_FIT_ORTHO_BOUND = 4 * 2.0 ** -53      # csrc/plane_fit.hpp


def small_clouds():
    rng = np.random.default_rng(300)
    scene = pm.scene(n=300, seed=2)[0]
    holes = scene.copy()
    for k, i in enumerate(rng.choice(300, 40, replace=False)):
        holes[i, k % 3] = (np.nan, np.inf, -np.inf)[(k // 3) % 3]
    g = np.stack(np.meshgrid(np.arange(10), np.arange(10), indexing="ij"), axis=-1).reshape(-1, 2)
    sheets = np.concatenate([np.stack([g[:, 0] * 0.5, np.zeros(100), g[:, 1] * 0.5], axis=1), np.stack([g[:, 0] * 0.5, np.ones(100), g[:, 1] * 0.5], axis=1)])
    far = np.float32([(1e6, 0, 0), (3e38, 0, 0), (-3e38, 3e38, -3e38), (np.finfo(np.float32).max,) * 3])
    t = np.arange(-50, 50, dtype=np.float32)
    y20 = ((0.0, 1.0, 0.0), math.cos(math.radians(20.0)))
    free = ((0.0, 0.0, 0.0), 0.0)
    return {
        "scene": (scene, 0.02, 96, 1) + free,
        "scene, Y within 20 degrees": (scene, 0.02, 96, 1) + y20,
        "scene, a zero axis with a cosine": (scene, 0.02, 40, 1, (0.0, 0.0, 0.0), 0.9),
        "scene, an axis with cosine 0": (scene, 0.02, 40, 1, (0.0, 0.0, 1.0), 0.0),
        "scene, seed 2^64 - 1": (scene, 0.02, 40, 2 ** 64 - 1) + free,
        "non-finite": (holes, 0.02, 128, 3) + free,
        "mirrored sheets": (sheets.astype(np.float32), 0.125, 64, 4) + free,
        "far points": (np.concatenate([scene[:100], far, scene[100:200]]), 0.02, 200, 5) + free,
        "collinear": (np.stack([t, 2 * t, -t], axis=1), 0.5, 32, 6) + free,
        "duplicates": (np.tile(np.float32([[1, 2, 3]]), (60, 1)), 0.01, 32, 7) + free,
        "three points": (scene[:3], 0.02, 64, 8) + free,
        "two points": (scene[:2], 0.02, 16, 8) + free,
        "empty": (scene[:0], 0.02, 16, 8) + free,
    }


@pytest.mark.parametrize("name", list(small_clouds()))
@pytest.mark.parametrize("refine", [True, False])
def test_model_equals_brute_force(name, refine):
    xyz, distance, H, seed, axis, mac = small_clouds()[name]
    m = pm.find(xyz, distance, H, seed, axis, mac, refine)
    b = pm.brute_force(xyz, distance, H, seed, axis, mac, refine)
    assert m.triples.tolist() == b.triples and m.valid_rows.tolist() == b.valid_rows and m.counts.tolist() == b.counts
    assert m.planes.tobytes() == np.float64(b.planes).tobytes()
    assert m.sums == b.sums and m.tobytes() == b.tobytes()
    if name in ("collinear", "duplicates", "two points", "empty"):
        assert not m.found and m.tobytes() == pm.Found().tobytes()
    if name == "mirrored sheets":
        top = [h for h in range(H) if b.valid_rows[h] and b.counts[h] == max(b.counts)]
        assert len(top) > 1 and m.best == top[0] and max(b.counts) == 100
    if name == "scene, a zero axis with a cosine" or name == "scene, an axis with cosine 0":      # both mean: unconstrained
        free = pm.find(xyz, distance, H, seed, refine=refine)
        assert free.tobytes() == m.tobytes()
    if name == "scene, Y within 20 degrees":
        free = pm.find(xyz, distance, H, seed, refine=refine)
        assert free.triples.tobytes() == m.triples.tobytes() and 0 < m.valid < free.valid


def test_draws_and_index_rule():
    # splitmix64 of 0 and the first outputs of its stream from 0 (Steele, Lea, Flood: the published test values)
    assert pm.splitmix64_int(pm.GOLDEN) == 0xE220A8397B1DCDAF and pm.splitmix64_int(2 * pm.GOLDEN) == 0x6E789E6AA1B965F4
    assert int(pm.splitmix64(np.uint64(pm.GOLDEN))) == 0xE220A8397B1DCDAF
    for n in (1, 2, 3, 1000, 2 ** 32 - 1):
        t = pm.triples(5, 500, n)
        assert t.dtype == np.uint32 and t.max() < n
    assert pm.triples(5, 500, 2 ** 32 - 1).max() > 2 ** 31 and not pm.triples(5, 500, 0).any()
    assert np.array_equal(pm.triples(5, 10, 1000), pm.triples(5, 500, 1000)[:10]) and not np.array_equal(pm.triples(5, 10, 1000), pm.triples(6, 10, 1000))
    # uniform enough: 30 000 draws over 10 bins, each within 5 sigma of 3000 (sigma = sqrt(3000 * 0.9) = 52)
    hist = np.bincount(pm.triples(1, 10000, 10).reshape(-1), minlength=10)
    assert np.all(np.abs(hist - 3000) < 5 * 52)


def test_python_refusals_and_registration(cwipc):
    from cwipc_util_amd import filters, registration
    names = {m.CustomFilter.filtername for m in filters.all_filters}
    assert {"plane", "level_floor"} <= names
    assert filters.factory("plane(0.01)").filtername == "plane" and filters.factory("level_floor(0.02, 10.0, 128, 3, True)").remove is True
    assert "plane" in filters.__doc__ and "level_floor" in filters.__doc__
    assert callable(registration.find_floor) and callable(registration.level_to_floor)
    pts = pm.to_points(pm.scene(n=50)[0])
    for kw in (dict(distance=0.0), dict(distance=float("nan")), dict(distance=1e31), dict(iterations=0), dict(iterations=65537), dict(seed=-1), dict(seed=2 ** 64),
               dict(axis=(0, 0, 0), max_angle=10.0), dict(axis=(0, 1, 0)), dict(max_angle=91.0), dict(max_angle=-1.0), dict(axis=(0, float("nan"), 0), max_angle=10.0),
               dict(axis=(0, 1), max_angle=10.0)):
        args = dict(distance=0.01, iterations=16, seed=0)
        args.update(kw)
        with pytest.raises(ValueError):
            cwipc.cwipc_hip_plane_find_host(pts, **args)
    with pytest.raises(ValueError):
        cwipc.cwipc_plane_filter(None, (0, 1, 0, 0), 0.01, keep="all")
    for plane in ((0, 0, 0, 1), (0, 1, 0), (0, float("inf"), 0, 0), (float("nan"), 1, 0, 0)):
        with pytest.raises(ValueError):
            cwipc.cwipc_hip_plane_level_matrix(plane)
    nothing = cwipc.cwipc_hip_plane_find_host(pts[:2], 0.01, 16)[0]
    assert not nothing.found
    with pytest.raises(ValueError):
        cwipc.cwipc_hip_plane_level_matrix(nothing)
    # the constraint: an angle in degrees becomes the cosine, the axis is normalised, +Y is the default axis
    assert cwipc.cwipc_plane_constraint() == ((0.0, 0.0, 0.0), 0.0)
    assert cwipc.cwipc_plane_constraint(None, 60.0) == ((0.0, 1.0, 0.0), math.cos(math.radians(60.0)))
    axis, mac = cwipc.cwipc_plane_constraint((3.0, 0.0, 4.0), 0.0)
    assert axis == (0.6, 0.0, 0.8) and mac == 1.0 and cwipc.cwipc_plane_constraint((0, 2, 0), 90.0)[1] < 1e-16
    # NULL and the C refusals of the entries that need no GPU to refuse
    import ctypes
    dll = cwipc.cwipc_util_dll_load()
    m = np.zeros(16)
    good = np.float64([0, 1, 0, 0])
    assert dll.cwipc_hip_plane_level_matrix(good.ctypes.data, m.ctypes.data) == 0
    assert dll.cwipc_hip_plane_level_matrix(None, m.ctypes.data) == -1 and dll.cwipc_hip_plane_level_matrix(good.ctypes.data, None) == -1
    assert dll.cwipc_hip_plane_level_matrix(np.zeros(4).ctypes.data, m.ctypes.data) == -1
    n_first = ctypes.c_uint64(7)
    assert not dll.cwipc_hip_plane_partition(None, good.ctypes.data, 0.01, 3, ctypes.byref(n_first)) and n_first.value == 0
    res, par = cwipc.cwipc_hip_plane_result(), cwipc.cwipc_hip_plane_params(0.01, 0, (ctypes.c_double * 3)(), 0.0, 16, 1)
    assert dll.cwipc_hip_plane_find(None, ctypes.addressof(par), ctypes.addressof(res)) == -1
    assert dll.cwipc_hip_plane_scores(None, ctypes.addressof(par), None, None, None, None) == -1
    assert ctypes.sizeof(cwipc.cwipc_hip_plane_result) == pm.struct.calcsize(pm.RESULT_FORMAT) == 232 and ctypes.sizeof(cwipc.cwipc_hip_plane_params) == 56


def level_cases():
    rng = np.random.default_rng(9)
    cases = [(0.0, 1.0, 0.0, 0.0), (0.0, -1.0, 0.0, 0.25), (0.0, 1.0, 0.0, -3.0), (1.0, 0.0, 0.0, 0.5), (0.0, 0.0, -1.0, 2.0), (0.6, 0.0, 0.8, -1.0),
             (0.0, 3.0, 0.0, 6.0), (1e-9, 1.0, -1e-9, 0.1), (1e150, 1e150, 0.0, 1e150), (1e-150, 2e-150, -1e-150, 3e-150)]
    for _ in range(200):
        n = rng.normal(size=3)
        n /= np.linalg.norm(n)
        cases.append((n[0], n[1], n[2], rng.uniform(-5, 5)))
    return [tuple(float(v) for v in c) for c in cases]


def test_level_matrix(cwipc):
    """R^T R - I within PLANE_FIT_ORTHO_BOUND (plus what numpy's own f64 product adds: three products and two sums of magnitude at
    most 1, 5 * 2^-53); n -> (0, 1, 0); a point of the plane lands at |y| within a bound from the operand sizes:  y' = r . p + t with
    r, t the rounded unit normal and offset (each within 2^-53 relative), evaluated here in f64 with four roundings, for a point
    that itself satisfies n . p + d = 0 only to the rounding of its construction (three roundings of terms of size |n_i p_i|, |d|):
    8 * 2^-53 * (|r_x x| + |r_y y| + |r_z z| + |t|) covers all of it.  n = +-Y, n_y = 0 and negated input are among the cases."""
    rng = np.random.default_rng(10)
    for plane in level_cases():
        M = cwipc.cwipc_hip_plane_level_matrix(plane)
        R, t = M[:3, :3], M[:3, 3]
        assert np.array_equal(M[3], [0, 0, 0, 1]) and t[0] == 0 and t[2] == 0
        assert np.abs(R.T @ R - np.eye(3)).max() <= PLANE_FIT_ORTHO_BOUND + 5 * 2.0 ** -53, plane
        sign = -1.0 if plane[1] < 0 else 1.0
        scale = max(abs(v) for v in plane[:3])                      # (1e150 squared would overflow)
        length = float(np.linalg.norm(np.array(plane[:3]) / scale)) * scale
        n, d = sign * np.array(plane[:3]) / length, sign * plane[3] / length
        assert np.abs(R @ n - [0, 1, 0]).max() <= 8 * 2.0 ** -53 and np.abs(R[1] - n).max() <= 4 * 2.0 ** -53 and abs(t[1] - d) <= 4 * 2.0 ** -53 * max(1.0, abs(d))
        assert np.linalg.det(R) > 0.999
        # negated input: the same motion
        assert np.array_equal(cwipc.cwipc_hip_plane_level_matrix([-v for v in plane]), M) or plane[1] == 0
        # points of the plane: any two coordinates, the third solved for along the normal's largest component
        k = int(np.argmax(np.abs(n)))
        p = rng.uniform(-3, 3, (50, 3))
        others = [a for a in range(3) if a != k]
        p[:, k] = -(d + p[:, others[0]] * n[others[0]] + p[:, others[1]] * n[others[1]]) / n[k]
        y = ((R[1, 0] * p[:, 0] + R[1, 1] * p[:, 1]) + R[1, 2] * p[:, 2]) + t[1]
        bound = 8 * 2.0 ** -53 * ((np.abs(R[1] * p)).sum(axis=1) + abs(t[1])) / abs(n[k])      # (the construction divides by n_k)
        assert np.all(np.abs(y) <= bound), (plane, float(np.abs(y / bound).max()))
    # n = +Y is the identity rotation exactly, n = -Y too (negated first); a plane with n_y = 0 turns by a right angle
    assert np.array_equal(cwipc.cwipc_hip_plane_level_matrix((0, 1, 0, 0.5)), [[1, 0, 0, 0], [0, 1, 0, 0.5], [0, 0, 1, 0], [0, 0, 0, 1]])
    assert np.array_equal(cwipc.cwipc_hip_plane_level_matrix((0, -2, 0, 1.0)), [[1, 0, 0, 0], [0, 1, 0, -0.5], [0, 0, 1, 0], [0, 0, 0, 1]])
    assert np.array_equal(cwipc.cwipc_hip_plane_level_matrix((1, 0, 0, 0)), [[0, -1, 0, 0], [1, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
