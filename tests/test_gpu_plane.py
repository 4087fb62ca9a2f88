"""Plane segmentation on the GPU (RULE S of include/cwipc_util_amd/hip_ext.h): cwipc_find_plane, cwipc_hip_plane_scores,
cwipc_plane_filter, cwipc_level_to_plane, cwipc_find_planes, the plane and level_floor filters and registration.floor against
tests/plane_model.py, EXACTLY: tables, counts, results and clouds are compared as bytes.  Two geometric checks carry a tolerance, each
derived where it stands: the model's own angle to the scene's true normal, and |y| of the inliers after levelling.

Every GPU step runs in ONE child process under a time limit (_CHILD below: the search cases, then the partitions, then the
scenarios); the tests compare what it left with the model's answers, which are computed once.

  scene       20 000 points: a 30 % noisy tilted floor, a body blob, a wall; distance 0.01, H 1024
  threshold   a lattice plane y = 0 (lattice triples give n = (0, +-1, 0) exactly): points at y = +-distance are in, one float32 step
              beyond they are out; BELOW_IS_INLIER
  tile edges  N around the score kernel's points per workgroup (2048) and its grid stride (512 * 2048), H around its hypothesis block
              (63, 64, 65; 127, 128, 129; 1023, 1024, 1025), 1 and 1000, and H = 257 on 2^20 + 1 points, where a workgroup walks two
              tiles and two hypothesis blocks; n = 0, 1, 2, 3
  invalid     4096 duplicates, collinear points, non-finite coordinates in drawn triples, an all-NaN cloud, far points out to FLT_MAX
  ties        two mirrored sheets: several hypotheses share the top count, the lowest h wins
  constraint  a 15 % floor, where the wall wins unconstrained; with Y within 15 degrees and H 4096 the floor is found
  seeds       two seeds, the same seed twice, a permuted cloud
  partition   all flag combinations, n_first, metadata, an empty class, device-resident input
  and         levelling, cwipc_floor_filter downstream, peeling, four host threads, the two filters through the factory"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import plane_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

FLT_MAX = float(np.finfo(np.float32).max)
TILE, GRID, HBLOCK = 2048, 512, 64      # the score kernel's shape (cwipc_util_amd.util.CWIPC_HIP_PLANE_SCORE_*; asserted below)
DISTANCE = 0.01
Y15 = ((0.0, 1.0, 0.0), 15.0)
THRESHOLD_DISTANCE = 0.5                  # exactly a float32


def threshold_cloud():
    """a 32 x 32 lattice on y = 0 and eight points off it: two each at y = d, the float32 above d, -d, the float32 below -d"""
    g = np.stack(np.meshgrid(np.arange(32), np.arange(32), indexing="ij"), axis=-1).reshape(-1, 2)
    lat = np.stack([g[:, 0] * 0.25, np.zeros(len(g)), g[:, 1] * 0.25], axis=1).astype(np.float32)
    d = np.float32(THRESHOLD_DISTANCE)
    ys = [d, d, np.nextafter(d, np.float32(2)), np.nextafter(d, np.float32(2)), -d, -d, np.nextafter(-d, np.float32(-2)), np.nextafter(-d, np.float32(-2))]
    off = np.float32([[1.0 + k, y, 2.0 + k] for k, y in enumerate(ys)])
    xyz = np.concatenate([lat[:500], off, lat[500:]])
    return xyz, np.arange(500, 508)


def mirrored_sheets():
    g = np.stack(np.meshgrid(np.arange(16), np.arange(16), indexing="ij"), axis=-1).reshape(-1, 2)
    a = np.stack([g[:, 0] * 0.5, np.zeros(len(g)), g[:, 1] * 0.5], axis=1)
    b = a + [0.0, 1.0, 0.0]
    both = np.concatenate([a, b]).astype(np.float32)
    return both[np.random.default_rng(512).permutation(len(both))]


@functools.lru_cache(maxsize=None)
def big_scene():
    return pm.scene(n=GRID * TILE + 1, seed=77)[0]


@functools.lru_cache(maxsize=None)
def search_cases():
    """{name: dict(xyz, distance, H, seed, axis, max_angle, refine)}"""
    cases = {}

    def add(name, xyz, distance=DISTANCE, H=64, seed=0, con=(None, None), refine=True):
        cases[name] = dict(xyz=np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3), distance=distance, H=H, seed=seed, axis=con[0], max_angle=con[1],
                           refine=refine)

    scene = pm.scene()[0]
    add("scene", scene, H=1024)
    add("scene, no refine", scene, H=1024, refine=False)
    add("threshold", threshold_cloud()[0], distance=THRESHOLD_DISTANCE, H=256, refine=False)   # (the refit would tilt the plane towards the eight)
    for n in (TILE - 1, TILE, TILE + 1):
        add("N = %d" % n, scene[:n], H=65)
    big = big_scene()
    for n in (GRID * TILE - 1, GRID * TILE, GRID * TILE + 1):
        add("N = %d" % n, big[:n], H=3)
    add("N = %d, H = 257" % (GRID * TILE + 1), big, H=4 * HBLOCK + 1)     # grid.y is 4 there: block 4 is the first workgroups' second
    for H in (1, HBLOCK - 1, HBLOCK, HBLOCK + 1, 2 * HBLOCK - 1, 2 * HBLOCK, 2 * HBLOCK + 1, 1023, 1024, 1025, 1000):
        add("H = %d" % H, scene[:TILE + 1], H=H, seed=9)
    for n in (0, 1, 2, 3):
        add("n = %d" % n, scene[:n], H=64, seed=3)
    add("4096 duplicates", np.tile(np.float32([[0.3, -1.7, 2.9]]), (4096, 1)))
    t = np.arange(-300, 300, dtype=np.float32)
    add("collinear", np.stack([t, 2 * t, -t], axis=1), distance=0.5)
    rng = np.random.default_rng(3000)
    holes = scene[:3000].copy()
    bad = rng.choice(3000, 300, replace=False)
    for k, i in enumerate(bad):
        holes[i, k % 3] = (np.nan, np.inf, -np.inf)[(k // 3) % 3]
    add("non-finite", holes, H=512)
    add("all NaN", np.full((70, 3), np.nan))
    far = np.float32([(1e6, 0, 0), (-1e6, .5, .5), (3e38, 0, 0), (-3e38, 3e38, -3e38), (FLT_MAX, FLT_MAX, FLT_MAX), (1e6, 0, 0.05)])
    add("far points", np.concatenate([scene[:300], far, scene[300:600]]), H=1024)
    add("ties", mirrored_sheets(), distance=0.125, H=256)
    floor15 = pm.scene(floor_share=0.15)[0]
    add("15 % floor", floor15, H=4096)
    add("15 % floor, Y within 15 degrees", floor15, H=4096, con=Y15)
    add("seed 1", scene[:5000], H=256, seed=1)
    add("seed 2", scene[:5000], H=256, seed=2)
    add("seed 1 again", scene[:5000], H=256, seed=1)
    add("seed 1, permuted", scene[:5000][np.random.default_rng(5).permutation(5000)], H=256, seed=1)
    add("seed 2^64 - 1", scene[:5000], H=256, seed=2 ** 64 - 1)
    return cases


def constraint_of(case):
    import cwipc_util_amd as cw
    return cw.cwipc_plane_constraint(case["axis"], case["max_angle"])


@functools.lru_cache(maxsize=None)
def search_answers():
    """{name: plane_model.Found}, computed once"""
    out = {}
    for name, c in search_cases().items():
        axis, mac = constraint_of(c)
        out[name] = pm.find(c["xyz"], c["distance"], c["H"], c["seed"], axis, mac, c["refine"])
    return out


@functools.lru_cache(maxsize=None)
def partition_cases():
    """{name: (points, plane, distance)}; every case runs with flags 0 .. 7"""
    scene = pm.scene()[0]
    truth = pm.scene()[1:]
    plane = [float(v) for v in truth[0]] + [truth[1]]
    holes = search_cases()["non-finite"]["xyz"]
    xyz, _ = threshold_cloud()
    return {
        "scene": (pm.to_points(scene), plane, DISTANCE),
        "scene, odd size": (pm.to_points(scene[:TILE // 2 + 77]), plane, DISTANCE),
        "non-finite": (pm.to_points(holes), plane, 0.05),
        "threshold": (pm.to_points(xyz), [0.0, 1.0, 0.0, 0.0], THRESHOLD_DISTANCE),
        "threshold, negated": (pm.to_points(xyz), [0.0, -1.0, 0.0, -0.0], THRESHOLD_DISTANCE),
        "empty class": (pm.to_points(scene[:3000]), [0.0, 1.0, 0.0, 1000.0], DISTANCE),
        "one point": (pm.to_points(scene[:1]), plane, DISTANCE),
    }


_CHILD = r"""
import sys, threading, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import torch  # noqa: F401  (as the test session: torch's HIP runtime first)
import cwipc_util_amd as cw
from cwipc_util_amd import filters
from cwipc_util_amd.registration import floor
from conftest import make_cloud
import plane_model as pm
cw.cwipc_hip_set_device(0)
dll = cw.cwipc_util_dll_load()
d = np.load(sys.argv[2], allow_pickle=True)
out = {}

def con(c):
    axis = d["axis_%d" % c]
    return (tuple(axis), float(d["angle_%d" % c])) if len(axis) else (None, None)

# 1. the searches
for c in range(int(d["nsearch"])):
    pc = make_cloud(cw, pm.to_points(d[str(d["xyz_%d" % c])][:int(d["n_%d" % c])]))
    axis, angle = con(c)
    args = (float(d["distance_%d" % c]), int(d["H_%d" % c]), int(d["seed_%d" % c]), axis, angle)
    tab = cw.cwipc_hip_plane_scores(pc, *args)
    for k in ("planes", "counts", "triples", "valid"):
        out["%s_%d" % (k, c)] = tab[k]
    out["result_%d" % c] = np.frombuffer(cw.cwipc_find_plane(pc, *args, refine=bool(d["refine_%d" % c])).tobytes(), dtype=np.uint8)
    pc.free()

# 2. the partitions: flags 0 .. 7; the last result of a case is partitioned once more where it lies
for c in range(int(d["npartition"])):
    pc = make_cloud(cw, d["ppts_%d" % c], cellsize=0.0625, timestamp=4711 + c)
    plane, distance = d["pplane_%d" % c], float(d["pdistance_%d" % c])
    for flags in range(8):
        res, n_first = cw.cwipc_hip_plane_partition(pc, plane, distance, flags)
        out["part_%d_%d" % (c, flags)] = res.get_numpy_array()
        out["partmeta_%d_%d" % (c, flags)] = np.array([n_first, res.timestamp(), res.cellsize(), dll.cwipc_hip_is_device_resident(res.as_cwipc_p())], dtype=np.float64)
        if flags == 3:
            again, first2 = cw.cwipc_hip_plane_partition(res, plane, distance, 2 | 4)
            out["again_%d" % c] = again.get_numpy_array()
            again.free()
        res.free()
    pc.free()

# 3. the scenarios
scene = pm.to_points(d["scene"])
pc = make_cloud(cw, scene, cellsize=0.0078125, timestamp=99)
found = cw.cwipc_find_plane(pc, 0.01, 1024)
levelled = cw.cwipc_level_to_plane(pc, found)
out["levelled"] = levelled.get_numpy_array()
out["level_matrix"] = cw.cwipc_hip_plane_level_matrix(found.plane)
kept = cw.cwipc_floor_filter(levelled, float(d["floor_level"]))
out["floor_filtered"] = kept.get_numpy_array()
kept.free(); levelled.free()

two = make_cloud(cw, pm.to_points(d["floor_wall"]))
planes, rest = cw.cwipc_find_planes(two, 0.01, 5, min_inliers=int(d["min_inliers"]), iterations=512, seed=4)
out["peel_results"] = np.stack([np.frombuffer(p.tobytes(), dtype=np.uint8) for p in planes]) if planes else np.zeros((0, 1), dtype=np.uint8)
out["peel_rest"] = rest.get_numpy_array()
out["peel_resident"] = np.array(dll.cwipc_hip_is_device_resident(rest.as_cwipc_p()))
rest.free(); two.free()

results = [None] * 4
def work(i):
    mine = make_cloud(cw, scene)
    results[i] = [cw.cwipc_find_plane(mine, 0.01, 256, seed=100 + i).tobytes() for _ in range(3)]
    mine.free()
threads = [threading.Thread(target=work, args=(i,)) for i in range(4)]
for t in threads: t.start()
for t in threads: t.join()
out["threads"] = np.stack([np.frombuffer(b"".join(r), dtype=np.uint8) for r in results])

for k, desc in enumerate(("plane(0.01)", "plane(0.01, 'inliers', 512, 3)", "plane(0.01, 'both')", "level_floor(0.01)", "level_floor(0.01, 15.0, 4096, 0, True)")):
    f = filters.factory(desc)
    res = f.filter(pc)
    out["filter_%d" % k] = res.get_numpy_array()
    out["filtermeta_%d" % k] = np.array([res.timestamp(), res.cellsize()])
    res.free()
dup = make_cloud(cw, pm.to_points(np.tile(np.float32([[1, 2, 3]]), (50, 1))))
for k, desc in enumerate(("plane(0.01)", "plane(0.01, 'inliers')", "level_floor(0.01)")):
    res = filters.factory(desc).filter(dup)
    out["nofloor_%d" % k] = res.get_numpy_array()
    res.free()
lev, matrix, plane = floor.level_to_floor(pc, 0.01, seed=0)
out["floor_levelled"] = lev.get_numpy_array()
out["floor_matrix"] = matrix
out["floor_plane"] = np.frombuffer(plane.tobytes(), dtype=np.uint8)
out["find_floor"] = np.frombuffer(floor.find_floor(pc, 0.01).tobytes(), dtype=np.uint8)
lev.free(); dup.free(); pc.free()
np.savez(sys.argv[3], **out)
"""

FLOOR_LEVEL = 0.02      # cwipc_floor_filter's level downstream: twice the distance
PEEL_MIN_INLIERS = 2000
_child_cache = {}


def floor_wall():
    """the scene without its body blob, more or less: floor and wall are the two planes to peel"""
    return pm.scene(n=12000, floor_share=0.5, seed=21)[0]


@pytest.fixture(scope="module")
def child(gpu, tmp_path_factory):
    """what the one child process computed, run once"""
    if "out" not in _child_cache:
        assert (gpu.CWIPC_HIP_PLANE_SCORE_TILE, gpu.CWIPC_HIP_PLANE_SCORE_GRID, gpu.CWIPC_HIP_PLANE_SCORE_HBLOCK) == (TILE, GRID, HBLOCK)
        tmp = tmp_path_factory.mktemp("plane")
        inp, out = str(tmp / "in.npz"), str(tmp / "out.npz")
        cases = search_cases()
        arrays = {"nsearch": np.array(len(cases)), "npartition": np.array(len(partition_cases())), "scene": pm.scene()[0], "floor_wall": floor_wall(),
                  "floor_level": np.float64(FLOOR_LEVEL), "min_inliers": np.array(PEEL_MIN_INLIERS), "big": big_scene()}
        for c, case in enumerate(cases.values()):
            xyz = case["xyz"]
            if len(xyz) > 100000:     # (slices of the big scene: stored once)
                arrays["xyz_%d" % c] = np.array("big")
            else:
                arrays["xyz_%d" % c], arrays["own_%d" % c] = np.array("own_%d" % c), xyz
            arrays["n_%d" % c] = np.array(len(xyz))
            arrays["distance_%d" % c], arrays["H_%d" % c], arrays["seed_%d" % c] = np.float64(case["distance"]), np.array(case["H"]), np.array(case["seed"], dtype=np.uint64)
            arrays["axis_%d" % c] = np.array(case["axis"] if case["axis"] is not None else [], dtype=np.float64)
            arrays["angle_%d" % c] = np.float64(case["max_angle"] if case["max_angle"] is not None else 0.0)
            arrays["refine_%d" % c] = np.array(case["refine"])
        for c, (pts, plane, distance) in enumerate(partition_cases().values()):
            arrays["ppts_%d" % c], arrays["pplane_%d" % c], arrays["pdistance_%d" % c] = pts, np.float64(plane), np.float64(distance)
        np.savez(inp, **arrays)
        subprocess.run([sys.executable, "-c", _CHILD, ROOT, inp, out], check=True, timeout=240)
        _child_cache["out"] = dict(np.load(out))
    return _child_cache["out"]


def case_index(name):
    return list(search_cases()).index(name)


def assert_case_equal(child, name):
    c, want = case_index(name), search_answers()[name]
    assert child["triples_%d" % c].tobytes() == want.triples.tobytes(), name
    assert np.array_equal(child["valid_%d" % c], want.valid_rows), (name, np.flatnonzero(child["valid_%d" % c] != want.valid_rows)[:5])
    assert child["planes_%d" % c].tobytes() == want.planes.tobytes(), name
    assert child["counts_%d" % c].dtype == np.uint32 and np.array_equal(child["counts_%d" % c], want.counts), name
    got = child["result_%d" % c].tobytes()
    assert got == want.tobytes(), (name, pm.struct.unpack(pm.RESULT_FORMAT, got), pm.struct.unpack(pm.RESULT_FORMAT, want.tobytes()))


# ---------------------------------------------------------------------------
# the search
# ---------------------------------------------------------------------------
def test_scene(child):
    """The model is held to the scene first: its best normal within 0.5 degrees of the truth (the floor's noise is 0.004 over 4 m: a
    triple's normal is typically within 0.1 degrees), the refit accepted and closer than the hypothesis.  Then the GPU to the model."""
    want = search_answers()["scene"]
    _, normal, d = pm.scene()
    assert want.found and want.refined and want.recount >= want.count > 5800 and want.sums[0] == want.count
    hyp, ref = pm.angle_deg(want.hypothesis, normal), pm.angle_deg(want.plane, normal)
    print("scene: count %d recount %d, hypothesis %.4f deg, refit %.4f deg from the truth" % (want.count, want.recount, hyp, ref))
    assert hyp < 0.5 and ref < hyp and want.plane[1] > 0 and abs(want.plane[3] - d) < DISTANCE
    # the eigenvector of the port against numpy.linalg.eigh of the exact matrix: the gap of a plane's matrix is huge, the angle tiny
    vec, w = pm.eigh_normal(pm.refit_matrix(want.sums)[1])
    assert w[1] > 1e3 * abs(w[0]) and pm.angle_deg(vec, want.plane) < 1e-6
    assert_case_equal(child, "scene")
    assert_case_equal(child, "scene, no refine")
    plain = search_answers()["scene, no refine"]
    assert not plain.refined and plain.plane == pm.orient(plain.hypothesis) and plain.sums == [0] * 10


def test_threshold(child):
    want = search_answers()["threshold"]
    xyz, off = threshold_cloud()
    assert want.found and [abs(v) for v in want.hypothesis] == [0.0, 1.0, 0.0, 0.0] and want.plane[:3] == [0.0, 1.0, 0.0]
    inl = pm.inliers(xyz, want.plane, THRESHOLD_DISTANCE)
    assert inl[off].tolist() == [True, True, False, False, True, True, False, False] and want.count == 1024 + 4 and inl.sum() == want.count
    assert_case_equal(child, "threshold")


@pytest.mark.parametrize("name", [n for n in search_cases() if n.startswith(("N = ", "H = ", "n = "))])
def test_tile_edges(child, name):
    want = search_answers()[name]
    if name.startswith("n = "):
        assert want.found == (1 if name == "n = 3" and want.valid else 0) and (name == "n = 3" or want.valid == 0)
    else:
        assert want.found and want.valid > 0
    assert_case_equal(child, name)


def test_invalid_hypotheses(child):
    ans = search_answers()
    for name in ("4096 duplicates", "collinear", "all NaN"):
        assert not ans[name].found and ans[name].valid == 0 and not ans[name].planes.any(), name
        assert ans[name].tobytes() == pm.Found().tobytes()
    holes, want = search_cases()["non-finite"]["xyz"], ans["non-finite"]
    drawn_bad = ~np.isfinite(holes[want.triples]).all(axis=(1, 2))
    assert drawn_bad.sum() > 50 and not want.valid_rows[drawn_bad].any() and want.found and 0 < want.valid < 512
    far, want = search_cases()["far points"]["xyz"], ans["far points"]
    drawn_far = ((want.triples >= 300) & (want.triples < 306)).any(axis=1)
    assert drawn_far.sum() >= 3 and want.found and want.count > 100
    for name in ("4096 duplicates", "collinear", "all NaN", "non-finite", "far points"):
        assert_case_equal(child, name)


def test_ties(child):
    want = search_answers()["ties"]
    top = np.flatnonzero(want.valid_rows & (want.counts == want.counts.max()))
    sheets = {round(abs(float(want.planes[h][3]))) for h in top}
    assert len(top) >= 4 and sheets == {0, 1} and want.counts.max() == 256 and want.best == top[0]
    assert_case_equal(child, "ties")


def test_constraint(child):
    ans = search_answers()
    free, held = ans["15 % floor"], ans["15 % floor, Y within 15 degrees"]
    _, normal, _ = pm.scene(floor_share=0.15)
    assert pm.angle_deg(free.plane, normal) > 45          # the wall wins
    assert pm.angle_deg(held.plane, normal) < 0.5 and held.refined
    assert free.triples.tobytes() == held.triples.tobytes() and held.valid < free.valid
    assert not (held.valid_rows & ~free.valid_rows).any()
    assert_case_equal(child, "15 % floor")
    assert_case_equal(child, "15 % floor, Y within 15 degrees")


def test_seeds(child):
    for name in ("seed 1", "seed 2", "seed 1 again", "seed 1, permuted", "seed 2^64 - 1"):
        assert_case_equal(child, name)
    one, two, again = case_index("seed 1"), case_index("seed 2"), case_index("seed 1 again")
    assert child["planes_%d" % one].tobytes() != child["planes_%d" % two].tobytes()
    for k in ("planes", "counts", "triples", "valid", "result"):
        assert child["%s_%d" % (k, one)].tobytes() == child["%s_%d" % (k, again)].tobytes(), k


# ---------------------------------------------------------------------------
# the partition
# ---------------------------------------------------------------------------
def test_partition(child):
    for c, (name, (pts, plane, distance)) in enumerate(partition_cases().items()):
        xyz = np.stack([pts["x"], pts["y"], pts["z"]], axis=1)
        for flags in range(8):
            idx, n_first = pm.partition(xyz, plane, distance, flags)
            got, meta = child["part_%d_%d" % (c, flags)], child["partmeta_%d_%d" % (c, flags)]
            assert got.tobytes() == pts[idx].tobytes(), (name, flags)
            assert meta[:3].tolist() == [n_first, 4711 + c, 0.0625] and (len(got) == 0 or meta[3] == 1), (name, flags, meta)
        idx, _ = pm.partition(xyz, plane, distance, 3)
        both = pts[idx]
        idx2, _ = pm.partition(np.stack([both["x"], both["y"], both["z"]], axis=1), plane, distance, 2 | 4)
        assert child["again_%d" % c].tobytes() == both[idx2].tobytes(), name
    # what the constructions are for
    xyz, off = threshold_cloud()
    assert pm.partition(xyz, [0.0, 1.0, 0.0, 0.0], THRESHOLD_DISTANCE, 1)[1] == 1024 + 4
    assert pm.partition(xyz, [0.0, 1.0, 0.0, 0.0], THRESHOLD_DISTANCE, 1 | 4)[1] == 1024 + 6      # ... and the two below -d
    assert pm.partition(xyz, [0.0, -1.0, 0.0, -0.0], THRESHOLD_DISTANCE, 1 | 4)[1] == 1024 + 6    # negated: the two above +d
    pts, plane, distance = partition_cases()["empty class"]
    assert pm.partition(np.stack([pts["x"], pts["y"], pts["z"]], axis=1), plane, distance, 3)[1] == 0
    holes = partition_cases()["non-finite"][0]
    bad = ~np.isfinite(np.stack([holes["x"], holes["y"], holes["z"]], axis=1)).all(axis=1)
    idx, n_first = pm.partition(np.stack([holes["x"], holes["y"], holes["z"]], axis=1), partition_cases()["non-finite"][1], 0.05, 3)
    assert n_first > 500 and bad[idx[:n_first]].sum() == 0       # a non-finite point is never an inlier


# ---------------------------------------------------------------------------
# levelling and what follows it
# ---------------------------------------------------------------------------
def test_levelling_and_floor_filter_downstream(child):
    """After level_to_plane an inlier's |y| is below distance plus rounding.  The bound: in exact arithmetic y' = (n . p + d) / |n|.
    The model's e is that sum with at most four roundings, the matrix entries are rounded once (2^-53 relative), the transform's own
    f64 sum has four roundings more and |n| is within 2^-51 of 1: together within 16 * 2^-53 * (|n_x x| + |n_y y| + |n_z z| + |d|)
    = slack.  The result is rounded to float32: 2^-24 relative.  So |y'| <= (distance + slack) * (1 + 2^-24)."""
    want = search_answers()["scene"]
    scene = pm.scene()[0]
    lev = child["levelled"]
    assert len(lev) == len(scene)
    inl = pm.inliers(scene, want.plane, DISTANCE)
    P = scene.astype(np.float64)
    slack = 16 * 2.0 ** -53 * (np.abs(P * np.float64(want.plane[:3])[None, :]).sum(axis=1) + abs(want.plane[3]))
    bound = (DISTANCE + slack) * (1 + 2.0 ** -24)
    assert inl.sum() == want.recount and np.all(np.abs(lev["y"][inl].astype(np.float64)) <= bound[inl])
    assert np.abs(lev["y"][inl]).max() > 0.9 * DISTANCE          # (the bound is not idle)
    # the rest of the scene is above the floor
    assert (lev["y"][~inl] > DISTANCE).mean() > 0.95
    R = child["level_matrix"][:3, :3]
    # PLANE_FIT_ORTHO_BOUND (4 * 2^-53) for the exact product; numpy's own f64 product rounds three products and two sums below 1
    assert np.abs(R.T @ R - np.eye(3)).max() <= (4 + 5) * 2.0 ** -53
    # downstream: cwipc_floor_filter keeps y >= level, in input order; no point it keeps is one the partition calls an inlier
    keep = ~(lev["y"].astype(np.float64) < float(np.float32(FLOOR_LEVEL)))
    assert child["floor_filtered"].tobytes() == lev[keep].tobytes()
    assert not (keep & inl).any() and keep.sum() > 0.6 * len(scene)
    below = pm.inliers(scene, want.plane, DISTANCE, below=True)
    assert not (keep & below).any()


def test_peeling(child):
    xyz = floor_wall()
    pts = pm.to_points(xyz)
    want, rest = [], pts
    for _ in range(5):
        f = pm.find(np.stack([rest["x"], rest["y"], rest["z"]], axis=1), 0.01, 512, seed=4)
        if not f.found or (f.recount if f.refined else f.count) < PEEL_MIN_INLIERS:
            break
        want.append(f)
        idx, _ = pm.partition(np.stack([rest["x"], rest["y"], rest["z"]], axis=1), f.plane, 0.01, pm.KEEP_REST)
        rest = rest[idx]
    assert len(want) == 2 and pm.angle_deg(want[0].plane, want[1].plane) > 80      # floor and wall
    got = child["peel_results"]
    assert len(got) == 2 and all(got[k].tobytes() == want[k].tobytes() for k in range(2))
    assert child["peel_rest"].tobytes() == rest.tobytes() and int(child["peel_resident"]) == 1 and len(rest) < 3300


def test_four_host_threads(child):
    scene = pm.scene()[0]
    for i in range(4):
        want = pm.find(scene, 0.01, 256, seed=100 + i).tobytes()
        assert child["threads"][i].tobytes() == want * 3, i


def test_filters_and_floor_module(child):
    scene = pm.scene()[0]
    pts = pm.to_points(scene)
    f0 = search_answers()["scene"]
    rest, _ = pm.partition(scene, f0.plane, 0.01, pm.KEEP_REST)
    assert child["filter_0"].tobytes() == pts[rest].tobytes() and child["filtermeta_0"].tolist() == [99, 0.0078125]
    f1 = pm.find(scene, 0.01, 512, seed=3)
    assert child["filter_1"].tobytes() == pts[pm.partition(scene, f1.plane, 0.01, pm.KEEP_INLIERS)[0]].tobytes()
    assert child["filter_2"].tobytes() == pts[pm.partition(scene, f0.plane, 0.01, 3)[0]].tobytes()
    # level_floor: the plane under the Y constraint with 4096 triples, then the levelling; remove drops the floor and what is under it
    import cwipc_util_amd as cw
    axis, mac = cw.cwipc_plane_constraint(*Y15)
    fl = pm.find(scene, 0.01, 4096, 0, axis, mac)
    assert fl.found and pm.angle_deg(fl.plane, pm.scene()[1]) < 0.5
    assert child["floor_plane"].tobytes() == fl.tobytes() == child["find_floor"].tobytes()     # (registration.floor's default distance aside: 0.01 given)
    lev = child["filter_3"]
    assert lev.tobytes() == child["floor_levelled"].tobytes() and len(lev) == len(scene)
    inl = pm.inliers(scene, fl.plane, 0.01)
    assert np.abs(lev["y"][inl]).max() <= 0.01 * (1 + 1e-6) and np.array_equal(lev["r"], pts["r"]) and np.array_equal(lev["tile"], pts["tile"])
    above = ~pm.inliers(scene, fl.plane, 0.01, below=True)
    assert child["filter_4"].tobytes() == lev[above].tobytes() and child["filter_4"]["y"].min() > 0.01 * (1 - 1e-6)
    assert np.array_equal(child["floor_matrix"][3], [0, 0, 0, 1]) and child["floor_matrix"][1, 1] > 0.96
    # a cloud without a plane: nothing removed, nothing kept as the plane, nothing moved
    dup = pm.to_points(np.tile(np.float32([[1, 2, 3]]), (50, 1)))
    assert child["nofloor_0"].tobytes() == dup.tobytes() and len(child["nofloor_1"]) == 0 and child["nofloor_2"].tobytes() == dup.tobytes()
