"""tests/neigh_model.py, the numpy and scipy model of RULE N, against brute force over all pairs on clouds of up to 300 points, and
the constructions of the GPU tests (tests/test_gpu_neigh.py) held to what their names say.  CPU only.

The model takes its candidates from a k-d tree and sums in int64; brute force looks at every pair and sums in Python integers.  The two
share only the rule's text."""
import numpy as np
import pytest

import neigh_model as nm


def small_clouds():
    rng = np.random.default_rng(300)
    clouds = {}
    clouds["uniform"] = (rng.uniform(0, 1, (300, 3)).astype(np.float32), 0.17, None)
    clouds["uniform, tiles"] = (rng.uniform(0, 1, (300, 3)).astype(np.float32), 0.2, rng.choice(np.uint8([0, 5, 255]), 300))
    xyz = rng.uniform(0, 1, (250, 3)).astype(np.float32)
    xyz[::17, 0] = np.nan
    xyz[5::31, 2] = np.inf
    xyz[9] = -np.inf
    clouds["non-finite"] = (xyz, 0.25, None)
    dup = np.repeat(rng.uniform(0, 1, (40, 3)).astype(np.float32), 5, axis=0)
    clouds["duplicates"] = (dup[rng.permutation(200)], 0.3, rng.choice(np.uint8([1, 2]), 200))
    g = np.stack(np.meshgrid(*[np.arange(6)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    clouds["lattice, r = spacing"] = ((g * 0.25).astype(np.float32), 0.25, None)
    clouds["lattice, one step above"] = ((g * 0.25).astype(np.float32), float(np.nextafter(0.25, 1)), None)
    clouds["one point"] = (np.float32([[1, 2, 3]]), 0.5, None)
    clouds["two points"] = (np.float32([[1, 2, 3], [1, 2, 3.25]]), 0.5, None)
    clouds["far apart"] = (np.float32([[0, 0, 0], [3e38, 0, 0], [-3e38, 3e38, 0], [0, 0, 1e-3]]), 1e30, None)
    clouds["whole cloud"] = (rng.normal(0, 1, (120, 3)).astype(np.float32), 50.0, None)
    return clouds


@pytest.mark.parametrize("name", list(small_clouds()))
def test_model_against_brute_force(name):
    xyz, radius, tiles = small_clouds()[name]
    near = nm.brute_force_neighbours(xyz, radius, tiles)
    pairs = nm.directed_pairs(xyz, radius, tiles)
    assert [(i, j) for i, row in enumerate(near) for j in row] == [tuple(p) for p in pairs.tolist()]
    finite = np.isfinite(xyz).all(axis=1)
    assert all((i in row) == bool(finite[i]) for i, row in enumerate(near))      # a finite point is its own neighbour (r2 > 0)
    cnt = nm.counts(xyz, radius, tiles)
    assert cnt.dtype == np.uint32 and cnt.tolist() == [max(len(row) - 1, 0) for row in near]
    W, S1, S2, n_i = nm.sums(xyz, radius, tiles)
    for i, (bw, b1, b2, bc) in enumerate(nm.brute_force_sums(xyz, radius, tiles)):
        assert (int(W[i]), S1[i].tolist(), S2[i].tolist(), int(n_i[i])) == (bw, b1, b2, bc), (name, i)
        assert bw >= 4096 * bool(finite[i]) and all(abs(v) <= bc << 28 for v in b1) and all(abs(v) <= bc << 44 for v in b2)
    out, moved, gap, _ = nm.smooth_xyz(xyz, radius, 2, tiles)
    assert moved.tolist() == [bool(finite[i]) and len(row) - 1 >= 2 for i, row in enumerate(near)]
    assert out[~moved].tobytes() == np.asarray(xyz, np.float32)[~moved].tobytes()


def test_constructions_of_the_small_clouds():
    clouds = small_clouds()
    assert np.all(nm.counts(*clouds["lattice, r = spacing"][:2]) == 0)
    g = np.stack(np.meshgrid(*[np.arange(6)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    inner = ((g > 0) & (g < 5)).sum(axis=1)         # 3: interior, 2: face, 1: edge, 0: corner
    assert np.array_equal(nm.counts(*clouds["lattice, one step above"][:2]), 3 + inner)
    assert nm.counts(*clouds["far apart"][:2]).tolist() == [1, 0, 0, 1]     # d2 = 9e76 and more: not under r2 = 1e60
    assert np.all(nm.counts(*clouds["whole cloud"][:2]) == 119)
    assert np.all(nm.counts(*clouds["duplicates"][:2]) >= 4)


@pytest.mark.parametrize("radius,want", [(1e-170, 0), (1e-162, 0), (1e-30, 0), (1e200, 299), (1e30, 299)])
def test_radius_extremes(radius, want):
    """RULE K's: r2 == 0 finds nobody (not even the point itself), r2 == inf every finite point"""
    xyz = small_clouds()["uniform"][0]
    assert np.all(nm.counts(xyz, radius) == want)
    dup = np.zeros((7, 3), dtype=np.float32)
    assert np.all(nm.counts(dup, radius) == (0 if radius * radius == 0 else 6))


def test_move_decision():
    for mn in (0, 1, 2, 3, 7, 300000):
        need = max(2, mn)
        for cnt in (1, 2, 3, 4, need, need + 1, need + 2, 262144, 262145, 1 << 20):
            assert nm.moves(cnt, mn) == (cnt - 1 >= need and cnt <= 262144)
    assert not nm.moves(2, 0) and nm.moves(3, 0) and nm.moves(262144, 0) and not nm.moves(262145, 0)


@pytest.mark.parametrize("name", list(nm.SMOOTH_INPUTS))
def test_caps_of_the_smoothing_inputs(name):
    """The share of moved points with an eigengap under GAP_MIN, with the model alone, stays under half the cap that the host-twin
    and the GPU tests allow; the inputs have the neighbourhood sizes their docstrings name."""
    make, cap = nm.SMOOTH_INPUTS[name]
    pts, radius = make()
    out, moved, gap, cnt = nm.smooth_xyz(nm.xyz_of(pts), radius)
    low = (moved & (gap < nm.GAP_MIN)).sum() / moved.sum()
    mean = (cnt - 1).mean()
    print("%s: %d points, %d moved, %.1f neighbours on average, %.2f %% of the moved under the gap (cap %.0f %%)" % (
        name, len(pts), moved.sum(), mean, 100 * low, 100 * cap))
    assert 2 * low <= cap
    assert {"noisy plane": 28 < mean < 33 and moved.all(), "noisy sphere": 21 < mean < 25 and moved.all(),
            "gaussian blob": 0 < (~moved).sum() < 200 and cnt.max() > 200}[name]
    step = np.linalg.norm(out.astype(np.float64) - nm.xyz_of(pts).astype(np.float64), axis=1)
    assert np.all(step[moved] < radius) and np.all(step[~moved] == 0)
    if name == "noisy plane":
        before, after = nm.plane_rms(nm.xyz_of(pts)), nm.plane_rms(out)
        print("noisy plane: rms distance to the true plane %.3e before, %.3e after" % (before, after))
        assert after < 0.5 * before


def test_radius_outlier_filter_of_the_model():
    rng = np.random.default_rng(5)
    xyz = np.concatenate([rng.uniform(0, 1, (280, 3)), rng.uniform(5, 50, (20, 3))]).astype(np.float32)
    xyz[3, 1] = np.nan
    pts = nm.as_points(xyz[rng.permutation(300)], tile=rng.choice(np.uint8([1, 2]), 300))
    near = nm.brute_force_neighbours(nm.xyz_of(pts), 0.2)
    for mn in (0, 1, 3, 400):
        keep = np.array([len(row) >= 1 and len(row) - 1 >= mn for row in near])
        assert nm.radius_outlier_filter(pts, 0.2, mn).tobytes() == pts[keep].tobytes()
    assert len(nm.radius_outlier_filter(pts, 0.2, 0)) == 299 and len(nm.radius_outlier_filter(pts, 0.2, 1)) < 290
    near = nm.brute_force_neighbours(nm.xyz_of(pts), 0.2, pts["tile"])
    keep = np.array([len(row) - 1 >= 2 for row in near])
    assert nm.radius_outlier_filter(pts, 0.2, 2, same_tile=True).tobytes() == pts[keep].tobytes()
