"""The numpy model of the floor and tile helpers (tests/floor_model.py) against numpy's own functions, on the CPU: the GPU tests
compare the library with the model, these pin the model."""
import numpy as np
import pytest

import floor_model as model


@pytest.fixture(autouse=True)
def library_has_the_helpers(cwipc):
    """The model is the yardstick of five library entry points: a library without them has nothing these tests could vouch for."""
    dll = cwipc.cwipc_util_dll_load()
    for name in ("cwipc_hip_floor_partition", "cwipc_hip_randomize_floor", "cwipc_hip_floor_radius_stats", "cwipc_hip_tile_counts", "cwipc_hip_bounds"):
        assert hasattr(dll, name), name


def test_percentile_step_equals_numpy_percentile():
    rng = np.random.default_rng(11)
    sizes = [1, 2, 3, 50, 100, 101, 102, 399, 4097, 229401, 229402, 229403]   # 101: the weight is 0; 229402: see the next test
    for n in sizes + [int(v) for v in rng.integers(1, 400, 200)]:
        scale = np.float32(rng.choice([1e-3, 1.0, 1e3]))
        d = rng.random(n, dtype=np.float32) * scale
        assert model.percentile99(d).tobytes() == np.percentile(d, 99).tobytes(), n
    for n in (1, 2, 7, 101, 250):
        d = np.full(n, np.float32(0.3), dtype=np.float32)
        assert model.percentile99(d).tobytes() == np.percentile(d, 99).tobytes() == np.float32(0.3).tobytes()
    assert model.percentile99_neighbours(1) == (0, 0, np.float32(0))
    assert model.percentile99_neighbours(2)[:2] == (0, 1)
    assert model.percentile99_neighbours(101) == (99, 100, np.float32(0))


def test_percentile_index_is_computed_in_float32():
    """numpy divides 99 by float32(100) for float32 data: at 229402 values the virtual index 229401 * float32(0.99) rounds up to
    227107.0 in float32, where the same product in float64 is 227106.99 -- one element further down."""
    n = 229402
    assert int(np.floor(0.99 * (n - 1))) == 227106
    assert model.percentile99_neighbours(n) == (227107, 227108, np.float32(0))
    d = np.arange(n, dtype=np.float32)
    assert np.percentile(d, 99) == np.float32(227107) == model.percentile99(d)


def test_norm_equals_numpy_linalg_norm_bit_for_bit():
    rng = np.random.default_rng(12)
    m = (rng.standard_normal((20000, 3)) * 10.0 ** rng.integers(-20, 20, (20000, 1))).astype(np.float32)
    m[:50] = 0
    m[50:60] = np.float32(1e-30)          # squares that are denormal or underflow
    m[60:70] = np.float32(3e19)           # squares that overflow
    with np.errstate(over='ignore'):
        want = np.linalg.norm(m, axis=1)
    assert want.dtype == np.float32
    assert model.norm3(m[:, 0], m[:, 1], m[:, 2]).tobytes() == want.tobytes()
    flat = m.copy()
    flat[:, 1] = 0
    pts = model.empty(len(m))
    pts['x'], pts['y'], pts['z'] = m[:, 0], m[:, 1], m[:, 2]
    with np.errstate(over='ignore'):
        assert model.xz_distances(pts).tobytes() == np.linalg.norm(flat, axis=1).tobytes()


def test_threshold_conversion_rule():
    """y = float32(0.7) is above the double 0.7: a Python float is rounded to float32 before numpy compares (not floor), an
    np.float64 scalar is compared as a double (floor)."""
    y = np.array([np.float32(0.7)], dtype=np.float32)
    assert not (y < 0.7)[0] and (y < np.float64(0.7))[0] and not (y < np.float32(0.7))[0]
    for level in (0.7, np.float64(0.7), np.float32(0.7), 1, np.float64(0.1), 0.1):
        d = model.threshold(level)
        assert isinstance(d, float)
        for v in (np.float32(0.7), np.nextafter(np.float32(0.7), np.float32(0)), np.nextafter(np.float32(0.7), np.float32(1)),
                  np.float32(0.1), np.nextafter(np.float32(0.1), np.float32(0)), np.float32(1), np.float32(np.nan)):
            col = np.array([v], dtype=np.float32)
            assert (float(v) < d) == bool((col < level)[0]), (level, v)
    assert model.threshold(0.7) == float(np.float32(0.7)) != 0.7 == model.threshold(np.float64(0.7))
    pts = model.empty(1)
    pts['y'] = np.float32(0.7)
    assert len(model.floor_filter(pts, 0.7, keep=True)) == 0 and len(model.floor_filter(pts, np.float64(0.7), keep=True)) == 1


def test_product_threshold_matches_the_model(cwipc):
    from cwipc_util_amd.util import _threshold, _percentile99_from_neighbours
    for level in (0.7, np.float64(0.7), np.float32(0.7), 1, 0.1, np.float64(0.1)):
        assert _threshold(level) == model.threshold(level)
    rng = np.random.default_rng(13)
    for n in (1, 2, 50, 101, 399, 229402):
        d = np.sort(rng.random(n, dtype=np.float32))
        lo, hi, _ = model.percentile99_neighbours(n)
        assert _percentile99_from_neighbours(n, d[lo], d[hi]).tobytes() == np.percentile(d, 99).tobytes()
    assert np.isnan(_percentile99_from_neighbours(0, np.float32(0), np.float32(0)))


def test_permutation_model():
    for seed in (0, 1, 0xDEADBEEF, (1 << 64) - 1):
        for n in (0, 1, 2, 1000):
            perm = model.permutation_from_keys(model.shuffle_keys(seed, n))
            assert sorted(perm.tolist()) == list(range(n))
    # splitmix64 of seed 0: the generator's published first outputs
    assert [int(v) for v in model.shuffle_keys(0, 3)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    assert not np.array_equal(model.permutation_from_keys(model.shuffle_keys(1, 1000)), model.permutation_from_keys(model.shuffle_keys(2, 1000)))
    # forced ties: equal keys keep their index order
    keys = np.array([5, 3, 5, 3, 3, 9, 5], dtype=np.uint64)
    assert model.permutation_from_keys(keys).tolist() == [1, 3, 4, 0, 2, 6, 5]
    big = np.array([1 << 63, (1 << 63) - 1, 1 << 63, 0], dtype=np.uint64)   # unsigned order
    assert model.permutation_from_keys(big).tolist() == [3, 1, 0, 2]


def test_model_filters_on_a_small_cloud():
    pts = model.empty(6)
    pts['y'] = [0.0, 0.2, np.nan, 0.05, 0.1, -1.0]
    pts['x'] = [3, 0, 0, 30, 0, 0]
    pts['z'] = [4, 0, 0, 40, 0, 0]
    pts['tile'] = [1, 2, 3, 4, 5, 6]
    assert model.floor_filter(pts)['tile'].tolist() == [2, 3, 5]          # float32(0.1) is not below float32(0.1); NaN is not floor
    assert model.floor_filter(pts, keep=True)['tile'].tolist() == [1, 4, 6]
    assert model.limit_floor_to_radius(pts, 5.0)['tile'].tolist() == [6, 2, 3, 5]    # |(3, 0, 4)| = 5 is not below 5
    assert model.limit_floor_to_radius(pts, 5.1)['tile'].tolist() == [1, 6, 2, 3, 5]
    out = model.randomize_floor(pts, seed=7)
    assert sorted(out['tile'][:3].tolist()) == [1, 4, 6] and out['tile'][3:].tolist() == [2, 3, 5]
    assert out['x'].tolist() == [3, 30, 0, 0, 0, 0]
    assert model.occupancy_from_counts(model.tile_counts(np.concatenate((pts, pts[:2])))) == [(1, 2), (2, 2), (3, 1), (4, 1), (5, 1), (6, 1)]
    assert model.tile_counts(pts, nonfloor_only=True)[[2, 3, 5]].tolist() == [1, 1, 1] and model.tile_counts(pts, nonfloor_only=True).sum() == 3
    b = model.bounds(pts)
    assert b.tolist() == [0, -1, 0, 30, np.float32(0.2), 40]
    loop = model.AnalyzeLoop()
    loop.filter(pts)
    assert loop.state()[:2] == (0.0, 30.0) and loop.min_y == -1.0 and loop.max_y == float(np.float32(0.2))
