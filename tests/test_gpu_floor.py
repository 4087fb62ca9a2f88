"""The floor and tile helpers of the registration pipeline on the GPU (csrc/kernels_floor.hip, the entry points in csrc/registration.cpp,
the wrappers in util.py) against the numpy model of tests/floor_model.py, which tests/test_floor_model.py pins on the CPU.

Every cloud the library returns is compared with the model's as bytes -- count, order and all four planes -- and its timestamp and
cellsize are checked (the input's timestamp; cellsize 0, that of a cloud fresh from cwipc_from_numpy_matrix, whatever the input
had).  Sizes: the wave (64) and 256-point edges, one point below, at and above the kernels' 1024-point workgroup tile, several
tiles with a ragged tail, both sides of 262144 (the scan kernel's and the bounds kernel's second round) and of 524288 (the
second grid-stride round of the histogram kernels).
"""
import numpy as np
import pytest

import floor_model as model
from conftest import make_cloud

pytestmark = pytest.mark.gpu

TILE = 1024                    # csrc/kernels_floor.hip FTILE
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 5 * TILE + 3, 262144, 262145, 524288, 524289, 600001]
KEEP_FLOOR, KEEP_REST, LIMIT = 1, 2, 4
TS, CS = 987654321, 0.03125    # the input's timestamp and a cellsize the results must NOT inherit

_clouds = {}


def random_points(n, seed=0):
    """A seeded cloud, made once per size and left unchanged: y around the default level, a handful of tiles, every point distinct."""
    key = (n, seed)
    if key not in _clouds:
        rng = np.random.default_rng(1000 + 7 * n + seed)
        pts = model.empty(n)
        pts['x'] = rng.uniform(-3, 3, n)
        pts['y'] = rng.uniform(-0.2, 0.5, n)
        pts['z'] = rng.uniform(-3, 3, n)
        pts['r'], pts['g'], pts['b'] = rng.integers(0, 256, n), rng.integers(0, 256, n), rng.integers(0, 256, n)
        pts['tile'] = rng.choice([1, 2, 4, 8, 3], n)
        pts.setflags(write=False)
        _clouds[key] = pts
    return _clouds[key]


def check(out, exp, what=None):
    got = out.get_numpy_array()
    assert len(got) == len(exp), (what, len(got), len(exp))
    if got.tobytes() != exp.tobytes():
        bad = np.flatnonzero((got.view(np.uint8).reshape(-1, 16) != exp.view(np.uint8).reshape(-1, 16)).any(axis=1))
        raise AssertionError((what, "differing points", len(bad), bad[:8].tolist()))
    assert out.count() == len(exp), what
    assert out.timestamp() == TS and out.cellsize() == 0, (what, out.timestamp(), out.cellsize())


def partition_model(pts, level, flags, radius):
    f = model.is_floor(pts, level)
    first = pts[f] if flags & (KEEP_FLOOR | LIMIT) else pts[:0]
    if flags & LIMIT:
        with np.errstate(invalid='ignore'):
            first = first[model.norm3(first['x'], first['y'], first['z']) < radius]
    rest = pts[~f] if flags & KEEP_REST else pts[:0]
    return np.concatenate((first, rest)), len(first)


def check_all_flags(gpu, pts, level=0.1, radius=2.0, what=None):
    pc = make_cloud(gpu, pts, CS, TS)
    for flags in (KEEP_FLOOR, KEEP_REST, KEEP_FLOOR | KEEP_REST, KEEP_FLOOR | KEEP_REST | LIMIT, KEEP_FLOOR | LIMIT):
        exp, n_first = partition_model(pts, level, flags, radius)
        out, got_first = gpu.cwipc_hip_floor_partition(pc, level, flags, radius)
        assert got_first == n_first, (what, flags, got_first, n_first)
        check(out, exp, (what, flags))
    check(gpu.cwipc_floor_filter(pc, level), model.floor_filter(pts, level), (what, "filter"))
    check(gpu.cwipc_floor_filter(pc, level, True), model.floor_filter(pts, level, True), (what, "filter keep"))
    check(gpu.cwipc_limit_floor_to_radius(pc, radius, level), model.limit_floor_to_radius(pts, radius, level), (what, "limit"))


# ---------------------------------------------------------------------------
# partition
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_partition_sizes(gpu, n):
    check_all_flags(gpu, random_points(n), what=n)


@pytest.mark.parametrize("n", [1, 64, 257, TILE + 1, 5 * TILE + 3])
def test_partition_patterns(gpu, n):
    base = random_points(n)
    i = np.arange(n)
    patterns = {
        "all floor": np.full(n, -1.0), "no floor": np.full(n, 1.0),
        "last lane": np.where(i % 256 >= 252, 0.0, 1.0), "last point of a wave step": np.where(i % 256 == 255, 0.0, 1.0),
        "last point": np.where(i == n - 1, 0.0, 1.0), "first point": np.where(i == 0, 0.0, 1.0),
        "alternating": np.where(i % 2 == 0, 0.0, 1.0), "alternating lanes": np.where((i // 4) % 2 == 0, 0.0, 1.0),
        "nan": np.where(i % 3 == 0, np.nan, np.where(i % 3 == 1, 0.0, 1.0)), "all nan": np.full(n, np.nan),
    }
    for name, y in patterns.items():
        pts = base.copy()
        pts['y'] = y
        check_all_flags(gpu, pts, what=(n, name))


def test_partition_level_boundaries(gpu):
    """y exactly float32(level) and its two neighbours, for levels handed in as Python floats, np.float32 and np.float64."""
    n = 3 * TILE + 7
    for level in (0.1, 0.7, np.float32(0.7), np.float64(0.7), np.float64(0.1), 0, -0.0, 1, np.float32(-2.5), float('inf'), float('-inf'), float('nan')):
        lf = np.float32(level)
        near = np.array([lf, np.nextafter(lf, np.float32(-np.inf)), np.nextafter(lf, np.float32(np.inf)), -lf, np.nan, np.inf, -np.inf, 0.0, -0.0],
                        dtype=np.float32)
        pts = random_points(n).copy()
        pts['y'] = near[np.arange(n) % len(near)]
        check_all_flags(gpu, pts, level=level, what=("level", repr(level)))
    # the rule of the wrapper, end to end: float32(0.7) is floor for the double 0.7 and is not for the Python float 0.7
    pts = random_points(64).copy()
    pts['y'] = np.float32(0.7)
    pc = make_cloud(gpu, pts, CS, TS)
    assert gpu.cwipc_floor_filter(pc, 0.7, True).count() == 0 and gpu.cwipc_floor_filter(pc, np.float64(0.7), True).count() == 64


def test_partition_radius_boundaries(gpu):
    """d exactly equal to the radius and its neighbours: (3, 0, 4) 2^k has norm 5 2^k and (2, -3, 6) 2^k has 7 2^k, exactly."""
    n = 2 * TILE + 5
    for k in (-20, -3, 0, 5, 40):
        s = np.float32(2.0) ** k
        five, seven = np.float32(5) * s, np.float32(7) * s
        pts = random_points(n).copy()
        i = np.arange(n)
        pts['x'] = np.where(i % 2 == 0, 3 * s, 2 * s)
        pts['y'] = np.where(i % 2 == 0, 0, -3 * s)
        pts['z'] = np.where(i % 2 == 0, 4 * s, 6 * s)
        pts['y'][i % 5 == 4] = np.float32(1e30)          # some points that are not floor
        # (x, y and z one float32 step away from the exact triples: norms on either side)
        pts['x'][i % 7 == 3] = np.nextafter(pts['x'][i % 7 == 3], np.float32(np.inf))
        pts['z'][i % 7 == 5] = np.nextafter(pts['z'][i % 7 == 5], np.float32(0))
        assert model.norm3(3 * s, 0, 4 * s) == five and model.norm3(2 * s, -3 * s, 6 * s) == seven
        level = 0.1 if k <= 0 else 1e20
        for r in (five, seven):
            for radius in (r, np.nextafter(r, np.float32(0)), np.nextafter(r, np.float32(np.inf)), float(r), np.float64(r) * (1 + 2.0 ** -40),
                           np.float64(r) * (1 - 2.0 ** -40)):
                check_all_flags(gpu, pts, level=level, radius=radius, what=("radius", k, repr(radius)))
    # non-finite coordinates and radii: overflowing squares (d = inf), NaN
    pts = random_points(TILE + 9).copy()
    pts['y'] = 0
    pts['x'][::3] = np.float32(3e19)
    pts['z'][1::5] = np.nan
    for radius in (1.0, float('inf'), float('nan'), 0.0, -1.0):
        check_all_flags(gpu, pts, radius=radius, what=("non-finite", radius))


def test_partition_of_a_filter_result_and_shared_planes(gpu):
    """An input whose planes are spaced wider than its size (a compaction's result), and the results that are the input itself."""
    pts = random_points(5 * TILE + 3).copy()
    pc = make_cloud(gpu, pts, CS, TS)
    sub = gpu.cwipc_tilefilter(pc, 2)
    check(gpu.cwipc_floor_filter(sub), model.floor_filter(pts[pts['tile'] == 2]), "of a tile filter's result")
    high = pts.copy()
    high['y'] = 1
    hpc = make_cloud(gpu, high, CS, TS)
    out = gpu.cwipc_floor_filter(hpc)
    check(out, high, "every point kept")
    assert gpu.cwipc_hip_device_planes(out)[:4] == gpu.cwipc_hip_device_planes(hpc)[:4]
    check(gpu.cwipc_floor_filter(hpc, 0.1, True), high[:0], "no point kept")
    assert hpc.cellsize() == CS and hpc.get_numpy_array().tobytes() == high.tobytes()      # the input is untouched


@pytest.mark.parametrize("y,name", [(-1.0, "all floor"), (1.0, "no floor")])
def test_same_planes_exit_and_its_result_as_an_input(gpu, y, name):
    """One class holds every one of 4096 points: the partition's result holds the input's planes, with the input's tile set.  It is
    the input point for point, and a cloud like any other: into a join with itself, a tile filter, a second partition that splits it."""
    n = 4096
    pts = random_points(n).copy()
    pts['y'] = y
    pc = make_cloud(gpu, pts, CS, TS)
    assert gpu.get_tiles_used(pc) == [1, 2, 3, 4, 8]        # (a census: the cloud knows its tiles from here on)
    out, n_first = gpu.cwipc_hip_floor_partition(pc, 0.1, KEEP_FLOOR | KEEP_REST, 0.0)
    assert n_first == (n if y < 0 else 0)
    check(out, pts, name)
    assert gpu.cwipc_hip_device_planes(out) == gpu.cwipc_hip_device_planes(pc)
    assert gpu.cwipc_tilefilter(out, 16).count() == 0      # (not a point looked at: the tile set came along)
    joined = gpu.cwipc_join(out, out)
    assert joined.count() == 2 * n and joined.get_numpy_array().tobytes() == np.concatenate((pts, pts)).tobytes()
    assert gpu.cwipc_tilefilter(out, 2).get_numpy_array().tobytes() == pts[pts['tile'] == 2].tobytes()
    # a second partition, at a level in x's terms: turn the cloud so that x becomes y
    turn = np.array([[0, 1, 0, 0], [1, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float64)
    turned = pts.copy()
    turned['x'], turned['y'] = pts['y'], pts['x']
    again, first = gpu.cwipc_hip_floor_partition(gpu.cwipc_transform(out, turn), 0.0, KEEP_FLOOR | KEEP_REST, 0.0)
    exp, exp_first = partition_model(turned, 0.0, KEEP_FLOOR | KEEP_REST, 0.0)
    assert 0 < first == exp_first < n and again.get_numpy_array().tobytes() == exp.tobytes()
    assert pc.get_numpy_array().tobytes() == pts.tobytes()                                  # the input is untouched


# ---------------------------------------------------------------------------
# shuffle
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_randomize_floor_equals_the_model(gpu, n):
    pts = random_points(n)
    pc = make_cloud(gpu, pts, CS, TS)
    for seed in (0, 12345, (1 << 64) - 1):
        check(gpu.cwipc_randomize_floor(pc, seed=seed), model.randomize_floor(pts, seed=seed), (n, seed))
    assert pc.get_numpy_array().tobytes() == pts.tobytes()


def test_randomize_floor_properties(gpu):
    n = 1000
    pts = random_points(n).copy()
    pts['y'] = 0
    pts['tile'] = np.where(np.arange(n) < 500, 1, 2)
    rest = random_points(300, 1).copy()
    rest['y'] = 1
    both = np.concatenate((pts, rest))
    pc = make_cloud(gpu, both, CS, TS)
    a = gpu.cwipc_randomize_floor(pc, seed=1).get_numpy_array()
    b = gpu.cwipc_randomize_floor(pc, seed=2).get_numpy_array()
    assert a.tobytes() != b.tobytes() and not np.array_equal(a['tile'][:n], pts['tile'])
    for out in (a, b, gpu.cwipc_randomize_floor(pc).get_numpy_array(), gpu.cwipc_randomize_floor(pc, 0.1).get_numpy_array()):
        for f in ('x', 'y', 'z', 'r', 'g', 'b'):
            assert out[f].tobytes() == both[f].tobytes(), f                       # floor first, rest behind: the input's order here
        assert out[n:].tobytes() == rest.tobytes()                              # the non-floor part is untouched
        assert np.bincount(out['tile'][:n], minlength=3).tolist() == [0, 500, 500]   # the multiset of floor tiles is kept
    # all floor / no floor / one floor point
    check(gpu.cwipc_randomize_floor(make_cloud(gpu, pts, CS, TS), seed=5), model.randomize_floor(pts, seed=5), "all floor")
    check(gpu.cwipc_randomize_floor(make_cloud(gpu, rest, CS, TS), seed=5), rest, "no floor")
    one = np.concatenate((rest[:70], pts[:1], rest[70:]))
    check(gpu.cwipc_randomize_floor(make_cloud(gpu, one, CS, TS), seed=5), np.concatenate((pts[:1], rest)), "one floor point")
    # the filter
    from cwipc_util_amd import filters
    f = filters.factory("randomize_floor(0.1, 9)")
    check(f.filter(pc), model.randomize_floor(both, seed=9), "filter")
    assert f.count == 1 and len(f.times) == 1


# ---------------------------------------------------------------------------
# radius statistics
# ---------------------------------------------------------------------------
def cloud_from_distances(floor_x, rest_x, rng=None, floor_z=None, rest_z=None):
    """Points (x, y, z) with the given x (and z, default 0) per class, the classes interleaved in a seeded random order."""
    nf, nr = len(floor_x), len(rest_x)
    pts = model.empty(nf + nr)
    pts['x'] = np.concatenate((np.asarray(floor_x, dtype=np.float32), np.asarray(rest_x, dtype=np.float32)))
    pts['z'] = np.concatenate((np.zeros(nf) if floor_z is None else floor_z, np.zeros(nr) if rest_z is None else rest_z)).astype(np.float32)
    pts['y'] = np.concatenate((np.full(nf, -0.5), np.full(nr, 0.5)))
    pts['tile'] = 1
    if rng is not None:
        pts = pts[rng.permutation(nf + nr)]
    return pts


def check_radius(gpu, pts, level=0.1, what=None):
    pc = make_cloud(gpu, pts, CS, TS)
    count, stat = gpu.cwipc_hip_floor_radius_stats(pc, level)
    exp_count, exp_stat = model.radius_stats(pts, level)
    assert count.tolist() == exp_count.tolist(), (what, count, exp_count)
    assert np.array_equal(stat, exp_stat, equal_nan=True), (what, stat, exp_stat, stat.view(np.uint32), exp_stat.view(np.uint32))
    got, exp = gpu.cwipc_compute_radius(pc, level), model.compute_radius(pts, level)
    assert all(isinstance(v, np.float32) for v in got), got
    assert np.array_equal(np.array(got), np.array(exp), equal_nan=True), (what, got, exp)


@pytest.mark.parametrize("n", SIZES)
def test_radius_sizes(gpu, n):
    check_radius(gpu, random_points(n), what=n)


def test_radius_class_sizes(gpu):
    rng = np.random.default_rng(21)
    for nf in (0, 1, 2, 100, 101, 102):
        for nr in (0, 1, 2, 100, 101, 102):
            pts = cloud_from_distances(rng.uniform(0, 3, nf), rng.uniform(0, 5, nr), rng, rng.uniform(-3, 3, nf), rng.uniform(-1, 1, nr))
            check_radius(gpu, pts, what=(nf, nr))


def consecutive_floats(v, below, above):
    """The float32 values from `below` steps under v to `above` steps over it, ascending."""
    bits = np.float32(v).view(np.uint32).astype(np.int64)
    return (bits + np.arange(-below, above + 1)).astype(np.uint32).view(np.float32)


def test_radius_adversarial_values(gpu):
    rng = np.random.default_rng(22)
    # all-equal distances
    for n in (1, 2, 101, 2 * TILE + 1):
        check_radius(gpu, cloud_from_distances(np.full(n, 1.25), np.full(n + 3, 0.75), rng), what=("equal", n))
    # distances that differ only in the lowest mantissa byte of the key: s = 1 + j^2 2^-24, j < 16
    j = rng.integers(0, 16, 3000)
    z = (j * 2.0 ** -12).astype(np.float32)
    s = (np.float32(1) + z * z).view(np.uint32)
    assert len(np.unique(s)) > 8 and (s >> 8 == s[0] >> 8).all()
    check_radius(gpu, cloud_from_distances(np.ones(3000), np.ones(3000), rng, z, z[::-1]), what="low byte")
    # the two order statistics at and around the values where the key crosses a bin boundary of every radix pass: 201 values
    # put rank lo = 198 and rank 199 at, below or above the crossing (x x crosses 0.5: byte 3; 1.0: bytes 2, 1, 0; 1 + 2^-7: bytes 1, 0;
    # 1 + 2^-15: byte 0 alone)
    for v in (np.sqrt(0.5), 1.0, np.sqrt(1 + 2.0 ** -7), np.sqrt(1 + 2.0 ** -15), 2.0 ** -63, 2.0 ** 60):
        for shift in (-2, -1, 0, 1):
            xs = consecutive_floats(v, 198 + shift, 2 - shift)
            assert len(xs) == 201
            keys = (xs * xs).view(np.uint32)
            pts = cloud_from_distances(xs, xs[::-1].copy(), rng)
            check_radius(gpu, pts, what=("crossing", float(v), shift, hex(int(keys[198])), hex(int(keys[199]))))
    # zeros and denormals: squares that are 0, denormal and just normal
    tiny = np.array([0, 0, 0, -0.0, 1e-23, 1e-30, 1e-20, 2e-20, 3e-20, 1.1e-19, 1e-19, 1.2e-19, 2e-19, 5e-10], dtype=np.float32)
    for n in (3, 14, 101, 1500):
        xs = tiny[rng.integers(0, len(tiny), n)]
        check_radius(gpu, cloud_from_distances(xs, np.sort(xs), rng), what=("tiny", n))
    check_radius(gpu, cloud_from_distances(np.zeros(500), -np.zeros(77), rng), what="zeros")
    # huge values and infinite squares; levels handed in the three ways
    big = np.array([1e19, 2e19, 3e19, 1e18, 1.5e19, 1.8e19], dtype=np.float32)
    check_radius(gpu, cloud_from_distances(big[rng.integers(0, 6, 300)], big[rng.integers(0, 3, 300)], rng), what="big")
    pts = random_points(3 * TILE + 1).copy()
    pts['y'][::4] = np.float32(0.7)
    for level in (0.7, np.float32(0.7), np.float64(0.7)):
        check_radius(gpu, pts, level=level, what=("level", repr(level)))


def test_radius_rank_follows_numpy_float32_index(gpu):
    """229402 values: numpy's float32 virtual index is 227107, one above what the product gives in float64 (tests/test_floor_model.py)."""
    n = 229402
    rng = np.random.default_rng(23)
    assert model.percentile99_neighbours(n)[0] == 227107 == int(np.floor(0.99 * (n - 1))) + 1
    xs = rng.uniform(0, 4, n).astype(np.float32)
    pts = cloud_from_distances(xs[:1000], xs, rng)
    check_radius(gpu, pts, what="229402")
    d = np.sort(model.xz_distances(pts[pts['y'] > 0.1]))
    assert gpu.cwipc_compute_radius(make_cloud(gpu, pts, CS, TS))[1] == np.percentile(d, 99) == d[227107]


# ---------------------------------------------------------------------------
# tile histogram
# ---------------------------------------------------------------------------
def check_counts(gpu, pts, what=None):
    pc = make_cloud(gpu, pts, CS, TS)
    for nonfloor in (False, True):
        got = gpu.cwipc_hip_tile_counts(pc, nonfloor)
        exp = np.bincount(pts['tile'][~model.is_floor(pts, 0.1)] if nonfloor else pts['tile'], minlength=256)
        assert got.dtype == np.uint64 and got.tolist() == exp.tolist(), (what, nonfloor)
        assert got.tolist() == model.tile_counts(pts, nonfloor).tolist()
        assert gpu.cwipc_compute_tile_occupancy(pc, 0, nonfloor) == model.occupancy_from_counts(exp), (what, nonfloor)


@pytest.mark.parametrize("n", SIZES)
def test_tile_counts_sizes(gpu, n):
    check_counts(gpu, random_points(n), n)


@pytest.mark.parametrize("n", [257, 5 * TILE + 3, 524289])
def test_tile_counts_values(gpu, n):
    rng = np.random.default_rng(31 + n)
    i = np.arange(n)
    for name, tiles in (("one value", np.full(n, 7)), ("tile 0", np.zeros(n)), ("tile 255", np.full(n, 255)), ("0 and 255", np.where(i % 2, 0, 255)),
                        ("all 256", rng.integers(0, 256, n)), ("all 256 in turn", i % 256), ("runs", (i // 100) % 5),
                        ("one stranger per wave", np.where(i % 64 == 17, 9, 4)), ("strangers first", np.where(i % 64 == 0, 9, 4))):
        pts = random_points(n).copy()
        pts['tile'] = tiles
        check_counts(gpu, pts, (n, name))
    pts = random_points(n).copy()
    pts['y'][::2] = np.nan                                   # NaN is not floor: counted
    pts['y'][1::4] = np.float32(0.1)                         # not below the level either
    check_counts(gpu, pts, (n, "nan"))


def test_tile_occupancy_downsampled_and_tie_order(gpu, synth):
    pts, cellsize = synth(40000)
    pts = pts.copy()
    pts['tile'] = (np.arange(len(pts)) * 7 // 13) % 6 + 1
    pts['y'][::3] -= np.float32(0.9)                         # a floor of its own
    pc = make_cloud(gpu, pts, cellsize, TS)
    for cell in (0.02, 0.05):
        for filterfloor in (False, True):
            chain = gpu.cwipc_downsample(gpu.cwipc_floor_filter(pc) if filterfloor else pc, cell)
            exp = model.occupancy_from_counts(np.bincount(chain.get_numpy_array()['tile'], minlength=256))
            assert exp and gpu.cwipc_compute_tile_occupancy(pc, cell, filterfloor) == exp, (cell, filterfloor)
    # ties: equal counts come in ascending tile order behind larger counts
    tie = model.empty(70)
    tie['tile'] = [9] * 10 + [3] * 20 + [200] * 10 + [1] * 20 + [5] * 10
    tie['y'] = 1
    assert gpu.cwipc_compute_tile_occupancy(make_cloud(gpu, tie, CS, TS)) == [(1, 20), (3, 20), (5, 10), (9, 10), (200, 10)]
    assert gpu.cwipc_compute_tile_occupancy(make_cloud(gpu, tie[:0], CS, TS)) == []


# ---------------------------------------------------------------------------
# bounds and filters
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_bounds_sizes(gpu, n):
    pts = random_points(n).copy()
    if n > 2:
        pts['x'][n // 2] = np.nan
        pts['y'][0] = np.nan
        pts['z'][n - 1] = np.nan
        pts['z'][1] = np.inf
    got = gpu.cwipc_hip_bounds(make_cloud(gpu, pts, CS, TS))
    exp = model.bounds(pts)
    assert got.dtype == np.float32 and np.array_equal(got, exp), (n, got, exp)


def test_bounds_edge_values(gpu):
    for n in (5, TILE + 1):
        pts = model.empty(n)
        pts['x'] = np.nan
        pts['y'] = -np.inf
        pts['z'][:] = 3
        pts['z'][n - 1] = -7.5          # the extreme in the ragged last lane
        got = gpu.cwipc_hip_bounds(make_cloud(gpu, pts, CS, TS))
        assert got.tolist() == [np.inf, -np.inf, -7.5, -np.inf, -np.inf, 3.0]


def test_analyze_filter_against_the_reference_loop(gpu):
    from cwipc_util_amd import filters
    f = filters.factory("analyze")
    loop = model.AnalyzeLoop()
    frames = [random_points(300, 3).copy(), random_points(257, 4).copy(), model.empty(0)]
    frames[0]['x'][5] = np.nan
    frames[1]['y'] += np.float32(2)
    for pts in frames:
        pc = make_cloud(gpu, pts, CS, TS)
        assert f.filter(pc) is pc
        loop.filter(pts)
        assert (f.min_x, f.max_x, f.sum_avg_x, f.min_y, f.max_y, f.sum_avg_y, f.min_z, f.max_z, f.sum_avg_z) == loop.state()
    assert f.count == 3
    big = model.empty(3)
    big['x'] = [2e6, -3e6, np.nan]      # beyond the sentinels: the frame's bounds win over them
    f2, loop2 = filters.factory("analyze"), model.AnalyzeLoop()
    f2.filter(make_cloud(gpu, big, CS, TS))
    loop2.filter(big)
    assert (f2.min_x, f2.max_x, f2.sum_avg_x, f2.min_y, f2.max_y) == loop2.state()[:5]


def test_analyze_filter_statistics_text(gpu, capsys):
    from cwipc_util_amd import filters
    f = filters.factory("analyze")
    pts = model.empty(2)
    pts['x'], pts['y'], pts['z'] = [-1, 3], [0, 1.5], [2, 4]
    f.filter(make_cloud(gpu, pts, CS, TS))
    f.statistics()
    assert capsys.readouterr().out.splitlines() == [
        "analyze: count=1", "analyze: x: min=-1.000, max=3.000, average centroid=1.000", "analyze: y: min=0.000, max=1.500, average centroid=0.750",
        "analyze: z: min=2.000, max=4.000, average centroid=3.000",
        "analyze: approximate adjustment for humans: --filter 'transform(-1.000000, 0, -3.000000, 1.200000)'"]


@pytest.mark.parametrize("n", [TILE + 1, 262145])
def test_limit_floor_to_computed_radius(gpu, n):
    pts = random_points(n)
    pc = make_cloud(gpu, pts, CS, TS)
    radius = gpu.cwipc_compute_radius(pc)[0]
    assert radius == model.compute_radius(pts)[0]
    exp = model.limit_floor_to_radius(pts, model.compute_radius(pts)[0])
    assert 0 < len(exp) < n
    check(gpu.cwipc_limit_floor_to_radius(pc, radius), exp, n)


def test_foreign_order_of_calls_leaves_no_state(gpu):
    """The helpers share the thread's scratch and pinned words with the compaction: interleaved calls keep their results."""
    pts = random_points(5 * TILE + 3)
    pc = make_cloud(gpu, pts, CS, TS)
    for _ in range(3):
        check(gpu.cwipc_floor_filter(pc), model.floor_filter(pts), "floor")
        assert gpu.cwipc_tilefilter(pc, 2).get_numpy_array().tobytes() == pts[pts['tile'] == 2].tobytes()
        check(gpu.cwipc_randomize_floor(pc, seed=3), model.randomize_floor(pts, seed=3), "shuffle")
        assert gpu.cwipc_hip_tile_counts(pc).tolist() == model.tile_counts(pts).tolist()
