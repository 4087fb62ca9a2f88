"""The seeded random filters on the GPU -- cwipc_hip_noise, cwipc_hip_simulatecams_soft, NoiseFilter, SimulatecamsFilter(hard=False) --
and the analysis-test creator, against the numpy model of tests/scene_model.py (which tests/test_scene_model.py and
tests/test_noise_terms_host.py hold to the reference's expressions and to the header the kernels include).

The noise filter's bar is RAW BITS of every coordinate: both sides are IEEE f64 with one stated order of operations on the same
draws.  The soft camera rule's bar is every tile for skew 1; for other skews every tile except where the model's own chance lies
within 1e-12 of zero relative to the weights (the device's pow and the host's are different routines), at most 0.1 % of the points.
"""
import json

import numpy as np
import pytest

import exact_model as model
import scene_model as sm
from conftest import make_cloud
from floor_model import MASK64

pytestmark = pytest.mark.gpu

#: noise_kernel takes four points per lane, 256 lanes per workgroup and at most 2048 workgroups (NOISE_MAX_BLOCKS, kernels_basic.hip --
#: not grid_for's 8192): the smallest counts at which lanes take a second quad, plus 257 more quads and a ragged tail of three
NOISE_SECOND_ROUND = 2048 * 256 * 4 + 257 * 4 + 3


def planes(gpu, pc):
    return gpu.cwipc_hip_device_planes(pc)[:4]


def resident(gpu, pc):
    return gpu.util.cwipc_util_dll_load().cwipc_hip_is_device_resident(pc.as_cwipc_p()) == 1


def bits(pts):
    return np.stack([pts['x'].view(np.uint32), pts['y'].view(np.uint32), pts['z'].view(np.uint32)], axis=1)


def check_noise(gpu, pts, distance, seed, what):
    pc = make_cloud(gpu, pts, 0.125, 77)
    out = gpu.cwipc_hip_noise(pc, distance, seed)
    assert resident(gpu, out), what
    assert out.count() == len(pts) and out.timestamp() == 77 and out.cellsize() == 0.125, what
    assert planes(gpu, out)[3] == planes(gpu, pc)[3], what                     # colours and tiles: the input's very words
    if len(pts):
        assert planes(gpu, out)[0] != planes(gpu, pc)[0], what
    got, want = out.get_numpy_array(), sm.noise(pts, distance, seed)
    assert len(got) == len(want), what
    bad = np.flatnonzero((bits(got) != bits(want)).any(axis=1))
    assert not len(bad), (what, len(bad), bad[:8].tolist(), bits(got)[bad[:4]].tolist(), bits(want)[bad[:4]].tolist())
    for f in ('r', 'g', 'b', 'tile'):
        assert np.array_equal(got[f], pts[f]), (what, f)
    # how far a point with finite coordinates moves: less than `distance`, plus the rounding of three float32 coordinates
    a = np.stack([pts['x'], pts['y'], pts['z']], axis=1).astype(np.float64)
    b = np.stack([got['x'], got['y'], got['z']], axis=1).astype(np.float64)
    finite = np.isfinite(a).all(axis=1)
    assert np.isfinite(b[finite]).all(), what
    moved = np.sqrt(((b[finite] - a[finite]) ** 2).sum(axis=1))
    biggest = np.maximum(np.abs(a[finite]).max(axis=1, initial=0), np.abs(b[finite]).max(axis=1, initial=0))
    assert (moved <= distance + np.sqrt(3) * 2.0 ** -23 * biggest).all(), (what, moved.max(initial=0))
    # ... and non-finite coordinates stay what they are
    for k in range(3):
        assert np.array_equal(np.isnan(a[:, k]), np.isnan(b[:, k])) and np.array_equal(a[np.isinf(a[:, k]), k], b[np.isinf(a[:, k]), k]), what
    return pc, out, got


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 4099])
def test_noise_bit_for_bit(gpu, n):
    pts = model.edge_cloud(np.random.default_rng(n), n, special=0.4)
    for seed in (0, 1, MASK64):
        for distance in (0.0, 0.01, 1e30):
            check_noise(gpu, pts, distance, seed, (n, seed, distance))


def test_noise_bit_for_bit_where_lanes_take_a_second_quad(gpu):
    pts = model.edge_cloud(np.random.default_rng(8), NOISE_SECOND_ROUND, special=0.05)
    check_noise(gpu, pts, 0.01, 12345, "second round")


def test_noise_seeds_and_sources(gpu):
    pts = model.edge_cloud(np.random.default_rng(21), 4099, special=0.2)
    pc, out, got = check_noise(gpu, pts, 0.01, 99, "seed 99")
    again = gpu.cwipc_hip_noise(pc, 0.01, 99).get_numpy_array()
    assert again.tobytes() == got.tobytes()
    other = gpu.cwipc_hip_noise(pc, 0.01, 100).get_numpy_array()
    assert (bits(other) != bits(got)).any(axis=1).sum() > 3000
    # seed + GOLDEN is another stream, not this one shifted by a point
    assert not np.array_equal(bits(gpu.cwipc_hip_noise(pc, 0.01, 99 + 0x9E3779B97F4A7C15).get_numpy_array())[:-1], bits(got)[1:])
    # a cloud that lives on the device only gives what the host array gave
    dev = make_cloud(gpu, pts, 0.125, 77)
    gpu.cwipc_hip_upload(dev, drop_host_copy=True)
    assert resident(gpu, dev)
    assert gpu.cwipc_hip_noise(dev, 0.01, 99).get_numpy_array().tobytes() == got.tobytes()
    # no seed: 64 bits from the operating system, two calls differ
    a, b = gpu.cwipc_hip_noise(pc, 0.01).get_numpy_array(), gpu.cwipc_hip_noise(pc, 0.01).get_numpy_array()
    assert a.tobytes() != b.tobytes()
    # a result is a cloud like any other: noise on noise
    twice = gpu.cwipc_hip_noise(out, 0.01, 7).get_numpy_array()
    assert twice.tobytes() == sm.noise(got, 0.01, 7).tobytes()


def check_soft(gpu, pts, centroid, ncam, skew, seed, what):
    cams = sm.camera_vectors(ncam)
    pc = make_cloud(gpu, pts, 0.125, 77)
    out = gpu.cwipc_hip_simulatecams_soft(pc, cams, np.asarray(centroid, dtype=np.float32), skew, seed=seed)
    assert resident(gpu, out), what
    assert out.count() == len(pts) and out.timestamp() == 77 and out.cellsize() == 0.125, what
    assert planes(gpu, out)[:3] == planes(gpu, pc)[:3] and planes(gpu, out)[3] != planes(gpu, pc)[3], what
    got = out.get_numpy_array()
    want, fragile = sm.soft_tiles(pts, centroid, ncam, skew, seed)
    if skew == 1.0:
        assert not fragile.any()
    print(what, "left out:", int(fragile.sum()), "of", len(pts))
    assert fragile.sum() <= len(pts) // 1000, what
    bad = np.flatnonzero((got['tile'] != want) & ~fragile)
    assert not len(bad), (what, len(bad), bad[:8].tolist(), got['tile'][bad[:8]].tolist(), want[bad[:8]].tolist())
    for f in ('x', 'y', 'z'):
        assert got[f].tobytes() == pts[f].tobytes(), (what, f)
    for f in ('r', 'g', 'b'):
        assert np.array_equal(got[f], pts[f]), (what, f)
    return got['tile'], want


@pytest.mark.parametrize("ncam", [2, 3, 7, 8])
def test_soft_cameras_skew_one(gpu, ncam):
    for name, (pts, centroid) in sm.tie_inputs().items():
        for seed in (0, MASK64):
            got, want = check_soft(gpu, pts, centroid, ncam, 1.0, seed, (name, ncam, seed))
        if name == "on the centroid":
            assert (got == 1 << (ncam - 2)).all()              # every dot product 0: the chance is 0, not below it
        if name == "random":
            assert len(np.unique(got)) == ncam


@pytest.mark.parametrize("skew", [2.0, 2.5])
@pytest.mark.parametrize("ncam", [2, 3, 7, 8])
def test_soft_cameras_skewed(gpu, ncam, skew):
    for name, (pts, centroid) in sm.tie_inputs().items():
        got, want = check_soft(gpu, pts, centroid, ncam, skew, 3, (name, ncam, skew))
        if name == "random" and skew == 2.5 and ncam <= 3:
            # a negative second dot product: its weight and the chance are NaN, not left out, and `second` it is
            dots = sm.camera_dots(pts['x'], pts['z'], centroid, sm.camera_vectors(ncam))
            cam, chance, _, _ = sm.soft_cameras(dots, skew, sm.cams_draws(3, len(pts)))
            nan = np.isnan(chance)
            assert nan.sum() > 50 and np.array_equal(got[nan], (1 << np.argsort(dots, axis=1, kind="stable")[:, -2])[nan])


def test_soft_cameras_need_two(gpu):
    pts = model.edge_cloud(np.random.default_rng(1), 100, special=0.0)
    pc = make_cloud(gpu, pts)
    with pytest.raises(ValueError):
        gpu.cwipc_hip_simulatecams_soft(pc, sm.camera_vectors(1), np.zeros(3, dtype=np.float32), 1.0, seed=1)
    cams = np.ascontiguousarray(sm.camera_vectors(1)[:, [0, 2]])
    assert not gpu.util.cwipc_util_dll_load().cwipc_hip_simulatecams_soft(pc.as_cwipc_p(), 1, 0.0, 0.0, cams.ctypes.data, 1.0, 1)
    # the hard rule with its positional arguments is what it was
    hard = gpu.cwipc_hip_simulatecams(pc, sm.camera_vectors(1), np.zeros(3, dtype=np.float32)).get_numpy_array()
    assert (hard['tile'] == 1).all()


def test_filters_are_seeded(gpu):
    from cwipc_util_amd.filters.noise import NoiseFilter
    from cwipc_util_amd.filters.simulatecams import SimulatecamsFilter
    pts = model.edge_cloud(np.random.default_rng(31), 5000, special=0.0)
    pc = make_cloud(gpu, pts, 0.25, 11)
    f = NoiseFilter(0.01, seed=5)
    first, second = f.filter(pc), f.filter(pc)
    assert first.get_numpy_array().tobytes() == sm.noise(pts, 0.01, 5).tobytes()
    assert second.get_numpy_array().tobytes() == sm.noise(pts, 0.01, 6).tobytes()
    assert first.timestamp() == 11 and first.cellsize() == 0.25 and resident(gpu, second) and f.count == 2 and len(f.times) == 2
    a, b = NoiseFilter(0.01).filter(pc), NoiseFilter(0.01).filter(pc)
    assert a.get_numpy_array().tobytes() != b.get_numpy_array().tobytes()

    one = SimulatecamsFilter(8, False, 2.0, seed=3).filter(pc).get_numpy_array()
    two = SimulatecamsFilter(8, False, 2.0, seed=3).filter(pc).get_numpy_array()
    assert one.tobytes() == two.tobytes()
    g = SimulatecamsFilter(8, False, 2.0, seed=3)
    assert g.filter(pc).get_numpy_array().tobytes() == one.tobytes() and g.filter(pc).get_numpy_array().tobytes() != one.tobytes()   # frame 1: seed 4
    a, b = SimulatecamsFilter(8, False).filter(pc).get_numpy_array(), SimulatecamsFilter(8, False).filter(pc).get_numpy_array()
    assert a.tobytes() != b.tobytes()
    # the soft tiles are camera bits, and most points go to the nearest camera
    hard = SimulatecamsFilter(8, True).filter(pc).get_numpy_array()
    assert set(np.unique(one['tile'])) <= {1 << c for c in range(8)} and (one['tile'] == hard['tile']).mean() > 0.5
    assert (a['tile'] == hard['tile']).mean() > 0.5
    with pytest.raises(ValueError):
        SimulatecamsFilter(1, False).filter(pc)


SCENE = ["in.ply", "out.ply", "--ncamera", "4", "--skew", "1", "--move", "0", "--move", "0.03", "--rotate", "0", "--rotate", "0", "--rotate", "0.02",
         "--noise", "0.005", "--descr", "--seed", "42"]


def test_creator_is_the_composition_of_the_models(gpu, synth, tmp_path):
    from cwipc_util_amd.scripts.cwipc_create_analysis_test import AnalysisTestCreator, build_parser, rotation_matrix
    pts, cellsize = synth(100000)
    pc = make_cloud(gpu, pts, cellsize, 1234)
    creator = AnalysisTestCreator(build_parser().parse_args(SCENE), input_pc=pc)
    creator.run()
    out = creator.output_pc
    got = out.get_numpy_array()
    assert resident(gpu, out) and out.count() == len(pts) and set(np.unique(got['tile'])) == {1, 2, 4, 8}

    # the ground truth, derived again: tile 1 moved by 3 cm at the first angle of default_rng(42), tile 2 rotated about y
    angle = np.random.default_rng(42).uniform(0, 2 * np.pi)
    moved = np.identity(4)
    moved[0, 3], moved[2, 3] = 0.03 * np.cos(angle), 0.03 * np.sin(angle)
    truth = [np.identity(4), moved, rotation_matrix('y', 0.02), np.identity(4)]
    assert np.allclose(rotation_matrix('y', 0.02)[:3, :3] @ [0, 0, 1], [np.sin(0.02), 0, np.cos(0.02)])
    for cam in range(4):
        assert np.array_equal(creator.transforms[cam], truth[cam]), cam

    # the composition: soft tiles, per-tile transform, concatenation in camera order, noise
    centroid = np.mean(pc.get_numpy_matrix()[:, :3], axis=0)
    centroid[1] = 0.0
    tiles, _ = sm.soft_tiles(pts, centroid, 4, 1.0, 42)
    tiled = pts.copy()
    tiled['tile'] = tiles
    parts = []
    for cam in range(4):
        part = tiled[tiles == 1 << cam]
        assert len(part) > 10000
        parts.append(part if np.array_equal(truth[cam], np.identity(4)) else sm.transform(part, truth[cam]))
    want = sm.noise(np.concatenate(parts), 0.005, 42)
    assert got.tobytes() == want.tobytes()
    assert out.timestamp() == 1234 and out.cellsize() == pc.cellsize()

    # the description: the reference's entries, the seed and every tile's transform
    creator.save_output(str(tmp_path / "scene.ply"))
    d = json.load(open(tmp_path / "scene.json"))
    assert d["seed"] == 42 and d["noise"] == 0.005 and len(d["tiles"]) == 4
    for cam in range(4):
        assert np.array_equal(np.array(d["tiles"][cam]["transform"]), truth[cam]) and set(d["tiles"][cam]) == {"corr", "move", "rotate", "transform"}
    assert d["tiles"][1]["move"] == {"x": moved[0, 3], "y": 0, "z": moved[2, 3]} and d["tiles"][1]["corr"] == 0.03
    assert d["tiles"][2]["rotate"] == {"x": 0, "y": 0.02, "z": 0} and d["tiles"][2]["corr"] == abs(0.2 * 0.02)
    assert gpu.cwipc_read(str(tmp_path / "scene.ply"), 0).count() == len(pts)

    # the same seed, the same cloud; another seed, another cloud
    again = AnalysisTestCreator(build_parser().parse_args(SCENE), input_pc=pc)
    again.run()
    assert again.output_pc.get_numpy_array().tobytes() == got.tobytes()
    other = AnalysisTestCreator(build_parser().parse_args(SCENE[:-1] + ["43"]), input_pc=pc)
    other.run()
    assert other.output_pc.count() == len(pts) and other.output_pc.get_numpy_array().tobytes() != got.tobytes()
