"""The seeded random filters without a GPU: the draws of tests/scene_model.py against published values, the model's noise against the
reference's expression on the same draws, its distribution, and the Python surface that needs no device (factory, argument checks,
the creator's argument parser)."""
import numpy as np
import pytest

import scene_model as sm
from floor_model import GOLDEN, MASK64, splitmix64


def test_draw_known_values():
    # splitmix64's first output for seed 0 (the state steps by GOLDEN, then the output function)
    assert int(sm.draw(0, 0)) == 0xE220A8397B1DCDAF
    assert int(sm.draw(0, 0)) == int(splitmix64(np.uint64(GOLDEN)))
    assert int(sm.draw(5, 2)) == int(splitmix64(np.uint64((5 + 3 * GOLDEN) & MASK64)))
    assert sm.base(7, sm.TAG_NOISE) == int(splitmix64(np.uint64(7 + 0x6e6f697365)))
    assert sm.base(MASK64, sm.TAG_CAMS) == int(splitmix64(np.uint64(0x63616d73 - 1)))      # (seed + tag) mod 2^64
    assert sm.base(7, sm.TAG_NOISE) != sm.base(7, sm.TAG_CAMS)
    # an array of counters is the scalar draws
    assert sm.draw(99, np.arange(5)).tolist() == [int(sm.draw(99, k)) for k in range(5)]


def test_u01_ends():
    assert float(sm.u01(MASK64)) == 1.0 - 2.0 ** -53
    assert float(sm.u01(0)) == 0.0
    assert float(sm.u01((1 << 11) - 1)) == 0.0 and float(sm.u01(1 << 11)) == 2.0 ** -53


def test_streams_of_shifted_seeds_are_not_shifted_copies():
    a, b = sm.noise_draws(1, 64).ravel(), sm.noise_draws((1 + GOLDEN) & MASK64, 64).ravel()
    assert not np.array_equal(a[1:], b[:-1]) and not np.array_equal(a[:-1], b[1:])


def test_model_noise_is_the_reference_expression_bit_for_bit():
    for seed, distance in ((0, 0.01), (12345, 0.005), (MASK64, 1e30), (3, 0.0)):
        u = sm.noise_draws(seed, 20000)
        got, want = sm.noise_vectors(u, distance), sm.noise_vectors_reference_expression(u, distance)
        assert got.dtype == np.float64 and got.tobytes() == want.tobytes(), (seed, distance)
    # the in-place add of a float64 array to a float32 one (noise.py:35) rounds once, from the f64 sum
    rng = np.random.default_rng(1)
    xyz = (rng.random((20000, 3)) * 4 - 2).astype(np.float32)
    nv = sm.noise_vectors(sm.noise_draws(9, 20000), 0.01)
    inplace = xyz.copy()
    inplace += nv
    assert inplace.dtype == np.float32 and inplace.tobytes() == sm.add_noise(xyz, nv).tobytes()


def test_model_noise_length_is_uniform():
    n, distance = 100000, 0.01
    nv = sm.noise_vectors(sm.noise_draws(12345, n), distance)
    share = np.sqrt((nv * nv).sum(axis=1)) / distance
    assert (np.sqrt((nv * nv).sum(axis=1)) < distance).all()
    # |n| / distance is unif up to rounding: a true uniform sample exceeds 2.7 / sqrt(n) with probability 1e-6 (Kolmogorov)
    ks = sm.ks_distance_from_uniform(share)
    print("KS distance", ks, "bound", 2.7 / np.sqrt(n))
    assert ks < 2.7 / np.sqrt(n)


def test_factory_builds_the_noise_filter():
    from cwipc_util_amd import filters
    from cwipc_util_amd.filters.noise import NoiseFilter
    f = filters.factory("noise(0.01)")
    assert isinstance(f, NoiseFilter) and f.distance == 0.01 and f.seed is None and f.filtername == "noise"
    g = filters.factory("noise(0.01, 7)")
    assert isinstance(g, NoiseFilter) and (g.distance, g.seed) == (0.01, 7)
    assert filters.noise in filters.all_filters and filters.noise.CustomFilter is NoiseFilter
    assert "noise" in NoiseFilter.__doc__ and "distance" in NoiseFilter.__doc__


def test_soft_rule_needs_two_cameras():
    from cwipc_util_amd.filters.simulatecams import SimulatecamsFilter
    with pytest.raises(ValueError):
        SimulatecamsFilter(1, False).filter(None)
    f = SimulatecamsFilter(4, False, 2.0, seed=3)
    assert (f.hard, f.skew, f.seed) == (False, 2.0, 3)
    assert SimulatecamsFilter(4).seed is None and SimulatecamsFilter(4, True).hard is True


def test_library_exports_the_new_symbols(cwipc):
    import cwipc_util_amd
    dll = cwipc.cwipc_util_dll_load()
    assert not dll.cwipc_hip_noise(None, 0.01, 1)
    assert not dll.cwipc_hip_simulatecams_soft(None, 4, 0.0, 0.0, None, 1.0, 1)
    assert "cwipc_hip_noise" in cwipc_util_amd.util.__all__ and "cwipc_hip_simulatecams_soft" in cwipc_util_amd.util.__all__


def test_creator_parser_accepts_the_reference_command_lines():
    from cwipc_util_amd.scripts.cwipc_create_analysis_test import build_parser
    p = build_parser()
    a = p.parse_args(["in.ply", "out.ply"])
    assert (a.input, a.output, a.ncamera, a.skew, a.move, a.rotate, a.tilt, a.noise, a.descr, a.verbose, a.seed) == \
        ("in.ply", "out.ply", 1, 1, None, None, None, 0.0, False, False, None)
    a = p.parse_args(["in.ply", "out.ply", "--ncamera", "4", "--skew", "2.5", "--move", "0", "--move", "0.03", "--rotate", "0", "--rotate", "0",
                      "--rotate", "0.02", "--tilt", "0.01", "--noise", "0.005", "--descr", "--verbose", "--seed", "42"])
    assert (a.ncamera, a.skew, a.move, a.rotate, a.tilt, a.noise, a.descr, a.verbose, a.seed) == \
        (4, 2.5, [0.0, 0.03], [0.0, 0.0, 0.02], [0.01], 0.005, True, True, 42)
    with pytest.raises(SystemExit):
        p.parse_args(["in.ply", "out.ply", "--debugpy"])
