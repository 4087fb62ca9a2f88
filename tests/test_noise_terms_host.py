"""The seeded draws, the noise filter's arithmetic and the soft camera step (csrc/counter_rng.hpp) compiled for the host as a stand-alone
program (tests/abi/noise_terms_host.cpp, its own main) with -ffp-contract=off -fsanitize=address,undefined, and held to the numpy model
(tests/scene_model.py) as RAW BITS.  The kernels include the same header; here the formulas get draws that no seed gives them on the
GPU (u_3 = 0, v = 0) and non-finite coordinates.  CPU only; the host C++ compiler is required (a missing one fails the tests)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import exact_model as model
import scene_model as sm
from floor_model import MASK64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTH = {"draw": 2, "noise": 8, "at": 6, "cams": 74}


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler: counter_rng.hpp cannot be checked"
    d = tmp_path_factory.mktemp("noise_terms")
    exe = str(d / "noise_terms_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "cwipc_util_amd", "csrc"), os.path.join(ROOT, "tests", "abi", "noise_terms_host.cpp"), "-o", exe], check=True)

    def run(mode, slots, out_dtype, width):
        """slots: (n, WIDTH[mode]) 8-byte values, float64 or uint64 columns already viewed as float64"""
        slots = np.ascontiguousarray(slots, dtype=np.float64).reshape(-1, WIDTH[mode])
        inp, out = str(d / "in.bin"), str(d / "out.bin")
        slots.tofile(inp)
        subprocess.run([exe, mode, inp, out], check=True, timeout=120)
        got = np.fromfile(out, dtype=out_dtype).reshape(-1, width)
        assert len(got) == len(slots)
        return got
    return run


def u64_slots(values):
    return np.asarray(values, dtype=np.uint64).view(np.float64)


def noise_records(u, distance, xyz):
    rec = np.zeros((len(u), 8))
    rec[:, :4], rec[:, 4], rec[:, 5:] = u, distance, np.asarray(xyz, dtype=np.float32)
    return rec


def model_noise(u, distance, xyz):
    return sm.add_noise(xyz, sm.noise_vectors(u, distance))


def test_draws_bit_for_bit(host):
    rng = np.random.default_rng(5)
    b = np.concatenate([np.array([0, 0, MASK64, MASK64, 1], dtype=np.uint64), rng.integers(0, 1 << 64, 2000, dtype=np.uint64)])
    k = np.concatenate([np.array([0, MASK64, 0, MASK64, (1 << 63) + 5], dtype=np.uint64), rng.integers(0, 1 << 64, 2000, dtype=np.uint64)])
    got = host("draw", np.stack([u64_slots(b), u64_slots(k)], axis=1), np.uint64, 2)
    want = np.array([int(sm.draw(int(bb), int(kk))) for bb, kk in zip(b[:50], k[:50])], dtype=np.uint64)
    assert got[0, 0] == 0xE220A8397B1DCDAF
    assert np.array_equal(got[:50, 0], want)
    assert np.array_equal(got[:, 1].view(np.float64), sm.u01(got[:, 0]))
    assert ((got[:, 1].view(np.float64) >= 0) & (got[:, 1].view(np.float64) < 1)).all()


def test_noise_on_ordinary_draws_bit_for_bit(host):
    rng = np.random.default_rng(11)
    n = 20000
    xyz = model.edge_cloud(rng, n, special=0.3, finite=True)
    xyz = np.stack([xyz['x'], xyz['y'], xyz['z']], axis=1)
    for seed, distance in ((0, 0.01), (MASK64, 0.0), (77, 1e30)):
        u = sm.noise_draws(seed, n)
        got = host("noise", noise_records(u, distance, xyz), np.uint32, 3)
        want = model_noise(u, distance, xyz)
        assert np.array_equal(got, want.view(np.uint32)), (seed, distance)
        # ... and the same points by seed and index: the header's own draws
        idx = np.arange(n, dtype=np.uint64)
        rec = np.zeros((n, 6))
        rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3:] = u64_slots(np.full(n, seed, dtype=np.uint64)), u64_slots(idx), distance, xyz
        assert np.array_equal(host("at", rec, np.uint32, 3), want.view(np.uint32)), (seed, distance)
    # a point far down a cloud: the counter 4 i + j in 64 bits
    i = (1 << 40) + 3
    u = sm.u01(sm.draw(sm.base(9, sm.TAG_NOISE), 4 * i + np.arange(4, dtype=np.uint64))).reshape(1, 4)
    rec = np.zeros((1, 6))
    rec[0, 0], rec[0, 1], rec[0, 2], rec[0, 3:] = u64_slots([9])[0], u64_slots([i])[0], 0.01, [0.5, -1.25, 2.0]
    assert np.array_equal(host("at", rec, np.uint32, 3), model_noise(u, 0.01, np.float32([[0.5, -1.25, 2.0]])).view(np.uint32))


def test_noise_at_the_edges_bit_for_bit(host):
    """Injected draws.  (A NaN coordinate under v = 0 is left out: which of two NaN operands an addition returns is the host
    compiler's choice of operand order, not the formula's.)"""
    p = np.float32([0.5, -1.25, 2.0])
    cases = []
    for distance in (0.0, 0.01, 1e30):
        cases += [
            ([0.25, 0.75, 0.5, 0.0], distance, p),                                 # u_3 = 0: infinite scale, no noise
            ([0.5, 0.5, 0.5, 0.3], distance, p),                                   # v = 0: s = 0, 0 / 0
            ([0.5, 0.5, 0.5, 0.0], distance, p),                                   # both: 0 / 0 again (scale = 0 / 0)
            ([0.0, 0.0, 0.0, 1 - 2.0 ** -53], distance, p),                        # the corner of the cube, the longest share
            ([1 - 2.0 ** -53] * 4, distance, p),
            ([0.5 + 2.0 ** -53, 0.5, 0.5, 2.0 ** -53], distance, p),               # the shortest vector, the smallest share
            ([0.1, 0.9, 0.4, 0.6], distance, np.float32([np.nan, np.inf, -np.inf])),
            ([0.1, 0.9, 0.4, 0.0], distance, np.float32([np.nan, np.inf, -np.inf])),
            ([0.1, 0.9, 0.4, 0.6], distance, np.float32([model.FLT_MAX, -model.FLT_MAX, 1e-45])),
            ([0.9, 0.1, 0.6, 0.99], distance, np.float32([-0.0, 0.0, -1e-39])),
        ]
    u = np.array([c[0] for c in cases])
    distance = np.array([c[1] for c in cases])
    xyz = np.stack([c[2] for c in cases])
    rec = noise_records(u, 0.0, xyz)
    rec[:, 4] = distance
    got = host("noise", rec, np.uint32, 3)
    want = np.stack([model_noise(u[k:k + 1], distance[k], xyz[k:k + 1])[0] for k in range(len(cases))])
    assert np.array_equal(got, want.view(np.uint32)), [(k, got[k], want[k]) for k in np.flatnonzero((got != want.view(np.uint32)).any(axis=1))]
    # what the edges are: no noise under u_3 = 0 (for a finite distance times 0 ... a finite vector over an infinite scale), NaN under s = 0
    assert np.array_equal(want[0], p) and np.isnan(want[1]).all() and np.isnan(want[2]).all()
    assert np.isnan(want[6][0]) and want[6][1] == np.inf and want[6][2] == -np.inf


def camera_records(pts, centroid, ncam, skew, u=None, seed=None):
    n = len(pts)
    rec = np.zeros((n, 74))
    rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3], rec[:, 4], rec[:, 5] = ncam, pts['x'], pts['z'], np.float32(centroid[0]), np.float32(centroid[2]), skew
    if u is not None:
        rec[:, 7] = u
    else:
        rec[:, 6], rec[:, 8], rec[:, 9] = 1.0, u64_slots(np.full(n, seed, dtype=np.uint64)), u64_slots(np.arange(n, dtype=np.uint64))
    rec[:, 10:10 + 2 * ncam] = sm.camera_vectors(ncam)[:, [0, 2]].ravel()
    return rec


@pytest.mark.parametrize("ncam", [2, 3, 4, 7, 8])
def test_soft_cameras_on_ties_and_random_points(host, ncam):
    for name, (pts, centroid) in sm.tie_inputs().items():
        for skew in (1.0, 2.0, 2.5):
            for seed in (0, 3):
                want, fragile = sm.soft_tiles(pts, centroid, ncam, skew, seed)
                got = host("cams", camera_records(pts, centroid, ncam, skew, seed=seed), np.int32, 1)[:, 0]
                differ = (1 << got) != want
                assert not (differ & ~fragile).any(), (name, ncam, skew, seed, np.flatnonzero(differ & ~fragile)[:8])
                assert fragile.sum() <= len(pts) // 1000
        if name == "on the centroid":
            # every dot product is 0: the order is by camera index alone, the chance is 0, which is not below 0: the second
            assert (want == 1 << (ncam - 2)).all()
        if name == "bisectors" and ncam == 4:
            # the first and second cameras tie: the higher index is `first`; u near 0 takes it, u near 1 the other
            lo = host("cams", camera_records(pts, centroid, 4, 1.0, u=np.zeros(len(pts))), np.int32, 1)[:, 0]
            hi = host("cams", camera_records(pts, centroid, 4, 1.0, u=np.full(len(pts), 1 - 2.0 ** -53)), np.int32, 1)[:, 0]
            dots = sm.camera_dots(pts['x'], pts['z'], centroid, sm.camera_vectors(4))
            order = np.argsort(dots, axis=1, kind="stable")[:, ::-1]
            assert np.array_equal(lo, order[:, 0]) and np.array_equal(hi, order[:, 1])
            tied = dots[np.arange(len(pts)), order[:, 0]] == dots[np.arange(len(pts)), order[:, 1]]
            assert tied.sum() > 50 and (order[tied, 0] > order[tied, 1]).all()


def test_nan_chance_takes_the_second_camera(host):
    """skew 2.5 of a negative second weight is NaN: the comparison `chance < 0` is false"""
    pts, centroid = sm.tie_inputs()["random"]
    dots = sm.camera_dots(pts['x'], pts['z'], centroid, sm.camera_vectors(2))
    cam, chance, _, _ = sm.soft_cameras(dots, 2.5, sm.cams_draws(1, len(pts)))
    assert np.isnan(chance).sum() > 100 and (cam[np.isnan(chance)] == np.argsort(dots, axis=1, kind="stable")[:, 0][np.isnan(chance)]).all()
    got = host("cams", camera_records(pts, centroid, 2, 2.5, seed=1), np.int32, 1)[:, 0]
    assert np.array_equal(got[np.isnan(chance)], cam[np.isnan(chance)])
