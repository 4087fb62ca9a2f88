"""RULE Q's per-pair arithmetic (csrc/quality_terms.hpp: the 10 terms of a matched pair of cwipc_hip_distortion) compiled for the
host as a stand-alone program (tests/abi/quality_terms_host.cpp, its own main) with -ffp-contract=off -fsanitize=address,undefined,
and held to the numpy model (tests/quality_model.py) BIT FOR BIT: both sides are IEEE f64 with one stated order of operations, so
equal bytes are the bar.  The sums kernel includes the same header, and the GPU tests (tests/test_gpu_quality.py) hold the device to
the same model.  CPU only; the host C++ compiler is required (a missing one fails the tests)."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import quality_model as qm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler: quality_terms.hpp cannot be checked"
    d = tmp_path_factory.mktemp("quality_terms")
    exe = str(d / "quality_terms_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "cwipc_util_amd", "csrc"), os.path.join(ROOT, "tests", "abi", "quality_terms_host.cpp"), "-o", exe], check=True)

    def run(p, q, m, has, src_word, ref_word, d2):
        n = len(p)
        rec = np.zeros((n, 13))
        rec[:, 0:3], rec[:, 3:6], rec[:, 6:9] = p, q, m
        rec[:, 9], rec[:, 10], rec[:, 11], rec[:, 12] = has, src_word, ref_word, d2
        inp, out = str(d / "in.bin"), str(d / "out.bin")
        np.ascontiguousarray(rec).tofile(inp)
        subprocess.run([exe, inp, out], check=True, timeout=120)
        got = np.fromfile(out, dtype=np.float64).reshape(-1, qm.NSUM)
        assert len(got) == n
        return got
    return run


def words(rgb, tile):
    """the packed colour words r | g << 8 | b << 16 | tile << 24"""
    rgb = np.asarray(rgb, dtype=np.uint32).reshape(-1, 3)
    return rgb[:, 0] | (rgb[:, 1] << 8) | (rgb[:, 2] << 16) | (np.asarray(tile, dtype=np.uint32) << 24)


def check(host, p, q, m, has, src_rgb, ref_rgb, d2, rng):
    """The program on the packed words (random tile bytes: they must not reach a term) against the model on the colour bytes."""
    n = len(p)
    got = host(p, q, m, has, words(src_rgb, rng.integers(0, 256, n)), words(ref_rgb, rng.integers(0, 256, n)), d2)
    want = qm.pair_terms(p, q, m, has, src_rgb, ref_rgb, d2)
    assert np.isfinite(want).all()
    assert got.tobytes() == want.tobytes()
    return got


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def test_random_pairs_bit_for_bit(host):
    rng = np.random.default_rng(31)
    n = 20000
    p, q = f32(rng.uniform(-3, 3, (n, 3))), f32(rng.uniform(-3, 3, (n, 3)))
    m = rng.normal(size=(n, 3))
    m = f32(m / np.linalg.norm(m, axis=1)[:, None])
    has = rng.integers(0, 2, n).astype(bool)
    got = check(host, p, q, m, has, rng.integers(0, 256, (n, 3)), rng.integers(0, 256, (n, 3)), rng.uniform(0, 1, n), rng)
    assert 5000 < has.sum() < 15000 and np.array_equal(got[:, 1], has.astype(np.float64))
    assert (got[~has, 3] == 0).all() and (got[has, 3] > 0).sum() > 4000
    # negating a normal leaves every term's bits as they are
    assert check(host, p, q, -m, has, rng.integers(0, 1, (n, 3)), rng.integers(0, 1, (n, 3)), np.zeros(n), rng)[:, 3].tobytes() == got[:, 3].tobytes()


def test_every_extreme_colour_difference(host):
    """dR, dG, dB each -255, 0 and 255: the 27 combinations, by hand for the pure ones."""
    rng = np.random.default_rng(32)
    combos = np.array(list(itertools.product((-255, 0, 255), repeat=3)))
    src, ref = np.where(combos > 0, 255, 0), np.where(combos < 0, 255, 0)
    n = len(combos)
    got = check(host, np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n), src, ref, np.zeros(n), rng)
    assert np.array_equal(got[:, 4:7], (combos * combos).astype(np.float64))
    white = got[[tuple(c) == (255, 255, 255) for c in combos]][0]
    # 0.2126 + 0.7152 + 0.0722 = 1 (up to rounding), the chroma rows sum to 0 (up to rounding)
    assert abs(white[7] - 65025.0) < 1e-8 and white[8] < 1e-20 and white[9] < 1e-20
    red = got[[tuple(c) == (255, 0, 0) for c in combos]][0]
    y, u, v = 0.2126 * 255.0, -0.1146 * 255.0, 0.5 * 255.0
    assert red[7] == y * y and red[8] == u * u and red[9] == v * v


def test_zero_normals_denormals_and_the_largest_floats(host):
    rng = np.random.default_rng(33)
    big, tiny = float(np.float32(3.4e38)), float(np.float32(1e-45))
    assert tiny > 0 and tiny < float(np.finfo(np.float32).tiny)
    values = [big, -big, tiny, -tiny, 0.0, 1.0]
    p = np.array(list(itertools.product(values, repeat=3)))
    q = p[::-1].copy()
    n = len(p)
    unit = f32(np.tile([0.6, 0.0, -0.8], (n, 1)))
    e = p - q
    d2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
    for m in (unit, np.zeros((n, 3))):
        got = check(host, p, q, m, np.ones(n), rng.integers(0, 256, (n, 3)), rng.integers(0, 256, (n, 3)), d2, rng)
        assert (got[:, 1] == 1.0).all()                       # a zero normal is a normal: the pair counts, its residual is 0
        assert (got[:, 3] == 0).all() if not m.any() else (got[:, 3] > 1e70).any()
