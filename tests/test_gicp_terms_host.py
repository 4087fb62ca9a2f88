"""Generalized ICP's per-point and per-pair arithmetic (csrc/gicp_terms.hpp: the orientation of a normal, the covariance from a
normal, the 30 terms of a matched pair) compiled for the host as a stand-alone program (tests/abi/gicp_terms_host.cpp, its own main)
with -ffp-contract=off -fsanitize=address,undefined, and held to the numpy model (tests/icp_gicp_model.py) BIT FOR BIT: both sides are
IEEE f64 with one stated order of operations, so numpy.array_equal is the bar.  The kernels include the same header, and the GPU
tests (tests/test_gpu_icp_gicp.py) hold the device to the same model.  CPU only; the host C++ compiler is required (a missing one
fails the tests)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import icp_gicp_model as gm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = np.sqrt(1 - 0.995 ** 2)
#: (normal, direction or None): the band around -x where open3d's Rx is the identity, its two sides, the axes, zero normals
BAND = [((-1, 0, 0), None), ((-0.995, S, 0), None), ((-0.98, np.sqrt(1 - 0.98 ** 2), 0), None), ((1, 0, 0), None), ((0, 0, 1), None),
        ((-1, 0, 0), (1, 0, 0)), ((-0.995, S, 0), (1, 0, 0)), ((0.995, -S, 0), (-1, 0, 0)), ((0, 0, 0), (0.6, 0, 0.8)), ((0, 0, 0), (-1, 0, 0)),
        ((0, 0, 0), None), ((0, 1, 0), (np.nan, np.nan, np.nan)), ((0, 0, 0), (np.nan, 0, 0)), ((0, -1, 0), (0, 1, np.nan))]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler: gicp_terms.hpp cannot be checked"
    d = tmp_path_factory.mktemp("gicp_terms")
    exe = str(d / "gicp_terms_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "cwipc_util_amd", "csrc"), os.path.join(ROOT, "tests", "abi", "gicp_terms_host.cpp"), "-o", exe], check=True)

    def run(mode, records, width):
        records = np.ascontiguousarray(records, dtype=np.float64)
        inp, out = str(d / "in.bin"), str(d / "out.bin")
        records.tofile(inp)
        subprocess.run([exe, mode, inp, out], check=True, timeout=120)
        got = np.fromfile(out, dtype=np.float64).reshape(-1, width)
        assert len(got) == len(records)
        return got
    return run


def unit_normals(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1)[:, None]).astype(np.float32)


def test_covariances_bit_for_bit(host):
    rng = np.random.default_rng(2024)
    normals = unit_normals(rng, 10000)
    normals[:2000, 0] = -np.abs(normals[:2000, 0]) * 0.02 - 0.98      # many around the band's edge at -0.99
    for eps in (1e-3, 1e-2, 1.0):
        for direction in (None, rng.normal(size=3)):
            rec = np.zeros((len(normals), 8))
            rec[:, :3] = normals
            if direction is not None:
                rec[:, 3:6], rec[:, 6] = direction, 1.0
            rec[:, 7] = eps
            got = host("cov", rec, 6)
            want = gm.covariances(normals, direction, eps)
            assert np.isfinite(want).all() and np.array_equal(got, want), (eps, direction)
            assert (normals[:, 0] < -0.99).sum() > 100 and (normals[:2000, 0] >= -0.99).sum() > 100


def test_band_cases_bit_for_bit(host):
    for eps in (1e-3, 1.0):
        rec = np.zeros((len(BAND), 8))
        want = np.zeros((len(BAND), 6))
        for k, (m, d) in enumerate(BAND):
            rec[k, :3] = np.float32(m)
            if d is not None:
                rec[k, 3:6], rec[k, 6] = d, 1.0
            rec[k, 7] = eps
            want[k] = gm.covariances(np.float32([m]), d, eps)[0]
        got = host("cov", rec, 6)
        assert np.array_equal(got, want, equal_nan=True)
        assert np.array_equal(np.isnan(got), np.isnan(want))


def random_pairs(rng, n, eps):
    """(p, q, Cs, Ct, R, d2): points within +-2, covariances of random unit normals, one random rotation per pair"""
    p, q = rng.uniform(-2, 2, size=(n, 3)), rng.uniform(-2, 2, size=(n, 3)).astype(np.float32).astype(np.float64)
    Cs, Ct = gm.covariances(unit_normals(rng, n), None, eps), gm.covariances(unit_normals(rng, n), None, eps)
    R = np.linalg.qr(rng.normal(size=(n, 3, 3)))[0]
    return p, q, Cs, Ct, R, rng.uniform(0, 1, n)


def test_pair_terms_bit_for_bit(host):
    rng = np.random.default_rng(77)
    for eps in (1e-3, 1e-2, 1.0):
        n = 3334
        p, q, Cs, Ct, R, d2 = random_pairs(rng, n, eps)
        got = host("pair", np.concatenate([p, q, Cs, Ct, R.reshape(n, 9), d2[:, None]], axis=1), 30)
        want = np.concatenate([gm.pair_terms(p[k:k + 1], q[k:k + 1], Cs[k:k + 1], Ct[k:k + 1], R[k], d2[k:k + 1]) for k in range(n)])
        assert np.isfinite(want).all()
        assert np.array_equal(got[:, 0], np.ones(n)) and np.array_equal(got[:, 1:], want), eps
        assert np.array_equal(got[:, 29], d2)
