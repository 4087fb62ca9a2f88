"""The direction filter's eigen-solver (csrc/smallest_eigvec.hpp: cyclic Jacobi in f64, at most 12 sweeps) compiled for the host
and checked against numpy.linalg.eigh.  CPU only; the host C++ compiler is required (a missing one fails the tests).

Compared up to sign, and only where the relative eigengap (w1 - w0) / w2 is at least 1e-2.  The bound: both solvers are backward
stable (an error of a small multiple of eps * |A|), and the eigenvector of w0 moves by the perturbation over its distance to the
nearest other eigenvalue, |A| / (w1 - w0) = 1 / gap for these positive semi-definite matrices: EIG_C * eps / gap, with EIG_C = 64
for the at most 36 rotations the solver accumulates and eigh's own share.  EIG_TERM = EIG_C * eps / 1e-2 = 1.42e-12 rad is the
eigen-solver term of the GPU tests' bar (tests/test_gpu_direction.py); the largest angles measured here are in DESIGN.md 3.7."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
GAP_MIN = 1e-2
EIG_C = 64.0
EIG_TERM = EIG_C * EPS / GAP_MIN


@pytest.fixture(scope="module")
def solver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler: the eigen-solver cannot be checked"
    lib = str(tmp_path_factory.mktemp("eigvec") / "libeigvec_host.so")
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "cwipc_util_amd", "csrc"),
                    os.path.join(ROOT, "tests", "abi", "eigvec_host.cpp"), "-o", lib], check=True)
    dll = ctypes.CDLL(lib)
    dll.smallest_eigvec_many.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long]
    dll.smallest_eigvec_many.restype = None

    def solve(A):
        A = np.ascontiguousarray(A, dtype=np.float64).reshape(-1, 3, 3)
        out = np.zeros((len(A), 3))
        dll.smallest_eigvec_many(A.ctypes.data, out.ctypes.data, len(A))
        return out
    return solve


def angle(a, b):
    """The angle between the lines of a and b (up to sign), accurate for small angles."""
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=-1), np.abs((a * b).sum(axis=-1)))


def against_eigh(solve, A, label):
    """Asserts the bound where the gap allows; returns {gap decade: largest angle}."""
    got = solve(A)
    assert np.allclose(np.linalg.norm(got, axis=1), 1.0, rtol=0, atol=4 * EPS)
    w, v = np.linalg.eigh(A)
    with np.errstate(divide="ignore", invalid="ignore"):
        gap = np.where(w[:, 2] > 0, (w[:, 1] - w[:, 0]) / w[:, 2], 0.0)
    ok = gap >= GAP_MIN
    ang = angle(got[ok], v[ok][:, :, 0])
    worst = {}
    for dec in (-2, -1):
        sel = (gap[ok] >= 10.0 ** dec) & (gap[ok] < 10.0 ** (dec + 1)) if dec < -1 else gap[ok] >= 0.1
        if sel.any():
            worst[dec] = float(ang[sel].max())
    print("smallest_eigvec against eigh, %s: %d of %d compared, largest angle per gap decade %s" % (label, ok.sum(), len(A), worst))
    assert np.all(ang <= EIG_C * EPS / gap[ok]), (label, float((ang * gap[ok]).max() / EPS))
    return worst


def moment_matrices(rng, n):
    """cnt * S2 - S1 S1^T of random integer offsets up to 2^20 a side (cnt 3 to 128: entries up to about 2^54), flattened along a
    random axis by a random factor so that the gaps spread over every decade."""
    out = np.empty((n, 3, 3))
    for i in range(n):
        cnt = int(rng.integers(3, 129))
        u = rng.integers(-2 ** 20, 2 ** 20 + 1, (cnt, 3)).astype(np.float64)
        flat = 10.0 ** rng.uniform(-4, 0, 3)
        rot, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        u = np.rint((u * flat) @ rot.T).astype(np.int64)
        s1 = u.sum(axis=0)
        s2 = u.T @ u
        out[i] = float(cnt) * s2.astype(np.float64) - np.outer(s1.astype(np.float64), s1.astype(np.float64))
    return out


def test_moment_matrices_of_random_integer_offsets(solver):
    A = moment_matrices(np.random.default_rng(1), 120000)
    assert np.abs(A).max() > 2.0 ** 50
    worst = against_eigh(solver, A, "integer moments")
    assert set(worst) == {-2, -1}


def test_diagonal_matrices_and_the_lowest_index_on_a_tie(solver):
    cases = {(1, 1, 1): 0, (2, 1, 1): 1, (1, 2, 1): 0, (1, 1, 0.5): 2, (3, 2, 2): 1, (0, 0, 0): 0, (5, 0, 0): 1, (7, 3, 9): 1, (4, 6, 1): 2}
    A = np.array([np.diag(d) for d in cases], dtype=np.float64)
    got = solver(A)
    want = np.eye(3)[list(cases.values())]
    assert np.array_equal(got, want)


def test_rank_one_and_rank_two(solver):
    rng = np.random.default_rng(2)
    u, v = rng.normal(size=(5000, 3)), rng.normal(size=(5000, 3))
    one = u[:, :, None] * u[:, None, :]
    got = solver(one)          # the gap is 0: any unit vector orthogonal to u will do
    assert np.all(np.abs((got * u).sum(axis=1)) <= 1e-7 * np.linalg.norm(u, axis=1))
    two = one + v[:, :, None] * v[:, None, :]
    got = solver(two)
    against_eigh(solver, two, "rank 2")
    n = np.cross(u, v)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    w = np.linalg.eigvalsh(two)
    ok = w[:, 1] / w[:, 2] >= GAP_MIN
    assert ok.sum() > 4000 and np.all(angle(got[ok], n[ok]) <= 1e-9)


@pytest.mark.parametrize("power", [100, -100])
def test_entries_scaled_by_powers_of_two(solver, power):
    A = moment_matrices(np.random.default_rng(3), 20000)
    scaled = A * 2.0 ** power
    # every operation of the solver is exact under a power of two (the stop is relative, nothing overflows or goes subnormal)
    assert np.array_equal(solver(scaled), solver(A))
    against_eigh(solver, scaled, "scaled by 2^%d" % power)


def test_one_dominant_off_diagonal_entry(solver):
    rng = np.random.default_rng(4)
    A = np.empty((30000, 3, 3))
    for i in range(len(A)):
        m = np.diag(rng.uniform(0, 1, 3))
        p, q = [(0, 1), (0, 2), (1, 2)][i % 3]
        m[p, q] = m[q, p] = 10.0 ** rng.uniform(0, 8) * rng.choice([-1, 1])
        others = [(a, b) for a, b in [(0, 1), (0, 2), (1, 2)] if (a, b) != (p, q)]
        for a, b in others:
            m[a, b] = m[b, a] = rng.uniform(-1, 1) * (i % 2)
        A[i] = m
    # (indefinite: the gap of against_eigh is taken against w2 > 0, the largest eigenvalue, which is |A| here too)
    against_eigh(solver, A, "dominant off-diagonal")
