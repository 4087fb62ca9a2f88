"""The point-to-plane ICP step's host solve (csrc/plane_fit.hpp: LDL^T with diagonal pivoting of the 6x6 system, open3d's check_det
rule, R = Rz Ry Rx) compiled for the host as a stand-alone program (tests/abi/plane_fit_host.cpp, its own main) with
-fsanitize=address,undefined, and checked against numpy.  CPU only; the host C++ compiler is required (a missing one fails the tests).

Bars:
  * |x - x_numpy|_2 <= 128 * 2^-53 * cond_2(A) * |x_numpy|_2 on random symmetric positive definite systems with cond_2 from 1 to 1e10:
    Higham's forward bound for a Cholesky solve, 2 gamma_19 cond for n = 6 (gamma_19 ~ 19 * 2^-53: 38, rounded up to 64), doubled for
    numpy.linalg.solve's own error.  The largest ratio seen is printed (measured: 0.004).
  * a singular system (rank 3: all normals equal), a zero system, NaN anywhere and det just under 1e-6 give the identity update.
  * every entry of R^T R - I within 4 * 2^-53, R^T R evaluated in extended precision (numpy.longdouble, 64-bit mantissa: the
    test's own rounding is 2^-11 of the bar) -- for the angles of the random systems and for sweeps over +-pi, +-0.1 and +-1e-6
    (measured: 1.5; the header's PLANE_FIT_ORTHO_BOUND says why)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
IU = np.triu_indices(6)


@pytest.fixture(scope="module")
def fit(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler: the plane fit cannot be checked"
    d = tmp_path_factory.mktemp("plane_fit")
    exe = str(d / "plane_fit_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "cwipc_util_amd", "csrc"), os.path.join(ROOT, "tests", "abi", "plane_fit_host.cpp"), "-o", exe], check=True)
    header = open(os.path.join(ROOT, "cwipc_util_amd", "csrc", "plane_fit.hpp")).read()
    assert "PLANE_FIT_MIN_DET = 1e-6" in header   # the rule the header states

    def run(A, b):
        """A: (k, 6, 6) symmetric, b: (k, 6) -> x (k, 6), det (k,), solved (k,) bool, R (k, 3, 3), t (k, 3)"""
        A = np.asarray(A, dtype=np.float64).reshape(-1, 6, 6)
        b = np.asarray(b, dtype=np.float64).reshape(-1, 6)
        records = np.ascontiguousarray(np.concatenate([A[:, IU[0], IU[1]], b], axis=1))
        inp, out = str(d / "in.bin"), str(d / "out.bin")
        records.tofile(inp)
        subprocess.run([exe, inp, out], check=True, timeout=120)
        got = np.fromfile(out, dtype=np.float64).reshape(-1, 20)
        assert len(got) == len(records)
        return got[:, :6], got[:, 6], got[:, 7] == 1.0, got[:, 8:17].reshape(-1, 3, 3), got[:, 17:]
    return run


def rotation(x):
    """Rz(x2) Ry(x1) Rx(x0) by numpy"""
    sa, ca, sb, cb, sc, cc = np.sin(x[0]), np.cos(x[0]), np.sin(x[1]), np.cos(x[1]), np.sin(x[2]), np.cos(x[2])
    Rx = np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]])
    Ry = np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])
    Rz = np.array([[cc, -sc, 0], [sc, cc, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def orthonormality(R):
    """The largest |entry| of R^T R - I, in extended precision"""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -60, "numpy.longdouble has no more bits than float64 here"
    Rl = R.astype(np.longdouble)
    return float(np.abs(np.swapaxes(Rl, -1, -2) @ Rl - np.eye(3, dtype=np.longdouble)).max())


def is_identity(solved, R, t):
    return (not solved) and np.array_equal(R, np.eye(3)) and np.array_equal(t, np.zeros(3))


def test_against_numpy_solve(fit):
    rng = np.random.default_rng(66)
    A, b, conds = [], [], []
    for cond in 10.0 ** np.repeat(np.arange(0, 11), 40):
        Q, _ = np.linalg.qr(rng.normal(size=(6, 6)))
        expo = np.concatenate([[0.0, 1.0], rng.uniform(0, 1, 4)])
        M = (Q * cond ** expo) @ Q.T                  # eigenvalues from 1 to cond: det >= 1
        A.append((M + M.T) / 2)
        b.append(rng.normal(size=6) * 10.0 ** rng.uniform(-3, 3))
    A, b = np.array(A), np.array(b)
    x, det, solved, R, t = fit(A, b)
    assert solved.all()
    worst = worst_ortho = 0.0
    for Ai, bi, xi, di, Ri, ti in zip(A, b, x, det, R, t):
        want = np.linalg.solve(Ai, -bi)
        cond = np.linalg.cond(Ai, 2)
        ratio = float(np.linalg.norm(xi - want)) / (128 * U * cond * float(np.linalg.norm(want)))
        worst = max(worst, ratio)
        assert ratio <= 1.0, (cond, ratio)
        assert abs(di - np.linalg.det(Ai)) <= 128 * U * cond * abs(di)   # (a product of pivots: each within the factorisation's bound)
        assert np.array_equal(ti, xi[3:])
        assert np.abs(Ri - rotation(xi)).max() <= 8 * U
        worst_ortho = max(worst_ortho, orthonormality(Ri))
    print("plane_fit against numpy.linalg.solve: largest error over bound %.3f; worst |R^T R - I| %.2f * 2^-53" % (worst, worst_ortho / U))
    assert worst_ortho <= 4 * U


@pytest.mark.parametrize("scale", [np.pi, 0.1, 1e-6])
def test_rotation_is_orthonormal(fit, scale):
    rng = np.random.default_rng(7)
    want = rng.uniform(-scale, scale, size=(2000, 6))
    want[:8, :3] = scale * np.array([[1, 1, 1], [-1, 1, -1], [0.5, 0.5, 0.5], [1, 0, 0], [0, 1, 0], [0, 0, 1], [0.25, -0.75, 0.5], [0, 0, 0]])
    x, det, solved, R, t = fit(np.tile(np.eye(6), (len(want), 1, 1)), -want)
    assert solved.all() and np.array_equal(x, want) and np.all(det == 1.0)
    worst = max(orthonormality(Ri) for Ri in R)
    print("R = Rz Ry Rx, angles within %g: worst |R^T R - I| %.2f * 2^-53 (bar 4)" % (scale, worst / U))
    assert worst <= 4 * U
    for xi, Ri in zip(x[:50], R[:50]):
        assert np.abs(Ri - rotation(xi)).max() <= 8 * U
        assert abs(np.linalg.det(Ri) - 1.0) <= 16 * U


def plane_system(p, m, r):
    J = np.concatenate([np.cross(p, m), m], axis=1)
    return J.T @ J, J.T @ r


def test_systems_that_are_not_trusted_give_the_identity(fit):
    rng = np.random.default_rng(3)
    p = rng.normal(size=(500, 3))
    r = rng.normal(size=500) * 0.01
    good = plane_system(p, rng.normal(size=(500, 3)), r)
    x, det, solved, R, t = fit(*good)
    assert solved[0] and not np.array_equal(R[0], np.eye(3))
    # all normals equal: J J^T has rank 3 (the plane constrains two rotations and one translation)
    A, b = plane_system(p, np.tile([0.0, 0.0, 1.0], (500, 1)), r)
    assert np.linalg.matrix_rank(A) == 3
    x, det, solved, R, t = fit(A, b)
    assert is_identity(solved[0], R[0], t[0]) and np.array_equal(x[0], np.zeros(6))
    A, b = plane_system(p, np.tile([0.6, 0.0, 0.8], (500, 1)), r)   # ... where rounding leaves tiny pivots of either sign
    assert is_identity(*[v[0] for v in fit(A, b)[2:]])
    # nothing at all
    assert is_identity(*[v[0] for v in fit(np.zeros((6, 6)), np.zeros(6))[2:]])
    # NaN or inf in any place
    for k in range(27):
        A, b = good[0].copy(), good[1].copy()
        for bad in (np.nan, np.inf):
            if k < 21:
                A[IU[0][k], IU[1][k]] = A[IU[1][k], IU[0][k]] = bad
            else:
                b[k - 21] = bad
            assert is_identity(*[v[0] for v in fit(A, b)[2:]]), (k, bad)
    # det on either side of 1e-6 (a diagonal system: det is the product of its entries, the last one decides)
    for last, want_solved in ((0.999e-6, False), (1.001e-6, True), (1e-6 * (1 - 2 ** -50), False)):
        A = np.diag([1.0, 1.0, 1.0, 1.0, 1.0, last])
        x, det, solved, R, t = fit(A, np.full(6, -1e-3 * last))
        assert det[0] == last and solved[0] == want_solved
        if want_solved:
            assert np.allclose(x[0], [1e-3 * last] * 5 + [1e-3], rtol=1e-15)
        else:
            assert is_identity(solved[0], R[0], t[0])
    # a negative pivot (not a sum of squares at all) is turned away whatever the determinant
    A = np.diag([2.0, 2.0, 2.0, 2.0, -2.0, -2.0])
    assert np.linalg.det(A) > 1 and is_identity(*[v[0] for v in fit(A, np.ones(6))[2:]])
