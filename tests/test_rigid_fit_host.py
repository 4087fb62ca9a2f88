"""The ICP step's rigid fit (csrc/rigid_fit.hpp: umeyama without scaling, the SVD by one-sided Jacobi rotations) compiled for the
host as a stand-alone program (tests/abi/rigid_fit_host.cpp, its own main) with -fsanitize=address,undefined, and checked against
the numpy umeyama of tests/icp_model.py.  CPU only; the host C++ compiler is required (a missing one fails the tests).

Bars, from the header: R^T R - I and det R - 1 within RIGID_FIT_BOUND = 64 * 2^-48 = 2.3e-13 on every set, degenerate ones
included.  Against numpy R agrees within RIGID_FIT_BOUND times the condition of the problem, sigma_1 / (sigma_2 + s sigma_3) with
s = sign(det U det V) (two backward stable solvers: each is off by its backward error over the gap that separates the optimum
from the next best rotation), and t within the same times (1 + |cp + mu_a|) -- wherever the optimum is unique.  Where it is not
(collinear or coincident pairs, n < 3: sigma_2 + s sigma_3 = 0) any proper rotation that maps the pairs' common direction onto
its image is a minimiser; there the residual sum |R a + t - b|^2 must equal numpy's within the bound (relative to sum |a|^2 +
|b|^2), and R is still a proper rotation."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import icp_model as im

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 64.0 * 2.0 ** -48


@pytest.fixture(scope="module")
def fit(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler: the rigid fit cannot be checked"
    d = tmp_path_factory.mktemp("rigid_fit")
    exe = str(d / "rigid_fit_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "cwipc_util_amd", "csrc"), os.path.join(ROOT, "tests", "abi", "rigid_fit_host.cpp"), "-o", exe], check=True)
    header = open(os.path.join(ROOT, "cwipc_util_amd", "csrc", "rigid_fit.hpp")).read()
    assert "RIGID_FIT_BOUND = 64.0 * RIGID_FIT_TOL" in header and "3.5527136788005009e-15" in header   # the bound the header states

    def run(records):
        records = np.ascontiguousarray(records, dtype=np.float64).reshape(-1, 22)
        inp, out = str(d / "in.bin"), str(d / "out.bin")
        records.tofile(inp)
        subprocess.run([exe, inp, out], check=True, timeout=120)
        got = np.fromfile(out, dtype=np.float64).reshape(-1, 12)
        assert len(got) == len(records)
        return got[:, :9].reshape(-1, 3, 3), got[:, 9:]
    return run


def record(p, q, cp, cq):
    a, b = p - cp, q - cq
    s = np.concatenate([a.sum(axis=0), b.sum(axis=0), (a[:, :, None] * b[:, None, :]).sum(axis=0).reshape(9)])
    return np.concatenate([[len(p)], s, cp, cq]), s


def make_sets(rng, kind, count):
    """[(p, q, cp, cq)]: q = a rigid (or, reflected, mirrored) image of p plus a little noise."""
    sets = []
    for i in range(count):
        n = {"n1": 1, "n2": 2, "n3": 3}.get(kind, int(rng.integers(4, 200)))
        p = rng.normal(size=(n, 3)) * np.array([3.0, 2.0, 1.0])      # anisotropic: sigma_2 - sigma_3 stays away from 0
        if kind == "planar":
            p[:, 2] = 0.0
        elif kind == "collinear":
            p = np.outer(rng.normal(size=n), rng.normal(size=3))
        elif kind == "coincident":
            p = np.tile(rng.normal(size=3), (n, 1))
        rot, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        if np.linalg.det(rot) < 0:
            rot[:, 0] = -rot[:, 0]
        if kind == "reflected":
            rot = rot @ np.diag([1.0, 1.0, -1.0])
        if kind in ("planar", "collinear", "coincident"):
            p = p @ np.linalg.qr(rng.normal(size=(3, 3)))[0].T
        offset = rng.normal(size=3) * 2
        p = p + offset
        q = p @ rot.T + rng.normal(size=3)
        if kind in ("random", "reflected", "n3"):
            q = q + rng.normal(size=q.shape) * 1e-3
        pivot_error = rng.normal(size=3) * 0.01
        sets.append((p, q, p.mean(axis=0) + pivot_error, q.mean(axis=0) - pivot_error))
    return sets


@pytest.mark.parametrize("kind", ["random", "planar", "collinear", "coincident", "reflected", "n1", "n2", "n3"])
def test_against_numpy_umeyama(fit, kind):
    rng = np.random.default_rng(sum(map(ord, kind)))
    sets = make_sets(rng, kind, 300)
    recs = [record(*s) for s in sets]
    R, t = fit(np.array([r[0] for r in recs]))
    worst_ortho = worst_rel = 0.0
    unique = 0
    for (p, q, cp, cq), (_, s), Ri, ti in zip(sets, recs, R, t):
        n = len(p)
        ortho = max(float(np.abs(Ri.T @ Ri - np.eye(3)).max()), abs(float(np.linalg.det(Ri)) - 1.0))
        worst_ortho = max(worst_ortho, ortho)
        assert ortho <= BOUND, (kind, ortho)
        Rn, tn = im.umeyama(n, np.concatenate([s, [0.0]]), cp, cq)
        sigma = (s[6:15].reshape(3, 3).T - np.outer(s[3:6], s[0:3]) / n) / n
        U, d, Vt = np.linalg.svd(sigma)
        sign = -1.0 if np.linalg.det(U) * np.linalg.det(Vt) < 0 else 1.0
        gap = d[1] + sign * d[2]
        noise = 1e-9 * float(((p - cp) ** 2).sum() + ((q - cq) ** 2).sum()) / n   # a covariance below this is rounding, not data
        if d[0] > noise and gap > 1e-6 * d[0]:
            unique += 1
            cond = d[0] / gap
            rel = float(np.abs(Ri - Rn).max()) / cond
            worst_rel = max(worst_rel, rel)
            assert rel <= BOUND, (kind, rel, cond)
            assert float(np.abs(ti - tn).max()) <= BOUND * cond * (1.0 + float(np.abs(p.mean(axis=0)).max())), kind
        else:
            res = float((((p @ Ri.T + ti) - q) ** 2).sum())
            res_n = float((((p @ Rn.T + tn) - q) ** 2).sum())
            scale = float((p ** 2).sum() + (q ** 2).sum())
            assert abs(res - res_n) <= BOUND * scale, (kind, res, res_n)
    print("rigid_fit against numpy, %s: %d of %d unique; worst orthonormality %.2e, worst |R - R_numpy| / condition %.2e (bound %.2e)"
          % (kind, unique, len(sets), worst_ortho, worst_rel, BOUND))
    if kind in ("random", "planar", "reflected", "n3"):
        assert unique == len(sets)
    if kind in ("collinear", "coincident", "n1", "n2"):
        assert unique == 0


def test_no_pairs_give_the_identity(fit):
    R, t = fit(np.zeros((1, 22)))
    assert np.array_equal(R[0], np.eye(3)) and np.array_equal(t[0], np.zeros(3))
