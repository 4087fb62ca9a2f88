"""The three users of the exact grid walk (exact_walk.hpp: walk_exact) agree with each other and with brute force.

cwipc_hip_correspondences' d2, cwipc_hip_nn_distance2 at nth = 0 and one unrestricted job of cwipc_hip_nn_distance2_jobs answer the
same question for T = identity: the squared f64 distance to the nearest reference point under max_distance.  They share the walk,
so the same 257 doubles must come back bit for bit, and they are the brute-force value of tests/icp_model.py.

Below that: the tie rule and flat references in each of the library's three grid flows (test_each_flow).  What a wrong bound of the
walk does -- it loses an equally distant candidate with a smaller index in a cell across a face -- shows only where reference points
lie ON the grid's faces, and the grid's h is decided on the device, unknown to a test: tests/test_exact_walk_host.py runs the same
header on grids of its own choosing; here several dyadic spacings and offsets are offered, of which one that makes faces and points
coincide is likely, not guaranteed."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import make_cloud
import analyze_oracle as ao
import icp_model as im
from test_gpu_icp import as_points, lattice, midpoints

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

NREF, NSRC = 37, 257
FINITE = 0.3


@pytest.fixture(scope="module")
def clouds():
    """(reference xyz, source xyz): the reference fills a box of half a metre and holds one exact duplicate pair; a good part of the
    source lies outside that box, on every side, and one source point sits on the duplicate pair (a tie at distance 0)."""
    rng = np.random.default_rng(37257)
    ref = rng.uniform(0.0, 0.5, (NREF, 3)).astype(np.float32)
    ref[NREF - 1] = ref[5]
    src = rng.uniform(-0.4, 0.9, (NSRC, 3)).astype(np.float32)
    src[100] = ref[5]
    inside = ((src >= ref.min(axis=0)) & (src <= ref.max(axis=0))).all(axis=1)
    assert 10 < inside.sum() < NSRC - 100
    return ref, src


@pytest.mark.parametrize("max_distance", [np.inf, FINITE], ids=["inf", "finite"])
def test_three_searches_one_answer(gpu, clouds, max_distance):
    ref_xyz, src_xyz = clouds
    ref, src = make_cloud(gpu, as_points(ref_xyz)), make_cloud(gpu, as_points(src_xyz))
    dll = gpu.cwipc_util_dll_load()

    idx, d2_icp = gpu.cwipc_hip_correspondences(src, ref, None, max_distance)

    d2_nn = np.full(NSRC, -1.0)
    assert dll.cwipc_hip_nn_distance2(src.as_cwipc_p(), ref.as_cwipc_p(), 0, float(max_distance), d2_nn.ctypes.data, NSRC) == 0

    table = (gpu.NNJob * 1)(gpu.NNJob(nth=0, max_distance=max_distance))
    d2_job = np.full((1, NSRC), -1.0)
    assert dll.cwipc_hip_nn_distance2_jobs(src.as_cwipc_p(), ref.as_cwipc_p(), ctypes.addressof(table), 1, d2_job.ctypes.data, NSRC) == 0

    want_idx, want = im.correspondences(src_xyz, ref_xyz, None, max_distance)
    assert want.shape == (NSRC,) and want[100] == 0.0 and want_idx[100] == 5
    if np.isfinite(max_distance):
        assert np.isposinf(want).any() and np.isfinite(want).any()   # the bound cuts through this source
    else:
        assert np.isfinite(want).all()
    assert d2_icp.tobytes() == want.tobytes()
    assert d2_nn.tobytes() == want.tobytes()
    assert d2_job[0].tobytes() == want.tobytes()
    assert np.array_equal(idx, want_idx)
    src.free()
    ref.free()


# ---------------------------------------------------------------------------
# ties and flat references, in every grid flow
# ---------------------------------------------------------------------------
NTHS = (0, 1, 3, 31)


def scaled_lattice(spacing, offset, side=16):
    g = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    return (g * spacing + np.array(offset)).astype(np.float32)


def tie_queries(lat, spacing, side=16):
    """Every 29th of the lattice's edge, face and cell midpoints (2, 4, 8 equally distant points; test_gpu_icp.midpoints, which
    is written for the spacing 1/64, scaled), and every 499th of them pushed one and three lattice steps outside the box, through
    each of its six sides: outside along one axis, its ties among the points of that side."""
    unit = lattice(side)
    scale = spacing * 64.0
    mids = np.concatenate([(v.astype(np.float64) - unit[0]) * scale + lat[0] for v in midpoints(unit, side).values()]).astype(np.float32)
    lo, hi = lat.min(axis=0).astype(np.float64), lat.max(axis=0).astype(np.float64)
    out = [mids[::29]]
    for a in range(3):
        for steps in (1, 3):
            for value in (lo[a] - steps * spacing, hi[a] + steps * spacing):
                q = mids[::499].copy()
                q[:, a] = value
                out.append(q)
    return np.concatenate(out).astype(np.float32)


def flow_cases():
    """{name: (reference xyz, source xyz, max_distances)} -- a few thousand points each, the same for every flow."""
    rng = np.random.default_rng(2718)
    cases = {}
    lat = lattice()
    both = np.concatenate([lat, lat])
    refs = {"lattice": lat, "duplicated": both, "permuted": lat[rng.permutation(len(lat))], "duplicated, permuted": both[rng.permutation(len(both))]}
    for name, ref in refs.items():
        cases["ties 1/64, " + name] = (ref, tie_queries(lat, 1 / 64), (np.inf, 1 / 128))      # 1/128: the 2-tie distance, strictly excluded
    for spacing in (1 / 32, 1 / 128):
        for offset in ((0.0, 0.0, 0.0), (1.0, 0.5, -1.0)):
            sl = scaled_lattice(spacing, offset)
            cases["ties %g at %s" % (spacing, offset)] = (sl[rng.permutation(len(sl))], tie_queries(sl, spacing), (np.inf, spacing / 2))
    # flat references: what cwipc_hip_flatten_y makes for the multi-camera aligner -- no extent in y, dim[1] == 1
    probe = np.concatenate([rng.uniform(-0.2, 1.2, size=(200, 3)), rng.uniform(-30, 30, size=(57, 3))]).astype(np.float32)
    probe[:50, 1] = 0.25
    plane = np.stack([rng.uniform(0, 1, 2000), np.full(2000, 0.25), rng.uniform(0, 1, 2000)], axis=1).astype(np.float32)
    plane[1000:1100] = plane[:100]
    t = rng.uniform(0, 1, 500).astype(np.float32)
    t[250:300] = t[:50]
    line = np.stack([t, np.full(500, np.float32(0.25)), np.full(500, np.float32(-0.5))], axis=1)
    diagonal = np.stack([t, t, t], axis=1)
    one = np.tile(np.float32([[0.5, 0.25, 0.75]]), (64, 1))
    for name, ref in (("plane", plane), ("line along x", line), ("diagonal line", diagonal), ("64 copies of one point", one)):
        q = probe.copy()
        q[100:130] = ref[rng.integers(0, len(ref), 30)]        # queries on reference points: ties at distance 0 where there are duplicates
        assert len(q) == 257
        cases["flat: " + name] = (ref, q, (np.inf, 0.3))
    return cases


_FLOW_CHILD = r"""
import ctypes, sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import torch  # noqa: F401  (as the test session: torch's HIP runtime first)
import cwipc_util_amd as cw
from conftest import make_cloud
cw.cwipc_hip_set_device(0)
dll = cw.cwipc_util_dll_load()
d = np.load(sys.argv[2])
nths = [int(v) for v in d["nths"]]
out = {}
for c in range(int(d["ncases"])):
    ref, src = make_cloud(cw, d["ref_%d" % c]), make_cloud(cw, d["src_%d" % c])
    n = src.count()
    for b, maxd in enumerate(d["maxd_%d" % c]):
        maxd = float(maxd)
        out["idx_%d_%d" % (c, b)], out["d2_%d_%d" % (c, b)] = cw.cwipc_hip_correspondences(src, ref, None, maxd)
        nn = np.full((len(nths), n), -1.0)
        for k, nth in enumerate(nths):
            assert dll.cwipc_hip_nn_distance2(src.as_cwipc_p(), ref.as_cwipc_p(), nth, maxd, nn[k].ctypes.data, n) == 0
        table = (cw.NNJob * len(nths))(*[cw.NNJob(nth=nth, max_distance=maxd) for nth in nths])
        jobs = np.full((len(nths), n), -1.0)
        assert dll.cwipc_hip_nn_distance2_jobs(src.as_cwipc_p(), ref.as_cwipc_p(), ctypes.addressof(table), len(nths), jobs.ctypes.data, n) == 0
        out["nn_%d_%d" % (c, b)], out["jobs_%d_%d" % (c, b)] = nn, jobs
    src.free()
    ref.free()
np.savez(sys.argv[3], **out)
"""


@pytest.fixture(scope="module")
def flow_model():
    """The cases and brute force's answers, computed once for the three flows: per case and bound (idx, d2, {nth: d2}).  Both models
    only compare their unbounded answer with max_distance^2, strictly (icp_model: dd[~(dd < max2)] = inf before the argmin;
    analyze_oracle: where(kth < max2, kth, inf)), so the bounded answers of the lattices are taken from one unbounded run, and the
    models called WITH the bound confirm them on every 16th query; the flat cases call them with the bound outright."""
    cases = flow_cases()
    want = {}
    for name, (ref, src, bounds) in cases.items():
        widx, wd2 = im.correspondences(src, ref, None, np.inf)
        kth = {nth: ao.nn_distance2(src, ref, nth, np.inf) for nth in NTHS}
        for maxd in bounds:
            max2 = np.float64(maxd) * np.float64(maxd)
            every = 1 if name.startswith("flat") else 16
            gone = ~(wd2 < max2)
            idx, d2 = np.where(gone, np.uint32(im.NONE), widx), np.where(gone, np.inf, wd2)
            kk = {nth: np.where(v < max2, v, np.inf) for nth, v in kth.items()}
            i, d = im.correspondences(src[::every], ref, None, maxd)
            assert np.array_equal(i, idx[::every]) and d.tobytes() == d2[::every].tobytes()
            for nth in NTHS:
                assert ao.nn_distance2(src[::every], ref, nth, maxd).tobytes() == kk[nth][::every].tobytes()
            want[(name, maxd)] = (idx, d2, kk)
    # the constructions do what they say
    idx, d2, kk = want[("ties 1/64, duplicated, permuted", np.inf)]
    ref, src, _ = cases["ties 1/64, duplicated, permuted"]
    dd = ((src[:582:3, None, :].astype(np.float64) - ref[None].astype(np.float64)) ** 2).sum(axis=2)
    ties = (dd == dd.min(axis=1, keepdims=True)).sum(axis=1)
    assert {4, 8, 16}.issubset(set(ties.tolist())) and np.array_equal(idx[:582:3], np.argmax(dd == dd.min(axis=1, keepdims=True), axis=1))
    assert np.all(want[("ties 1/64, lattice", 1 / 128)][0][:582] == im.NONE)      # the bound AT the nearest tie distance: no answer
    for name, (ref, _, _) in cases.items():
        if name.startswith("flat"):
            assert np.ptp(ref[:, 1]) == 0 or name == "flat: diagonal line"
    return cases, want


@pytest.mark.parametrize("env", [{}, {"CWIPC_SOR_SMALL_CELLS": "0"}, {"CWIPC_SOR_SPARSE": "1"}], ids=["small clouds", "dense", "sparse"])
def test_each_flow(gpu, flow_model, env, tmp_path):
    """One child process per flow does every case's calls: cwipc_hip_correspondences, cwipc_hip_nn_distance2 at nth 0, 1, 3, 31 and
    one unrestricted job per nth, without a bound and with one -- for the ties exactly the nearest tie distance, where the strict
    bound means no answer.  All of it equals brute force, bit for bit, the index included."""
    cases, want = flow_model
    inp, out = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    arrays = {"ncases": np.array(len(cases)), "nths": np.array(NTHS)}
    for c, (ref, src, bounds) in enumerate(cases.values()):
        arrays["ref_%d" % c], arrays["src_%d" % c], arrays["maxd_%d" % c] = as_points(ref), as_points(src), np.array(bounds, dtype=np.float64)
    np.savez(inp, **arrays)
    subprocess.run([sys.executable, "-c", _FLOW_CHILD, ROOT, inp, out], check=True, timeout=300, env=dict(os.environ, **env))
    got = np.load(out)
    for c, (name, (ref, src, bounds)) in enumerate(cases.items()):
        for b, maxd in enumerate(bounds):
            widx, wd2, kk = want[(name, maxd)]
            label = (env, name, maxd)
            assert got["d2_%d_%d" % (c, b)].tobytes() == wd2.tobytes(), label
            assert np.array_equal(got["idx_%d_%d" % (c, b)], widx), (label, int(np.sum(got["idx_%d_%d" % (c, b)] != widx)))
            for k, nth in enumerate(NTHS):
                assert got["nn_%d_%d" % (c, b)][k].tobytes() == kk[nth].tobytes(), (label, nth)
                assert got["jobs_%d_%d" % (c, b)][k].tobytes() == kk[nth].tobytes(), (label, nth)
            assert got["nn_%d_%d" % (c, b)][0].tobytes() == wd2.tobytes()
