"""cwipc_hip_nn_distance2_jobs / cwipc_hip_nn_distance_jobs on the GPU: the tile-aware batched nearest-distance search.

Two independent yardsticks, both bit for bit (numpy.array_equal, no tolerance -- a distance is a value, it does not depend on the
grid that was walked):
  * the numpy oracle (tests/analyze_oracle.py: nn_distance2_grid_many) on numpy-masked arrays;
  * the existing per-cloud path: cwipc_hip_nn_distance on cwipc_tilefilter_masked / cwipc_crop / cwipc_floor_filter clouds.
"""
import ctypes
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from conftest import make_cloud
import analyze_oracle as ao
from multicam_frames import make_frame, takes_part, xyz_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
ALL_Y = (-INF, INF)
SAMPLED = 30000
FLOOR32 = float(np.float32(0.1))


def job_tuple(smask=0, rmask=0, nth=0, bound=INF, sy=ALL_Y, ry=ALL_Y):
    return (smask, rmask, nth, bound, sy, ry)


def to_jobs(gpu, tuples):
    return [gpu.NNJob(source_mask=s, reference_mask=r, nth=n, max_distance=b, source_y=sy, reference_y=ry) for s, r, n, b, sy, ry in tuples]


def raw_rows(gpu, src, ref, tuples, cap=None):
    """The C entry itself: (rc, njobs x cap squared distances, NaN where the source point sits out)."""
    jobs = to_jobs(gpu, tuples)
    table = (gpu.NNJob * len(jobs))(*jobs)
    cap = src.count() if cap is None else cap
    out = np.full((len(jobs), max(cap, 1)), -1.0)
    rc = gpu.cwipc_util_dll_load().cwipc_hip_nn_distance2_jobs(src.as_cwipc_p(), ref.as_cwipc_p(), ctypes.addressof(table), len(jobs), out.ctypes.data, cap)
    return rc, out


def oracle_rows(src_pts, ref_pts, tuples, sample_seed=None):
    """Per job (indices of the participating source points that are checked, their distances) from the numpy oracle."""
    rows = []
    for k, (s, r, nth, bound, sy, ry) in enumerate(tuples):
        ps, pr = takes_part(src_pts, s, sy), takes_part(ref_pts, r, ry)
        idx = np.flatnonzero(ps)
        q = np.arange(len(idx))
        if sample_seed is not None and len(idx) > SAMPLED // len(tuples):
            q = np.sort(np.random.default_rng(sample_seed + k).choice(len(idx), SAMPLED // len(tuples), replace=False))
        if pr.any() and len(idx):
            want = np.sqrt(ao.nn_distance2_grid(xyz_of(src_pts[idx[q]]), xyz_of(ref_pts[pr]), nth, bound, per_cell=48))
        else:
            want = np.full(len(q), np.inf)
        rows.append((len(idx), q, want))
    return rows


def existing_path(gpu, src, ref, job):
    """cwipc_hip_nn_distance on the clouds the existing filters make of the job's predicates."""
    s, r, nth, bound, sy, ry = job

    def cut(pc, mask, lim):
        if mask:
            pc = gpu.cwipc_tilefilter_masked(pc, mask)
        if lim[0] != -INF:   # y > lo: a crop whose only finite face is the next float32 above lo
            pc = gpu.cwipc_crop(pc, (-INF, INF, float(np.nextafter(np.float32(lim[0]), np.float32(np.inf))), INF, -INF, INF))
        if lim[1] != INF:    # y < hi
            pc = gpu.cwipc_floor_filter(pc, np.float64(lim[1]), keep=True)
        return pc
    return gpu.cwipc_hip_nn_distance(cut(src, s, sy), cut(ref, r, ry), nth, bound)


def check(gpu, src_pts, ref_pts, tuples, same=False, sample_seed=None, compare_existing=True):
    src = make_cloud(gpu, src_pts)
    ref = src if same else make_cloud(gpu, ref_pts)
    got = gpu.cwipc_hip_nn_distance_jobs(src, ref, to_jobs(gpu, tuples))
    assert len(got) == len(tuples)
    for k, (count, q, want) in enumerate(oracle_rows(src_pts, ref_pts, tuples, sample_seed)):
        assert got[k].dtype == np.float64 and got[k].shape == (count,), (k, tuples[k])
        assert np.array_equal(got[k][q], want), (k, tuples[k], int(np.sum(got[k][q] != want)))
        if compare_existing:
            assert np.array_equal(got[k], existing_path(gpu, src, ref, tuples[k])), (k, tuples[k])
    return got


def camera_jobs(ntiles=4, nths=(0, 1, 3, 31)):
    """Both directions of each camera against the others: eight jobs over all three list widths."""
    out = []
    for k in range(ntiles):
        t = 1 << k
        out.append(job_tuple(t, 0xff ^ t, nths[k % len(nths)]))
        out.append(job_tuple(0xff ^ t, t, nths[(k + 1) % len(nths)]))
    return out


@pytest.fixture(scope="module")
def frames(synth):
    cache = {}

    def get(n):
        if n not in cache:
            pts, _ = synth(int(n / 1.12))
            cache[n] = make_frame(pts, 4, seed=n % 97)
        return cache[n]
    return get


@pytest.mark.parametrize("npoints", [6000, 72000])
def test_eight_jobs_all_list_widths(gpu, frames, npoints):
    frame = frames(npoints)
    assert set(np.unique(frame["tile"]).tolist()) == {1, 2, 4, 8} and np.sum(frame["y"] < 0.1) > npoints // 20
    got = check(gpu, frame, frame, camera_jobs(), same=True, sample_seed=None if npoints <= 6000 else 1)
    assert any(np.any(row == 0.0) for row in got)   # the duplicated points: d = 0 between two tiles


_CHILD = r"""
import sys, json, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import torch  # noqa: F401  (as the test session: torch's HIP runtime first)
import cwipc_util_amd as cw
from conftest import make_cloud
cw.cwipc_hip_set_device(0)
frame = np.load(sys.argv[2])["frame"]
pc = make_cloud(cw, frame)
jobs = [cw.NNJob(source_mask=s, reference_mask=r, nth=n) for s, r, n in json.loads(sys.argv[4])]
np.savez(sys.argv[3], **{"row%d" % i: row for i, row in enumerate(cw.cwipc_hip_nn_distance_jobs(pc, pc, jobs))})
"""


# the library's three grid flows (small clouds, the dense layout, the sparse one), forced where the size alone would not take them
@pytest.mark.parametrize("npoints,env", [(72000, {"CWIPC_SOR_SMALL_CELLS": "0"}), (72000, {"CWIPC_SOR_SPARSE": "1"}), (600000, {})])
def test_each_grid_flow(gpu, frames, npoints, env, tmp_path):
    import json
    frame = frames(npoints)
    tuples = camera_jobs()
    inp, out = str(tmp_path / "in.npz"), str(tmp_path / "rows.npz")
    np.savez(inp, frame=frame)
    subprocess.run([sys.executable, "-c", _CHILD, ROOT, inp, out, json.dumps([[s, r, n] for s, r, n, _b, _sy, _ry in tuples])], check=True, timeout=600,
                   env=dict(os.environ, **env))
    got = np.load(out)
    for k, (count, q, want) in enumerate(oracle_rows(frame, frame, tuples, sample_seed=3)):
        assert got["row%d" % k].shape == (count,)
        assert np.array_equal(got["row%d" % k][q], want), (npoints, env, k, tuples[k])


def test_camera_against_itself(gpu, frames):
    """toSelf: source is reference, the same mask on both sides, nth = 1 -- the point itself is the nearest, at 0."""
    frame = frames(6000)
    tuples = [job_tuple(t, t, 1) for t in (1, 2, 4, 8)] + [job_tuple(2, 2, 0)]
    got = check(gpu, frame, frame, tuples, same=True)
    assert np.all(got[4] == 0.0)
    pc = make_cloud(gpu, frame)
    for k, t in enumerate((1, 2, 4, 8)):
        tile = gpu.cwipc_tilefilter_masked(pc, t)
        assert np.array_equal(got[k], gpu.cwipc_hip_nn_distance(tile, tile, 1))


@pytest.mark.parametrize("count", [127, 128, 129, 257])
def test_source_counts_around_a_workgroup(gpu, frames, count):
    frame = frames(6000)
    check(gpu, frame[:count], frame, [job_tuple(1, 0xfe, 0), job_tuple(0, 0, 3), job_tuple(6, 9, 1)])


def test_a_whole_workgroup_sits_out(gpu, frames):
    """Source points in tile order: runs of far more than 128 consecutive points take no part in a job."""
    frame = frames(6000)
    ordered = frame[np.argsort(frame["tile"], kind="stable")]
    first = int(np.sum(ordered["tile"] == 1))
    assert first > 3 * 128
    tuples = [job_tuple(2, 0xfd, 0), job_tuple(8, 1, 1), job_tuple(1, 8, 3)]
    check(gpu, ordered, frame, tuples)
    src, ref = make_cloud(gpu, ordered), make_cloud(gpu, frame)
    rc, rows = raw_rows(gpu, src, ref, tuples)
    assert rc == 0
    assert np.all(np.isnan(rows[0, :first])) and not np.any(np.isnan(rows[0, first:first + int(np.sum(ordered["tile"] == 2))]))
    assert np.array_equal(np.isnan(rows[1]), ordered["tile"] != 8)


def test_jobs_that_are_not_searched(gpu, frames):
    frame = frames(6000)
    pc = make_cloud(gpu, frame)
    tuples = [job_tuple(1, 0x40, 0), job_tuple(0x40, 1, 0), job_tuple(1, 2, 0), job_tuple(0x40, 0x20, 31), job_tuple(3, 0x80, 3, 0.01)]
    rc, rows = raw_rows(gpu, pc, pc, tuples)
    assert rc == 0
    one = frame["tile"] == 1
    # no reference point takes part: +inf for the source points that do, NaN for the others
    assert np.all(np.isposinf(rows[0][one])) and np.all(np.isnan(rows[0][~one]))
    three = (frame["tile"] & 3) != 0
    assert np.all(np.isposinf(rows[4][three])) and np.all(np.isnan(rows[4][~three]))
    # no source point takes part: NaN everywhere
    assert np.all(np.isnan(rows[1])) and np.all(np.isnan(rows[3]))
    # ... and the job between them is searched as ever
    assert np.array_equal(np.sqrt(rows[2][one]), existing_path(gpu, pc, pc, tuples[2]))
    got = gpu.cwipc_hip_nn_distance_jobs(pc, pc, to_jobs(gpu, tuples))
    assert [len(g) for g in got] == [int(one.sum()), 0, int(one.sum()), 0, int(three.sum())]
    # an empty reference cloud, an empty source cloud
    empty = make_cloud(gpu, frame[:0])
    got = gpu.cwipc_hip_nn_distance_jobs(pc, empty, to_jobs(gpu, tuples[:1]))
    assert got[0].shape == (int(one.sum()),) and np.all(np.isposinf(got[0]))
    assert gpu.cwipc_hip_nn_distance_jobs(empty, pc, to_jobs(gpu, tuples[:1]))[0].shape == (0,)


def test_one_job_and_sixty_four(gpu, frames):
    frame = frames(6000)
    check(gpu, frame, frame, [job_tuple(4, 0xfb, 1)], same=True)
    nths = (0, 1, 3, 31, 2, 5)
    tuples = [job_tuple(1 + (k % 15), 1 + ((k * 7) % 15), nths[k % len(nths)], INF if k % 3 else 0.02) for k in range(64)]
    check(gpu, frame, frame, tuples, same=True, sample_seed=5)


def test_finite_max_distance(gpu, frames):
    frame = frames(6000)
    got = check(gpu, frame, frame, [job_tuple(1, 0xfe, 0, 0.004), job_tuple(0xfe, 1, 1, 0.004), job_tuple(2, 2, 3, 0.01), job_tuple(8, 7, 31, 0.05)], same=True)
    assert all(np.any(np.isinf(g)) and np.any(np.isfinite(g)) for g in got)


def test_y_limits(gpu, frames):
    frame = frames(6000)
    not_floor, floor_only = (FLOOR32, INF), (-INF, FLOOR32)
    tuples = [job_tuple(1, 0xfe, 0, INF, not_floor, not_floor), job_tuple(0xfe, 1, 1, INF, not_floor, not_floor),   # ignore_floor on both clouds
              job_tuple(2, 0, 0, INF, floor_only, ALL_Y), job_tuple(4, 0xfb, 3, 0.05, floor_only, ALL_Y),            # floor-only on the source only
              job_tuple(0, 0, 1, INF, not_floor, not_floor), job_tuple(8, 8, 31, INF, floor_only, floor_only)]
    check(gpu, frame, frame, tuples, same=True)
    # points with y exactly at float32(0.1) and at its two float32 neighbours, in both clouds, on both sides of both predicates
    edge = np.float32(0.1)
    ys = np.array([np.nextafter(edge, np.float32(-1)), edge, np.nextafter(edge, np.float32(1))], dtype=np.float32)
    assert FLOOR32 == float(gpu.NNJob.ignore_floor()[0]) == float(gpu.NNJob.floor_only()[1])
    rng = np.random.default_rng(2)
    pts = frame[:900].copy()
    pts["y"] = ys[np.arange(900) % 3]
    pts["x"] = rng.normal(0, 0.05, 900).astype(np.float32)
    pts["z"] = rng.normal(0, 0.05, 900).astype(np.float32)
    got = check(gpu, pts, pts, [job_tuple(0, 0, 0, INF, not_floor, not_floor), job_tuple(0, 0, 0, INF, floor_only, ALL_Y),
                                job_tuple(0, 0, 1, INF, ALL_Y, floor_only), job_tuple(3, 12, 0, INF, not_floor, floor_only)], same=True)
    assert [len(g) for g in got[:3]] == [300, 300, 900]
    src = make_cloud(gpu, pts)
    rc, rows = raw_rows(gpu, src, src, [job_tuple(0, 0, 0, INF, not_floor, ALL_Y), job_tuple(0, 0, 0, INF, floor_only, ALL_Y)])
    assert rc == 0
    assert np.array_equal(~np.isnan(rows[0]), pts["y"] > edge) and np.array_equal(~np.isnan(rows[1]), pts["y"] < edge)


def test_two_calls_and_four_threads_give_the_same_bytes(gpu, frames):
    frame = frames(72000)
    pc = make_cloud(gpu, frame)
    tuples = camera_jobs()
    alone = [row.tobytes() for row in gpu.cwipc_hip_nn_distance_jobs(pc, pc, to_jobs(gpu, tuples))]
    assert alone == [row.tobytes() for row in gpu.cwipc_hip_nn_distance_jobs(pc, pc, to_jobs(gpu, tuples))]
    got, errors = [None] * 4, []

    def work(i):
        try:
            gpu.cwipc_hip_set_device(0)
            for _ in range(2):
                got[i] = [row.tobytes() for row in gpu.cwipc_hip_nn_distance_jobs(pc, pc, to_jobs(gpu, tuples))]
        except Exception as e:   # pragma: no cover - reported below
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert all(g == alone for g in got)


def test_error_paths(gpu, frames):
    frame = frames(6000)
    pc = make_cloud(gpu, frame)
    dll = gpu.cwipc_util_dll_load()
    n = pc.count()
    good = job_tuple(1, 2, 0)
    assert raw_rows(gpu, pc, pc, [good])[0] == 0
    assert raw_rows(gpu, pc, pc, [good], cap=n + 5)[0] == 0          # a wider row is fine
    table = (gpu.NNJob * 65)(*to_jobs(gpu, [good] * 65))
    buf = np.zeros((65, n))
    assert dll.cwipc_hip_nn_distance2_jobs(None, pc.as_cwipc_p(), ctypes.addressof(table), 1, buf.ctypes.data, n) == -1
    assert dll.cwipc_hip_nn_distance2_jobs(pc.as_cwipc_p(), None, ctypes.addressof(table), 1, buf.ctypes.data, n) == -1
    assert dll.cwipc_hip_nn_distance2_jobs(pc.as_cwipc_p(), pc.as_cwipc_p(), ctypes.addressof(table), 0, buf.ctypes.data, n) == -1
    assert dll.cwipc_hip_nn_distance2_jobs(pc.as_cwipc_p(), pc.as_cwipc_p(), ctypes.addressof(table), 65, buf.ctypes.data, n) == -1
    assert dll.cwipc_hip_nn_distance2_jobs(pc.as_cwipc_p(), pc.as_cwipc_p(), ctypes.addressof(table), 64, buf.ctypes.data, n) == 0
    assert raw_rows(gpu, pc, pc, [good], cap=n - 1)[0] == -1
    nan = float("nan")
    bad = [job_tuple(1, 2, -1), job_tuple(1, 2, 32), job_tuple(1, 2, 0, 0.0), job_tuple(1, 2, 0, -1.0), job_tuple(1, 2, 0, nan),
           job_tuple(1, 2, 0, INF, (nan, INF)), job_tuple(1, 2, 0, INF, (-INF, nan)), job_tuple(1, 2, 0, INF, ALL_Y, (nan, INF)),
           job_tuple(1, 2, 0, INF, ALL_Y, (-INF, nan))]
    for b in bad:
        assert raw_rows(gpu, pc, pc, [good, b])[0] == -1, b
        with pytest.raises(gpu.CwipcError):
            gpu.cwipc_hip_nn_distance_jobs(pc, pc, to_jobs(gpu, [b]))
    with pytest.raises(gpu.CwipcError):
        gpu.cwipc_hip_nn_distance_jobs(pc, pc, [])
    with pytest.raises(gpu.CwipcError):
        gpu.cwipc_hip_nn_distance_jobs(None, pc, to_jobs(gpu, [good]))
