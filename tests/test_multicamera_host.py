"""The host side of the multi-camera layer, no GPU: the transformation helpers, the step-acceptance table, the job lists a batched
analysis builds, and the NaN compaction of cwipc_hip_nn_distance_jobs."""
import math

import numpy as np
import pytest

from multicam_frames import rigid

INF = float("inf")
F01 = float(np.float32(0.1))


@pytest.fixture(scope="module")
def reg():
    from cwipc_util_amd import registration
    return registration


class FakeCloud:
    """Stands where a cloud is only held, counted and compared by identity."""

    def __init__(self, n=10):
        self.n = n

    def count(self):
        return self.n


# ---- transformations ----
def test_transformation_invert_and_compare(reg):
    from cwipc_util_amd.registration import util as ru
    assert np.array_equal(ru.transformation_identity(), np.identity(4)) and ru.transformation_identity().dtype == np.float64
    quarter = np.array([[0.0, -1, 0, 1], [1, 0, 0, 2], [0, 0, 1, 3], [0, 0, 0, 1]])      # 90 degrees about z, then (1, 2, 3)
    inv = ru.transformation_invert(quarter)
    assert np.array_equal(inv, np.array([[0.0, 1, 0, -2], [-1, 0, 0, 1], [0, 0, 1, -3], [0, 0, 0, 1]]))
    assert np.array_equal(inv @ quarter, np.identity(4))
    m = rigid(0.3, -0.2, 0.4, (0.004, -0.002, 0.003), pivot=(0.1, 1.0, -0.2))
    assert np.allclose(ru.transformation_invert(m) @ m, np.identity(4), atol=1e-15)
    t, r = ru.transformation_compare(None, quarter)
    assert np.array_equal(t, [1, 2, 3]) and np.allclose(r, [0, 0, 90], atol=1e-12)
    t, r = ru.transformation_compare(quarter, quarter)
    assert np.allclose(t, 0, atol=1e-15) and np.allclose(r, 0, atol=1e-12)
    t, r = ru.transformation_compare(quarter, None)
    assert np.allclose(t, [-2, 1, -3], atol=1e-15) and np.allclose(r, [0, 0, -90], atol=1e-12)
    about_x = rigid(rx_deg=0.25, t=(0.001, 0, 0))
    t, r = ru.transformation_compare(None, about_x)
    assert np.allclose(t, [0.001, 0, 0], atol=1e-15) and np.allclose(r, [0.25, 0, 0], atol=1e-10)
    half = rigid(ry_deg=180.0)
    assert np.allclose(np.abs(ru.transformation_compare(None, half)[1]), [0, 180, 0], atol=1e-9)
    # old -> new composed on the left: new = diff @ old
    t, r = ru.transformation_compare(quarter, about_x @ quarter)
    assert np.allclose(t, [0.001, 0, 0], atol=1e-12) and np.allclose(r, [0.25, 0, 0], atol=1e-10)
    assert ru.transformation_topython(ru.transformation_frompython(quarter.tolist())) == quarter.tolist()
    assert np.array_equal(ru.transformation_get_translation(quarter), [1, 2, 3])


# ---- the step-acceptance table (reference multicamera.py:573-596) ----
def test_accept_step_table(reg):
    from cwipc_util_amd.registration.multicamera import accept_step
    below = lambda v: math.nextafter(v, 0.0)   # noqa: E731
    assert accept_step(0.99, 0.99) == (True, "very good, accept")
    assert accept_step(below(0.99), 0.99)[0] is False and accept_step(0.99, below(0.99))[0] is False
    assert accept_step(0.8, 1.25) == (True, "good overall, accept") and accept_step(1.25, 0.8) == (True, "good overall, accept")
    assert accept_step(below(0.8), 1.3)[0] is False and accept_step(0.8, below(1.25))[0] is False and accept_step(1.3, below(0.8))[0] is False
    assert accept_step(2.0, 1.0)[0] is True and accept_step(4.0, 0.5) == (True, "great (but at cost of count), accept")
    assert accept_step(4.0, below(0.5))[1] == "borderline, accept" and accept_step(below(2.0), 0.76)[1] == "borderline, accept"
    assert accept_step(1.5, 1.0)[0] is True and accept_step(3.0, 0.5) == (True, "borderline, accept")
    assert accept_step(below(1.5), 0.7) == (False, "bad, reject") and accept_step(1.9, 0.78) == (False, "bad, reject")
    assert accept_step(3.0, below(0.5)) == (False, "bad, reject")

    # ... through the method, from two analysis results
    alg = reg.MultiCameraIterative()

    def rr(corr, count):
        r = reg.AnalysisResults()
        r.minCorrespondence, r.minCorrespondenceCount = corr, count
        return r
    alg.current_step_results = [rr(0.010, 1000), rr(0.005, 1000)]
    assert alg._accept_step(1, None) == (True, False)
    alg.current_step_results = [rr(0.010, 1000), rr(0.011, 1000)]
    assert alg._accept_step(1, None) == (False, False)
    alg.current_step_results = [rr(0.010, 1000), rr(0.008, 800)]
    assert alg._accept_step(1, None) == (True, False)
    assert alg.orientation_filter == -0.3 and alg.randomize_floor is True and alg.candidate_measure == "2mode" and alg.floor_seed is None
    assert alg.proposed_cellsize_factor == math.sqrt(2) and alg.batch_analysis is False   # (off: it measured slower)
    assert reg.DEFAULT_MULTICAMERA_ALGORITHM is reg.MultiCameraIterative
    assert reg.ALL_MULTICAMERA_ALGORITHMS == [reg.MultiCameraOneToAllOthers, reg.MultiCameraToFloor, reg.MultiCameraIterative, reg.MultiCameraToGroundTruth]
    assert reg.MultiCameraToFloor().aligner_class is reg.RegistrationComputer_ICP_Generalized
    assert reg.MultiCameraOneToAllOthers().randomize_floor is False


# ---- the job lists of a batched analysis ----
def job_fields(j):
    return (j.source_mask, j.reference_mask, j.nth, j.max_distance, tuple(j.source_y), tuple(j.reference_y))


def analyzers_for(reg, kind, frame, other=None, symmetric=False, ignore_floor=False, floor_only=False):
    out = []
    for t in (1, 2, 4):
        a = (reg.RegistrationAnalyzerSymmetric if symmetric else reg.RegistrationAnalyzer)()
        a.set_source_pointcloud(frame, t)
        if kind == "toSelf":
            a.set_reference_pointcloud(frame, t)
            a.set_ignore_nearest(1)
        elif kind == "toOthers":
            a.set_reference_pointcloud(frame, 0xff ^ t)
        else:
            a.set_reference_pointcloud(other)
        if ignore_floor:
            a.set_ignore_floor(True)
        if floor_only:
            a.set_source_floor_only(0.1)
        out.append(a)
    return out


def test_job_lists(reg):
    frame, truth = FakeCloud(), FakeCloud()
    everything, not_floor, floor = (-INF, INF), (F01, INF), (-INF, F01)

    fwd, back, owners = reg.build_analyzer_jobs(analyzers_for(reg, "toSelf", frame))
    assert [job_fields(j) for j in fwd] == [(t, t, 1, INF, everything, everything) for t in (1, 2, 4)] and back == [] and owners == []
    fwd, back, owners = reg.build_analyzer_jobs(analyzers_for(reg, "toSelf", frame, ignore_floor=True))
    assert [job_fields(j) for j in fwd] == [(t, t, 1, INF, not_floor, not_floor) for t in (1, 2, 4)] and back == []

    # the symmetric analyzer: forward jobs on (source, reference), then backward jobs on (reference, source), sides swapped
    fwd, back, owners = reg.build_analyzer_jobs(analyzers_for(reg, "toOthers", frame, symmetric=True))
    assert [job_fields(j) for j in fwd] == [(t, 0xff ^ t, 0, INF, everything, everything) for t in (1, 2, 4)]
    assert [job_fields(j) for j in back] == [(0xff ^ t, t, 0, INF, everything, everything) for t in (1, 2, 4)] and owners == [0, 1, 2]
    fwd, back, owners = reg.build_analyzer_jobs(analyzers_for(reg, "toOthers", frame, symmetric=True, ignore_floor=True))
    assert [job_fields(j) for j in fwd] == [(t, 0xff ^ t, 0, INF, not_floor, not_floor) for t in (1, 2, 4)]
    assert [job_fields(j) for j in back] == [(0xff ^ t, t, 0, INF, not_floor, not_floor) for t in (1, 2, 4)]

    # against a reference cloud: no mask on it (0: every point); floor-only limits the SOURCE side, which is the reference side on the way back
    fwd, back, owners = reg.build_analyzer_jobs(analyzers_for(reg, "toReference", frame, truth))
    assert [job_fields(j) for j in fwd] == [(t, 0, 0, INF, everything, everything) for t in (1, 2, 4)] and back == []
    fwd, back, owners = reg.build_analyzer_jobs(analyzers_for(reg, "toReference", frame, truth, ignore_floor=True))
    assert [job_fields(j) for j in fwd] == [(t, 0, 0, INF, not_floor, not_floor) for t in (1, 2, 4)]
    fwd, back, owners = reg.build_analyzer_jobs(analyzers_for(reg, "toReference", frame, truth, symmetric=True, floor_only=True))
    assert [job_fields(j) for j in fwd] == [(t, 0, 0, INF, floor, everything) for t in (1, 2, 4)]
    assert [job_fields(j) for j in back] == [(0, t, 0, INF, everything, floor) for t in (1, 2, 4)] and owners == [0, 1, 2]
    fwd, _back, _owners = reg.build_analyzer_jobs(analyzers_for(reg, "toReference", frame, truth, ignore_floor=True, floor_only=True))
    assert job_fields(fwd[0]) == (1, 0, 0, INF, (F01, F01), not_floor)

    # a mixed list: only the symmetric analyzers go backward
    mixed = analyzers_for(reg, "toOthers", frame) + analyzers_for(reg, "toOthers", frame, symmetric=True)
    mixed[1].set_max_correspondence_distance(0.05)
    fwd, back, owners = reg.build_analyzer_jobs(mixed)
    assert len(fwd) == 6 and owners == [3, 4, 5] and fwd[1].max_distance == 0.05 and len(back) == 3

    # what does not qualify
    assert reg.build_analyzer_jobs([]) is None
    assert reg.build_analyzer_jobs(analyzers_for(reg, "toOthers", frame) + analyzers_for(reg, "toOthers", FakeCloud())) is None
    assert reg.build_analyzer_jobs(analyzers_for(reg, "toReference", frame, truth) + analyzers_for(reg, "toReference", frame, FakeCloud())) is None
    filtered = analyzers_for(reg, "toReference", frame, truth)
    filtered[2].apply_reference_filter(lambda pc: pc)
    assert reg.build_analyzer_jobs(filtered) is None
    wide = analyzers_for(reg, "toOthers", frame)
    wide[0].set_source_pointcloud(frame, 0x100)
    assert reg.build_analyzer_jobs(wide) is None
    deep = analyzers_for(reg, "toSelf", frame)
    deep[0].set_ignore_nearest(32)
    assert reg.build_analyzer_jobs(deep) is None

    class Other(reg.RegistrationAnalyzer):
        pass
    assert reg.build_analyzer_jobs([Other()]) is None
    unset = reg.RegistrationAnalyzer()
    assert reg.build_analyzer_jobs([unset]) is None


def test_filters_stack_and_reset(reg):
    a, b, c = FakeCloud(1), FakeCloud(2), FakeCloud(3)
    an = reg.RegistrationAnalyzer()
    an.set_source_pointcloud(a)
    an.set_reference_pointcloud(b)
    assert an.get_source_pointcloud() is a and an.get_filtered_source_pointcloud() is a and an.get_filtered_reference_pointcloud() is b
    seen = []
    an.apply_source_filter(lambda pc: (seen.append(pc), c)[1])
    an.apply_source_filter(lambda pc: (seen.append(pc), pc)[1])
    assert seen == [a, c] and an.get_filtered_source_pointcloud() is c and an.get_source_pointcloud() is a
    an.set_source_pointcloud(b)
    assert an.get_filtered_source_pointcloud() is b


# ---- the NaN compaction ----
def test_compact_job_rows():
    from cwipc_util_amd import compact_job_rows
    nan = float("nan")
    rows = np.array([[4.0, nan, 0.25, INF, nan], [nan, nan, nan, nan, nan], [1.0, 9.0, 16.0, 0.0, 2.25]])
    got = compact_job_rows(rows)
    assert [g.tolist() for g in got] == [[2.0, 0.5, INF], [], [1.0, 3.0, 4.0, 0.0, 1.5]]
    assert all(g.dtype == np.float64 for g in got)
    assert compact_job_rows(np.zeros((0, 5))) == []
    assert [g.shape for g in compact_job_rows(np.zeros((2, 0)))] == [(0,), (0,)]


def test_nnjob_fields():
    import ctypes
    from cwipc_util_amd import NNJob
    assert ctypes.sizeof(NNJob) == 48 and NNJob.nth.offset == 4 and NNJob.max_distance.offset == 8 and NNJob.reference_y.offset == 32
    j = NNJob(source_mask=3, nth=2, source_y=(0.1, INF))
    assert (j.source_mask, j.reference_mask, j.nth, j.max_distance) == (3, 0, 2, INF)
    assert tuple(j.source_y) == (F01, INF) and tuple(j.reference_y) == (-INF, INF)    # a Python float limit is numpy's float32 comparison
    assert NNJob(source_y=(np.float64(0.1), INF)).source_y[0] == 0.1
    assert NNJob.ignore_floor() == (F01, INF) and NNJob.floor_only(0.1) == (-INF, F01)
