"""registration/multicamera.py on the GPU: a frame of three cameras (about 20 000 points each, overlapping sectors of the synthetic
cloud, a floor band), cameras 2 and 3 moved by a few millimetres and a few tenths of a degree.

  * batched analysis == per-analyzer analysis, for every algorithm class: transformations, result cloud and every field of every
    AnalysisResults, byte for byte;
  * the orchestration of MultiCameraOneToAllOthers and MultiCameraToGroundTruth == the loop spelled out here from public calls;
  * structure: points and per-tile counts conserved, every camera accepted or merged, the kept camera's matrix the identity, the
    floor cloud flat;
  * the alignment helps: each moved camera ends up closer to where the kept camera says it belongs than it started.
"""
import numpy as np
import pytest

from conftest import make_cloud
from multicam_frames import make_frame, rigid, xyz_of

pytestmark = pytest.mark.gpu

FLOOR_SEED = 20240607
TILES = (1, 2, 4)
#: camera 2: 4 mm and 0.3 degrees; camera 3: 3 mm and 0.2 degrees (about a point near the scene's middle)
MOTIONS = {2: dict(rx_deg=0.1, ry_deg=0.3, rz_deg=-0.1, t=(0.003, 0.001, -0.0025)), 4: dict(rx_deg=-0.1, ry_deg=-0.2, rz_deg=0.05, t=(-0.002, 0.0015, 0.002))}


def moved_by(pts, m):
    out = pts.copy()
    p = xyz_of(pts).astype(np.float64) @ m[:3, :3].T + m[:3, 3]
    out["x"], out["y"], out["z"] = p[:, 0].astype(np.float32), p[:, 1].astype(np.float32), p[:, 2].astype(np.float32)
    return out


@pytest.fixture(scope="module")
def scene(synth):
    """(the frame as it should be, the frame with cameras 2 and 3 moved, the motions as matrices, a ground truth: another sampling
    of the same scene -- against the frame's own points every distance of the unmoved camera would be 0)"""
    pts, _ = synth(54000)
    truth = make_frame(pts, 3, seed=5, duplicates=0)
    groundtruth = make_frame(synth(66000)[0], 3, seed=6, duplicates=0)
    pivot = (float(np.mean(truth["x"])), float(np.mean(truth["y"])), float(np.mean(truth["z"])))
    motions = {t: rigid(pivot=pivot, **kw) for t, kw in MOTIONS.items()}
    frame = truth.copy()
    for t, m in motions.items():
        sel = frame["tile"] == t
        frame[sel] = moved_by(frame[sel], m)
    assert all(15000 < np.sum(frame["tile"] == t) < 26000 for t in TILES) and np.sum(frame["y"] < 0.1) > 3000
    return truth, frame, motions, groundtruth


def configured(gpu, cls, scene, batch):
    from cwipc_util_amd import registration as reg
    _, frame, _, groundtruth = scene
    alg = cls()
    alg.batch_analysis = batch
    alg.floor_seed = FLOOR_SEED
    alg.set_analyzer_class(reg.RegistrationAnalyzerSymmetric)
    alg.set_tiled_pointcloud(make_cloud(gpu, frame))
    if cls is reg.MultiCameraToGroundTruth:
        alg.set_groundtruth(make_cloud(gpu, groundtruth))
    return alg


_runs = {}


def run_of(gpu, cls, scene, batch):
    key = (cls.__name__, batch)
    if key not in _runs:
        alg = configured(gpu, cls, scene, batch)
        assert alg.run() is True
        _runs[key] = alg
    return _runs[key]


def same_results(a, b):
    assert len(a) == len(b) and len(a) > 0
    for ra, rb in zip(a, b):
        assert vars(ra).keys() == vars(rb).keys()
        for name, va in vars(ra).items():
            vb = getattr(rb, name)
            if isinstance(va, np.ndarray):
                assert isinstance(vb, np.ndarray) and va.dtype == vb.dtype and va.tobytes() == vb.tobytes(), name
            elif isinstance(va, (float, np.floating)):
                assert np.float64(va).tobytes() == np.float64(vb).tobytes(), name
            else:
                assert type(va) == type(vb) and va == vb, name


def algorithm_classes():
    from cwipc_util_amd import registration as reg
    return reg.ALL_MULTICAMERA_ALGORITHMS


@pytest.mark.parametrize("index", range(4))
def test_batched_analysis_equals_per_analyzer_analysis(gpu, scene, index):
    cls = algorithm_classes()[index]
    one, two = run_of(gpu, cls, scene, True), run_of(gpu, cls, scene, False)
    assert np.array(one.get_result_transformations()).tobytes() == np.array(two.get_result_transformations()).tobytes()
    assert one.get_result_pointcloud_full().get_numpy_array().tobytes() == two.get_result_pointcloud_full().get_numpy_array().tobytes()
    same_results(one.pre_analysis_results, two.pre_analysis_results)
    same_results(one.results, two.results)
    assert one.proposed_cellsize == two.proposed_cellsize and one.tile_occupancy == two.tile_occupancy
    for r in one.pre_analysis_results + one.results:
        assert r.histogram is not None and len(r.histogram) > 1 and r.sourcePointCount > 0 and r.minCorrespondence > 0


def test_orchestration_is_the_spelled_out_sequence(gpu, scene):
    from cwipc_util_amd import registration as reg
    _, frame, _, groundtruth = scene
    # one to all others: analyzer per camera, cameras by ascending correspondence, aligner per camera on the cloud as it stands
    pc = make_cloud(gpu, frame)
    found = []
    for t in TILES:
        an = reg.RegistrationAnalyzerSymmetric()
        an.set_source_pointcloud(pc, t)
        an.set_reference_pointcloud(pc, 0xff ^ t)
        an.set_correspondence_measure('2mode')
        assert an.run()
        found.append((an.get_results().minCorrespondence, t))
    want = {t: np.identity(4) for t in TILES}
    for corr, t in sorted(found, key=lambda ct: ct[0]):
        icp = reg.RegistrationComputer_ICP_Generalized()
        icp.set_source_pointcloud(pc, t)
        icp.set_reference_pointcloud(pc, 0xff ^ t)
        icp.set_correspondence(corr)
        assert icp.run()
        pc = icp.get_result_pointcloud_full()
        want[t] = np.matmul(icp.get_result_transformation(), want[t])
    got = run_of(gpu, reg.MultiCameraOneToAllOthers, scene, True)
    assert np.array(got.get_result_transformations()).tobytes() == np.array([want[t] for t in TILES]).tobytes()
    assert got.get_result_pointcloud_full().get_numpy_array().tobytes() == pc.get_numpy_array().tobytes()
    # to the ground truth: analyzer per camera (floor ignored, median), aligner per camera against the truth, camera order
    pc, gt = make_cloud(gpu, frame), make_cloud(gpu, groundtruth)
    want = []
    for t in TILES:
        an = reg.RegistrationAnalyzer()
        an.set_source_pointcloud(pc, t)
        an.set_reference_pointcloud(gt)
        an.set_correspondence_measure('median')
        an.set_ignore_floor(True)
        assert an.run()
        icp = reg.RegistrationComputer_ICP_Generalized()
        icp.set_source_pointcloud(pc, t)
        icp.set_reference_pointcloud(gt)
        icp.set_correspondence(an.get_results().minCorrespondence)
        assert icp.run()
        want.append(np.matmul(icp.get_result_transformation(), np.identity(4)))
    got = run_of(gpu, reg.MultiCameraToGroundTruth, scene, True)
    assert np.array(got.get_result_transformations()).tobytes() == np.array(want).tobytes()


def test_structure(gpu, scene):
    from cwipc_util_amd import registration as reg
    _, frame, _, _ = scene
    counts = {t: int(np.sum(frame["tile"] == t)) for t in TILES}
    for cls in algorithm_classes():
        alg = run_of(gpu, cls, scene, True)
        out = alg.get_result_pointcloud_full().get_numpy_array()
        assert len(out) == len(frame), cls.__name__
        # (the iterative class shuffles the FLOOR's tile numbers among the floor points: the counts stay, per tile too)
        assert {t: int(np.sum(out["tile"] == t)) for t in TILES} == counts, cls.__name__
        assert len(alg.get_result_transformations()) == 3 and len(alg.results) == 3 and len(alg.pre_analysis_results) == 3
        assert len(alg.change) == 3
    it = run_of(gpu, reg.MultiCameraIterative, scene, True)
    assert sorted(it.accepted_tiles + it.merged_tiles) == list(TILES)   # every camera was accepted, or merged unaligned at the end
    first = it.camera_index_for_tilemask(it.accepted_tiles[0])
    assert np.array_equal(it.get_result_transformations()[first], np.identity(4))
    fl = run_of(gpu, reg.MultiCameraToFloor, scene, True)
    flat = fl.floor_pointcloud.get_numpy_array()
    assert flat["y"].tobytes() == bytes(4 * len(frame))
    for name in ("x", "z", "r", "g", "b", "tile"):
        assert flat[name].tobytes() == frame[name].tobytes(), name
    assert fl.floor_pointcloud.timestamp() == 0 and fl.floor_pointcloud.cellsize() == 0


def test_the_alignment_helps(gpu, scene):
    """Per moved camera the largest distance of its points from where they belong, before and after MultiCameraIterative.  Where a
    point belongs is said by the camera the algorithm keeps unmoved (its matrix stays the identity): its unmoved position carried
    along with that camera's own motion -- the unmoved position itself when the kept camera is the unmoved one."""
    from cwipc_util_amd import registration as reg
    truth, frame, motions, _ = scene
    it = run_of(gpu, reg.MultiCameraIterative, scene, True)
    kept = it.accepted_tiles[0]
    anchor = motions.get(kept, np.identity(4))
    trafos = it.get_result_transformations()
    report = {}
    for t in TILES:
        if t == kept:
            continue
        sel = frame["tile"] == t
        unmoved = xyz_of(truth[sel]).astype(np.float64)
        belongs = unmoved @ anchor[:3, :3].T + anchor[:3, 3]
        start = xyz_of(frame[sel]).astype(np.float64)
        m = trafos[it.camera_index_for_tilemask(t)]
        end = start @ m[:3, :3].T + m[:3, 3]
        before = float(np.max(np.linalg.norm(start - belongs, axis=1)))
        after = float(np.max(np.linalg.norm(end - belongs, axis=1)))
        report[t] = (before, after)
    print("kept tile", kept, "accepted", it.accepted_tiles, "merged", it.merged_tiles, "largest displacement before/after per tile:", report)
    for t, (before, after) in report.items():
        if t in motions or kept in motions:
            assert after < before, (t, before, after)


def test_transform44_filter(gpu, scene):
    from cwipc_util_amd.filters import factory
    _, frame, motions, _ = scene
    pc = make_cloud(gpu, frame)
    m = motions[2]
    flt = factory("transform44(%r)" % (m.tolist(),))
    out = flt.filter(pc)
    want = gpu.cwipc_transform(pc, m)
    assert out.get_numpy_array().tobytes() == want.get_numpy_array().tobytes()
    assert out.timestamp() == want.timestamp() and out.cellsize() == want.cellsize()
