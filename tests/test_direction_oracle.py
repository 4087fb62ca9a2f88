"""Known answers of the direction filter's numpy oracle (tests/direction_oracle.py), and the filter's place in the factory.
CPU only."""
import numpy as np
import pytest

import direction_oracle as do


def test_jittered_plane_gives_its_normal_away_from_the_centroid():
    rng = np.random.default_rng(1)
    g = np.stack(np.meshgrid(np.arange(40), np.arange(40)), -1).reshape(-1, 2) * 0.005
    plane = np.column_stack([g[:, 0], g[:, 1], np.zeros(len(g))]) + rng.normal(0, 1e-4, (len(g), 3))
    # a far blob below the plane puts the centroid under it: every normal of the plane then points to +z
    blob = rng.normal(0, 0.01, (200, 3)) + np.array([0.1, 0.1, -1.0])
    xyz = np.vstack([plane, blob]).astype(np.float32)
    est = do.estimate(xyz, query=np.arange(len(plane)))
    assert np.all(est["nn"] >= 3)
    assert np.all(est["normals"][:, 2] > 0.99)


def test_sphere_shell_gives_outward_radial_normals():
    rng = np.random.default_rng(2)
    v = rng.normal(size=(40000, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    xyz = (v * 0.3).astype(np.float32)   # about 45 points within 0.02 of each: max_nn bounds every neighbourhood
    est = do.estimate(xyz)
    radial = xyz.astype(np.float64) - est["centroid"]
    radial /= np.linalg.norm(radial, axis=1, keepdims=True)
    ok = est["nn"] == 30
    assert ok.mean() > 0.99
    cosines = (est["normals"][ok] * radial[ok]).sum(axis=1)
    assert np.all(cosines > 0.95)


def test_isolated_and_coincident_points_take_the_z_rule_then_the_orientation():
    xyz = np.array([[0, 0, 0], [1, 0, 0], [1, 0.005, 0],             # an isolated point, a pair: fewer than 3 neighbours
                    [0, 2, 1], [0, 2, 1], [0, 2, 1], [0, 2, 1]],     # four coincident points: a zero covariance
                   dtype=np.float32)
    est = do.estimate(xyz)
    assert list(est["nn"]) == [1, 2, 2, 4, 4, 4, 4]
    cen = est["centroid"]
    for i, p in enumerate(xyz.astype(np.float64)):
        raw = np.array([0.0, 0.0, 1.0])
        if raw @ (cen - p) < 0:
            raw = -raw
        assert np.array_equal(est["normals"][i], -raw)
    # the centroid lies at z = 4/7: points at z = 0 get (0, 0, -1), the stack at z = 1 gets (0, 0, 1)
    assert est["normals"][0, 2] == -1.0 and est["normals"][3, 2] == 1.0


def test_max_nn_and_radius_bound_the_neighbourhood():
    rng = np.random.default_rng(3)
    dense = rng.uniform(-0.01, 0.01, (200, 3))                    # 200 points within 0.0174 of the origin
    xyz = np.vstack([[0, 0, 0], dense, [[1, 1, 1], [1.015, 1, 1], [1, 1.03, 1]]]).astype(np.float32)
    pts = xyz.astype(np.float64)
    est = do.estimate(xyz, radius=0.02, max_nn=30, query=[0, 201])
    d = np.linalg.norm(pts - pts[0], axis=1)
    assert est["nn"][0] == 30
    assert list(est["neighbours"][0]) == list(np.lexsort((np.arange(len(d)), d))[:30])
    # the point at (1, 1, 1): itself and the one 0.015 away, not the one 0.03 away
    assert est["nn"][1] == 2 and sorted(est["neighbours"][1]) == [201, 202]


def test_direction_mask_and_zero_direction():
    est = {"normals": np.array([[0, 0, 1.0], [0, 0, -1.0], [1.0, 0, 0]])}
    keep, margin = do.direction_mask(est, (0, 0, 2), 0.5)
    assert list(keep) == [True, False, False] and np.allclose(margin, [0.5, 1.5, 0.5])
    keep, _ = do.direction_mask(est, (0, 0, 0), 0.0)
    assert keep.all()
    keep, _ = do.direction_mask(est, (0, 0, 0), 0.1)
    assert not keep.any()


def test_neighbour_sets_match_a_kd_tree():
    spatial = pytest.importorskip("scipy.spatial")
    rng = np.random.default_rng(4)
    xyz = rng.uniform(0, 0.2, (20000, 3)).astype(np.float32)
    pts = xyz.astype(np.float64)
    query = rng.choice(len(xyz), 2000, replace=False)
    est = do.estimate(xyz, radius=0.02, max_nn=30, query=query)
    dist, idx = spatial.cKDTree(pts).query(pts[query], k=30, distance_upper_bound=0.02)
    checked = 0
    for j in range(len(query)):
        if est["tie"][j] or est["boundary"][j]:
            continue
        want = set(idx[j][np.isfinite(dist[j])].tolist())
        assert set(est["neighbours"][j].tolist()) == want
        assert est["nn"][j] == len(want)
        checked += 1
    assert checked > 0.95 * len(query)


def test_factory_knows_the_direction_filter():
    from cwipc_util_amd.filters import factory, all_filters
    from cwipc_util_amd.filters.direction import DirectionFilter
    f = factory("direction(0, 0, 1, 0.5)")
    assert isinstance(f, DirectionFilter)
    assert f.filtername == "direction"
    assert f.direction == (0, 0, 1) and f.threshold == 0.5
    assert factory("direction(1, 0, 0)").threshold == 0.0
    assert any(m.CustomFilter is DirectionFilter for m in all_filters)
