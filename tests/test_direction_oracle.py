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


# ---------------------------------------------------------------------------
# the exact-neighbourhood oracle (estimate_exact): the kernel's definition of N(p)
# ---------------------------------------------------------------------------
def angle(a, b):
    """The angle between the lines of a and b (up to sign), accurate for small angles."""
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=-1), np.abs((a * b).sum(axis=-1)))


def brute_neighbourhoods(xyz, radius, max_nn):
    """N(p) of every point over all pairs, straight from the definition: a list of sorted index arrays."""
    xyz = np.asarray(xyz, dtype=np.float32)
    r2 = do.r2_of(radius)
    out = []
    for i in range(len(xyz)):
        d2 = do.flann_d2(xyz[i], xyz)
        under = np.sort(d2[d2 < r2])
        cutoff = under[max_nn - 1] if len(under) >= max_nn else r2
        out.append(np.flatnonzero((d2 <= cutoff) & (d2 < r2)))
    return out


def small_clouds():
    rng = np.random.default_rng(11)
    g = np.arange(10, dtype=np.float64) * 0.125
    yield "box", rng.uniform(0, 0.2, (2000, 3)), 0.02
    yield "lattice at the radius", np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3), 0.125
    yield "lattice above the radius", np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3), float(np.nextafter(np.float32(0.125), np.float32(1)))
    yield "lattice, decimal spacing", np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) * 0.16, 0.02 * 2
    yield "dupes", rng.uniform(0, 1, (30, 3))[rng.integers(0, 30, 1500)], 0.3
    yield "shifted sheet", np.column_stack([rng.uniform(0, 1, (1500, 2)), np.full(1500, 0.25)]) + 100.0, 0.08
    yield "radius above the cloud", rng.uniform(-1, 1, (100, 3)), 10.0
    yield "radius of many cells", rng.uniform(0, 1, (2000, 3)), 0.5


@pytest.mark.parametrize("max_nn", [1, 3, 30, 128])
def test_exact_neighbourhoods_equal_brute_force_over_all_pairs(max_nn):
    """... so the bucket grid's candidates (27 cells a little wider than the radius) are a superset of N(p)."""
    for name, xyz, radius in small_clouds():
        xyz = xyz.astype(np.float32)
        est = do.estimate_exact(xyz, radius=radius, max_nn=max_nn)
        want = brute_neighbourhoods(xyz, radius, max_nn)
        assert list(est["nn"]) == [len(w) for w in want], name
        for j in range(len(xyz)):
            assert np.array_equal(np.sort(do.neighbours_of(est, j)), want[j]), (name, j)


def test_exact_and_f64_estimators_agree_where_the_f64_one_flags_nothing():
    rng = np.random.default_rng(12)
    v = rng.normal(size=(40000, 3))
    clouds = [(rng.uniform(0, 0.2, (20000, 3)).astype(np.float32), 0.02, 30),
              ((v / np.linalg.norm(v, axis=1, keepdims=True) * 0.3).astype(np.float32), 0.03, 50),
              (rng.uniform(0, 0.2, (20000, 3)).astype(np.float32), 0.01, 4)]
    for xyz, radius, max_nn in clouds:
        query = rng.choice(len(xyz), 2000, replace=False)
        old = do.estimate(xyz, radius=radius, max_nn=max_nn, query=query)
        new = do.estimate_exact(xyz, radius=radius, max_nn=max_nn, query=query)
        clean = ~old["tie"] & ~old["boundary"]
        assert clean.mean() > 0.95
        assert np.array_equal(new["nn"][clean], old["nn"][clean])
        for j in np.flatnonzero(clean):
            assert set(do.neighbours_of(new, j).tolist()) == set(old["neighbours"][j].tolist())
        good = clean & (old["gap"] >= 1e-2) & (old["orient"] >= 2e-3)
        assert np.all(angle(new["normals"][good], old["normals"][good]) <= 1e-9)
        assert np.all((new["normals"][good] * old["normals"][good]).sum(axis=1) > 0)
        assert np.allclose(new["gap"][good], old["gap"][good], rtol=1e-6, atol=1e-9)


def test_quantised_and_unquantised_normals_differ_by_what_the_fixed_point_predicts():
    """Offsets are rounded to 2^-20 of the cutoff distance R: an error e, |e| <= sqrt(3)/2 units, per neighbour at |x| <= R = 2^20
    units moves its term x x^T by at most 2 |x| |e| + |e|^2 and the mean's term by as much again, so the covariance by
    |dC| <= 2 sqrt(3) 2^-20 R^2 (second order aside); the eigenvector of w0 then turns by at most |dC| / (w1 - w0) (Davis-Kahan,
    to first order).  Twice that is asserted: angle <= 4 sqrt(3) 2^-20 R^2 / (w1 - w0), where the relative gap is at least 1e-2."""
    rng = np.random.default_rng(13)
    v = rng.normal(size=(40000, 3))
    sphere = (v / np.linalg.norm(v, axis=1, keepdims=True) * 0.3).astype(np.float32)
    box = rng.uniform(0, 0.2, (20000, 3)).astype(np.float32)
    worst = {}
    for xyz, radius, max_nn in ((sphere, 0.02, 30), (sphere, 0.08, 128), (box, 0.02, 30), (box, 0.01, 4), (sphere + np.float32(100), 0.02, 30)):
        est = do.estimate_exact(xyz, radius=radius, max_nn=max_nn, query=rng.choice(len(xyz), 3000, replace=False))
        ok = (est["gap"] >= 1e-2) & np.isfinite(est["gap"])
        ang = angle(est["raw_q"][ok], est["raw"][ok])
        bound = 4 * np.sqrt(3) * 2.0 ** -20 * est["cutoff"][ok].astype(np.float64) / est["split"][ok]
        assert np.all(ang <= bound), float((ang / bound).max())
        for dec in (-2, -1):
            sel = (est["gap"][ok] >= 10.0 ** dec) & ((est["gap"][ok] < 10.0 ** (dec + 1)) | (dec == -1))
            if sel.any():
                worst[dec] = max(worst.get(dec, 0.0), float(ang[sel].max()))
    print("quantised against unquantised normal, largest angle per gap decade: %s" % worst)
    assert worst[-2] < 1e-3 and worst[-1] < 1e-4   # (far inside the GPU tests' outer bar of 1e-3 rad)


def test_exact_known_answers():
    g = np.arange(6, dtype=np.float32) * np.float32(0.125)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    est = do.estimate_exact(lattice, radius=0.125, max_nn=30)
    assert np.all(est["nn"] == 1)                            # points exactly at the radius are out: d2 < r2 is strict
    up = do.estimate_exact(lattice, radius=float(np.nextafter(np.float32(0.125), np.float32(1))), max_nn=30)
    inner = np.all((lattice > 0) & (lattice < 0.6), axis=1)
    assert np.all(up["nn"][inner] == 7) and up["nn"].min() == 4
    stack = np.vstack([np.zeros((40, 3)), [[1.0, 1.0, 1.0]]]).astype(np.float32)
    est = do.estimate_exact(stack, max_nn=30)
    assert list(est["nn"]) == [40] * 40 + [1]                # every point tied at the cutoff is in
    assert np.array_equal(est["normals_q"][:40], np.tile([0, 0, -1.0], (40, 1)))
    rng = np.random.default_rng(14)
    xyz = rng.uniform(0, 0.1, (3000, 3)).astype(np.float32)
    for max_nn in (1, 2):                                    # fewer than 3 points: always the z rule
        est = do.estimate_exact(xyz, radius=0.02, max_nn=max_nn)
        assert np.all(est["nn"] == max_nn)
        for key in ("normals", "normals_q"):
            assert np.all(np.abs(est[key][:, 2]) == 1.0) and np.all(est[key][:, :2] == 0)
        assert np.all(np.isinf(est["gap"]))
    est = do.estimate_exact(xyz, radius=0.02, max_nn=3)      # and from 3 on the eigenvector
    assert np.all(est["nn"] == 3) and np.all(np.isfinite(est["gap"]))


def test_exact_oracle_at_a_wide_radius():
    """3 000 queries at radius 0.3 on a 40 k-point sphere shell, a third of the cloud in reach of each (10^8 candidate pairs):
    the per-query loop of estimate() takes a minute on this."""
    v = np.random.default_rng(15).normal(size=(40000, 3))
    xyz = (v / np.linalg.norm(v, axis=1, keepdims=True) * 0.3).astype(np.float32)
    query = np.arange(0, 40000, 13)[:3000]
    est = do.estimate_exact(xyz, radius=0.3, max_nn=128, query=query)
    assert np.all(est["nn"] == 128)
    j = 1234
    d2 = do.flann_d2(xyz[query[j]], xyz)
    assert np.array_equal(np.sort(do.neighbours_of(est, j)), np.flatnonzero(d2 <= np.sort(d2)[127]))
