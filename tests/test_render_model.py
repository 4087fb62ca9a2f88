"""The numpy model of cwipc_hip_render (tests/render_model.py) against a plain loop, and the host arithmetic of
registration/render.py: look_at and deproject.  No GPU."""
import math

import numpy as np
import pytest

import render_model as rm
from cwipc_util_amd.registration.render import PinholeView, default_view, look_at, deproject
from cwipc_util_amd.util import cwipc_point_numpy_dtype


def _cloud(rng, n, view, special=True):
    """n points around the view's frustum in cloud coordinates: inside and outside the image, in front of and behind the camera,
    half of them on a coarse lattice (equal depths and equal pixels), a few not finite."""
    cam = np.empty((n, 3))
    cam[:, 2] = rng.uniform(-0.5, 4.0, n)
    cam[:, 0] = rng.uniform(-1.5, 1.5, n) * np.abs(cam[:, 2]) * (view.width / view.fx)
    cam[:, 1] = rng.uniform(-1.5, 1.5, n) * np.abs(cam[:, 2]) * (view.height / view.fy)
    lattice = rng.random(n) < 0.5
    cam[lattice] = np.round(cam[lattice] * 4) / 4
    inv = np.linalg.inv(np.asarray(view.extrinsic, dtype=np.float64))
    world = cam @ inv[:3, :3].T + inv[:3, 3]
    pts = np.zeros(n, dtype=cwipc_point_numpy_dtype)
    pts['x'], pts['y'], pts['z'] = world[:, 0], world[:, 1], world[:, 2]
    pts['r'], pts['g'], pts['b'] = rng.integers(0, 256, (3, n))
    pts['tile'] = rng.choice([1, 2, 3, 4], n)
    if special and n >= 8:
        for k, (f, v) in enumerate((('x', np.nan), ('y', np.inf), ('z', -np.inf), ('x', 1e30), ('z', 1e30))):
            pts[f][k] = v
    return pts


def _views():
    yield "identity 9x7", PinholeView(9, 7, 6.0, 6.0, 4.0, 3.0)
    yield "identity 1x1", PinholeView(1, 1, 1.0, 1.0, 0.0, 0.0)
    yield "look_at 8x5", PinholeView(8, 5, 5.5, 4.5, 3.5, 2.0, look_at((0.3, 1.0, -3.0), (0.0, 1.0, 0.0), (0, 1, 0)), near=0.5, far=3.5)
    yield "look_at tilted 5x7", PinholeView(5, 7, 4.0, 4.0, 2.25, 3.5, look_at((1.0, 2.0, -2.0), (0.0, 0.0, 0.5), (0.1, 1, 0)))


@pytest.mark.parametrize("point_size", [1, 3, 5, 15])
def test_model_equals_the_loops(point_size):
    rng = np.random.default_rng(100 + point_size)
    for name, view in _views():
        for n in (0, 1, 7, 300):
            pts = _cloud(rng, n, view)
            for tilemask in (0, 2, 6, 128):
                got = rm.render_model(pts, view, point_size, tilemask, (10, 20, 30))
                want = rm.render_loops(pts, view, point_size, tilemask, (10, 20, 30))
                for g, w, what in zip(got, want, ("rgb", "depth", "index", "covered")):
                    assert np.array_equal(np.asarray(g), np.asarray(w)), (name, n, tilemask, what)
                assert got[1].tobytes() == want[1].tobytes(), (name, n, tilemask)
            if n == 300 and name != "identity 1x1":
                assert 0 < got[3] or tilemask == 128


def test_model_ties_and_uncovered_pixels():
    view = PinholeView(4, 3, 2.0, 2.0, 1.5, 1.0)
    pts = np.zeros(3, dtype=cwipc_point_numpy_dtype)
    pts['z'] = [2.0, 1.0, 1.0]          # all three in pixel (1, 1); the two nearest tie, the lower index wins
    pts['r'] = [1, 2, 3]
    rgb, depth, index, covered = rm.render_model(pts, view, 1)
    assert covered == 1 and index[1, 1] == 1 and depth[1, 1] == 1.0 and rgb[1, 1].tolist() == [2, 0, 0]
    assert (index.reshape(-1)[np.arange(12) != 5] == -1).all() and (depth.reshape(-1)[np.arange(12) != 5] == 0).all()
    assert (rgb.reshape(-1, 3)[0] == 255).all()


def _views_for_deproject():
    yield default_view(64, 48)
    v = default_view(64, 48, 70.0, look_at((0.5, 1.5, -2.0), (0.0, 0.2, 0.3), (0, 1, 0)))
    yield v


def test_deproject_lands_in_the_pixel_it_came_from():
    """deproject truncates (u, v) to a pixel and uses that pixel's depth: projecting its result with the contract's arithmetic must
    give that pixel again (u comes out as the integer up to rounding, hence the +-1e-9 before the floor is compared)."""
    rng = np.random.default_rng(5)
    for view in _views_for_deproject():
        depth = rng.uniform(0.5, 3.0, (view.height, view.width)).astype(np.float32)
        depth[10, 10] = 0
        E = np.asarray(view.extrinsic)
        for _ in range(200):
            uv = (rng.uniform(0, view.width), rng.uniform(0, view.height))
            p = deproject(view, depth, uv)
            if (int(uv[0]), int(uv[1])) == (10, 10):
                assert p is None
                continue
            cam = E[:3, :3] @ np.array(p) + E[:3, 3]
            assert cam[2] == pytest.approx(float(depth[int(uv[1]), int(uv[0])]), rel=1e-12)
            u = view.fx * (cam[0] / cam[2]) + view.cx
            v = view.fy * (cam[1] / cam[2]) + view.cy
            assert math.floor(u + 1e-9) == int(uv[0]) and abs(u - int(uv[0])) < 1e-9
            assert math.floor(v + 1e-9) == int(uv[1]) and abs(v - int(uv[1])) < 1e-9
        for uv in ((-1, 3), (3, -1), (view.width, 3), (3, view.height), (10.9, 10.2)):
            assert deproject(view, depth, uv) is None


@pytest.mark.parametrize("eye, target, up", [((0, 1, -3), (0, 1, 0), (0, 1, 0)), ((1.2, 1.4, 0.3), (0, 0, 0), (0, 1, 0)),
                                             ((-2, 0.5, 2), (0.3, 0, -0.4), (0.2, 1, 0.1)), ((0, 3, 0), (0, 0, 0), (0, 0, 1))])
def test_look_at(eye, target, up):
    m = look_at(eye, target, up)
    rot = m[:3, :3]
    assert np.allclose(rot @ rot.T, np.identity(3), atol=1e-14) and np.linalg.det(rot) == pytest.approx(1.0, abs=1e-14)
    assert m[3].tolist() == [0, 0, 0, 1]
    assert np.allclose(m @ np.array([*eye, 1.0]), [0, 0, 0, 1], atol=1e-14)
    t = m @ np.array([*target, 1.0])
    dist = np.linalg.norm(np.array(target, dtype=float) - np.array(eye, dtype=float))
    assert np.allclose(t[:3], [0, 0, dist], atol=1e-13)
    # up is towards the top of the image: its image-y component is negative
    assert (rot @ np.array(up, dtype=float))[1] < 0


def test_default_view():
    v = default_view()
    assert (v.width, v.height, v.cx, v.cy) == (1920, 1080, 959.5, 539.5) and v.fx == v.fy == pytest.approx(540 / math.tan(math.radians(30)))
    assert v.near == 0.01 and v.far == math.inf and np.array_equal(v.extrinsic, np.identity(4))
    s = v.as_struct()
    assert (s.width, s.height, s.fx, s.cy, s.far) == (1920, 1080, v.fx, 539.5, math.inf) and list(s.extrinsic) == np.identity(4).reshape(-1).tolist()
