"""The arithmetic of the RGB-D source's raw entry (csrc/rgbd_lens.hpp) compiled for the host as a stand-alone program
(tests/abi/rgbd_lens_host.cpp, its own main) with -ffp-contract=off -fsanitize=address,undefined, and held to the numpy model
(tests/rgbd_lens_model.py) as RAW BITS: distort, whole ray tables, the colour pixel decisions at their edges, the erosion words.  Then
two checks that do not go through the model: every table entry distorts back onto its pixel, and the erosion model's separable
statement equals the definition.  The kernels include the same header.  CPU only; the host C++ compiler is required."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import rgbd_lens_model as lm
import rgbd_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

#: name -> (k1 k2 p1 p2 k3 k4 k5 k6, width, height, fx = fy, cx, cy)
SETS = {
    "pinhole": (lm.PINHOLE, 67, 45, 52.5, 33.25, 22.0),
    "mild Brown": ((-0.1, 0.05, 1e-3, -5e-4, 0.0, 0.0, 0.0, 0.0), 1280, 720, 600.0, 640.0, 360.0),
    "strong barrel": ((-0.28, 0.07, 1e-3, -5e-4, 0.0, 0.0, 0.0, 0.0), 1280, 720, 600.0, 640.0, 360.0),
    "rational colour lens": ((0.4569, -2.7217, 4.7e-4, -1.6e-4, 1.5964, 0.3335, -2.5460, 1.5223), 1280, 720, 607.0, 638.0, 367.0),
    "rational depth lens": ((4.9, 3.1, 1e-4, -5e-5, 0.16, 5.2, 4.8, 0.85), 640, 576, 504.0, 320.0, 330.0),
}
FOLDED = ((-1.5, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0), 1280, 720, 600.0, 640.0, 360.0)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler: rgbd_lens.hpp cannot be checked"
    d = tmp_path_factory.mktemp("rgbd_lens")
    exe = str(d / "rgbd_lens_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "cwipc_util_amd", "csrc"), os.path.join(ROOT, "tests", "abi", "rgbd_lens_host.cpp"), "-o", exe], check=True)

    def run(mode, records, dtype=np.float64):
        inp, out = str(d / "in.bin"), str(d / "out.bin")
        np.ascontiguousarray(records, dtype=np.float64).tofile(inp)
        subprocess.run([exe, mode, inp, out], check=True, timeout=300)
        return np.fromfile(out, dtype=dtype)

    return run


@pytest.fixture(scope="module")
def tables(host):
    """name -> the program's ray table, float64[H, W, 2] (computed once)"""
    out = {}
    for name, (k, w, h, f, cx, cy) in list(SETS.items()) + [("folded", FOLDED)]:
        out[name] = host("table", [*k, f, f, cx, cy, w, h]).reshape(h, w, 2)
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_distort_bit_for_bit(host):
    """Every set, points over and beyond the image's normalised extent, the axes and the origin included."""
    rng = np.random.default_rng(5)
    for name, (k, *_rest) in SETS.items():
        x = np.concatenate([rng.uniform(-2.0, 2.0, 4000), [0.0, 0.0, 1.0, -1.0, 1e-300, 2.0]])
        y = np.concatenate([rng.uniform(-2.0, 2.0, 4000), [0.0, 1.0, 0.0, -1.0, -1e-300, -2.0]])
        got = host("distort", np.column_stack([np.tile(k, (len(x), 1)), x, y])).reshape(-1, 2)
        wx, wy = lm.distort(k, x, y)
        assert np.array_equal(bits(got[:, 0]), bits(wx)) and np.array_equal(bits(got[:, 1]), bits(wy)), name
    # all coefficients zero: distort is the identity, bit for bit
    x = rng.uniform(-3, 3, 1000)
    got = host("distort", np.column_stack([np.zeros((1000, 8)), x, x[::-1]])).reshape(-1, 2)
    assert np.array_equal(bits(got[:, 0]), bits(x)) and np.array_equal(bits(got[:, 1]), bits(x[::-1]))


@pytest.mark.parametrize("name", list(SETS))
def test_table_entries_bit_for_bit(tables, name):
    k, w, h, f, cx, cy = SETS[name]
    want = lm.ray_table(w, h, f, f, cx, cy, k)
    assert np.array_equal(bits(tables[name]), bits(want))


def opencv_distort(k, x, y):
    """OpenCV's rational model as its documentation writes it (not the model's statement: no fixed order)."""
    k1, k2, p1, p2, k3, k4, k5, k6 = k
    r2 = x * x + y * y
    rad = (1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3) / (1 + k4 * r2 + k5 * r2 ** 2 + k6 * r2 ** 3)
    return x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x), y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y


def numeric_det(k, x, y, h=1e-6):
    """The Jacobian's determinant by central differences of opencv_distort."""
    ax1, ay1 = opencv_distort(k, x + h, y)
    ax0, ay0 = opencv_distort(k, x - h, y)
    bx1, by1 = opencv_distort(k, x, y + h)
    bx0, by0 = opencv_distort(k, x, y - h)
    return ((ax1 - ax0) * (by1 - by0) - (bx1 - bx0) * (ay1 - ay0)) / (4 * h * h)


@pytest.mark.parametrize("name", list(SETS))
def test_round_trip_every_pixel_has_a_ray(tables, name):
    """Independent of the model: no NaN entry, and distort(ray) is the pixel within 1e-12 * sqrt(fx^2 + fy^2) pixels -- the acceptance
    threshold taken to pixels."""
    k, w, h, f, cx, cy = SETS[name]
    table = tables[name]
    assert not np.isnan(table).any()
    xd, yd = opencv_distort(k, table[..., 0], table[..., 1])
    v, u = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    err = np.hypot(f * xd + cx - u, f * yd + cy - v)
    bound = 1e-12 * np.hypot(f, f)
    print("%s: worst round trip %.3g px, bound %.3g px" % (name, err.max(), bound))
    assert err.max() <= bound
    assert (numeric_det(k, table[..., 0], table[..., 1]) > 0).all()


def test_folded_lens_has_pixels_without_a_ray(tables):
    """k1 = -1.5: r (1 - 1.5 r^2) turns back at r^2 = 1/4.5, where the image folds over and the determinant changes sign.  The table
    must have NaN entries, every entry it does have must sit where the determinant is positive (never on the folded-over sheet
    between r^2 = 1/4.5 and r^2 = 1/1.5) and must distort back onto its pixel; the pixels round the centre all have rays."""
    k, w, h, f, cx, cy = FOLDED
    table = tables["folded"]
    v, u = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    rd = np.hypot((u - cx) / f, (v - cy) / f)
    nan = np.isnan(table[..., 0])
    assert np.array_equal(nan, np.isnan(table[..., 1]))
    assert nan.any() and not nan.all()
    x, y = table[..., 0][~nan], table[..., 1][~nan]
    assert (numeric_det(k, x, y, 1e-7) > 0).all() and (lm.jacobian_det(k, x, y) > 0).all()
    r2 = x * x + y * y
    assert not ((r2 > 1 / 4.5) & (r2 < 1 / 1.5)).any()
    assert not nan[rd < 0.1].any()
    xd, yd = opencv_distort(k, x, y)
    assert np.hypot(f * xd + cx - u[~nan], f * yd + cy - v[~nan]).max() <= 1e-12 * np.hypot(f, f)


IDENTITY12 = [1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0]


def colour_case(intr, k, m12, size, xc, yc, z):
    return [*intr, *k, *m12, *size, xc, yc, z]


def colour_model(case):
    m = np.identity(4)
    m[:3] = np.reshape(case[12:24], (3, 4))
    a = lambda value: np.array([value], dtype=np.float64)   # noqa: E731
    ok, uc, vc = lm.colour_pixel(case[0:4], case[4:12], m, case[24:26], a(case[26]), a(case[27]), a(case[28]))
    return [int(ok[0]), int(uc[0]), int(vc[0])]


def test_colour_pixel_decisions(host):
    """Unit focal length, no offset, no lens, the identity, z = 1: the projection is xc itself.  x.5 goes up; -0.5 is pixel 0; the step
    below it is outside; Wc - 0.5 is outside, the step below it is the last pixel; Pz = 0, Pz < 0, an infinite Pz and a NaN ray give
    none.  Then random cases with lenses and rigid matrices, all against the model."""
    unit = (1.0, 1.0, 0.0, 0.0)
    size = (8.0, 6.0)
    down = lambda value: float(np.nextafter(value, -np.inf))   # noqa: E731
    edge = [(2.5, 1.5, 1.0), (-0.5, -0.5, 1.0), (down(-0.5), 0.0, 1.0), (0.0, down(-0.5), 1.0), (7.5, 0.0, 1.0), (down(7.5), down(5.5), 1.0),
            (0.0, 5.5, 1.0), (0.0, 0.0, 0.0), (1.0, 1.0, -1.0), (1.0, 1.0, float('inf')), (float('nan'), float('nan'), 1.0),
            (float('nan'), 1.0, 1.0), (1.0, float('inf'), 1.0), (1e300, 0.0, 1e-300)]
    cases = [colour_case(unit, lm.PINHOLE, IDENTITY12, size, *e) for e in edge]
    want_edge = [[1, 3, 2], [1, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0], [1, 7, 5], [0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0],
                 [0, 0, 0], [0, 0, 0]]
    rng = np.random.default_rng(23)
    for n in range(4000):
        k, w, h, f, cx, cy = list(SETS.values())[n % len(SETS)]
        m = rm.random_rigid(rng, 0.05) if n % 3 else np.identity(4)
        if n % 7 == 0:
            m[:3, :3] = -m[:3, :3]                          # most points behind the colour camera
        z = rng.uniform(0.3, 4.0)
        cases.append(colour_case((f, f * rng.uniform(0.9, 1.1), cx, cy), k, m[:3].reshape(12), (w, h), rng.uniform(-1.3, 1.3) * z, rng.uniform(-0.8, 0.8) * z,
                                 z))
    got = host("colour", cases, np.int32).reshape(-1, 3)
    want = np.array([colour_model(c) for c in cases], dtype=np.int32)
    assert got[:len(edge)].tolist() == want_edge
    assert np.array_equal(got, want)
    assert 0.2 < got[len(edge):, 0].mean() < 0.9           # (both decisions occur in numbers)


def masks(rng, shape=(23, 37)):
    depth = rng.integers(300, 4000, shape).astype(np.uint16)
    depth[rng.random(shape) < rng.choice([0.002, 0.02, 0.2])] = 0
    return depth


@pytest.mark.parametrize("ex", [0, 1, 3, 32])
@pytest.mark.parametrize("ey", [0, 1, 3, 32])
def test_erosion_model_equals_the_definition(ex, ey):
    """The separable statement against a brute-force window scan of the definition, on random 37 x 23 masks."""
    rng = np.random.default_rng(1000 + 40 * ex + ey)
    for _ in range(4):
        depth = masks(rng)
        assert np.array_equal(lm.erode(depth, ex, ey), lm.erode_brute(depth, ex, ey))
    full = np.full((23, 37), 7, dtype=np.uint16)
    assert np.array_equal(lm.erode(full, ex, ey), full)      # pixels outside the image do not erode


def test_erosion_words_equal_the_model(host):
    """rgbd_erode_word on 64-pixel words, as the kernels use it: widths on both sides of one and two words, holes on the seams."""
    rng = np.random.default_rng(77)
    for (w, h), (ex, ey) in [((37, 23), (3, 1)), ((64, 5), (32, 0)), ((65, 4), (1, 32)), ((130, 9), (32, 32)), ((130, 9), (7, 2)), ((1, 1), (5, 5)),
                             ((200, 3), (31, 1))]:
        depth = masks(rng, (h, w))
        for u in (63, 64, 65, 127, 128, 129):
            if u < w:
                depth[rng.integers(0, h), u] = 0
        got = host("erode", np.concatenate([[w, h, ex, ey], depth.reshape(-1).astype(np.float64)])).reshape(h, w)
        assert np.array_equal(got.astype(np.uint16), lm.erode(depth, ex, ey)), (w, h, ex, ey)
