"""The RGB-D source's per-pixel arithmetic (csrc/rgbd_terms.hpp) compiled for the host as a stand-alone program
(tests/abi/rgbd_terms_host.cpp, its own main) with -ffp-contract=off -fsanitize=address,undefined, and held to the numpy model
(tests/rgbd_model.py) as RAW BITS: the points, the keep / drop decisions at every filter's boundary, and the green screen over all
2^24 colours.  The kernels include the same header.  CPU only; the host C++ compiler is required (a missing one fails the tests)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import rgbd_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENTITY = np.identity(4)
OFF = rm.Filter()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler: rgbd_terms.hpp cannot be checked"
    d = tmp_path_factory.mktemp("rgbd_terms")
    exe = str(d / "rgbd_terms_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "cwipc_util_amd", "csrc"), os.path.join(ROOT, "tests", "abi", "rgbd_terms_host.cpp"), "-o", exe], check=True)

    def pixels(records):
        records = np.ascontiguousarray(records, dtype=np.float64).reshape(-1, 29)
        inp, out = str(d / "in.bin"), str(d / "out.bin")
        records.tofile(inp)
        subprocess.run([exe, "pixel", inp, out], check=True, timeout=120)
        got = np.fromfile(out, dtype=np.uint32).reshape(-1, 4)
        assert len(got) == len(records)
        return got

    def green():
        out = str(d / "green.bin")
        subprocess.run([exe, "green", out], check=True, timeout=300)
        return np.unpackbits(np.fromfile(out, dtype=np.uint8), bitorder='little').astype(bool)

    pixels.green = green
    return pixels


def record(cam, flt, u, v, d, rgb=(200, 30, 40)):
    m = np.asarray(cam.trafo, dtype=np.float64)
    return [cam.fx, cam.fy, cam.cx, cam.cy, cam.depth_scale, *m[:3].reshape(12), flt.threshold_near, flt.threshold_far, flt.height_min, flt.height_max,
            float(np.float32(flt.radius)), 1.0 if flt.greenscreen else 0.0, u, v, d, *rgb]


def model(cam, flt, u, v, d, rgb=(200, 30, 40)):
    """(kept, x, y, z as float32 bits) of one pixel, from the numpy model"""
    a = lambda value: np.array([value])   # noqa: E731
    keep, x, y, z = rm.keep_mask(cam, flt, a(u), a(v), a(d), a(rgb[0]), a(rgb[1]), a(rgb[2]))
    xyz = np.float32([x[0], y[0], z[0]]).view(np.uint32) if d != 0 else np.zeros(3, dtype=np.uint32)
    return [int(keep[0]), *xyz]


def check(host, cases):
    got = host([record(*c) for c in cases])
    want = np.array([model(*c) for c in cases], dtype=np.uint32)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert len(bad) == 0, [(int(k), got[k].tolist(), want[k].tolist()) for k in bad[:5]]
    return got


def test_points_and_decisions_bit_for_bit(host):
    """u and v at 0 and at the last pixel, d at 1 and at 65535, both depth scales, random rigid matrices, every filter on and off."""
    rng = np.random.default_rng(17)
    width, height = 67, 45
    cases = []
    for k in range(3000):
        scale = (0.001, 1.0 / 1024)[k & 1]
        cam = rm.Camera(rng.uniform(30, 700), rng.uniform(30, 700), rng.uniform(0, width), rng.uniform(0, height), scale,
                        rm.random_rigid(rng) if k % 5 else IDENTITY)
        u = int(rng.choice([0, width - 1, rng.integers(0, width)]))
        v = int(rng.choice([0, height - 1, rng.integers(0, height)]))
        d = int(rng.choice([0, 1, 65535, rng.integers(1, 65536), rng.integers(300, 4000)], p=[0.05, 0.15, 0.15, 0.25, 0.4]))
        on = rng.integers(0, 16)
        flt = rm.Filter(*(rng.uniform(0.2, 2.0), rng.uniform(2.0, 40.0)) if on & 1 else (1.0, 1.0),
                        *(rng.uniform(-3, 0), rng.uniform(0, 3)) if on & 2 else (0.5, 0.5),
                        float(np.float32(rng.uniform(0.5, 4.0))) if on & 4 else (0.0, -1.0)[k & 1], bool(on & 8))
        rgb = tuple(int(c) for c in rng.integers(0, 256, 3))
        cases.append((cam, flt, u, v, d, rgb))
    got = check(host, cases)
    assert 0.2 < got[:, 0].mean() < 0.8   # (both decisions occur in numbers)


def test_depth_range_boundary(host):
    """z == threshold_near and z == threshold_far are kept; one ulp beyond either is dropped; far <= near is "off"."""
    cam = rm.Camera(500.0, 500.0, 3.0, 2.0, 1.0 / 1024, IDENTITY)   # depth 512: z = 0.5 exactly
    up, down = float(np.nextafter(0.5, 1.0)), float(np.nextafter(0.5, 0.0))
    cases = [(cam, rm.Filter(0.5, 1.0), 5, 4, 512), (cam, rm.Filter(0.25, 0.5), 5, 4, 512), (cam, rm.Filter(0.5, up), 5, 4, 512),
             (cam, rm.Filter(up, 1.0), 5, 4, 512), (cam, rm.Filter(0.25, down), 5, 4, 512), (cam, rm.Filter(2.0, 2.0), 5, 4, 512),
             (cam, rm.Filter(2.0, 1.0), 5, 4, 512)]
    assert check(host, cases)[:, 0].tolist() == [1, 1, 1, 0, 0, 1, 1]


def test_height_boundary(host):
    """y == height_min is kept (and y == height_max); one float64 step inside the range's complement is dropped; min == max is "off"."""
    cam = rm.Camera(500.0, 1.0, 3.0, 2.0, 1.0 / 1024, IDENTITY)   # u = 3, v = 3, depth 512: x = 0, y = 0.5, z = 0.5 exactly
    up, down = float(np.nextafter(0.5, 1.0)), float(np.nextafter(0.5, 0.0))
    cases = [(cam, rm.Filter(height_min=0.5, height_max=1.0), 3, 3, 512), (cam, rm.Filter(height_min=0.0, height_max=0.5), 3, 3, 512),
             (cam, rm.Filter(height_min=up, height_max=1.0), 3, 3, 512), (cam, rm.Filter(height_min=0.0, height_max=down), 3, 3, 512),
             (cam, rm.Filter(height_min=0.7, height_max=0.7), 3, 3, 512)]
    got = check(host, cases)
    assert got[0, 1:].view(np.float32).tolist() == [0.0, 0.5, 0.5]
    assert got[:, 0].tolist() == [1, 1, 0, 0, 1]


def test_radius_boundary(host):
    """depth_scale 1/1024, the identity matrix and cx = u: depth 512 gives d2 == 0.25 exactly, which is not < 0.5 * 0.5 -- dropped at
    radius 0.5 -- and depth 511 is kept.  radius <= 0 is "off"."""
    cam = rm.Camera(500.0, 500.0, 7.0, 2.0, 1.0 / 1024, IDENTITY)
    cases = [(cam, rm.Filter(radius=0.5), 7, 2, 512), (cam, rm.Filter(radius=0.5), 7, 2, 511), (cam, rm.Filter(radius=0.0), 7, 2, 512),
             (cam, rm.Filter(radius=-1.0), 7, 2, 512), (cam, rm.Filter(radius=float(np.nextafter(np.float32(0.5), np.float32(1)))), 7, 2, 512)]
    got = check(host, cases)
    x, z = got[0, 1:].view(np.float32)[[0, 2]]
    assert (x, z) == (0.0, 0.5) and np.float32(np.float64(x) * np.float64(x) + np.float64(z) * np.float64(z)) == np.float32(0.25)
    assert got[:, 0].tolist() == [0, 1, 1, 1, 1]


def test_green_pixel_cases(host):
    """Colour (51, 86, 0) has hue 60 by truncation (85 + trunc(-25.5) = 60) and 59 by floor: it must come out dropped."""
    assert int(rm.hue(51, 86, 0)[0]) == 60 and int(rm.hue(51, 86, 0, floor=True)[0]) == 59
    cam = rm.Camera(500.0, 500.0, 3.0, 2.0, 0.001, IDENTITY)
    on = rm.Filter(greenscreen=True)
    cases = [(cam, on, 1, 1, 900, (51, 86, 0)), (cam, OFF, 1, 1, 900, (51, 86, 0)), (cam, on, 1, 1, 900, (200, 30, 40)), (cam, on, 1, 1, 900, (0, 0, 0)),
             (cam, on, 1, 1, 900, (0, 255, 0)), (cam, on, 1, 1, 900, (255, 255, 255)), (cam, on, 1, 1, 0, (200, 30, 40))]
    assert check(host, cases)[:, 0].tolist() == [0, 1, 1, 1, 0, 1, 0]


def test_green_screen_over_all_colours(host):
    """All 2^24 colours: the program's bitmask equals the model's full restatement of rgbToHsv + isNotGreen (its s and v conditions and
    its colour edits included) and equals the bare hue-window test -- inside the window the reference's other conditions always hold."""
    got = host.green()
    assert got.shape == (1 << 24,)
    edited = 0
    for chunk in range(16):
        c = np.arange(chunk << 20, (chunk + 1) << 20, dtype=np.int64)
        r, g, b = c & 255, (c >> 8) & 255, (c >> 16) & 255
        full, new_r, new_b = rm.is_not_green_full(r, g, b)
        window = rm.in_hue_window(r, g, b)
        part = got[chunk << 20: (chunk + 1) << 20]
        assert np.array_equal(part, full), chunk
        assert np.array_equal(part, ~window), chunk
        # the edits happen, and only to colours that are dropped: they reach no output
        changed = (new_r != r) | (new_b != b)
        assert not (changed & full).any()
        edited += int(changed.sum())
    assert edited > 100000
    assert 0.1 < 1.0 - got.mean() < 0.4   # (the window is 71 of 256 hues wide)
    assert not got[51 | (86 << 8)]
