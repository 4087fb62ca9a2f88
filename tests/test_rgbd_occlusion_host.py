"""The occlusion test's arithmetic (csrc/rgbd_lens.hpp: rgbd_depth_key, rgbd_colour_pixel_depth, rgbd_occluded, rgbd_splat_box)
compiled for the host as a stand-alone program (tests/abi/rgbd_occlusion_host.cpp, its own main) with -ffp-contract=off
-fsanitize=address,undefined, and held to the numpy model (tests/rgbd_occlusion_model.py) as RAW BITS: the key is monotone, Pz and the
pixel decision equal the model on the lens test's coefficient sets, the predicate turns exactly at Zmin == Pz - margin, and a host loop
over a small sensor pair gives the model's z-buffer word for word -- written square by square as the rule states it, and read square by
square as the kernels do it.  The kernels include the same header.  CPU only; the host C++
compiler is required."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import rgbd_lens_model as lm
import rgbd_model as rm
import rgbd_occlusion_model as om
from test_rgbd_lens_host import IDENTITY12, SETS, colour_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DBL_MAX = float(np.finfo(np.float64).max)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler: rgbd_lens.hpp cannot be checked"
    d = tmp_path_factory.mktemp("rgbd_occlusion")
    exe = str(d / "rgbd_occlusion_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "cwipc_util_amd", "csrc"), os.path.join(ROOT, "tests", "abi", "rgbd_occlusion_host.cpp"), "-o", exe], check=True)

    def run(mode, records, dtype=np.float64):
        inp, out = str(d / "in.bin"), str(d / "out.bin")
        np.ascontiguousarray(records, dtype=np.float64).tofile(inp)
        subprocess.run([exe, mode, inp, out], check=True, timeout=300)
        return np.fromfile(out, dtype=dtype)

    return run


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def up(value):
    return float(np.nextafter(value, np.inf))


def down(value):
    return float(np.nextafter(value, -np.inf))


def test_key_is_monotone(host):
    """A sorted list of positive doubles -- the smallest denormal and its neighbour, the largest denormal, the smallest normal, values
    one ulp apart round 1 and round a depth in metres, powers of two, DBL_MAX and the one below it -- has strictly rising keys, every
    key is below the empty word, and the key is the double's bit pattern."""
    tiny = float(np.finfo(np.float64).tiny)
    values = [5e-324, 1e-323, down(tiny), tiny, up(tiny), 1e-300, 1e-9, down(0.5), 0.5, up(0.5), down(1.0), 1.0, up(1.0), up(up(1.0)), down(1.25), 1.25,
              up(1.25), 2.0, up(2.0), 3.999, 4.0, 65.535, 1e300, down(DBL_MAX), DBL_MAX]
    rng = np.random.default_rng(3)
    values = np.unique(np.concatenate([values, rng.uniform(0.2, 8.0, 2000), np.exp(rng.uniform(-700, 700, 2000))]))
    assert (np.diff(values) > 0).all() and values[0] == 5e-324 and values[-1] == DBL_MAX
    keys = host("key", values, np.uint64)
    assert np.array_equal(keys, bits(values))
    assert (keys[1:] > keys[:-1]).all()
    assert (keys < np.uint64(0xffffffffffffffff)).all()
    assert keys[1] - keys[0] == 1 and keys[-1] - keys[-2] == 1          # one ulp apart: neighbouring keys


def depth_model(case):
    m = np.identity(4)
    m[:3] = np.reshape(case[12:24], (3, 4))
    xc, yc, z = (np.array([case[i]], dtype=np.float64) for i in (26, 27, 28))
    ok, uc, vc = lm.colour_pixel(case[0:4], case[4:12], m, case[24:26], xc, yc, z)
    with np.errstate(all='ignore'):
        pz = ((m[2, 0] * xc + m[2, 1] * yc) + m[2, 2] * z) + m[2, 3]
    return [float(ok[0]), float(uc[0]), float(vc[0]), float(pz[0])]


def test_depth_and_pixel_equal_the_model(host):
    """rgbd_colour_pixel_depth's Pz, as raw bits, and its pixel decision against the model on the lens test's coefficient sets with
    rigid and mirrored matrices; rgbd_colour_pixel (the existing function, which now calls it) decides what it decides.  Edge cases:
    Pz = 0, Pz < 0, an infinite Pz, a NaN ray: none, and Pz is what the third row gave."""
    unit = (1.0, 1.0, 0.0, 0.0)
    edge = [(2.5, 1.5, 1.0), (0.0, 0.0, 0.0), (1.0, 1.0, -1.0), (1.0, 1.0, float('inf')), (float('nan'), float('nan'), 1.0), (7.5, 0.0, 1.0)]
    cases = [colour_case(unit, lm.PINHOLE, IDENTITY12, (8.0, 6.0), *e) for e in edge]
    rng = np.random.default_rng(29)
    for n in range(4000):
        k, w, h, f, cx, cy = list(SETS.values())[n % len(SETS)]
        m = rm.random_rigid(rng, 0.05) if n % 3 else np.identity(4)
        if n % 7 == 0:
            m[:3, :3] = -m[:3, :3]
        z = rng.uniform(0.3, 4.0)
        cases.append(colour_case((f, f * rng.uniform(0.9, 1.1), cx, cy), k, m[:3].reshape(12), (w, h), rng.uniform(-1.3, 1.3) * z, rng.uniform(-0.8, 0.8) * z, z))
    got = host("depth", cases).reshape(-1, 7)
    want = np.array([depth_model(c) for c in cases])
    assert got[:len(edge), 0].tolist() == [1, 0, 0, 0, 0, 0]
    assert np.array_equal(got[:, :3], want[:, :3])
    assert np.array_equal(bits(got[:, 3]), bits(want[:, 3]))
    assert np.array_equal(got[:, 4:7], got[:, :3])                       # the existing function: the same decision and pixel
    assert 0.2 < got[len(edge):, 0].mean() < 0.9
    assert (got[got[:, 0] == 1, 3] > 0).all()


def test_predicate_turns_at_zmin_equal_to_pz_minus_margin(host):
    """Zmin == Pz - margin: kept.  One ulp below: dropped.  One ulp above, Zmin == Pz, margin 0 with equal depths: kept.  An empty
    z-buffer word (a NaN as a double) never occludes."""
    records, want = [], []
    rng = np.random.default_rng(31)
    for pz, margin in [(2.0, 0.02), (1.25, 0.0), (3.999, 0.5), (0.3, 0.25), (65.535, 1e-9)] + [(rng.uniform(0.3, 6.0), rng.uniform(0.0, 0.2)) for _ in range(200)]:
        edge = float(np.float64(pz) - np.float64(margin))
        assert edge > 0
        records += [(edge, pz, margin), (down(edge), pz, margin), (up(edge), pz, margin), (pz, pz, margin)]
        want += [0, 1, 0, 0]
    records += [(1.0, 1.0, 0.0), (down(1.0), 1.0, 0.0), (float('nan'), 2.0, 0.0), (5e-324, 1e-323, 0.0), (5e-324, 5e-324, 0.0), (DBL_MAX, DBL_MAX, 0.0),
                (down(DBL_MAX), DBL_MAX, 0.0)]
    want += [0, 1, 0, 1, 0, 0, 1]
    got = host("occluded", records, np.int32)
    assert got.tolist() == want
    # the model's predicate says the same
    r = np.array(records)
    with np.errstate(all='ignore'):
        assert ((r[:, 0] < r[:, 1] - r[:, 2]).astype(int)).tolist() == want


@pytest.mark.parametrize("splat", [0, 1, 2, 8])
@pytest.mark.parametrize("lens", ["pinhole", "mild Brown"])
def test_host_loop_gives_the_models_zbuffer(host, splat, lens):
    """A 9 x 7 depth image and an 18 x 14 colour image, the colour sensor to the side and turned a little: some candidates land outside,
    squares are clipped at every border, cells get several writers.  The program's loop (minimum of keys) against the model's
    (np.minimum.at of doubles), word for word; +inf in the model is the empty word."""
    rng = np.random.default_rng(41 + splat)
    w, h, wc, hc = 9, 7, 18, 14
    fx, fy, cx, cy = 8.0, 7.5, 4.2, 3.1
    intr = (16.5, 15.0, 8.7, 6.4)
    k = SETS[lens][0]
    a, b = 0.12, -0.07                                         # turned about y, then about x, and 50 mm to the side
    d2c = np.identity(4)
    d2c[:3, :3] = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]]) @ np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    d2c[:3, 3] = (0.05, 0.004, -0.002)
    depth = rng.integers(400, 3000, (h, w)).astype(np.uint16)
    depth[2:5, 3:6] = 350                                      # a near patch in front of the rest
    depth[0, 0] = depth[6, 8] = 0
    s = lm.Sensor(w, h, fx, fy, cx, cy, lm.PINHOLE, 0.001, (wc, hc), 3, intr, k, d2c, np.identity(4), 1)
    _xc, _yc, _z, cand, uc, vc, pz = om.projection(s, depth)
    assert 20 < cand.sum() < w * h - 2                         # (some land outside the colour image)
    zmin = om.zbuffer((wc, hc), cand, uc, vc, pz, splat)
    want = np.where(np.isinf(zmin), np.uint64(0xffffffffffffffff), bits(zmin))
    record = np.concatenate([[fx, fy, cx, cy, 0.001, w, h], intr, k, d2c[:3].reshape(12), [wc, hc, splat], depth.reshape(-1).astype(np.float64)])
    got = host("zbuffer", record, np.uint64).reshape(hc, wc)
    assert np.array_equal(got, want)
    # what the kernels do instead -- every key to its own cell, the minimum read over the square -- finds the same word for every candidate
    gathered = host("zgather", record, np.uint64).reshape(h, w)
    assert np.array_equal(gathered, np.where(cand, want[vc, uc], np.uint64(0xffffffffffffffff)))
    if splat == 0:
        assert np.isinf(zmin).any()
    # a pixel is always in its own square
    assert (zmin[vc[cand], uc[cand]] <= pz[cand]).all()
